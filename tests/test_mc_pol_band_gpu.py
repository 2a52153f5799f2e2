"""GPU: the N0 Monte Carlo of the polarisation estimators and their MV combination in ONE call on map sides 2^a 3^b 5^c -- the leg-band
draw straight into the inner grid (oa_grf_mix_band_inner), the Monte-Carlo set-up entry (oa_mc_mv_band_bind), oa_mc_run_mv on the band
grid, and mc.GaussianN0MonteCarloPol(one_call=True).  The reference is the host loop of existing entries (sample_host), as on
power-of-two sides.  Geometry and estimator set-up: those of tests/test_mc_pol_gpu.py (1.5' beam, 1 uK' T noise and twice that power in P,
T and P filters 300-2000, kappa mask 20-3000, EDGES = linspace(100, 2900, 12), five estimators)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ESTS = ("TT", "TE", "EE", "EB", "TB")
EDGES = np.linspace(100, 2900, 12)
SENTINEL = complex(-7.5, 3.25)


@functools.lru_cache(maxsize=None)
def geometry(shape, res):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    nP = 2 * nT
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3000)
    cl = {k: th.lCl(k, ml) for k in ("TT", "EE", "BB", "TE")}
    nxh = shape[1] // 2
    tot = dict(TT=cl["TT"] * beam ** 2 + nT, EE=cl["EE"] * beam ** 2 + nP, BB=cl["BB"] * beam ** 2 + nP, TE=cl["TE"] * beam ** 2)
    tot_h = {k: np.ascontiguousarray(v[:, :nxh + 1]) for k, v in tot.items()}
    return dict(g=g, th=th, beam=beam, nT=nT, nP=nP, tmask=tmask, kmask=kmask, tot_h=tot_h)


@functools.lru_cache(maxsize=None)
def estimator(shape, res, prec, grid="auto"):
    from orphics_amd import lensing
    G = geometry(shape, res)
    return lensing.qest(shape, G["g"], G["th"], noise2d=G["nT"], beam2d=G["beam"], kmask=G["tmask"], noise2d_P=G["nP"], kmask_P=G["tmask"],
                        kmask_K=G["kmask"], pol=True, unlensed_equals_lensed=True, dtype=prec, row_grid=grid, col_grid=grid)


def driver(shape, res, prec, grid="auto", **kw):
    from orphics_amd import mc
    return mc.GaussianN0MonteCarloPol(estimator(shape, res, prec, grid), geometry(shape, res)["tot_h"], EDGES, **kw)


def close(got, ref, tol):
    """the project's moment comparison: rtol, plus the same factor times the largest |entry| (cross spectra scatter around zero)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    print("max |got - ref| / max |ref| = %.3e (tol %.1e)" % (np.abs(got - ref).max() / np.abs(ref).max(), tol))
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())


def host_moments(drv, sims):
    X = torch.stack([drv.sample_host(i) for i in sims]).cpu().numpy()
    return X, X.sum(0), X.T @ X


def device_moments(drv):
    n, S, C = drv.acc.device_moments("n0", drv.D)
    return int(n.item()), S.cpu().numpy().copy(), C.cpu().numpy().copy()


# ---- oa_grf_mix_band_inner ---------------------------------------------------------------------------------------------------------
MY, PITCH = 32, 32
SID = (0xC0FFEE << 32) + 12           # a stream id with its upper half set


def mix_table(e, ncomp, gen):
    cs = [[None] * ncomp for _ in range(ncomp)]
    for i in range(ncomp):
        for j in range(i + 1):               # lower triangle; the upper blocks stay NULL
            cs[i][j] = (torch.rand((e.ny, e.kp), generator=gen, device="cuda", dtype=torch.float64) + 0.25).to(e.rdt)
    if ncomp == 3:
        cs[2][0] = None                      # a NULL block inside the triangle too
    return cs


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("width,rband", [(13, 7), (16, 16), (17, 1)])
@pytest.mark.parametrize("shape", [(60, 90), (64, 128)])
def test_inner_draw_is_the_band_draw_at_the_mapped_rows(shape, width, rband, prec):
    """Inside the band the (32, 32) inner planes hold oa_grf_mix_band's N-grid values bit for bit at row y (y < rband) or y - ny + 32
    (the negative-ky rows); everything else keeps the sentinel.  (60, 90): nx/2 = 45 makes the N-grid pitch odd; rband 16 fills 31 of
    the 32 inner rows; width 17 = the inner grid's Mx/2 + 1 with a single row."""
    from orphics_amd.engine import Engine
    ny, nx = shape
    e = Engine(ny, nx, prec)
    assert (e.kp % 2 == 1) == (shape == (60, 90))
    gen = torch.Generator(device="cuda").manual_seed(11)
    rows = torch.arange(ny, device="cuda")
    inrow = (rows < rband) | (rows > ny - rband)
    ys = rows[inrow]
    yo = torch.where(ys < rband, ys, ys - ny + MY)
    assert ys.numel() == 2 * rband - 1 and int(yo.unique().numel()) == 2 * rband - 1
    band = torch.zeros((MY, PITCH), dtype=torch.bool, device="cuda")
    band[yo, :width] = True
    for ncomp, scale in ((1, 1.0), (3, 0.75)):
        cs = mix_table(e, ncomp, gen)
        ref = [torch.zeros((ny, e.kp), dtype=e.cdt, device="cuda") for _ in range(ncomp)]
        e.grf_mix_band(77, cs, ref, width=width, rband=rband, scale=scale, stream_id0=SID)
        out = [torch.full((MY, PITCH), SENTINEL, dtype=e.cdt, device="cuda") for _ in range(ncomp)]
        e.grf_mix_band_inner(77, cs, out, MY, PITCH, width, rband, scale=scale, stream_id0=SID)
        for c in range(ncomp):
            a, b = torch.view_as_real(out[c][yo, :width]), torch.view_as_real(ref[c][ys, :width])
            assert bool((b != 0).any()) and torch.equal(a, b), (ncomp, c)
            assert bool((out[c][~band] == SENTINEL).all()), (ncomp, c)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_inner_draw_refusals(prec):
    """every listed refusal returns non-zero with its message before anything is launched: the planes keep their sentinel"""
    from orphics_amd.engine import Engine
    e = Engine(60, 90, prec)
    gen = torch.Generator(device="cuda").manual_seed(3)
    cs = mix_table(e, 3, gen)
    tab = (ctypes.c_void_p * 9)(*[c.data_ptr() if c is not None else None for r in cs for c in r])
    planes = [torch.full((128, 64), SENTINEL, dtype=e.cdt, device="cuda") for _ in range(3)]
    outs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in planes])
    holed = (ctypes.c_void_p * 3)(planes[0].data_ptr(), None, planes[2].data_ptr())

    def call(ncomp=3, my=32, pitch=32, width=13, rband=7, out=outs):
        rc = e.lib.oa_grf_mix_band_inner(e.plan, 5, 0, ncomp, tab, 1.0, out, my, pitch, width, rband, None)
        return rc, (e.lib.oa_last_error() or b"").decode()
    cases = [
        (dict(ncomp=0), "1 <= ncomp <= 3"),
        (dict(ncomp=4), "1 <= ncomp <= 3"),
        (dict(rband=17), "2 rband - 1 <= min(ny, my)"),                   # 33 rows > my = 32
        (dict(my=128, pitch=64, rband=31), "2 rband - 1 <= min(ny, my)"),  # 61 rows > ny = 60
        (dict(pitch=64, width=47), "width <= nx/2 + 1"),                   # nx/2 + 1 = 46
        (dict(pitch=16, width=17), "do not fit the output row pitch"),     # 2 ceil(17 / 2) = 18 > 16
        (dict(out=holed), "NULL output plane"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err and "oa_grf_mix_band_inner" in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in planes)
    assert call()[0] == 0                                   # the accepted call, for contrast
    torch.cuda.synchronize()
    flat = planes[0].view(-1)                               # the call's (32, 32) layout lies at the front of the allocation
    assert bool((flat[:32 * 32].view(32, 32)[:7, :13] != SENTINEL).all()) and bool((flat[32 * 32:] == SENTINEL).all())
    with pytest.raises(ValueError):
        e.grf_mix_band_inner(5, cs, [t[:32, :32] for t in planes], 32, 32, 13, 7)     # not (my, pitch) contiguous planes


# ---- oa_mc_run_mv on the band grid ---------------------------------------------------------------------------------------------------
INNER = {(300, 360): (128, 128), (300, 750): (128, 256)}


@pytest.mark.parametrize("prec,tol", [("f64", 1e-10), ("f32", 2e-5)])
@pytest.mark.parametrize("shape", [(300, 360), (300, 750)])
def test_band_grid_shard_equals_the_host_loop(shape, prec, tol):
    """1' pixels; (300, 750): My != Mx and an odd N-grid pitch.  Five estimators, the ten crosses and the MV auto, 6 realisations:
    n, S, C of the one-call shard == the sums of x and x x^T over the host loop, at the project's tolerance for this comparison;
    [0, 6) in one call == [0, 2) then [2, 6) bit for bit; OA_OPT_MV_BATCH = 0 gives the same moments; one estimator alone (EB, no
    weights) works and its auto is the EB block of the five-estimator run."""
    q = estimator(shape, 1.0, prec)
    grid = q.pol_band_grid(ESTS, ext_norm=True)
    print("band grid of", shape, ":", grid)
    assert grid is not None and grid[0] < shape[0] and grid[1] < shape[1]
    assert tuple(grid) == INNER[shape]
    drv = driver(shape, 1.0, prec, base_seed=31, one_call=True)
    assert drv.one_call and drv.eng.mixed and len(drv.spectra) == 16 and drv.D == 16 * 11
    X, Sref, Cref = host_moments(drv, range(6))
    assert np.all(np.isfinite(X)) and np.all(X[:, :5 * 11] > 0)
    drv.run_local(range(6))
    assert q.pol_bound_grid == INNER[shape]
    n, S, C = device_moments(drv)
    assert n == 6
    close(S, Sref, tol)
    close(C, Cref, tol)
    # cut into two calls
    cut = driver(shape, 1.0, prec, base_seed=31, one_call=True)
    cut.run_local(range(0, 2))
    cut.run_local(range(2, 6))
    n2, S2, C2 = device_moments(cut)
    assert n2 == 6 and np.array_equal(S2, S) and np.array_equal(C2, C)
    # the estimators one at a time
    e = drv.eng
    e.set_option("mv_batch", 0)
    try:
        one = driver(shape, 1.0, prec, base_seed=31, one_call=True)
        one.run_local(range(6))
        n3, S3, C3 = device_moments(one)
    finally:
        e.set_option("mv_batch", 1)
    assert n3 == 6
    close(S3, Sref, tol)
    close(C3, Cref, tol)
    # nest = 1, no cross, no MV: mv_weights NULL
    eb = driver(shape, 1.0, prec, base_seed=31, one_call=True, estimators=("EB",), cross=False, mv=False)
    assert eb.spectra == [("EB", "EB")] and eb.w is None
    _, Se, Ce = host_moments(eb, range(3))
    eb.run_local(range(3))
    n4, S4, C4 = device_moments(eb)
    assert n4 == 3
    close(S4, Se, tol)
    close(C4, Ce, tol)
    close(S4 / 3, X[:3, 3 * 11:4 * 11].mean(0), tol)


def test_band_grid_shard_on_an_explicit_grid():
    """row_grid = col_grid = 256 on (300, 360), one step above the automatic 128 x 128: the host loop's moments again"""
    shape, tol = (300, 360), 1e-10
    q = estimator(shape, 1.0, "f64", 256)
    assert q.pol_band_grid(ESTS, ext_norm=True) == (256, 256)
    drv = driver(shape, 1.0, "f64", 256, base_seed=31, one_call=True)
    _, Sref, Cref = host_moments(drv, range(6))
    drv.run_local(range(6))
    assert q.pol_bound_grid == (256, 256)
    n, S, C = device_moments(drv)
    assert n == 6
    close(S, Sref, tol)
    close(C, Cref, tol)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_interleaving_the_two_paths(prec):
    """[0, 3) in one call, a sample_host call on the same estimator (it re-binds the plan per estimator underneath), then [3, 6): the
    moments of the uninterrupted [0, 6) run, bit for bit"""
    shape = (300, 360)
    ref = driver(shape, 1.0, prec, base_seed=9, one_call=True)
    ref.run_local(range(6))
    n0, S0, C0 = device_moments(ref)
    drv = driver(shape, 1.0, prec, base_seed=9, one_call=True)
    drv.run_local(range(0, 3))
    x = drv.sample_host(3)
    assert bool(torch.isfinite(x).all())
    drv.run_local(range(3, 6))
    n1, S1, C1 = device_moments(drv)
    assert n0 == n1 == 6 and np.array_equal(S1, S0) and np.array_equal(C1, C0)


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def test_driver_paths_agree_on_300_360():
    tol = 1e-10
    a = driver((300, 360), 1.0, "f64", base_seed=7, one_call=True)
    b = driver((300, 360), 1.0, "f64", base_seed=7, one_call=False)
    assert a.one_call and not b.one_call
    a.run(6)
    b.run(6)
    assert a.acc.count("n0") == b.acc.count("n0") == 6
    close(a.acc.mean("n0"), b.acc.mean("n0"), tol)
    close(a.cov(), b.cov(), 50 * tol)
    for x in ESTS + ("MV",):
        close(a.mean(x), b.mean(x), tol)
    close(a.mean("TT", "TE"), b.mean("TE", "TT"), tol)


def test_driver_default_and_sides_without_a_one_call_path():
    from orphics_amd._lib import OrphicsAmdError
    assert not driver((300, 360), 1.0, "f32", base_seed=3).one_call          # the automatic choice is unchanged
    with pytest.raises(OrphicsAmdError, match="one_call=False"):
        driver((84, 84), 2.0, "f32", base_seed=3, one_call=True)              # 84 = 2^2 3 7: chirp-z transforms
    assert not driver((84, 84), 2.0, "f32", base_seed=3).one_call


# ---- refusals of the entry -----------------------------------------------------------------------------------------------------------
def test_entry_refusals_on_a_bound_plan():
    """raw oa_mc_run_mv calls on the bound (300, 360) plan: each is refused with a message naming the entry, the accumulators untouched"""
    drv = driver((300, 360), 1.0, "f32", base_seed=5, one_call=True)
    drv.run_local(range(1))                               # binds: oa_qe_band_bind, then oa_mc_mv_band_bind
    e, q, A = drv.eng, drv.q, drv._entry_args()
    nE, nS = len(ESTS), len(drv.spectra)
    wstride = drv.w[0].numel()
    n = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    S = torch.full((drv.D,), -3.0, dtype=torch.float64, device="cuda")
    C = torch.full((drv.D, drv.D), -3.0, dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    wl, wk, rl, rk = drv._bands
    other = torch.zeros_like(drv.fn[0])
    ids2, w2 = drv.ids.clone(), drv.w.clone()

    def call(nest=nE, fgs=A["fgs"], w=drv.w, ids=drv.ids, nids=drv.nids, nspec=nS, a=A["a"], b=A["b"], wl_=wl):
        rc = e.lib.oa_mc_run_mv(e.plan, 5, 0, 1, A["cs"], nest, A["npieces"], A["signs"], fgs, A["fhs"], A["swaps"], A["xsrc"], A["ysrc"],
                                A["fns"], P(w), wstride, nspec, a, b, P(ids), nids, P(drv.counts), float(drv.norm), int(wl_), int(wk), int(rl),
                                int(rk), int(q.mrow), P(n), P(S), P(C), None)
        return rc, (e.lib.oa_last_error() or b"").decode()

    def untouched():
        torch.cuda.synchronize()
        return int(n.item()) == 41 and bool((S == -3.0).all()) and bool((C == -3.0).all())
    bad_fg = type(A["fgs"])(*([other.data_ptr()] + list(A["fgs"])[1:]))
    zero = (ctypes.c_int * 1)(0)
    cases = [
        (dict(wl_=wl - 1), "oa_qe_band_bind"),                                   # other bands than those bound
        (dict(fgs=bad_fg), "a filter plane of this call is not bound"),
        (dict(ids=ids2), "oa_mc_mv_band_bind"),
        (dict(nids=drv.nids - 1), "oa_mc_mv_band_bind"),
        (dict(w=w2), "oa_mc_mv_band_bind"),
        (dict(nest=nE - 1, nspec=1, a=zero, b=zero), "oa_mc_mv_band_bind"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and "oa_mc_run_mv" in err and msg in err, (list(kw), rc, err)
        assert untouched(), list(kw)
    try:
        # nspec above the binding's nspec_max
        assert e.lib.oa_mc_mv_band_bind(e.plan, P(drv.w), wstride, nE, P(drv.ids), drv.nids, 4) == 0
        rc, err = call()
        assert rc != 0 and "oa_mc_run_mv" in err and "oa_mc_mv_band_bind" in err and "nspec" in err, err
        assert untouched()
        assert e.lib.oa_mc_mv_band_bind(e.plan, P(drv.w), wstride, nE, P(drv.ids), drv.nids, nS) == 0
        # a second oa_qe_band_bind drops the Monte-Carlo binding
        e._pol_owner = None
        q._pol_bind(drv.estimators, [drv.fn[i] for i in range(nE)], drv._bands, split=False)
        rc, err = call()
        assert rc != 0 and "oa_mc_run_mv" in err and "oa_mc_mv_band_bind" in err and "one_call=False" in err, err
        assert untouched()
    finally:
        e._pol_owner = None
        e._mc_owner = None
    # ... and the driver binds again by itself
    assert call()[0] != 0
    drv.run_local(range(1, 2))
    assert int(drv.acc.device_moments("n0", drv.D)[0].item()) == 2
