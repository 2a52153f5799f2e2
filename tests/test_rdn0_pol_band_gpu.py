"""GPU: the realisation-dependent N0 of the polarisation estimators and their MV combination in ONE call on map sides 2^a 3^b 5^c -- both
triples of a realisation in one inner-grid draw launch (``oa_grf_mix_band_inner_triples``), ``oa_rdn0_set_data_mv`` + ``oa_mc_run_rdn0_mv`` on
the band grid behind ``oa_qe_band_bind`` + ``oa_mc_mv_band_bind``, and ``mc.RDN0MonteCarloPol(one_call="band")``.  The reference is the
host loop of existing entries (``sample_host``), as on power-of-two sides.

Geometry and estimator set-up are tests/test_mc_pol_band_gpu.py's: 1' pixels, 1.5' beam, 1 uK' T noise and twice that power in P, T and P
filters 300-2000, kappa mask 20-3000, EDGES = linspace(100, 2900, 12), five estimators.  Band grids: (300, 360) -> (128, 128) and
(300, 750) -> (128, 256), the second with My != Mx and an odd N-grid pitch.  Data triple: e.grf_mix(17, cs, stream_id0 = 10^6), as in
tests/test_rdn0_pol_gpu.py, whose tolerances these are: close(S, Sref, tol), close(C, Cref, 50 tol) with tol = 1e-10 (f64), 4e-5 (f32)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ESTS = ("TT", "TE", "EE", "EB", "TB")
EDGES = np.linspace(100, 2900, 12)
ND = EDGES.size - 1
TOL = {"f64": 1e-10, "f32": 4e-5}
INNER = {(300, 360): (128, 128), (300, 750): (128, 256)}
SHAPES = [(300, 360), (300, 750)]
SENTINEL = complex(-7.5, 3.25)
SIMS = range(4)


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


def driver(shape, res, prec, one_call, grid="auto", data_seed=17, base_seed=31, **kw):
    """a driver whose data triple is the Gaussian draw e.grf_mix(data_seed, cs, stream_id0 = 10^6): stream ids far from the simulations'"""
    from orphics_amd import mc
    q = estimator(shape, res, prec, grid)
    e = q.eng
    drv = mc.RDN0MonteCarloPol(q, [e.hc(), e.hc(), e.hc()], geometry(shape, res)["tot_h"], EDGES, base_seed=base_seed, one_call=one_call, **kw)
    drv.set_data(e.grf_mix(data_seed, drv.cs, stream_id0=10 ** 6))
    return drv


def close(got, ref, tol, what=""):
    """the project's moment comparison: rtol, plus the same factor times the largest |entry| (cross spectra scatter around zero)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    print("%s max |got - ref| / max |ref| = %.3e (tol %.1e)" % (what, np.abs(got - ref).max() / np.abs(ref).max(), tol))
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def host_moments(shape, prec, grid="auto", ests=ESTS):
    """X, sum x, sum x x^T of the host loop over SIMS: computed once per geometry and precision, shared, never modified"""
    kw = {} if ests == ESTS else dict(estimators=ests, cross=False, mv=False)
    drv = driver(shape, 1.0, prec, False, grid, **kw)
    assert not drv.one_call
    X = torch.stack([drv.sample_host(i) for i in SIMS]).cpu().numpy()
    out = (X, X.sum(0), X.T @ X)
    for a in out:
        a.setflags(write=False)
    return out


def raw(drv):
    n, S, C = drv.acc.device_moments("rdn0", drv.D)
    torch.cuda.synchronize()
    return int(n.item()), S.cpu().numpy().copy(), C.cpu().numpy().copy()


def band_moments(shape, prec, sims=SIMS, grid="auto", **kw):
    drv = driver(shape, 1.0, prec, "band", grid, **kw)
    assert drv.one_call and drv.band_call and drv.eng.mixed
    return raw(drv.run_local(sims))


# ---- oa_grf_mix_band_inner_triples ---------------------------------------------------------------------------------------------------
MY, PITCH = 32, 32
SID = (0xC0FFEE << 32) + 12           # a stream id with its upper half set


def mix_table(e, gen):
    cs = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i + 1):               # lower triangle; the upper blocks stay NULL
            cs[i][j] = (torch.rand((e.ny, e.kp), generator=gen, device="cuda", dtype=torch.float64) + 0.25).to(e.rdt)
    cs[2][0] = None                          # a NULL block inside the triangle too
    return cs


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("width,rband", [(13, 7), (16, 16), (17, 1)])
@pytest.mark.parametrize("shape", [(60, 90), (64, 128)])
def test_two_triples_in_one_launch_are_two_single_draws(shape, width, rband, prec):
    """The six (32, 32) planes of one ntriples = 2 call == two oa_grf_mix_band_inner calls (streams SID .., SID + 3 ..) bit for bit, the
    sentinel survives everywhere outside the band, and ntriples = 1 == the existing entry.  (60, 90): odd N-grid pitch; rband 16 fills 31
    of the 32 inner rows; width 17 = the inner grid's Mx/2 + 1 with a single row."""
    from orphics_amd.engine import Engine
    ny, nx = shape
    e = Engine(ny, nx, prec)
    gen = torch.Generator(device="cuda").manual_seed(11)
    cs = mix_table(e, gen)
    rows = torch.arange(ny, device="cuda")
    ys = rows[(rows < rband) | (rows > ny - rband)]
    yo = torch.where(ys < rband, ys, ys - ny + MY)
    band = torch.zeros((MY, PITCH), dtype=torch.bool, device="cuda")
    band[yo, :width] = True
    fresh = lambda k: [torch.full((MY, PITCH), SENTINEL, dtype=e.cdt, device="cuda") for _ in range(k)]
    ref = fresh(6)
    e.grf_mix_band_inner(77, cs, ref[:3], MY, PITCH, width, rband, scale=0.75, stream_id0=SID)
    e.grf_mix_band_inner(77, cs, ref[3:], MY, PITCH, width, rband, scale=0.75, stream_id0=SID + 3)
    out = fresh(6)
    e.grf_mix_band_inner_triples(77, cs, out, MY, PITCH, width, rband, scale=0.75, stream_id0=SID)
    one = fresh(3)
    e.grf_mix_band_inner_triples(77, cs, one, MY, PITCH, width, rband, scale=0.75, stream_id0=SID)
    torch.cuda.synchronize()
    for c in range(6):
        assert torch.equal(torch.view_as_real(out[c]), torch.view_as_real(ref[c])), c
        assert bool((out[c][band] != SENTINEL).all()) and bool((out[c][~band] == SENTINEL).all()), c
    assert not torch.equal(out[0][band], out[3][band])                  # (the second triple is another draw)
    for c in range(3):
        assert torch.equal(torch.view_as_real(one[c]), torch.view_as_real(ref[c])), c


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_triples_draw_refusals(prec):
    """ntriples 0 and 3 and the existing entry's list: each returns non-zero with the entry's name before anything is launched"""
    from orphics_amd.engine import Engine
    e = Engine(60, 90, prec)
    gen = torch.Generator(device="cuda").manual_seed(3)
    cs = mix_table(e, gen)
    tab = (ctypes.c_void_p * 9)(*[c.data_ptr() if c is not None else None for r in cs for c in r])
    planes = [torch.full((128, 64), SENTINEL, dtype=e.cdt, device="cuda") for _ in range(6)]
    outs = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in planes])
    holed = (ctypes.c_void_p * 6)(*[None if i == 4 else t.data_ptr() for i, t in enumerate(planes)])

    def call(ntriples=2, my=32, pitch=32, width=13, rband=7, out=outs):
        rc = e.lib.oa_grf_mix_band_inner_triples(e.plan, 5, 0, ntriples, tab, 1.0, out, my, pitch, width, rband, None)
        return rc, (e.lib.oa_last_error() or b"").decode()
    cases = [
        (dict(ntriples=0), "1 <= ntriples <= 2"),
        (dict(ntriples=3), "1 <= ntriples <= 2"),
        (dict(rband=0), "must be positive"),
        (dict(width=0), "must be positive"),
        (dict(rband=17), "2 rband - 1 <= min(ny, my)"),                   # 33 rows > my = 32
        (dict(my=128, pitch=64, rband=31), "2 rband - 1 <= min(ny, my)"),  # 61 rows > ny = 60
        (dict(pitch=64, width=47), "width <= nx/2 + 1"),                   # nx/2 + 1 = 46
        (dict(pitch=16, width=17), "do not fit the output row pitch"),     # 2 ceil(17 / 2) = 18 > 16
        (dict(out=holed), "NULL output plane"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err and "oa_grf_mix_band_inner_triples" in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in planes)
    assert call(ntriples=1, out=holed)[0] == 0                  # (one triple reads three planes only)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in planes[3:])
    with pytest.raises(ValueError):
        e.grf_mix_band_inner_triples(5, cs, [t[:32, :32] for t in planes[:4]], 32, 32, 13, 7)


# ---- the shard on the band grid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_band_grid_shard_equals_the_host_loop(shape, prec):
    """Five estimators, the ten crosses and the MV auto, 4 realisations: n, S, C of one_call="band" == the sums of x and x x^T over the host
    loop of existing entries, at the project's tolerance for this comparison; the same with OA_OPT_MV_BATCH = 0 and with
    OA_OPT_MV_CHAIN = 0; one estimator alone (EB, no crosses, no MV, NULL weights) matches its own host loop."""
    tol = TOL[prec]
    q = estimator(shape, 1.0, prec)
    assert tuple(q.pol_band_grid(ESTS, ext_norm=True)) == INNER[shape]
    X, Sref, Cref = host_moments(shape, prec)
    assert X.shape == (4, 2 * 16 * ND) and np.all(np.isfinite(X)) and np.all(X[:, 16 * ND:21 * ND] > 0)
    n, S, C = band_moments(shape, prec)
    assert n == 4 and q.pol_bound_grid == INNER[shape]
    close(S, Sref, tol, "S %s %s" % (shape, prec))
    close(C, Cref, 50 * tol, "C %s %s" % (shape, prec))
    e = q.eng
    for opt in ("mv_batch", "mv_chain"):
        e.set_option(opt, 0)
        try:
            n2, S2, C2 = band_moments(shape, prec)
        finally:
            e.set_option(opt, 1)
        assert n2 == 4
        close(S2, Sref, tol, "S %s = 0" % opt)
        close(C2, Cref, 50 * tol, "C %s = 0" % opt)
    _, Se, Ce = host_moments(shape, prec, ests=("EB",))
    n3, S3, C3 = band_moments(shape, prec, estimators=("EB",), cross=False, mv=False)
    assert n3 == 4 and S3.shape == (2 * ND,)
    close(S3, Se, tol, "S EB alone")
    close(C3, Ce, 50 * tol, "C EB alone")


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_cuts_and_interleaved_host_calls_are_bit_equal(prec):
    """[0, 4) in one call == [0, 1) then [1, 4), bit for bit; and [0, 2), a sample_host(2) call, a data_bandpowers("EB") call (both re-bind
    the plan per estimator underneath), then [2, 4): the uninterrupted run, bit for bit -- the driver binds and sets the data again."""
    shape = (300, 360)
    n0, S0, C0 = band_moments(shape, prec)
    cut = driver(shape, 1.0, prec, "band")
    cut.run_local(range(0, 1))
    cut.run_local(range(1, 4))
    n1, S1, C1 = raw(cut)
    assert n0 == n1 == 4 and np.array_equal(S1, S0) and np.array_equal(C1, C0)
    drv = driver(shape, 1.0, prec, "band")
    drv.run_local(range(0, 2))
    own = drv.eng._pol_owner
    x = drv.sample_host(2)
    assert bool(torch.isfinite(x).all())
    assert np.all(np.isfinite(drv.data_bandpowers("EB")))
    assert drv.eng._pol_owner is not own                                # (the plan was bound by something else in between)
    drv.run_local(range(2, 4))
    n2, S2, C2 = raw(drv)
    assert n2 == 4 and np.array_equal(S2, S0) and np.array_equal(C2, C0)


def test_set_data_binds_another_triple():
    """another triple on the same driver == a fresh driver on that triple, bit for bit"""
    shape, prec = (300, 360), "f32"
    drv = driver(shape, 1.0, prec, "band")
    drv.run_local(range(2))
    first = raw(drv)
    e = drv.eng
    drv.acc = type(drv.acc)(comm=None, device=e.device)
    drv.set_data(e.grf_mix(23, drv.cs, stream_id0=10 ** 6))
    drv.run_local(range(2))
    n1, S1, C1 = raw(drv)
    n2, S2, C2 = raw(driver(shape, 1.0, prec, "band", data_seed=23).run_local(range(2)))
    assert n1 == n2 == 2 and np.array_equal(S1, S2) and np.array_equal(C1, C2)
    assert not np.array_equal(S1, first[1])


def test_band_grid_shard_on_an_explicit_grid():
    """row_grid = col_grid = 256 on (300, 360), one step above the automatic 128 x 128: the host loop's moments again"""
    shape, tol = (300, 360), TOL["f64"]
    q = estimator(shape, 1.0, "f64", 256)
    assert q.pol_band_grid(ESTS, ext_norm=True) == (256, 256)
    _, Sref, Cref = host_moments(shape, "f64", 256)
    n, S, C = band_moments(shape, "f64", grid=256)
    assert n == 4 and q.pol_bound_grid == (256, 256)
    close(S, Sref, tol, "S grid 256")
    close(C, Cref, 50 * tol, "C grid 256")


# ---- refusals of the entries ---------------------------------------------------------------------------------------------------------
def test_entry_refusals_on_a_bound_plan():
    """raw oa_rdn0_set_data_mv / oa_mc_run_rdn0_mv calls on the bound (300, 360) plan: each is refused with a message naming the entry and
    what the case is about, n, S, C untouched; afterwards run_local repairs every binding by itself."""
    from orphics_amd.engine import Engine
    shape, prec = (300, 360), "f32"
    ref = band_moments(shape, prec, sims=range(2))
    drv = driver(shape, 1.0, prec, "band")
    e, q, g = drv.eng, drv.q, drv._set
    A = g._entry_args()
    nE, nS = len(ESTS), drv.nspec
    wstride = g.w[0].numel()
    wl, wk, rl, rk = drv._bands
    n = torch.full((1,), 41, dtype=torch.int64, device="cuda")
    S = torch.full((drv.D,), -3.0, dtype=torch.float64, device="cuda")
    C = torch.full((drv.D, drv.D), -3.0, dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    kd = (ctypes.c_void_p * 3)(*[k.data_ptr() for k in drv.kd])
    other = torch.zeros_like(g.fn[0])
    ids2, w2 = drv.ids.clone(), g.w.clone()
    err = lambda: (e.lib.oa_last_error() or b"").decode()

    def set_data(plan=e.plan, fgs=A["fgs"], wl_=wl):
        return e.lib.oa_rdn0_set_data_mv(plan, kd, nE, A["npieces"], fgs, A["fhs"], A["swaps"], A["xsrc"], A["ysrc"], int(wl_), int(wk), int(rl),
                                         int(rk), int(q.mrow), None)

    def run(plan=e.plan, nest=nE, fgs=A["fgs"], w=g.w, ids=drv.ids, nids=drv.nids, nspec=nS, a=A["a"], b=A["b"], wl_=wl):
        return e.lib.oa_mc_run_rdn0_mv(plan, 5, 0, 1, A["cs"], nest, A["npieces"], A["signs"], fgs, A["fhs"], A["swaps"], A["xsrc"], A["ysrc"],
                                       A["fns"], P(w), wstride, nspec, a, b, P(ids), nids, P(drv.counts), float(drv.norm), int(wl_), int(wk),
                                       int(rl), int(rk), int(q.mrow), P(n), P(S), P(C), None)

    def untouched():
        torch.cuda.synchronize()
        return int(n.item()) == 41 and bool((S == -3.0).all()) and bool((C == -3.0).all())

    def bind(nspec_max=nS):
        e._pol_owner = None
        q._pol_bind(drv.estimators, [g.fn[i] for i in range(nE)], drv._bands, split=False)
        assert e.lib.oa_mc_mv_band_bind(e.plan, P(g.w), wstride, nE, P(drv.ids), drv.nids, nspec_max) == 0
    bad_fg = type(A["fgs"])(*([other.data_ptr()] + list(A["fgs"])[1:]))
    zero = (ctypes.c_int * 1)(0)
    try:
        e.release_pools()                                   # whatever an earlier driver left on this shared plan: no data set
        bind()
        # a run before oa_rdn0_set_data_mv
        assert run() != 0 and "oa_mc_run_rdn0_mv" in err() and "no data set" in err() and "oa_rdn0_set_data_mv" in err(), err()
        assert untouched()
        # the set-up entry's own refusals
        assert set_data(wl_=wl - 1) != 0 and "oa_rdn0_set_data_mv" in err() and "differ from the bound ones" in err(), err()
        assert set_data(fgs=bad_fg) != 0 and "oa_rdn0_set_data_mv" in err() and "a filter plane of this call is not bound" in err(), err()
        assert set_data() == 0
        cases = [
            (dict(wl_=wl - 1), "differ from the bound ones"),                        # other bands than those bound
            (dict(fgs=bad_fg), "a filter plane of this call is not bound"),
            (dict(ids=ids2), "Monte-Carlo binding"),
            (dict(nids=drv.nids - 1), "Monte-Carlo binding"),
            (dict(w=w2), "Monte-Carlo binding"),
            (dict(nest=nE - 1, nspec=1, a=zero, b=zero), "Monte-Carlo binding"),
        ]
        for kw, msg in cases:
            assert run(**kw) != 0, list(kw)
            assert "oa_mc_run_rdn0_mv" in err() and msg in err() and "one_call=False" in err(), (list(kw), err())
            assert untouched(), list(kw)
        # nspec above the binding's nspec_max
        assert e.lib.oa_mc_mv_band_bind(e.plan, P(g.w), wstride, nE, P(drv.ids), drv.nids, 4) == 0
        assert run() != 0 and "oa_mc_run_rdn0_mv" in err() and "nspec" in err() and "Monte-Carlo binding" in err(), err()
        assert untouched()
        assert e.lib.oa_mc_mv_band_bind(e.plan, P(g.w), wstride, nE, P(drv.ids), drv.nids, nS) == 0
        # the windowed entry is not on the band grid
        win = torch.ones((e.ny, e.nx), dtype=e.rdt, device="cuda")
        rc_, rs_ = q._qu_rot(False)
        assert e.lib.oa_mc_run_rdn0_mv_windowed(e.plan, 5, 0, 1, A["cs"], nE, A["npieces"], A["signs"], A["fgs"], A["fhs"], A["swaps"], A["xsrc"],
                                                A["ysrc"], A["fns"], P(g.w), wstride, nS, A["a"], A["b"], P(drv.ids), drv.nids, P(drv.counts),
                                                float(drv.norm), int(wl), int(wk), int(rl), int(rk), int(q.mrow), P(win), P(rc_), P(rs_), P(n),
                                                P(S), P(C), None) != 0
        assert "oa_mc_run_rdn0_mv_windowed" in err() and "power-of-two" in err() and "one_call=False" in err(), err()
        assert untouched()
        # the accepted call, for contrast; then a second oa_qe_band_bind: the data legs are stale
        assert run() == 0
        torch.cuda.synchronize()
        assert int(n.item()) == 42
        n.fill_(41); S.fill_(-3.0); C.fill_(-3.0)
        bind()
        assert run() != 0 and "oa_mc_run_rdn0_mv" in err() and "stale" in err() and "oa_rdn0_set_data_mv again" in err(), err()
        assert untouched()
        # an unbound plan of sides 2^a 3^b 5^c
        unbound = Engine(48, 80, prec)
        assert run(plan=unbound.plan) != 0
        assert all(w_ in err() for w_ in ("oa_mc_run_rdn0_mv", "RDN0MonteCarloPol", "one_call=False", "power-of-two", "oa_qe_band_bind",
                                          "oa_mc_mv_band_bind")), err()
        assert set_data(plan=unbound.plan) != 0
        assert all(w_ in err() for w_ in ("oa_rdn0_set_data_mv", "RDN0MonteCarloPol", "one_call=False", "oa_qe_band_bind")), err()
        assert untouched()
    finally:
        e._pol_owner = None                                 # (this test went behind the driver's back)
        e._mc_owner = None
        e._rdn0mv_owner = None
    n1, S1, C1 = raw(drv.run_local(range(2)))
    assert n1 == 2 and np.array_equal(S1, ref[1]) and np.array_equal(C1, ref[2])


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_paths_agree_on_300_360():
    tol = TOL["f64"]
    a = driver((300, 360), 1.0, "f64", "band", base_seed=7)
    b = driver((300, 360), 1.0, "f64", False, base_seed=7)
    assert a.one_call and not b.one_call
    a.run(4)
    b.run(4)
    assert a.acc.count("rdn0") == b.acc.count("rdn0") == 4
    close(a.acc.mean("rdn0"), b.acc.mean("rdn0"), tol, "mean")
    close(a.cov(), b.cov(), 50 * tol, "cov")
    for x in ESTS + ("MV",):
        close(a.rdn0(x), b.rdn0(x), tol, "rdn0 " + x)
        close(a.mcn0(x), b.mcn0(x), tol, "mcn0 " + x)
    close(a.rdn0("TT", "TE"), b.rdn0("TE", "TT"), tol, "rdn0 TT x TE")


def test_driver_opt_in_and_its_refusals():
    """one_call=True and None on (300, 360) behave as before; "band" on chirp-z sides raises naming one_call=False; another string is a
    ValueError; set_window on a "band" driver raises (set_window(None) does not); on (256, 256) "band" == True, bit for bit."""
    from orphics_amd._lib import OrphicsAmdError
    with pytest.raises(OrphicsAmdError, match="one_call=False"):
        driver((300, 360), 1.0, "f32", True)
    assert not driver((300, 360), 1.0, "f32", None).one_call
    with pytest.raises(OrphicsAmdError, match="one_call=False"):
        driver((84, 84), 2.0, "f32", "band")                               # 84 = 2^2 3 7: chirp-z transforms
    with pytest.raises(ValueError):
        driver((300, 360), 1.0, "f32", "bands")
    drv = driver((300, 360), 1.0, "f32", "band")
    assert drv.set_window(None) is drv and drv.one_call
    yy, xx = np.meshgrid(np.hanning(300), np.hanning(360), indexing="ij")
    with pytest.raises(OrphicsAmdError, match="one_call=False"):
        drv.set_window(yy * xx)
    assert drv.window is None and drv.one_call
    a = driver((256, 256), 2.0, "f32", "band")
    b = driver((256, 256), 2.0, "f32", True)
    assert a.one_call and a.eng.pow2
    na, Sa, Ca = raw(a.run_local(range(2)))
    nb, Sb, Cb = raw(b.run_local(range(2)))
    assert na == nb == 2 and np.array_equal(Sa, Sb) and np.array_equal(Ca, Cb)
