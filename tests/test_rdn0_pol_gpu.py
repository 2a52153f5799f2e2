"""GPU: the realisation-dependent N0 of an estimator set and its MV combination -- ``oa_rdn0_set_data_mv`` + ``oa_mc_run_rdn0_mv`` behind
``mc.RDN0MonteCarloPol`` -- against the host loop of existing entries (``one_call=False``), against the definition stated in NumPy with
the oracle estimators, and what it is for.

Geometry and set-up are tests/test_mc_pol_gpu.py's: (256, 256) and (128, 256) at 2' (1.5' beam, 1 uK' T noise and twice that power in P,
T and P filters 300-2000, kappa mask 20-3000), EDGES = linspace(100, 2900, 12), its close().  At those sizes the row stage takes one map
per launch: the one call runs its per-piece fallback.  The chain row stage needs row grids of 1024 points and more: (1024, 2048) at 1'.

Tolerance of one call against host loop: close(S, Sref, tol), close(C, Cref, 50 tol) with tol = 1e-10 (f64) and 4e-5 (f32): the project's
2e-5 per f32 kappa_hat bandpower term, doubled because an rdn0 entry is a difference of two terms (tests/test_rdn0_gpu.py)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ESTS = ("TT", "TE", "EE", "EB", "TB")
EDGES = np.linspace(100, 2900, 12)
TOL = {"f64": 1e-10, "f32": 4e-5}
SMALL = [(256, 256), (128, 256)]
BIG = ((1024, 2048), 1.0)
ND = EDGES.size - 1


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
    return dict(g=g, th=th, ml=ml, beam=beam, nT=nT, nP=nP, tmask=tmask, kmask=kmask, cl=cl, tot_h=tot_h)


@functools.lru_cache(maxsize=None)
def estimator(shape, res, prec):
    from orphics_amd import lensing
    G = geometry(shape, res)
    if prec == "f32" and shape == BIG[0]:               # the large geometry is set up once, in float64
        return estimator(shape, res, "f64").astype("f32")
    return lensing.qest(shape, G["g"], G["th"], noise2d=G["nT"], beam2d=G["beam"], kmask=G["tmask"], noise2d_P=G["nP"], kmask_P=G["tmask"],
                        kmask_K=G["kmask"], pol=True, unlensed_equals_lensed=True, dtype=prec)


def close(got, ref, tol):
    """the project's moment comparison: rtol, plus the same factor times the largest |entry| (cross spectra scatter around zero)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())


def driver(shape, res, prec, one_call, data_seed=17, scale=1.0, edges=EDGES, base_seed=31, **kw):
    """a driver whose data triple is the Gaussian draw e.grf_mix(data_seed, cs, stream_id0 = 10^6) times `scale` (0: zero data): stream ids
    far from the simulations' 6 i .. 6 i + 5"""
    from orphics_amd import mc
    q = estimator(shape, res, prec)
    e = q.eng
    drv = mc.RDN0MonteCarloPol(q, [e.hc(), e.hc(), e.hc()], geometry(shape, res)["tot_h"], edges, base_seed=base_seed, one_call=one_call, **kw)
    if scale:
        drv.set_data(e.grf_mix(data_seed, drv.cs, stream_id0=10 ** 6, scale=scale))
    return drv


def host_moments(drv, sims):
    X = torch.stack([drv.sample_host(i) for i in sims]).cpu().numpy()
    return X, X.sum(0), X.T @ X


def raw(drv):
    n, S, C = drv.acc.device_moments("rdn0", drv.D)
    torch.cuda.synchronize()
    return int(n.item()), S.cpu().numpy().copy(), C.cpu().numpy().copy()


def one_call_moments(*a, sims=range(4), **kw):
    drv = driver(*a, **kw)
    assert drv.one_call
    return raw(drv.run_local(sims))


# ---- one call == host loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", SMALL)
def test_one_call_equals_the_host_loop(shape, prec):
    """Five estimators, the ten crosses and the MV auto, 4 realisations: n, S, C of oa_mc_run_rdn0_mv == the sums of x and x x^T over the
    host loop of existing entries; the same with OA_OPT_MV_BATCH = 0 (one leg launch per field, one divergence per plane); the same for
    one estimator alone (EB, no crosses, no MV)."""
    tol = TOL[prec]
    host = driver(shape, 2.0, prec, False)
    assert not host.one_call and len(host.spectra) == 16 and host.D == 2 * 16 * ND
    X, Sref, Cref = host_moments(host, range(4))
    assert np.all(np.isfinite(X)) and np.all(X[:, 16 * ND:21 * ND] > 0)
    n, S, C = one_call_moments(shape, 2.0, prec, True)
    assert n == 4
    print("rdn0 pol %s %s: S err %.3g, C err %.3g (of the largest entry)" % (shape, prec, np.abs(S - Sref).max() / np.abs(Sref).max(),
                                                                         np.abs(C - Cref).max() / np.abs(Cref).max()))
    close(S, Sref, tol)
    close(C, Cref, 50 * tol)
    e = host.eng
    e.set_option("mv_batch", 0)
    try:
        n2, S2, C2 = one_call_moments(shape, 2.0, prec, True)
    finally:
        e.set_option("mv_batch", 1)
    assert n2 == 4
    close(S2, Sref, tol)
    close(C2, Cref, 50 * tol)
    kw = dict(estimators=("EB",), cross=False, mv=False)
    eb = driver(shape, 2.0, prec, False, **kw)
    assert eb.spectra == [("EB", "EB")] and eb.D == 2 * ND
    _, Se, Ce = host_moments(eb, range(4))
    n3, S3, C3 = one_call_moments(shape, 2.0, prec, True, **kw)
    assert n3 == 4
    close(S3, Se, tol)
    close(C3, Ce, 50 * tol)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_chain_row_stage(prec):
    """(1024, 2048) at 1': the first of the issue's two candidate geometries -- its row grid has 1024 points, where the row stage is the
    two-rows-per-transform kernel the chain launch needs, so the 2 nest = 10 chains (4 x the set's pieces) run as chain launches; that
    they do is visible in the moments: with OA_OPT_MV_CHAIN = 0 the same pieces are summed by accumulating launches, in another
    order, and the sums differ in their last bits (if the chain did not engage, both runs would take the per-piece launches and be
    bit-equal).  2 realisations; chain and per-piece agree to tol, and both agree with the host loop."""
    shape, res = BIG
    tol = TOL[prec]
    host = driver(shape, res, prec, False)
    _, Sref, Cref = host_moments(host, range(2))
    n1, S1, C1 = one_call_moments(shape, res, prec, True, sims=range(2))
    e = host.eng
    e.set_option("mv_chain", 0)
    try:
        n0, S0, C0 = one_call_moments(shape, res, prec, True, sims=range(2))
    finally:
        e.set_option("mv_chain", 1)
    assert n1 == n0 == 2
    assert not np.array_equal(S1, S0), "the chain row stage did not engage on this geometry"
    close(S1, S0, tol)
    close(C1, C0, 50 * tol)
    close(S1, Sref, tol)
    close(C1, Cref, 50 * tol)
    close(S0, Sref, tol)
    close(C0, Cref, 50 * tol)


# ---- determinism and identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_repeat_runs_and_cuts_are_bit_equal(prec):
    a = one_call_moments((128, 256), 2.0, prec, True)
    b = one_call_moments((128, 256), 2.0, prec, True)
    assert a[0] == 4 and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    cut = driver((128, 256), 2.0, prec, True)
    cut.run_local(range(0, 1))
    cut.run_local(range(1, 4))
    c = raw(cut)
    assert c[0] == 4 and np.array_equal(c[1], a[1]) and np.array_equal(c[2], a[2])


def test_zero_data_data_independence_scaling_and_unit_weights():
    shape, prec = (256, 256), "f64"
    h = 16 * ND
    _, S0, _ = one_call_moments(shape, 2.0, prec, True, scale=0.0)
    assert np.all(S0[h:h + 5 * ND] > 0) and np.array_equal(S0[:h], -S0[h:])        # zero data: p(A) = 0, rdn0 = -mcn0 exactly
    _, S1, _ = one_call_moments(shape, 2.0, prec, True, data_seed=17)
    _, S2, _ = one_call_moments(shape, 2.0, prec, True, data_seed=18)
    assert np.array_equal(S1[h:], S2[h:]) and np.array_equal(S1[h:], S0[h:])       # the mcn0 half carries no data
    assert not np.array_equal(S1[:h], S2[:h])
    _, S4, _ = one_call_moments(shape, 2.0, prec, True, data_seed=17, scale=2.0)
    pA1, pA4 = S1[:h] + S1[h:], S4[:h] + S4[h:]                                    # rdn0 + mcn0 = p(A), quadratic in the data
    assert np.abs(pA4 - 4 * pA1).max() <= 1e-13 * np.abs(4 * pA1).max()
    # one estimator and a weight plane of ones: the MV field is that estimator
    drv = driver(shape, 2.0, prec, True, estimators=("EB",), cross=False, mv=True)
    assert drv.spectra == [("EB", "EB"), ("MV", "MV")]
    drv.w.fill_(1.0)
    _, S, _ = raw(drv.run_local(range(4)))
    x = S.reshape(2, 2, ND)
    for half in range(2):
        assert np.abs(x[half, 1] - x[half, 0]).max() <= 1e-12 * np.abs(x[half, 0]).max()


def test_blocks_match_the_oracle_on_the_downloaded_draws():
    """128^2 float64, realisation 0: the TT and EB auto blocks and the (TT, EB) cross block of the one call == the same vector from
    QEOracle.kappa_ft applied to the downloaded data and draws (Engine.grf_mix, same seed and streams), binned with the oracle's bin2D;
    1e-8 of the largest |p(A)| of the block (test_driver_autos_match_the_oracle_on_the_downloaded_draws's bound)."""
    from oracle import qe_oracle as qo
    from oracle import stats_oracle as so
    shape, res = (128, 128), 2.0
    G = geometry(shape, res)
    g, ml = G["g"], G["ml"]
    drv = driver(shape, res, "f64", True, estimators=("TT", "EB"), cross=True, mv=False, base_seed=19)
    assert drv.spectra == [("TT", "TT"), ("EB", "EB"), ("TT", "EB")]
    e = drv.eng
    qr = qo.QEOracle(shape, g.step_y, g.step_x, G["cl"], dict(T=G["nT"], P=G["nP"]), G["beam"], dict(T=G["tmask"], P=G["tmask"]),
                     kmask_K=G["kmask"])
    bo = so.bin2D(ml, EDGES)
    full = lambda ks: [e.hc_to_full(k).cpu().numpy() for k in ks]
    d, s, sp = full(drv.kd), full(e.grf_mix(19, drv.cs, stream_id0=0)), full(e.grf_mix(19, drv.cs, stream_id0=3))
    i = {"T": 0, "E": 1, "B": 2}
    qe = lambda XY, X, Y: qr.kappa_ft(XY, X[i[XY[0]]], Y[i[XY[1]]])
    A = {XY: qe(XY, d, s) + qe(XY, s, d) for XY in ("TT", "EB")}
    B = {XY: qe(XY, s, sp) + qe(XY, sp, s) for XY in ("TT", "EB")}
    p = lambda u, v: bo.bin((u * np.conj(v)).real * drv.norm)[1]
    _, S, _ = raw(drv.run_local([0]))
    x = S.reshape(2, 3, ND)
    for j, (a, b) in enumerate(drv.spectra):
        pa, pb = p(A[a], A[b]), p(B[a], B[b])
        scale = np.abs(pa).max()
        err = max(np.abs(x[0, j] - (pa - pb / 2)).max(), np.abs(x[1, j] - pb / 2).max()) / scale
        print("rdn0 pol against NumPy, block %s x %s: %.3g of max |p(A)|" % (a, b, err))
        assert scale > 0 and err <= 1e-8, (a, b, err)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def raw_calls(drv):
    """the two C entries with the driver's own arguments (nest overridable), and the last error"""
    from orphics_amd.engine import _ptr, _stream
    e, q, g = drv.eng, drv.q, drv._set
    A = g._entry_args()
    wl, wk, rl, rk = g._bands
    nE = len(drv.estimators)
    n, S, C = drv.acc.device_moments("rdn0", drv.D)
    kd = (ctypes.c_void_p * 3)(*[k.data_ptr() for k in drv.kd])

    def set_data(plan=e.plan):
        return e.lib.oa_rdn0_set_data_mv(plan, kd, nE, A["npieces"], A["fgs"], A["fhs"], A["swaps"], A["xsrc"], A["ysrc"], int(wl), int(wk), int(rl),
                                         int(rk), int(q.mrow), _stream())

    def run(lo, hi, nest=nE, plan=e.plan):
        return e.lib.oa_mc_run_rdn0_mv(plan, drv.base_seed, lo, hi, A["cs"], nest, A["npieces"], A["signs"], A["fgs"], A["fhs"], A["swaps"], A["xsrc"],
                                       A["ysrc"], A["fns"], _ptr(drv.w), drv.w[0].numel(), drv.nspec, A["a"], A["b"], _ptr(drv.ids), drv.nids,
                                       _ptr(drv.counts), float(drv.norm), int(wl), int(wk), int(rl), int(rk), int(q.mrow), _ptr(n), _ptr(S), _ptr(C),
                                       _stream())
    err = lambda: (e.lib.oa_last_error() or b"").decode()
    return set_data, run, err, (n, S, C)


def test_refusals_leave_the_moments_untouched():
    """Refused by name before anything is launched: a (48, 80) plan (both entries; the message names the driver and one_call=False), a run
    before any data is set, stale data legs after oa_plan_set_col_grid with another grid -- repaired by oa_rdn0_set_data_mv --, and
    nest = 7.  n, S, C keep what the accepted calls left."""
    from orphics_amd._lib import check
    from orphics_amd.engine import Engine
    shape, res = BIG                                                   # (a geometry with a column grid: 512 of its 1024 rows)
    drv = driver(shape, res, "f32", True)
    e, q = drv.eng, drv.q
    set_data, run, err, (n, S, C) = raw_calls(drv)
    snap = lambda: (int(n.item()), S.clone(), C.clone())
    same = lambda s: int(n.item()) == s[0] and torch.equal(S, s[1]) and torch.equal(C, s[2])
    e.release_pools()                                                  # whatever an earlier driver left on this shared plan
    check(e.lib.oa_plan_set_col_grid(e.plan, int(q.mcol)))
    s0 = snap()
    # a mixed-radix plan
    other = Engine(48, 80, "f32")
    assert run(0, 1, plan=other.plan) != 0
    assert "oa_mc_run_rdn0_mv" in err() and "RDN0MonteCarloPol" in err() and "one_call=False" in err() and "power-of-two" in err()
    assert set_data(plan=other.plan) != 0 and "oa_rdn0_set_data_mv" in err() and "RDN0MonteCarloPol" in err() and "one_call=False" in err()
    # no data set
    assert run(0, 2) != 0 and "no data set" in err() and "oa_rdn0_set_data_mv" in err()
    torch.cuda.synchronize()
    assert same(s0) and s0[0] == 0
    drv.run_local([0, 1])                                              # sets the data, runs two realisations
    torch.cuda.synchronize()
    s1 = snap()
    assert s1[0] == 2
    # nest = 7
    assert run(2, 4, nest=7) != 0 and "1 <= nest <= 6" in err()
    # another column grid: the data legs are stale
    assert q.eng.lib.oa_plan_set_col_grid(e.plan, 0) == 0
    assert run(2, 4) != 0 and "stale" in err() and "oa_plan_set_col_grid" in err() and "oa_rdn0_set_data_mv" in err()
    torch.cuda.synchronize()
    assert same(s1)
    check(set_data())
    check(run(2, 4))
    torch.cuda.synchronize()
    assert int(n.item()) == 4
    e._rdn0mv_owner = None                                             # (this test went behind the driver's back)
    check(e.lib.oa_plan_set_col_grid(e.plan, int(q.mcol)))
    ref = one_call_moments(shape, res, "f32", True)
    close(S.cpu().numpy(), ref[1], TOL["f32"])                        # (realisations 2, 3 ran on the map's own rows: same sums, other rounding)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
def test_driver_on_other_sides_and_accessors():
    """300 x 360 at 1': one_call=None is the host loop, one_call=True raises naming one_call=False; 2 realisations give finite means with
    positive mcn0 autos; the accessors are symmetric in (a, b) and debiased = data_bandpowers - rdn0."""
    from orphics_amd._lib import OrphicsAmdError
    drv = driver((300, 360), 1.0, "f32", None)
    assert not drv.one_call
    with pytest.raises(OrphicsAmdError, match="one_call=False"):
        driver((300, 360), 1.0, "f32", True)
    st = drv.run(2)
    assert st.count("rdn0") == 2 and np.all(np.isfinite(st.mean("rdn0")))
    for x in ESTS + ("MV",):
        assert drv.mcn0(x).shape == (ND,) and np.all(drv.mcn0(x) > 0), x
    np.testing.assert_array_equal(drv.rdn0("TT", "TE"), drv.rdn0("TE", "TT"))
    np.testing.assert_array_equal(drv.mcn0("TT", "TE"), drv.mcn0("TE", "TT"))
    np.testing.assert_allclose(drv.debiased("EB"), drv.data_bandpowers("EB") - drv.rdn0("EB"), rtol=1e-13)
    np.testing.assert_allclose(drv.debiased("TT", "TE"), drv.data_bandpowers("TE", "TT") - drv.rdn0("TT", "TE"), rtol=1e-13)
    assert drv.sem("MV").shape == (ND,) and drv.cov().shape == (drv.D, drv.D) and drv.centers.shape == (ND,)
    assert drv.spectra[:5] == [(x, x) for x in ESTS] and drv.spectra[-1] == ("MV", "MV")
    with pytest.raises(KeyError):
        drv.rdn0("TT", "BB")


def test_driver_paths_agree_and_take_real_tqu_maps():
    """256^2 float64: run() of the one call and of the host loop agree; data given as real T, Q, U maps (qu=True) equals data given as the
    T, E, B transforms those maps rotate to."""
    a = driver((256, 256), 2.0, "f64", None)
    b = driver((256, 256), 2.0, "f64", False)
    assert a.one_call and not b.one_call
    a.run(3)
    b.run(3)
    assert a.acc.count("rdn0") == b.acc.count("rdn0") == 3
    close(a.acc.mean("rdn0"), b.acc.mean("rdn0"), 1e-10)
    for x in ESTS + ("MV",):
        close(a.rdn0(x), b.rdn0(x), 1e-10)
    q, e = a.q, a.eng
    maps_ = [torch.randn((e.ny, e.nx), dtype=e.rdt, device=e.device, generator=torch.Generator(device=e.device).manual_seed(3 + j)) for j in range(3)]
    from orphics_amd import mc
    tot = geometry((256, 256), 2.0)["tot_h"]
    m = mc.RDN0MonteCarloPol(q, maps_, tot, EDGES, base_seed=31, qu=True)
    k = mc.RDN0MonteCarloPol(q, q._maps_to_hc([tuple(maps_)], True, False)[0], tot, EDGES, base_seed=31)
    assert np.array_equal(raw(m.run_local([0]))[1], raw(k.run_local([0]))[1])


# ---- what the feature is for ---------------------------------------------------------------------------------------------------------------
def test_rdn0_follows_the_power_of_the_data():
    """The data triple is drawn with total power (1 + eps) times the simulations', eps = 0.5; 256^2 at 2', float64, 12 realisations, five
    estimators and MV.  A plain N0 (the mcn0 half) knows nothing of that; the RDN0 follows the data's power: the expectation of
    sum_j rdn0_MV / sum_j mcn0_MV is 1 + 2 eps = 2 (A is linear in the data: p(A) scales with 1 + eps, and rdn0 = p(A) - mcn0 with
    E p(A) = 2 mcn0 at eps = 0), against 1 for a plain N0.
    The margin is not taken from the GPU result: the same ratio, computed on the CPU with QEOracle.kappa_ft (weights w_a = N_a^-1 / sum_b
    N_b^-1 of its Nlkk) on rng_oracle.grf_mix's statement of the draws (simulations: seed 31, streams 6 i and 6 i + 3, i < 12; data: seeds
    101 .. 105, stream 10^6, times sqrt(1.5)), gave for the five data seeds
        1.97888145  1.99943526  2.01106386  2.00086063  1.97794846
    mean 1.99364, scatter (ddof = 1) 0.014606; three times that, 0.043818, is the margin.  The data of this test is seed 101's."""
    eps, margin = 0.5, 0.043818
    drv = driver((256, 256), 2.0, "f64", True, data_seed=101, scale=np.sqrt(1 + eps))
    drv.run(12)
    assert drv.acc.count("rdn0") == 12
    ratio = drv.rdn0("MV").sum() / drv.mcn0("MV").sum()
    print("sum rdn0_MV / sum mcn0_MV = %.8f (1 + 2 eps = %.1f, margin %.6f)" % (ratio, 1 + 2 * eps, margin))
    assert abs(ratio - (1 + 2 * eps)) <= margin
    assert abs(ratio - 1) > 10 * margin
