"""GPU: the windowed N0 / mean-field Monte Carlo of the polarisation estimators and their MV combination -- the one-call shard
``oa_mc_run_mv_windowed`` (power-of-two sides) against the host loop of the existing entries, the driver arguments ``window`` and
``mean_field`` of ``mc.GaussianN0MonteCarloPol``, the oracle on the same windowed maps, and what the feature is for: the window multiplies
Q and U, so a taper leaks E into B.

Geometry: that of tests/test_mc_pol_gpu.py (2' pixels, 1.5' beam, 1 uK' T noise and twice that power in P, T and P masks 300-2000, kappa
mask 20-3000, EDGES = linspace(100, 2900, 12)); the taper is ``maps.get_taper(shape, g, 12.0, 3.0)[0]``.  Moments are compared with that
file's ``close`` (rtol = tol, atol = tol max|ref|), a stack as max|a - b| < tol max|b| per label.  Tolerances, from the windowed TT and
the unwindowed pol tests: windowed one call vs host loop 1e-10 (f64) / 3e-5 (f32), unwindowed 1e-10 / 2e-5."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import maps_oracle as mo  # noqa: E402
from oracle import qe_oracle as qo  # noqa: E402

ESTS = ("TT", "TE", "EE", "EB", "TB")
EDGES = np.linspace(100, 2900, 12)
NB = EDGES.size - 1
WTOL = {"f64": 1e-10, "f32": 3e-5}
UTOL = {"f64": 1e-10, "f32": 2e-5}


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
    return lensing.qest(shape, G["g"], G["th"], noise2d=G["nT"], beam2d=G["beam"], kmask=G["tmask"], noise2d_P=G["nP"], kmask_P=G["tmask"],
                        kmask_K=G["kmask"], pol=True, unlensed_equals_lensed=True, dtype=prec)


@functools.lru_cache(maxsize=None)
def taper(shape, res):
    from orphics_amd import maps
    return np.asarray(maps.get_taper(shape, geometry(shape, res)["g"], 12.0, 3.0)[0], dtype=np.float64)


def driver(shape, res, prec, tot_h=None, **kw):
    from orphics_amd import mc
    return mc.GaussianN0MonteCarloPol(estimator(shape, res, prec), geometry(shape, res)["tot_h"] if tot_h is None else tot_h, EDGES, **kw)


def close(got, ref, tol):
    """the project's moment comparison: rtol, plus the same factor times the largest |entry| (cross spectra scatter around zero)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())


def moments(drv):
    n, S, C = drv.acc.device_moments("n0", drv.D)
    return int(n.item()), S.cpu().numpy().copy(), C.cpu().numpy().copy()


def stacks(drv):
    return {lab: t.cpu().numpy().copy() for lab, t in zip(drv.mf_labels, drv._stacks())}


def host_reference(drv, sims):
    """sums of x and x x^T over the host loop, and its stacks"""
    X = torch.stack([drv.sample_host(i, stack=drv.mean_field) for i in sims]).cpu().numpy()
    return X, X.sum(0), X.T @ X, stacks(drv)


def stacks_close(got, ref, tol, labels=None):
    for lab in (labels or ref):
        a, b = got[lab], ref[lab]
        scale = np.abs(b).max()
        assert scale > 0, lab
        err = np.abs(a - b).max()
        print("stack %-6s max|a - b| / max|b| = %.3g" % (lab, err / scale))
        assert err < tol * scale, (lab, err / scale)


# ---- one call == host loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(256, 256), (128, 256), (256, 128)])
def test_one_call_equals_the_host_loop(shape, prec):
    """Five estimators, the ten crosses and the MV auto, 4 realisations, the 12 % / 3 % taper, mean_field=True: n, S, C and all six stacks
    of oa_mc_run_mv_windowed == the host loop (Engine.grf_mix(rot=(c, -s)), Engine.irfft(window=...), Engine.rfft, Engine.rot2,
    reconstruct_hc per estimator, the weighted sum and the stacks in torch); [0, 4) in one call == [0, 1) then [1, 4) bit for bit;
    OA_OPT_MV_BATCH = 0 gives the same within tolerance; EB alone works and its block equals the EB block of the full run."""
    tol = WTOL[prec]
    w = taper(shape, 2.0)
    kw = dict(base_seed=31, window=w, mean_field=True)
    ref = driver(shape, 2.0, prec, one_call=False, **kw)
    X, Sref, Cref, Mref = host_reference(ref, range(4))
    assert not ref.one_call and np.all(np.isfinite(X)) and np.all(X[:, :5 * NB] > 0)
    drv = driver(shape, 2.0, prec, **kw)
    assert drv.one_call and len(drv.spectra) == 16 and drv.mf_labels == ["mf_" + x for x in ESTS + ("MV",)]
    drv.run_local(range(4))
    n, S, C = moments(drv)
    M = stacks(drv)
    drv.acc.allreduce()
    assert n == 4 and drv.acc.count("n0") == 4
    close(S, Sref, tol)
    close(C, Cref, tol)
    stacks_close(M, Mref, tol)
    sup = (drv.rk, drv.wk)
    for lab in drv.mf_labels:
        assert drv.acc.stack_count(lab) == 4 and M[lab].shape == (shape[0], drv.eng.kp, 2)
        assert drv.acc._pile[lab].support == sup
    # cut into two calls
    cut = driver(shape, 2.0, prec, **kw)
    cut.run_local(range(0, 1))
    cut.run_local(range(1, 4))
    n2, S2, C2 = moments(cut)
    M2 = stacks(cut)
    assert n2 == 4 and np.array_equal(S2, S) and np.array_equal(C2, C)
    for lab in drv.mf_labels:
        assert np.array_equal(M2[lab], M[lab]), lab
    # the estimators one at a time
    e = drv.eng
    e.set_option("mv_batch", 0)
    try:
        one = driver(shape, 2.0, prec, **kw)
        one.run_local(range(4))
        n3, S3, C3 = moments(one)
        M3 = stacks(one)
    finally:
        e.set_option("mv_batch", 1)
    assert n3 == 4
    close(S3, Sref, tol)
    close(C3, Cref, tol)
    stacks_close(M3, Mref, tol)
    # nest = 1
    eb = driver(shape, 2.0, prec, estimators=("EB",), cross=False, mv=False, **kw)
    assert eb.spectra == [("EB", "EB")] and eb.mf_labels == ["mf_EB"]
    eb.run_local(range(4))
    n4, S4, C4 = moments(eb)
    assert n4 == 4
    close(S4, S[3 * NB:4 * NB], tol)
    close(C4, C[3 * NB:4 * NB, 3 * NB:4 * NB], tol)
    stacks_close(stacks(eb), M, tol, labels=["mf_EB"])


def test_one_call_equals_the_host_loop_with_row_and_column_grids_engaged():
    """2048^2 at 1', float32, 2 realisations: the smallest geometry at which the 1024-point row grid and the 1024-row column grid engage
    (test_pol_and_mv_match_oracle_with_row_and_column_grids_engaged); moments and the MV stack against the host loop"""
    shape, res, prec = (2048, 2048), 1.0, "f32"
    tol = WTOL[prec]
    kw = dict(base_seed=5, window=taper(shape, res), mean_field=True)
    ref = driver(shape, res, prec, one_call=False, **kw)
    X, Sref, Cref, Mref = host_reference(ref, range(2))
    assert np.all(np.isfinite(X))
    drv = driver(shape, res, prec, **kw)
    drv.run_local(range(2))
    n, S, C = moments(drv)
    assert n == 2
    close(S, Sref, tol)
    close(C, Cref, tol)
    stacks_close(stacks(drv), Mref, tol, labels=["mf_MV"])


# ---- fused row pass == two-pass flow ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_fused_row_pass_equals_the_two_pass_flow(prec):
    shape, tol = (256, 256), WTOL[prec]
    kw = dict(base_seed=11, window=taper(shape, 2.0), mean_field=True)
    e = estimator(shape, 2.0, prec).eng
    out = {}
    try:
        for fused in (0, 1):
            e.set_option("win_fused", fused)
            drv = driver(shape, 2.0, prec, **kw)
            drv.run_local(range(3))
            out[fused] = moments(drv) + (stacks(drv),)
    finally:
        e.set_option("win_fused", 1)
    assert out[0][0] == out[1][0] == 3
    close(out[1][1], out[0][1], tol)
    close(out[1][2], out[0][2], tol)
    stacks_close(out[1][3], out[0][3], tol)


# ---- window == 1, window NULL ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_unit_window_and_no_window(prec):
    """window = ones reproduces the unwindowed driver's means (same Philox counters: rounding only); window=None with mean_field=True gives
    the plain driver's moments bit for bit, and its stacks equal the host loop's"""
    shape, tol = (256, 256), UTOL[prec]
    plain = driver(shape, 2.0, prec, base_seed=23)
    plain.run_local(range(3))
    plain.acc.allreduce()
    n0, S0, C0 = moments(plain)
    ones = driver(shape, 2.0, prec, base_seed=23, window=np.ones(shape))
    assert ones.window_moments == (1.0, 1.0)
    ones.run_local(range(3))
    ones.acc.allreduce()
    close(ones.acc.mean("n0"), plain.acc.mean("n0"), tol)
    for x in ESTS + ("MV",):
        close(ones.debiased_mean(x), plain.mean(x), tol)
    mf = driver(shape, 2.0, prec, base_seed=23, mean_field=True)
    assert mf.window is None and mf.one_call
    mf.run_local(range(3))
    n1, S1, C1 = moments(mf)
    assert n1 == n0 == 3 and np.array_equal(S1, S0) and np.array_equal(C1, C0)
    ref = driver(shape, 2.0, prec, base_seed=23, mean_field=True, one_call=False)
    _, _, _, Mref = host_reference(ref, range(3))
    stacks_close(stacks(mf), Mref, tol)


# ---- the oracle on the same maps -------------------------------------------------------------------------------------------------------
def test_stacks_match_the_oracle_on_the_windowed_maps():
    """128^2 float64, 2 realisations, TT and EB: the windowed T, Q, U maps of the host-loop steps, downloaded; in NumPy fft2, the oracle's
    Q,U -> E,B rotation and QEOracle.kappa_ft; mf_TT and mf_EB of the ONE-CALL path divided by the count == the oracle mean within
    1e-8 max|ref| over the kappa mask's support (test_pol_estimators_match_oracle's tolerance)"""
    shape, res = (128, 128), 2.0
    G = geometry(shape, res)
    g = G["g"]
    kw = dict(base_seed=19, estimators=("TT", "EB"), cross=False, mv=False, window=taper(shape, res), mean_field=True)
    host = driver(shape, res, "f64", one_call=False, **kw)
    qr = qo.QEOracle(shape, g.step_y, g.step_x, G["cl"], dict(T=G["nT"], P=G["nP"]), G["beam"], dict(T=G["tmask"], P=G["tmask"]),
                     kmask_K=G["kmask"])
    for XY in ("TT", "EB"):
        qr.setup(XY)
    fo = mo.FourierCalc((3,) + shape, g.step_y, g.step_x)
    mean = {XY: 0 for XY in ("TT", "EB")}
    for i in range(2):
        host.sample_host(i)
        tqu = np.stack([m.cpu().numpy() for m in host.host_maps])
        assert np.abs(tqu[:, 0, :]).max() == 0 and np.abs(tqu).max() > 0          # the taper's padding: the maps ARE windowed
        k = np.fft.fft2(tqu, axes=(-2, -1))
        teb = k.copy()
        teb[-2:] = mo.map_mul(fo.rot, k[-2:])                                      # the oracle's Q,U -> E,B rotation (iau=False)
        f = dict(T=teb[0], E=teb[1], B=teb[2])
        for XY in mean:
            mean[XY] = mean[XY] + qr.kappa_ft(XY, f[XY[0]], f[XY[1]]) / 2
    drv = driver(shape, res, "f64", **kw)
    drv.run_local(range(2))
    drv.acc.allreduce()
    M = stacks(drv)
    nxh = shape[1] // 2
    sup = G["kmask"][:, :nxh + 1] > 0
    for XY in ("TT", "EB"):
        got = (M["mf_" + XY][..., 0] + 1j * M["mf_" + XY][..., 1])[:, :nxh + 1] / drv.acc.stack_count("mf_" + XY)
        ref = mean[XY][:, :nxh + 1]
        err = np.abs(got - ref)[sup].max() / np.abs(ref[sup]).max()
        print("oracle %s: max|stack / n - oracle mean| / max|ref| over the kappa mask = %.3g" % (XY, err))
        assert err < 1e-8, (XY, err)


# ---- what it is for --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(256, 256), (128, 256)])
def test_a_taper_leaks_E_into_B(shape, prec):
    """total_power with BB = 0: the draw has no B.  With window = ones the EB auto (quadratic in B) is at rounding level; with the taper,
    which multiplies Q and U, E leaks into B (NumPy: B/E power 9.4e-3 at 256^2, 2.6e-2 at 128 x 256 in 300 < l < 2000, against 3e-32):
    in every bin EB(ones) <= 1e-6 EB(taper) and EB(taper) > 0.  Windowing E and B as scalars, or skipping either rotation, fails this."""
    tot = dict(geometry(shape, 2.0)["tot_h"])
    tot["BB"] = np.zeros_like(tot["BB"])
    kw = dict(base_seed=41, estimators=("EB",), cross=False, mv=False)
    flat = driver(shape, 2.0, prec, tot_h=tot, window=np.ones(shape), **kw)
    flat.run_local(range(3))
    flat.acc.allreduce()
    tap = driver(shape, 2.0, prec, tot_h=tot, window=taper(shape, 2.0), **kw)
    tap.run_local(range(3))
    tap.acc.allreduce()
    a, b = flat.mean("EB"), tap.mean("EB")
    print("EB auto, ones / taper per bin:", a / b)
    assert a.shape == b.shape == (NB,) and np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    assert np.all(b > 0)
    assert np.all(a <= 1e-6 * b)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _last_error(lib):
    return (lib.oa_last_error() or b"").decode()


def test_the_entry_refuses_other_sides_before_any_launch():
    """a 48 x 80 (mixed-radix) plan through the raw entry: refused by name, accumulators and stack untouched"""
    from orphics_amd.engine import Engine
    e = Engine(48, 80, "f32")
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    one_i, one_d, one_p = (ctypes.c_int * 1)(1), (ctypes.c_double * 1)(1.0), (ctypes.c_void_p * 1)(t.data_ptr())
    zero_i = (ctypes.c_int * 1)(0)
    nine = (ctypes.c_void_p * 9)(*([t.data_ptr()] * 9))
    rc = e.lib.oa_mc_run_mv_windowed(e.plan, 1, 0, 1, nine, 1, one_i, one_d, one_p, one_p, zero_i, zero_i, zero_i, one_p, None, 0, 1, zero_i, zero_i,
                                     p, 14, p, 1.0, 4, 4, 4, 4, -1, p, p, p, p, p, p, one_p, None)
    err = _last_error(e.lib)
    assert rc != 0 and "oa_mc_run_mv_windowed" in err and "GaussianN0MonteCarloPol" in err and "one_call=False" in err, err
    torch.cuda.synchronize()
    assert bool((t == 0).all())


def test_the_entry_refuses_a_window_without_rotation_planes():
    """the driver's own arguments on a 128^2 plan, the rotation planes withheld: refused the same way, n, S, C and the stacks stay zero"""
    from orphics_amd.engine import _ptr
    drv = driver((128, 128), 2.0, "f32", base_seed=3, window=taper((128, 128), 2.0), mean_field=True)
    e, q, A = drv.eng, drv.q, drv._entry_args()
    n, S, C = drv.acc.device_moments("n0", drv.D)
    mfs = drv._stacks()
    mfp = (ctypes.c_void_p * len(mfs))(*[t.data_ptr() for t in mfs])
    wl, wk, rl, rk = drv._bands
    for rc_, rs_ in ((None, None), (_ptr(drv.rot[0]), None), (None, _ptr(drv.rot[1]))):
        rc = e.lib.oa_mc_run_mv_windowed(e.plan, drv.base_seed, 0, 2, A["cs"], len(drv.estimators), A["npieces"], A["signs"], A["fgs"], A["fhs"],
                                         A["swaps"], A["xsrc"], A["ysrc"], A["fns"], _ptr(drv.w), drv.w[0].numel(), len(drv.spectra), A["a"], A["b"],
                                         _ptr(drv.ids), drv.nids, _ptr(drv.counts), float(drv.norm), int(wl), int(wk), int(rl), int(rk), int(q.mrow),
                                         _ptr(drv.window), rc_, rs_, _ptr(n), _ptr(S), _ptr(C), mfp, None)
        err = _last_error(e.lib)
        assert rc != 0 and "oa_mc_run_mv_windowed" in err and "GaussianN0MonteCarloPol" in err and "one_call=False" in err and "rot_c" in err, err
    torch.cuda.synchronize()
    assert int(n.item()) == 0 and bool((S == 0).all()) and bool((C == 0).all()) and all(bool((t == 0).all()) for t in mfs)


def test_driver_on_other_sides():
    """300 x 360 at 1': one_call=True with a window raises, naming one_call=False; the automatic choice is the host loop -- 2 realisations,
    finite results, stacks counted"""
    from orphics_amd import _lib
    shape, res = (300, 360), 1.0
    w = taper(shape, res)
    with pytest.raises(_lib.OrphicsAmdError, match="one_call=False"):
        driver(shape, res, "f32", base_seed=3, window=w, one_call=True)
    with pytest.raises(_lib.OrphicsAmdError, match="one_call=False"):
        driver(shape, res, "f32", base_seed=3, mean_field=True, one_call=True)
    drv = driver(shape, res, "f32", base_seed=3, window=w, mean_field=True)
    assert not drv.one_call
    st = drv.run(2)
    assert st.count("n0") == 2
    m = drv.debiased_mean("TT")
    assert m.shape == (NB,) and np.all(np.isfinite(st.mean("n0"))) and np.all(m > 0) and np.all(drv.mean("MV") > 0)
    np.testing.assert_allclose(m * np.mean(w ** 4), drv.mean("TT"), rtol=1e-14)
    for lab in drv.mf_labels:
        assert st.stack_count(lab) == 2
        s = st.stack_sum(lab)
        assert s.shape == (shape[0], drv.eng.kp, 2) and np.all(np.isfinite(s)) and np.abs(s).max() > 0
