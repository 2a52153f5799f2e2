"""GPU: oa_qe_pol / oa_qe_mv on map sides 2^a 3^b 5^c (BAND GRID behind oa_qe_band_bind, include/orphics_amd.h): TE / EE / EB / TB / TT
through ``reconstruct_hc`` and the five-estimator MV combination through ``reconstruct_mv_hc`` against the modular chain of the same
object and the NumPy oracle, split legs, the independence of the TT and the polarisation bindings, the refusals, and power-of-two
plans unchanged."""
import ctypes

import numpy as np
import pytest

from oracle import qe_oracle as qo

pytestmark = pytest.mark.gpu

ESTS = ("TT", "TE", "EE", "EB", "TB")
TOL = {"f64": 1e-11, "f32": 2e-5}            # the TT band-grid tolerances (tests/test_mixed_onecall_gpu.py), on max |kappa_hat|

# name -> shape, arcmin, lmax of the kappa mask, lmax of the polarisation mask (None: the T mask's 2000), estimator keywords.
# 600 x 750 at 1': My != Mx (ell spacing 36 x 28.8: legs 56 rows x 70 columns, kappa 98 x 122 -> 2*56+98 = 210 -> 256 rows,
# 2*70+122 = 262 -> 512 columns); 1200^2 at 0.5': the notebook's patch (56 / 84 -> 196 -> 256^2); a polarisation mask to 1800 with
# kappa to 3400 (P legs 51 x 63, kappa 95 x 119 -> 2*63+119 = 245 -> 256 x 256, not the TT binding's 2*70+119 = 259 -> 256 x 512; the
# kappa cut stays below 2 x 1800 = 3600, where EE / EB have no mode pairs left and 1 / response is rounding noise in ANY path);
# row / column grid 512, one step above the automatic 256.
CASES = {
    "600x750": ((600, 750), 1.0, 3500, None, {}),
    "1200": ((1200, 1200), 0.5, 3000, None, {}),
    "narrowP": ((600, 750), 1.0, 3400, 1800, {}),
    "explicit": ((1200, 1200), 0.5, 3000, None, dict(row_grid=512, col_grid=512)),
}


def _setup(shape, res, kmax, pmax, seed):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    nP = 2 * nT
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    pmask = tmask if pmax is None else maps.mask_kspace(shape, g, lmin=300, lmax=pmax)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=kmax)
    cl = {k: th.lCl(k, ml) for k in ("TT", "EE", "BB", "TE")}
    rng = np.random.default_rng(seed)
    sc = 1.0 / np.sqrt(g.pixarea)
    w1, w2, w3 = (np.fft.fft2(rng.standard_normal(shape)) for _ in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.nan_to_num(cl["TE"] / np.sqrt(cl["TT"] * cl["EE"]))
    kT = w1 * np.sqrt(cl["TT"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nT) * sc
    kE = (r * w1 + np.sqrt(1 - r ** 2) * w2) * np.sqrt(cl["EE"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nP) * sc
    kB = w3 * np.sqrt(cl["BB"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nP) * sc
    return dict(g=g, th=th, ml=ml, beam=beam, nT=nT, nP=nP, tmask=tmask, pmask=pmask, kmask=kmask, cl=cl, k=dict(T=kT, E=kE, B=kB))


_SET = {}       # case -> host set-up and the float64 estimator
_Q = {}         # (case, prec) -> (estimator, hc transforms)


def _prepared(case, prec):
    from orphics_amd import lensing
    if case not in _SET:
        shape, res, kmax, pmax, kw = CASES[case]
        s = _setup(shape, res, kmax, pmax, seed=sum(shape) + (pmax or 0))
        s["q"] = lensing.qest(shape, s["g"], s["th"], dtype="f64", noise2d=s["nT"], beam2d=s["beam"], kmask=s["tmask"], noise2d_P=s["nP"],
                              kmask_P=s["pmask"], kmask_K=s["kmask"], pol=True, unlensed_equals_lensed=True, **kw)
        s["q"].mv_weights(ESTS)              # every estimator set up once, in float64
        _SET[case] = s
    if (case, prec) not in _Q:
        q = _SET[case]["q"] if prec == "f64" else _SET[case]["q"].astype("f32")
        e = q.eng
        _Q[(case, prec)] = (q, {X: e.full_to_hc(e.to_complex(_SET[case]["k"][X])) for X in "TEB"})
    return _SET[case], _Q[(case, prec)][0], _Q[(case, prec)][1]


def _band(e, wk, rk):
    import torch
    ky = np.fft.fftfreq(e.ny, 1.0 / e.ny)
    m = np.zeros((e.ny, e.kp), dtype=bool)
    m[np.abs(ky) < rk, :wk] = True
    return torch.as_tensor(m, device=e.device)


def _close(got, ref, e, tol):
    d = float((got - ref)[:, :e.nxh + 1].abs().max())
    s = float(ref.abs().max())
    print("max |diff| / max |ref| = %.3e (tol %.1e)" % (d / s, tol))
    assert d <= tol * s


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_onecall_pol_and_mv_on_band_grid_equal_modular_chain(case, prec):
    """Every XY through reconstruct_hc and the MV of five through reconstruct_mv_hc == the modular chain of the same object; exact
    zeros outside kappa's band, also in a caller plane that held 7 + 7j; accumulate twice == 2 x one call."""
    s, q, k = _prepared(case, prec)
    e = q.eng
    shape = CASES[case][0]
    tol = TOL[prec]
    assert e.mixed and q.one_call_pol(ESTS) and all(q.one_call_pol(XY) for XY in ESTS)
    for XY in ESTS:
        G = q._setup_general(XY)
        grid = q.pol_band_grid(XY)
        assert grid is not None and grid[0] < shape[0] and grid[1] < shape[1]
        ref = q._reconstruct_hc_modular(XY, k[XY[0]], k[XY[1]]).clone()
        got = q.reconstruct_hc(XY, k[XY[0]], k[XY[1]])
        assert q.pol_bound_grid == grid                       # the call went through the binding, on the grid the host rule gives
        band = _band(e, G["wk"], G["rk"])
        _close(got, ref, e, tol)
        assert float(got[~band].abs().max()) == 0.0
        out = e.hc()
        out.fill_(7 + 7j)
        assert q.reconstruct_hc(XY, k[XY[0]], k[XY[1]], out=out) is out
        assert float(out[~band].abs().max()) == 0.0
        _close(out, ref, e, tol)
        acc = e.hc()
        q.reconstruct_hc(XY, k[XY[0]], k[XY[1]], out=acc, accumulate=True)
        q.reconstruct_hc(XY, k[XY[0]], k[XY[1]], out=acc, accumulate=True)
        _close(acc, 2 * ref, e, tol)
        assert float(acc[~band].abs().max()) == 0.0
    grid = q.pol_band_grid(ESTS)
    ref = q.reconstruct_mv_hc(k["T"], k["E"], k["B"], fused=False).clone()
    got = q.reconstruct_mv_hc(k["T"], k["E"], k["B"])
    assert q.pol_bound_grid == grid
    band = _band(e, *q._wK)
    _close(got, ref, e, tol)
    assert float(got[~band].abs().max()) == 0.0
    out = e.hc()
    out.fill_(7 + 7j)
    assert q.reconstruct_mv_hc(k["T"], k["E"], k["B"], out=out) is out
    assert float(out[~band].abs().max()) == 0.0
    _close(out, ref, e, tol)
    if case == "600x750":
        assert grid == (256, 512)
    if case == "1200":
        assert grid == (256, 256) and q.pol_band_grid("EB") == (256, 256)
    if case == "narrowP":                # the polarisation band is narrower than the TT binding's: another grid
        assert q.band_grid == (256, 512) and q.pol_band_grid("EB") == (256, 256) and grid == (256, 512)
    if case == "explicit":
        assert grid == (512, 512) and q.pol_band_grid("EB") == (512, 512)


_ORACLE = {}


def _oracle():
    """QEOracle at 1200^2 on the set-up of case "1200": EB, TE and the MV of five, computed once"""
    if not _ORACLE:
        from oracle import maps_oracle as mo
        s = _prepared("1200", "f64")[0]
        g = s["g"]
        mo.set_workers(16)
        qr = qo.QEOracle((1200, 1200), g.step_y, g.step_x, s["cl"], dict(T=s["nT"], P=s["nP"]), s["beam"], dict(T=s["tmask"], P=s["pmask"]),
                         kmask_K=s["kmask"])
        for XY in ("EB", "TE"):
            qr.setup(XY)
            _ORACLE[XY] = (qr.kappa_ft(XY, s["k"][XY[0]], s["k"][XY[1]]), qr.R[XY] != 0)
        _ORACLE["MV"] = (qr.kappa_mv_ft(s["k"], ESTS), True)
        mo.set_workers(1)
    return _ORACLE


@pytest.mark.parametrize("what", ["EB", "TE", "MV"])
def test_onecall_pol_on_band_grid_matches_oracle(what):
    """kappa_from_map("EB" / "TE", alreadyFTed) and reconstruct_mv_hc at 1200^2 (now one call on the 256^2 band grid) against
    oracle.QEOracle: float64 1e-8 on kappa_hat's DFT over the notebook-patch selection, float32 1e-5 on 19 bandpowers."""
    from orphics_amd import stats
    s, q, k = _prepared("1200", "f64")
    ml = s["ml"]
    kref, nz = _oracle()[what]
    sel = (ml > 40) & (ml < 2900) & nz
    binner = stats.bin2D(ml, np.linspace(20, 3000, 20))
    ref_b = binner.bin(np.abs(kref) ** 2)[1]
    for prec in ("f64", "f32"):
        s, q, k = _prepared("1200", prec)
        e = q.eng
        assert q.one_call_pol(ESTS if what == "MV" else what)
        if what == "MV":
            got = e.hc_to_full(q.reconstruct_mv_hc(k["T"], k["E"], k["B"])).cpu().numpy()
        else:
            got = q.kappa_from_map(what, T2DData=s["k"]["T"], E2DData=s["k"]["E"], B2DData=s["k"]["B"], alreadyFTed=True, returnFt=True)
        assert q.pol_bound_grid == (256, 256)
        got = np.asarray(got, dtype=np.complex128)
        if prec == "f64":
            err = np.abs(got - kref)[sel].max() / np.abs(kref[sel]).max()
            print("f64 max rel err", err)
            assert err < 1e-8
        else:
            err = np.max(np.abs(binner.bin(np.abs(got) ** 2)[1] / ref_b - 1))
            print("f32 bandpower err", err)
            assert err < 1e-5


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_onecall_pol_split_legs(prec):
    """EB with the B leg from ANOTHER map than the E leg (the SplitLensing contract: X and Y legs are different sources), and EE with
    two different E maps, against the modular chain."""
    import torch
    s, q, k = _prepared("600x750", prec)
    e = q.eng
    other = {X: torch.roll(k[X], shifts=3, dims=0) * (0.5 + 0.25j) for X in "EB"}
    for XY, kX, kY in (("EB", k["E"], other["B"]), ("EE", k["E"], other["E"]), ("EB", other["E"], k["B"])):
        ref = q._reconstruct_hc_modular(XY, kX, kY).clone()
        _close(q.reconstruct_hc(XY, kX, kY), ref, e, TOL[prec])
    assert q.pol_bound_grid == q.pol_band_grid("EB")


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_tt_and_pol_bindings_do_not_interfere(prec):
    """TT one-call, then the polarisation set bound and run on the same shared plan, then TT again: the TT results are bit-identical;
    the same in the reverse order for EB (with an MV call -- another binding of the same entry -- in between as well)."""
    import torch
    s, q, k = _prepared("narrowP", prec)
    e = q.eng
    tt0 = q.reconstruct_tt_hc(k["T"]).clone()
    grid_tt = q.band_grid
    eb0 = q.reconstruct_hc("EB", k["E"], k["B"]).clone()
    mv0 = q.reconstruct_mv_hc(k["T"], k["E"], k["B"]).clone()
    tt1 = q.reconstruct_tt_hc(k["T"]).clone()
    assert q.band_grid == grid_tt
    assert torch.equal(tt0, tt1)
    eb1 = q.reconstruct_hc("EB", k["E"], k["B"]).clone()
    tt2 = q.reconstruct_tt_hc(k["T"]).clone()
    eb2 = q.reconstruct_hc("EB", k["E"], k["B"]).clone()
    assert torch.equal(eb0, eb1) and torch.equal(eb1, eb2) and torch.equal(tt0, tt2)
    assert torch.equal(mv0, q.reconstruct_mv_hc(k["T"], k["E"], k["B"]))
    assert float(tt0.abs().max()) > 0 and float(eb0.abs().max()) > 0


def _raw_mv(q, XY, kX, kY, out, Fn=None, fgs=None, bands=None, mrow=None):
    """oa_qe_mv with one estimator through raw ctypes: (rc, message)"""
    from orphics_amd.engine import _ptr, _stream
    e = q.eng
    G = q._setup_general(XY)
    pcs = G["pieces"]
    n = len(pcs)
    wl, wk, rl, rk = bands if bands is not None else (G["wl"], G["wk"], G["rl"], G["rk"])
    one = ctypes.c_void_p * 1
    fg = [pc[1].data_ptr() for pc in pcs] if fgs is None else fgs
    rc = e.lib.oa_qe_mv(e.plan, 1, (ctypes.c_int * 1)(n), (ctypes.c_double * n)(*[float(pc[0]) for pc in pcs]), (ctypes.c_void_p * n)(*fg),
                        (ctypes.c_void_p * n)(*[pc[2].data_ptr() for pc in pcs]), (ctypes.c_int * n)(*[1 if pc[3] else 0 for pc in pcs]),
                        one(kX.data_ptr()), one(kY.data_ptr()), one((G["Fnorm"] if Fn is None else Fn).data_ptr()), _ptr(out), 0,
                        int(wl), int(wk), int(rl), int(rk), int(q.mrow if mrow is None else mrow), 1, _stream())
    return rc, e.lib.oa_last_error().decode()


def _raw_bind(q, XY, bands=None, mrow=None, mcol=None):
    e = q.eng
    G = q._setup_general(XY)
    planes = []
    for pc in G["pieces"]:
        for t in pc[1:3]:
            if t.data_ptr() not in planes:
                planes.append(t.data_ptr())
    wl, wk, rl, rk = bands if bands is not None else (G["wl"], G["wk"], G["rl"], G["rk"])
    e._pol_owner = None                    # the Python handle binds again on its next call
    rc = e.lib.oa_qe_band_bind(e.plan, len(planes), (ctypes.c_void_p * len(planes))(*planes), 1, (ctypes.c_void_p * 1)(G["Fnorm"].data_ptr()),
                               int(wl), int(wk), int(rl), int(rk), int(q.mrow if mrow is None else mrow), int(q.mcol if mcol is None else mcol), 0)
    return rc, e.lib.oa_last_error().decode()


def test_pol_band_grid_refusals():
    """Raw C-ABI: an unbound filter / normalisation pointer, band numbers other than the bound ones, unbounded filters, a band whose
    grid would not be smaller than the map, a chirp-z side -- each refused with a message naming the reason -- and the plan still
    serves a correct modular reconstruction afterwards."""
    from orphics_amd import lensing
    s, q, k = _prepared("600x750", "f64")
    e = q.eng
    G = q._setup_general("EB")
    ref = q._reconstruct_hc_modular("EB", k["E"], k["B"]).clone()
    out = e.hc()
    bands = (G["wl"], G["wk"], G["rl"], G["rk"])
    rc, msg = _raw_bind(q, "EB")
    assert rc == 0, msg
    rc, msg = _raw_mv(q, "EB", k["E"], k["B"], out)
    assert rc == 0, msg
    _close(out, ref, e, TOL["f64"])
    # a filter plane the binding has not seen (a copy of a bound one: same contents, another address)
    stranger = G["pieces"][0][1].clone()
    rc, msg = _raw_mv(q, "EB", k["E"], k["B"], out, fgs=[stranger.data_ptr()] + [pc[1].data_ptr() for pc in G["pieces"][1:]])
    assert rc != 0 and "not bound" in msg and "oa_qe_band_bind" in msg, msg
    rc, msg = _raw_mv(q, "EB", k["E"], k["B"], out, Fn=G["Fnorm"].clone())
    assert rc != 0 and "not bound" in msg and "oa_qe_band_bind" in msg, msg
    # band numbers other than the bound ones
    rc, msg = _raw_mv(q, "EB", k["E"], k["B"], out, bands=(bands[0] - 1,) + bands[1:])
    assert rc != 0 and "differ from the bound" in msg and "oa_qe_band_bind" in msg, msg
    # oa_qe_pol shares the checks
    pcs = G["pieces"]
    n = len(pcs)
    from orphics_amd.engine import _ptr, _stream
    rc = e.lib.oa_qe_pol(e.plan, n, (ctypes.c_double * n)(*[float(pc[0]) for pc in pcs]), (ctypes.c_void_p * n)(*[pc[1].data_ptr() for pc in pcs]),
                         (ctypes.c_void_p * n)(*[pc[2].data_ptr() for pc in pcs]), (ctypes.c_int * n)(*[1 if pc[3] else 0 for pc in pcs]),
                         _ptr(k["E"]), _ptr(k["B"]), _ptr(G["Fnorm"]), _ptr(out), 0, *[int(b) for b in bands], int(q.mrow), 1, _stream())
    assert rc == 0, e.lib.oa_last_error().decode()
    _close(out, ref, e, TOL["f64"])
    rc = e.lib.oa_qe_pol(e.plan, n, (ctypes.c_double * n)(*[float(pc[0]) for pc in pcs]), (ctypes.c_void_p * n)(*[pc[1].data_ptr() for pc in pcs]),
                         (ctypes.c_void_p * n)(*[pc[2].data_ptr() for pc in pcs]), (ctypes.c_int * n)(*[1 if pc[3] else 0 for pc in pcs]),
                         _ptr(k["E"]), _ptr(k["B"]), _ptr(G["Fnorm"]), _ptr(out), 0, int(bands[0]), int(bands[1]) + 1, int(bands[2]), int(bands[3]),
                         int(q.mrow), 1, _stream())
    assert rc != 0 and "oa_qe_band_bind" in e.lib.oa_last_error().decode()
    # unbounded filters (0 = all), the map's own grid: no band grid; nothing stays bound after a refused set-up
    rc, msg = _raw_bind(q, "EB", bands=(0, bands[1], bands[2], bands[3]))
    assert rc != 0 and "band-limited" in msg, msg
    rc, msg = _raw_mv(q, "EB", k["E"], k["B"], out)
    assert rc != 0 and "oa_qe_band_bind" in msg, msg
    rc, msg = _raw_bind(q, "EB", mrow=0)
    assert rc != 0 and "mrow = 0" in msg, msg
    # a grid that would alias
    rc, msg = _raw_bind(q, "EB", mrow=128)
    assert rc != 0 and "alias" in msg, msg
    # ... and the Python path is intact: binds again, one call, and the modular chain of the same plan
    _close(q.reconstruct_hc("EB", k["E"], k["B"]), ref, e, TOL["f64"])
    _close(q._reconstruct_hc_modular("EB", k["E"], k["B"]), ref, e, TOL["f64"])

    # a band too wide for its side: 480 x 600 at 2' (kappa to 3500 needs 512 columns of 600 -- but 512 rows of 480)
    for shape, res, words in (((480, 600), 2.0, ["band too wide", "512", "480"]), ((700, 700), 1.0, ["chirp-z"])):
        st = _setup(shape, res, 3500, None, seed=5)
        qw = lensing.qest(shape, st["g"], st["th"], dtype="f64", noise2d=st["nT"], beam2d=st["beam"], kmask=st["tmask"], noise2d_P=st["nP"],
                          kmask_P=st["pmask"], kmask_K=st["kmask"], pol=True, unlensed_equals_lensed=True)
        ew = qw.eng
        assert not ew.pow2 and ew.mixed == (shape != (700, 700))
        assert not qw.one_call_pol("EB") and not qw.one_call_pol(ESTS)
        rc, msg = _raw_bind(qw, "EB")
        assert rc != 0 and all(w in msg for w in words), msg
        kw_ = {X: ew.full_to_hc(ew.to_complex(st["k"][X])) for X in "EB"}
        refw = qw._reconstruct_hc_modular("EB", kw_["E"], kw_["B"]).clone()
        outw = ew.hc()
        rc, msg = _raw_mv(qw, "EB", kw_["E"], kw_["B"], outw)
        assert rc != 0 and ("oa_qe_band_bind" in msg or "chirp-z" in msg), msg
        _close(qw.reconstruct_hc("EB", kw_["E"], kw_["B"]), refw, ew, TOL["f64"])      # the modular chain, silently


def test_band_bind_leaves_power_of_two_plans_unchanged():
    """256^2: oa_qe_band_bind returns 0 and does nothing; reconstruct_mv_hc before and after it is bit-identical."""
    import torch
    from orphics_amd import lensing
    shape = (256, 256)
    st = _setup(shape, 2.0, 3000, None, seed=2)
    q = lensing.qest(shape, st["g"], st["th"], dtype="f64", noise2d=st["nT"], beam2d=st["beam"], kmask=st["tmask"], noise2d_P=st["nP"],
                     kmask_P=st["pmask"], kmask_K=st["kmask"], pol=True, unlensed_equals_lensed=True)
    e = q.eng
    assert e.pow2 and q.one_call_pol(ESTS) and q.pol_band_grid(ESTS) is None
    k = {X: e.full_to_hc(e.to_complex(st["k"][X])) for X in "TEB"}
    before = q.reconstruct_mv_hc(k["T"], k["E"], k["B"]).clone()
    eb = q.reconstruct_hc("EB", k["E"], k["B"]).clone()
    rc, msg = _raw_bind(q, "EB")
    assert rc == 0, msg
    assert q.pol_bound_grid == (0, 0)
    assert torch.equal(before, q.reconstruct_mv_hc(k["T"], k["E"], k["B"]))
    assert torch.equal(eb, q.reconstruct_hc("EB", k["E"], k["B"]))
    assert float(before.abs().max()) > 0
