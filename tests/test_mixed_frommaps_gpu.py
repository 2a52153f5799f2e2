"""GPU: the polarisation and MV estimators from REAL T, Q, U (or T, E, B) maps on map sides 2^a 3^b 5^c (``oa_qe_mv_maps``, include/orphics_amd.h;
``Estimator.reconstruct_from_maps`` / ``reconstruct_mv_from_maps``; the routing of ``kappa_from_map``).  The reference is always the
transform path of the SAME estimator object on the SAME real maps: ``Engine.rfft`` / ``FourierCalc(layout="half").iqu2teb(normalize=False)``,
then ``reconstruct_hc`` / ``reconstruct_mv_hc``.  Tolerances: those of the from-map TT entry against the rfft-fed chain
(tests/test_mixed_onecall_gpu.py), on max |kappa_hat|.

Shapes: 300 x 360 at 2' (300 = 4 3 5^2, N = 180 = 4 3^2 5: all four radices; legs 67 columns x 56 rows, kappa 117 x 98, inner grid
256 x 256) and 600 x 750 at 1' (kp = 391 odd, inner grid 256 x 512)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ESTS = ("TT", "TE", "EE", "EB", "TB")
TOL = {"f64": 1e-11, "f32": 2e-5}
CASES = {"300x360": ((300, 360), 2.0), "600x750": ((600, 750), 1.0)}


def _setup(shape, res, seed):
    """masks, spectra and real T, E, B, Q, U maps made from Hermitian transforms (E, B inverse-rotated, then ifft2(...).real); a second
    set of maps (index 1) for the Y legs of split calls"""
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    nP = 2 * nT
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    cl = {k: th.lCl(k, ml) for k in ("TT", "EE", "BB", "TE")}
    rng = np.random.default_rng(seed)
    sc = 1.0 / np.sqrt(g.pixarea)
    rot = maps.queb_rotmat(g.lmap())
    c, s = rot[0, 0], rot[1, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.nan_to_num(cl["TE"] / np.sqrt(cl["TT"] * cl["EE"]))
    real = {X: [] for X in "TEBQU"}
    for _ in range(2):
        w1, w2, w3 = (np.fft.fft2(rng.standard_normal(shape)) for _ in range(3))
        kT = w1 * np.sqrt(cl["TT"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nT) * sc
        kE = (r * w1 + np.sqrt(1 - r ** 2) * w2) * np.sqrt(cl["EE"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nP) * sc
        kB = w3 * np.sqrt(cl["BB"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nP) * sc
        for X, k in (("T", kT), ("E", kE), ("B", kB), ("Q", c * kE + s * kB), ("U", -s * kE + c * kB)):
            real[X].append(np.fft.ifft2(k).real)
    return dict(g=g, th=th, beam=beam, nT=nT, nP=nP, tmask=tmask, kmask=kmask, real=real)


def _qest(s, shape, prec="f64"):
    from orphics_amd import lensing
    return lensing.qest(shape, s["g"], s["th"], dtype=prec, noise2d=s["nT"], beam2d=s["beam"], kmask=s["tmask"], noise2d_P=s["nP"],
                        kmask_P=s["tmask"], kmask_K=s["kmask"], pol=True, unlensed_equals_lensed=True)


_SET = {}
_Q = {}


def _prepared(case, prec):
    """(set-up, estimator, device maps {field: [map, second map]}, reference transforms {field: [hc, hc of the second map]}); the
    transforms E, B come from the E, B maps, "Eq" / "Bq" from the rotated Q, U maps.  Computed once per (case, precision)."""
    import torch
    from orphics_amd import maps
    shape, res = CASES[case]
    if case not in _SET:
        s = _setup(shape, res, seed=sum(shape))
        s["q"] = _qest(s, shape)
        s["q"].mv_weights(ESTS)
        _SET[case] = s
    s = _SET[case]
    if (case, prec) not in _Q:
        q = s["q"] if prec == "f64" else s["q"].astype("f32")
        e = q.eng
        m = {X: [e.to_real(a) for a in s["real"][X]] for X in "TEBQU"}
        k = {X: [e.rfft(a) for a in m[X]] for X in "TEB"}
        fc = maps.FourierCalc((3,) + shape, s["g"], layout="half")
        k["Eq"], k["Bq"] = [], []
        for i in range(2):
            teb = fc.iqu2teb(torch.stack([m["T"][i], m["Q"][i], m["U"][i]]), normalize=False).t
            k["Eq"].append(teb[1].contiguous())
            k["Bq"].append(teb[2].contiguous())
        _Q[(case, prec)] = (q, m, k)
    return (s,) + _Q[(case, prec)]


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
    assert s > 0 and d <= tol * s


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_mv_and_single_estimators_from_maps_equal_transform_path(case, prec):
    import torch
    s, q, m, k = _prepared(case, prec)
    e = q.eng
    tol = TOL[prec]
    shape = CASES[case][0]
    grid = q.pol_band_grid(ESTS)
    assert e.mixed and q.one_call_pol(ESTS) and grid[0] < shape[0] and grid[1] < shape[1]
    assert grid == ((256, 256) if case == "300x360" else (256, 512))
    band = _band(e, q._support_cols(q.mask_K), q._support_rows(q.mask_K))
    for maps3, kw, ref3 in (((m["T"][0], m["Q"][0], m["U"][0]), dict(qu=True), (k["T"][0], k["Eq"][0], k["Bq"][0])),
                            ((m["T"][0], m["E"][0], m["B"][0]), {}, (k["T"][0], k["E"][0], k["B"][0]))):
        ref = q.reconstruct_mv_hc(*ref3).clone()
        got = q.reconstruct_mv_from_maps(*maps3, **kw)
        assert q.pol_bound_grid == grid
        _close(got, ref, e, tol)
        assert float(got[~band].abs().max()) == 0.0
        out = e.hc()
        out.fill_(7 + 7j)
        assert q.reconstruct_mv_from_maps(*maps3, out=out, **kw) is out
        assert float(out[~band].abs().max()) == 0.0
        assert torch.equal(out, got)                          # two identical calls, bit for bit
    if case == "300x360":                  # the band numbers the shapes were chosen for
        assert (q._mv[2]["wl"], q._mv[2]["rl"]) == (67, 56) and tuple(q._wK) == (117, 98)
    for XY in ("EB", "TE", "EE"):
        G = q._setup_general(XY)
        bxy = _band(e, G["wk"], G["rk"])
        ref = q.reconstruct_hc(XY, k[XY[0]][0], k[XY[1]][0]).clone()
        got = q.reconstruct_from_maps(XY, m[XY[0]][0], m[XY[1]][0])
        assert q.pol_bound_grid == q.pol_band_grid(XY)
        _close(got, ref, e, tol)
        assert float(got[~bxy].abs().max()) == 0.0
        out = e.hc()
        out.fill_(7 + 7j)
        assert q.reconstruct_from_maps(XY, m[XY[0]][0], m[XY[1]][0], out=out) is out
        assert float(out[~bxy].abs().max()) == 0.0
        assert torch.equal(out, got)
        acc = e.hc()
        q.reconstruct_from_maps(XY, m[XY[0]][0], m[XY[1]][0], out=acc, accumulate=True)
        q.reconstruct_from_maps(XY, m[XY[0]][0], m[XY[1]][0], out=acc, accumulate=True)
        _close(acc, 2 * ref, e, tol)
        assert float(acc[~bxy].abs().max()) == 0.0


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_split_legs_from_maps(case, prec):
    """the Y leg from ANOTHER map than the X leg: two maps of E / B, and six maps (two (T, Q, U) triples: both rotated pairs)"""
    s, q, m, k = _prepared(case, prec)
    e = q.eng
    for XY, y in (("EB", "B"), ("EE", "E")):
        ref = q.reconstruct_hc(XY, k["E"][0], k[y][1]).clone()
        _close(q.reconstruct_from_maps(XY, m["E"][0], m[y][1]), ref, e, TOL[prec])
        ref = q.reconstruct_hc(XY, k["Eq"][0], k[y + "q"][1]).clone()
        got = q.reconstruct_from_maps(XY, (m["T"][0], m["Q"][0], m["U"][0]), (m["T"][1], m["Q"][1], m["U"][1]), qu=True)
        _close(got, ref, e, TOL[prec])
    # one triple, both legs from it: three maps
    ref = q.reconstruct_hc("EB", k["Eq"][1], k["Bq"][1]).clone()
    _close(q.reconstruct_from_maps("EB", (m["T"][1], m["Q"][1], m["U"][1]), qu=True), ref, e, TOL[prec])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kappa_from_map_takes_the_from_maps_path(prec, monkeypatch):
    """real NumPy maps into kappa_from_map("EB"): no full transform is run (Engine.rfft raises), and the result is that of the
    alreadyFTed call fed with np.fft.fft2 of the same maps; returnFt=False is the inverse transform of it"""
    s, q, m, k = _prepared("300x360", prec)
    e = q.eng
    rdt = np.float64 if prec == "f64" else np.float32
    T, E, B = (s["real"][X][0].astype(rdt) for X in "TEB")
    ref = q.kappa_from_map("EB", *(np.fft.fft2(a.astype(np.float64)) for a in (T, E, B)), alreadyFTed=True, returnFt=True)

    def boom(*a, **kw):
        raise AssertionError("Engine.rfft called: a full N-grid transform on the from-maps path")
    with monkeypatch.context() as mp:
        mp.setattr(e, "rfft", boom)
        got = q.kappa_from_map("EB", T, E, B, returnFt=True)
    assert isinstance(got, np.ndarray) and got.shape == (300, 360) and np.iscomplexobj(got)
    d, sc = np.abs(got - ref).max(), np.abs(ref).max()
    print("kappa_from_map EB %s: max |diff| / max |ref| = %.3e" % (prec, d / sc))
    assert sc > 0 and d <= TOL[prec] * sc
    rec = q.kappa_from_map("EB", T, E, B, returnFt=False)
    want = e.irfft(e.full_to_hc(e.to_complex(got))).cpu().numpy()
    assert isinstance(rec, np.ndarray) and rec.shape == (300, 360) and not np.iscomplexobj(rec)
    assert np.abs(rec - want).max() <= TOL[prec] * np.abs(want).max()
    # a different Y-leg map is a second source
    with monkeypatch.context() as mp:
        mp.setattr(e, "rfft", boom)
        got2 = q.kappa_from_map("EB", T, E, B, B2DDataY=s["real"]["B"][1].astype(rdt), returnFt=True)
    ref2 = e.hc_to_full(q.reconstruct_hc("EB", k["E"][0], k["B"][1])).cpu().numpy()
    assert np.abs(got2 - ref2).max() <= TOL[prec] * np.abs(ref2).max()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bindings_and_pools(prec, monkeypatch):
    """a from-maps call reuses the binding of the from-transforms call of the same set; a TT one-call before and after is bit-identical;
    after release_pools the next from-maps call returns the same bits"""
    import torch
    s, q, m, k = _prepared("300x360", prec)
    e = q.eng
    calls = []
    real_bind = e.lib.oa_qe_band_bind

    def counting(*a):
        calls.append(1)
        return real_bind(*a)
    tqu = (m["T"][0], m["Q"][0], m["U"][0])
    tt0 = q.reconstruct_tt_from_map(m["T"][0]).clone()
    with monkeypatch.context() as mp:
        mp.setattr(e.lib, "oa_qe_band_bind", counting)
        e._pol_owner = None
        q.reconstruct_mv_hc(k["T"][0], k["Eq"][0], k["Bq"][0])
        assert len(calls) == 1
        mv0 = q.reconstruct_mv_from_maps(*tqu, qu=True).clone()
        assert len(calls) == 1
        q.reconstruct_hc("EB", k["E"][0], k["B"][0])
        assert len(calls) == 2
        eb0 = q.reconstruct_from_maps("EB", m["E"][0], m["B"][0]).clone()
        assert len(calls) == 2
    tt1 = q.reconstruct_tt_from_map(m["T"][0]).clone()
    assert torch.equal(tt0, tt1) and float(tt0.abs().max()) > 0
    assert torch.equal(eb0, q.reconstruct_from_maps("EB", m["E"][0], m["B"][0]))
    assert torch.equal(mv0, q.reconstruct_mv_from_maps(*tqu, qu=True))
    e.release_pools()
    assert torch.equal(mv0, q.reconstruct_mv_from_maps(*tqu, qu=True))
    assert torch.equal(tt0, q.reconstruct_tt_from_map(m["T"][0]))


def _raw_maps(e, q, XY, maps, out, rot=(None, None), src=(0, 1), fgs=None, Fn=None, bands=None, mrow=None, nmaps=None):
    """oa_qe_mv_maps with one estimator through raw ctypes on the plan of engine ``e``: (rc, message)"""
    from orphics_amd.engine import _ptr, _stream
    G = q._setup_general(XY)
    pcs = G["pieces"]
    n = len(pcs)
    wl, wk, rl, rk = bands if bands is not None else (G["wl"], G["wk"], G["rl"], G["rk"])
    one = ctypes.c_void_p * 1
    fg = [pc[1].data_ptr() for pc in pcs] if fgs is None else fgs
    ptrs = [None if t is None else t.data_ptr() for t in maps]
    rc = e.lib.oa_qe_mv_maps(e.plan, len(maps) if nmaps is None else nmaps, (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs),
                             None if rot[0] is None else _ptr(rot[0]), None if rot[1] is None else _ptr(rot[1]), 1, (ctypes.c_int * 1)(n),
                             (ctypes.c_double * n)(*[float(pc[0]) for pc in pcs]), (ctypes.c_void_p * n)(*fg),
                             (ctypes.c_void_p * n)(*[pc[2].data_ptr() for pc in pcs]), (ctypes.c_int * n)(*[1 if pc[3] else 0 for pc in pcs]),
                             (ctypes.c_int * 1)(src[0]), (ctypes.c_int * 1)(src[1]), one((G["Fnorm"] if Fn is None else Fn).data_ptr()), _ptr(out), 0,
                             int(wl), int(wk), int(rl), int(rk), int(q.mrow if mrow is None else mrow), 1, _stream())
    return rc, e.lib.oa_last_error().decode()


def _raw_bind(e, q, XY, bands=None, max_leg_planes=0):
    G = q._setup_general(XY)
    planes = []
    for pc in G["pieces"]:
        for t in pc[1:3]:
            if t.data_ptr() not in planes:
                planes.append(t.data_ptr())
    wl, wk, rl, rk = bands if bands is not None else (G["wl"], G["wk"], G["rl"], G["rk"])
    e._pol_owner = None                    # a Python handle binds again on its next call
    rc = e.lib.oa_qe_band_bind(e.plan, len(planes), (ctypes.c_void_p * len(planes))(*planes), 1, (ctypes.c_void_p * 1)(G["Fnorm"].data_ptr()),
                               int(wl), int(wk), int(rl), int(rk), int(q.mrow), int(q.mcol), int(max_leg_planes))
    return rc, e.lib.oa_last_error().decode()


def test_raw_entry_refusals_leave_the_output_untouched():
    """every refusal of include/orphics_amd.h: non-zero, the named words in oa_last_error, nothing written -- and the entry still serves
    a correct call afterwards"""
    import torch
    from orphics_amd.engine import Engine
    s, q, m, k = _prepared("300x360", "f64")
    G = q._setup_general("EB")
    bands = (G["wl"], G["wk"], G["rl"], G["rk"])
    ref = q.reconstruct_hc("EB", k["E"][0], k["B"][0]).clone()
    e = Engine(300, 360, "f64")            # a plan of its own (not the shared one): nothing bound, its pools never grown
    ly, lx = s["g"].laxes()
    e.set_laxes(ly, lx)
    out = e.hc()
    out.fill_(7 + 7j)
    keep = out.clone()
    EB = [m["E"][0], m["B"][0]]
    TQU = [m["T"][0], m["Q"][0], m["U"][0]]
    c, sn = q._qu_rot(False)

    def refused(words, *a, **kw):
        rc, msg = _raw_maps(e, q, "EB", *a, **kw)
        assert rc != 0 and all(w in msg for w in words), msg
        torch.cuda.synchronize()
        assert torch.equal(out, keep)
    refused(["oa_qe_band_bind"], EB, out)                                                     # no binding
    rc, msg = _raw_bind(e, q, "EB", max_leg_planes=1)
    assert rc == 0, msg
    refused(["leg planes", "oa_qe_band_bind"], EB, out)                                       # more leg planes than the binding was told
    rc, msg = _raw_bind(e, q, "EB")
    assert rc == 0, msg
    refused(["differ from the bound", "oa_qe_band_bind"], EB, out, bands=(bands[0] - 1,) + bands[1:])
    refused(["differ from the bound", "oa_qe_band_bind"], EB, out, mrow=512)
    stranger = G["pieces"][0][1].clone()
    refused(["not bound", "oa_qe_band_bind"], EB, out, fgs=[stranger.data_ptr()] + [pc[1].data_ptr() for pc in G["pieces"][1:]])
    refused(["not bound", "oa_qe_band_bind"], EB, out, Fn=G["Fnorm"].clone())
    refused(["nmaps"], EB, out, nmaps=0)
    refused(["nmaps"], EB + TQU + TQU, out, nmaps=7)
    refused(["NULL map"], [m["E"][0], None], out)
    refused(["rot_c and rot_s"], TQU, out, rot=(c, None), src=(1, 2))
    refused(["rot_c and rot_s"], TQU, out, rot=(None, sn), src=(1, 2))
    refused(["rotation planes", "nmaps = 3"], EB, out, rot=(c, sn))
    refused(["source index"], EB, out, src=(0, 2))
    refused(["source index"], EB, out, src=(-1, 1))
    # ... and serves the call: two maps, and T, Q, U with the rotation
    rc, msg = _raw_maps(e, q, "EB", EB, out)
    assert rc == 0, msg
    _close(out, ref, e, TOL["f64"])
    rc, msg = _raw_maps(e, q, "EB", TQU, out, rot=(c, sn), src=(1, 2))
    assert rc == 0, msg
    _close(out, q.reconstruct_hc("EB", k["Eq"][0], k["Bq"][0]), e, TOL["f64"])
    # a chirp-z plan (140 = 4 5 7) and a power-of-two plan: refused whatever the planes are
    out.fill_(7 + 7j)
    for shape, words in (((140, 140), ["chirp-z"]), ((256, 256), ["oa_fft_r2c", "oa_rot2", "oa_qe_mv"])):
        e2 = Engine.get(shape[0], shape[1], "f64")
        rc, msg = _raw_maps(e2, q, "EB", EB, out)
        assert rc != 0 and all(w in msg for w in words), msg
        torch.cuda.synchronize()
        assert torch.equal(out, keep)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape,res", [((256, 256), 2.0), ((480, 600), 2.0)], ids=["256", "480x600"])
def test_fallback_where_there_is_no_band_grid(shape, res, prec):
    """a power-of-two plan, and 480 x 600 at 2' (the band grid would need 512 rows of 480): the methods are the composition
    rfft per map + rot2 + the from-transforms method"""
    import torch
    from orphics_amd import maps
    s = _setup(shape, res, seed=7)
    q = _qest(s, shape, prec)
    e = q.eng
    assert (e.pow2 or e.mixed) and q.pol_band_grid(ESTS) is None
    T, Q, U, E, B = (e.to_real(s["real"][X][0]) for X in "TQUEB")
    teb = maps.FourierCalc((3,) + shape, s["g"], layout="half").iqu2teb(torch.stack([T, Q, U]), normalize=False).t
    ref = q.reconstruct_mv_hc(teb[0].contiguous(), teb[1].contiguous(), teb[2].contiguous()).clone()
    _close(q.reconstruct_mv_from_maps(T, Q, U, qu=True), ref, e, TOL[prec])
    ref = q.reconstruct_hc("EB", e.rfft(E), e.rfft(B)).clone()
    _close(q.reconstruct_from_maps("EB", E, B), ref, e, TOL[prec])
