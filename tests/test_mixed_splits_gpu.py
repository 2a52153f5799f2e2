"""GPU: the split-based TT cross estimator in one call on map sides 2^a 3^b 5^c (BAND GRID; include/orphics_amd.h oa_qe_tt_splits /
oa_qe_tt_split_power): Estimator.tt_pairs against pairwise one-call reconstructions, SplitLensing.cross_estimator's device path
against the NumPy oracle and against the generic pairwise loop of the same plan, and the raw C entry.  (600, 750) at 1' is the smallest
band-grid geometry: its band wraps the negative ky rows onto 600 rows on the map and 256 on the inner grid."""
import ctypes

import numpy as np
import pytest

from oracle import maps_oracle as mo
from oracle import qe_oracle as qo

pytestmark = pytest.mark.gpu

SHAPE, RES = (600, 750), 1.0


def _setup(shape, res, seed):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    cl = th.lCl("TT", ml)
    rng = np.random.default_rng(seed)
    tk = np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cl * beam ** 2 + noise) / g.pixarea)
    tmap = np.fft.ifft2(tk).real
    split_maps = [tmap + 0.3 * rng.standard_normal(shape) for _ in range(6)]      # one map + 0.3 x white noise per split
    return dict(g=g, th=th, cl=cl, beam=beam, noise=noise, tmask=tmask, kmask=kmask, maps=split_maps)


_GEOM = {}
_ORACLE = {}


def _prepared(prec, shape=SHAPE, res=RES):
    """the geometry's fixtures and its estimator of this precision (made once per module)"""
    from orphics_amd import lensing
    key = (shape, res)
    if key not in _GEOM:
        s = _setup(shape, res, seed=shape[0] + shape[1])
        s["f64"] = lensing.qest(shape, s["g"], s["th"], noise2d=s["noise"], beam2d=s["beam"], kmask=s["tmask"], kmask_K=s["kmask"],
                                unlensed_equals_lensed=True, dtype="f64")
        _GEOM[key] = s
    s = _GEOM[key]
    if prec not in s:
        s[prec] = s["f64"].astype(prec)
    return s, s[prec]


def _oracle_cross(n):
    """the reference's ordering of the estimator with the NumPy oracle QE on the first n splits (computed once, never modified)"""
    if n not in _ORACLE:
        s, _ = _prepared("f64")
        g = s["g"]
        qr = qo.QEOracleTT(SHAPE, g.step_y, g.step_x, s["cl"], s["cl"], s["noise"], s["beam"], s["tmask"], kmask_K=s["kmask"])
        fo = mo.FourierCalc(SHAPE, g.step_y, g.step_x)
        splits = np.array([np.fft.fft2(m) for m in s["maps"][:n]])
        ref = qo.split_cross_estimator(lambda a, b: qr.kappa_from_map("TT", a, T2DDataY=b, alreadyFTed=True, returnFt=True), fo.f2power, splits)
        ref.setflags(write=False)
        splits.setflags(write=False)
        _ORACLE[n] = (splits, ref)
    return _ORACLE[n]


def _band_mask(q):
    """(Ny, kp) True on kappa's band: columns < kappa_cols, rows |ky| < kappa_rows"""
    e = q.eng
    ky = np.fft.fftfreq(e.ny, 1.0 / e.ny)
    m = np.zeros((e.ny, e.kp), dtype=bool)
    m[np.abs(ky) < q.kappa_rows, :q.kappa_cols] = True
    return m


class _DuckQest(object):
    """any object with kappa_from_map is a valid qest for SplitLensing: forces the generic pairwise loop"""

    def __init__(self, fn):
        self.fn = fn
        self.calls = 0

    def kappa_from_map(self, XY, T2DData=None, T2DDataY=None, alreadyFTed=False, returnFt=False, **unused):
        assert XY == "TT" and alreadyFTed and returnFt
        self.calls += 1
        return self.fn(T2DData, T2DDataY)


def _generic(shape, g, q, half):
    from orphics_amd import lensing
    duck = _DuckQest(lambda a, b: q.kappa_from_map("TT", T2DData=a, T2DDataY=b, alreadyFTed=True, returnFt=True))
    gen = lensing.SplitLensing(shape, g, duck, "TT").cross_estimator(half)
    assert duck.calls == half.t.shape[0] ** 2
    return gen


@pytest.mark.parametrize("prec,tol", [("f64", 1e-11), ("f32", 2e-5)])
def test_tt_pairs_on_band_grid_equals_pairwise_calls(prec, tol):
    """oa_qe_tt_splits on a band-grid plan: K[i, j] equals the one-call two-leg reconstruction of the same plan (the tolerances of
    one-call against modular in test_mixed_onecall_gpu), a dirty caller block comes back zero outside kappa's band, an owned one is
    not written there, and calls with fewer / more splits reuse / regrow the plan's buffers."""
    import torch
    s, q = _prepared(prec)
    e = q.eng
    assert e.mixed and q.one_call() and q.band_grid == (256, 512)
    hcs = [e.rfft(e.to_real(m)) for m in s["maps"]]
    band = torch.as_tensor(_band_mask(q), device=e.device)
    n = 5
    K = q.tt_pairs(hcs[:n])
    assert tuple(K.shape) == (n, n, e.ny, e.kp)

    def check_pairs(Kn, pairs):
        for i, j in pairs:
            one = q.reconstruct_tt_hc(hcs[i], hcs[j]).clone()
            scale = float(one.abs().max())
            assert scale > 0
            err = float((Kn[i, j] - one).abs().max())
            print("tt_pairs %s n=%d pair (%d, %d): max |K - one| / max |one| = %.3g" % (prec, Kn.shape[0], i, j, err / scale))
            assert err <= tol * scale

    check_pairs(K, ((0, 0), (1, 3), (4, 2)))                   # a diagonal, an upper and a lower pair
    assert float(K[:, :, ~band].abs().max()) == 0.0
    # a dirty caller block: zero-filled outside the band in the scatter launch, the band equal
    buf = torch.full_like(K, 7 + 7j)
    got = q.tt_pairs(hcs[:n], out=buf)
    assert got is buf
    assert float(buf[:, :, ~band].abs().max()) == 0.0
    assert torch.equal(buf, K)
    # an owned block: nothing is written out of band
    own = torch.full_like(K, 7 + 7j)
    q.tt_pairs(hcs[:n], out=own, owned=True)
    assert bool((own[:, :, ~band] == (7 + 7j)).all())
    assert torch.equal(own[:, :, band], K[:, :, band])
    # fewer splits after more (buffers reused), then more than ever before (buffers regrown)
    K4 = q.tt_pairs(hcs[:4])
    assert torch.equal(K4, K[:4, :4])
    check_pairs(K4, ((3, 1),))
    K6 = q.tt_pairs(hcs[:6])
    assert torch.equal(K6[:n, :n], K)
    check_pairs(K6, ((5, 0), (2, 5)))
    e.release_pools()


def test_cross_estimator_band_path_matches_oracle():
    """SplitLensing.cross_estimator on the band grid (one oa_qe_tt_split_power call) against the reference's ordering of the estimator
    evaluated with the NumPy oracle QE, f64, n = 4 and 5: 1e-8 of the reference's maximum (the bound of
    test_split_lensing_cross_estimator_matches_numpy); the estimator's kappa_from_map is never called."""
    from orphics_amd import lensing
    s, q = _prepared("f64")
    calls = []
    orig = q.kappa_from_map
    q.kappa_from_map = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        for n in (4, 5):
            splits, ref = _oracle_cross(n)
            got = lensing.SplitLensing(SHAPE, s["g"], q, "TT").cross_estimator(splits)
            assert isinstance(got, np.ndarray) and got.shape == SHAPE
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print("cross_estimator f64 n=%d vs oracle: %.3g" % (n, err))
            assert err < 1e-8
    finally:
        del q.kappa_from_map
    assert not calls                                           # the device path was taken


@pytest.mark.parametrize("prec,tol", [("f64", 1e-9), ("f32", 2e-3)])
def test_cross_estimator_band_path_equals_generic_loop(prec, tol):
    """Device path against the generic pairwise loop of the same plan (n^2 kappa_from_map calls + host combination), HalfPlane in and
    out, n = 5: the bounds of test_split_device_path_equals_pairwise_calls.  In f32 the device path may not be further from the f64
    oracle result than twice what the generic path is (the estimator cancels heavily: the yardstick is the existing code)."""
    import torch
    from orphics_amd import lensing
    from orphics_amd.stats import HalfPlane
    s, q = _prepared(prec)
    e = q.eng
    n = 5
    half = HalfPlane(torch.stack([e.rfft(e.to_real(m)) for m in s["maps"][:n]]), e)
    dev = lensing.SplitLensing(SHAPE, s["g"], q, "TT").cross_estimator(half)
    assert isinstance(dev, HalfPlane) and tuple(dev.t.shape) == (e.ny, e.kp) and dev.t.dtype == e.rdt
    gen = _generic(SHAPE, s["g"], q, half)
    w = e.nxh + 1
    a, b = dev.t.double()[:, :w], gen.t.double()[:, :w]
    err = float((a - b).abs().max() / b.abs().max())
    print("cross_estimator %s device vs generic: %.3g" % (prec, err))
    assert err < tol
    band = torch.as_tensor(_band_mask(q), device=e.device)
    assert float(dev.t[~band].abs().max()) == 0.0
    if prec == "f32":
        ref = torch.as_tensor(np.array(_oracle_cross(n)[1][:, :w]), device=e.device)
        scale = float(ref.abs().max())
        dev_err, gen_err = float((a - ref).abs().max()) / scale, float((b - ref).abs().max()) / scale
        print("cross_estimator f32 vs f64 oracle: device %.3g, generic %.3g" % (dev_err, gen_err))
        assert dev_err <= 2.0 * gen_err


class _Dev(object):
    """device buffers through the library's own allocator (no torch involved)"""

    def __init__(self, lib, check):
        self.lib, self.check, self.ptrs = lib, check, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        self.check(self.lib.oa_malloc(ctypes.byref(p), a.nbytes))
        self.check(self.lib.oa_memcpy(p, a.ctypes.data_as(ctypes.c_void_p), a.nbytes, 1, None))
        self.ptrs.append(p)
        return p

    def down(self, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self.check(self.lib.oa_memcpy(out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes, 2, None))
        self.check(self.lib.oa_stream_synchronize(None))
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.oa_free(p)


def test_split_power_entry_from_raw_pointers():
    """oa_qe_tt_split_power driven with oa_malloc'ed pointers, n = 4, f64: zero_outside = 1 into a garbage plane equals the Python
    path; 3 and 9 splits are refused before anything is launched; a power-of-two plan refuses, naming the two calls that serve it."""
    import torch
    from orphics_amd import _lib, lensing
    from orphics_amd._lib import check
    from orphics_amd.stats import HalfPlane
    lib = _lib.load()
    s, q = _prepared("f64")
    e = q.eng
    n = 4
    hcs = [e.rfft(e.to_real(m)) for m in s["maps"][:n]]
    sl = lensing.SplitLensing(SHAPE, s["g"], q, "TT")
    want = sl.cross_estimator(HalfPlane(torch.stack(hcs), e)).t.cpu().numpy()
    ny, nx = SHAPE
    dev = _Dev(lib, check)
    plan, plan2 = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        check(lib.oa_plan_create(ny, nx, _lib.OA_F64, ctypes.byref(plan)))
        ly, lx = s["g"].laxes()
        check(lib.oa_plan_set_laxes(plan, ly.ctypes.data_as(ctypes.c_void_p), lx.ctypes.data_as(ctypes.c_void_p)))
        d_k = [dev.up(k.cpu().numpy()) for k in hcs]
        ins = (ctypes.c_void_p * 9)(*([p.value for p in d_k] * 3)[:9])
        garbage = np.full((ny, e.kp), 7.0)
        d_out = dev.up(garbage)
        norm = float(sl.fc.normfact)
        assert lib.oa_qe_tt_split_power(plan, n, ins, d_out, norm, 1, None) != 0 and b"oa_plan_set_filters" in lib.oa_last_error()
        FG, FH, Fn = [dev.up(t.cpu().numpy()) for t in q._F["TT"]]
        check(lib.oa_plan_set_filters(plan, FG, FH, Fn, q.leg_cols, q.kappa_cols, q.leg_rows, q.kappa_rows, -1))
        for bad in (3, 9):
            assert lib.oa_qe_tt_split_power(plan, bad, ins, d_out, norm, 1, None) != 0
            assert b"4 <= nsplits <= 8" in lib.oa_last_error()
        assert np.array_equal(dev.down(d_out, (ny, e.kp), np.float64), garbage)          # nothing was launched
        check(lib.oa_qe_tt_split_power(plan, n, ins, d_out, norm, 1, None))
        got = dev.down(d_out, (ny, e.kp), np.float64)
        assert np.all(got[~_band_mask(q)] == 0.0)
        assert np.abs(want).max() > 0 and np.array_equal(got, want)                     # same kernels' arithmetic on the same inputs
        # zero_outside = 0 writes kappa's band only
        check(lib.oa_memcpy(d_out, garbage.ctypes.data_as(ctypes.c_void_p), garbage.nbytes, 1, None))
        check(lib.oa_qe_tt_split_power(plan, n, ins, d_out, norm, 0, None))
        got0 = dev.down(d_out, (ny, e.kp), np.float64)
        assert np.all(got0[~_band_mask(q)] == 7.0) and np.array_equal(got0[_band_mask(q)], want[_band_mask(q)])
        check(lib.oa_plan_release_pools(plan))
        # a power-of-two plan has no inner grid: refused with the documented message
        check(lib.oa_plan_create(128, 128, _lib.OA_F64, ctypes.byref(plan2)))
        assert lib.oa_qe_tt_split_power(plan2, n, ins, d_out, norm, 1, None) != 0
        msg = lib.oa_last_error()
        assert b"oa_qe_tt_splits" in msg and b"oa_split_cross_power" in msg
    finally:
        for p in (plan, plan2):
            if p.value:
                lib.oa_plan_destroy(p)
        dev.free()


def test_cross_estimator_band_path_at_1200():
    """The notebook's own geometry, 1200^2 at 0.5', f32, n = 4: device path against the generic loop of the same plan."""
    import torch
    from orphics_amd import lensing
    from orphics_amd.stats import HalfPlane
    shape, res = (1200, 1200), 0.5
    s, q = _prepared("f32", shape, res)
    e = q.eng
    assert e.mixed and q.one_call() and q.band_grid == (256, 256)
    n = 4
    half = HalfPlane(torch.stack([e.rfft(e.to_real(m)) for m in s["maps"][:n]]), e)
    dev = lensing.SplitLensing(shape, s["g"], q, "TT").cross_estimator(half)
    gen = _generic(shape, s["g"], q, half)
    w = e.nxh + 1
    a, b = dev.t.double()[:, :w], gen.t.double()[:, :w]
    err = float((a - b).abs().max() / b.abs().max())
    print("cross_estimator f32 1200^2 device vs generic: %.3g" % err)
    assert err < 2e-3
    e.release_pools()
    _GEOM.pop((shape, res), None)
