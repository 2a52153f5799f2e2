"""GPU: the realisation-dependent N0 of the TT estimator -- ``oa_rdn0_set_data`` + ``oa_mc_run_rdn0`` behind ``mc.RDN0MonteCarlo`` --
against the host loop of existing entries (``one_call=False``) and against the definition stated in NumPy with the oracle estimator.

Geometries: 512^2 at 2' (the row stage takes one map per launch: one-by-one path), 2048^2 at 1' (batched path) -- the two power-of-two
cases of test_mc_run_in_batches_equals_one_by_one -- and (600, 750) at 1' (band grid).  7 realisations = 6 + 1 at batch 6, 3 + 3 + 1 at 3.

Tolerance of one-call against host loop: 1e-10 (f64), 4e-5 (f32) of the scale max_b p(A)_b -- not of rdn0 itself, which is a difference of
two terms; 2e-5 per |kappa_hat|^2 bandpower is the f32 bound of one-call against modular (test_mixed_onecall_gpu.py), two terms double it."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GEOMS = {"p512": ((512, 512), 2.0), "p2048": ((2048, 2048), 1.0), "band": ((600, 750), 1.0)}
TOL = {"f64": 1e-10, "f32": 4e-5}
EDGES = np.linspace(20, 3500, 20)
NSIMS = 7
_CACHE = {}


def _inputs(shape, res):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    return g, th, ml, beam, noise, tmask, kmask


def _est(geom, prec):
    """(estimator, total power on the half plane) of a geometry: set up once in f64, converted for f32"""
    from orphics_amd import lensing
    if (geom, "f64") not in _CACHE:
        shape, res = GEOMS[geom]
        g, th, ml, beam, noise, tmask, kmask = _inputs(shape, res)
        q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f64")
        _CACHE[(geom, "f64")] = (q, (th.lCl("TT", ml) * beam ** 2 + noise)[:, :shape[1] // 2 + 1])
    if (geom, prec) not in _CACHE:
        q64, tot = _CACHE[(geom, "f64")]
        _CACHE[(geom, prec)] = (q64.astype(prec), tot)
    return _CACHE[(geom, prec)]


def _driver(geom, prec, one_call, data_seed=17, scale=1.0, edges=EDGES):
    """a driver whose data is the Gaussian draw e.grf_hc(data_seed, 10**6, cs) times `scale` (scale = 0: zero data)"""
    from orphics_amd import mc
    q, tot = _est(geom, prec)
    drv = mc.RDN0MonteCarlo(q, q.eng.hc(), tot, edges, comm=None, base_seed=31, one_call=one_call)
    if scale:
        drv.set_data(q.eng.grf_hc(data_seed, 10 ** 6, drv.cs) * scale)
    return drv


def _moments(drv):
    st = drv.acc
    st.allreduce()
    return st.count("rdn0"), np.array(st.mean("rdn0")), np.array(st.cov("rdn0"))


def _raw(drv):
    n, S, C = drv.acc.device_moments("rdn0", 2 * drv.d)
    torch.cuda.synchronize()
    return int(n[0]), S.cpu().numpy().copy(), C.cpu().numpy().copy()


class Dev(object):
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

    def zeros(self, nbytes):
        p = ctypes.c_void_p()
        self.check(self.lib.oa_malloc(ctypes.byref(p), nbytes))
        self.check(self.lib.oa_memset(p, 0, nbytes, None))
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


ALL = [(g, p) for g in GEOMS for p in ("f64", "f32")]


@pytest.mark.parametrize("geom,prec", ALL)
def test_one_call_equals_the_host_loop(geom, prec):
    one = _driver(geom, prec, None)
    assert one.one_call
    n1, m1, c1 = _moments(one.run_local(range(NSIMS)))
    host = _driver(geom, prec, False)
    n0, m0, c0 = _moments(host.run_local(range(NSIMS)))
    d = one.d
    assert n1 == n0 == NSIMS and m1.shape == (2 * d,) and c1.shape == (2 * d, 2 * d)
    scale = np.max(m0[:d] + m0[d:])                                  # max_b of the mean p(A)_b
    assert scale > 0 and np.all(m0[d:] > 0)
    err = np.abs(m1 - m0).max() / scale
    cerr = np.abs(c1 - c0).max() / np.abs(c0).max()
    print("rdn0 %s %s: mean err %.3g of max p(A), cov err %.3g of max cov" % (geom, prec, err, cerr))
    assert err <= TOL[prec]
    assert cerr <= 50 * TOL[prec]
    np.testing.assert_array_equal(one.rdn0(), m1[:d])
    np.testing.assert_array_equal(one.mcn0(), m1[d:])
    assert one.sem().shape == (d,) and one.cov().shape == (2 * d, 2 * d) and one.centers.shape == (d,)
    np.testing.assert_allclose(one.debiased(), one.data_bandpowers() - m1[:d], rtol=1e-13)


def test_host_loop_sample_is_the_numpy_statement():
    """sample 0 of the host loop at (600, 750) f64 == [p(A) - p(B) / 2, p(B) / 2] with A = QE(d, s) + QE(s, d), B = QE(s, s') + QE(s', s) of
    the oracle estimator, the draws copied from the device, bandpowers = bin means of |Z|^2 area / Npix^2 over the full plane."""
    from oracle import stats_oracle as so
    from oracle.qe_oracle import QEOracleTT
    shape, res = GEOMS["band"]
    g, th, ml, beam, noise, tmask, kmask = _inputs(shape, res)
    drv = _driver("band", "f64", False)
    e = drv.eng
    x = drv.sample_host(0).cpu().numpy()
    full = lambda k: e.hc_to_full(k).cpu().numpy()
    d, s, sp = full(drv.kd), full(e.grf_hc(31, 0, drv.cs)), full(e.grf_hc(31, 1, drv.cs))
    cl = th.lCl("TT", ml)
    qo = QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    A = qo.kappa_ft(d, s) + qo.kappa_ft(s, d)
    B = qo.kappa_ft(s, sp) + qo.kappa_ft(sp, s)
    bo = so.bin2D(ml, EDGES)
    pa = bo.bin(np.abs(A) ** 2 * drv.norm)[1]
    pb = bo.bin(np.abs(B) ** 2 * drv.norm)[1]
    ref = np.concatenate((pa - pb / 2, pb / 2))
    err = np.abs(x - ref).max() / pa.max()
    print("rdn0 host sample against NumPy: %.3g of max p(A)" % err)
    assert err <= 1e-9


@pytest.mark.parametrize("geom,prec", ALL)
def test_moments_do_not_depend_on_the_batch_size(geom, prec):
    q, _ = _est(geom, prec)
    res = {}
    for batch in (1, 3, 6):
        q.eng.set_option("mc_batch", batch)
        try:
            res[batch] = _moments(_driver(geom, prec, True).run_local(range(NSIMS)))
        finally:
            q.eng.set_option("mc_batch", 0)
    n1, m1, c1 = res[1]
    assert n1 == NSIMS
    for batch in (3, 6):
        nb, mb, cb = res[batch]
        assert nb == NSIMS
        np.testing.assert_allclose(mb, m1, rtol=1e-13)
        np.testing.assert_allclose(cb, c1, rtol=1e-9)


@pytest.mark.parametrize("geom,prec", ALL)
def test_sharding_and_repeat_runs(geom, prec):
    """run_local(0..6) == run_local(0..3) then run_local(4..6); two runs of the same driver are bit-equal."""
    whole = _driver(geom, prec, True).run_local(range(NSIMS))
    again = _driver(geom, prec, True).run_local(range(NSIMS))
    parts = _driver(geom, prec, True)
    parts.run_local([0, 1, 2, 3])
    parts.run_local([4, 5, 6])
    rw, ra = _raw(whole), _raw(again)
    assert rw[0] == NSIMS and np.array_equal(rw[1], ra[1]) and np.array_equal(rw[2], ra[2])
    (nw, mw, cw), (np_, mp, cp) = _moments(whole), _moments(parts)
    assert nw == np_ == NSIMS
    np.testing.assert_allclose(mp, mw, rtol=1e-13)
    np.testing.assert_allclose(cp, cw, rtol=1e-9)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_zero_data_data_independence_and_scaling(geom):
    prec = "f64"
    d = _driver(geom, prec, True).d
    _, S0, _ = _raw(_driver(geom, prec, True, scale=0.0).run_local(range(NSIMS)))
    assert np.all(S0[d:] > 0) and np.array_equal(S0[:d], -S0[d:])          # zero data: p(A) = 0, rdn0 = -mcn0 exactly
    _, S1, _ = _raw(_driver(geom, prec, True, data_seed=17).run_local(range(NSIMS)))
    _, S2, _ = _raw(_driver(geom, prec, True, data_seed=18).run_local(range(NSIMS)))
    assert np.array_equal(S1[d:], S2[d:]) and np.array_equal(S1[d:], S0[d:])  # the mcn0 half carries no data
    assert not np.array_equal(S1[:d], S2[:d])
    _, S4, _ = _raw(_driver(geom, prec, True, data_seed=17, scale=2.0).run_local(range(NSIMS)))
    np.testing.assert_allclose(S4[:d] + S4[d:], 4 * (S1[:d] + S1[d:]), rtol=1e-13)   # rdn0 + mcn0 = p(A), quadratic in the data


def test_stale_data_legs_are_refused_and_set_data_repairs():
    from orphics_amd._lib import check
    from orphics_amd.engine import _ptr, _stream
    drv = _driver("p512", "f32", True).run_local([0, 1])
    q, e = drv.q, drv.eng
    n, S, C = drv.acc.device_moments("rdn0", 2 * drv.d)
    run = lambda: e.lib.oa_mc_run_rdn0(e.plan, 31, 2, 4, _ptr(drv.cs), _ptr(n), _ptr(S), _ptr(C), _stream())
    check(run())
    FG, FH, Fn = q._F["TT"]
    check(e.lib.oa_plan_set_filters(e.plan, _ptr(FG), _ptr(FH), _ptr(Fn), q.leg_cols, q.kappa_cols, q.leg_rows, q.kappa_rows, int(q.mrow)))
    check(e.lib.oa_plan_set_col_grid(e.plan, int(q.mcol)))
    assert run() != 0
    msg = e.lib.oa_last_error().decode()
    assert "stale" in msg and "oa_rdn0_set_data" in msg
    check(e.lib.oa_rdn0_set_data(e.plan, _ptr(drv.kd), _stream()))
    check(run())
    torch.cuda.synchronize()
    assert int(n[0]) == 6                                             # 2 + 2 + 0 (refused: nothing launched) + 2
    ref = _raw(_driver("p512", "f32", True).run_local([0, 1, 2, 3, 2, 3]))
    assert np.array_equal(S.cpu().numpy(), ref[1])
    e._rdn0_owner = None                                              # (this test went behind the driver's back)


def test_chirp_z_sides_take_the_host_loop():
    from orphics_amd import lensing, mc
    from orphics_amd._lib import OrphicsAmdError
    shape = (112, 154)
    g, th, ml, beam, noise, tmask, kmask = _inputs(shape, 4.0)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f64")
    tot = (th.lCl("TT", ml) * beam ** 2 + noise)[:, :shape[1] // 2 + 1]
    edges = np.linspace(100, 2400, 8)
    with pytest.raises(OrphicsAmdError, match="one_call=False"):
        mc.RDN0MonteCarlo(q, np.zeros(shape), tot, edges, comm=None, one_call=True)
    drv = mc.RDN0MonteCarlo(q, np.random.default_rng(1).standard_normal(shape), tot, edges, comm=None, one_call=None)
    assert not drv.one_call
    st = drv.run(2)
    assert st.count("rdn0") == 2 and np.all(np.isfinite(st.mean("rdn0"))) and np.all(drv.mcn0() > 0)
    from orphics_amd.engine import _ptr
    n = torch.zeros(1, dtype=torch.int64, device=q.eng.device)
    S, C = (torch.zeros(k, dtype=torch.float64, device=q.eng.device) for k in (14, 196))
    assert q.eng.lib.oa_mc_run_rdn0(q.eng.plan, 1, 0, 1, _ptr(drv.cs), _ptr(n), _ptr(S), _ptr(C), None) != 0
    assert b"chirp-z" in q.eng.lib.oa_last_error()


def test_raw_pointers_and_refusals():
    """The C entries from oa_malloc pointers, no torch tensor involved: refused without bins and without data, then the moments of the
    Python driver on the same geometry."""
    from orphics_amd import _lib
    from orphics_amd._lib import check
    from orphics_amd import lensing
    lib = _lib.load()
    N = 256
    g, th, ml, beam, noise, tmask, kmask = _inputs((N, N), 2.0)
    q = lensing.qest((N, N), g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f32")
    tot = th.lCl("TT", ml) * beam ** 2 + noise
    tmap = np.fft.ifft2(np.fft.fft2(np.random.default_rng(4).standard_normal((N, N))) * np.sqrt(tot / g.pixarea)).real.astype(np.float32)
    dev = Dev(lib, check)
    try:
        plan = ctypes.c_void_p()
        check(lib.oa_plan_create(N, N, _lib.OA_F32, ctypes.byref(plan)))
        ly, lx = g.laxes()
        check(lib.oa_plan_set_laxes(plan, ly.ctypes.data_as(ctypes.c_void_p), lx.ctypes.data_as(ctypes.c_void_p)))
        edges = np.linspace(100, 3000, 12)
        nids, dd = edges.size + 1, 2 * (edges.size - 1)
        n, S, C = dev.zeros(8), dev.zeros(8 * dd), dev.zeros(8 * dd * dd)
        from orphics_amd import mc
        drv = mc.RDN0MonteCarlo(q, tmap, tot[:, :N // 2 + 1], edges, comm=None, base_seed=11)
        d_cs, d_kd = dev.up(drv.cs.cpu().numpy()), dev.up(drv.kd.cpu().numpy())
        run = lambda lo, hi: lib.oa_mc_run_rdn0(plan, 11, lo, hi, d_cs, n, S, C, None)
        assert run(0, 5) != 0 and b"oa_plan_set_filters" in lib.oa_last_error()
        assert lib.oa_rdn0_set_data(plan, d_kd, None) != 0 and b"oa_plan_set_filters" in lib.oa_last_error()
        FG, FH, Fn = [dev.up(t.cpu().numpy()) for t in q._F["TT"]]
        check(lib.oa_plan_set_filters(plan, FG, FH, Fn, q.leg_cols, q.kappa_cols, q.leg_rows, q.kappa_rows, -1))
        assert run(0, 5) != 0 and b"no bins bound" in lib.oa_last_error()
        d_ids = dev.up(drv.ids.cpu().numpy())
        check(lib.oa_plan_set_bins(plan, d_ids, nids, drv.norm, None))
        assert run(0, 5) != 0 and b"no data set" in lib.oa_last_error() and b"oa_rdn0_set_data" in lib.oa_last_error()
        check(lib.oa_rdn0_set_data(plan, d_kd, None))
        check(run(0, 5))
        check(run(5, 9))
        check(lib.oa_plan_release_pools(plan))
        assert run(9, 10) != 0 and b"no data set" in lib.oa_last_error()
        st = drv.run(9)
        assert dev.down(n, (1,), np.int64)[0] == 9 == st.count("rdn0")
        np.testing.assert_allclose(dev.down(S, (dd,), np.float64) / 9, st.mean("rdn0"), rtol=1e-13)
        assert np.all(st.mean("rdn0")[dd // 2:] > 0)
        check(lib.oa_plan_destroy(plan))
    finally:
        dev.free()
