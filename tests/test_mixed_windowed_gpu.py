"""GPU: the windowed N0 / mean-field Monte Carlo (``oa_mc_run_windowed``, ``mc.GaussianN0MonteCarlo(window=..., one_call=...)``) on map
sides 2^a 3^b 5^c.  Geometries: 300 x 360 at 2' (300 = 4 3 5^2, packed row length 180 = 4 3^2 5: all four radices; band grid 256^2) and
600 x 750 at 1' (band grid 256 x 512, packed row length 375 odd); filters T 300-2000, kappa 20-3500, taper
``maps.get_taper(shape, g, 12.0, 3.0)``.  Tolerances: one call against an equivalent launch sequence 1e-10 (f64) / 3e-5 (f32); mean field
against the NumPy oracle on the same maps 1e-9 / 2e-4 on 40 < ell < 3000; window == 1 against the unwindowed driver 1e-10 / 2e-5."""
import numpy as np
import pytest

from oracle import qe_oracle as qo

pytestmark = pytest.mark.gpu

GEOMS = {"300x360": ((300, 360), 2.0, (256, 256)), "600x750": ((600, 750), 1.0, (256, 512))}
# 300 x 1200 at 2': the same filters need 833 inner columns -> band grid 256 x 1024, the smallest inner row grid whose row stage takes a
# BATCH of realisations per launch (the two grids above run one realisation per launch behind the batched front end)
BATCHED = {"300x1200": ((300, 1200), 2.0, (256, 1024))}
# geometries no other test of this file touches (their plans keep the row-pass option unset): 360 x 300 at 2' (rows of 300 points: the
# automatic choice is the unfused flow; band grid 256^2) and 300 x 2400 at 2' (rows of 2400 points: the fused pass; band grid 256 x 2048)
UNTOUCHED = {"360x300": ((360, 300), 2.0, (256, 256)), "300x2400": ((300, 2400), 2.0, (256, 2048))}
GEOMS_ALL = dict(GEOMS, **BATCHED, **UNTOUCHED)
EDGES = np.linspace(100, 3000, 12)


def _setup(shape, res):
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
    taper, _ = maps.get_taper(shape, g, taper_percent=12.0, pad_percent=3.0)
    return g, th, ml, beam, noise, tmask, kmask, cl, taper


_CACHE = {}


def _prepared(name, prec):
    """geometry, filters, taper and estimator of one (geometry, precision), made once and shared by the tests that follow"""
    from orphics_amd import lensing
    key = (name, prec)
    if key not in _CACHE:
        shape, res, grid = GEOMS_ALL[name]
        g, th, ml, beam, noise, tmask, kmask, cl, taper = _setup(shape, res)
        q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype=prec)
        tot_h = (cl * beam ** 2 + noise)[:, :shape[1] // 2 + 1]
        _CACHE.clear()
        _CACHE[key] = dict(shape=shape, grid=grid, g=g, ml=ml, beam=beam, noise=noise, tmask=tmask, kmask=kmask, cl=cl, taper=taper, q=q, tot_h=tot_h)
    return _CACHE[key]


def _result(st, nx):
    mf = st.stack_sum("mf")
    return st.count("n0"), np.array(st.mean("n0")), (mf[..., 0] + 1j * mf[..., 1])[:, :nx // 2 + 1].copy()


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", list(GEOMS) + list(BATCHED))
def test_one_call_equals_the_host_loop_of_existing_entries(name, prec):
    """oa_mc_run_windowed on the band grid (full-plane draw, inverse columns, fused windowed row pass, pruned columns, batched inner
    launches) == Engine.grf_hc -> Engine.irfft -> x window -> tt_moments (+ reconstruct_tt_from_map into the stack) on the same plan:
    count, mean bandpowers and the mean-field stack; batches of 1 and of 6 (8 sims: a full batch and a remainder of 2), fused row pass
    and the unfused flow (win_fused = 0)."""
    from orphics_amd import mc
    P = _prepared(name, prec)
    q, shape = P["q"], P["shape"]
    e = q.eng
    assert e.mixed and q.one_call() and q.band_grid == P["grid"]
    nsims, seed = 8, 77
    tol = 1e-10 if prec == "f64" else 3e-5
    kw = dict(base_seed=seed, mean_field=True, window=P["taper"])
    n0, m0, s0 = _result(mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, one_call=False, **kw).run(nsims), shape[1])
    assert n0 == nsims and np.all(m0 > 0) and np.abs(s0).max() > 0
    try:
        for batch, fused in ((6, 1), (1, 1), (6, 0), (1, 0)):
            e.set_option("mc_batch", batch)
            e.set_option("win_fused", fused)
            st = mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, one_call=True, **kw).run(nsims)
            n1, m1, s1 = _result(st, shape[1])
            print("%s %s batch %d fused %d: mean %.3g stack %.3g" % (name, prec, batch, fused, np.abs(m1 / m0 - 1).max(),
                                                                      np.abs(s1 - s0).max() / np.abs(s0).max()))
            assert n1 == nsims and st.stack_count("mf") == nsims
            np.testing.assert_allclose(m1, m0, rtol=tol)
            assert np.abs(s1 - s0).max() < tol * np.abs(s0).max()
    finally:
        e.set_option("mc_batch", 0)
        e.set_option("win_fused", -1)         # back to the plan's automatic choice


@pytest.mark.parametrize("name,prec", [("360x300", "f64"), ("300x2400", "f32")])
def test_automatic_row_pass_choice_on_a_plan_whose_option_was_never_set(name, prec):
    """no win_fused option anywhere: the plan picks by row length (unfused up to 1200 points, fused above) and either way equals the host
    loop; batches of the default size"""
    from orphics_amd import mc
    P = _prepared(name, prec)
    q, shape = P["q"], P["shape"]
    e = q.eng
    assert e.mixed and q.one_call() and q.band_grid == P["grid"]
    assert "win_fused" not in getattr(e, "_options", {}) and "mc_batch" not in getattr(e, "_options", {})
    nsims = 8
    tol = 1e-10 if prec == "f64" else 3e-5
    kw = dict(base_seed=31, mean_field=True, window=P["taper"])
    n0, m0, s0 = _result(mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, one_call=False, **kw).run(nsims), shape[1])
    n1, m1, s1 = _result(mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, one_call=True, **kw).run(nsims), shape[1])
    print("%s %s automatic: mean %.3g stack %.3g" % (name, prec, np.abs(m1 / m0 - 1).max(), np.abs(s1 - s0).max() / np.abs(s0).max()))
    assert n0 == n1 == nsims and np.all(m0 > 0)
    np.testing.assert_allclose(m1, m0, rtol=tol)
    assert np.abs(s1 - s0).max() < tol * np.abs(s0).max()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bin_counts_on_an_odd_row_pitch_equal_the_whole_plane_counts(prec):
    """600 x 750: the N-grid row pitch 375 + 16 is odd; oa_plan_set_bins (which refused such a plan before) keeps the mode counts of the
    whole half plane, those of Engine.bin_power"""
    P = _prepared("600x750", prec)
    q = P["q"]
    e = q.eng
    assert e.kp % 4
    import torch
    ids = e.modl_digitize(torch.as_tensor(EDGES, device=e.device), half=True)
    nids = EDGES.size + 1
    norm = q.geom.area / float(e.npix) ** 2
    q.bind_bins(ids, nids, norm)
    zero = e.hc()
    want = e.bin_power(zero, zero, norm, ids, nids, herm=True)[1].cpu().numpy()
    got = q.bin_counts().cpu().numpy()
    assert got.sum() > 0 and np.array_equal(got, want)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_unit_window_reproduces_the_unwindowed_band_grid_driver(name, prec):
    """window == 1: the full-plane draw's leg band is the band draw of oa_mc_run, and C2R -> R2C is the identity there"""
    from orphics_amd import mc
    P = _prepared(name, prec)
    q, shape = P["q"], P["shape"]
    q.eng.set_option("win_fused", 1)          # the fused row kernel (unset, rows this short take the unfused flow)
    nsims = 8
    plain = mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, base_seed=5).run(nsims)
    ones = mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, base_seed=5, window=np.ones(shape), one_call=True).run(nsims)
    assert ones.count("n0") == plain.count("n0") == nsims
    np.testing.assert_allclose(ones.mean("n0"), plain.mean("n0"), rtol=(1e-10 if prec == "f64" else 2e-5))


@pytest.mark.parametrize("prec,tol", [("f64", 1e-9), ("f32", 2e-4)])
def test_windowed_mean_field_matches_the_oracle_on_the_same_maps(prec, tol):
    """300 x 360: the stacked mean field of the one call == oracle.QEOracleTT on the same maps (the driver's draw, C2R / Npix, taper),
    and its low-ell power dwarfs the unwindowed run's"""
    from orphics_amd import mc
    P = _prepared("300x360", prec)
    q, shape, ml, taper = P["q"], P["shape"], P["ml"], P["taper"]
    e = q.eng
    e.set_option("win_fused", 1)              # the fused row kernel (unset, rows this short take the unfused flow)
    nxh = shape[1] // 2 + 1
    nsims = 8               # (the unwindowed stack is reconstruction noise and averages down as 1 / nsims: the most this file runs)
    drv = mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, base_seed=5, mean_field=True, window=taper, one_call=True)
    st = drv.run(nsims)
    assert st.count("n0") == nsims and st.stack_count("mf") == nsims
    mfk = _result(st, shape[1])[2] / nsims
    qr = qo.QEOracleTT(shape, P["g"].step_y, P["g"].step_x, P["cl"], P["cl"], P["noise"], P["beam"], P["tmask"], kmask_K=P["kmask"])
    ref = 0
    for i in range(nsims):
        m = e.irfft(e.grf_hc(5, i, drv.cs)).double().cpu().numpy() * taper
        ref = ref + qr.kappa_from_map("TT", m, returnFt=True)[:, :nxh]
    ref = ref / nsims
    sel = (ml[:, :nxh] > 40) & (ml[:, :nxh] < 3000)
    err = np.abs(mfk - ref)[sel].max() / np.abs(ref[sel]).max()
    print("mean field against the oracle, %s: %.3g" % (prec, err))
    assert err < tol
    plain = mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, base_seed=5, mean_field=True).run(nsims)
    pmk = _result(plain, shape[1])[2] / nsims
    # "low ell": the taper is defined in fractions of the patch side, so its transform -- and the mean field it induces -- is a function
    # of L in units of the patch's fundamental l_f = 2 pi / sqrt(area); the power-of-two test's band 20 < L < 200 on its 512 x 1' patch
    # (l_f = 42.2) is L < 4.74 l_f, which is L < 156 on this 10 x 12 degree patch (l_f = 32.9)
    lf = 2 * np.pi / np.sqrt(P["g"].area)
    low = (ml[:, :nxh] > 20) & (ml[:, :nxh] < 4.74 * lf)
    print("low-ell (< 4.74 l_f = %.0f) mean-field power, windowed / unwindowed: %.3g" % (4.74 * lf, np.mean(np.abs(mfk[low]) ** 2) /
                                                                                       np.mean(np.abs(pmk[low]) ** 2)))
    assert np.mean(np.abs(mfk[low]) ** 2) > 20 * np.mean(np.abs(pmk[low]) ** 2)


def test_three_streams_equal_one_stream():
    """streams=3 (forked estimator handles, their own plans, band grids and windowed buffers): same realisations, same moments and stack
    up to summation order"""
    from orphics_amd import mc
    P = _prepared("300x360", "f32")
    q, shape = P["q"], P["shape"]
    q.eng.set_option("win_fused", 1)          # the fused row kernel on every lane (Estimator.fork copies the plan options)
    kw = dict(base_seed=6, mean_field=True, window=P["taper"], one_call=True)
    a = mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, **kw).run(24)
    drv = mc.GaussianN0MonteCarlo(q, P["tot_h"], EDGES, streams=3, **kw)
    b = drv.run(24)
    assert getattr(drv, "_lanes", None) is not None and len(drv._lanes) == 3
    assert a.count("n0") == b.count("n0") == 24 and b.stack_count("mf") == 24
    np.testing.assert_allclose(b.mean("n0"), a.mean("n0"), rtol=1e-12)
    sa, sb = _result(a, shape[1])[2], _result(b, shape[1])[2]
    assert np.abs(sa - sb).max() < 1e-12 * np.abs(sa).max()


def test_raw_entries():
    """oa_mc_run_windowed refuses a mixed-radix plan without bound filters and a chirp-z plan, each with a message; oa_fft_c2r_windowed
    on 300 x 360 == irfft2 x window"""
    import torch
    from orphics_amd.engine import Engine, _ptr
    for (ny, nx), words in (((300, 360), ["oa_plan_set_filters"]), ((112, 154), ["chirp-z"])):
        e = Engine(ny, nx, "f64")
        assert (e.mixed, e.pow2) == ((ny, nx) == (300, 360), False)
        cs, w = e.hcreal(), e.real()
        n = torch.zeros(1, dtype=torch.int64, device=e.device)
        S = torch.zeros(3, dtype=torch.float64, device=e.device)
        C = torch.zeros((3, 3), dtype=torch.float64, device=e.device)
        rc = e.lib.oa_mc_run_windowed(e.plan, 1, 0, 1, _ptr(cs), _ptr(w), _ptr(n), _ptr(S), _ptr(C), None, None)
        msg = e.lib.oa_last_error().decode()
        assert rc != 0 and "oa_mc_run_windowed" in msg and all(x in msg for x in words), msg
        torch.cuda.synchronize()
        assert int(n.item()) == 0
    rng = np.random.default_rng(11)
    x = rng.standard_normal((300, 360))
    w = rng.uniform(0.0, 1.0, (300, 360))
    for prec, tol in (("f32", 3e-6), ("f64", 1e-12)):
        e = Engine.get(300, 360, prec)
        k = e.rfft(e.to_real(x))
        yw = e.irfft(k, window=e.to_real(w)).cpu().numpy()
        ref = np.fft.irfft2(k.cpu().numpy().astype(np.complex128)[:, :181], s=(300, 360)) * w.astype(yw.dtype)
        assert np.abs(yw - ref).max() / np.abs(ref).max() < tol


def test_geometry_without_a_band_grid_refuses_the_one_call_and_runs_the_host_loop():
    """480 x 600 at 2': the band grid would need 512 rows.  one_call=True raises naming the way out; one_call=False runs the modular
    host loop, whose mean field matches the oracle on the same maps."""
    from orphics_amd import lensing, mc
    from orphics_amd._lib import OrphicsAmdError
    shape, res = (480, 600), 2.0
    g, th, ml, beam, noise, tmask, kmask, cl, taper = _setup(shape, res)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f64")
    e = q.eng
    assert e.mixed and not q.one_call()
    nxh = shape[1] // 2 + 1
    tot_h = (cl * beam ** 2 + noise)[:, :nxh]
    with pytest.raises(OrphicsAmdError, match="band grid not smaller than the map.*one_call=False"):
        mc.GaussianN0MonteCarlo(q, tot_h, EDGES, mean_field=True, window=taper, one_call=True)
    nsims = 4
    drv = mc.GaussianN0MonteCarlo(q, tot_h, EDGES, base_seed=5, mean_field=True, window=taper, one_call=False)
    st = drv.run(nsims)
    assert st.count("n0") == nsims and st.stack_count("mf") == nsims and np.all(st.mean("n0") > 0)
    mfk = _result(st, shape[1])[2] / nsims
    qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    ref = 0
    for i in range(nsims):
        m = e.irfft(e.grf_hc(5, i, drv.cs)).double().cpu().numpy() * taper
        kap = qr.kappa_from_map("TT", m, returnFt=True)
        ref = ref + kap[:, :nxh]
    ref = ref / nsims
    sel = (ml[:, :nxh] > 40) & (ml[:, :nxh] < 3000)
    assert np.abs(mfk - ref)[sel].max() < 1e-9 * np.abs(ref[sel]).max()
