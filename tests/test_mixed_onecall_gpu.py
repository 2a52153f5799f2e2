"""GPU: the one-call TT entries on map sides 2^a 3^b 5^c (BAND GRID, include/orphics_amd.h oa_plan_band_grid): oa_qe_tt from a
map and from kX [, kY], oa_qe_tt_moments(2) and oa_mc_run on the notebooks' 1200^2 / 2400^2 patches at 0.5' and a 600 x 750 patch
at 1', against the modular chain of the same plan, the NumPy oracle, and the refusals that keep the modular chain."""
import ctypes

import numpy as np
import pytest

from oracle import qe_oracle as qo

pytestmark = pytest.mark.gpu

GEOMS = [((1200, 1200), 0.5, (256, 256)), ((2400, 2400), 0.5, (512, 512)), ((600, 750), 1.0, (256, 512))]


def _setup(shape, res, seed=0):
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
    return g, th, ml, beam, noise, tmask, kmask, cl, np.fft.ifft2(tk).real


def _qest(shape, g, th, beam, noise, tmask, kmask, prec, **kw):
    from orphics_amd import lensing
    return lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype=prec, **kw)


def _band_mask(q):
    """(Ny, kp) True on kappa's band: columns < kappa_cols, rows |ky| < kappa_rows"""
    e = q.eng
    ky = np.fft.fftfreq(e.ny, 1.0 / e.ny)
    m = np.zeros((e.ny, e.kp), dtype=bool)
    m[np.abs(ky) < q.kappa_rows, :q.kappa_cols] = True
    return m


_CACHE = {}


def _prepared(shape, res, prec):
    key = (shape, res, prec)
    if key not in _CACHE:
        g, th, ml, beam, noise, tmask, kmask, cl, tmap = _setup(shape, res, seed=shape[0] + shape[1])
        q = _qest(shape, g, th, beam, noise, tmask, kmask, "f64")
        _CACHE.clear()
        _CACHE[key] = (g, ml, beam, noise, tmask, kmask, cl, tmap, q if prec == "f64" else q.astype("f32"))
    return _CACHE[key]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape,res,grid", GEOMS)
def test_onecall_tt_on_band_grid_equals_modular_chain(shape, res, grid, prec):
    """oa_qe_tt on a mixed-radix plan (from the map, from kX, from kX + kY) == the modular chain of the same plan (f64 1e-11 on
    kappa_hat), exact zeros outside kappa's band in a caller plane, and the plan reports the notebook's inner grid."""
    import torch
    from orphics_amd._lib import check
    g, ml, beam, noise, tmask, kmask, cl, tmap, q = _prepared(shape, res, prec)
    e = q.eng
    assert e.mixed and q.one_call()
    assert q.band_grid == grid
    my, mx = ctypes.c_int(-1), ctypes.c_int(-1)
    check(e.lib.oa_plan_band_grid(e.plan, ctypes.byref(my), ctypes.byref(mx)))
    assert (my.value, mx.value) == grid
    tm = e.to_real(tmap)
    k = e.rfft(tm)
    k2 = e.rfft(e.to_real(np.roll(tmap, 17, axis=1)))
    mod = q.reconstruct_tt_hc(k, fused=False).clone()
    mod2 = q.reconstruct_tt_hc(k, k2, fused=False).clone()
    tol = 1e-11 if prec == "f64" else 2e-5
    band = torch.as_tensor(_band_mask(q), device=e.device)
    scale = float(mod.abs().max())
    assert float(mod[~band].abs().max()) == 0.0
    for got, ref in ((q.reconstruct_tt_from_map(tm), mod), (q.reconstruct_tt_hc(k), mod), (q.reconstruct_tt_hc(k, k2), mod2)):
        assert float((got - ref)[:, :e.nxh + 1].abs().max()) <= tol * scale
    # caller plane holding garbage: zero-filled outside the band, band written
    out = e.hc()
    out.fill_(7 + 7j)
    got = q.reconstruct_tt_hc(k, out=out)
    assert got is out
    assert float(out[~band].abs().max()) == 0.0
    assert float((out - mod)[:, :e.nxh + 1].abs().max()) <= tol * scale


@pytest.mark.parametrize("shape,res,grid", GEOMS)
def test_onecall_tt_on_band_grid_matches_oracle(shape, res, grid):
    """kappa_from_map("TT") (now the one-call band-grid path) against oracle.QEOracleTT: f64 1e-8 on kappa_hat's DFT, f32 1e-5 on
    its bandpowers."""
    from orphics_amd import stats
    g, ml, beam, noise, tmask, kmask, cl, tmap, q = _prepared(shape, res, "f64")
    qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    ref = qr.kappa_from_map("TT", tmap, returnFt=True)
    got = q.kappa_from_map("TT", tmap, returnFt=True)
    assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max()
    binner = stats.bin2D(ml, np.linspace(20, 3500, 20))
    ref_b = binner.bin(np.abs(ref) ** 2)[1]
    got32 = q.astype("f32").kappa_from_map("TT", tmap.astype(np.float32), returnFt=True)
    b32 = binner.bin(np.abs(np.asarray(got32, dtype=np.complex128)) ** 2)[1]
    assert np.max(np.abs(b32 / ref_b - 1)) <= 1e-5


def _bins(q, edges):
    import torch
    e = q.eng
    ids = e.modl_digitize(torch.as_tensor(edges, device=e.device), half=True)
    nids = edges.size + 1
    norm = q.geom.area / float(e.npix) ** 2
    return ids, nids, norm


def _host_bandpower(q, kappa, ids, nids, norm):
    sums, counts = q.eng.bin_power(kappa, kappa, norm, ids, nids)
    return (sums.cpu().numpy() / counts.cpu().numpy())[1:-1], counts.cpu().numpy()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_tt_moments_on_band_grid(prec):
    """tt_moments / tt_moments2 at 1200^2: n, S, C equal the numpy moments of the modular chain's bandpowers of the same maps, and
    bin_counts equals the whole-plane mode counts."""
    import torch
    shape, res = (1200, 1200), 0.5
    g, ml, beam, noise, tmask, kmask, cl, tmap, q = _prepared(shape, res, prec)
    e = q.eng
    edges = np.linspace(20, 3500, 20)
    ids, nids, norm = _bins(q, edges)
    q.bind_bins(ids, nids, norm)
    d = nids - 2
    rng = np.random.default_rng(4)
    maps = [e.to_real(tmap), e.to_real(np.roll(tmap, 101, axis=0))] + [e.to_real(tmap * rng.uniform(0.5, 1.5)) for _ in range(3)]
    n = torch.zeros(1, dtype=torch.int64, device=e.device)
    S = torch.zeros(d, dtype=torch.float64, device=e.device)
    C = torch.zeros((d, d), dtype=torch.float64, device=e.device)
    q.tt_moments(maps[0], n, S, C)
    q.tt_moments2(maps[1], maps[2], n, S, C)
    q.tt_moments(maps[3], n, S, C)
    q.tt_moments(maps[4], n, S, C)
    bs = []
    for m in maps:
        b, counts = _host_bandpower(q, q.reconstruct_tt_hc(e.rfft(m), fused=False), ids, nids, norm)
        bs.append(b)
    bs = np.array(bs)
    tol = 1e-10 if prec == "f64" else 2e-5
    assert int(n.item()) == len(maps)
    np.testing.assert_allclose(S.cpu().numpy(), bs.sum(0), rtol=tol)
    np.testing.assert_allclose(C.cpu().numpy(), bs.T @ bs, rtol=tol)
    assert np.array_equal(q.bin_counts().cpu().numpy(), counts)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_gaussian_n0_monte_carlo_on_band_grid(prec):
    """GaussianN0MonteCarlo at 1200^2 (the verification notebook's cell 4 on its own geometry), with and without the mean field,
    OA_OPT_MC_BATCH 1 and 6: moments == a host loop of Engine.grf_hc (full-plane draw, same seed and stream) -> modular chain ->
    binning, and the stack == the sum of those kappa_hat."""
    import torch
    from orphics_amd import mc
    shape, res = (1200, 1200), 0.5
    g, ml, beam, noise, tmask, kmask, cl, tmap, q = _prepared(shape, res, prec)
    e = q.eng
    nx = shape[1]
    tot_h = (cl * beam ** 2 + noise)[:, :nx // 2 + 1]
    edges = np.linspace(100, 3000, 12)
    nsims, seed = 8, 41
    ids, nids, norm = _bins(q, edges)
    ref_b, stack = [], 0
    drv0 = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=seed)
    for i in range(nsims):
        kap = q.reconstruct_tt_hc(e.grf_hc(seed, i, drv0.cs), fused=False)
        ref_b.append(_host_bandpower(q, kap, ids, nids, norm)[0])
        stack = stack + kap.to(torch.complex128).cpu().numpy()
    ref_b = np.array(ref_b)
    tol = 1e-10 if prec == "f64" else 2e-5
    for batch in (1, 6):
        e.set_option("mc_batch", batch)
        for mean_field in (False, True):
            st = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=seed, mean_field=mean_field).run(nsims)
            assert st.count("n0") == nsims
            np.testing.assert_allclose(st.mean("n0"), ref_b.mean(0), rtol=tol)
            np.testing.assert_allclose(st.cov("n0"), np.cov(ref_b.T), rtol=50 * tol, atol=50 * tol * np.abs(np.cov(ref_b.T)).max())
            if mean_field:
                mf = st.stack_sum("mf")
                mfk = mf[..., 0] + 1j * mf[..., 1]
                sc = np.abs(stack).max()
                assert np.abs(mfk - stack)[:, :nx // 2 + 1].max() <= tol * sc
    e.set_option("mc_batch", 0)


def test_band_grid_refusals_and_modular_fallback():
    """mrow = 0, unbounded filters, a band too wide for its side (480 x 600 at 2') and a chirp-z side (112 x 154): oa_plan_set_filters
    refuses naming the reason, the Python path takes the modular chain (still matching the oracle), and the windowed Monte Carlo
    refuses up front."""
    import torch
    from orphics_amd import mc
    from orphics_amd._lib import OrphicsAmdError
    from orphics_amd.engine import _ptr

    def refused(q, words):
        e = q.eng
        FG, FH, Fn = q._F["TT"]
        (wl, wk), (rl, rk) = q._W["TT"], q._R["TT"]
        rc = e.lib.oa_plan_set_filters(e.plan, _ptr(FG), _ptr(FH), _ptr(Fn), int(wl), int(wk), int(rl), int(rk), int(q.mrow))
        msg = e.lib.oa_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), msg
        e._pipe_owner = None

    def falls_back(q, shape, g, cl, noise, beam, tmask, kmask, tmap):
        assert not q.one_call()
        ref = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask).kappa_from_map("TT", tmap, returnFt=True)
        got = q.kappa_from_map("TT", tmap, returnFt=True)
        assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max()
        with pytest.raises(OrphicsAmdError):
            q._bind()

    shape, res = (600, 750), 1.0
    g, th, ml, beam, noise, tmask, kmask, cl, tmap = _setup(shape, res, seed=9)
    q0 = _qest(shape, g, th, beam, noise, tmask, kmask, "f64", row_grid="full")
    refused(q0, ["mrow = 0"])
    falls_back(q0, shape, g, cl, noise, beam, tmask, kmask, tmap)
    qa = _qest(shape, g, th, beam, noise, tmask, kmask, "f64", prune=False)
    assert qa.mrow == 0
    qa.mrow = -1
    refused(qa, ["band-limited"])
    qa.mrow = 0
    q1 = _qest(shape, g, th, beam, noise, tmask, kmask, "f64")
    with pytest.raises(OrphicsAmdError, match="window"):
        mc.GaussianN0MonteCarlo(q1, (cl * beam ** 2 + noise)[:, :shape[1] // 2 + 1], np.linspace(100, 3000, 12), window=np.ones(shape))

    shape, res = (480, 600), 2.0
    g, th, ml, beam, noise, tmask, kmask, cl, tmap = _setup(shape, res, seed=3)
    qw = _qest(shape, g, th, beam, noise, tmask, kmask, "f64")
    refused(qw, ["band too wide", "512", "480"])
    falls_back(qw, shape, g, cl, noise, beam, tmask, kmask, tmap)

    shape, res = (112, 154), 8.0
    g, th, ml, beam, noise, tmask, kmask, cl, tmap = _setup(shape, res, seed=1)
    qc = _qest(shape, g, th, beam, noise, tmask, kmask, "f64")
    assert not qc.eng.mixed and not qc.eng.pow2
    refused(qc, ["chirp-z"])
    assert not qc.one_call()
    got = qc.kappa_from_map("TT", tmap, returnFt=True)
    ref = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask).kappa_from_map("TT", tmap, returnFt=True)
    assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max()
