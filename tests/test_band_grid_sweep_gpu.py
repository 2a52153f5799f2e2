"""GPU: the BAND GRID of the one-call TT entries on map sides 2^a 3^b 5^c (include/orphics_amd.h oa_plan_band_grid, csrc/band.hip,
csrc/pipeline.hip band_grid_rule) across filter bands, map geometries and explicit grids, chosen so that each edge of the band
kernels and of the grid rule is hit: one and many row segments of band_cols_kernel, band widths on and off its 16-wide tiles, the
smallest grid (BAND_MIN = 128), My != Mx both ways, explicit row / column grids, a power-of-two map side, and kappa bands wider than
the hc plane of the smallest alias-free grid.  For each case and precision:
  (d) the resolved grid holds kappa's columns (Mx / 2 + 1 >= kappa_cols) and is the one engine.band_grid predicts;
  (a) oa_qe_tt from the map, from kX and from kX + kY == the plan's modular chain (f64 1e-11, f32 2e-5 of max |kappa_hat|), exact
      zeros outside kappa's band;
  (b) f64: kappa_from_map == oracle.QEOracleTT to 1e-8;
  (c) tt_moments == NumPy moments of the modular chain's bandpowers, bin_counts == the whole-plane mode counts.
Values are compared on the modes L < 1.8 l_T,max: above 2 l_T,max the response is roundoff-sized and both paths divide by it."""
import ctypes

import numpy as np
import pytest

from oracle import qe_oracle as qo

pytestmark = pytest.mark.gpu

# (id, shape, res arcmin, T lmin / lmax, kappa lmin / lmax, row_grid, col_grid, expected (My, Mx))
CASES = [
    # Defect-2 geometry: kappa 84 columns wide, legs 20 -> 2 wl + wk = 124 alone gives Mx = 128 (65 hc columns); the grid must be 256.
    # Also MANY row segments in band_cols_kernel (6 tiles -> 38 segments of 32 rows, a 16-row tail) and wl off a multiple of 16
    ("wide_kappa_1200", (1200, 1200), 0.5, (100, 700), (20, 3000), "auto", "auto", (256, 256)),
    # Defect-2 geometry: wk = 300 on Mx = 512 (272 pitch columns) before; now 1024 x 1024; 5 segments of 480 rows
    ("wide_kappa_2400", (2400, 2400), 0.5, (300, 1900), (20, 5400), "auto", "auto", (1024, 1024)),
    # ONE row segment at its edge: legs to l 4500 -> wl = 250, 2 rl - 1 = 499 -> 16 x 32 tiles = BC_TARGET_WG (512) exactly
    ("one_segment_2400", (2400, 2400), 0.5, (300, 4500), (20, 4500), "auto", "auto", (1024, 1024)),
    # wl = 32 on a multiple of BC_TX, 2 rl - 1 = 63 one under a multiple of BC_TK; the grid is BAND_MIN on both axes
    ("tiles_on_16", (1200, 1200), 0.5, (300, 1130), (20, 1130), "auto", "auto", (128, 128)),
    # wl = 33 one over a multiple of 16, 2 rl - 1 = 65 one over; 19 segments of 64 rows with a 48-row tail
    ("tiles_off_16", (1200, 1200), 0.5, (300, 1160), (20, 1000), "auto", "auto", (128, 128)),
    # BAND_MIN in y with an explicit larger row grid in x: My < Mx
    ("min_rows_row_grid", (1200, 1200), 0.5, (300, 1000), (20, 1000), 512, "auto", (128, 512)),
    # explicit larger row and column grids than the rule's 256 x 256 (the same kappa modes); 13 segments of 96 rows, 48-row tail
    ("explicit_grids", (1200, 1200), 0.5, (300, 2000), (20, 3500), 512, 1024, (1024, 512)),
    # a power-of-two map side (ny = 1024) next to a mixed one
    ("pow2_rows", (1024, 1200), 0.5, (300, 2000), (20, 3500), "auto", "auto", (256, 256)),
    # My > Mx (600 x 750 in test_mixed_onecall_gpu has My < Mx); 12 segments of 64 rows, a 46-row tail
    ("tall_750x600", (750, 600), 1.0, (300, 2000), (20, 3500), "auto", "auto", (512, 256)),
]
IDS = [c[0] for c in CASES]


def _setup(shape, res, tl, kl, seed):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=tl[0], lmax=tl[1])
    kmask = maps.mask_kspace(shape, g, lmin=kl[0], lmax=kl[1])
    cl = th.lCl("TT", ml)
    rng = np.random.default_rng(seed)
    tk = np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cl * beam ** 2 + noise) / g.pixarea)
    return g, th, ml, beam, noise, tmask, kmask, cl, np.fft.ifft2(tk).real


_CACHE = {}


def _prepared(case, prec):
    """(setup, estimator) of a case; the f64 and f32 estimators of the last case stay cached"""
    from orphics_amd import lensing
    name, shape, res, tl, kl, row_grid, col_grid, grid = case
    if name not in _CACHE:
        _CACHE.clear()
        s = _setup(shape, res, tl, kl, seed=shape[0] + 3 * shape[1] + tl[1])
        g, th, ml, beam, noise, tmask, kmask, cl, tmap = s
        q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f64",
                         row_grid=row_grid, col_grid=col_grid)
        _CACHE[name] = {"setup": s, "f64": q}
    ent = _CACHE[name]
    if prec not in ent:
        ent[prec] = ent["f64"].astype(prec)
    return ent["setup"], ent[prec]


def _low_modes(e, ml, lmax):
    """(Ny, kp) True on the hc modes with L < lmax"""
    m = np.zeros((e.ny, e.kp), dtype=bool)
    m[:, :e.nxh + 1] = ml[:, :e.nxh + 1] < lmax
    return m


def _band_mask(q):
    e = q.eng
    ky = np.fft.fftfreq(e.ny, 1.0 / e.ny)
    m = np.zeros((e.ny, e.kp), dtype=bool)
    m[np.abs(ky) < q.kappa_rows, :q.kappa_cols] = True
    return m


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_band_grid_sweep(case, prec):
    import torch
    from orphics_amd._lib import check
    from orphics_amd.engine import band_grid
    name, shape, res, tl, kl, row_grid, col_grid, grid = case
    (g, th, ml, beam, noise, tmask, kmask, cl, tmap), q = _prepared(case, prec)
    e = q.eng
    assert e.mixed and q.one_call()

    # (d) the grid the plan resolved holds kappa's columns and rows, and is engine.band_grid's
    (wl, wk), (rl, rk) = q._W["TT"], q._R["TT"]
    my, mx = ctypes.c_int(-1), ctypes.c_int(-1)
    q._bind()
    check(e.lib.oa_plan_band_grid(e.plan, ctypes.byref(my), ctypes.byref(mx)))
    my, mx = my.value, mx.value
    assert (my, mx) == grid == band_grid(e.ny, e.nx, wl, wk, rl, rk, q.mrow, q.mcol)
    assert mx // 2 + 1 >= q.kappa_cols == wk and my >= 2 * rk and mx >= 2 * wl + wk and my >= 2 * rl + rk

    # (a) one call == modular chain on the compared modes; exact zeros outside kappa's band
    tm = e.to_real(tmap)
    k = e.rfft(tm)
    k2 = e.rfft(e.to_real(np.roll(tmap, 17, axis=1)))
    mod = q.reconstruct_tt_hc(k, fused=False).clone()
    mod2 = q.reconstruct_tt_hc(k, k2, fused=False).clone()
    tol = 1e-11 if prec == "f64" else 2e-5
    band = torch.as_tensor(_band_mask(q), device=e.device)
    low = torch.as_tensor(_low_modes(e, ml, 1.8 * tl[1]), device=e.device)
    for got, ref in ((q.reconstruct_tt_from_map(tm), mod), (q.reconstruct_tt_hc(k), mod), (q.reconstruct_tt_hc(k, k2), mod2)):
        scale = float(ref[low].abs().max())
        assert scale > 0
        err = float((got - ref)[low].abs().max()) / scale
        assert err <= tol, (name, err)
    out = e.hc()
    out.fill_(7 + 7j)
    got = q.reconstruct_tt_hc(k, out=out)
    assert float(out[~band].abs().max()) == 0.0
    assert float((got - mod)[low].abs().max()) <= tol * float(mod[low].abs().max())

    # (b) f64: the one-call kappa_from_map against the NumPy oracle
    if prec == "f64":
        qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
        ref = qr.kappa_from_map("TT", tmap, returnFt=True)
        got = np.asarray(q.kappa_from_map("TT", tmap, returnFt=True))
        sel = ml < 1.8 * tl[1]
        assert np.abs(got - ref)[sel].max() <= 1e-8 * np.abs(ref[sel]).max()

    # (c) tt_moments == NumPy moments of the modular chain's bandpowers; bin_counts == the whole-plane counts
    edges = np.linspace(kl[0], min(kl[1], 1.8 * tl[1]), 9)
    ids = e.modl_digitize(torch.as_tensor(edges, device=e.device), half=True)
    nids = edges.size + 1
    norm = q.geom.area / float(e.npix) ** 2
    q.bind_bins(ids, nids, norm)
    d = nids - 2
    maps = [tm, e.to_real(np.roll(tmap, 101, axis=0)), e.to_real(0.7 * tmap)]
    n = torch.zeros(1, dtype=torch.int64, device=e.device)
    S = torch.zeros(d, dtype=torch.float64, device=e.device)
    C = torch.zeros((d, d), dtype=torch.float64, device=e.device)
    for m in maps:
        q.tt_moments(m, n, S, C)
    bs = []
    for m in maps:
        kap = q.reconstruct_tt_hc(e.rfft(m), fused=False)
        sums, counts = e.bin_power(kap, kap, norm, ids, nids)
        bs.append((sums.cpu().numpy() / counts.cpu().numpy())[1:-1])
    bs = np.array(bs)
    mtol = 1e-10 if prec == "f64" else 2e-5
    assert int(n.item()) == len(maps)
    np.testing.assert_allclose(S.cpu().numpy(), bs.sum(0), rtol=mtol)
    np.testing.assert_allclose(C.cpu().numpy(), bs.T @ bs, rtol=mtol)
    assert np.array_equal(q.bin_counts().cpu().numpy(), counts.cpu().numpy())


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_gaussian_n0_monte_carlo_on_wide_kappa_band(prec):
    """GaussianN0MonteCarlo with the mean field on the 1200^2 Defect-2 geometry (kappa 84 columns wide, legs 20): moments and the
    mean-field stack (band_stack_add into the N-grid accumulator) == a host loop of Engine.grf_hc -> modular chain -> binning."""
    import torch
    from orphics_amd import mc
    case = CASES[0]
    name, shape, res, tl, kl, row_grid, col_grid, grid = case
    (g, th, ml, beam, noise, tmask, kmask, cl, tmap), q = _prepared(case, prec)
    e = q.eng
    nx = shape[1]
    tot_h = (cl * beam ** 2 + noise)[:, :nx // 2 + 1]
    edges = np.linspace(kl[0], 1.8 * tl[1], 9)
    nsims, seed = 4, 23
    ids = e.modl_digitize(torch.as_tensor(edges, device=e.device), half=True)
    nids, norm = edges.size + 1, q.geom.area / float(e.npix) ** 2
    drv0 = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=seed)
    ref_b, stack = [], 0
    for i in range(nsims):
        kap = q.reconstruct_tt_hc(e.grf_hc(seed, i, drv0.cs), fused=False)
        sums, counts = e.bin_power(kap, kap, norm, ids, nids)
        ref_b.append((sums.cpu().numpy() / counts.cpu().numpy())[1:-1])
        stack = stack + kap.to(torch.complex128).cpu().numpy()
    ref_b = np.array(ref_b)
    tol = 1e-10 if prec == "f64" else 2e-5
    st = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=seed, mean_field=True).run(nsims)
    assert st.count("n0") == nsims
    np.testing.assert_allclose(st.mean("n0"), ref_b.mean(0), rtol=tol)
    np.testing.assert_allclose(st.cov("n0"), np.cov(ref_b.T), rtol=50 * tol, atol=50 * tol * np.abs(np.cov(ref_b.T)).max())
    mf = st.stack_sum("mf")
    mfk = (mf[..., 0] + 1j * mf[..., 1])[:, :nx // 2 + 1]
    low = ml[:, :nx // 2 + 1] < 1.8 * tl[1]
    ref = stack[:, :nx // 2 + 1]
    assert np.abs(mfk - ref)[low].max() <= tol * np.abs(ref[low]).max()
    # outside kappa's band the stack holds nothing
    ky = np.fft.fftfreq(shape[0], 1.0 / shape[0])
    outside = ~((np.abs(ky)[:, None] < q.kappa_rows) & (np.arange(nx // 2 + 1)[None, :] < q.kappa_cols))
    assert np.abs(mfk[outside]).max() == 0.0


def test_power_of_two_set_filters_refuses_bands_beyond_the_plane():
    """oa_plan_set_filters on a power-of-two plan refuses kappa / leg columns beyond nx / 2 + 1 and rows beyond the plane (the inner
    plans of the band grid are such plans), and still binds the estimator's own bands."""
    from orphics_amd.engine import _ptr
    (g, th, ml, beam, noise, tmask, kmask, cl, tmap) = _setup((256, 256), 2.0, (300, 2000), (20, 3500), seed=5)
    from orphics_amd import lensing
    q = lensing.qest((256, 256), g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f64")
    e = q.eng
    assert e.pow2
    FG, FH, Fn = q._F["TT"]
    (wl, wk), (rl, rk) = q._W["TT"], q._R["TT"]
    for args, words in (((wl, 130, rl, rk), "columns"), ((130, wk, rl, rk), "columns"), ((wl, wk, rl, 129), "rows"), ((wl, wk, 129, rk), "rows")):
        rc = e.lib.oa_plan_set_filters(e.plan, _ptr(FG), _ptr(FH), _ptr(Fn), *[int(a) for a in args], int(q.mrow))
        assert rc != 0 and words in e.lib.oa_last_error().decode()
    assert e.lib.oa_plan_set_filters(e.plan, _ptr(FG), _ptr(FH), _ptr(Fn), int(wl), int(wk), int(rl), int(rk), int(q.mrow)) == 0
    e._pipe_owner = None
