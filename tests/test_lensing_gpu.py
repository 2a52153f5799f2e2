"""GPU parity of the TT quadratic estimator vs oracle/qe_oracle.py (float64
NumPy).  Tolerances: f64 kernels 1e-9 on kappa modes, f32 kernels 1e-5 on the
binned kappa bandpowers (BASELINE.json north_star)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import maps_oracle as mo  # noqa: E402
from oracle import qe_oracle as qo  # noqa: E402
from oracle import stats_oracle as so  # noqa: E402


def setup(N, res_arcmin, seed=0, tlmax=2000):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (N, N)
    g = FlatGeometry.from_res(shape, res_arcmin)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=tlmax)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    cl = th.lCl("TT", ml)
    rng = np.random.default_rng(seed)
    tk = np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cl * beam ** 2 + noise) / g.pixarea)
    t1 = np.fft.ifft2(tk).real
    tk = np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cl * beam ** 2 + noise) / g.pixarea)
    t2 = np.fft.ifft2(tk).real
    return shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2


@pytest.mark.parametrize("N,res", [(128, 4.0), (512, 1.0)])
def test_tt_normalisation_and_recon_f64(N, res):
    from orphics_amd import lensing
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype="f64")
    qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    sel = (ml > 20) & (ml < 3500) & (qr.R != 0)
    Rf = q._full(q.R_TT)
    assert np.max(np.abs(Rf[sel] / qr.R[sel] - 1)) < 1e-9
    NL = q.N_kappa("TT")
    assert np.max(np.abs(NL[sel] / qr.Nlkk[sel] - 1)) < 1e-9
    rec = q.kappa_from_map("TT", t1)
    ref = qr.kappa_from_map("TT", t1)
    assert np.abs(rec - ref).max() / np.abs(ref).max() < 1e-9
    # distinct legs, FT in / FT out (SplitLensing contract)
    k1, k2 = np.fft.fft2(t1), np.fft.fft2(t2)
    kft = q.kappa_from_map("TT", k1, T2DDataY=k2, alreadyFTed=True, returnFt=True)
    kref = qr.kappa_from_map("TT", k1, T2DDataY=k2, alreadyFTed=True, returnFt=True)
    assert np.abs(kft - kref).max() / np.abs(kref).max() < 1e-9


@pytest.mark.parametrize("N,res", [(512, 1.0), (1024, 0.5)])
def test_tt_bandpowers_f32_within_1e5(N, res):
    from orphics_amd import lensing, maps, stats
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=1)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype="f32")
    qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    edges = np.linspace(20, 3500, 20)
    bo = so.bin2D(ml, edges)
    fo = mo.FourierCalc(shape, g.step_y, g.step_x)
    kref = qr.kappa_from_map("TT", t1, returnFt=True)
    _, pref = bo.bin(fo.f2power(kref, kref))
    # device-native path: real map (cuda f32) -> HalfPlane kappa FT -> half-plane binning
    fc = maps.FourierCalc(shape, g, layout="half")
    binner = stats.bin2D(ml, edges)
    assert np.array_equal(binner.digitized, bo.digitized)
    kT = fc.fft(torch.as_tensor(t1.astype(np.float32)).cuda())
    kk = q.kappa_from_map("TT", kT, alreadyFTed=True, returnFt=True)
    _, p1 = binner.bin(fc.f2power(kk, kk))
    assert np.max(np.abs(p1 / pref - 1)) < 1e-5
    # numpy drop-in path
    rec = q.kappa_from_map("TT", t1.astype(np.float32))
    _, p2 = binner.bin(maps.FourierCalc(shape, g).power2d(np.asarray(rec, np.float64))[0])
    assert np.max(np.abs(p2 / pref - 1)) < 1e-5


def test_n0_of_gaussian_sims_matches_AL():
    """MC N0 on unlensed Gaussian maps equals the analytic N_L^kk from A_L."""
    from orphics_amd import lensing, maps, stats
    N, res = 256, 2.0
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=5)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype="f32")
    fc = maps.FourierCalc(shape, g, layout="half")
    edges = np.linspace(100, 3000, 12)
    binner = stats.bin2D(ml, edges)
    rng = np.random.default_rng(11)
    acc = 0
    nsim = 40
    for i in range(nsim):
        tk = np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cl * beam ** 2 + noise) / g.pixarea)
        t = np.fft.ifft2(tk).real.astype(np.float32)
        kk = q.kappa_from_map("TT", fc.fft(torch.as_tensor(t).cuda()), alreadyFTed=True, returnFt=True)
        acc = acc + binner.bin(fc.f2power(kk, kk))[1]
    _, nl = binner.bin(q.N_kappa("TT"))
    assert np.max(np.abs(acc / nsim / nl - 1)) < 0.08


def test_split_lensing_cross_estimator_matches_numpy():
    """Device path (one oa_qe_tt_splits call + oa_split_cross_power) vs the reference's ordering of the estimator
    (oracle/qe_oracle.split_cross_estimator, pinned by tests/golden/splits_reference.npz) evaluated with the oracle QE."""
    from orphics_amd import lensing
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(128, 4.0, seed=7)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype="f64")
    qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    fo = mo.FourierCalc(shape, g.step_y, g.step_x)
    rng = np.random.default_rng(8)
    for n in (4, 5):
        splits = np.array([np.fft.fft2(t1 + 0.3 * rng.standard_normal(shape)) for _ in range(n)])
        sl = lensing.SplitLensing(shape, g, q, "TT")
        got = sl.cross_estimator(splits)
        assert isinstance(got, np.ndarray) and got.shape == shape
        ref = qo.split_cross_estimator(lambda a, b: qr.kappa_from_map("TT", a, T2DDataY=b, alreadyFTed=True, returnFt=True),
                                       fo.f2power, splits)
        assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-8


class _DuckQest(object):
    """Any object with kappa_from_map is a valid qest for SplitLensing (lensing.py:961-976)."""

    def __init__(self, fn):
        self.fn = fn
        self.calls = 0

    def kappa_from_map(self, XY, T2DData=None, T2DDataY=None, alreadyFTed=False, returnFt=False, **unused):
        assert XY == "TT" and alreadyFTed and returnFt
        self.calls += 1
        return self.fn(T2DData, T2DDataY)


def test_split_estimators_match_the_reference_functions():
    """SplitLensing.cross_estimator with a caller-supplied qest, and maps.split_calc, vs outputs of the REFERENCE's own
    definitions (tests/golden/splits_reference.npz; lensing.py:980-1003, maps.py:2296-2333)."""
    import os
    from orphics_amd import lensing, maps
    from orphics_amd.geometry import FlatGeometry
    gd = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splits_reference.npz"))
    U, V = gd["U"], gd["V"]
    shape = U.shape
    geo = FlatGeometry.from_res(shape, 2.0)
    for n in (4, 5, 6):
        duck = _DuckQest(lambda a, b: U * a * b + V * a * np.roll(b, (1, 2), (0, 1)))
        sl = lensing.SplitLensing(shape, geo, duck, "TT")
        sl.fc.normfact = float(gd["normfact"])
        got = sl.cross_estimator(gd["cross_splits_%d" % n])
        want = gd["cross_out_%d" % n]
        assert duck.calls == n * n                         # pairwise reconstructions only (reference: 1 + 3n + n(n-1))
        assert np.abs(got - want).max() < 1e-11 * np.abs(want).max()
    fc = maps.FourierCalc(shape, geo)
    fc.normfact = float(gd["normfact"])
    isp, jsp = gd["sc_isplits"], gd["sc_jsplits"]
    for alt, tag in ((True, "alt"), (False, "loop")):
        t, c, nz = maps.split_calc(isp, jsp, isp.mean(0), jsp.mean(0), fourier_calc=fc, alt=alt)
        for got, key in ((t, "sc_total_"), (c, "sc_crosses_"), (nz, "sc_noise_")):
            want = gd[key + tag]
            assert np.abs(np.asarray(got) - want).max() < 1e-12 * np.abs(want).max(), (tag, key)


@pytest.mark.parametrize("prec,tol", [("f64", 1e-9), ("f32", 2e-3)])
def test_split_device_path_equals_pairwise_calls(prec, tol):
    """oa_qe_tt_splits (each split's leg planes transformed once) returns the same K_ij as n^2 separate two-leg
    reconstructions, and the one-launch combination equals the generic host combination of those planes."""
    from orphics_amd import lensing
    from orphics_amd.stats import HalfPlane
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(256, 2.0, seed=5)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype=prec)
    e = q.eng
    rng = np.random.default_rng(9)
    n = 5
    maps_ = [t1 + 0.3 * rng.standard_normal(shape) for _ in range(n)]
    hcs = [e.rfft(e.to_real(m)) for m in maps_]
    K = q.tt_pairs(hcs)
    for i, j in ((0, 0), (1, 3), (4, 2)):
        one = q.reconstruct_tt_hc(hcs[i], hcs[j]).clone()
        assert torch.equal(K[i, j], one)                   # same kernels on the same inputs: bit-identical
    buf = torch.full_like(K, 7.0)                          # a caller-owned (dirty) output block is zero-filled outside
    assert torch.equal(q.tt_pairs(hcs, out=buf), K)
    sl = lensing.SplitLensing(shape, g, q, "TT")
    half = HalfPlane(torch.stack(hcs), e)
    dev = sl.cross_estimator(half)
    assert isinstance(dev, HalfPlane)
    duck = _DuckQest(lambda a, b: q.kappa_from_map("TT", T2DData=a, T2DDataY=b, alreadyFTed=True, returnFt=True))
    gen = lensing.SplitLensing(shape, g, duck, "TT").cross_estimator(half)
    assert duck.calls == n * n
    a, b = dev.t.double(), gen.t.double()
    assert float((a - b).abs().max() / b.abs().max()) < tol


@pytest.mark.parametrize("prec,tol", [("f64", 1e-11), ("f32", 2e-5)])
@pytest.mark.parametrize("N", [64, 512, 2048])
def test_fused_pipeline_equals_modular(N, prec, tol):
    """oa_fft_cols + oa_qe_rows (fused row stage) == the modular C2R / product / R2C sequence."""
    from orphics_amd import lensing
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, 1.0 * 512 / N if N < 512 else 1.0, seed=3)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype=prec)
    e = q.eng
    k1 = e.rfft(e.to_real(t1)); k2 = e.rfft(e.to_real(t2))
    a = q.reconstruct_tt_hc(k1, k2, fused=True).clone()
    b = q.reconstruct_tt_hc(k1, k2, fused=False).clone()
    w = N // 2 + 1
    a, b = a.cpu().numpy()[:, :w], b.cpu().numpy()[:, :w]
    assert np.abs(a - b).max() / np.abs(b).max() < tol


def test_mc_driver_n0_and_mean_field():
    """GaussianN0MonteCarlo: device GRFs -> TT QE -> bandpower moments (+ mean-field stack);
    the MC N0 equals the analytic N_L^kk, moments equal a host recomputation."""
    from orphics_amd import lensing, mc, stats
    N, res = 256, 2.0
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=2)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype="f32")
    tot_h = (cl * beam ** 2 + noise)[:, :N // 2 + 1]
    edges = np.linspace(100, 3000, 12)
    drv = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=77, mean_field=True)
    st = drv.run(48)
    assert st.count("n0") == 48 and st.stack_count("mf") == 48
    _, nl = stats.bin2D(ml, edges).bin(q.N_kappa("TT"))
    assert np.max(np.abs(st.mean("n0") / nl - 1)) < 0.08
    assert st.cov("n0").shape == (11, 11) and np.all(np.diag(st.cov("n0")) > 0)
    # same seeds -> identical moments (counter-based RNG, deterministic binning)
    st2 = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=77).run(48)
    np.testing.assert_allclose(st2.mean("n0"), st.mean("n0"), rtol=0, atol=0)
    # mean field of Gaussian sims is consistent with zero: |<kappa_hat>|^2 ~ N0 / nsims
    mf = st.stack_sum("mf")
    mfk = (mf[..., 0] + 1j * mf[..., 1])[:, :N // 2 + 1] / 48.0
    p_mf = np.abs(mfk) ** 2 * (g.area / float(N * N) ** 2)
    sel = (ml[:, :N // 2 + 1] > 300) & (ml[:, :N // 2 + 1] < 2500)
    ratio = p_mf[sel].mean() / (q.N_kappa("TT")[:, :N // 2 + 1][sel].mean() / 48.0)
    assert 0.7 < ratio < 1.3


def test_windowed_monte_carlo_mean_field_matches_oracle_on_the_same_maps():
    """A Monte-Carlo run with a real-space taper (maps.get_taper: the reference's analysis flow, maps.py:1350-1361,
    1873-1878): (i) window == 1 reproduces the unwindowed driver (the band draw is a subset of the full-plane draw);
    (ii) with the taper, the stacked mean field equals the NumPy oracle's on the SAME maps (same Philox draws, C2R, taper,
    fed to oracle.QEOracleTT) and is far larger than the unwindowed one; (iii) bandpowers / mean(w^4) stay near N0."""
    from orphics_amd import lensing, maps, mc
    N, res = 512, 1.0
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=2)
    nsims = 12
    tot = cl * beam ** 2 + noise
    tot_h = tot[:, :N // 2 + 1]
    edges = np.linspace(100, 3000, 12)
    taper, w2 = maps.get_taper(shape, g, taper_percent=12.0, pad_percent=3.0)
    for prec, tol in (("f64", 1e-9), ("f32", 2e-4)):
        q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype=prec)
        e = q.eng
        plain = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=5, mean_field=True).run(nsims)
        ones = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=5, mean_field=True, window=np.ones(shape)).run(nsims)
        np.testing.assert_allclose(ones.mean("n0"), plain.mean("n0"), rtol=(1e-10 if prec == "f64" else 2e-5))
        drv = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=5, mean_field=True, window=taper)
        assert abs(drv.window_moments[0] - w2) < 1e-15
        st = drv.run(nsims)
        assert st.count("n0") == nsims and st.stack_count("mf") == nsims
        mf = st.stack_sum("mf")
        mfk = (mf[..., 0] + 1j * mf[..., 1])[:, :N // 2 + 1] / nsims
        # the oracle on the same maps: the driver's draw (key = (base_seed, sim)), C2R / Npix, taper
        qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
        ref = 0
        for i in range(nsims):
            m = e.irfft(e.grf_hc(5, i, drv.cs)).double().cpu().numpy() * taper
            ref = ref + qr.kappa_from_map("TT", m, returnFt=True)[:, :N // 2 + 1]
        ref = ref / nsims
        sel = (ml[:, :N // 2 + 1] > 40) & (ml[:, :N // 2 + 1] < 3000)
        assert np.abs(mfk - ref)[sel].max() < tol * np.abs(ref[sel]).max()
        # the window's mean field dwarfs the noise-only "mean field" of the unwindowed run at low L
        pm = plain.stack_sum("mf")
        pmk = (pm[..., 0] + 1j * pm[..., 1])[:, :N // 2 + 1] / nsims
        low = (ml[:, :N // 2 + 1] > 20) & (ml[:, :N // 2 + 1] < 200)
        assert np.mean(np.abs(mfk[low]) ** 2) > 20 * np.mean(np.abs(pmk[low]) ** 2)
        # bandpowers: the mean field dominates the lowest bands; above L ~ 1000 the debiased level is N0 within MC scatter
        hi = drv.centers > 1000
        assert np.all(np.abs(drv.debiased_mean()[hi] / plain.mean("n0")[hi] - 1) < 0.5)


def test_mc_driver_on_several_streams_equals_one_stream():
    """streams=3 splits a rank's simulations over three HIP streams (forked estimator handles, private accumulators
    summed at the end): same realisations, same moments and mean-field stack up to summation order."""
    from orphics_amd import lensing, mc
    N, res = 512, 1.0
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=2)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f32")
    tot_h = (cl * beam ** 2 + noise)[:, :N // 2 + 1]
    edges = np.linspace(100, 3000, 12)
    a = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=5).run(40)
    drv = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=5, streams=3)
    b = drv.run(40)
    assert getattr(drv, "_lanes", None) is not None and len(drv._lanes) == 3
    assert a.count("n0") == b.count("n0") == 40
    np.testing.assert_allclose(b.mean("n0"), a.mean("n0"), rtol=1e-12)
    np.testing.assert_allclose(b.cov("n0"), a.cov("n0"), rtol=1e-9, atol=1e-30)
    # the windowed flow (oa_mc_run_windowed) on three lanes, with the mean-field stack
    from orphics_amd import maps
    taper, _ = maps.get_taper(shape, g, taper_percent=12.0, pad_percent=3.0)
    aw = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=6, mean_field=True, window=taper).run(30)
    dw = mc.GaussianN0MonteCarlo(q, tot_h, edges, base_seed=6, mean_field=True, window=taper, streams=3)
    bw = dw.run(30)
    assert getattr(dw, "_lanes", None) is not None and aw.count("n0") == bw.count("n0") == 30 and bw.stack_count("mf") == 30
    np.testing.assert_allclose(bw.mean("n0"), aw.mean("n0"), rtol=1e-12)
    sa, sb = aw.stack_sum("mf"), bw.stack_sum("mf")
    assert np.abs(sa - sb).max() < 1e-5 * np.abs(sa).max()


def pol_setup(N, res_arcmin, seed=0):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (N, N) if np.isscalar(N) else tuple(N)
    g = FlatGeometry.from_res(shape, res_arcmin)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    nP = 2 * nT
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3000)
    cl = {k: th.lCl(k, ml) for k in ("TT", "EE", "BB", "TE")}
    rng = np.random.default_rng(seed)
    sc = 1.0 / np.sqrt(g.pixarea)
    # correlated T,E + independent B Gaussian observed fields (beam-convolved + noise), as DFTs
    w1, w2, w3 = (np.fft.fft2(rng.standard_normal(shape)) for _ in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.nan_to_num(cl["TE"] / np.sqrt(cl["TT"] * cl["EE"]))
    kT = w1 * np.sqrt(cl["TT"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nT) * sc
    kE = (r * w1 + np.sqrt(1 - r ** 2) * w2) * np.sqrt(cl["EE"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nP) * sc
    kB = w3 * np.sqrt(cl["BB"]) * beam * sc + np.fft.fft2(rng.standard_normal(shape)) * np.sqrt(nP) * sc
    return shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, dict(T=kT, E=kE, B=kB)


@pytest.mark.parametrize("XY", ["TT", "EE", "EB", "TE", "TB"])
def test_pol_estimators_match_oracle(XY):
    """Device general estimators (f64 kernels) vs oracle.QEOracle: response, N0 and kappa_hat DFT;
    f32 kernels: kappa bandpowers within 1e-5."""
    from orphics_amd import lensing, maps, stats
    N, res = 128, 2.0
    shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, k = pol_setup(N, res, seed=4)
    qr = qo.QEOracle(shape, g.step_y, g.step_x, cl, dict(T=nT, P=nP), beam, dict(T=tmask, P=tmask), kmask_K=kmask)
    qr.setup(XY)
    X, Y = XY[0], XY[1]
    kref = qr.kappa_ft(XY, k[X], k[Y])
    kw = dict(noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask, kmask_K=kmask, pol=True,
              unlensed_equals_lensed=True)
    q = lensing.qest(shape, g, th, dtype="f64", **kw)
    args = dict(T2DData=k["T"], E2DData=k["E"], B2DData=k["B"], alreadyFTed=True, returnFt=True)
    got = q.kappa_from_map(XY, **args)
    sel = (ml > 40) & (ml < 2900) & (qr.R[XY] != 0)
    Rf = q._full(q._gen[XY]["R"]) if XY != "TT" else q._full(q.R_TT)
    assert np.max(np.abs(Rf[sel] / qr.R[XY][sel] - 1)) < 1e-8
    assert np.max(np.abs(q.N_kappa(XY)[sel] / qr.Nlkk[XY][sel] - 1)) < 1e-7
    assert np.abs(got - kref)[sel].max() / np.abs(kref[sel]).max() < 1e-8
    q32 = lensing.qest(shape, g, th, dtype="f32", **kw)
    got32 = q32.kappa_from_map(XY, **{kk: (v.astype(np.complex64) if isinstance(v, np.ndarray) else v) for kk, v in args.items()})
    edges = np.linspace(40, 2900, 16)
    bo = so.bin2D(ml, edges)
    fo = mo.FourierCalc(shape, g.step_y, g.step_x)
    _, pref = bo.bin(fo.f2power(kref, kref))
    _, p32 = stats.bin2D(ml, edges).bin(maps.FourierCalc(shape, g).f2power(got32.astype(np.complex128), got32.astype(np.complex128)))
    assert np.max(np.abs(p32 / pref - 1)) < 1e-5


def test_mv_combination_matches_oracle():
    """BASELINE config 3 shape (TT/EE/EB/TE/TB minimum-variance combination) at test size."""
    from orphics_amd import lensing
    N, res = 128, 2.0
    shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, k = pol_setup(N, res, seed=9)
    qr = qo.QEOracle(shape, g.step_y, g.step_x, cl, dict(T=nT, P=nP), beam, dict(T=tmask, P=tmask), kmask_K=kmask)
    ref = qr.kappa_mv_ft(k)
    for prec, tol in (("f64", 1e-8), ("f32", 3e-4)):
        q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask, kmask_K=kmask,
                         pol=True, unlensed_equals_lensed=True, dtype=prec)
        e = q.eng
        hk = {X: e.full_to_hc(e.to_complex(k[X])) for X in "TEB"}
        got = e.hc_to_full(q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"])).cpu().numpy()
        sel = (ml > 40) & (ml < 2900)
        assert np.abs(got - ref)[sel].max() / np.abs(ref[sel]).max() < tol
        nmv = q._full(q.Nlkk["MV"])
        assert np.max(np.abs(nmv[sel & (qr.Nlkk["MV"] > 0)] / qr.Nlkk["MV"][sel & (qr.Nlkk["MV"] > 0)] - 1)) < 1e-6
        assert np.all(nmv[sel] <= q.N_kappa("TT")[sel] * (1 + 1e-9))   # MV is never noisier than TT


def test_pol_and_mv_match_oracle_with_row_and_column_grids_engaged():
    """TE / EE / EB / TB / TT through the batched general path (``reconstruct_hc`` -> oa_qe_mv with one estimator) and the
    five-estimator MV combination (``reconstruct_mv_hc`` -> one oa_qe_mv call), at 2048^2 1' where the band limits put the
    row stage on a 1024-point row grid and the column stages on a 1024-row column grid -- against oracle.QEOracle on the
    same Gaussian T, E, B: kappa bandpowers within 1e-5 (f32 kernels) / 1e-8 (f64 kernels)."""
    from orphics_amd import lensing
    N, res = 2048, 1.0
    shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, k = pol_setup(N, res, seed=14)
    mo.set_workers(16)
    qr = qo.QEOracle(shape, g.step_y, g.step_x, cl, dict(T=nT, P=nP), beam, dict(T=tmask, P=tmask), kmask_K=kmask)
    ests = ("TT", "TE", "EE", "EB", "TB")
    edges = np.linspace(40, 2900, 16)
    bo = so.bin2D(ml, edges)
    fo = mo.FourierCalc(shape, g.step_y, g.step_x)
    pref = {}
    for XY in ests:
        qr.setup(XY)
        kr = qr.kappa_ft(XY, k[XY[0]], k[XY[1]])
        pref[XY] = bo.bin(fo.f2power(kr, kr))[1]
    kr = qr.kappa_mv_ft(k, ests)
    pref["MV"] = bo.bin(fo.f2power(kr, kr))[1]
    mo.set_workers(1)
    kw = dict(noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask, kmask_K=kmask, pol=True, unlensed_equals_lensed=True)
    q64 = lensing.qest(shape, g, th, dtype="f64", **kw)
    for prec, tol in (("f64", 1e-8), ("f32", 1e-5)):
        q = q64 if prec == "f64" else q64.astype("f32")
        e = q.eng
        hk = {X: e.full_to_hc(e.to_complex(k[X])) for X in "TEB"}
        ids = e.modl_digitize(torch.as_tensor(edges, device=e.device), half=True)
        _, counts = e.bin_power(hk["T"], hk["T"], 1.0, ids, len(edges) + 1, herm=True)
        assert np.array_equal(counts[1:-1].cpu().numpy(), np.bincount(bo.digitized, minlength=len(edges) + 1)[1:len(edges)])

        def bandpowers(kk):
            sums, _ = e.bin_power(kk, kk, g.area / float(N * N) ** 2, ids, len(edges) + 1, herm=True)
            return (sums[1:-1] / counts[1:-1].double()).cpu().numpy()
        for XY in ests:
            kk = q.reconstruct_hc(XY, hk[XY[0]], hk[XY[1]])
            G = q._gen[XY]
            # both grids engaged: a 1024-point row grid and a 1024-row column grid hold the band-limited products exactly
            assert 0 < 2 * G["wl"] + G["wk"] <= 1024 and 0 < max(2 * G["rl"] + G["rk"], 2 * G["rk"]) <= 1024, (XY, G["wl"], G["wk"], G["rl"], G["rk"])
            err = np.max(np.abs(bandpowers(kk) / pref[XY] - 1))
            assert err < tol, "%s %s: bandpowers differ from the oracle by %.3g" % (XY, prec, err)
        kk = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"], ests)
        err = np.max(np.abs(bandpowers(kk) / pref["MV"] - 1))
        assert err < tol, "MV %s: bandpowers differ from the oracle by %.3g" % (prec, err)
        # an estimator set up on the converted handle AFTER astype must not pick up planes of the other precision
        if prec == "f32":
            fresh = lensing.qest(shape, g, th, dtype="f32", **kw)
            for a_, b_ in zip(q._gen["EB"]["pieces"], fresh._setup_general("EB")["pieces"]):
                assert a_[1].dtype == torch.float32 and a_[2].dtype == torch.float32
                assert torch.equal(a_[1], b_[1]) and torch.equal(a_[2], b_[2])


def test_estimator_set_up_after_astype_uses_its_own_precision():
    """q64 set up for EE, then q64.astype('f32') set up for EB (which shares the W^EE filtered fields with EE): the f32
    handle must build / convert f32 planes (its own tag cache), and the f64 handle's cache must stay f64."""
    from orphics_amd import lensing
    N, res = 256, 2.0
    shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, k = pol_setup(N, res, seed=3)
    kw = dict(noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask, kmask_K=kmask, pol=True, unlensed_equals_lensed=True)
    q64 = lensing.qest(shape, g, th, dtype="f64", **kw)
    q64._setup_general("EE")
    q32 = q64.astype("f32")
    e = q32.eng
    hk = {X: e.full_to_hc(e.to_complex(k[X].astype(np.complex64))) for X in "EB"}
    got = q32.reconstruct_hc("EB", hk["E"], hk["B"])
    fresh = lensing.qest(shape, g, th, dtype="f32", **kw)
    ref = fresh.reconstruct_hc("EB", hk["E"], hk["B"])
    assert all(t.dtype == torch.float32 for t in q32._fdev.values())
    assert all(t.dtype == torch.float64 for t in q64._fdev.values())
    assert (got - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    # and the f64 handle still reconstructs EB with f64 planes afterwards
    e64 = q64.eng
    hk64 = {X: e64.full_to_hc(e64.to_complex(k[X])) for X in "EB"}
    got64 = q64.reconstruct_hc("EB", hk64["E"], hk64["B"])
    assert (got64.to(torch.complex64) - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


@pytest.mark.parametrize("N,res,prune,masks", [(128, 2.0, True, "same"), (512, 1.0, True, "differ"), (256, 2.0, False, "same"), (1024, 1.0, True, "same")])
def test_mv_one_call_equals_per_estimator_calls(N, res, prune, masks):
    """oa_qe_mv (every distinct filtered field transformed once, one inverse pass-2 launch over all leg planes) vs one
    oa_qe_pol call per estimator: the same kernels on the same operands piece by piece."""
    from orphics_amd import lensing
    shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, k = pol_setup(N, res, seed=4)
    pmask = tmask if masks == "same" else ((ml > 200) & (ml < 1400)).astype(tmask.dtype)      # different T / P leg bands
    for prec, tol in (("f64", 1e-12), ("f32", 1e-5)):
        q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=pmask, kmask_K=kmask,
                         pol=True, unlensed_equals_lensed=True, dtype=prec, prune=prune)
        e = q.eng
        hk = {X: e.full_to_hc(e.to_complex(k[X])) for X in "TEB"}
        one = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"]).clone()
        per = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"], fused=False).clone()
        assert float((one - per).abs().max() / per.abs().max()) < tol
        shared = len({pc[1].data_ptr() for XY in ("TT", "TE", "EE", "EB", "TB") for pc in q._gen[XY]["pieces"]})
        assert shared == 6                                  # W^TT T; W^TE T cos, sin; W^EE E cos, sin; W^ET E: 6 gradient fields for 10 pieces
        dirty = torch.full_like(one, 3.0)                   # caller-owned plane: zero-filled outside kappa's region
        again = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"], out=dirty)
        assert torch.equal(again[:, :e.nxh + 1], one[:, :e.nxh + 1])       # (columns beyond nx/2 are row padding)
        e.set_option("mv_batch", 0)                  # one leg launch per distinct field instead of one for all
        try:
            per_field = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"]).clone()
        finally:
            e.set_option("mv_batch", 1)
        # (the one-call default sums an estimator's pieces in REAL space inside one row-stage launch -- estimator chains --, the
        # switched-off paths accumulate them in Fourier space piece by piece: equal to rounding, not bit for bit)
        assert float((per_field - one).abs().max() / one.abs().max()) < tol
        e.set_option("mv_rowbatch", 0)               # one row-stage launch per piece instead of one per estimator chain
        try:
            per_piece = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"]).clone()
        finally:
            e.set_option("mv_rowbatch", 1)
        assert float((per_piece - one).abs().max() / one.abs().max()) < tol
        e.set_option("mv_chain", 0)                  # the k-th piece of every estimator per launch, accumulating: bit-identical to per-piece launches
        try:
            ranked = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"]).clone()
        finally:
            e.set_option("mv_chain", 1)
        assert torch.equal(ranked, per_piece)
        sub = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"], estimators=("TT", "EB")).clone()
        sub_per = q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"], estimators=("TT", "EB"), fused=False).clone()
        assert float((sub - sub_per).abs().max() / sub_per.abs().max()) < tol


def test_flat_lensing_op_matches_oracle_and_remaps():
    """kappa -> phi -> alpha and the FFT-only Taylens (lensing.py:395-454,651-665) vs the NumPy restatement;
    a constant one-pixel displacement is an exact roll."""
    from orphics_amd import lensing
    from orphics_amd.geometry import FlatGeometry
    N = 128
    g = FlatGeometry.from_res((N, N), 2.0)
    rng = np.random.default_rng(21)
    ml = g.modlmap()
    kap = np.fft.ifft2(np.fft.fft2(rng.standard_normal((N, N))) * 1.5 / (1 + (ml / 200.) ** 2)).real
    T = np.fft.ifft2(np.fft.fft2(rng.standard_normal((N, N))) / (1 + (ml / 400.) ** 2)).real
    L = lensing.FlatLenser((N, N), g, dtype="f64")
    ay, ax = L.alpha_from_kappa(kap)
    ray, rax = qo.alpha_from_kappa(kap, g.step_y, g.step_x)
    assert np.abs(ay.cpu().numpy() - ray).max() < 1e-12 * np.abs(ray).max() + 1e-18
    assert np.abs(ax.cpu().numpy() - rax).max() < 1e-12 * np.abs(rax).max() + 1e-18
    assert np.abs(ray).max() / abs(g.step_y) > 0.5        # a real multi-pixel test
    lensed = L.lens(T, (ay, ax), taylor_order=5).cpu().numpy()
    ref = qo.flat_taylens((ray, rax), T, g.step_y, g.step_x, taylor_order=5)
    assert np.abs(lensed - ref).max() / np.abs(ref).max() < 1e-10
    # the fused path (one derivative kernel for all 14 terms, one gather pass) against the term-by-term one, and a lower order
    per_term = L.lens(T, (ay, ax), taylor_order=5, fused=False).cpu().numpy()
    assert np.abs(lensed - per_term).max() / np.abs(ref).max() < 1e-12
    # the fine-grained C-ABI sequence oa_lens_maps replaces (oa_hc_derivs -> C2R per term -> oa_lens_taylor): same result; and
    # several maps per call (T, 2 T, -T by the same deflection) == one map per call
    from orphics_amd._lib import check
    from orphics_amd.engine import _ptr, _stream
    e = L.eng
    sx, sy, dx, dy = L.split((ay, ax))
    src = e.to_real(T)
    dk = torch.empty((14, e.ny, e.kp), dtype=e.cdt, device=e.device)
    dr = torch.empty((14, e.ny, e.nx), dtype=e.rdt, device=e.device)
    check(e.lib.oa_hc_derivs(e.plan, _ptr(e.rfft(src)), 5, _ptr(dk), e.ny * e.kp, _stream()))
    for i in range(14):
        e.irfft(dk[i], out=dr[i])
    fine = e.real()
    check(e.lib.oa_lens_taylor(e.plan, _ptr(src), _ptr(dr), e.ny * e.nx, 5, _ptr(sx), _ptr(sy), _ptr(dx), _ptr(dy), _ptr(fine), _stream()))
    assert np.abs(fine.cpu().numpy() - lensed).max() / np.abs(ref).max() < 1e-13
    three = L.lens_many(torch.stack([src, 2 * src, -src]), (ay, ax), taylor_order=5).cpu().numpy()
    assert np.abs(three[0] - lensed).max() / np.abs(ref).max() < 1e-14
    assert np.abs(three[1] - 2 * lensed).max() / np.abs(ref).max() < 1e-13 and np.abs(three[2] + lensed).max() / np.abs(ref).max() < 1e-14
    L.release()                                                 # the plan-owned planes come back on the next call
    assert np.abs(L.lens(T, (ay, ax), taylor_order=5).cpu().numpy() - lensed).max() == 0
    ref3 = qo.flat_taylens((ray, rax), T, g.step_y, g.step_x, taylor_order=3)
    assert np.abs(L.lens(T, (ay, ax), taylor_order=3).cpu().numpy() - ref3).max() / np.abs(ref3).max() < 1e-10
    L32 = lensing.FlatLenser((N, N), g, dtype="f32")
    a32 = (ay.float(), ax.float())
    assert np.abs(L32.lens(T.astype(np.float32), a32).cpu().numpy() - ref).max() / np.abs(ref).max() < 2e-5
    torch_ = torch
    one_y = torch_.full((N, N), g.step_y, dtype=torch_.float64, device="cuda")
    one_x = torch_.full((N, N), 2 * g.step_x, dtype=torch_.float64, device="cuda")
    rolled = L.lens(T, (one_y, one_x)).cpu().numpy()
    assert np.allclose(rolled, np.roll(np.roll(T, -1, axis=0), -2, axis=1), atol=1e-12)
    # a second deflection written INTO THE SAME BUFFERS (raw-pointer writers do not bump tensor versions; the caching
    # allocator reuses freed blocks): the split follows the contents, not the addresses
    one_y.fill_(2 * g.step_y); one_x.fill_(-g.step_x)
    rolled2 = L.lens(T, (one_y, one_x)).cpu().numpy()
    assert np.allclose(rolled2, np.roll(np.roll(T, -2, axis=0), 1, axis=1), atol=1e-12)
    kap2 = -0.5 * kap
    ay2, ax2 = L.alpha_from_kappa(kap2)
    ay.copy_(ay2); ax.copy_(ax2)
    ray2, rax2 = qo.alpha_from_kappa(kap2, g.step_y, g.step_x)
    ref_b = qo.flat_taylens((ray2, rax2), T, g.step_y, g.step_x, taylor_order=5)
    assert np.abs(L.lens(T, (ay, ax)).cpu().numpy() - ref_b).max() / np.abs(ref_b).max() < 1e-10
    sp = L.split((ay, ax))                                      # explicit split shared by several maps
    assert np.abs(L.lens(2 * T, (ay, ax), split=sp).cpu().numpy() - 2 * ref_b).max() / np.abs(ref_b).max() < 1e-10


def test_tt_qe_is_unbiased_on_lensed_sims():
    """tutorials/tt_verification.ipynb criterion: mean of (C^{kappa_hat kappa} - C^{kk})/C^{kk} over lensed
    sims is consistent with 0 (here 1024^2 1' maps, 24 sims, |bias| < 6 % + 3 sigma for L < 1500)."""
    from orphics_amd import cosmology, lensing, maps, stats
    from orphics_amd.geometry import FlatGeometry
    N, res = 1024, 1.0
    shape = (N, N)
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    sims = lensing.FlatLensingSims(shape, g, th, 1.5, 1.0, dtype="f32")
    n2d = sims.ps_noise[0, 0]
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2500)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3000)
    q = lensing.qest(shape, g, th, noise2d=n2d, beam2d=sims.kbeam, kmask=tmask, kmask_K=kmask,
                     unlensed_equals_lensed=True, dtype="f32")
    fc = maps.FourierCalc(shape, g, layout="half")
    edges = np.linspace(40, 1500, 9)
    binner = stats.bin2D(ml, edges)
    st = stats.Stats()
    for i in range(24):
        unl, kappa, lensed, beamed, noise, obs = sims.get_sim(seed_cmb=(1, i), seed_kappa=(2, i), seed_noise=(3, i),
                                                              return_intermediate=True)
        kk_in = fc.fft(kappa)
        rec = q.kappa_from_map("TT", fc.fft(obs), alreadyFTed=True, returnFt=True)
        _, pc = binner.bin(fc.f2power(rec, kk_in))
        _, pi = binner.bin(fc.f2power(kk_in, kk_in))
        st.add_to_stats("ratio", (pc - pi) / pi)
    st.get_stats(verbose=False)
    y, e = st.stats["ratio"]["mean"], st.stats["ratio"]["errmean"]
    assert np.all(np.abs(y) < 0.06 + 3 * e), (y, e)
    assert abs(y.mean()) < 0.04


def test_tt_and_eb_unbiased_through_the_verifier():
    """examples/qe_unbiasedness.py (the committed verifier behind profiles/r02_unbiasedness_*.txt) at a size that
    runs in seconds: TT AND EB cross-powers with the input kappa are consistent with the input auto-power."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("qe_unbiasedness", os.path.join(root, "examples", "qe_unbiasedness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.run(nsims=16, side=512, res=1.0, estimators=("TT", "EB"), nbins=10, lrange=(40., 2500.), filt=(300., 2500.))
    assert "chi2" in mod.table(res)
    for est in ("TT", "EB"):
        r = res["estimators"][est]
        assert r["max_abs_pull"] < 4.5, (est, r["pull"])
        assert abs(r["weighted_mean_bias"]) < 0.03 + 3 * r["weighted_mean_sigma"], (est, r)
        assert r["chi2"] < 3.5 * r["nbands"]


def test_every_estimator_is_unbiased_on_lensed_sims():
    """The physical check that does not share a line with the oracle's separable-term tables: for EACH of TT, TE, EE,
    EB, TB the cross-power of kappa_hat with the input kappa on lensed simulations reproduces the input auto-power (a
    sign or convention slip in a weight table shows up as a bias of order unity)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("qe_unbiasedness", os.path.join(root, "examples", "qe_unbiasedness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ests = ("TT", "TE", "EE", "EB", "TB")
    res = mod.run(nsims=24, side=512, res=1.0, estimators=ests, nbins=8, lrange=(40., 2000.), filt=(300., 2500.))
    for est in ests:
        r = res["estimators"][est]
        assert r["max_abs_pull"] < 5.0, (est, r["pull"])
        assert abs(r["weighted_mean_bias"]) < 0.05 + 3 * r["weighted_mean_sigma"], (est, r["weighted_mean_bias"], r["weighted_mean_sigma"])
        assert r["weighted_mean_sigma"] < 0.25, (est, "no constraining power: the test would pass on anything")


def test_linear_response_normalisation_of_every_estimator():
    """The normalisation of EVERY estimator at the few-per-mille level, independent of the oracle's tables: paired
    simulations (the same CMB and noise lensed by +kappa and -kappa; the odd part of kappa_hat has no N0 scatter) with the
    UNLENSED spectra in the gradient leg (the exact first-order response) at two lensing amplitudes s = 1 and s = 1/4.
    The bias b(s) = b0 + b2 s^2: the O(kappa^3) part must scale as s^2 and the extrapolated linear-response error
    b0 = (16 b(1/4) - b(1)) / 15 must vanish: |b0| < 0.4 % + 3 sigma (profiles/r03_unbiasedness_attribution.txt has the
    4096^2 / 200-pair version: every |b0| <= 0.2 %).  A 1 % normalisation slip fails this gate."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("qe_unbiasedness", os.path.join(root, "examples", "qe_unbiasedness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ests = ("TT", "TE", "EE", "EB", "TB")
    kw = dict(nsims=32, side=2048, res=0.5, estimators=ests, nbins=12, lrange=(20., 3000.), paired=True, gradient="unlensed")
    full = mod.run(kappa_scale=1.0, **kw)["estimators"]
    quarter = mod.run(kappa_scale=0.25, **kw)["estimators"]
    for est in ests:
        b1, s1 = full[est]["weighted_mean_bias"], full[est]["weighted_mean_sigma"]
        bq, sq = quarter[est]["weighted_mean_bias"], quarter[est]["weighted_mean_sigma"]
        b0 = (16. * bq - b1) / 15.
        s0 = np.hypot(16. * sq, s1) / 15.
        assert s0 < 0.01, (est, s0, "no constraining power")
        assert abs(b0) < 0.004 + 3 * s0, (est, b0, s0)
        # the full-amplitude bias is higher-order lensing: negative, and 16 x smaller at a quarter of the amplitude (within errors)
        assert b1 < -0.01 and abs(bq - b1 / 16.) < 0.004 + 3 * np.hypot(sq, s1 / 16.), (est, b1, bq, sq)


def test_nlgenerator_against_the_reference_held_noise_curves():
    """SURVEY 8(c)-4 (sanity, not parity: the generating configurations are not in the reference tree).  The only
    reference-held numbers that speak to the estimator normalisation are the N_L^kk curves under data/
    (so_v3_1_deproj0_goal_fsky0p4_it.dat, legacy/test_mv.csv; sampled into tests/golden/nl_reference_curves.npz).
    NlGenerator for an SO-goal-like experiment (1.4' beam, 6 uK' T, sqrt(2) x that in P, ell in (30, 3000)) must reproduce
    their LEVEL within a factor of a few, the ORDERING of the estimators (MV below everything, TB far above, TT / EE / EB
    within an order of magnitude of each other) and the SHAPE (flat plateau below L ~ 300, monotonic rise above)."""
    from orphics_amd import cosmology, lensing
    from orphics_amd.geometry import FlatGeometry
    gd = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nl_reference_curves.npz"))
    ells, so_nl, cols = gd["ells"], gd["so_nl"], [str(c) for c in gd["so_columns"]]
    N, res = 1024, 2.0
    shape = (N, N)
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    edges = np.geomspace(40, 3000, 25)
    nlgen = lensing.NlGenerator(shape, g, th, edges, lensedEqualsUnlensed=True)
    nlgen.updateNoise(beamX=1.4, noiseTX=6.0, noisePX=6.0 * np.sqrt(2.), tellminX=30, tellmaxX=3000, pellminX=30, pellmaxX=3000)
    ours = {}
    for XY in ("TT", "TE", "EE", "TB", "EB"):
        ls, ours[XY] = nlgen.getNl(XY)
    ls, ours["MV"] = nlgen.getNlMV(["TT", "TE", "EE", "EB", "TB"])
    ref = {c: np.interp(ls, ells, so_nl[:, i]) for i, c in enumerate(cols)}
    band = (ls > 60) & (ls < 2000)
    for XY in ("TT", "EE", "EB", "MV"):
        ratio = ours[XY][band] / ref[XY][band]
        assert np.all(ratio > 1 / 4.) and np.all(ratio < 4.), (XY, ratio.min(), ratio.max())     # level: same normalisation convention
    for XY in ("TE", "TB"):
        ratio = ours[XY][band] / ref[XY][band]
        assert np.all(ratio > 1 / 10.) and np.all(ratio < 10.), (XY, ratio.min(), ratio.max())
    for cur in (ours, ref):
        assert np.all(cur["MV"][band] <= np.minimum.reduce([cur[x][band] for x in ("TT", "TE", "EE", "EB", "TB")]) * 1.0001)
        assert np.all(cur["TB"][band] > 10 * cur["MV"][band])
        hi = (ls > 500) & (ls < 2900)
        for XY in ("TT", "EE", "EB", "MV"):
            assert np.all(np.diff(cur[XY][hi]) > 0), XY                                        # rising above the plateau
        lo = (ls > 60) & (ls < 300)
        for XY in ("TT", "MV"):                                                                # (EE / EB leave their plateau earlier)
            assert cur[XY][lo].max() / cur[XY][lo].min() < 2.0, XY                                # plateau at low L
    # the legacy MV curve: same plateau-then-rise shape and a comparable dynamic range between L = 100 and 2900
    lm, mv = gd["legacy_mv_ells"], gd["legacy_mv"]
    dyn_ref = np.interp(2900, lm, mv) / np.interp(100, lm, mv)
    dyn_ours = np.interp(2900, ls, ours["MV"]) / np.interp(100, ls, ours["MV"])
    assert 0.2 < dyn_ours / dyn_ref < 5, (dyn_ours, dyn_ref)
    assert np.all(np.diff(mv[(lm > 300) & (lm < 2900)]) >= 0)


def test_nlgenerator_contract_and_iterative_delensing():
    """NlGenerator.getNl / getNlIterative (notebook contract), lensing-B convolution vs a direct sum."""
    from orphics_amd import cosmology, lensing, stats
    from orphics_amd.geometry import FlatGeometry
    N, res = 64, 4.0
    shape = (N, N)
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    edges = np.arange(80, 2000, 160.)
    nlgen = lensing.NlGenerator(shape, g, th, edges, lensedEqualsUnlensed=True)
    out = nlgen.updateNoise(beamX=1.5, noiseTX=1.0, noisePX=1.4, tellminX=100, tellmaxX=2400, pellminX=100, pellmaxX=2400)
    assert len(out) == 4
    ls, nl_tt = nlgen.getNl("TT")
    # oracle: same N_L from the NumPy estimator
    ml = g.modlmap()
    cl = {k: th.lCl(k, ml) for k in ("TT", "EE", "BB", "TE")}
    qr = qo.QEOracle(shape, g.step_y, g.step_x, cl, dict(T=nlgen.nT, P=nlgen.nP), nlgen.beam2d,
                     dict(T=nlgen.tmask, P=nlgen.pmask))
    qr.setup("TT"); qr.setup("EB")
    _, ref_tt = so.bin2D(ml, edges).bin(qr.Nlkk["TT"])
    np.testing.assert_allclose(nl_tt, ref_tt, rtol=1e-7)
    _, nl_eb = nlgen.getNl("EB")
    _, ref_eb = so.bin2D(ml, edges).bin(qr.Nlkk["EB"])
    np.testing.assert_allclose(nl_eb, ref_eb, rtol=1e-7)
    # lensing B-mode convolution against the O(N^4) direct sum at a few modes
    q = nlgen.q
    L = q.modl_h
    with np.errstate(divide="ignore", invalid="ignore"):
        clpp = np.nan_to_num(th.gCl("kk", L) * 4. / (L * (L + 1.)) ** 2)
    bb = q._full(nlgen.lensed_bb(q.cl_grad["EE"], clpp))
    ly, lx = g.laxes()
    lyd, lxd = ly.copy(), lx.copy(); lyd[N // 2] = 0; lxd[N // 2] = 0
    angf = -2 * np.arctan2(-lx[None, :] * np.ones((N, 1)), ly[:, None] * np.ones((1, N)))
    cleef, clppf = q._full(q.cl_grad["EE"]), q._full(clpp)
    for (yi, xi) in [(2, 3), (5, 60), (10, 0)]:
        bf = qo.lensed_bb_brute(lyd, lxd, g.area, angf, cleef, clppf, yi, xi)
        assert abs(bb[yi, xi] / bf - 1) < 1e-6   # Nyquist-row conventions differ at the 1e-7 level
    # lensing B power ~ few x 1e-6 muK^2 at low ell (white, ~5 muK-arcmin): order-of-magnitude sanity
    level = np.sqrt(bb[2, 3]) * 180 * 60 / np.pi
    assert 2.0 < level < 10.0
    ls2, nls, bells, nlbb, eff = nlgen.getNlIterative(['TT', 'TE', 'EE', 'EB', 'TB'], 80, 2000, 2400, 100, 2400, dell=200)
    assert ls2.shape == nls.shape and np.all(nls[np.isfinite(nls)] > 0)
    assert 0.0 < eff < 100.0                                # some, not all, of the lensing B power is removed
    assert np.all(nls[:4] <= nl_tt[:4] * (1 + 1e-9))         # MV never noisier than TT
    _, nl_eb_it = nlgen.getNl("EB")
    assert np.all(nl_eb_it[:4] <= nl_eb[:4] * (1 + 1e-9))    # delensing lowers the EB noise


def test_active_column_pruning_is_exact():
    """prune=True (default) skips the hc columns where the band-limited filters vanish: kappa_hat must equal the
    unpruned pipeline's (same arithmetic on the surviving columns -> f64 ~1e-13, f32 ~1e-6 of the peak mode)
    and stay zero elsewhere; width-limited rfft / irfft / bin_power agree with their full versions."""
    from orphics_amd import lensing
    N, res = 1024, 1.0
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=8)
    kw = dict(noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True)
    for prec, tol in (("f64", 1e-12), ("f32", 2e-6)):
        qp = lensing.qest(shape, g, th, dtype=prec, **kw)
        qf = lensing.qest(shape, g, th, dtype=prec, prune=False, **kw)
        wl, wk = qp.leg_cols, qp.kappa_cols
        assert 0 < wl < wk < N // 2 + 1 and qf.leg_cols == 0 and qf.kappa_cols == 0
        e = qp.eng
        x = e.to_real(t1)
        kT = e.rfft(x)
        # width-limited forward transform: same leading columns, rest untouched
        kTw = e.hc(); kTw[:] = 7.0
        e.rfft(x, out=kTw, width=wl)
        assert torch.equal(kTw[:, :wl], kT[:, :wl]) and bool((kTw[:, wl:] == 7.0).all())
        rl = qp.leg_rows
        assert 0 < rl < N // 2
        kTw[:] = 7.0
        e.rfft(x, out=kTw, width=wl, rband=rl)             # band rows of the leading columns only
        band = np.r_[0:rl, N - rl + 1:N]
        assert torch.equal(kTw[band][:, :wl], kT[band][:, :wl]) and bool((kTw[:, wl:] == 7.0).all())
        kTw[rl:N - rl + 1] = 1e30                            # whatever sits outside the band must never be read
        full = qf.reconstruct_tt_hc(kT).clone()
        dirty = e.hc(); dirty[:] = 3.0
        pr = qp.reconstruct_tt_hc(kTw, out=dirty)          # garbage beyond wl in the input, garbage in `out`
        scale = float(full.abs().max())
        assert float((pr - full).abs().max()) / scale < tol
        assert bool((pr[:, wk:] == 0).all()) and bool((full[:, wk:N // 2 + 1] == 0).all())
        pr2 = qp.reconstruct_tt_hc(kTw, out=dirty)         # second use of the same output plane
        assert torch.equal(pr2, pr)
        # width-limited inverse transform of a band-limited plane
        kf = kT.clone(); kf[:, wl:] = 0
        r_full = e.irfft(kf)
        kf[:, wl:] = 5.0
        r_w = e.irfft(kf, width=wl)
        assert float((r_w - r_full).abs().max()) / float(r_full.abs().max()) < (1e-13 if prec == "f64" else 1e-6)
        # restricted binning: same sums
        edges = torch.as_tensor(np.linspace(20, 3000, 15), device=e.device)
        ids = e.modl_digitize(edges, half=True)
        s_full, c_full = e.bin_power(full, full, 1.0, ids, 16, herm=True)
        s_w, c_w = e.bin_power(pr, pr, 1.0, ids, 16, herm=True, active_cols=wk)
        assert float(((s_w[1:-1] - s_full[1:-1]) / s_full[1:-1]).abs().max()) < 10 * tol
        assert bool((c_w[1:-1] <= c_full[1:-1]).all())
        rk = qp.kappa_rows
        assert 0 < rk < N // 2 and bool((full[rk:N - rk + 1] == 0).all())        # kappa_hat vanishes outside the row band
        s_b, c_b = e.bin_power(pr, pr, 1.0, ids, 16, herm=True, active_cols=wk, active_rows=rk)
        assert float(((s_b[1:-1] - s_full[1:-1]) / s_full[1:-1]).abs().max()) < 10 * tol
        assert bool((c_b[1:-1] <= c_w[1:-1]).all())


def test_column_grid_is_exact():
    """col_grid="auto" (default): legs, row stage and divergence of the one-call TT path run on the smallest alias-free
    power-of-two number of rows (include/orphics_amd.h, COLUMN GRID).  kappa_hat must equal the col_grid="full"
    result (f64: rounding only), from a real map and from Fourier-space legs, with garbage outside the leg band of the
    input and in the output plane; a grid below the alias bound is refused."""
    from orphics_amd import lensing
    from orphics_amd._lib import OrphicsAmdError
    N, res = 1024, 1.0
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=11)
    kw = dict(noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True)
    for prec, tol in (("f64", 1e-12), ("f32", 2e-6)):
        qc = lensing.qest(shape, g, th, dtype=prec, **kw)
        qf = lensing.qest(shape, g, th, dtype=prec, col_grid="full", **kw)
        e = qc.eng
        x = e.to_real(t1)
        full = qf.reconstruct_tt_from_map(x).clone()
        assert qf.col_grid == 0
        dirty = e.hc(); dirty[:] = 3.0
        rec = qc.reconstruct_tt_from_map(x, out=dirty).clone()
        my = qc.col_grid
        rl, rk = qc.leg_rows, qc.kappa_rows
        assert 0 < my < N and my >= max(2 * rl + rk, 2 * rk) and my // 2 < max(2 * rl + rk, 2 * rk)
        scale = float(full.abs().max())
        assert float((rec - full).abs().max()) / scale < tol
        assert bool((rec[rk:N - rk + 1] == 0).all()) and bool((rec[:, qc.kappa_cols:] == 0).all())
        # Fourier-space legs (distinct X and Y), garbage outside the leg band
        kX, kY = e.rfft(x), e.rfft(e.to_real(t2))
        full2 = qf.reconstruct_tt_hc(kX, kY).clone()
        kXg, kYg = kX.clone(), kY.clone()
        kXg[rl:N - rl + 1] = 1e30; kYg[rl:N - rl + 1] = 1e30
        kXg[:, qc.leg_cols:] = 1e30; kYg[:, qc.leg_cols:] = 1e30
        rec2 = qc.reconstruct_tt_hc(kXg, kYg, out=dirty)
        assert float((rec2 - full2).abs().max()) / float(full2.abs().max()) < tol
        # explicit grids: twice the minimum is fine, half of it aliases and is refused
        q2 = lensing.qest(shape, g, th, dtype=prec, col_grid=2 * my if 2 * my < N else my, **kw)
        rec3 = q2.reconstruct_tt_from_map(x)
        assert float((rec3 - full).abs().max()) / scale < tol
        qbad = lensing.qest(shape, g, th, dtype=prec, col_grid=my // 2, **kw)
        with pytest.raises(OrphicsAmdError):
            qbad.reconstruct_tt_from_map(x)


@pytest.mark.parametrize("ny,nx,tl,kl", [(256, 256, 500, 800), (512, 256, 700, 1200), (1024, 256, 700, 1300), (256, 1024, 900, 1200)])
def test_column_grid_small_and_rectangular(ny, nx, tl, kl):
    """Tiny column grids (64 ... 256 rows: sub-lengths down to 8 points) and rectangular maps.  (The kappa mask stays
    below twice the leg band limit: beyond it no pair of leg modes reaches L, the response is rounding noise and
    A_L = 1/R amplifies it -- in every path, the modular one included.)"""
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (ny, nx)
    g = FlatGeometry.from_res(shape, 2.0)
    th = cosmology.default_theory()
    ml = g.modlmap()
    kw = dict(noise2d=np.full(shape, cosmology.white_noise_power(1.0)), beam2d=maps.gauss_beam(ml, 1.5),
              kmask=maps.mask_kspace(shape, g, lmin=100, lmax=tl), kmask_K=maps.mask_kspace(shape, g, lmin=20, lmax=kl),
              unlensed_equals_lensed=True, dtype="f64")
    qc = lensing.qest(shape, g, th, **kw)
    qf = lensing.qest(shape, g, th, col_grid="full", **kw)
    x = qc.eng.to_real(np.random.default_rng(ny + nx).standard_normal(shape))
    full = qf.reconstruct_tt_from_map(x).clone()
    rec = qc.reconstruct_tt_from_map(x)
    assert 0 < qc.col_grid < ny, (qc.col_grid, qc.leg_rows, qc.kappa_rows)
    assert float((rec - full).abs().max()) / float(full.abs().max()) < 1e-12


def test_column_grid_is_exact_for_pol_and_mv():
    """The polarised one-call path (oa_qe_pol) and the MV accumulation on the column grid equal the full-row results."""
    from orphics_amd import cosmology, lensing, maps
    N, res = 1024, 1.0
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=12)
    kw = dict(noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, noise2d_P=2 * noise, kmask_P=tmask, pol=True,
              unlensed_equals_lensed=True)
    rng = np.random.default_rng(3)
    for prec, tol in (("f64", 1e-11), ("f32", 5e-6)):
        qc = lensing.qest(shape, g, th, dtype=prec, **kw)
        qf = lensing.qest(shape, g, th, dtype=prec, col_grid="full", **kw)
        e = qc.eng
        kT, kE, kB = [e.rfft(e.to_real(rng.standard_normal(shape))) for _ in range(3)]
        f = {"T": kT, "E": kE, "B": kB}
        for XY in ("TE", "EE", "EB", "TB"):
            full = qf.reconstruct_hc(XY, f[XY[0]], f[XY[1]]).clone()
            dirty = e.hc(); dirty[:] = 3.0
            rec = qc.reconstruct_hc(XY, f[XY[0]], f[XY[1]], out=dirty)
            assert float((rec - full).abs().max()) / float(full.abs().max()) < tol, XY
        full = qf.reconstruct_mv_hc(kT, kE, kB).clone()
        rec = qc.reconstruct_mv_hc(kT, kE, kB)
        assert float((rec - full).abs().max()) / float(full.abs().max()) < tol


@pytest.mark.parametrize("N,res", [(1024, 1.0), (2048, 1.0)])
def test_reconstruct_from_map_fused_forward_legs(N, res):
    """reconstruct_tt_from_map (forward column pass 2 + leg filters + inverse pass 1 in one kernel; kT never
    written) == reconstruct_tt_hc(rfft(map)), pruned and dense; 2048 exercises the asymmetric column split."""
    from orphics_amd import lensing
    shape, g, th, ml, beam, noise, tmask, kmask, cl, t1, t2 = setup(N, res, seed=9)
    kw = dict(noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True)
    for prec, tol in (("f64", 1e-12), ("f32", 3e-6)):
        for prune in (True, False):
            q = lensing.qest(shape, g, th, dtype=prec, prune=prune, **kw)
            e = q.eng
            x = e.to_real(t1)
            ref = q.reconstruct_tt_hc(e.rfft(x)).clone()
            got = q.reconstruct_tt_from_map(x)
            w = N // 2 + 1
            assert float((got - ref)[:, :w].abs().max()) / float(ref.abs().max()) < tol


def test_tt_estimator_on_non_power_of_two_map():
    """A 480 x 600 patch (mixed-radix FFTs, modular estimator chain): kappa bandpowers == NumPy oracle."""
    from orphics_amd import cosmology, lensing, maps, stats
    from orphics_amd.geometry import FlatGeometry
    from oracle import maps_oracle as mo
    from oracle import qe_oracle as qo
    from oracle import stats_oracle as so
    shape = (480, 600)
    g = FlatGeometry.from_res(shape, 2.0)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    cltt = th.lCl("TT", ml)
    rng = np.random.default_rng(3)
    tmap = np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cltt * beam ** 2 + noise) / g.pixarea)).real
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f64")
    rec = q.kappa_from_map("TT", tmap)
    ref = qo.QEOracleTT(shape, g.step_y, g.step_x, cltt, cltt, noise, beam, tmask, kmask_K=kmask).kappa_from_map("TT", tmap)
    assert np.abs(rec - ref).max() < 1e-8 * np.abs(ref).max()
    edges = np.linspace(20, 3500, 20)
    p2d, _, _ = maps.FourierCalc(shape, g).power2d(rec)
    _, p1d = stats.bin2D(ml, edges).bin(p2d)
    _, p1r = so.bin2D(ml, edges).bin(mo.FourierCalc(shape, g.step_y, g.step_x).power2d(ref)[0])
    assert np.max(np.abs(p1d / p1r - 1)) < 1e-9


@pytest.mark.parametrize("XY", ["EB", "TE", "EE"])
def test_pol_estimators_on_non_power_of_two_map(XY):
    """The reference's verification notebook runs pol=True estimators on a 1200 x 1200 patch: on sides that are
    not powers of two the general estimators go through the modular chain (mixed-radix FFTs; the patch itself:
    test_notebook_patch_1200_estimators_match_oracle) and match the oracle."""
    from orphics_amd import lensing
    shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, k = pol_setup((96, 160), 2.0, seed=5)
    qr = qo.QEOracle(shape, g.step_y, g.step_x, cl, dict(T=nT, P=nP), beam, dict(T=tmask, P=tmask), kmask_K=kmask)
    qr.setup(XY)
    kref = qr.kappa_ft(XY, k[XY[0]], k[XY[1]])
    q = lensing.qest(shape, g, th, dtype="f64", noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask,
                     kmask_K=kmask, pol=True, unlensed_equals_lensed=True)
    assert not q.eng.pow2
    got = q.kappa_from_map(XY, T2DData=k["T"], E2DData=k["E"], B2DData=k["B"], alreadyFTed=True, returnFt=True)
    sel = (ml > 40) & (ml < 2900) & (qr.R[XY] != 0)
    assert np.max(np.abs(q.N_kappa(XY)[sel] / qr.Nlkk[XY][sel] - 1)) < 1e-7
    assert np.abs(got - kref)[sel].max() / np.abs(kref[sel]).max() < 1e-8


@pytest.mark.parametrize("XY", ["TT", "EB"])
def test_notebook_patch_1200_estimators_match_oracle(XY):
    """The reference's verification loop runs on a 10 degree patch at 0.5' = 1200 x 1200 pixels (tutorials/tt_verification.ipynb
    cells 1-4): 1200 = 2^4 3 5^2, so every transform of the modular estimator chain is a mixed-radix transform (csrc/fft_mixed.hpp;
    until round 4: a chirp-z convolution on an inner 4096^2 plan).  qest.kappa_from_map("TT" / "EB") against oracle.QEOracle, float64
    1e-8 on the DFT of kappa_hat, float32 1e-5 on its bandpowers."""
    from orphics_amd import lensing, maps, stats
    shape, g, th, ml, beam, nT, nP, tmask, kmask, cl, k = pol_setup(1200, 0.5, seed=11)
    qr = qo.QEOracle(shape, g.step_y, g.step_x, cl, dict(T=nT, P=nP), beam, dict(T=tmask, P=tmask), kmask_K=kmask)
    qr.setup(XY)
    kref = qr.kappa_ft(XY, k[XY[0]], k[XY[1]])
    kw = dict(noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask, kmask_K=kmask, pol=True, unlensed_equals_lensed=True)
    args = dict(T2DData=k["T"], E2DData=k["E"], B2DData=k["B"], alreadyFTed=True, returnFt=True)
    q = lensing.qest(shape, g, th, dtype="f64", **kw)
    assert not q.eng.pow2
    got = q.kappa_from_map(XY, **args)
    sel = (ml > 40) & (ml < 2900) & (qr.R[XY] != 0)
    assert np.abs(got - kref)[sel].max() / np.abs(kref[sel]).max() < 1e-8
    edges = np.linspace(20, 3000, 20)
    binner = stats.bin2D(ml, edges)
    ref_b = binner.bin(np.abs(kref) ** 2)[1]
    got32 = q.astype("f32").kappa_from_map(XY, **args)
    b32 = binner.bin(np.abs(np.asarray(got32, dtype=np.complex128)) ** 2)[1]
    assert np.max(np.abs(b32 / ref_b - 1)) < 1e-5


@pytest.mark.parametrize("ny,nx", [(512, 2048), (2048, 512), (1024, 4096)])
def test_rectangular_maps_fused_equals_modular_and_oracle(ny, nx):
    """Rectangular power-of-two patches: the fused (pruned) pipeline, the from-map pipeline and the modular chain
    agree, and match the NumPy oracle (f64)."""
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (ny, nx)
    g = FlatGeometry.from_res(shape, 1.0)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    cltt = th.lCl("TT", ml)
    rng = np.random.default_rng(ny + nx)
    tmap = np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cltt * beam ** 2 + noise) / g.pixarea)).real
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype="f64")
    e = q.eng
    x = torch.as_tensor(tmap, dtype=e.rdt, device=e.device)
    kT = e.rfft(x)
    a = q.reconstruct_tt_hc(kT).clone()
    b = q.reconstruct_tt_hc(kT, fused=False).clone()
    c = q.reconstruct_tt_from_map(x).clone()
    w = nx // 2 + 1
    scale = float(b.abs().max())
    assert float((a - b)[:, :w].abs().max()) / scale < 1e-11
    assert float((c - b)[:, :w].abs().max()) / scale < 1e-11
    if ny * nx <= 2 ** 21:
        ref = qo.QEOracleTT(shape, g.step_y, g.step_x, cltt, cltt, noise, beam, tmask, kmask_K=kmask).kappa_from_map("TT", tmap)
        rec = q.kappa_from_map("TT", tmap)
        assert np.abs(rec - ref).max() < 1e-8 * np.abs(ref).max()


@pytest.mark.parametrize("prec,tol", [("f64", 1e-10), ("f32", 2e-4)])
def test_get_sim_teb_equals_iqu2teb_of_get_sim(prec, tol):
    """FlatLensingSims.get_sim_teb (kappa's drawn transform used directly, beam and noise applied in Fourier space, no transform
    taken twice) against the notebook's sequence on the same seeds: iqu2teb(get_sim(...)) and fft(kappa) -- same realisation, T, E,
    B equal to rounding on every mode below the Nyquist row / column (where a real-space round trip symmetrises the rotation)."""
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    N = 256
    shape = (3, N, N)
    g = FlatGeometry.from_res(shape, 1.5)
    th = cosmology.default_theory()
    sims = lensing.FlatLensingSims(shape, g, th, 1.5, 1.0, pol=True, dtype=prec)
    fc = maps.FourierCalc(shape, g, layout="half")
    teb, kin = sims.get_sim_teb(seed_cmb=(3, 1, 0), seed_kappa=(3, 2, 0), seed_noise=(3, 3, 0), lens_order=5)
    parts = sims.get_sim(seed_cmb=(3, 1, 0), seed_kappa=(3, 2, 0), seed_noise=(3, 3, 0), lens_order=5, return_intermediate=True)
    e = sims.lenser.eng
    ref = fc.iqu2teb(parts[5], normalize=False).t
    kref = e.rfft(parts[1].contiguous())
    w = N // 2                                        # columns 0 .. N/2 - 1 and rows != N/2: below Nyquist
    rows = torch.arange(N, device=e.device) != N // 2
    assert float((kin - kref)[rows][:, :w].abs().max() / kref.abs().max()) < tol
    for i in range(3):
        d = (teb[i] - ref[i])[rows][:, :w].abs().max() / ref[i].abs().max()
        assert float(d) < tol, (i, float(d))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_draw_hc_is_get_map_harm_in_one_pass(prec):
    """MapGen.draw_hc (oa_grf_mix: the white fields, the covsqrt mix, the E, B -> Q, U rotation and -- with inputs -- the beam, the
    Q, U -> E, B rotation and the sum, in ONE kernel) against the plane-by-plane path it replaces (oa_grf_hc + oa_cmul_real + add +
    oa_rot2): the same Philox streams and the same order of operations, so the draws are BIT-identical; the input mode agrees to
    rounding (torch's add(alpha=) contracts its multiply-add)."""
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    N = 128
    shape = (3, N, 2 * N)
    g = FlatGeometry.from_res(shape, 1.5)
    th = cosmology.default_theory()
    sims = lensing.FlatLensingSims(shape, g, th, 1.5, 1.0, pol=True, dtype=prec)
    e = sims.lenser.eng
    seed = (7, 1, 3)
    ref = sims.mgen.get_map(seed=seed, harm=True).t
    got = sims.mgen.draw_hc(seed)
    assert torch.equal(got, ref)                                           # T-E correlated: two terms per E mode, same order
    assert float(ref[1].abs().max()) > 0 and bool((got[..., e.nxh + 1:] == 0).all())
    mi = maps.queb_rotmat(g.lmap(), inverse=True)
    c, s = e.fullreal_to_hc(e.to_real(mi[0, 0])), e.fullreal_to_hc(e.to_real(mi[1, 0]))
    q, u = e.rot2(c, s, ref[1].contiguous(), ref[2].contiguous())
    rot = sims.mgen.draw_hc(seed, rot="inverse")
    assert torch.equal(rot[0], ref[0]) and torch.equal(rot[1], q) and torch.equal(rot[2], u)
    k = sims.kgen.draw_hc((7, 2, 3), scale=3.0)[0]
    assert torch.equal(k, sims.kgen.get_map(seed=(7, 2, 3), scalar=True, harm=True).t * 3.0)
    # inputs: rot(in * beam) + scale * noise draw
    mf = maps.queb_rotmat(g.lmap(), inverse=False)
    cf, sf = e.fullreal_to_hc(e.to_real(mf[0, 0])), e.fullreal_to_hc(e.to_real(mf[1, 0]))
    beam = e.fullreal_to_hc(e.to_real(maps.gauss_beam(g.modlmap(), 1.5)))
    ks = [e.cmul_real(rot[i].contiguous(), beam) for i in range(3)]
    ks[1], ks[2] = e.rot2(cf, sf, ks[1], ks[2])
    nk = sims.ngen.get_map(seed=(7, 3, 3), harm=True).t
    want = torch.stack([ks[i] + 2.5 * nk[i] for i in range(3)])
    out = sims.ngen.draw_hc((7, 3, 3), rot="forward", inputs=rot.clone(), filt=beam, scale=2.5)
    tol = 1e-14 if prec == "f64" else 1e-6
    assert float((out - want).abs().max() / want.abs().max()) < tol
    inp = rot.clone()                                                      # in place: the outputs may be the inputs
    sims.ngen.draw_hc((7, 3, 3), rot="forward", inputs=inp, filt=beam, scale=2.5, out=inp)
    assert torch.equal(inp, out)
    with pytest.raises(ValueError):
        sims.kgen.draw_hc(1, rot="inverse")
    with pytest.raises(ValueError):
        e.grf_mix(1, [[None]], filt=beam)


@pytest.mark.parametrize("prec,tol", [("f64", 1e-11), ("f32", 3e-5)])
@pytest.mark.parametrize("order", [1, 2, 5])
def test_lens_many_hc_equals_lens_many_of_the_inverse_transforms(prec, tol, order):
    """oa_lens_maps_hc (the maps' transforms in: no R2C, the undisplaced map one more plane of the batched row launches) against
    oa_lens_maps on the inverse-transformed maps: same lensed maps to rounding, for T, Q, U of one realisation."""
    from orphics_amd import cosmology, lensing
    from orphics_amd.geometry import FlatGeometry
    N = 256
    shape = (3, N, N)
    g = FlatGeometry.from_res(shape, 1.5)
    th = cosmology.default_theory()
    sims = lensing.FlatLensingSims(shape, g, th, 1.5, 1.0, pol=True, dtype=prec)
    e = sims.lenser.eng
    khc = sims.mgen.draw_hc((5, 1, 0), rot="inverse")
    unl = torch.stack([e.irfft(khc[i].contiguous(), scale=1.0 / np.sqrt(e.npix)) for i in range(3)])
    alpha = sims.lenser.alpha_from_kappa_hc(sims.kgen.draw_hc((5, 2, 0), scale=float(np.sqrt(e.npix)))[0])
    sp = sims.lenser.split(alpha)
    ref = sims.lenser.lens_many(unl, alpha, taylor_order=order, split=sp)
    got = sims.lenser.lens_many_hc(khc, alpha, taylor_order=order, split=sp)
    assert float((got - ref).abs().max() / ref.abs().max()) < tol
    assert float((ref - unl).abs().max() / ref.abs().max()) > 1e-3      # the deflection does something
    with pytest.raises(ValueError):
        sims.lenser.lens_many_hc(unl, alpha)


# (5400, 600): a float64 column transform of 5400 points takes the in-place stages (two [N][C] buffers would exceed the LDS).  Only
# float64 there: float32 runs the same two-buffer kernels as at the other shapes (its 5400-point transforms pass test_mixed_sides_gpu),
# and on this 180-degree patch the fifth-order Taylens in float32 is 5.4e-4 of max |T| from the NumPy one (measured)
@pytest.mark.parametrize("shape", [(120, 150), (96, 160), (5400, 600)])
def test_flat_lensing_op_on_mixed_radix_sides(shape):
    """oa_lens_maps / oa_lens_maps_hc on sides 2^a 3^b 5^c (the notebooks' patches; csrc/mixed.hip lens_derivs_t: per y-derivative
    order one inverse column transform with (i ly)^b at its load, one row launch that takes every (i lx)^a at its load): the lensed map
    against the NumPy Taylens, against the term-by-term chain of public calls, and from the map's own transform."""
    from orphics_amd import lensing
    from orphics_amd.geometry import FlatGeometry
    ny, nx = shape
    g = FlatGeometry.from_res(shape, 2.0)
    rng = np.random.default_rng(ny + nx)
    ml = g.modlmap()
    kap = np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) * 1.5 / (1 + (ml / 200.) ** 2)).real
    T = np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) / (1 + (ml / 400.) ** 2)).real
    for prec, tol in (("f64", 1e-10), ("f32", 3e-5)):
        if prec == "f32" and shape == (5400, 600):
            continue
        L = lensing.FlatLenser(shape, g, dtype=prec)
        e = L.eng
        assert e.mixed and not e.pow2
        ay, ax = L.alpha_from_kappa(kap)
        ray, rax = qo.alpha_from_kappa(kap, g.step_y, g.step_x)
        for order in (5, 3):
            ref = qo.flat_taylens((ray, rax), T, g.step_y, g.step_x, taylor_order=order)
            lensed = L.lens(T, (ay, ax), taylor_order=order)
            assert np.abs(lensed.cpu().numpy() - ref).max() / np.abs(ref).max() < tol
            per_term = L.lens(T, (ay, ax), taylor_order=order, fused=False)
            assert float((lensed - per_term).abs().max()) / np.abs(ref).max() < tol
            # from the transform (oa_lens_maps_hc): unnormalised rfft in, scale 1 / Npix
            src = e.to_real(T)
            k = e.rfft(src)
            hc = L.lens_many_hc(k[None].contiguous(), (ay, ax), taylor_order=order, scale=1.0 / e.npix)[0]
            assert float((hc - lensed).abs().max()) / np.abs(ref).max() < tol


def test_lensed_sims_loop_fast_path_equals_the_notebook_sequence():
    """mc.LensedSimsMonteCarlo (tutorials/tt_verification.ipynb's loop): the device pipeline (get_sim_teb: oa_grf_mix,
    oa_lens_maps_hc; estimator-owned output planes; binning over the bins' support only) against the notebook's sequence
    written out (get_sim -> iqu2teb -> reconstruct -> power2d/bin over full planes) on the same seeds: the per-realisation samples
    (C_b^{kappa_hat x kappa_in} - C_b^{in}) / C_b^{in} and the bandpower vectors agree to rounding, and the reconstruction correlates
    with its input."""
    from orphics_amd import cosmology, lensing, maps, mc
    from orphics_amd.geometry import FlatGeometry
    N = 256
    shape = (3, N, N)
    g = FlatGeometry.from_res(shape, 1.5)
    th = cosmology.default_theory()
    sims = lensing.FlatLensingSims(shape, g, th, 1.5, 1.0, pol=True, dtype="f64")
    keep = {k: maps.mask_kspace(shape, g, lmin=lo, lmax=hi) for k, (lo, hi) in (("T", (300., 2000.)), ("K", (20., 2500.)))}
    q = lensing.qest(shape, g, th, noise2d=sims.ps_noise[0, 0], beam2d=sims.kbeam, kmask=keep["T"], noise2d_P=sims.ps_noise[1, 1],
                     kmask_P=keep["T"], kmask_K=keep["K"], pol=True, unlensed_equals_lensed=True, dtype="f64")
    edges = np.linspace(40, 2400, 12)
    fast = mc.LensedSimsMonteCarlo(sims, q, edges, estimators=("TT", "EB"))
    assert fast._bin_region["active_cols"] > 0 and fast._bin_region["active_rows"] > 0       # the bins end below the Nyquist frequency
    slow = mc.LensedSimsMonteCarlo(sims, q, edges, estimators=("TT", "EB"))
    slow.fast_sims = False
    slow._bin_region = dict(active_cols=0, active_rows=0)
    fast.run_local(range(3)); slow.run_local(range(3))
    fast.acc.allreduce(); slow.acc.allreduce()
    for label in ("input", "cross_TT", "cross_EB", "TT", "EB"):
        a, b = np.asarray(fast.acc.mean(label)), np.asarray(slow.acc.mean(label))
        assert a.shape == (edges.size - 1,) and np.all(np.isfinite(a))
        assert np.abs(a - b).max() < 1e-9 * np.abs(b).max(), label
    # kappa_hat x kappa_in tracks the input power where the TT estimator has signal (three realisations: loose bound)
    r = np.asarray(fast.acc.mean("cross_TT")) / np.asarray(fast.acc.mean("input"))
    assert np.all(np.abs(r[1:5] - 1.0) < 0.3), r


def test_get_sim_teb_temperature_only():
    """the device-pipeline simulator without polarisation (one component, no rotation): T's observed transform and kappa's equal the
    transforms of get_sim's maps on the same seeds"""
    from orphics_amd import cosmology, lensing
    from orphics_amd.geometry import FlatGeometry
    N = 256
    shape = (N, N)
    g = FlatGeometry.from_res(shape, 1.5)
    sims = lensing.FlatLensingSims(shape, g, cosmology.default_theory(), 1.5, 1.0, pol=False, dtype="f64")
    e = sims.lenser.eng
    teb, kin = sims.get_sim_teb(seed_cmb=(4, 1, 0), seed_kappa=(4, 2, 0), seed_noise=(4, 3, 0), lens_order=5)
    assert tuple(teb.shape) == (1, N, e.kp)
    parts = sims.get_sim(seed_cmb=(4, 1, 0), seed_kappa=(4, 2, 0), seed_noise=(4, 3, 0), lens_order=5, return_intermediate=True)
    ref = e.rfft(parts[5].contiguous())
    kref = e.rfft(parts[1].contiguous())
    rows = torch.arange(N, device=e.device) != N // 2
    w = N // 2
    assert float((kin - kref)[rows][:, :w].abs().max() / kref.abs().max()) < 1e-10
    assert float((teb[0] - ref)[rows][:, :w].abs().max() / ref.abs().max()) < 1e-10


def test_draw_hc_two_correlated_components():
    """oa_grf_mix with two components (a 2 x 2 covariance with an off-diagonal block): bit-identical to the plane-by-plane draw"""
    from orphics_amd import maps
    from orphics_amd.geometry import FlatGeometry
    N = 128
    shape = (2, N, N)
    g = FlatGeometry.from_res(shape, 2.0)
    ml = g.modlmap()
    p11 = 1.0 / (1.0 + (ml / 500.0) ** 2)
    p22 = 0.5 / (1.0 + (ml / 800.0) ** 2)
    p12 = 0.4 * np.sqrt(p11 * p22)
    cov = np.array([[p11, p12], [p12, p22]])
    for prec in ("f64", "f32"):
        mg = maps.MapGen(shape, g, cov, dtype=prec)
        ref = mg.get_map(seed=(2, 5), harm=True).t
        got = mg.draw_hc((2, 5))
        assert torch.equal(got, ref) and float(ref[1].abs().max()) > 0
        with pytest.raises(ValueError):
            mg.draw_hc((2, 5), rot="inverse")
