"""GPU: the N0 Monte Carlo of the polarisation estimators and their MV combination -- the leg-band draw (oa_grf_mix_band), the
multi-spectrum binning pass (oa_bin_power_multi), the one-call shard (oa_mc_run_mv), the driver mc.GaussianN0MonteCarloPol, and what
they are for: the Monte-Carlo N0 of TT, TE, EE, EB, TB against the analytic N_L from A_L, and the variance of the MV kappa_hat against the
diagonal-approximation Nlkk["MV"].  Geometry: pol_setup of tests/test_lensing_gpu.py (1.5' beam, 1 uK' T noise and twice that power in P,
T and P filters 300-2000, kappa mask 20-3000)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import maps_oracle as mo  # noqa: E402
from oracle import qe_oracle as qo  # noqa: E402
from oracle import stats_oracle as so  # noqa: E402

ESTS = ("TT", "TE", "EE", "EB", "TB")
SENTINEL = complex(-7.5, 3.25)


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


def driver(shape, res, prec, edges, **kw):
    from orphics_amd import mc
    return mc.GaussianN0MonteCarloPol(estimator(shape, res, prec), geometry(shape, res)["tot_h"], edges, **kw)


def close(got, ref, tol):
    """the project's moment comparison: rtol, plus the same factor times the largest |entry| (cross spectra scatter around zero)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())


# ---- oa_grf_mix_band ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape,width,rband", [((64, 128), 21, 9), ((64, 128), 65, 9), ((64, 128), 65, 0), ((48, 80), 13, 7)])
def test_band_draw_is_a_bit_identical_subset(shape, width, rband, prec):
    """Inside the band (columns < width, rows y < rband or y > ny - rband: negative-ky rows included; width 21 / 13 stop short of the
    Nyquist column, 65 = nx/2 + 1 reaches it and its self-conjugate rows) the planes equal oa_grf_mix's bit for bit, for ncomp 1, 2, 3
    with a NULL block and with scale 1 and 0.75; outside it the sentinel the planes were prefilled with is intact."""
    from orphics_amd.engine import Engine
    ny, nx = shape
    e = Engine(ny, nx, prec)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.arange(ny, device="cuda")
    inrow = (rows < rband) | (rows > ny - rband) if rband else torch.ones(ny, dtype=torch.bool, device="cuda")
    band = inrow[:, None] & (torch.arange(e.kp, device="cuda") < width)[None, :]
    assert bool(inrow[ny - 1]) and 0 < int(band.sum()) <= ny * (nx // 2 + 1)
    for ncomp, scale in ((1, 1.0), (2, 0.75), (3, 1.0), (3, 0.75)):
        cs = [[None] * ncomp for _ in range(ncomp)]
        for i in range(ncomp):
            for j in range(i + 1):           # lower triangle; the upper blocks stay NULL
                cs[i][j] = (torch.rand((ny, e.kp), generator=gen, device="cuda", dtype=torch.float64) + 0.25).to(e.rdt)
        if ncomp == 3:
            cs[2][0] = None                  # a NULL block inside the triangle too
        full = e.grf_mix(77, cs, scale=scale, stream_id0=12)
        out = [torch.full((ny, e.kp), SENTINEL, dtype=e.cdt, device="cuda") for _ in range(ncomp)]
        e.grf_mix_band(77, cs, out, width=width, rband=rband, scale=scale, stream_id0=12)
        for c in range(ncomp):
            a, b = torch.view_as_real(out[c]), torch.view_as_real(full[c])
            assert torch.equal(a[band], b[band]), (ncomp, c)
            assert bool((out[c][~band] == SENTINEL).all()), (ncomp, c)
    # a NULL-only table is a zero field
    z = [torch.full((ny, e.kp), SENTINEL, dtype=e.cdt, device="cuda")]
    e.grf_mix_band(77, [[None]], z, width=width, rband=rband)
    assert bool((z[0][band] == 0).all()) and bool((z[0][~band] == SENTINEL).all())


# ---- oa_bin_power_multi ------------------------------------------------------------------------------------------------------------
def bin_case(shape, prec, nedges=13, lmax=2900.0):
    from orphics_amd.engine import Engine
    from orphics_amd.geometry import FlatGeometry
    ny, nx = shape
    e = Engine(ny, nx, prec)
    g = FlatGeometry.from_res(shape, 2.0)
    e.set_laxes(*g.laxes())
    edges = np.linspace(100.0, lmax, nedges)
    ids = e.modl_digitize(torch.as_tensor(edges, device="cuda"), half=True)
    gen = torch.Generator(device="cuda").manual_seed(ny + nx)
    k = torch.view_as_complex(torch.randn((3, ny, e.kp, 2), generator=gen, device="cuda", dtype=torch.float64)).to(e.cdt).contiguous()
    w = torch.rand((3, ny, e.kp), generator=gen, device="cuda", dtype=torch.float64).to(e.rdt).contiguous()
    return e, ids, edges.size + 1, g.area / float(ny * nx) ** 2, k, w


PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2), (3, 3), (0, 3)]


def ref_spectrum(e, ids, nids, norm, x, y, **region):
    """oa_bin_power on the same pair of stored values, promoted to double: its products are then formed in double as
    oa_bin_power_multi's are in both precisions (in float32 oa_bin_power rounds each product to float first, 1e-7 per mode)"""
    from orphics_amd.engine import dev_bin_power
    return dev_bin_power(x.to(torch.complex128).contiguous(), y.to(torch.complex128).contiguous(), norm, ids, nids, herm_pitch=e.kp,
                         herm_nxh=e.nxh, **region)[0]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(64, 128), (256, 256)])
def test_multi_binning_matches_bin_power(shape, prec):
    """12 interior bins.  Every spectrum of the list == oa_bin_power on the same pair (1e-12 relative + 1e-12 of the largest sum:
    both accumulate in double); the weighted-sum field == the same sum formed with torch; with unit weights the MV auto is the sum of
    all autos and twice the crosses; the active region gives the sums of a full visit for planes that vanish outside it; two runs are
    bit-identical."""
    e, ids, nids, norm, k, w = bin_case(shape, prec)
    assert nids - 2 == 12
    ny, nx = shape

    def check(got, fields, pairs, **region):
        ref = torch.stack([ref_spectrum(e, ids, nids, norm, fields[a], fields[b], **region) for a, b in pairs])
        err = (got - ref).abs()
        assert bool((err <= 1e-12 * ref.abs() + 1e-12 * float(ref.abs().max())).all()), float(err.max())
    kmv = (w.double() * k.to(torch.complex128)).sum(0)
    fields = [k[0], k[1], k[2], kmv]
    got = e.bin_power_multi(k, PAIRS, norm, ids, nids, weights=w)
    assert got.shape == (len(PAIRS), nids)
    check(got, fields, PAIRS)
    # without weights: the stored fields alone
    check(e.bin_power_multi(k, PAIRS[:6], norm, ids, nids), fields, PAIRS[:6])
    # bit-identical reruns
    assert torch.equal(got, e.bin_power_multi(k, PAIRS, norm, ids, nids, weights=w))
    # unit weights: |sum_a k_a|^2 = sum_a |k_a|^2 + 2 sum_{a<b} Re(conj k_a k_b)
    one = torch.ones_like(w)
    s1 = e.bin_power_multi(k, PAIRS[:7], norm, ids, nids, weights=one)
    comb = s1[0] + s1[1] + s1[2] + 2 * (s1[3] + s1[4] + s1[5])
    assert bool(((s1[6] - comb).abs() <= 1e-12 * comb.abs() + 1e-12 * float(s1.abs().max())).all())
    # active region: planes that vanish outside (columns < wc, rows |ky index| < rb) -- wc odd and no multiple of the wave size
    wc, rb = nx // 4 + 3, ny // 4 + 1
    rows = torch.arange(ny, device="cuda")
    keep = ((rows < rb) | (rows > ny - rb))[:, None] & (torch.arange(e.kp, device="cuda") < wc)[None, :]
    kz = (k * keep).contiguous()
    fz = [kz[0], kz[1], kz[2], (w.double() * kz.to(torch.complex128)).sum(0)]
    full = e.bin_power_multi(kz, PAIRS, norm, ids, nids, weights=w)
    act = e.bin_power_multi(kz, PAIRS, norm, ids, nids, weights=w, active_cols=wc, active_rows=rb)
    check(full, fz, PAIRS)
    check(act, fz, PAIRS, active_cols=wc, active_rows=rb)
    assert bool(((act - full).abs() <= 1e-12 * full.abs() + 1e-12 * float(full.abs().max())).all())
    # ... and the region is honoured: garbage outside it does not reach the sums
    kg = torch.where(keep, k, torch.full_like(k, 1e6))
    assert torch.equal(act, e.bin_power_multi(kg.contiguous(), PAIRS, norm, ids, nids, weights=w, active_cols=wc, active_rows=rb))


def test_multi_binning_at_the_table_limit():
    """nspec * nids = 4096 (4 spectra of 1024 ids): the workgroup's table takes 128 KiB of LDS -- the launch needs the raised
    dynamic-LDS limit -- and the sums still equal oa_bin_power's"""
    e, ids, nids, norm, k, w = bin_case((64, 128), "f64", nedges=1023, lmax=5000.0)
    assert nids == 1024
    pairs = [(0, 0), (1, 2), (3, 3), (2, 3)]
    got = e.bin_power_multi(k, pairs, norm, ids, nids, weights=w)
    fields = [k[0], k[1], k[2], (w * k).sum(0)]
    ref = torch.stack([ref_spectrum(e, ids, nids, norm, fields[a], fields[b]) for a, b in pairs])
    assert bool(((got - ref).abs() <= 1e-12 * ref.abs() + 1e-12 * float(ref.abs().max())).all())
    assert e.lib.oa_bin_power_multi_scratch_bytes(4, 1024) > 0 and e.lib.oa_bin_power_multi_scratch_bytes(5, 1024) == -1


def test_multi_binning_refusals():
    """every listed refusal returns non-zero with its message before anything is launched: the sums keep their sentinel"""
    from orphics_amd import _lib
    e, ids, nids, norm, k, w = bin_case((64, 128), "f32")
    lib = e.lib
    scr = torch.empty(int(lib.oa_bin_power_multi_scratch_bytes(28, 14)), dtype=torch.uint8, device="cuda")
    sums = torch.full((4096 + 64,), -3.0, dtype=torch.float64, device="cuda")
    plane = e.ny * e.kp
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(nf=3, k0=k, w0=w, pairs=((0, 0), (0, 3)), nspec=None, nids_=nids, ids_=ids, sums_=sums, scr_=scr, a_null=False):
        ns = len(pairs) if nspec is None else nspec
        n = max(len(pairs), 1)
        a = (ctypes.c_int * n)(*[p[0] for p in pairs])
        b = (ctypes.c_int * n)(*[p[1] for p in pairs])
        rc = lib.oa_bin_power_multi(e.code, nf, P(k0), plane, P(w0), plane, ns, None if a_null else a, b, norm, P(ids_), nids_, e.ny, e.kp, e.nxh,
                                    0, 0, P(sums_), P(scr_), None)
        return rc, (lib.oa_last_error() or b"").decode()
    assert call()[0] == 0                                   # the accepted call, for contrast
    torch.cuda.synchronize()
    assert bool((sums[:2 * nids] != -3.0).all())
    sums.fill_(-3.0)
    cases = [
        (dict(pairs=(), nspec=0), "nspec must be in [1,28]"),
        (dict(pairs=((0, 0),) * 29), "nspec must be in [1,28]"),
        (dict(nids_=0), "nids (= nedges+1) must be in [1,1024]"),
        (dict(nids_=1025), "nids (= nedges+1) must be in [1,1024]"),
        (dict(pairs=((0, 0),) * 5, nids_=1000), "nspec * nids must not exceed 4096"),
        (dict(pairs=((0, 4),)), "field index outside [0, nfields]"),
        (dict(pairs=((-1, 0),)), "field index outside [0, nfields]"),
        (dict(pairs=((0, 3),), w0=None), "needs weight planes"),
        (dict(k0=None), "NULL argument"),
        (dict(ids_=None), "NULL argument"),
        (dict(sums_=None), "NULL argument"),
        (dict(scr_=None), "NULL argument"),
        (dict(a_null=True), "NULL spectrum list"),
        (dict(nf=0), "nfields must be in [1,6]"),
        (dict(nf=7), "nfields must be in [1,6]"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err and "oa_bin_power_multi" in err, (kw.keys(), rc, err)
    torch.cuda.synchronize()
    assert bool((sums == -3.0).all())
    with pytest.raises((ValueError, _lib.OrphicsAmdError)):
        e.bin_power_multi(k, [(0, 0)] * 29, norm, ids, nids)


# ---- oa_mc_run_mv ------------------------------------------------------------------------------------------------------------------
EDGES = np.linspace(100, 2900, 12)


def host_moments(drv, sims):
    X = torch.stack([drv.sample_host(i) for i in sims]).cpu().numpy()
    return X, X.sum(0), X.T @ X


def device_moments(drv):
    n, S, C = drv.acc.device_moments("n0", drv.D)
    return int(n.item()), S.cpu().numpy().copy(), C.cpu().numpy().copy()


@pytest.mark.parametrize("prec,tol", [("f64", 1e-10), ("f32", 2e-5)])
@pytest.mark.parametrize("shape", [(256, 256), (128, 256)])
def test_one_call_shard_equals_the_host_loop(shape, prec, tol):
    """Five estimators, the ten crosses and the MV auto, 6 realisations: n, S, C of oa_mc_run_mv == the sums of x and x x^T over the
    host loop of existing entries (full-plane Engine.grf_mix with the same seed and streams, reconstruct_hc per estimator, the
    weighted sum in torch, Engine.bin_power per spectrum) at the project's tolerance for such comparisons; [0, 6) in one call ==
    [0, 2) then [2, 6) bit for bit; OA_OPT_MV_BATCH = 0 (the estimators one at a time into the entry's own planes) gives the same
    moments; one estimator alone (EB) works."""
    drv = driver(shape, 2.0, prec, EDGES, base_seed=31)
    assert drv.one_call and len(drv.spectra) == 16 and drv.D == 16 * 11
    X, Sref, Cref = host_moments(drv, range(6))
    assert np.all(np.isfinite(X)) and np.all(X[:, :5 * 11] > 0)
    drv.run_local(range(6))
    n, S, C = device_moments(drv)
    assert n == 6
    close(S, Sref, tol)
    close(C, Cref, tol)
    # cut into two calls
    cut = driver(shape, 2.0, prec, EDGES, base_seed=31)
    cut.run_local(range(0, 2))
    cut.run_local(range(2, 6))
    n2, S2, C2 = device_moments(cut)
    assert n2 == 6 and np.array_equal(S2, S) and np.array_equal(C2, C)
    # the estimators one at a time
    e = drv.eng
    e.set_option("mv_batch", 0)
    try:
        one = driver(shape, 2.0, prec, EDGES, base_seed=31)
        one.run_local(range(6))
        n3, S3, C3 = device_moments(one)
    finally:
        e.set_option("mv_batch", 1)
    assert n3 == 6
    close(S3, Sref, tol)
    close(C3, Cref, tol)
    # nest = 1
    eb = driver(shape, 2.0, prec, EDGES, base_seed=31, estimators=("EB",), cross=False, mv=False)
    assert eb.spectra == [("EB", "EB")]
    _, Se, Ce = host_moments(eb, range(3))
    eb.run_local(range(3))
    n4, S4, C4 = device_moments(eb)
    assert n4 == 3
    close(S4, Se, tol)
    close(C4, Ce, tol)
    # the EB auto does not depend on the company it is drawn in
    close(S4 / 3, X[:3, 3 * 11:4 * 11].mean(0), tol)


def test_one_call_shard_refuses_other_sides():
    """a 48 x 80 (mixed-radix) plan: refused before anything is launched, naming the driver's host loop"""
    from orphics_amd.engine import Engine
    e = Engine(48, 80, "f32")
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    one_i, one_d, one_p = (ctypes.c_int * 1)(1), (ctypes.c_double * 1)(1.0), (ctypes.c_void_p * 1)(t.data_ptr())
    zero_i = (ctypes.c_int * 1)(0)
    nine = (ctypes.c_void_p * 9)(*([t.data_ptr()] * 9))
    rc = e.lib.oa_mc_run_mv(e.plan, 1, 0, 1, nine, 1, one_i, one_d, one_p, one_p, zero_i, zero_i, zero_i, one_p, None, 0, 1, zero_i, zero_i, p, 14, p,
                            1.0, 4, 4, 4, 4, -1, p, p, p, None)
    err = (e.lib.oa_last_error() or b"").decode()
    assert rc != 0 and "oa_mc_run_mv" in err and "host loop" in err and "GaussianN0MonteCarloPol" in err and "one_call=False" in err
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def test_driver_paths_agree_on_256():
    tol = 1e-10
    a = driver((256, 256), 2.0, "f64", EDGES, base_seed=7)
    b = driver((256, 256), 2.0, "f64", EDGES, base_seed=7, one_call=False)
    assert a.one_call and not b.one_call
    a.run(6)
    b.run(6)
    assert a.acc.count("n0") == b.acc.count("n0") == 6
    close(a.acc.mean("n0"), b.acc.mean("n0"), tol)
    close(a.cov(), b.cov(), 50 * tol)
    for x in ESTS + ("MV",):
        close(a.mean(x), b.mean(x), tol)
    close(a.mean("TT", "TE"), b.mean("TE", "TT"), tol)
    assert a.cov().shape == (a.D, a.D) and a.centers.shape == (11,)
    assert a.spectra[:5] == [(x, x) for x in ESTS] and a.spectra[-1] == ("MV", "MV")
    with pytest.raises(KeyError):
        a.mean("TT", "BB")


def test_driver_runs_the_host_loop_on_other_sides():
    """300 x 360 at 1' (the side the from-maps tests use): the automatic choice is the host loop of existing entries"""
    drv = driver((300, 360), 1.0, "f32", EDGES, base_seed=3)
    assert not drv.one_call
    st = drv.run(2)
    assert st.count("n0") == 2
    m = drv.mean("TT")
    assert m.shape == (11,) and np.all(np.isfinite(st.mean("n0"))) and np.all(m > 0) and np.all(drv.mean("MV") > 0)


def test_driver_autos_match_the_oracle_on_the_downloaded_draws():
    """128^2 float64, two realisations: the TT and EB autos of the one-call path == QEOracle.kappa_ft applied to the downloaded draws
    (Engine.grf_mix, same seed and streams), binned with the oracle's bin2D; 1e-8 relative, as test_pol_estimators_match_oracle"""
    shape, res = (128, 128), 2.0
    G = geometry(shape, res)
    g, ml = G["g"], G["ml"]
    drv = driver(shape, res, "f64", EDGES, base_seed=19, estimators=("TT", "EB"), cross=False, mv=False)
    e = drv.eng
    qr = qo.QEOracle(shape, g.step_y, g.step_x, G["cl"], dict(T=G["nT"], P=G["nP"]), G["beam"], dict(T=G["tmask"], P=G["tmask"]),
                     kmask_K=G["kmask"])
    for XY in ("TT", "EB"):
        qr.setup(XY)
    bo = so.bin2D(ml, EDGES)
    fo = mo.FourierCalc(shape, g.step_y, g.step_x)
    n, S, C = drv.acc.device_moments("n0", drv.D)
    prev = np.zeros(drv.D)
    for i in range(2):
        draws = e.grf_mix(19, drv.cs, stream_id0=3 * i)
        k = {X: e.hc_to_full(draws[j]).cpu().numpy() for j, X in enumerate("TEB")}
        drv.run_local([i])
        now = S.cpu().numpy().copy()
        x = now - prev
        prev = now
        for j, XY in enumerate(("TT", "EB")):
            kref = qr.kappa_ft(XY, k[XY[0]], k[XY[1]])
            _, pref = bo.bin(fo.f2power(kref, kref))
            assert np.max(np.abs(x[j * 11:(j + 1) * 11] / pref - 1)) < 1e-8, XY
    assert int(n.item()) == 2


# ---- what the feature is for -----------------------------------------------------------------------------------------------------
def test_n0_of_every_estimator_matches_AL_and_mv_exceeds_its_diagonal_noise():
    """SURVEY 8(c)-3 for all five estimators: on 256^2 at 2', float32, 40 Gaussian realisations, in every bin of linspace(100, 2900, 12)
    |mean - binned N_kappa(XY)| <= 5 standard errors of the mean (from the run's own covariance) and the relative standard error is
    <= 0.05, so that a pull cannot pass on scatter alone.  (A NumPy loop of QEOracle.kappa_ft on draws of this covariance, geometry,
    bins and count gave: largest pull 2.5, largest relative standard error 0.020, largest |mean / N0 - 1| 0.034.)  And the finding
    the driver exists to expose: the auto spectrum of the MV kappa_hat is not below binned Nlkk["MV"] -- the diagonal approximation
    neglects the covariances between the estimators and cannot overstate the noise -- and stays under twice that."""
    from orphics_amd import stats
    shape, res, nsims = (256, 256), 2.0, 40
    q = estimator(shape, res, "f32")
    drv = driver(shape, res, "f32", EDGES, base_seed=2024)
    drv.run(nsims)
    assert drv.acc.count("n0") == nsims
    binner = stats.bin2D(geometry(shape, res)["ml"], EDGES)
    for XY in ESTS:
        nl = binner.bin(q.N_kappa(XY))[1]
        mean, sem = drv.mean(XY), drv.sem(XY)
        pull, rel = np.abs(mean - nl) / sem, sem / mean
        print(XY, "max pull %.2f  max rel sem %.4f  max |mean/N0 - 1| %.4f" % (pull.max(), rel.max(), np.abs(mean / nl - 1).max()))
        assert np.all(pull <= 5.0), (XY, pull)
        assert np.all(rel <= 0.05), (XY, rel)
    nmv = binner.bin(q._full(q.Nlkk["MV"]))[1]
    mean, sem = drv.mean("MV"), drv.sem("MV")
    print("MV  mean / Nlkk[MV]:", np.round(mean / nmv, 4), " sem / mean max %.4f" % (sem / mean).max())
    assert np.all(mean >= nmv - 5 * sem), mean / nmv
    assert np.all(mean <= 2 * nmv), mean / nmv
