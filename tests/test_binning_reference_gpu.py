"""GPU: the binning kernels of csrc/bin.hip (digitize_kernel, modl_digitize_kernel, bin_kernel in its four WEIGHTED x POWER builds,
bin_final_kernel, bin_multi_kernel) against the plain NumPy restatement of their contracts in oracle/stats_oracle.py -- never against
another kernel -- at the places where wave-level code goes wrong: sorted ids (segmented shuffle scan) and unsorted ids (ballot / match
loop), runs that start at any offset of a lane's four elements, ragged ends, the Hermitian multiplicities at columns 0 and nx/2, the
active region, the grid cap (a second step of the grid-stride loop), the dynamic-LDS limit and odd row pitches.

Tolerances.  Ids and counts are bit-exact.  The kernels add float64 terms in a fixed but arbitrary order, so per id, with the pinned
u64 = 2^-53, u32 = 2^-24 and 1.01 for second-order terms,

    |got - ref| <= 1.01 (c u_T + n_b u64) A_b,        A_b = sum of the terms' magnitudes, n_b = their number,

where c counts the roundings that form one term in the plane's precision u_T (0: stored data, the f32 -> f64 conversion is exact;
1: data x weight; 2: mode 1; 4: the power (two products, their sum, the norm's conversion and product); 5: weighted power), and
u_T = u64 for oa_bin_power_multi, which converts first.  One constant was corrected from the kernel's own operations: a spectrum of
oa_bin_power_multi that involves the weighted-sum field sum_f w_f k_f gets c = 4 + 2 nf and magnitudes built from sum_f |w_f| |k_f|,
because each operand carries up to nf roundings relative to that magnitude sum (products and running sum), not to its own value."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import stats_oracle as so  # noqa: E402

LD = np.longdouble
U64, U32 = 2.0 ** -53, 2.0 ** -24
UT = {"f32": U32, "f64": U64}
RDT = {"f32": np.float32, "f64": np.float64}
CDT = {"f32": np.complex64, "f64": np.complex128}
PRECS = ["f32", "f64"]
NORM = 0.37            # no power of two: the float32 build rounds it
IMAX = 2 ** 31 - 1


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def lib_and_code(prec):
    from orphics_amd import _lib
    return _lib.load(), {"f32": _lib.OA_F32, "f64": _lib.OA_F64}[prec]


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_error(lib):
    return (lib.oa_last_error() or b"").decode()


def assert_close(got, ref_sums, A, n, c, u_t, what):
    got = got.cpu().numpy().astype(LD)
    bound = LD(1.01) * (LD(c) * LD(u_t) + n.astype(LD) * LD(U64)) * A
    err = np.abs(got - ref_sums)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, "%s: id %d got %r ref %r err %.3g bound %.3g (n_b %d); %d ids off" % (
        what, bad[0], float(got[bad[0]]), float(ref_sums[bad[0]]), float(err[bad[0]]), float(bound[bad[0]]), n[bad[0]], bad.size)


# ---- one binning call and its reference -------------------------------------------------------------------------------------------
# variant -> (power, weighted, mode, skip_nan, c)
VARIANTS = {
    "plain": (False, False, 0, False, 0),
    "weighted": (False, True, 0, False, 1),
    "mode1": (False, False, 1, False, 2),
    "skip_nan": (False, False, 0, True, 0),
    "skip_nan_weighted": (False, True, 0, True, 1),
    "power_auto": (True, False, 0, False, 4),
    "power_cross": (True, False, 0, False, 4),
    "power_weighted": (True, True, 0, False, 5),
}


def make_inputs(prec, n, nids, rng):
    """stored values in the plane's precision: a real plane, the same with NaNs first, last and mid-run, two complex planes,
    weights of both signs, aux"""
    d = rng.standard_normal(n).astype(RDT[prec])
    dn = d.copy()
    dn[[0, n - 1, n // 2, min(n // 2 + 1, n - 1), n // 3]] = np.nan
    k1 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(CDT[prec])
    k2 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(CDT[prec])
    w = rng.uniform(-1.0, 2.0, n).astype(RDT[prec])
    return dict(d=d, dn=dn, k1=k1, k2=k2, w=w, aux=rng.standard_normal(nids))


def run_case(variant, prec, inp, ids, nids, pitch=0, nxh=-1, ac=0, ar=0, what="", check=True):
    """one oa_bin / oa_bin_power call through the engine wrappers, held against the reference; returns the two device outputs"""
    from orphics_amd.engine import dev_bin, dev_bin_power
    power, weighted, mode, skip_nan, c = VARIANTS[variant]
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    w = None
    if weighted:
        # the weights of dropped elements (id outside [0, nids), NaN under skip_nan) must not reach sums or wsums
        w = inp["w"].copy().reshape(-1)
        w[(ids < 0) | (ids >= nids)] = 1e6
        if skip_nan:
            w[np.isnan(inp["dn"].reshape(-1))] = 1e6
    wd = dev(w) if weighted else None
    idd = dev(ids)
    if power:
        k1 = inp["k1"].reshape(-1)
        k2 = k1 if variant == "power_auto" else inp["k2"].reshape(-1)
        k1d = dev(k1)
        k2d = k1d if variant == "power_auto" else dev(k2)
        got = dev_bin_power(k1d, k2d, NORM, idd, nids, herm_pitch=pitch, herm_nxh=nxh, active_cols=ac, active_rows=ar, weights=wd)
        ref = so.bin_power_ref(k1, k2, NORM, ids, nids, weights=w, pitch=pitch, nxh=nxh, active_cols=ac, active_rows=ar)
    else:
        data = (inp["dn"] if skip_nan else inp["d"]).reshape(-1)
        aux = inp["aux"] if mode == 1 else None
        got = dev_bin(dev(data), idd, nids, weights=wd, aux=dev(aux) if mode == 1 else None, mode=mode, skip_nan=skip_nan,
                      herm_pitch=pitch, herm_nxh=nxh)
        ref = so.bin_ref(data, ids, nids, weights=w, aux=aux, mode=mode, skip_nan=skip_nan, pitch=pitch, nxh=nxh)
    if check:
        what = "%s %s %s" % (variant, prec, what)
        assert_close(got[0], ref.sums, ref.A, ref.n, c, UT[prec], what + " sums")
        if weighted:
            assert got[1].dtype == torch.float64
            assert_close(got[1], ref.wsums, ref.wA, ref.n, 0, UT[prec], what + " wsums")     # w m is exact in float64
        else:
            assert got[1].dtype == torch.int64
            assert np.array_equal(got[1].cpu().numpy(), ref.counts), what + " counts"
    return got


# ---- sorted and unsorted ids, flat layout -----------------------------------------------------------------------------------------
# run lengths of the sorted pattern: 295 elements in 24 runs, so the four-run, three-run and two-run lanes fall on every offset of a
# lane's four elements as the cycle (odd length) repeats; 7171 elements hold 584 runs < FLAT_NIDS
RUNS = [1, 1, 1, 1, 2, 1, 1, 3, 1, 2, 2, 5, 7, 41, 1, 1, 1, 67, 3, 90, 1, 2, 1, 59]
FLAT_NIDS = 600
FLAT_N = [4 * 256 * 7 + r for r in range(4)] + [1, 3, 5]


def sorted_ids(n):
    lens = np.tile(RUNS, n // sum(RUNS) + 1)
    return np.repeat(np.arange(lens.size), lens)[:n].astype(np.int32)


def id_patterns(n, nids, rng):
    s = sorted_ids(n)
    assert s.max() < nids
    pats = {"sorted": s, "constant": np.full(n, 5, dtype=np.int32)}
    d = s.copy()                                   # one descent (to id 0) inside the wave instruction of elements 2304 .. 2559
    p = 256 * 9 + 130 if n > 256 * 10 else n // 2
    d[p:p + 2] = 0
    pats["descent"] = d
    t = s.copy()                                   # -1 mid-sequence: single ones, a whole lane, a run across two lanes
    t[rng.choice(n, max(1, n // 50), replace=False)] = -1
    if n > 2100:
        t[1024:1028] = -1
        t[2051:2057] = -1
    pats["minus_one"] = t
    e = s.copy()                                   # still sorted, ending beyond the table: nids itself ... 2^31 - 1
    tail = [nids, nids, nids + 1, IMAX, IMAX][-min(5, n):]
    e[n - len(tail):] = tail
    pats["beyond"] = e
    pats["alternating"] = np.where(np.arange(n) % 2 == 0, 3, 1).astype(np.int32)
    pats["random"] = rng.integers(0, nids, n).astype(np.int32)
    return pats


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_flat_ids_sorted_and_unsorted(variant, prec):
    """every build of bin_kernel on 256-element wave instructions (4 per lane): n = 4 * 256 * 7 + r and n = 1, 3, 5"""
    rng = np.random.default_rng(11)
    for n in FLAT_N:
        inp = make_inputs(prec, n, FLAT_NIDS, rng)
        for name, ids in id_patterns(n, FLAT_NIDS, rng).items():
            got = run_case(variant, prec, inp, ids, FLAT_NIDS, what="n=%d %s" % (n, name))
            if n == FLAT_N[3] and name in ("sorted", "random"):
                again = run_case(variant, prec, inp, ids, FLAT_NIDS, check=False)
                assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


# ---- digitize ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nedges", [1, 2, 4096])
def test_digitize_at_every_edge(nedges):
    from orphics_amd.engine import dev_digitize
    edges = (np.arange(nedges) - nedges // 2) * 0.25          # holds 0.0 exactly
    assert 0.0 in edges
    x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                        [np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -5e-324, 1.0]])
    while x.size % 256 == 0:
        x = np.append(x, 1.0)
    rng = np.random.default_rng(nedges)
    x = x[rng.permutation(x.size)]
    ids = dev_digitize(dev(x), dev(edges))
    assert ids.dtype == torch.int32
    ref = so.digitize_ref(x, edges)
    assert ref.min() == 0 and ref.max() == nedges
    assert np.array_equal(ids.cpu().numpy(), ref)
    assert torch.equal(ids, dev_digitize(dev(x), dev(edges)))


def test_digitize_refuses_4097_edges():
    lib, _ = lib_and_code("f64")
    edges = dev(np.arange(4097.0))
    x = dev(np.linspace(0.0, 5000.0, 300))
    ids = torch.full((300,), -7, dtype=torch.int32, device="cuda")
    rc = lib.oa_digitize(P(x), 300, P(edges), 4097, P(ids), stream())
    assert rc != 0 and "oa_digitize: nedges must be in [1,4096]" in last_error(lib)
    torch.cuda.synchronize()
    assert bool((ids == -7).all())
    assert lib.oa_digitize(P(x), 300, P(edges), 4096, P(ids), stream()) == 0
    assert np.array_equal(ids.cpu().numpy(), so.digitize_ref(x.cpu().numpy(), np.arange(4096.0)))


def axes(ny, nx, step_y=1.3e-3, step_x=0.7e-3):
    """anisotropic pixels: different fundamental frequencies along the two axes"""
    return np.fft.fftfreq(ny, step_y) * 2 * np.pi, np.fft.fftfreq(nx, step_x) * 2 * np.pi


def modl_edges(ly, lx, width, nedges=13):
    """edges taken from the |l| values themselves (ties go to the lower bin), 0 first, an overflow region above the last"""
    u = np.unique(np.sqrt(ly[:, None] ** 2 + lx[None, :width] ** 2))
    return u[np.linspace(0, u.size - 1, nedges + 1).astype(int)[:-1]]


def dev_modl_digitize(ly, lx, pitch, width, edges):
    lib, _ = lib_and_code("f64")
    ids = torch.full((ly.size, pitch), -9, dtype=torch.int32, device="cuda")
    modl = torch.full((ly.size, pitch), -9.0, dtype=torch.float64, device="cuda")
    lyd, lxd, ed = dev(ly), dev(lx), dev(edges)
    rc = lib.oa_modl_digitize(P(lyd), P(lxd), ly.size, lx.size, pitch, width, P(ed), edges.size, P(ids), P(modl), stream())
    assert rc == 0, last_error(lib)
    torch.cuda.synchronize()
    return ids, modl


@pytest.mark.parametrize("ny,nx", [(36, 750), (32, 64)])
def test_modl_digitize_half_plane(ny, nx):
    """hc layout (pitch nx/2 + 16: 391, odd, for nx = 750): ids and |l| bit-exact, the row padding gets id -1 and |l| 0"""
    ly, lx = axes(ny, nx)
    pitch, width = nx // 2 + 16, nx // 2 + 1
    edges = modl_edges(ly, lx, width)
    ids, modl = dev_modl_digitize(ly, lx, pitch, width, edges)
    rid, rmodl = so.modl_digitize_ref(ly, lx, pitch, width, edges)
    assert np.array_equal(ids.cpu().numpy(), rid)
    assert np.array_equal(modl.cpu().numpy(), rmodl)
    assert (rid[:, width:] == -1).all() and rid[:, :width].min() == 0 and rid.max() == edges.size
    ids2, modl2 = dev_modl_digitize(ly, lx, pitch, width, edges)
    assert torch.equal(ids, ids2) and torch.equal(modl, modl2)


# ---- Hermitian half plane ---------------------------------------------------------------------------------------------------------
# (ny, pitch, nxh, nx): rows of 12, 29, 64 and 129 four-column chunks (shorter than, equal to and longer than one wave), pitch nx/2 + 16;
# the last has a pitch wider than that, so that nxh is no multiple of 4
HERM = [(32, 48, 32, 64), (40, 116, 100, 200), (64, 516, 500, 1000), (16, 256, 240, 480), (40, 116, 98, 196)]
HERM_VARIANTS = ["plain", "weighted", "mode1", "power_auto", "power_cross", "power_weighted"]


def herm_inputs(prec, ny, pitch, nxh, nids, rng):
    """planes whose row padding (columns > nxh) holds 1e6 in data and weights: it must not count"""
    inp = make_inputs(prec, ny * pitch, nids, rng)
    for key in ("d", "k1", "k2", "w"):
        a = inp[key].reshape(ny, pitch)
        a[:, nxh + 1:] = 1e6 * (1 + 1j) if np.iscomplexobj(a) else 1e6
    return inp


def herm_ids(ny, pitch, nxh, nx):
    """radial ids from the device (checked against the reference), and a non-monotonic map with VALID ids on the row padding"""
    ly, lx = axes(ny, nx)
    edges = modl_edges(ly, lx, nxh + 1)
    ids, _ = dev_modl_digitize(ly, lx, pitch, nxh + 1, edges)
    radial = ids.cpu().numpy()
    assert np.array_equal(radial, so.modl_digitize_ref(ly, lx, pitch, nxh + 1, edges)[0])
    nids = edges.size + 1
    other = ((7 * np.arange(ny)[:, None] + 3 * np.arange(pitch)[None, :]) % nids).astype(np.int32)
    return nids, radial, other


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,pitch,nxh,nx", HERM)
def test_hermitian_half_plane(ny, pitch, nxh, nx, prec):
    rng = np.random.default_rng(ny + nx)
    nids, radial, other = herm_ids(ny, pitch, nxh, nx)
    inp = herm_inputs(prec, ny, pitch, nxh, nids, rng)
    for name, ids in (("radial", radial), ("non-monotonic", other)):
        for variant in HERM_VARIANTS:
            got = run_case(variant, prec, inp, ids, nids, pitch=pitch, nxh=nxh, what="%dx%d %s" % (ny, pitch, name))
            if variant in ("weighted", "power_cross"):
                again = run_case(variant, prec, inp, ids, nids, pitch=pitch, nxh=nxh, check=False)
                assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    # a plane that is non-zero only at columns 0 and nxh: multiplicity 1 there
    edge = make_inputs(prec, ny * pitch, nids, rng)
    for key in ("d", "k1", "k2"):
        a = edge[key].reshape(ny, pitch)
        keep = a[:, [0, nxh]].copy()
        a[:] = 0
        a[:, [0, nxh]] = keep
    for variant in ("plain", "weighted", "power_auto", "power_weighted"):
        got = run_case(variant, prec, edge, radial, nids, pitch=pitch, nxh=nxh, what="%dx%d columns 0 and nxh" % (ny, pitch))
        assert float(got[0].abs().sum()) > 0


# ---- active region ----------------------------------------------------------------------------------------------------------------
def dev_bin_power_multi(prec, fields, weights, pairs, norm, ids, nids, ny, pitch, nxh, ac, ar):
    """the raw C entry (plan-free: any pitch)"""
    lib, code = lib_and_code(prec)
    ns = len(pairs)
    need = int(lib.oa_bin_power_multi_scratch_bytes(ns, nids))
    assert need > 0
    scr = torch.empty(need, dtype=torch.uint8, device="cuda")
    sums = torch.full((ns, nids), -3.0, dtype=torch.float64, device="cuda")
    a = (ctypes.c_int * ns)(*[p[0] for p in pairs])
    b = (ctypes.c_int * ns)(*[p[1] for p in pairs])
    rc = lib.oa_bin_power_multi(code, fields.shape[0], P(fields), ny * pitch, P(weights), ny * pitch, ns, a, b, norm, P(ids), nids, ny, pitch,
                                nxh, ac, ar, P(sums), P(scr), stream())
    assert rc == 0, last_error(lib)
    torch.cuda.synchronize()
    return sums


MULTI_PAIRS = [(0, 0), (0, 1), (3, 3), (2, 3)]       # field 3 = the weighted sum of three stored fields


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,pitch,nxh,nx", [(40, 116, 100, 200), (64, 516, 500, 1000)])
def test_active_region_is_honoured_exactly(ny, pitch, nxh, nx, prec):
    """oa_bin_power (the kernel of the one-call Monte Carlo's bin_power_moments as well) and oa_bin_power_multi on planes that hold 1e6
    everywhere outside the region: sums and counts are those of the region, also where active_cols is no multiple of the four columns
    a lane moves"""
    rng = np.random.default_rng(ny * nx)
    ly, lx = axes(ny, nx)
    edges = modl_edges(ly, lx, nxh + 1)
    nids = edges.size + 1
    ids = so.modl_digitize_ref(ly, lx, pitch, nxh + 1, edges)[0]
    ids[:, nxh + 1:] = 3                                            # valid ids on the row padding: only its multiplicity 0 drops it
    nf = 3
    k = (rng.standard_normal((nf, ny, pitch)) + 1j * rng.standard_normal((nf, ny, pitch))).astype(CDT[prec])
    w = rng.uniform(-1.0, 2.0, (nf, ny, pitch)).astype(RDT[prec])
    idd = dev(ids)
    y, col = np.arange(ny), np.arange(pitch)
    small = ny * pitch < 10000
    for ac in (1, 2, 3, 4, 5, 37, nxh, nxh + 1):
        for ar in (0, 1, 2, ny // 4 + 1, ny // 2, ny // 2 + 1):
            rows = ((y < ar) | (y > ny - ar)) if ar > 0 else np.ones(ny, dtype=bool)
            region = rows[:, None] & (col < ac)[None, :]
            kg = np.where(region[None], k, CDT[prec](1e6 * (1 + 1j)))
            wg = np.where(region[None], w, RDT[prec](1e6))
            what = "active_cols=%d active_rows=%d" % (ac, ar)
            inp = dict(k1=kg[0], k2=kg[1], w=wg[0])
            for variant in ("power_cross", "power_weighted") if small else ("power_cross",):
                run_case(variant, prec, inp, ids, nids, pitch=pitch, nxh=nxh, ac=ac, ar=ar, what=what)
            pairs = MULTI_PAIRS if small else MULTI_PAIRS[1:3]
            got = dev_bin_power_multi(prec, dev(kg), dev(wg), pairs, NORM, idd, nids, ny, pitch, nxh, ac, ar)
            ref = so.bin_power_multi_ref(kg, pairs, NORM, ids, nids, nxh, weights=wg, active_cols=ac, active_rows=ar)
            for s, (a, b) in enumerate(pairs):
                c = 4 + 2 * nf if nf in (a, b) else 4
                assert_close(got[s], ref[s].sums, ref[s].A, ref[s].n, c, U64, "multi %s %s pair %d,%d" % (prec, what, a, b))
    again = dev_bin_power_multi(prec, dev(kg), dev(wg), pairs, NORM, idd, nids, ny, pitch, nxh, ac, ar)
    assert torch.equal(got, again)
    a1 = run_case("power_cross", prec, inp, ids, nids, pitch=pitch, nxh=nxh, ac=37, ar=2, check=False)
    a2 = run_case("power_cross", prec, inp, ids, nids, pitch=pitch, nxh=nxh, ac=37, ar=2, check=False)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])


@pytest.mark.parametrize("prec", PRECS)
def test_multi_binning_whole_half_plane(prec):
    """oa_bin_power_multi without a region on (40, 116), nxh = 98 (no multiple of 4) and a non-monotonic id map"""
    ny, pitch, nxh, nx = HERM[4]
    rng = np.random.default_rng(5)
    nids, radial, other = herm_ids(ny, pitch, nxh, nx)
    nf = 3
    k = (rng.standard_normal((nf, ny, pitch)) + 1j * rng.standard_normal((nf, ny, pitch))).astype(CDT[prec])
    w = rng.uniform(-1.0, 2.0, (nf, ny, pitch)).astype(RDT[prec])
    k[:, :, nxh + 1:] = 1e6 * (1 + 1j)
    w[:, :, nxh + 1:] = 1e6
    for ids in (radial, other):
        got = dev_bin_power_multi(prec, dev(k), dev(w), MULTI_PAIRS, NORM, dev(ids), nids, ny, pitch, nxh, 0, 0)
        ref = so.bin_power_multi_ref(k, MULTI_PAIRS, NORM, ids, nids, nxh, weights=w)
        for s, (a, b) in enumerate(MULTI_PAIRS):
            assert_close(got[s], ref[s].sums, ref[s].A, ref[s].n, 4 + 2 * nf if nf in (a, b) else 4, U64, "multi %s pair %d,%d" % (prec, a, b))


# ---- grid cap ---------------------------------------------------------------------------------------------------------------------
def test_grid_cap_flat_f32():
    """n = 1024 * 256 * 4 + 4 * 256 * 3 + 3: 1028 workgroups' worth of chunks on the 1024 the grid is capped at"""
    n = 1024 * 256 * 4 + 4 * 256 * 3 + 3
    rng = np.random.default_rng(1)
    inp = make_inputs("f32", n, FLAT_NIDS, rng)
    ids = (np.arange(n, dtype=np.int64) * FLAT_NIDS // n).astype(np.int32)
    ids[-3:] = FLAT_NIDS - 1
    got = run_case("plain", "f32", inp, ids, FLAT_NIDS, what="grid cap sorted")
    again = run_case("plain", "f32", inp, ids, FLAT_NIDS, check=False)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    run_case("power_weighted", "f32", inp, rng.integers(-1, FLAT_NIDS + 1, n).astype(np.int32), FLAT_NIDS, what="grid cap random")


def test_grid_cap_hermitian_f64():
    """(2048, 528), nx = 1024: 2048 rows of 192 padded chunk slots = 1536 workgroups' worth on 1024"""
    ny, pitch, nxh, nx = 2048, 528, 512, 1024
    rng = np.random.default_rng(2)
    ly, lx = axes(ny, nx)
    edges = modl_edges(ly, lx, nxh + 1, nedges=20)
    ids, _ = dev_modl_digitize(ly, lx, pitch, nxh + 1, edges)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, so.modl_digitize_ref(ly, lx, pitch, nxh + 1, edges)[0])
    inp = herm_inputs("f64", ny, pitch, nxh, edges.size + 1, rng)
    got = run_case("power_cross", "f64", inp, ids, edges.size + 1, pitch=pitch, nxh=nxh, what="grid cap")
    again = run_case("power_cross", "f64", inp, ids, edges.size + 1, pitch=pitch, nxh=nxh, check=False)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


# ---- LDS limit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nids", [1, 2, 768, 769, 1024])
def test_lds_limit(nids, prec):
    """64 * nids bytes of LDS per workgroup: 48 KiB at nids = 768, the raised dynamic-LDS limit above; ids reach the last slot"""
    n = 4 * 256 * 2 + 3
    rng = np.random.default_rng(nids)
    inp = make_inputs(prec, n, nids, rng)
    ids = rng.integers(-1, nids + 1, n).astype(np.int32)
    ids[[7, n - 1]] = nids - 1
    for name, i in (("random", ids), ("sorted", np.sort(ids))):
        for variant in ("plain", "weighted", "mode1", "power_auto", "power_weighted"):
            got = run_case(variant, prec, inp, i, nids, what="nids=%d %s" % (nids, name))
            assert variant == "mode1" or float(got[0][nids - 1].abs()) > 0
            if variant in ("weighted", "power_auto"):
                again = run_case(variant, prec, inp, i, nids, check=False)
                assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


def raw_bin(prec, n, nids, pitch=0, nxh=-1):
    """the raw oa_bin and oa_bin_power on sentinel-filled outputs: (rc, message, outputs) of each"""
    lib, code = lib_and_code(prec)
    rdt = {"f32": torch.float32, "f64": torch.float64}[prec]
    data = torch.ones(2 * n, dtype=rdt, device="cuda")
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    scr = torch.empty(max(int(lib.oa_bin_scratch_bytes(nids)), 8), dtype=torch.uint8, device="cuda")
    out = []
    for power in (False, True):
        sums = torch.full((nids + 8,), -3.0, dtype=torch.float64, device="cuda")
        counts = torch.full((nids + 8,), -3, dtype=torch.int64, device="cuda")
        if power:
            rc = lib.oa_bin_power(code, P(data), P(data), 1.0, P(ids), None, n, nids, pitch, nxh, P(sums), P(counts), None, P(scr), 0, 0, stream())
        else:
            rc = lib.oa_bin(code, P(data), P(ids), None, None, n, nids, 0, 0, pitch, nxh, P(sums), P(counts), None, P(scr), stream())
        msg = last_error(lib)
        torch.cuda.synchronize()
        out.append((rc, msg, sums, counts))
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_refusals_leave_the_outputs_alone(prec):
    for name, (rc, msg, sums, counts) in zip(("oa_bin", "oa_bin_power"), raw_bin(prec, 1024, 1025)):
        assert rc != 0 and (name + ": nids (= nedges+1) must be in [1,1024]") in msg, (rc, msg)
        assert bool((sums == -3.0).all()) and bool((counts == -3).all())
    # a Hermitian row pitch that is no multiple of 4 (nx = 750: 375 + 16)
    for name, (rc, msg, sums, counts) in zip(("oa_bin", "oa_bin_power"), raw_bin(prec, 36 * 391, 14, pitch=391, nxh=375)):
        assert rc != 0 and (name + ": herm_pitch must be a positive multiple of 4") in msg, (rc, msg)
        assert bool((sums == -3.0).all()) and bool((counts == -3).all())
    # the accepted calls, for contrast
    for rc, msg, sums, counts in raw_bin(prec, 36 * 392, 14, pitch=392, nxh=375):
        assert rc == 0, msg
        assert int(counts[0]) == 36 * 750 and float(sums[0]) in (36 * 750.0, 2 * 36 * 750.0) and bool((sums[14:] == -3.0).all())


# ---- odd row pitch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_engine_bin_power_on_an_odd_pitch(prec):
    """Engine.bin_power on a (36, 750) plan (pitch 391): the padded-copy route, with and without weights and a region"""
    from orphics_amd.engine import Engine
    ny, nx = 36, 750
    e = Engine.get(ny, nx, prec)
    pitch, nxh = e.kp, e.nxh
    assert pitch == 391 and nxh == 375
    rng = np.random.default_rng(3)
    ly, lx = axes(ny, nx)
    edges = modl_edges(ly, lx, nxh + 1)
    nids = edges.size + 1
    ids = so.modl_digitize_ref(ly, lx, pitch, nxh + 1, edges)[0]
    inp = herm_inputs(prec, ny, pitch, nxh, nids, rng)
    k1, k2, w = (inp[key].reshape(ny, pitch) for key in ("k1", "k2", "w"))
    k1d, k2d, wd, idd = dev(k1), dev(k2), dev(w), dev(ids)
    for kw in (dict(), dict(active_cols=37, active_rows=5)):
        s, c = e.bin_power(k1d, k2d, NORM, idd, nids, **kw)
        ref = so.bin_power_ref(k1, k2, NORM, ids, nids, pitch=pitch, nxh=nxh, **kw)
        assert_close(s, ref.sums, ref.A, ref.n, 4, UT[prec], "odd pitch %s %s" % (prec, kw))
        assert np.array_equal(c.cpu().numpy(), ref.counts)
        s2, c2 = e.bin_power(k1d, k2d, NORM, idd, nids, **kw)
        assert torch.equal(s, s2) and torch.equal(c, c2)
        s, ws = e.bin_power(k1d, k1d, NORM, idd, nids, weights=wd, **kw)
        ref = so.bin_power_ref(k1, k1, NORM, ids, nids, weights=w, pitch=pitch, nxh=nxh, **kw)
        assert_close(s, ref.sums, ref.A, ref.n, 5, UT[prec], "odd pitch weighted %s %s" % (prec, kw))
        assert_close(ws, ref.wsums, ref.wA, ref.n, 0, UT[prec], "odd pitch wsums %s %s" % (prec, kw))
