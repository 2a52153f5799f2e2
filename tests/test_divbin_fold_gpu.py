"""The hand-over of the fused divergence + binning launch: every divergence workgroup stores its bin partials and ends, and
divbin_fold_kernel, the next launch on the stream, folds them and updates n, S and C (orphics_amd/csrc/fft_divbin.hpp).

The smallest geometries that reach each fused instance, as tests/test_divbin_runs_gpu.py: a 4096^2 map at 0.5' on its 768-row from-map
grid (col_div3_sp_bin) and with the column grid forced to 1024 rows (col_div_sp_bin), both precisions, 19 bins from linspace(20, 3500, 20).
Against the fine-grained path (reconstruct_tt_from_map + bin_power: other kernels, per-point ids) n is exact and S, C agree to 1e-12
(float64) / 2e-6 (float32): the kappa values are the same, only the order of exact double additions differs.  Everything else here is an
identity to the last bit: the fold adds in one fixed order, per map in map order, and S += b, C += b b^T are IEEE double operations (the
library is built without contraction), so NumPy forms the same sums from the single-call values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4096
TOL = {"f64": 1e-12, "f32": 2e-6}
GRIDS = ["auto", 1024]
PRECS = ["f64", "f32"]
_cache = {}


def _inputs():
    if "in" not in _cache:
        from orphics_amd import cosmology, maps
        from orphics_amd.geometry import FlatGeometry
        shape = (N, N)
        g = FlatGeometry.from_res(shape, 0.5)
        ml = g.modlmap()
        kw = dict(noise2d=np.full(shape, cosmology.white_noise_power(1.0)), beam2d=maps.gauss_beam(ml, 1.5),
                  kmask=maps.mask_kspace(shape, g, lmin=300, lmax=2000), kmask_K=maps.mask_kspace(shape, g, lmin=20, lmax=3500),
                  unlensed_equals_lensed=True)
        rng = np.random.default_rng(23)
        _cache["in"] = (shape, g, cosmology.default_theory(), kw, [rng.standard_normal(shape) for _ in range(2)])
    return _cache["in"]


def _case(prec, grid):
    """estimator, its two maps and the id planes of one (precision, grid): 19 radial bins; a checkerboard of two bins (a run per point:
    no run table, DivBinTail); 600 radial bins (more ids than a float64 workgroup has threads: 384 / 512).  The 600 bins start at
    l = 100: the modes of this map are 10.5 apart in l, so rings 5.7 wide hold a dozen modes and more from there on, none is empty."""
    key = (prec, grid)
    if key not in _cache:
        from orphics_amd import lensing
        shape, g, th, kw, xs = _inputs()
        q = lensing.qest(shape, g, th, dtype=prec, col_grid=grid, **kw)
        e = q.eng
        ids = e.modl_digitize(torch.as_tensor(np.linspace(20, 3500, 20), device=e.device), half=True)
        y, x = torch.meshgrid(torch.arange(ids.shape[0], device=e.device), torch.arange(ids.shape[1], device=e.device), indexing="ij")
        chk = (((x + y) & 1) + 1).to(torch.int32).contiguous()
        many = e.modl_digitize(torch.as_tensor(np.linspace(100, 3500, 601), device=e.device), half=True)
        _cache[key] = dict(q=q, e=e, x=[e.to_real(x) for x in xs], pn=g.area / float(N * N) ** 2,
                           bins={"radial": (ids, 21), "checkerboard": (chk, 4), "many": (many, 602)})
        assert q.col_grid == (768 if grid == "auto" else 1024)
    return _cache[key]


def _reference(c, which):
    """bandpowers of both maps through the fine-grained path, computed once per id plane"""
    key = ("ref", which)
    if key not in c:
        q, e = c["q"], c["e"]
        ids, nids = c["bins"][which]
        q.bind_bins(ids, nids, c["pn"])
        counts = q.bin_counts()[1:-1].double()
        assert int(counts.min().item()) > 0
        bs = []
        for x in c["x"]:
            kk = q.reconstruct_tt_from_map(x)
            sums, _ = e.bin_power(kk, kk, c["pn"], ids, nids, herm=True, active_cols=q.kappa_cols, active_rows=q.kappa_rows)
            bs.append((sums[1:-1] / counts).cpu().numpy())
        c[key] = bs
    return c[key]


def _acc(c, nids):
    dev = c["e"].device
    d = nids - 2
    return (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(d, dtype=torch.float64, device=dev),
            torch.zeros(d, d, dtype=torch.float64, device=dev))


def _run(c, which, calls):
    """calls: a list of map-index tuples, one tuple per C-ABI call (one index: tt_moments, two: tt_moments2), issued back to back on one
    stream from zeroed accumulators, no host synchronisation between them"""
    q, x = c["q"], c["x"]
    ids, nids = c["bins"][which]
    q.bind_bins(ids, nids, c["pn"])
    n, S, C = _acc(c, nids)
    for m in calls:
        if len(m) == 2:
            q.tt_moments2(x[m[0]], x[m[1]], n, S, C)
        else:
            q.tt_moments(x[m[0]], n, S, C)
    torch.cuda.synchronize()
    eb = q._bind_bins()
    assert int(eb.lib.oa_plan_div_fused(eb.plan)) == 1
    return int(n.item()), S.cpu().numpy(), C.cpu().numpy()


def _single(c, which):
    """b of each map alone: S of one tt_moments call from zero (0 + b = b), kept per id plane"""
    key = ("single", which)
    if key not in c:
        c[key] = [_run(c, which, [(m,)])[1] for m in (0, 1)]
    return c[key]


def _compare(c, prec, which, nmaps):
    bs = _reference(c, which)[:nmaps]
    n, S, C = _run(c, which, [tuple(range(nmaps))])
    Sr = sum(bs)
    Cr = sum(np.outer(b, b) for b in bs)
    assert np.all(Sr > 0)
    eS, eC = np.max(np.abs(S / Sr - 1)), np.max(np.abs(C / Cr - 1))
    print("%s ids %s, %d map(s): n = %d, S %.3g, C %.3g (bound %.0e)" % (which, prec, nmaps, n, eS, eC, TOL[prec]))
    assert n == nmaps
    assert eS < TOL[prec] and eC < TOL[prec]


def _numpy_moments(bs):
    S = np.zeros_like(bs[0])
    C = np.zeros((S.size, S.size))
    for b in bs:
        S = S + b
        C = C + np.outer(b, b)
    return S, C


@pytest.mark.parametrize("nmaps", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("prec", PRECS)
def test_moments_match_the_fine_grained_path(prec, grid, nmaps):
    _compare(_case(prec, grid), prec, "radial", nmaps)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("prec", PRECS)
def test_two_identical_calls_are_bit_identical(prec, grid):
    c = _case(prec, grid)
    for calls in ([(0,)], [(0, 1)]):
        n0, S0, C0 = _run(c, "radial", calls)
        n1, S1, C1 = _run(c, "radial", calls)
        assert n0 == n1 == len(calls[0])
        assert np.array_equal(S0, S1) and np.array_equal(C0, C1)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("prec", PRECS)
def test_a_pair_call_is_two_single_calls_to_the_last_bit(prec, grid):
    """tt_moments2(a, b) against tt_moments(a) then tt_moments(b): the fold is per map in map order in both"""
    c = _case(prec, grid)
    n2, S2, C2 = _run(c, "radial", [(0, 1)])
    n1, S1, C1 = _run(c, "radial", [(0,), (1,)])
    assert n2 == n1 == 2
    assert np.array_equal(S2, S1) and np.array_equal(C2, C1)


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("prec", PRECS)
def test_eight_calls_back_to_back_reuse_the_partials_buffer(prec, grid, pair):
    """eight calls on one stream without a host synchronisation, the two maps alternating: the partials buffer belongs to the plan, so
    the fold of call k must have read it before the divergence workgroups of call k + 1 store into it (stream order).  S and C are the
    sums of the single-call values in call order, to the last bit."""
    c = _case(prec, grid)
    b = _single(c, "radial")
    calls = [((k & 1, 1 - (k & 1)) if pair else (k & 1,)) for k in range(8)]
    n, S, C = _run(c, "radial", calls)
    Sr, Cr = _numpy_moments([b[m] for call in calls for m in call])
    assert n == (16 if pair else 8)
    assert np.array_equal(S, Sr)
    assert np.array_equal(C, Cr)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("prec", PRECS)
def test_ids_without_a_run_table_take_the_same_hand_over(prec, grid):
    """a checkerboard of two bins has a run per point: no run table, DivBinTail stores the partials"""
    c = _case(prec, grid)
    _compare(c, prec, "checkerboard", 2)
    b = _single(c, "checkerboard")
    n, S, C = _run(c, "checkerboard", [(0, 1), (1,)])
    Sr, Cr = _numpy_moments([b[0], b[1], b[1]])
    assert n == 3 and np.array_equal(S, Sr) and np.array_equal(C, Cr)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("prec", PRECS)
def test_more_ids_than_threads_take_several_rounds_of_the_fold(prec, grid):
    """602 ids: the float64 launches have 384 (768 rows) and 512 (1024 rows) threads, the float32 ones 768 and 1024.  (The fold by the
    last workgroup of the divergence launch, which this kernel replaced, left ids 384 .. 511 out on the 384-thread launch.)"""
    c = _case(prec, grid)
    _compare(c, prec, "many", 2)
    b = _single(c, "many")
    n, S, C = _run(c, "many", [(0, 1)])
    Sr, Cr = _numpy_moments(b)
    assert n == 2 and np.array_equal(S, Sr) and np.array_equal(C, Cr)
