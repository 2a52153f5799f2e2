"""The fused divergence + binning launch with the bind-time run table (DivRunTail, orphics_amd/csrc/fft_divbin.hpp).

The smallest geometries that reach each fused instance: a 4096^2 map on its 768-row from-map grid (col_div3_sp_bin) and with the column
grid forced to 1024 rows (col_div_sp_bin), both precisions, one map (tt_moments) and two (tt_moments2).  n, S and C of the one-call
entry are compared with the fine-grained path (reconstruct_tt_from_map + bin_power: other kernels, per-point ids), 1e-12 relative at
float64 and 2e-6 at float32: the kappa values are the same, only the order of exact double additions differs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4096
TOL = {"f64": 1e-12, "f32": 2e-6}
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
        rng = np.random.default_rng(11)
        _cache["in"] = (shape, g, cosmology.default_theory(), kw, [rng.standard_normal(shape) for _ in range(2)])
    return _cache["in"]


def _case(prec, grid):
    """estimator, its two maps, and the bin ids of 19 radial bins, shared by the tests of one (precision, grid)"""
    key = (prec, grid)
    if key not in _cache:
        from orphics_amd import lensing
        shape, g, th, kw, xs = _inputs()
        q = lensing.qest(shape, g, th, dtype=prec, col_grid=grid, **kw)
        e = q.eng
        ids = e.modl_digitize(torch.as_tensor(np.linspace(20, 3500, 20), device=e.device), half=True)
        _cache[key] = dict(q=q, e=e, x=[e.to_real(x) for x in xs], ids=ids, pn=g.area / float(N * N) ** 2)
    return _cache[key]


def _reference(c, ids, nids):
    """bandpowers of both maps through the fine-grained path (kept per id plane: computed once)"""
    key = ("ref", id(c), id(ids))
    if key not in _cache:
        q, e = c["q"], c["e"]
        q.bind_bins(ids, nids, c["pn"])
        counts = q.bin_counts()[1:-1].double()
        bs = []
        for x in c["x"]:
            kk = q.reconstruct_tt_from_map(x)
            sums, _ = e.bin_power(kk, kk, c["pn"], ids, nids, herm=True, active_cols=q.kappa_cols, active_rows=q.kappa_rows)
            bs.append((sums[1:-1] / counts).cpu().numpy())
        _cache[key] = (ids, bs)                    # (the id plane is kept alive with its key)
    return _cache[key][1]


def _moments(c, ids, nids, nmaps):
    q, e = c["q"], c["e"]
    d = nids - 2
    q.bind_bins(ids, nids, c["pn"])
    n = torch.zeros(1, dtype=torch.int64, device=e.device)
    S = torch.zeros(d, dtype=torch.float64, device=e.device)
    C = torch.zeros(d, d, dtype=torch.float64, device=e.device)
    if nmaps == 2:
        q.tt_moments2(c["x"][0], c["x"][1], n, S, C)
    else:
        q.tt_moments(c["x"][0], n, S, C)
    torch.cuda.synchronize()
    eb = q._bind_bins()
    assert int(eb.lib.oa_plan_div_fused(eb.plan)) == 1
    return int(n.item()), S.cpu().numpy(), C.cpu().numpy()


def _compare(c, prec, ids, nids, nmaps, what):
    bs = _reference(c, ids, nids)[:nmaps]
    n, S, C = _moments(c, ids, nids, nmaps)
    Sr = sum(bs)
    Cr = sum(np.outer(b, b) for b in bs)
    assert np.all(Sr > 0)
    eS, eC = np.max(np.abs(S / Sr - 1)), np.max(np.abs(C / Cr - 1))
    print("%s %s, %d map(s): n = %d, S %.3g, C %.3g (bound %.0e)" % (what, prec, nmaps, n, eS, eC, TOL[prec]))
    assert n == nmaps
    assert eS < TOL[prec] and eC < TOL[prec]
    return S, C


@pytest.mark.parametrize("nmaps", [1, 2])
@pytest.mark.parametrize("grid", ["auto", 1024])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_moments_match_the_fine_grained_path(prec, grid, nmaps):
    c = _case(prec, grid)
    _compare(c, prec, c["ids"], 21, nmaps, "grid %s" % grid)
    assert c["q"].col_grid == (768 if grid == "auto" else 1024)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_two_identical_calls_are_bit_identical(prec):
    c = _case(prec, "auto")
    _, S0, C0 = _moments(c, c["ids"], 21, 2)
    _, S1, C1 = _moments(c, c["ids"], 21, 2)
    assert np.array_equal(S0, S1) and np.array_equal(C0, C1)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_ids_without_a_run_table_take_the_id_reading_tail(prec):
    """a checkerboard of two bins has a run per point: no run table, the same agreement through DivBinTail"""
    c = _case(prec, "auto")
    if "chk" not in c:
        y, x = torch.meshgrid(torch.arange(c["ids"].shape[0], device=c["e"].device), torch.arange(c["ids"].shape[1], device=c["e"].device),
                              indexing="ij")
        c["chk"] = (((x + y) & 1) + 1).to(torch.int32).contiguous()
    _compare(c, prec, c["chk"], 4, 2, "checkerboard ids")
    _compare(c, prec, c["ids"], 21, 2, "radial ids again")          # ... and the table comes back with the radial bins


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rebinding_other_edges_rebuilds_the_table(prec):
    """19 -> 7 bins on the same plan: the run table follows the bins (a stale one would put the power into the old rings)"""
    c = _case(prec, "auto")
    S19, _ = _compare(c, prec, c["ids"], 21, 1, "19 bins")
    if "ids7" not in c:
        c["ids7"] = c["e"].modl_digitize(torch.as_tensor(np.linspace(20, 3500, 8), device=c["e"].device), half=True)
    S7, _ = _compare(c, prec, c["ids7"], 9, 1, "7 bins")
    assert S7.shape == (7,) and S19.shape == (19,)
    _compare(c, prec, c["ids"], 21, 1, "19 bins again")
