"""The ensemble accumulators on the device -- oa_moments_add, oa_moments_add_binned (csrc/rng.hip), oa_stack_add
(csrc/elementwise.hip) and stats.Statistics(device="cuda") on top of them -- against float64 NumPy loops over the same samples
in the same order.

Tolerances come from the arithmetic alone.  A call does one IEEE add per element of S and of the stack (bit-equal to NumPy) and
one multiply-add per element of C, which the compiler may contract (one rounding instead of two): after k calls
|C - C_ref| <= k 2^-52 sum |x_a x_b|.  The binned entry forms x_a = sums[a] / counts[a] first, one more rounding per factor:
k 2^-51 sum |terms| for S and C.  d = 128 / 129 straddle the switch to the grid-stride loop (the grid is capped at 64 blocks of 256
threads = 128^2 elements of C); d = 300 makes every thread loop."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DIMS = [1, 19, 128, 129, 300]
K = 5


def lib():
    from orphics_amd import _lib
    return _lib.load()


def check(rc):
    from orphics_amd._lib import check as c
    return c(rc)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def samples(d, k, seed):
    """k vectors of mixed sign, magnitudes 1e-3 .. 1e3"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], size=(k, d)) * 10.0 ** rng.uniform(-3, 3, size=(k, d))


def accumulators(d):
    return (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(d, dtype=torch.float64, device="cuda"),
            torch.zeros((d, d), dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("d", DIMS)
def test_moments_add(d):
    X = samples(d, K, d)
    n, S, C = accumulators(d)
    Sr, Cr, A = np.zeros(d), np.zeros((d, d)), np.zeros((d, d))
    for x in X:
        xd = dev(x)
        check(lib().oa_moments_add(ptr(xd), d, ptr(n), ptr(S), ptr(C), stream()))
        Sr += x
        Cr += x[:, None] * x[None, :]
        A += np.abs(x[:, None] * x[None, :])
    assert int(n.item()) == K
    assert S.cpu().numpy().tobytes() == Sr.tobytes()
    err = np.abs(C.cpu().numpy() - Cr)
    print("moments_add d=%d: worst |C - C_ref| / bound = %.3f" % (d, (err / (K * 2.0 ** -52 * A)).max()))
    assert np.all(err <= K * 2.0 ** -52 * A)


def _binned_reference(sums, counts):
    d = sums.shape[1]
    Sr, Cr, AS, AC = np.zeros(d), np.zeros((d, d)), np.zeros(d), np.zeros((d, d))
    with np.errstate(divide="ignore", invalid="ignore"):
        for s, c in zip(sums, counts):
            x = s / c.astype(np.float64)
            Sr += x
            Cr += x[:, None] * x[None, :]
            AS += np.abs(x)
            AC += np.abs(x[:, None] * x[None, :])
    return Sr, Cr, AS, AC


def _run_binned(sums, counts):
    k, d = sums.shape
    n, S, C = accumulators(d)
    for s, c in zip(sums, counts):
        sd, cd = dev(s), dev(c)                   # both alive until the launch: a dropped temporary's block is handed out again
        check(lib().oa_moments_add_binned(ptr(sd), ptr(cd), d, ptr(n), ptr(S), ptr(C), stream()))
    return int(n.item()), S.cpu().numpy(), C.cpu().numpy()


@pytest.mark.parametrize("d", DIMS)
def test_moments_add_binned(d):
    rng = np.random.default_rng(100 + d)
    counts = rng.integers(1, 2 ** 40, size=(K, d), dtype=np.int64)
    counts[:, 0] = 2 ** 31 + 1 + np.arange(K)                      # above 2^31 for certain
    sums = samples(d, K, 200 + d) * counts
    n, S, C = _run_binned(sums, counts)
    Sr, Cr, AS, AC = _binned_reference(sums, counts)
    assert n == K
    eS, eC = np.abs(S - Sr), np.abs(C - Cr)
    print("moments_add_binned d=%d: worst S %.3f, C %.3f of the bound" % (d, (eS / (K * 2.0 ** -51 * AS)).max(), (eC / (K * 2.0 ** -51 * AC)).max()))
    assert np.all(eS <= K * 2.0 ** -51 * AS) and np.all(eC <= K * 2.0 ** -51 * AC)


@pytest.mark.parametrize("d", [19, 129])
def test_moments_add_binned_empty_bin(d):
    """An empty bin (count 0, sum 0) in one sample: NaN in that entry of S and in its row and column of C, like NumPy; every other
    entry stays finite and within tolerance."""
    rng = np.random.default_rng(300 + d)
    counts = rng.integers(1, 1000, size=(K, d), dtype=np.int64)
    sums = samples(d, K, 400 + d) * counts
    j = d // 3
    counts[2, j], sums[2, j] = 0, 0.0
    n, S, C = _run_binned(sums, counts)
    Sr, Cr, AS, AC = _binned_reference(sums, counts)
    assert n == K
    assert np.array_equal(np.isnan(S), np.isnan(Sr)) and np.array_equal(np.isnan(C), np.isnan(Cr))
    assert np.isnan(Sr).sum() == 1 and np.isnan(Cr).sum() == 2 * d - 1
    okS, okC = ~np.isnan(Sr), ~np.isnan(Cr)
    assert np.all(np.isfinite(S[okS])) and np.all(np.isfinite(C[okC]))
    assert np.all(np.abs(S - Sr)[okS] <= K * 2.0 ** -51 * AS[okS]) and np.all(np.abs(C - Cr)[okC] <= K * 2.0 ** -51 * AC[okC])


def test_moments_add_binned_from_bin_power():
    """fed as the Monte-Carlo loop feeds it: the interior slots sums[1:-1], counts[1:-1] of an Engine.bin_power result"""
    from orphics_amd.engine import Engine
    from orphics_amd.geometry import FlatGeometry
    ny, nx, k = 64, 64, 3
    e = Engine.get(ny, nx, "f64")
    g = FlatGeometry.from_res((ny, nx), 2.0)
    e.set_laxes(*g.laxes())
    ed = torch.as_tensor(np.arange(200., 4000., 300.), device=e.device)
    ids = e.modl_digitize(ed, half=True)
    nids = ed.numel() + 1
    d = nids - 2
    n, S, C = accumulators(d)
    rng = np.random.default_rng(11)
    hs, hc = [], []
    for i in range(k):
        kk = e.rfft(e.to_real(rng.standard_normal((ny, nx)) * 10.0 ** (i - 1)))
        sums, counts = e.bin_power(kk, kk, 0.37, ids, nids, herm=True)
        assert counts.dtype == torch.int64 and sums.dtype == torch.float64 and sums.numel() == nids
        check(lib().oa_moments_add_binned(ptr(sums[1:-1]), ptr(counts[1:-1]), d, ptr(n), ptr(S), ptr(C), stream()))
        hs.append(sums.cpu().numpy()[1:-1]); hc.append(counts.cpu().numpy()[1:-1])
    hs, hc = np.array(hs), np.array(hc)
    assert hc.min() > 0
    Sr, Cr, AS, AC = _binned_reference(hs, hc)
    assert int(n.item()) == k
    assert np.all(np.abs(S.cpu().numpy() - Sr) <= k * 2.0 ** -51 * AS) and np.all(np.abs(C.cpu().numpy() - Cr) <= k * 2.0 ** -51 * AC)


@pytest.mark.parametrize("n", [1, 1003, 64 * 80])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_stack_add(prec, n):
    from orphics_amd._lib import OA_F32, OA_F64
    k = 4
    X = samples(n, k, 500 + n).astype(np.float32 if prec == "f32" else np.float64)
    acc = torch.zeros(n + 4, dtype=torch.float64, device="cuda")
    ref = np.zeros(n + 4)
    for x in X:
        xd = dev(x)
        check(lib().oa_stack_add(OA_F32 if prec == "f32" else OA_F64, ptr(xd), ptr(acc), n, stream()))
        ref[:n] += x.astype(np.float64)
    assert acc.cpu().numpy().tobytes() == ref.tobytes()          # the four elements behind n included: untouched


def _close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_statistics_on_device_equals_host():
    from orphics_amd import stats
    d, k = 19, 6
    X = samples(d, k, 7)
    X32 = X.astype(np.float32)
    rng = np.random.default_rng(8)
    counts = rng.integers(1, 2 ** 36, size=(k, d), dtype=np.int64)
    sums = samples(d, k, 9) * counts
    planes = rng.standard_normal((4, 24, 40))
    block = samples(d, 11, 10)
    host, devs = stats.Statistics(), stats.Statistics(device="cuda")
    for i in range(k):
        host.add("f64", X[i]); devs.add("f64", dev(X[i]))
        host.add("f32", X32[i]); devs.add("f32", dev(X32[i]))
        host.add("host", X[i]); devs.add("host", X[i])
        host.add_binned("binned", sums[i], counts[i]); devs.add_binned("binned", dev(sums[i]), dev(counts[i]))
    for p in planes:
        host.add_stack("s64", p); devs.add_stack("s64", dev(p))
        host.add_stack("s32", p.astype(np.float32)); devs.add_stack("s32", dev(p.astype(np.float32)))
    host.extend("block", block); devs.extend("block", dev(block))
    host.extend("block", X[0]); devs.extend("block", dev(X[0]))
    # a label fed by kernels that add their own samples
    cell, S, C = devs.device_moments("own", d)
    for i in range(2):
        xd = dev(X[i])
        check(lib().oa_moments_add(ptr(xd), d, ptr(cell), ptr(S), ptr(C), stream()))
        host.add("own", X[i])
    devs.note_samples("own", 2)
    host.allreduce(); devs.allreduce()
    assert int(cell.item()) == 2 and devs.count("own") == 2
    for lab, cnt in (("f64", k), ("f32", k), ("host", k), ("binned", k), ("block", 12), ("own", 2)):
        assert devs.count(lab) == host.count(lab) == cnt
        _close(devs.mean(lab), host.mean(lab))
        _close(devs.cov(lab), host.cov(lab))
        _close(devs.var(lab), host.var(lab))
    for lab in ("s64", "s32"):
        assert devs.stack_count(lab) == host.stack_count(lab) == len(planes)
        _close(devs.stack_sum(lab), host.stack_sum(lab))
    assert sorted(devs.labels_stats()) == sorted(host.labels_stats()) and sorted(devs.labels_stack()) == sorted(host.labels_stack())
