"""CPU: the NumPy restatement of the binning entries (oracle/stats_oracle.py: digitize_ref ... bin_power_multi_ref), which
tests/test_binning_reference_gpu.py holds the HIP kernels against, is itself checked here against np.bincount on a FULL plane:
a Hermitian half plane is expanded with np.fft's symmetry F[-y, -x] = conj F[y, x], so the multiplicities of the half-plane
reference (1 at columns 0 and nx/2, 2 between, 0 on the row padding) are right exactly when both binnings agree."""
import numpy as np
import pytest

from oracle import stats_oracle as so


def expand(half, nx):
    """full (ny, nx) plane of the half plane half[:, :nx/2 + 1]"""
    ny, nxh = half.shape[0], nx // 2
    full = np.empty((ny, nx), dtype=half.dtype)
    full[:, :nxh + 1] = half[:, :nxh + 1]
    yy = (-np.arange(ny)) % ny
    for x in range(nxh + 1, nx):
        full[:, x] = np.conj(half[yy, nx - x])
    return full


@pytest.mark.parametrize("ny,nx,pad", [(16, 24, 16), (9, 10, 3), (12, 8, 0)])
def test_half_plane_reference_equals_bincount_on_the_full_plane(ny, nx, pad):
    rng = np.random.default_rng(ny * nx)
    nxh, pitch = nx // 2, nx // 2 + 1 + pad
    ly = np.fft.fftfreq(ny, 1.3) * 2 * np.pi
    lx = np.fft.fftfreq(nx, 0.9) * 2 * np.pi
    modl = np.sqrt(ly[:, None] ** 2 + lx[None, :] ** 2)
    edges = np.unique(np.concatenate([[0.0], rng.choice(np.unique(modl)[1:], 6, replace=False), [modl.max() * 0.8]]))   # ties included
    nids = edges.size + 1
    ids_full = np.digitize(modl.reshape(-1), edges, right=True)
    ids_half, modl_half = so.modl_digitize_ref(ly, lx, pitch, nxh + 1, edges)
    assert np.array_equal(ids_half[:, :nxh + 1], ids_full.reshape(ny, nx)[:, :nxh + 1]) and np.array_equal(modl_half[:, :nxh + 1], modl[:, :nxh + 1])
    assert (ids_half[:, nxh + 1:] == -1).all() and (modl_half[:, nxh + 1:] == 0).all()
    # a real map's transform is Hermitian: its half plane, garbage with VALID ids on the row padding
    k1 = np.fft.fft2(rng.standard_normal((ny, nx)))
    k2 = np.fft.fft2(rng.standard_normal((ny, nx)))
    assert np.allclose(expand(k1, nx), k1, rtol=0, atol=1e-12)
    h1 = np.full((ny, pitch), 1e6 + 1e6j)
    h2 = np.full((ny, pitch), 1e6 - 1e6j)
    h1[:, :nxh + 1], h2[:, :nxh + 1] = k1[:, :nxh + 1], k2[:, :nxh + 1]
    ids_h = ids_half.copy()
    ids_h[:, nxh + 1:] = 3
    norm = 0.37
    f1, f2 = expand(h1, nx), expand(h2, nx)
    pw = (np.conj(f1) * f2).real.reshape(-1) * norm
    r = so.bin_power_ref(h1, h2, norm, ids_h, nids, pitch=pitch, nxh=nxh)
    assert np.array_equal(r.counts, np.bincount(ids_full, minlength=nids))
    assert r.counts.sum() == ny * nx and r.n.sum() == ny * (nxh + 1)
    np.testing.assert_allclose(r.sums.astype(np.float64), np.bincount(ids_full, pw, minlength=nids), rtol=1e-12, atol=1e-12 * np.abs(pw).sum())
    assert (r.A >= np.abs(r.sums)).all()
    # the same through the real-plane entry, weighted (an even-symmetric weight plane) and unweighted
    p_half = np.full((ny, pitch), 1e6)
    p_half[:, :nxh + 1] = (np.conj(k1) * k1).real[:, :nxh + 1]
    w_half = rng.uniform(0.5, 2.0, (ny, pitch))
    p_full, w_full = expand(p_half, nx).reshape(-1), expand(w_half, nx).reshape(-1)
    r = so.bin_ref(p_half, ids_h, nids, pitch=pitch, nxh=nxh)
    assert np.array_equal(r.counts, np.bincount(ids_full, minlength=nids))
    np.testing.assert_allclose(r.sums.astype(np.float64), np.bincount(ids_full, p_full, minlength=nids), rtol=1e-12)
    r = so.bin_ref(p_half, ids_h, nids, weights=w_half, pitch=pitch, nxh=nxh)
    np.testing.assert_allclose(r.wsums.astype(np.float64), np.bincount(ids_full, w_full, minlength=nids), rtol=1e-12)
    np.testing.assert_allclose(r.sums.astype(np.float64), np.bincount(ids_full, p_full * w_full, minlength=nids), rtol=1e-12)
    # the multi-spectrum restatement is the pairwise one
    m = so.bin_power_multi_ref(np.stack([h1, h2]), [(0, 1), (1, 1)], norm, ids_h, nids, nxh)
    assert np.array_equal(m[0].sums, so.bin_power_ref(h1, h2, norm, ids_h, nids, pitch=pitch, nxh=nxh).sums)
    assert np.array_equal(m[1].sums, so.bin_power_ref(h2, h2, norm, ids_h, nids, pitch=pitch, nxh=nxh).sums)


def test_flat_reference_drops_what_the_contract_drops():
    """flat layout: ids outside [0, nids), NaN data under skip_nan and their weights are dropped; mode 1 bins squared deviations"""
    ids = np.array([0, 0, 1, -1, 1, 4, 2 ** 31 - 1, 3, 3, 3], dtype=np.int32)
    data = np.array([1.0, 2.0, np.nan, 5.0, 4.0, 7.0, 9.0, 1.5, np.nan, 2.5], dtype=np.float32)
    w = np.array([1.0, 2.0, 1e6, 1e6, 0.5, 1e6, 1e6, 2.0, 1e6, -1.0], dtype=np.float32)
    r = so.bin_ref(data, ids, 4, skip_nan=True)
    assert np.array_equal(r.counts, [2, 1, 0, 2]) and np.array_equal(r.sums, [3.0, 4.0, 0.0, 4.0])
    r = so.bin_ref(data, ids, 4, weights=w, skip_nan=True)
    assert np.array_equal(r.wsums, [3.0, 0.5, 0.0, 1.0]) and np.array_equal(r.sums, [5.0, 2.0, 0.0, 0.5]) and np.array_equal(r.A, [5.0, 2.0, 0.0, 5.5])
    aux = np.array([1.0, 1.0, 0.0, 2.0])
    r = so.bin_ref(np.nan_to_num(data), ids, 4, aux=aux, mode=1)
    assert np.array_equal(r.sums, [1.0, 10.0, 0.0, 4.5]) and np.array_equal(r.n, [2, 2, 0, 3])
    x = np.array([np.nan, -np.inf, np.inf, 0.0, -0.0, 5e-324, 1.0, np.nextafter(1.0, 2.0)])
    assert np.array_equal(so.digitize_ref(x, [0.0, 1.0]), [2, 0, 2, 0, 0, 1, 1, 2])
    assert np.array_equal(so.active_region(12, 4, 2, active_cols=3, active_rows=1), [True, True, True, False] + [False] * 8)
    assert np.array_equal(so.active_region(12, 4, 2, active_cols=0, active_rows=1), [True] * 12)
