"""NumPy restatement of the orphics.stats / orphics.mpi pieces on the hot path
(TEST INFRASTRUCTURE ONLY).

Pinned: ``tests/golden/make_golden.py`` imports the real
/root/reference/orphics/stats.py + mpi.py in the build container and stores
their outputs in ``tests/golden/*.npz``; ``tests/test_oracle_golden.py`` checks
this restatement against them (bin ids / counts bit-exact, sums <= 1e-15).
"""
import numpy as np


class bin2D(object):
    """stats.py:782-811.  Bins are (e[i-1], e[i]]; id 0 = underflow,
    len(edges) = overflow; ``[1:-1]`` strips both -- and silently drops the last
    real bin when nothing overflows (no ``minlength``), which
    is reproduced here."""

    def __init__(self, modrmap, bin_edges):
        bin_edges = np.asarray(bin_edges)
        self.centers = (bin_edges[1:] + bin_edges[:-1]) / 2.
        self.cents = self.centers
        self.digitized = np.digitize(np.asarray(modrmap).reshape(-1), bin_edges, right=True)
        self.bin_edges = bin_edges
        self.modrmap = modrmap

    def bin(self, data2d, weights=None, err=False, get_count=False, mask_nan=False):
        data2d = np.asarray(data2d)
        if weights is None:
            if mask_nan:
                keep = ~np.isnan(data2d.reshape(-1))
            else:
                keep = np.ones((data2d.size,), dtype=bool)
            count = np.bincount(self.digitized[keep])[1:-1]
            with np.errstate(divide="ignore", invalid="ignore"):
                res = np.bincount(self.digitized[keep], data2d.reshape(-1)[keep])[1:-1] / count
            if err:
                # Reference loops i over 0..nbins-1 against 1-based ids
                # (stats.py:799-801) -> mean map shifted by one bin.  That is
                # a reference bug; ``err_reference_shifted`` reproduces it,
                # this branch computes the intended std of the mean.
                meanmap = np.zeros(self.digitized.shape)
                for i in range(res.size):
                    meanmap[self.digitized == (i + 1)] = res[i]
                with np.errstate(divide="ignore", invalid="ignore"):
                    std = np.sqrt(np.bincount(self.digitized[keep], ((data2d.reshape(-1) - meanmap) ** 2.)[keep])[1:-1]
                                  / (count - 1) / count)
        else:
            count = np.bincount(self.digitized, np.asarray(weights).reshape(-1))[1:-1]
            with np.errstate(divide="ignore", invalid="ignore"):
                res = np.bincount(self.digitized, (data2d * weights).reshape(-1))[1:-1] / count
        if get_count:
            assert not err
            return self.centers, res, count
        if err:
            return self.centers, res, std
        return self.centers, res

    def err_reference_shifted(self, data2d):
        """Bug-compatible stats.py:798-801 (mean map indexed by ``i`` not
        ``i+1``); kept only so the fixture of the reference's own output can be
        matched."""
        data2d = np.asarray(data2d)
        count = np.bincount(self.digitized)[1:-1]
        res = np.bincount(self.digitized, data2d.reshape(-1))[1:-1] / count
        meanmap = np.asarray(self.modrmap).copy().reshape(-1) * 0
        for i in range(self.centers.size):
            if i < res.size:
                meanmap[self.digitized == i] = res[i]
        std = np.sqrt(np.bincount(self.digitized, ((data2d - meanmap.reshape(data2d.shape)) ** 2.).reshape(-1))[1:-1]
                      / (count - 1) / count)
        return self.centers, res, std


def bin_in_annuli(data2d, modrmap, bin_edges):
    """stats.py:853-855."""
    return bin2D(modrmap, bin_edges).bin(data2d)


def cov2corr(cov):
    d = np.sqrt(np.diagonal(cov))
    return cov / np.outer(d, d)


def get_stats(binned_vectors):
    """stats.py:859-898."""
    arr = np.asarray(binned_vectors)
    N = arr.shape[0]
    ret = {}
    ret['mean'] = np.nanmean(arr, axis=0)
    ret['cov'] = np.cov(arr.transpose())
    ret['covmean'] = ret['cov'] / N
    if arr.shape[1] == 1:
        ret['err'] = np.sqrt(ret['cov'])
    else:
        ret['err'] = np.sqrt(np.diagonal(ret['cov']))
    ret['errmean'] = ret['err'] / np.sqrt(N)
    ret['corr'] = 1. if arr.shape[1] == 1 else cov2corr(ret['cov'])
    return ret


def moments_merge(parts):
    """Statistics.allreduce semantics (stats.py:1184-1232): SUM of (n, S, C)."""
    n = sum(p[0] for p in parts)
    S = sum(p[1] for p in parts)
    C = sum(p[2] for p in parts)
    return n, S, C


def moments_mean_cov(n, S, C, ddof=1):
    """stats.py:1311-1370: mean = S/n ; cov = (C - S S^T/n)/(n-ddof)."""
    mean = S / n if n > 0 else np.full(S.shape, np.nan)
    if n <= ddof:
        cov = np.full(C.shape, np.nan)
    else:
        cov = (C - np.outer(S, S) / n) / (n - ddof)
    return mean, cov


def mpi_distribute(num_tasks, avail_cores, allow_empty=False):
    """mpi.py:78-91: contiguous blocks, remainder to the LAST ranks."""
    if not allow_empty:
        assert avail_cores <= num_tasks
    min_each, rem = divmod(num_tasks, avail_cores)
    num_each = np.array([min_each] * avail_cores)
    if rem > 0:
        num_each[-rem:] += 1
    task_range = list(range(num_tasks))
    cumul = np.cumsum(num_each).tolist()
    task_dist = [task_range[x:y] for x, y in zip([0] + cumul[:-1], cumul)]
    return num_each, task_dist


# ---- the binning entries of include/orphics_amd.h (oa_digitize ... oa_bin_power_multi), restated ----------------------------
# Plain NumPy, float64 ids / np.longdouble sums; shares no code with orphics_amd.engine.  Every binned sum also comes with the
# two quantities an error bound of a float64 accumulation in ANY order needs: A[id] = sum of the terms' magnitudes and
# n[id] = number of terms (tests/test_binning_reference_gpu.py).
LD = np.longdouble


def digitize_ref(x, edges):
    """oa_digitize: np.digitize(x, edges, right=True) (#edges strictly below x), NaN -> nedges; int32."""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    ids = np.digitize(x, edges, right=True)
    ids[np.isnan(x)] = edges.size
    return ids.astype(np.int32)


def modl_digitize_ref(ly, lx, pitch, width, edges):
    """oa_modl_digitize: (ids, modl) of shape (ny, pitch); columns >= width (the row padding) get id -1 and modl 0."""
    ly = np.asarray(ly, dtype=np.float64)
    lx = np.asarray(lx, dtype=np.float64)
    modl = np.zeros((ly.size, int(pitch)), dtype=np.float64)
    modl[:, :width] = np.sqrt(ly[:, None] ** 2 + lx[None, :width] ** 2)
    ids = np.full(modl.shape, -1, dtype=np.int32)
    ids[:, :width] = digitize_ref(modl[:, :width].reshape(-1), edges).reshape(ly.size, width)
    return ids, modl


def herm_multiplicity(n, pitch, nxh):
    """m per element of a flat array of n: 1 everywhere (nxh < 0), else by column = index % pitch: 1 at columns 0 and nxh, 2 strictly
    between them, 0 beyond nxh."""
    if nxh < 0:
        return np.ones(n, dtype=np.int64)
    col = np.arange(n, dtype=np.int64) % int(pitch)
    return np.where((col == 0) | (col == nxh), 1, np.where(col < nxh, 2, 0)).astype(np.int64)


def active_region(n, pitch, nxh, active_cols=0, active_rows=0):
    """bool per element: columns < active_cols, and -- only together with a column limit -- rows y < active_rows or
    y > ny - active_rows.  Everything when there is no Hermitian layout or no column limit."""
    keep = np.ones(n, dtype=bool)
    if nxh < 0 or active_cols <= 0:
        return keep
    idx = np.arange(n, dtype=np.int64)
    col, y = idx % int(pitch), idx // int(pitch)
    keep &= col < active_cols
    if active_rows > 0:
        ny = n // int(pitch)
        keep &= (y < active_rows) | (y > ny - active_rows)
    return keep


class Binned(object):
    """sums (longdouble), counts (int64: sums of m), wsums (longdouble: sums of w m, or None), A (longdouble: sums of |term|),
    wA (longdouble: sums of |w| m, or None), n (int64: number of terms), all per id."""

    def __init__(self, sums, counts, wsums, A, n, wA=None):
        self.sums, self.counts, self.wsums, self.A, self.n, self.wA = sums, counts, wsums, A, n, wA


def _per_id(values, sid, starts, nids, dtype):
    out = np.zeros(nids, dtype=dtype)
    if sid.size:
        out[sid[starts]] = np.add.reduceat(values, starts)
    return out


def reduce_terms(term, mag, ids, nids, m, keep, w=None):
    """Per-id sums of term * m (and of mag * m, m, w * m) over the elements with keep, 0 <= id < nids and m > 0.  ``term`` and ``mag``
    are longdouble per element WITHOUT the multiplicity; w (weights, already inside ``term``) only feeds wsums."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    sel = np.flatnonzero(keep & (ids >= 0) & (ids < nids) & (m > 0))
    order = sel[np.argsort(ids[sel], kind="stable")]
    sid = ids[order]
    starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]]) if sid.size else np.zeros(0, dtype=np.int64)
    ml = m[order].astype(LD)
    sums = _per_id(term[order] * ml, sid, starts, nids, LD)
    A = _per_id(np.abs(mag[order]) * ml, sid, starts, nids, LD)
    counts = _per_id(m[order], sid, starts, nids, np.int64)
    n = _per_id(np.ones(order.size, dtype=np.int64), sid, starts, nids, np.int64)
    wsums = None if w is None else _per_id(w[order] * ml, sid, starts, nids, LD)
    wA = None if w is None else _per_id(np.abs(w[order]) * ml, sid, starts, nids, LD)
    return Binned(sums, counts, wsums, A, n, wA)


def bin_ref(data, ids, nids, weights=None, aux=None, mode=0, skip_nan=False, pitch=0, nxh=-1):
    """oa_bin on the stored values ``data`` (their dtype is kept: every float32 is an exact longdouble)."""
    v = np.asarray(data).reshape(-1).astype(LD)
    ids = np.asarray(ids).reshape(-1)
    keep = ~np.isnan(v) if skip_nan else np.ones(v.size, dtype=bool)
    if mode == 1:
        a = np.asarray(aux, dtype=np.float64).astype(LD)
        v = (v - a[np.clip(ids, 0, nids - 1)]) ** 2
    w = None
    if weights is not None:
        w = np.asarray(weights).reshape(-1).astype(LD)
        v = v * w
    return reduce_terms(v, v, ids, nids, herm_multiplicity(v.size, pitch, nxh), keep, w)


def bin_power_ref(k1, k2, norm, ids, nids, weights=None, pitch=0, nxh=-1, active_cols=0, active_rows=0):
    """oa_bin_power: Re(conj k1 k2) * norm of the stored complex values; A holds (|a c| + |b d|) |norm| (|w|) m."""
    k1 = np.asarray(k1).reshape(-1)
    k2 = np.asarray(k2).reshape(-1)
    a, b, c, d = (x.astype(LD) for x in (k1.real, k1.imag, k2.real, k2.imag))
    term = (a * c + b * d) * LD(norm)
    mag = (np.abs(a * c) + np.abs(b * d)) * abs(LD(norm))
    w = None
    if weights is not None:
        w = np.asarray(weights).reshape(-1).astype(LD)
        term, mag = term * w, mag * np.abs(w)
    n = k1.size
    return reduce_terms(term, mag, ids, nids, herm_multiplicity(n, pitch, nxh), active_region(n, pitch, nxh, active_cols, active_rows), w)


def bin_power_multi_ref(fields, pairs, norm, ids, nids, nxh, weights=None, active_cols=0, active_rows=0):
    """oa_bin_power_multi on the (nf, ny, pitch) stack ``fields``: one Binned per (a, b) of ``pairs``; index nf is the per-mode weighted
    sum sum_f w_f k_f.  For that field A is built from sum_f |w_f| |Re k_f| (and Im): the magnitudes its own rounding errors scale with."""
    fields = np.asarray(fields)
    nf, ny, pitch = fields.shape
    re = [fields[f].real.reshape(-1).astype(LD) for f in range(nf)]
    im = [fields[f].imag.reshape(-1).astype(LD) for f in range(nf)]
    mre, mim = [np.abs(x) for x in re], [np.abs(x) for x in im]
    if weights is not None:
        w = [np.asarray(weights)[f].reshape(-1).astype(LD) for f in range(nf)]
        re.append(sum(w[f] * re[f] for f in range(nf)))
        im.append(sum(w[f] * im[f] for f in range(nf)))
        mre.append(sum(np.abs(w[f]) * mre[f] for f in range(nf)))
        mim.append(sum(np.abs(w[f]) * mim[f] for f in range(nf)))
    n = ny * pitch
    # the kernel's column limit: min(active_cols, nxh + 1) when one is given; the multiplicity is 0 beyond nxh anyway
    m, keep = herm_multiplicity(n, pitch, nxh), active_region(n, pitch, nxh, active_cols, active_rows)
    out = []
    for a, b in pairs:
        term = (re[a] * re[b] + im[a] * im[b]) * LD(norm)
        mag = (mre[a] * mre[b] + mim[a] * mim[b]) * abs(LD(norm))
        out.append(reduce_terms(term, mag, ids, nids, m, keep))
    return out
