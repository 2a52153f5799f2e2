"""Run table of the fused divergence + binning launch (orphics_amd/csrc/divbin_runs.hpp) against a NumPy run-length encoding.

The builder is plain C++; tests/emul/divbin_runs_host.cpp gives it a C entry, built here on first use.  Every plane is a coarse-grid id
plane [rows][columns] cut into tiles of C columns the way pack_tiles lays them out ([tile][row][C], zero beyond the plane).  For each
plane with a table a random double plane is summed through the table in table order and compared with np.add.at over the ids."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
WG = 384                      # threads of the float64 1536-row instance: a tile may hold 2 WG entries
MAXLEN = 64


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(EMUL, "libdivbin_runs.so")
    deps = [os.path.join(EMUL, "divbin_runs_host.cpp"), os.path.join(ROOT, "orphics_amd", "csrc", "divbin_runs.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, deps[0]])
    L = ctypes.CDLL(so)
    L.divbin_runs_build.restype = ctypes.c_long
    L.divbin_runs_build.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    return L


def pack(ids, logc):
    rows, cols = ids.shape
    C = 1 << logc
    tiles = (cols + C - 1) // C
    pad = np.zeros((rows, tiles * C), dtype=np.int32)
    pad[:, :cols] = ids
    return np.ascontiguousarray(pad.reshape(rows, tiles, C).transpose(1, 0, 2)), tiles


def build(lib, ids, logc, width, rband, nids, nxh, cap=2 * WG):
    """-> None (no run table) or per tile the list of (id, column in tile, first row, length) and the per-id offsets"""
    ids_t, tiles = pack(ids, logc)
    rows = ids.shape[0]
    ent = np.zeros(tiles * cap + 1, dtype=np.uint64)
    off = np.zeros(tiles * (nids + 1), dtype=np.int32)
    n = lib.divbin_runs_build(ids_t.ctypes.data, tiles, rows, logc, width, rband, nids, nxh, cap, ent.ctypes.data, ent.size, off.ctypes.data)
    if n < 0:
        return None
    off = off.reshape(tiles, nids + 1)
    assert off[0, 0] == 0 and off[-1, -1] == n and np.all(np.diff(off.ravel()) >= 0)
    out = []
    for t in range(tiles):
        e = ent[off[t, 0]:off[t, nids]]
        lo = (e & np.uint64(0xffffffff)).astype(np.int64)
        tab = [(int(i), int(c), int(f), int(ln)) for i, c, f, ln in zip((e >> np.uint64(32)).astype(np.int64), lo >> 24, lo & 0xffff, (lo >> 16) & 0xff)]
        for i in range(nids):             # "the entries of id i" is the range the offsets name
            assert all(x[0] == i for x in tab[off[t, i] - off[t, 0]:off[t, i + 1] - off[t, 0]])
        out.append(tab)
    return out


def kept_rows(rows, rband):
    y = np.arange(rows)
    return ~((y >= rband) & (y <= rows - rband)) if rband > 0 else np.ones(rows, dtype=bool)


def rle_reference(ids, logc, width, rband, nids, nxh):
    rows, cols = ids.shape
    C = 1 << logc
    kept = kept_rows(rows, rband)
    out = []
    for t in range((cols + C - 1) // C):
        tab = []
        for c in range(C):
            col = t * C + c
            if col >= cols or col >= width or col > nxh:
                continue
            v = np.where(kept & (ids[:, col] >= 0) & (ids[:, col] < nids), ids[:, col], -1)
            cut = np.flatnonzero(np.diff(v)) + 1
            for a, b in zip(np.r_[0, cut], np.r_[cut, rows]):
                if v[a] < 0:
                    continue
                for f in range(a, b, MAXLEN):
                    tab.append((int(v[a]), c, int(f), int(min(MAXLEN, b - f))))
        out.append(sorted(tab))
    return out


def check(lib, ids, logc, width, rband, nids, nxh, seed=0):
    got = build(lib, ids, logc, width, rband, nids, nxh)
    assert got is not None, "no run table"
    assert got == rle_reference(ids, logc, width, rband, nids, nxh)
    # a random plane summed through the table, in table order, against np.add.at over the ids
    rows, cols = ids.shape
    C = 1 << logc
    val = np.random.default_rng(seed).standard_normal((rows, cols)) ** 2
    sums = np.zeros(nids)
    for t, tab in enumerate(got):
        for i, c, f, ln in tab:
            s = 0.0
            for y in range(f, f + ln):
                s += val[y, t * C + c]
            sums[i] += s
    ok = kept_rows(rows, rband)[:, None] & (np.arange(cols)[None, :] < min(width, nxh + 1)) & (ids >= 0) & (ids < nids)
    ref = np.zeros(nids)
    np.add.at(ref, ids[ok], val[ok])
    assert np.all(np.abs(sums - ref) <= 1e-13 * np.abs(ref)), np.max(np.abs(sums - ref) / np.maximum(np.abs(ref), 1e-300))
    return got


def radial(rows, cols, nbins, lmax=None):
    ky = np.fft.fftfreq(rows, 1.0 / rows)
    ml = np.hypot(ky[:, None], np.arange(cols)[None, :])
    edges = np.linspace(2.0, lmax if lmax else 0.9 * rows / 2, nbins + 1)
    return np.digitize(ml, edges).astype(np.int32), nbins + 2


@pytest.mark.parametrize("logc", [2, 3])
@pytest.mark.parametrize("rband", [0, 100])
def test_radial_plane(lib, logc, rband):
    ids, nids = radial(256, 129, 19)
    got = check(lib, ids, logc, 129, rband, nids, 128)
    assert sum(len(t) for t in got) > 0 and len(got) == (129 + (1 << logc) - 1) >> logc


@pytest.mark.parametrize("nbins", [1, 68])
def test_few_and_many_ids(lib, nbins):
    ids, nids = radial(256, 129, nbins)
    assert nids in (3, 70)
    check(lib, ids, 2, 129, 90, nids, 128)


def test_column_out_of_range(lib):
    ids, nids = radial(256, 129, 19)
    ids[:, 5] = -1
    ids[:, 10] = nids
    got = check(lib, ids, 2, 129, 0, nids, 128)
    assert not [e for e in got[1] if e[1] == 1] and not [e for e in got[2] if e[1] == 2]      # columns 5 and 10: nothing
    assert [e for e in got[1] if e[1] == 0]


def test_edge_columns_and_beyond_nxh(lib):
    # pitch 132 > nx / 2 + 1 = 129: column 0 and column nx / 2 are kept, 129 .. 131 carry no weight and are dropped
    ids, nids = radial(256, 132, 19, lmax=200.0)
    got = check(lib, ids, 2, 132, 0, nids, 128)
    assert [e for e in got[0] if e[1] == 0] and [e for e in got[32] if e[1] == 0]
    assert all(e[1] == 0 for e in got[32])
    # ... and a band narrower than the plane cuts at `width`
    got = check(lib, ids, 2, 66, 0, nids, 128)
    assert all(e[1] < 2 for e in got[16]) and all(not t for t in got[17:])


def test_chunking_64_65_129(lib):
    ids = np.full((512, 8), -1, dtype=np.int32)
    ids[0:64, 0] = 1
    ids[64:129, 0] = 2
    ids[129:258, 0] = 3
    ids[300:429, 5] = 1
    got = check(lib, ids, 2, 8, 0, 5, 4096)
    assert got[0] == [(1, 0, 0, 64), (2, 0, 64, 64), (2, 0, 128, 1), (3, 0, 129, 64), (3, 0, 193, 64), (3, 0, 257, 1)]
    assert got[1] == [(1, 1, 300, 64), (1, 1, 364, 64), (1, 1, 428, 1)]


def test_first_and_last_kept_row(lib):
    ids = np.full((256, 4), 2, dtype=np.int32)
    got = check(lib, ids, 2, 4, 40, 4, 4096)       # kept: y < 40 and y > 216
    assert [e for e in got[0] if e[1] == 0] == [(2, 0, 0, 40), (2, 0, 217, 39)]
    got = check(lib, ids, 2, 4, 0, 4, 4096)        # every row: the run reaches row 0 and row 255
    assert [e for e in got[0] if e[1] == 3] == [(2, 3, 0, 64), (2, 3, 64, 64), (2, 3, 128, 64), (2, 3, 192, 64)]


def test_checkerboard_has_no_table(lib):
    y, x = np.mgrid[0:256, 0:129]
    ids = ((x + y) & 1).astype(np.int32) + 1
    assert build(lib, ids, 2, 129, 0, 4, 128) is None
    # the same ids fit when the cap allows one entry per point: the refusal is the cap's, not the plane's
    got = build(lib, ids, 2, 129, 0, 4, 128, cap=1024)
    assert got is not None and got == rle_reference(ids, 2, 129, 0, 4, 128)
