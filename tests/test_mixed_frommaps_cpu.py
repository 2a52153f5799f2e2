"""Batched band input stage of ``oa_qe_mv_maps`` (orphics_amd/csrc/fft_band.hpp: band_rows_body, band_cols_body, band_cols_fold_body)
under the CPU thread emulator (tests/emul/emul_band.cpp) against ``np.fft.rfft2`` with the band rows and columns picked and rotated in
NumPy, and the host-side declaration of the entry.

Geometry: ny = 100 = 4 5 5 rows (three full 32-row chunks + a tail of 4, four segments), nx = 72 (N = 36 = 4 3 3), leg_cols = 19,
leg_rows = 10 (2 rl - 1 = 19: neither band width is a multiple of the 16-wide tiles), inner planes of 32 rows with a pitch (24) wider
than the band.  Tolerances, relative to the largest band value: float64 1e-12, float32 1e-5."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL = os.path.join(HERE, "emul")

NY, NX, WL, RL, MY, OKP = 100, 72, 19, 10, 32, 24
OSTRIDE = MY * OKP + 8
KP = NX // 2 + 16                      # row pitch of the N-grid rotation planes (wider than the band)
FILL = 7 + 7j


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_band.so")
    srcs = [os.path.join(EMUL, "emul_band.cpp"), os.path.join(EMUL, "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("fft_band.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp", "fft_mixed.hpp",
                                            "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _types(prec):
    return (np.float64, np.complex128, 1e-12) if prec == "f64" else (np.float32, np.complex64, 1e-5)


def _band_rows(n):
    """rows of an n-row grid that hold the signed indices 0 .. rl - 1, -(rl - 1) .. -1, in band order"""
    return np.r_[0:RL, n - RL + 1:n]


def _inputs(prec, nmaps, seed=5):
    rdt = _types(prec)[0]
    rng = np.random.default_rng(seed)
    maps = rng.standard_normal((6, NY, NX)).astype(rdt)[:nmaps].copy()      # map m is the same whatever nmaps is
    phi = rng.uniform(0, 2 * np.pi, (NY, KP))
    return maps, np.cos(phi).astype(rdt), np.sin(phi).astype(rdt)


def _run(emu, prec, maps, rot=None):
    rdt, cdt, _ = _types(prec)
    nmaps = maps.shape[0]
    out = np.full(nmaps * OSTRIDE, FILL, dtype=cdt)
    fn = emu.emu_band_maps_f64 if prec == "f64" else emu.emu_band_maps_f32
    c, s = rot if rot is not None else (None, None)
    rc = fn(NY, NX, nmaps, _p(maps), _p(c), _p(s), ctypes.c_long(KP), WL, RL, _p(out), ctypes.c_long(OSTRIDE), ctypes.c_long(OKP), MY)
    assert rc == 0
    return out


def _reference(maps, rot):
    ref = np.fft.rfft2(maps.astype(np.float64))[:, _band_rows(NY), :WL]
    if rot is not None:
        c, s = (r.astype(np.float64)[_band_rows(NY), :WL] for r in rot)
        for q in range(1, maps.shape[0] - 1, 3):
            Q, U = ref[q].copy(), ref[q + 1].copy()
            ref[q], ref[q + 1] = Q * c - U * s, Q * s + U * c
    return ref


def test_segments_and_chunks_of_this_geometry(emu):
    """the geometry exercises what the docstring says: four segments of one 32-row chunk each, the last a tail of 4 rows"""
    assert emu.emu_band_segments(NY, WL, RL) == 4
    assert NY - 3 * 32 == 4 and (2 * RL - 1) % 16 and WL % 16


@pytest.mark.parametrize("rotate", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("nmaps", [3, 6])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_band_input_stage_against_numpy(emu, prec, nmaps, rotate):
    tol = _types(prec)[2]
    maps, c, s = _inputs(prec, nmaps)
    rot = (c, s) if rotate else None
    out = _run(emu, prec, maps, rot)
    ref = _reference(maps, rot)
    planes = [out[m * OSTRIDE:m * OSTRIDE + MY * OKP].reshape(MY, OKP) for m in range(nmaps)]
    got = np.stack([pl[_band_rows(MY), :WL] for pl in planes])
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("band input stage %s nmaps=%d rotate=%s: max err / max |band| = %.3g" % (prec, nmaps, rotate, err))
    assert err < tol
    # nothing outside the band is written: the other rows, the columns between the band and the pitch, the gaps between the planes
    keep = np.ones(nmaps * OSTRIDE, dtype=bool)
    for m in range(nmaps):
        pl = keep[m * OSTRIDE:m * OSTRIDE + MY * OKP].reshape(MY, OKP)
        pl[_band_rows(MY), :WL] = False
    assert keep.sum() == nmaps * (OSTRIDE - (2 * RL - 1) * WL)
    assert np.all(out[keep] == np.asarray(FILL, dtype=out.dtype))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_one_map_equals_map_zero_of_three_bit_for_bit(emu, prec):
    """batching does not change a map's arithmetic (same segments, chunks and fma order per output)"""
    maps, _, _ = _inputs(prec, 3)
    three = _run(emu, prec, maps)
    one = _run(emu, prec, maps[:1].copy())
    assert np.array_equal(one[:OSTRIDE].view(_types(prec)[0]), three[:OSTRIDE].view(_types(prec)[0]))


def test_ctypes_table_declares_the_entry_with_the_headers_signature():
    from orphics_amd import _lib
    txt = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+oa_qe_mv_maps\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/orphics_amd.h does not declare oa_qe_mv_maps"
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        want.append(ctypes.c_void_p if "*" in arg else {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}[arg.rsplit(" ", 1)[0]])
    res, args = _lib.SIGNATURES["oa_qe_mv_maps"]
    assert res is ctypes.c_int and list(args) == want and len(want) == 23
    assert int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.ABI_VERSION >= 406
