"""CPU: the pieces of ``oa_mc_run_mv_windowed`` on map sides 2^a 3^b 5^c under the thread emulator (tests/emul/emul_band_mf.cpp) against
NumPy -- the mean-field stacks from the inner planes of a band grid (``band_stack_add_multi_body``, orphics_amd/csrc/mc_pol.hpp), the
mixed-radix column transform of three planes in one launch (``mr_col_body`` with the plane on grid y), the pruned column DFT of three row
planes with the Q,U -> E,B rotation in the fold -- and the host-only surface: the ABI version and the driver's docstring.

Tolerances relative to the largest value: float64 1e-12, float32 1e-5 (the conventions of test_mixed_windowed_cpu.py); the stacks are
exact: the reference repeats the kernel's arithmetic (double accumulation in estimator order)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL = os.path.join(HERE, "emul")
SENT = -7.5


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_band_mf.so")
    srcs = [os.path.join(EMUL, f) for f in ("emul_band_mf.cpp", "emul_band.cpp", "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("mc_pol.hpp", "fft_band.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp",
                                            "fft_mixed.hpp", "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _types(prec):
    return (np.float64, np.complex128, 1e-12) if prec == "f64" else (np.float32, np.complex64, 1e-5)


def _band_row(i, r, m):
    return i if i < r else i - (2 * r - 1) + m


# ---- the stacks from the inner planes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("w,r", [(13, 7), (16, 16), (17, 1)])
@pytest.mark.parametrize("weights", [False, True], ids=["plain", "mv"])
@pytest.mark.parametrize("nest", [1, 5])
def test_band_stacks_against_a_numpy_loop(emu, nest, weights, w, r, prec):
    """nest inner 32 x 32 kappa_hat planes (and inner weights) onto (60, 46-pitch) N-grid float64 stacks: band row i sits at row i or
    i - (2 r - 1) + rows of either grid; each stack += its plane, the MV stack += sum_e w_e k_e formed in double in estimator order --
    exact against the same arithmetic in NumPy for both precisions; a second call adds again; outside the band the sentinel stays.
    r = 16 fills 31 of the 32 inner rows, w = 17 is the inner grid's Mx / 2 + 1, pitch 46 is odd."""
    rdt, cdt, _ = _types(prec)
    iny, ipitch, any_, apitch = 32, 32, 60, 46
    rng = np.random.default_rng(100 * nest + 10 * w + r)
    k = (rng.standard_normal((nest, iny, ipitch)) + 1j * rng.standard_normal((nest, iny, ipitch))).astype(cdt)
    wt = rng.uniform(0.1, 1.0, (nest, iny, ipitch)).astype(rdt)
    nacc = nest + (1 if weights else 0)
    acc = np.full((nacc, any_, apitch, 2), SENT, dtype=np.float64)
    fn = emu.emu_band_stack_multi_f64 if prec == "f64" else emu.emu_band_stack_multi_f32
    ref = acc.copy()
    for rep in range(2):
        rc = fn(_p(k), ctypes.c_long(iny * ipitch), _p(wt) if weights else None, ctypes.c_long(iny * ipitch), nest, _p(acc), int(weights), iny,
                ctypes.c_long(ipitch), any_, ctypes.c_long(apitch), w, r)
        assert rc == 0
        for i in range(2 * r - 1):
            si, ai = _band_row(i, r, iny), _band_row(i, r, any_)
            mr, mi = np.zeros(w), np.zeros(w)
            for e in range(nest):
                vr, vi = k[e, si, :w].real.astype(np.float64), k[e, si, :w].imag.astype(np.float64)
                ref[e, ai, :w, 0] += vr
                ref[e, ai, :w, 1] += vi
                if weights:
                    ww = wt[e, si, :w].astype(np.float64)
                    mr = mr + ww * vr
                    mi = mi + ww * vi
            if weights:
                ref[nest, ai, :w, 0] += mr
                ref[nest, ai, :w, 1] += mi
        assert np.array_equal(acc, ref), rep
    band = np.zeros((any_, apitch), dtype=bool)
    band[[_band_row(i, r, any_) for i in range(2 * r - 1)], :w] = True
    assert band.sum() == (2 * r - 1) * w and np.all(acc[:, ~band] == SENT) and np.all(acc[:, band] != SENT)


def test_band_stacks_refuse_a_band_beyond_a_plane(emu):
    k = np.zeros((1, 32, 32), dtype=np.complex128)
    acc = np.zeros((1, 60, 46, 2))
    call = lambda w, r: emu.emu_band_stack_multi_f64(_p(k), ctypes.c_long(1024), None, ctypes.c_long(0), 1, _p(acc), 0, 32, ctypes.c_long(32), 60,
                                                     ctypes.c_long(46), w, r)
    assert call(33, 4) != 0 and call(8, 17) != 0 and call(8, 0) != 0 and call(8, 4) == 0


# ---- the batched column launch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("inverse", [1, 0], ids=["inverse", "forward"])
@pytest.mark.parametrize("ip", [0, 1], ids=["two-buffer", "in-place-stages"])
@pytest.mark.parametrize("ny", [60, 300])
def test_three_planes_in_one_column_launch(emu, ny, ip, inverse, prec):
    """three (ny, 27) planes (23 columns transformed: not a multiple of the column tile; pitch 27 odd; a gap between the planes) in ONE
    launch with the plane on grid y, in place as the sequencer runs it: plane b == the single-plane launch of today (strides 0, grid
    y = 1, out of place) bit for bit, which == NumPy's transform along the axis; columns beyond the width and the gap keep their
    sentinel"""
    rdt, cdt, tol = _types(prec)
    pitch, width, gap, nplanes = 27, 23, 5, 3
    pstride = ny * pitch + gap
    rng = np.random.default_rng(ny + 2 * ip + inverse)
    buf = np.full(nplanes * pstride, SENT + 3j, dtype=cdt)
    planes = [buf[b * pstride:b * pstride + ny * pitch].reshape(ny, pitch) for b in range(nplanes)]
    for pl in planes:
        pl[:, :width] = (rng.standard_normal((ny, width)) + 1j * rng.standard_normal((ny, width))).astype(cdt)
    src = [pl.copy() for pl in planes]
    fn = emu.emu_cols_batch_f64 if prec == "f64" else emu.emu_cols_batch_f32
    singles = []
    for b in range(nplanes):
        out = np.full((ny, pitch), SENT + 3j, dtype=cdt)
        rc = fn(ny, 1, _p(src[b]), _p(out), ctypes.c_long(pitch), width, inverse, ctypes.c_long(0), ip)
        assert rc == 0                                     # (2: no in-place form of this length -- both lengths have one)
        singles.append(out)
    assert fn(ny, nplanes, _p(buf), _p(buf), ctypes.c_long(pitch), width, inverse, ctypes.c_long(pstride), ip) == 0
    for b in range(nplanes):
        assert np.array_equal(planes[b].view(rdt), singles[b].view(rdt)), b
        x = src[b][:, :width].astype(np.complex128)
        ref = np.fft.ifft(x, axis=0) * ny if inverse else np.fft.fft(x, axis=0)
        err = np.max(np.abs(singles[b][:, :width] - ref)) / np.max(np.abs(ref))
        assert err < tol, (b, err)
        assert np.all(planes[b][:, width:] == cdt(SENT + 3j))
    for b in range(nplanes - 1):
        assert np.all(buf[b * pstride + ny * pitch:(b + 1) * pstride] == cdt(SENT + 3j))
    assert not np.array_equal(planes[0], planes[1])


# ---- the fold with the rotation, three planes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("ny,wl,rl", [(60, 13, 7), (300, 21, 9)])
def test_fold_rotates_the_pair_of_three_planes(emu, ny, wl, rl, prec):
    """band_cols_body<T, 3> + band_cols_fold_body with rot_c / rot_s: planes 1 and 2 are E = Q c - U s and B = Q s + U c of NumPy's
    pruned column DFT (c, s read from (ny, 46-pitch) N-grid planes at the same mode), plane 0 is unrotated; without the planes all three
    are the plain DFT; outside the band the (32, 24) inner planes keep their sentinel"""
    rdt, cdt, tol = _types(prec)
    my, okp, rp = 32, 24, 46
    rng = np.random.default_rng(ny + wl)
    rows = (rng.standard_normal((3, ny, wl)) + 1j * rng.standard_normal((3, ny, wl))).astype(cdt)
    phi = rng.uniform(0, 2 * np.pi, (ny, rp))
    c, s = np.cos(2 * phi).astype(rdt), np.sin(2 * phi).astype(rdt)
    fn = emu.emu_band_cols3_f64 if prec == "f64" else emu.emu_band_cols3_f32
    full = np.fft.fft(rows.astype(np.complex128), axis=1)
    nrow = [_band_row(i, rl, ny) for i in range(2 * rl - 1)]
    irow = [_band_row(i, rl, my) for i in range(2 * rl - 1)]
    dft = full[:, nrow, :]
    c64, s64 = c.astype(np.float64)[nrow, :wl], s.astype(np.float64)[nrow, :wl]
    for rot in (True, False):
        out = np.full((3, my, okp), SENT + 3j, dtype=cdt)
        rc = fn(ny, _p(rows), wl, rl, _p(c) if rot else None, _p(s) if rot else None, ctypes.c_long(rp), _p(out), ctypes.c_long(my * okp),
                ctypes.c_long(okp), my)
        assert rc == 0
        ref = dft.copy()
        if rot:
            ref[1], ref[2] = dft[1] * c64 - dft[2] * s64, dft[1] * s64 + dft[2] * c64
        got = out[:, irow, :wl]
        err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
        print("fold B=3 ny=%d %s rot=%s: max err / max |value| = %.3g" % (ny, prec, rot, err))
        assert err < tol
        band = np.zeros((my, okp), dtype=bool)
        band[np.ix_(irow, np.arange(wl))] = True
        assert np.all(out[:, ~band] == cdt(SENT + 3j))
        if rot:
            assert np.max(np.abs(got[1] - dft[1])) > 0.1 * np.max(np.abs(dft[1]))     # the rotation did act


# ---- host surface -----------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_docstring():
    from orphics_amd import _lib, mc
    with open(os.path.join(ROOT, "include", "orphics_amd.h")) as f:
        hdr = f.read()
    ver = int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION >= 410
    assert 'one_call="band"' in mc.GaussianN0MonteCarloPol.__doc__
