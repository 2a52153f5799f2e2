"""CPU: the source stage of ``oa_mc_run_mv_windowed`` under the thread emulator (tests/emul/emul_win3.cpp) against NumPy -- the fused
windowed row pass ``row_fft_body<ROW_WIN>`` over three planes in one launch (``RowArgs::nz``, the window shared), the band-only Q,U -> E,B
rotation and the multi-field mean-field stack (orphics_amd/csrc/mc_pol.hpp) -- and the host-only surface: the entry's declaration and
binding, ``debiased_mean``.

Row reference: ``rfft(irfft(row, n=nx) * w_row / ny)[:wcols]`` per plane (the C2R is unnormalised, the scale is 1 / Npix).  Tolerances,
relative to the largest value: float64 1e-12, float32 1e-5 (the conventions of test_mixed_windowed_cpu.py)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL = os.path.join(HERE, "emul")
NROWS = 8


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_win3.so")
    srcs = [os.path.join(EMUL, f) for f in ("emul_win3.cpp", "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("mc_pol.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp", "fft_mixed.hpp",
                                            "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _types(prec):
    return (np.float64, np.complex128, 1e-12) if prec == "f64" else (np.float32, np.complex64, 1e-5)


def _band_rows(ny, rb):
    return np.arange(ny) if not rb else np.r_[0:rb, ny - rb + 1:ny]


# ---- the fused windowed row pass over three planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["w9", "wall"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("nx", [64, 256])
def test_three_planes_share_one_window(emu, nx, prec, full):
    """nz = 3 planes of 8 rows in ONE launch: every plane == rfft(irfft(row) * w_row / ny)[:wcols] with the SAME window (a window offset
    per plane would read rows 8 .. 23 of it: the planes' windows would differ), the columns beyond wcols and the pitch padding of the
    output keep their sentinel, and plane z equals a one-plane launch of it bit for bit"""
    rdt, cdt, tol = _types(prec)
    ny, N, kp = NROWS, nx // 2, nx // 2 + 16
    wcols = N + 1 if full else 9
    opitch, nz = wcols + 3, 3
    rng = np.random.default_rng(nx + wcols)
    rows = np.zeros((nz, ny, kp), dtype=np.complex128)
    rows[:, :, :N + 1] = rng.standard_normal((nz, ny, N + 1)) + 1j * rng.standard_normal((nz, ny, N + 1))
    rows[:, :, N + 1:] = 9 + 9j                        # the pitch padding is never read
    rows = rows.astype(cdt)
    win = (np.outer(np.sin(np.pi * (np.arange(ny) + 0.5) / ny) ** 2, np.sin(np.pi * (np.arange(nx) + 0.5) / nx) ** 2)
           * rng.uniform(0.9, 1.0, (ny, nx))).astype(rdt)
    fn = emu.emu_rows_win3_f64 if prec == "f64" else emu.emu_rows_win3_f32

    def run(planes):
        out = np.full((planes.shape[0], ny, opitch), -7 + 3j, dtype=cdt)
        rc = fn(ny, nx, planes.shape[0], _p(planes), ctypes.c_long(ny * kp), _p(win), _p(out), ctypes.c_long(opitch), ctypes.c_long(ny * opitch),
                ctypes.c_double(1.0 / (ny * nx)), wcols)
        assert rc == 0
        return out
    got = run(rows)
    r64 = rows.astype(np.complex128)[:, :, :N + 1]
    ref = np.fft.rfft(np.fft.irfft(r64, n=nx, axis=2) * win.astype(np.float64)[None] / ny, axis=2)[:, :, :wcols]
    err = np.max(np.abs(got[:, :, :wcols] - ref)) / np.max(np.abs(ref))
    print("ROW_WIN nz=3 nx=%d %s wcols=%d: max err / max |value| = %.3g" % (nx, prec, wcols, err))
    assert err < tol
    assert np.all(got[:, :, wcols:] == cdt(-7 + 3j))
    for z in range(nz):
        one = run(rows[z:z + 1].copy())
        assert np.array_equal(one[0].view(rdt), got[z].view(rdt))
    assert not np.array_equal(got[0], got[1])


# ---- the band rotation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("ny,nx,w,rb", [(16, 64, 21, 5), (16, 64, 33, 0), (8, 256, 129, 3), (32, 32, 70, 9)],
                         ids=["band", "allrows", "wide", "w>hw"])
def test_band_rotation_against_numpy(emu, ny, nx, w, rb, prec):
    """E = Q c - U s, B = Q s + U c (oa_rot2's combination) in place on the band only: 1 ulp of T from the double-precision reference
    (arithmetic in double, one rounding), everything outside the band untouched; w beyond the pitch is clamped to it"""
    rdt, cdt, _ = _types(prec)
    kp = nx // 2 + 16
    rng = np.random.default_rng(ny * nx + w)
    phi = rng.uniform(0, 2 * np.pi, (ny, kp))
    c, s = np.cos(2 * phi).astype(rdt), np.sin(2 * phi).astype(rdt)
    q0 = (rng.standard_normal((ny, kp)) + 1j * rng.standard_normal((ny, kp))).astype(cdt)
    u0 = (rng.standard_normal((ny, kp)) + 1j * rng.standard_normal((ny, kp))).astype(cdt)
    q, u = q0.copy(), u0.copy()
    fn = emu.emu_band_rot2_f64 if prec == "f64" else emu.emu_band_rot2_f32
    assert fn(_p(c), _p(s), _p(q), _p(u), ny, ctypes.c_long(kp), w, rb) == 0
    weff = min(w, kp)
    band = np.zeros((ny, kp), dtype=bool)
    band[np.ix_(_band_rows(ny, rb if 2 * rb - 1 < ny else 0), np.arange(weff))] = True
    c64, s64, q64, u64 = (x.astype(np.float64 if x.dtype.kind == "f" else np.complex128) for x in (c, s, q0, u0))
    e_ref, b_ref = q64 * c64 - u64 * s64, q64 * s64 + u64 * c64
    eps = np.finfo(rdt).eps
    assert np.max(np.abs(q[band] - e_ref[band])) <= 2 * eps * np.max(np.abs(e_ref))
    assert np.max(np.abs(u[band] - b_ref[band])) <= 2 * eps * np.max(np.abs(b_ref))
    assert np.array_equal(q[~band], q0[~band]) and np.array_equal(u[~band], u0[~band])
    assert band.sum() == weff * (2 * rb - 1 if rb else ny)


# ---- the multi-field stack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("nest,mv", [(5, True), (1, False), (6, True), (2, False)])
def test_multi_stack_against_numpy(emu, nest, mv, prec):
    """two launches over kappa's band (13 columns, rows |ky| < 4 of 16): stack e holds twice kappa_e, the MV stack twice
    sum_e w_e kappa_e (1e-15 relative: float64 sums of the stored values), nothing outside the band is touched, and planes behind a
    gap (kstride, wstride larger than a plane) are addressed by their strides"""
    rdt, cdt, _ = _types(prec)
    ny, nx, w, rb = 16, 64, 13, 4
    kp = nx // 2 + 16
    gap = 5
    rng = np.random.default_rng(nest)
    kbuf = (rng.standard_normal((nest, ny * kp + gap)) + 1j * rng.standard_normal((nest, ny * kp + gap))).astype(cdt)
    wbuf = rng.uniform(0.1, 1.0, (nest, ny * kp + 2 * gap)).astype(rdt)
    k = kbuf[:, :ny * kp].reshape(nest, ny, kp)
    wt = wbuf[:, :ny * kp].reshape(nest, ny, kp)
    nacc = nest + (1 if mv else 0)
    start = rng.standard_normal((nacc, ny, kp, 2))
    acc = start.copy()
    fn = emu.emu_stack_multi_f64 if prec == "f64" else emu.emu_stack_multi_f32
    for _ in range(2):
        rc = fn(_p(kbuf), ctypes.c_long(ny * kp + gap), _p(wbuf), ctypes.c_long(ny * kp + 2 * gap), nest, _p(acc), 1 if mv else 0, ny,
                ctypes.c_long(kp), w, rb)
        assert rc == 0
    band = np.zeros((ny, kp), dtype=bool)
    band[np.ix_(_band_rows(ny, rb), np.arange(w))] = True
    k64 = k.astype(np.complex128)
    add = [2 * k64[e] for e in range(nest)]
    if mv:
        add.append(2 * (wt.astype(np.float64) * k64).sum(0))
    for e in range(nacc):
        d = acc[e] - start[e]
        got = d[..., 0] + 1j * d[..., 1]
        assert np.max(np.abs(got[band] - add[e][band])) <= 1e-14 * max(1.0, np.max(np.abs(add[e]))), e
        assert np.array_equal(acc[e][~band], start[e][~band]), e
    # has_mv without weights is refused
    assert fn(_p(kbuf), ctypes.c_long(ny * kp + gap), None, ctypes.c_long(0), nest, _p(acc), 1, ny, ctypes.c_long(kp), w, rb) != 0


# ---- host only ------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_and_bound():
    from orphics_amd import _lib
    txt = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    name = "oa_mc_run_mv_windowed"
    decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
    assert decl, name + " is not declared in the header"
    assert name in _lib.SIGNATURES, name + " is not in _lib.SIGNATURES"
    nargs = len(decl.group(1).split(","))
    assert nargs == len(_lib.SIGNATURES[name][1])
    # oa_mc_run_mv's arguments plus window_real, rot_c, rot_s and host_meanfield
    assert nargs == len(_lib.SIGNATURES["oa_mc_run_mv"][1]) + 4
    for arg in ("window_real", "rot_c", "rot_s", "host_meanfield"):
        assert re.search(r"\b%s\b" % arg, decl.group(1)), arg
    assert int(re.search(r"#define OA_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION >= 409
    # oa_mc_run_mv keeps its signature
    old = re.search(r"\boa_mc_run_mv\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(old.split(",")) == 32 and "window" not in old


def test_debiased_mean_divides_by_the_fourth_moment():
    """``debiased_mean(a, b)`` = ``mean(a, b)`` / mean(w^4), on a driver object that never touched a GPU"""
    from orphics_amd import mc
    d, labels = 3, [("TT", "TT"), ("EB", "EB"), ("TT", "EB")]
    x = np.arange(1.0, 1.0 + len(labels) * d)
    drv = mc.GaussianN0MonteCarloPol.__new__(mc.GaussianN0MonteCarloPol)
    drv.spectra, drv.d = labels, d
    drv.acc = types.SimpleNamespace(mean=lambda label: x)
    w = np.linspace(0.0, 1.0, 12).reshape(3, 4)
    drv.window_moments = (float(np.mean(w ** 2)), float(np.mean(w ** 4)))
    np.testing.assert_allclose(drv.debiased_mean("EB"), x[3:6] / np.mean(w ** 4), rtol=1e-15)
    np.testing.assert_allclose(drv.debiased_mean("EB", "TT"), x[6:9] / np.mean(w ** 4), rtol=1e-15)
    drv.window_moments = (1.0, 1.0)
    assert np.array_equal(drv.debiased_mean("TT"), drv.mean("TT"))
