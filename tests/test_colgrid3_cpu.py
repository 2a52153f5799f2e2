"""3 x 2^k column grids of the from-map R-split path under the CPU thread emulator (tests/emul/emul_fft3.cpp): the single-pass column
stage with a 384- / 192-point inverse (col_fband3_body) and the 1536- / 768-point single-pass divergence (col_div3_body) against NumPy,
and the chain column stage -> row stage -> divergence on 3 x 2^k rows against the same chain on the next power of two.  Tolerances are
those of tests/test_emulator_cpu.py for the same bodies on power-of-two grids."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_fft3.so")
    srcs = [os.path.join(EMUL, "emul_fft3.cpp"), os.path.join(EMUL, "emul_fft.cpp")]
    csrc = os.path.join(HERE, "..", "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp", "fft_fband.hpp", "fft_rowqe8.hpp", "fft_mixed.hpp", "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.emu_kpitch.restype = ctypes.c_long
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _axes(ny, nx):
    lyd = 2 * np.pi * np.fft.fftfreq(ny) * 100
    lxd = 2 * np.pi * np.fft.fftfreq(nx) * 100
    lyd[ny // 2] = 0
    lxd[nx // 2] = 0
    return lxd, lyd


def _fband3_reference(Y, ny, FG, FH, lxd, lyd, w):
    """leg planes in the R-LAYOUT (row 4 y_lo + k1) of the 3 ny / 16-row coarse grid from the row pass's planes Y[k1][g][k]"""
    myf = ny // 4
    my3 = 3 * myf // 4
    mq = my3 // 4
    full = np.zeros((ny, w), dtype=np.complex128)
    for k1 in range(4):
        full[k1::4] = np.fft.fft(Y[k1][:, :w], axis=0)
    legs = [full * FH[:, :w], 1j * lxd[None, :w] * FG[:, :w] * full, 1j * lyd[:, None] * FG[:, :w] * full]    # H, Gx, Gy
    outs, fields = [], []
    ylo = np.arange(mq)
    for leg in legs:
        coarse = np.concatenate([leg[:my3 // 2], leg[ny - my3 // 2:]])          # the 3 x 2^k-row spectrum (band-limited legs)
        fields.append(np.fft.ifft(coarse, axis=0) * my3)
        plane = np.zeros((my3, w), dtype=np.complex128)
        for k1 in range(4):
            plane[k1::4] = np.fft.ifft(coarse[k1::4], axis=0) * mq * np.exp(2j * np.pi * k1 * ylo / my3)[:, None]
        outs.append(plane)
    return outs, fields


@pytest.mark.parametrize("packed", [0, 1], ids=["planes", "packed"])
@pytest.mark.parametrize("prec,nmaps,ny,rb", [("f64", 1, 8192, 380), ("f32", 2, 8192, 380), ("f64", 2, 4096, 150), ("f32", 1, 4096, 190),
                                              ("f64", 1, 8192, 768), ("f64", 1, 4096, 384)])
def test_fband_inverse_on_three_quarter_grid(emu, prec, nmaps, ny, rb, packed):
    """col_fband3_body: 2048- (1024-) point forward per k1, filters, 384- (192-) point inverse with one radix-3 stage, R-LAYOUT planes of
    1536 (768) rows; leg bands up to the widest the coarse spectrum holds (rb = 3 ny / 32: every kept bin live)"""
    nx, w = 2048, 21
    myf, my3 = ny // 4, 3 * ny // 16
    rdt, cdt, tol = (np.float64, np.complex128, 1e-12) if prec == "f64" else (np.float32, np.complex64, 4e-6)
    rng = np.random.default_rng(ny + rb)
    kp = emu.emu_kpitch(nx)
    pitch, opitch = 32, 40
    lxd, lyd = _axes(ny, nx)
    band = np.r_[0:rb, ny - rb + 1:ny]
    FG = np.zeros((ny, kp)); FH = np.zeros((ny, kp))
    FG[band, :w] = rng.uniform(0.5, 1.5, (band.size, w))
    FH[band, :w] = rng.uniform(0.5, 1.5, (band.size, w))
    Y = np.zeros((nmaps, 4, myf, pitch), dtype=cdt)
    Y[..., :w] = (rng.standard_normal((nmaps, 4, myf, w)) + 1j * rng.standard_normal((nmaps, 4, myf, w))).astype(cdt)
    outs = [np.full((nmaps, my3, opitch), 5.0 + 0j, dtype=cdt) for _ in range(3)]           # gx, gy, h
    fn = emu.emu3_fband_f64 if prec == "f64" else emu.emu3_fband_f32
    args = [a.astype(rdt) for a in (FG, FH, lxd, lyd)]
    assert fn(ny, nx, _p(Y), ctypes.c_long(pitch), _p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), _p(outs[0]), _p(outs[1]), _p(outs[2]),
              ctypes.c_long(opitch), w, rb, nmaps, ctypes.c_long(4 * myf * pitch), ctypes.c_long(my3 * opitch), packed) == 0
    for m in range(nmaps):
        (rh, rgx, rgy), fields = _fband3_reference(Y[m].astype(np.complex128), ny, FG, FH, lxd, lyd, w)
        for got, want in ((outs[2][m], rh), (outs[0][m], rgx), (outs[1][m], rgy)):
            assert np.abs(got[:, :w] - want).max() < tol * np.abs(want).max()
            assert np.all(got[:, w:] == 5.0)
        # the R-layout encodes the field on the coarse grid: x[y_lo + Mq y_hi] = sum_k1 W_4^(-k1 y_hi) B[k1][y_lo]
        mq = my3 // 4
        B = rh.reshape(mq, 4, w)
        x = np.stack([sum(B[:, k1] * np.exp(2j * np.pi * k1 * yh / 4.0) for k1 in range(4)) for yh in range(4)]).reshape(my3, w)
        assert np.abs(x - fields[0]).max() < 1e-9 * np.abs(fields[0]).max()


@pytest.mark.parametrize("prec,ny_full,my3,w,rb,nmaps", [("f64", 8192, 1536, 37, 664, 1), ("f32", 8192, 1536, 37, 664, 2), ("f64", 8192, 1536, 70, 0, 1),
                                                         ("f64", 4096, 768, 37, 300, 2), ("f32", 4096, 768, 150, 384, 1)])
def test_single_pass_divergence_on_three_quarter_grid(emu, prec, ny_full, my3, w, rb, nmaps):
    """col_div3_body: forward 1536- / 768-point column transform of the two product planes (six 256- / 128-point transforms + one radix-6
    stage) + divergence, with the column-grid row mapping of Fn, ly and the output; more than 16 tiles with 70 / 150 columns"""
    nx = 2048
    rdt, cdt, tol = (np.float64, np.complex128, 1e-11) if prec == "f64" else (np.float32, np.complex64, 4e-6)
    rng = np.random.default_rng(my3 + w)
    kp = emu.emu_kpitch(nx)
    pin = 160
    lxd, lyd = _axes(ny_full, nx)
    prod = np.zeros((nmaps, 2, my3, pin), dtype=cdt)
    prod[..., :w] = rng.standard_normal((nmaps, 2, my3, w)) + 1j * rng.standard_normal((nmaps, 2, my3, w))
    Fn = np.zeros((ny_full, kp), dtype=rdt)
    Fn[:, :w] = rng.uniform(0.5, 1.5, (ny_full, w))
    out = np.full((nmaps, ny_full, kp), 3.0 + 0j, dtype=cdt)
    fn = emu.emu3_cols_div_f64 if prec == "f64" else emu.emu3_cols_div_f32
    assert fn(ny_full, my3, nx, _p(prod[0, 0]), _p(prod[0, 1]), _p(Fn), _p(lxd.astype(rdt)), _p(lyd.astype(rdt)), _p(out), w, rb, ctypes.c_long(pin),
              nmaps, ctypes.c_long(2 * my3 * pin), ctypes.c_long(ny_full * kp)) == 0
    rows = np.r_[0:my3 // 2, ny_full - my3 // 2:ny_full]                     # full-resolution row of coarse row k
    kept = np.arange(my3) if rb == 0 else np.r_[0:rb, my3 - rb + 1:my3]
    for m in range(nmaps):
        A, B = prod[m, 0].astype(np.complex128), prod[m, 1].astype(np.complex128)
        want = Fn[rows][:, :w] * (1j * lxd[None, :w] * np.fft.fft(A[:, :w], axis=0) + 1j * lyd[rows][:, None] * np.fft.fft(B[:, :w], axis=0))
        assert np.abs(out[m][rows[kept]][:, :w] - want[kept]).max() < tol * np.abs(want).max()
        untouched = np.ones((ny_full, kp), dtype=bool)
        untouched[np.ix_(rows[kept], np.arange(w))] = False
        assert np.all(out[m][untouched] == 3.0)                               # nothing outside the kept rows x columns is written


@pytest.mark.parametrize("prec,ny,nx,wl,wk,rl,rk,mrow", [("f64", 4096, 2048, 20, 30, 150, 300, 1024), ("f32", 4096, 2048, 20, 30, 150, 300, 1024),
                                                         ("f64", 8192, 4096, 9, 12, 380, 664, 1024)])
def test_chain_equals_power_of_two_grid(emu, prec, ny, nx, wl, wk, rl, rk, mrow):
    """column stage -> row stage (R-LAYOUT) -> divergence on 3 ny / 16 rows == the same chain on ny / 4 rows, to rounding: the band
    2 rl + rk <= 3 ny / 16 is alias-free on both (include/orphics_amd.h, COLUMN GRID)"""
    myf, my3 = ny // 4, 3 * ny // 16
    assert max(2 * rl + rk, 2 * rk) <= my3
    rdt, cdt, tol = (np.float64, np.complex128, 1e-11) if prec == "f64" else (np.float32, np.complex64, 2e-5)
    rng = np.random.default_rng(ny + wl)
    kp = emu.emu_kpitch(nx)
    pitch = 32
    lxd, lyd = _axes(ny, nx)
    lband = np.r_[0:rl, ny - rl + 1:ny]
    kband = np.r_[0:rk, ny - rk + 1:ny]
    FG = np.zeros((ny, kp), dtype=rdt); FH = np.zeros((ny, kp), dtype=rdt); Fn = np.zeros((ny, kp), dtype=rdt)
    # filters even in ky, as every isotropic filter is: the filtered legs are REAL fields, which the row stage relies on
    for F in (FG, FH):
        F[:rl, :wl] = rng.uniform(0.5, 1.5, (rl, wl))
        F[ny - rl + 1:, :wl] = F[1:rl, :wl][::-1]
    Fn[kband, :wk] = rng.uniform(0.5, 1.5, (kband.size, wk))
    # the row pass's planes of a REAL map (the row stage packs two real rows per transform)
    x = rng.standard_normal((ny, nx))
    X = np.fft.rfft(x, axis=1)[:, :wl]
    g = np.arange(myf)
    Y = np.zeros((4, myf, pitch), dtype=cdt)
    for k1 in range(4):
        acc = sum(X[n * myf:(n + 1) * myf] * np.exp(-2j * np.pi * n * k1 / 4.0) for n in range(4))
        Y[k1, :, :wl] = acc * np.exp(-2j * np.pi * g * k1 / ny)[:, None]
    fn = emu.emu3_chain_f64 if prec == "f64" else emu.emu3_chain_f32
    res = []
    for my in (myf, my3):
        out = np.full((ny, kp), 3.0 + 0j, dtype=cdt)
        assert fn(ny, nx, my, _p(Y), ctypes.c_long(pitch), _p(FG), _p(FH), _p(Fn), _p(lxd.astype(rdt)), _p(lyd.astype(rdt)), _p(out), wl, wk, rl, rk,
                  mrow) == 0
        res.append(out)
    a, b = res
    scale = np.abs(a[kband][:, :wk]).max()
    assert scale > 0 and np.isfinite(scale)
    assert np.abs(a[kband][:, :wk] - b[kband][:, :wk]).max() < tol * scale
    untouched = np.ones((ny, kp), dtype=bool)
    untouched[np.ix_(kband, np.arange(wk))] = False
    assert np.all(b[untouched] == 3.0)
    # ... and both equal the estimator on the map's own rows
    K = np.fft.fft(np.fft.rfft(x, axis=1)[:, :wl], axis=0)
    pad = np.zeros((ny, nx // 2 + 1), dtype=np.complex128)
    legs = []
    for f in (1j * lxd[None, :wl] * FG[:, :wl] * K, 1j * lyd[:, None] * FG[:, :wl] * K, FH[:, :wl] * K):
        p = pad.copy(); p[:, :wl] = f
        legs.append(np.fft.irfft2(p, s=(ny, nx)))
    want = [np.fft.rfft2(legs[i] * legs[2])[:, :wk] for i in range(2)]
    kap = Fn[:, :wk] * (1j * lxd[None, :wk] * want[0] + 1j * lyd[:, None] * want[1])
    assert np.abs(b[kband][:, :wk] - kap[kband]).max() < 100 * tol * np.abs(kap[kband]).max()
