"""Windowed front end of ``oa_mc_run_windowed`` on map sides 2^a 3^b 5^c (orphics_amd/csrc/fft_band.hpp: band_rows_win_body) under the CPU
thread emulator (tests/emul/emul_band_win.cpp) against NumPy, and the ``one_call`` argument of ``mc.GaussianN0MonteCarlo``.

Row lengths of the two test geometries: 300 x 360 (N = 180 = 4 3 3 5: every radix) and 600 x 750 (N = 375 = 3 5 5 5, odd).  The row
kernel handles rows independently, so the row tests run NROWS rows of each geometry; the whole front end (inverse columns -> row kernel ->
pruned column DFT) runs on full planes.  Tolerances, relative to the largest band value: float64 1e-12, float32 1e-5.

The row reference is ``np.fft.rfft(c2r(row) * w_row * scale)[:wl]`` with ``c2r(row) = np.fft.irfft(row, n=nx) * nx`` the unnormalised
inverse and scale = 1 / Npix, i.e. ``rfft(irfft(row, n=nx) * w_row / ny)``."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL = os.path.join(HERE, "emul")

SHAPES = [(300, 360), (600, 750)]
NROWS = 6


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_band_win.so")
    srcs = [os.path.join(EMUL, f) for f in ("emul_band_win.cpp", "emul_band.cpp", "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("fft_band.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp", "fft_mixed.hpp",
                                            "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _types(prec):
    return (np.float64, np.complex128, 1e-12) if prec == "f64" else (np.float32, np.complex64, 1e-5)


def _window(ny, nx, rng):
    """a smooth taper-like window with values in (0, 1], different in every row and column"""
    y = np.sin(np.pi * (np.arange(ny) + 0.5) / ny) ** 2
    x = np.sin(np.pi * (np.arange(nx) + 0.5) / nx) ** 2
    return np.outer(y, x) * rng.uniform(0.9, 1.0, (ny, nx))


def _row_inputs(nx, prec, nplanes, seed):
    """nplanes x NROWS spectrum rows of nx / 2 + 1 columns at pitch kp (imaginary parts at the self-conjugate columns included: the
    kernel drops them, as irfft does) and a window for the NROWS rows"""
    rdt, cdt, _ = _types(prec)
    N, kp = nx // 2, nx // 2 + 16
    rng = np.random.default_rng(seed)
    rows = np.zeros((6, NROWS, kp), dtype=np.complex128)
    rows[:, :, :N + 1] = rng.standard_normal((6, NROWS, N + 1)) + 1j * rng.standard_normal((6, NROWS, N + 1))
    rows[:, :, N + 1:] = 9 + 9j                       # the pitch padding is never read
    win = _window(NROWS, nx, rng)
    return rows[:nplanes].astype(cdt).copy(), win.astype(rdt)


def _run_rows(emu, prec, nx, rows, win, wl, npix):
    cdt = _types(prec)[1]
    B, kp = rows.shape[0], rows.shape[2]
    out = np.zeros((B, NROWS, wl), dtype=cdt)
    fn = emu.emu_band_rows_win_f64 if prec == "f64" else emu.emu_band_rows_win_f32
    rc = fn(NROWS, nx, B, _p(rows), ctypes.c_long(kp), _p(win), ctypes.c_double(1.0 / npix), wl, _p(out))
    assert rc == 0
    return out


@pytest.mark.parametrize("full", [False, True], ids=["wl67", "wlN"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["300x360", "600x750"])
def test_windowed_row_kernel_against_numpy(emu, shape, prec, full):
    ny, nx = shape
    N = nx // 2
    wl = N if full else 67
    rows, win = _row_inputs(nx, prec, 1, seed=nx)
    got = _run_rows(emu, prec, nx, rows, win, wl, ny * nx)[0]
    r64 = rows[0].astype(np.complex128)[:, :N + 1]
    ref = np.fft.rfft(np.fft.irfft(r64, n=nx, axis=1) * nx * win.astype(np.float64) / (ny * nx), axis=1)[:, :wl]
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("windowed row kernel %dx%d %s wl=%d: max err / max |band| = %.3g" % (ny, nx, prec, wl, err))
    assert err < _types(prec)[2]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["300x360", "600x750"])
def test_plane_of_a_batch_of_three_equals_the_single_plane_run_bit_for_bit(emu, shape, prec):
    ny, nx = shape
    rows, win = _row_inputs(nx, prec, 3, seed=nx + 1)
    three = _run_rows(emu, prec, nx, rows, win, 67, ny * nx)
    rdt = _types(prec)[0]
    for b in range(3):
        one = _run_rows(emu, prec, nx, rows[b:b + 1].copy(), win, 67, ny * nx)
        assert np.array_equal(one[0].view(rdt), three[b].view(rdt))
    assert not np.array_equal(three[0], three[1])


def _band_rows(n, rl):
    return np.r_[0:rl, n - rl + 1:n]


@pytest.mark.parametrize("shape,prec,wl,rl,my,okp", [((300, 360), "f64", 67, 60, 256, 129), ((300, 360), "f32", 67, 60, 256, 129),
                                                    ((600, 750), "f64", 133, 120, 256, 257)],
                         ids=["300x360-f64", "300x360-f32", "600x750-f64"])
def test_whole_front_end_against_numpy(emu, shape, prec, wl, rl, my, okp):
    """inverse columns (in place) -> windowed row kernel -> emulated pruned column DFT == rfft2(irfft2(k) * w) on the leg band, and
    nothing outside the band of the inner plane is written"""
    ny, nx = shape
    rdt, cdt, tol = _types(prec)
    N, kp = nx // 2, nx // 2 + 16
    rng = np.random.default_rng(ny + nx)
    k = np.zeros((ny, kp), dtype=np.complex128)
    k[:, :N + 1] = np.fft.rfft2(rng.standard_normal((ny, nx)))
    k[:, N + 1:] = 9 + 9j
    win = _window(ny, nx, rng).astype(rdt)
    kk = k.astype(cdt)
    k64 = kk.astype(np.complex128)[:, :N + 1]          # (the emulated sequencer transforms kk's columns in place)
    fill = np.asarray(7 + 7j, dtype=cdt)
    out = np.full((my, okp), fill, dtype=cdt)
    fn = emu.emu_band_win_front_f64 if prec == "f64" else emu.emu_band_win_front_f32
    rc = fn(ny, nx, _p(kk), ctypes.c_long(kp), _p(win), wl, rl, _p(out), ctypes.c_long(okp), my)
    assert rc == 0
    ref = np.fft.rfft2(np.fft.irfft2(k64, s=(ny, nx)) * win.astype(np.float64))[_band_rows(ny, rl), :wl]
    got = out[_band_rows(my, rl), :wl]
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("windowed front end %dx%d %s: max err / max |band| = %.3g" % (ny, nx, prec, err))
    assert err < tol
    keep = np.ones((my, okp), dtype=bool)
    keep[np.ix_(_band_rows(my, rl), np.arange(wl))] = False
    assert np.all(out[keep] == fill)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_c2r_with_the_window_at_the_row_store_against_numpy(emu, prec):
    """the unfused flow's C2R on a mixed-radix side (MrRowArgs::mul): == irfft2(k) * w"""
    ny, nx = 60, 360
    rdt, cdt, tol = _types(prec)
    N, kp = nx // 2, nx // 2 + 16
    rng = np.random.default_rng(8)
    k = np.zeros((ny, kp), dtype=np.complex128)
    k[:, :N + 1] = np.fft.rfft2(rng.standard_normal((ny, nx)))
    win = _window(ny, nx, rng).astype(rdt)
    kk = k.astype(cdt)
    out = np.zeros((ny, nx), dtype=rdt)
    fn = emu.emu_c2r_win_f64 if prec == "f64" else emu.emu_c2r_win_f32
    assert fn(ny, nx, _p(kk), ctypes.c_long(kp), _p(win), ctypes.c_double(1.0 / (ny * nx)), _p(out)) == 0
    ref = np.fft.irfft2(kk.astype(np.complex128)[:, :N + 1], s=(ny, nx)) * win.astype(np.float64)
    assert np.max(np.abs(out - ref)) / np.max(np.abs(ref)) < tol


# ---- the one_call argument of mc.GaussianN0MonteCarlo (no GPU: a stub engine and estimator) ------------------------------------------
class _StubEngine(object):
    def __init__(self, pow2, mixed):
        self.ny, self.nx, self.npix, self.pow2, self.mixed, self.device = 4, 6, 24, pow2, mixed, None

    def modl_digitize(self, edges, half=True):
        return np.zeros((self.ny, self.nx // 2 + 1), dtype=np.int32)

    def to_real(self, w):
        return np.asarray(w)


class _StubGeom(object):
    area = 1.0


class _StubEstimator(object):
    def __init__(self, pow2=False, mixed=True, band=True):
        self.eng, self.geom, self._band = _StubEngine(pow2, mixed), _StubGeom(), band

    def _hcreal(self, e, a):
        return a

    def bind_bins(self, ids, nids, norm):
        return self

    def one_call(self):
        return self.eng.pow2 or (self.eng.mixed and self._band)


def _driver(q, **kw):
    from orphics_amd import mc
    return mc.GaussianN0MonteCarlo(q, np.ones((4, 4)), np.linspace(1.0, 2.0, 4), comm=object(), **kw)


def test_one_call_argument_handling():
    from orphics_amd import mc
    from orphics_amd._lib import OrphicsAmdError
    sig = inspect.signature(mc.GaussianN0MonteCarlo.__init__)
    assert sig.parameters["one_call"].default is None and list(sig.parameters)[-1] == "one_call"
    w = np.ones((4, 6))
    # None: the refusal of a window on a side that is no power of two stays, and now names both ways out
    with pytest.raises(OrphicsAmdError, match="window") as exc:
        _driver(_StubEstimator(), window=w)
    assert "one_call=True" in str(exc.value) and "one_call=False" in str(exc.value)
    # True: taken where the estimator has its one-call path, refused by name where it has none
    assert _driver(_StubEstimator(), window=w, one_call=True).one_call is True
    for q in (_StubEstimator(band=False), _StubEstimator(mixed=False)):
        with pytest.raises(OrphicsAmdError, match="one_call=False"):
            _driver(q, window=w, one_call=True)
    # False: any side
    for q in (_StubEstimator(), _StubEstimator(band=False), _StubEstimator(mixed=False), _StubEstimator(pow2=True)):
        assert _driver(q, window=w, one_call=False).one_call is False
    # power-of-two sides and unwindowed drivers are untouched by the argument
    assert _driver(_StubEstimator(pow2=True), window=w).window is not None
    assert _driver(_StubEstimator()).window is None
    with pytest.raises(ValueError):
        _driver(_StubEstimator(), window=np.ones((3, 3)), one_call=True)


def test_host_loop_is_taken_only_with_a_window_and_one_call_false():
    from orphics_amd import mc
    src = inspect.getsource(mc.GaussianN0MonteCarlo.run_local)
    assert "self.window is not None and self.one_call is False" in src and "_run_host" in src
    host = inspect.getsource(mc.GaussianN0MonteCarlo._run_host)
    for word in ("grf_hc", "irfft", "self.window", "tt_moments", "reconstruct_tt_from_map"):
        assert word in host
