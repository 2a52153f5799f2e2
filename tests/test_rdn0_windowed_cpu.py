"""CPU: the host-only surface of the windowed RDN0 (``oa_mc_run_rdn0_windowed``, ``oa_grf_hc_icols``, ``OA_OPT_DRAW_FUSED``) and the draw
fused into inverse column pass 1 (``col_grf_body`` / ``GrfColLoad`` / ``grf_col_fill``, orphics_amd/csrc/fft_kernels.hpp) under the thread
emulator (tests/emul/emul_grf_icols.cpp) against the NumPy draw statement of oracle/rng_oracle.py taken through ``np.fft.ifft`` along the
columns, times Ny.

Host ``logf`` / ``sinf`` / ``cosf`` are not the device's, so the emulator pins counters, self-conjugate edge rules and the index mapping of the
lane-pair split, not bits (the bits are pinned on the GPU: tests/test_grf_icols_gpu.py).

Tolerance.  A drawn mode is within the bound of ``rng_oracle.grf_hc(..., with_bound=True)`` -- the one tests/test_rng_parity_gpu.py holds the
draw kernels to.  An output of the unscaled inverse column transform is a sum of Ny modes with unit-modulus factors, each mixing the real and
the imaginary part, so its error is at most Ny times the largest per-part bound of its column."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import rng_oracle as ro

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL = os.path.join(HERE, "emul")


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_grf_icols.so")
    srcs = [os.path.join(EMUL, f) for f in ("emul_grf_icols.cpp", "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("philox.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp", "fft_mixed.hpp",
                                            "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.emu_grf_kpitch.restype = ctypes.c_long
    for name in ("emu_grf_icols_f64", "emu_grf_icols_f32"):
        getattr(lib, name).argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_long, ctypes.c_int, ctypes.c_int]
    return lib


def _run(lib, ny, nx, seed, sid, nreal, cs, prec, tiles=0, plain=0, fill=0.0):
    """(nreal, ny, kp) complex planes of the emulated oa_grf_hc_icols; `cs`: (ny, nx/2 + 1) amplitudes or None; untouched elements = fill"""
    kp = lib.emu_grf_kpitch(nx)
    rdt, cdt = (np.float64, np.complex128) if prec == "f64" else (np.float32, np.complex64)
    out = np.full((nreal, ny, kp), fill, dtype=cdt)
    csp = None
    if cs is not None:
        csp = np.zeros((ny, kp), dtype=rdt)
        csp[:, :nx // 2 + 1] = cs
    fn = lib.emu_grf_icols_f64 if prec == "f64" else lib.emu_grf_icols_f32
    rc = fn(ny, nx, seed, sid, nreal, None if csp is None else csp.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ny * kp,
            tiles, plain)
    assert rc == 0
    return out


def _reference(ny, nx, seed, sid, cs, prec):
    """(Ny x ifft along columns of the NumPy draw, allowed |error| per real number of each output)"""
    plane, bound = ro.grf_hc(ny, nx, seed, sid, covsqrt=cs, with_bound=True, prec=prec)
    ref = np.fft.ifft(plane, axis=0) * ny
    tol = ny * bound.max(axis=(0, 2))
    return ref, np.broadcast_to(tol[None, :], ref.shape)


def _amp(ny, nx):
    y, x = np.meshgrid(np.arange(ny), np.arange(nx // 2 + 1), indexing="ij")
    return 0.5 + ((3 * y + 7 * x) % 11) / 11.0          # no symmetry in y or x: a transposed or mirrored index cannot pass


CASES = [((32, 32), "f64", 0, True), ((32, 32), "f32", 0, False), ((64, 256), "f64", 3, True), ((64, 256), "f64", 0, False)]


@pytest.mark.parametrize("shape,prec,tiles,with_cs", CASES)
def test_emulated_draw_in_the_column_pass_is_the_numpy_statement(emu, shape, prec, tiles, with_cs):
    ny, nx = shape
    nxh = nx // 2
    cs = _amp(ny, nx) if with_cs else None
    seed, sid, nreal = 0x1234567811, 2 ** 32 + 5, 2               # (a stream id above 2^32: both counter words of the stream are live)
    got = _run(emu, ny, nx, seed, sid, nreal, cs, prec, tiles=tiles, fill=-7.5)
    w = min(32 * tiles, nxh + 1) if tiles else nxh + 1            # (64, 256) with 3 tiles: the 96-column band
    for z in range(nreal):
        ref, tol = _reference(ny, nx, seed, sid + z, cs, prec)
        worst = ro.draw_mismatch(got[z, :, :w], ref[:, :w], tol[:, :w])
        print("emulated grf_icols %s %s plane %d: worst |err| / bound %.3g over %d columns" % (shape, prec, z, worst, w))
        assert worst <= 1.0
        # a wrong counter, slot or edge rule is off by O(1) per mode; the bound is ~1e-5 of that
        assert np.abs(ref[:, :w]).max() > 1e3 * tol[:, :w].max() / ny
    assert np.all(got[:, :, w:] == np.asarray(-7.5, dtype=got.dtype))   # nothing is written beyond the columns run / the valid columns


@pytest.mark.parametrize("shape", [(32, 32), (64, 256), (128, 64)])
def test_lane_pair_split_equals_the_per_element_statement(emu, shape):
    """grf_col_fill (one counter per column PAIR, halves swapped between neighbouring lanes) against GrfColLoad::get (one counter per
    element) through the same pipeline on the same host: bit for bit, Nyquist column, column 0 and the mirrored rows included."""
    ny, nx = shape
    cs = _amp(ny, nx)
    for prec in ("f64", "f32"):
        a = _run(emu, ny, nx, 99, 7, 2, cs, prec, plain=0)
        b = _run(emu, ny, nx, 99, 7, 2, cs, prec, plain=1)
        assert np.array_equal(a, b)
        assert np.abs(a[:, :, :nx // 2 + 1]).min() > 0


def test_header_ctypes_and_docstrings_agree():
    import inspect
    from orphics_amd import _lib, mc
    from orphics_amd.engine import Engine
    hdr = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    ver = int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION >= 413
    flat = " ".join(hdr.split())
    protos = {
        "oa_mc_run_rdn0_windowed": "int oa_mc_run_rdn0_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, "
                                   "const void* window_real, int64_t* n, double* S, double* C, void* stream);",
        "oa_grf_hc_icols": "int oa_grf_hc_icols(oa_plan* p, uint64_t seed, uint64_t stream_id, int nreal, const void* covsqrt_hc, void* hc_out, "
                           "long zstride, void* stream);",
    }
    ctype_of = {"oa_plan*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p,
                "double*": ctypes.c_void_p, "uint64_t": ctypes.c_uint64, "long": ctypes.c_long, "int": ctypes.c_int}
    for name, proto in protos.items():
        assert proto in flat, name
        args = [a.strip().rsplit(" ", 1)[0] for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and list(argtypes) == [ctype_of[a] for a in args], name
    enum = re.search(r"enum\s*\{([^}]*OA_OPT_MC_BATCH[^}]*)\}", hdr).group(1)
    assert re.search(r"\bOA_OPT_DRAW_FUSED\s*=\s*7\b", enum)
    assert Engine.OPTIONS["draw_fused"] == 7 and hasattr(Engine, "grf_hc_icols")
    comment = " ".join(hdr[hdr.index("oa_mc_run_rdn0_windowed: oa_mc_run_rdn0's definition"):].split("*/")[0].replace("\n *", " ").split())
    assert "NO mean-field argument" in comment and "carry no mean field" in comment
    sig = inspect.signature(mc.RDN0MonteCarlo.__init__)
    assert list(sig.parameters)[1:] == ["qest", "data", "total_power_half", "bin_edges", "comm", "base_seed", "one_call", "window"]
    assert sig.parameters["window"].default is None
    assert list(inspect.signature(mc.RDN0MonteCarlo.data_bandpowers).parameters) == ["self", "mean_field"]
    assert list(inspect.signature(mc.RDN0MonteCarlo.debiased).parameters) == ["self", "data_bandpowers", "mean_field"]
    doc = " ".join(mc.RDN0MonteCarlo.__doc__.split())
    for piece in ("``window``", "ALREADY apodised", "oa_mc_run_rdn0_windowed", "window_moments", "one_call=None"):
        assert piece in doc, piece
