"""CPU: the host-only surface of the windowed pol / MV RDN0 (``oa_mc_run_rdn0_mv_windowed``, ``oa_grf_mix_icols``,
``RDN0MonteCarloPol.set_window``) and the mixed T, Q, U draw fused into inverse column pass 1 (``col_mix_body`` / ``MixColLoad`` /
``mix_col_normals`` / ``mix_col_fill``, orphics_amd/csrc/fft_kernels.hpp) under the thread emulator (tests/emul/emul_grf_mix_icols.cpp)
against the NumPy draw statement ``rng_oracle.grf_mix(..., rot=...)`` taken through ``np.fft.ifft`` along the columns, times Ny.

Host ``logf`` / ``sinf`` / ``cosf`` are not the device's, so the emulator pins counters, self-conjugate edge rules, the mixing, the rotation
and the index mapping of the once-per-triple evaluation, not bits (the bits are pinned on the GPU: tests/test_grf_mix_icols_gpu.py).

Tolerance (the argument of tests/test_rdn0_windowed_cpu.py).  A drawn mode is within the bound of ``rng_oracle.grf_mix(...,
with_bound=True)``.  An output of the unscaled inverse column transform is a sum of Ny modes with unit-modulus factors, each mixing the real
and the imaginary part, so its error is at most Ny times the largest per-part bound of its column."""
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
    so = os.path.join(EMUL, "libemul_grf_mix_icols.so")
    srcs = [os.path.join(EMUL, f) for f in ("emul_grf_mix_icols.cpp", "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("philox.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp", "fft_mixed.hpp",
                                            "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.emu_mix_kpitch.restype = ctypes.c_long
    for name in ("emu_grf_mix_icols_f64", "emu_grf_mix_icols_f32"):
        getattr(lib, name).argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int]
    return lib


def _plane(ny, nx, a, b, m, lo=0.5):
    y, x = np.meshgrid(np.arange(ny), np.arange(nx // 2 + 1), indexing="ij")
    return lo + ((a * y + b * x) % m) / float(m)         # no symmetry in y or x: a transposed or mirrored index cannot pass


def _blocks(ny, nx, full=False):
    """the 3 x 3 amplitude table: the four blocks the driver uses (TT, ET, EE, BB), or all nine"""
    cs = [[None] * 3 for _ in range(3)]
    cs[0][0] = _plane(ny, nx, 3, 7, 11)
    cs[1][0] = _plane(ny, nx, 5, 3, 13, lo=-0.4)
    cs[1][1] = _plane(ny, nx, 7, 5, 17)
    cs[2][2] = _plane(ny, nx, 11, 9, 19, lo=0.25)
    if full:
        k = 0
        for i in range(3):
            for j in range(3):
                if cs[i][j] is None:
                    cs[i][j] = _plane(ny, nx, 2 + k, 13 - k, 23, lo=-0.3)
                    k += 1
    return cs


def _rot(ny, nx):
    ang = 2.0 * np.pi * _plane(ny, nx, 3, 5, 29, lo=0.1)
    return np.cos(ang), np.sin(ang)


def _run(lib, ny, nx, seed, sid, ntriples, cs, rot, prec, tiles=0, plain=0, fill=0.0):
    """(3 ntriples, ny, kp) complex planes of the emulated oa_grf_mix_icols; untouched elements = fill"""
    kp = lib.emu_mix_kpitch(nx)
    rdt, cdt = (np.float64, np.complex128) if prec == "f64" else (np.float32, np.complex64)
    out = np.full((3 * ntriples, ny, kp), fill, dtype=cdt)

    def pad(a):
        p = np.zeros((ny, kp), dtype=rdt)
        p[:, :nx // 2 + 1] = a
        return p
    keep = [None if cs[i][j] is None else pad(cs[i][j]) for i in range(3) for j in range(3)]
    tab = (ctypes.c_void_p * 9)(*[None if k is None else k.ctypes.data for k in keep])
    rc, rs = (None, None) if rot is None else (pad(rot[0]), pad(rot[1]))
    fn = lib.emu_grf_mix_icols_f64 if prec == "f64" else lib.emu_grf_mix_icols_f32
    r = fn(ny, nx, seed, sid, ntriples, ctypes.cast(tab, ctypes.c_void_p), None if rc is None else rc.ctypes.data_as(ctypes.c_void_p),
           None if rs is None else rs.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ny * kp, tiles, plain)
    assert r == 0
    return out


def _reference(ny, nx, seed, sid, cs, rot, prec):
    """per component: (Ny x ifft along columns of the NumPy draw rotated E, B -> Q, U, allowed |error| per real number of each output)"""
    orot = None if rot is None else (rot[0], -rot[1])
    planes, bounds = ro.grf_mix(ny, nx, seed, sid, cs, rot=orot, with_bound=True, prec=prec)
    out = []
    for plane, bound in zip(planes, bounds):
        ref = np.fft.ifft(plane, axis=0) * ny
        tol = ny * bound.max(axis=(0, 2))
        out.append((ref, np.broadcast_to(tol[None, :], ref.shape)))
    return out


CASES = [((32, 32), "f64", 0, False), ((32, 32), "f32", 0, True), ((64, 256), "f64", 3, False), ((64, 256), "f64", 0, False)]


@pytest.mark.parametrize("shape,prec,tiles,full", CASES)
def test_emulated_mixed_draw_in_the_column_pass_is_the_numpy_statement(emu, shape, prec, tiles, full):
    ny, nx = shape
    nxh = nx // 2
    cs, rot = _blocks(ny, nx, full), _rot(ny, nx)
    seed, sid, ntriples = 0x1234567811, 2 ** 32 + 5, 2           # (a stream id above 2^32: both counter words of the stream are live)
    got = _run(emu, ny, nx, seed, sid, ntriples, cs, rot, prec, tiles=tiles, fill=-7.5)
    w = min(32 * tiles, nxh + 1) if tiles else nxh + 1            # (64, 256) with 3 tiles: the 96-column band
    for t in range(ntriples):
        for c, (ref, tol) in enumerate(_reference(ny, nx, seed, sid + 3 * t, cs, rot, prec)):
            worst = ro.draw_mismatch(got[3 * t + c, :, :w], ref[:, :w], tol[:, :w])
            print("emulated grf_mix_icols %s %s plane %d: worst |err| / bound %.3g over %d columns" % (shape, prec, 3 * t + c, worst, w))
            assert worst <= 1.0
            # a wrong counter, slot, block or edge rule is off by O(1) per mode; the bound is ~1e-5 of that
            assert np.abs(ref[:, :w]).max() > 1e3 * tol[:, :w].max() / ny
    assert np.all(got[:, :, w:] == np.asarray(-7.5, dtype=got.dtype))   # nothing is written beyond the columns run / the valid columns


def test_emulated_draw_without_rotation_is_t_e_b(emu):
    ny, nx = 32, 32
    cs = _blocks(ny, nx)
    got = _run(emu, ny, nx, 7, 3, 1, cs, None, "f64")
    for c, (ref, tol) in enumerate(_reference(ny, nx, 7, 3, cs, None, "f64")):
        assert ro.draw_mismatch(got[c, :, :nx // 2 + 1], ref, tol) <= 1.0


@pytest.mark.parametrize("shape", [(32, 32), (64, 256), (128, 64)])
def test_once_per_triple_evaluation_equals_the_per_element_statement(emu, shape):
    """col_mix_body (a lane's counters evaluated once per triple, the normals kept across the three planes, halves swapped between
    neighbouring lanes) against MixColLoad::get (three stream evaluations per element and plane) through the same pipeline on the same
    host: bit for bit, Nyquist column, column 0 and the mirrored rows included."""
    ny, nx = shape
    cs, rot = _blocks(ny, nx, full=True), _rot(ny, nx)
    for prec in ("f64", "f32"):
        a = _run(emu, ny, nx, 99, 7, 2, cs, rot, prec, plain=0)
        b = _run(emu, ny, nx, 99, 7, 2, cs, rot, prec, plain=1)
        assert np.array_equal(a, b)
        assert np.abs(a[:, :, :nx // 2 + 1]).min() > 0


def test_header_ctypes_and_docstrings_agree():
    import inspect
    from orphics_amd import _lib, mc
    from orphics_amd.engine import Engine
    hdr = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    ver = int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION >= 414
    flat = " ".join(hdr.split())
    protos = {
        "oa_grf_mix_icols": "int oa_grf_mix_icols(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ntriples, const void* const* covsqrt_hc, "
                            "const void* rot_c, const void* rot_s, void* hc_out, long zstride, void* stream);",
        "oa_mc_run_rdn0_mv_windowed":
            "int oa_mc_run_rdn0_mv_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest, "
            "const int* host_npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH, const int* host_swap, "
            "const int* host_xsrc, const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights, long mv_wstride, int nspec, "
            "const int* host_a, const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts, double norm, int leg_cols, "
            "int kappa_cols, int leg_rows, int kappa_rows, int mrow, const void* window_real, const void* rot_c, const void* rot_s, int64_t* n, "
            "double* S, double* C, void* stream);",
    }
    vp = ctypes.c_void_p
    ctype_of = {"oa_plan*": vp, "const void*": vp, "void*": vp, "int64_t*": vp, "double*": vp, "const void* const*": vp, "const int*": vp,
                "const double*": vp, "const int32_t*": vp, "const int64_t*": vp, "uint64_t": ctypes.c_uint64, "long": ctypes.c_long,
                "int": ctypes.c_int, "double": ctypes.c_double}
    for name, proto in protos.items():
        assert proto in flat, name
        args = [a.strip().rsplit(" ", 1)[0] for a in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and list(argtypes) == [ctype_of[a] for a in args], name
    # the windowed entry = the unwindowed one's arguments + (window_real, rot_c, rot_s) behind mrow
    plain = list(_lib.SIGNATURES["oa_mc_run_rdn0_mv"][1])
    assert list(_lib.SIGNATURES["oa_mc_run_rdn0_mv_windowed"][1]) == plain[:-4] + [vp] * 3 + plain[-4:]
    assert "oa_mc_run_rdn0_mv_windowed" in flat[flat.index("OA_OPT_DRAW_FUSED oa_mc_run_rdn0_windowed"):flat.index("enum { OA_OPT_MC_BATCH")]
    assert hasattr(Engine, "grf_mix_icols")
    assert list(inspect.signature(Engine.grf_mix_icols).parameters)[:6] == ["self", "seed", "covsqrt_hc", "rot", "stream_id0", "ntriples"]
    sig = inspect.signature(mc.RDN0MonteCarloPol.__init__)
    assert list(sig.parameters)[1:] == ["qest", "data", "total_power_half", "bin_edges", "estimators", "cross", "mv", "comm", "base_seed", "one_call",
                                        "qu", "iau"]
    assert list(inspect.signature(mc.RDN0MonteCarloPol.set_window).parameters) == ["self", "window"]
    assert list(inspect.signature(mc.RDN0MonteCarloPol.data_bandpowers).parameters) == ["self", "a", "b", "mean_field"]
    assert list(inspect.signature(mc.RDN0MonteCarloPol.debiased).parameters) == ["self", "a", "b", "mean_field"]
    doc = " ".join(mc.RDN0MonteCarloPol.__doc__.split())
    for piece in ("There is no window argument to the constructor", "set_window", "ALREADY apodised", "oa_mc_run_rdn0_mv_windowed",
                  "window_moments", "band-grid sides (2^a 3^b 5^c) run the host loop for now", "oa_grf_mix_icols"):
        assert piece in doc, piece
    tt = " ".join(mc.RDN0MonteCarlo.__doc__.split())
    assert "no ``window`` argument" in tt and "set_window" in tt
