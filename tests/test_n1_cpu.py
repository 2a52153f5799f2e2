"""CPU: the analytic N1 bias sums of the TT estimator (``oa_n1_tt`` / ``Estimator.n1_sums``) without a GPU -- the NumPy statement of
S(L) (this module; tests/test_n1_gpu.py imports it), its own properties, the kernel bodies of orphics_amd/csrc/n1.hpp under the thread
emulator (tests/emul/emul_n1.cpp) against it, and the host-only surface.

The statement follows include/orphics_amd.h term by term (two bracket terms, the four f written out); the kernel evaluates the
algebraically equal fused form  sum G(l1) H(q) Cpp(l1 - q) f f  with H(q) = G(q) + G(L - q) in another order.

Tolerance: |S - S_ref| <= 1e-12 sum|term| -- a float64 rounding bound for a reordered sum of <= 3e6 terms of ~20 operations each
(eps = 1.1e-16; sqrt(n) growth gives ~2e-13 of the largest partial sums, n eps an absolute worst case of 3e-10 never approached),
relative to the ABSOLUTE sum because S changes sign."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL = os.path.join(HERE, "emul")
TOL = 1e-12


# ---- the NumPy statement -------------------------------------------------------------------------------------------------------------------
def n1_statement(ly, lx, wg, wh, cr, cpp, leg_rows, leg_cols, Lyi, Lxi, terms=False):
    """S(L) at the full-plane mode (Lyi, Lxi), broadcast over (l1, l1') pairs of the box |ky| < leg_rows, |kx| < leg_cols.  All planes
    are full (Ny, Nx) float64 arrays read at MODULAR indices; l vectors come from the axes.  Returns (S, sum|term|), or with
    ``terms`` (S1, S2, A1, A2): the two bracket terms and their absolute sums."""
    Ny, Nx = wg.shape
    ky, kx = (a.ravel() for a in np.meshgrid(np.arange(-(leg_rows - 1), leg_rows), np.arange(-(leg_cols - 1), leg_cols), indexing="ij"))
    kLy = Lyi - Ny if Lyi > Ny // 2 else Lyi
    kLx = Lxi - Nx if Lxi > Nx // 2 else Lxi
    k2y, k2x = kLy - ky, kLx - kx
    Ly, Lx = ly[Lyi], lx[Lxi]
    l1y, l1x, l2y, l2x = ly[ky % Ny], lx[kx % Nx], ly[k2y % Ny], lx[k2x % Nx]
    C1, C2 = cr[ky % Ny, kx % Nx], cr[k2y % Ny, k2x % Nx]
    g = (Ly * l1y + Lx * l1x) * wg[ky % Ny, kx % Nx] * wh[k2y % Ny, k2x % Nx]
    i, j = np.s_[:, None], np.s_[None, :]                        # l1 along rows, l1' along columns

    def f(Ca, ay, ax, Cb, by, bx):                               # f(a, -b) = C_a (m.a) - C_b (m.b),  m = a - b
        my, mx = ay - by, ax - bx
        return Ca * (my * ay + mx * ax) - Cb * (my * by + mx * bx)
    cpp1 = cpp[(ky[i] - ky[j]) % Ny, (kx[i] - kx[j]) % Nx]
    cpp2 = cpp[(ky[i] - k2y[j]) % Ny, (kx[i] - k2x[j]) % Nx]
    # f(l2, -l2') = -C(l2) (m.l2) + C(l2') (m.l2') with m = l1 - l1' = -(l2 - l2'): f(l2, -l2') in the same helper
    t1 = g[i] * g[j] * cpp1 * f(C1[i], l1y[i], l1x[i], C1[j], l1y[j], l1x[j]) * f(C2[i], l2y[i], l2x[i], C2[j], l2y[j], l2x[j])
    t2 = g[i] * g[j] * cpp2 * f(C1[i], l1y[i], l1x[i], C2[j], l2y[j], l2x[j]) * f(C2[i], l2y[i], l2x[i], C1[j], l1y[j], l1x[j])
    if terms:
        return t1.sum(), t2.sum(), np.abs(t1).sum(), np.abs(t2).sum()
    return t1.sum() + t2.sum(), np.abs(t1).sum() + np.abs(t2).sum()


def n1_scalar_terms(ly, lx, wg, wh, cr, cpp, Lyi, Lxi):
    """The two bracket terms by scalar loops over ALL modes of the full plane in modular index arithmetic: f(a, b) = C_a (m.a) +
    C_b (m.b), m = a + b, exactly as the definition reads."""
    Ny, Nx = wg.shape
    vec = lambda y, x: np.array([ly[y % Ny], lx[x % Nx]])
    Lv = vec(Lyi, Lxi)

    def f(Ca, a, Cb, b):
        m = a + b
        return Ca * (m @ a) + Cb * (m @ b)
    modes = [(y, x) for y in range(Ny) for x in range(Nx)]
    gs = []
    for (y, x) in modes:
        gs.append((Lv @ vec(y, x)) * wg[y, x] * wh[(Lyi - y) % Ny, (Lxi - x) % Nx])
    s1 = s2 = 0.0
    for a, (y1, x1) in enumerate(modes):
        if gs[a] == 0:
            continue
        y2, x2 = (Lyi - y1) % Ny, (Lxi - x1) % Nx
        l1, l2 = vec(y1, x1), vec(y2, x2)
        for b, (y1p, x1p) in enumerate(modes):
            if gs[b] == 0:
                continue
            y2p, x2p = (Lyi - y1p) % Ny, (Lxi - x1p) % Nx
            l1p, l2p = vec(y1p, x1p), vec(y2p, x2p)
            w = gs[a] * gs[b]
            s1 += w * cpp[(y1 - y1p) % Ny, (x1 - x1p) % Nx] * f(cr[y1, x1], l1, cr[y1p, x1p], -l1p) * f(cr[y2, x2], l2, cr[y2p, x2p], -l2p)
            s2 += w * cpp[(y1 - y2p) % Ny, (x1 - x2p) % Nx] * f(cr[y1, x1], l1, cr[y2p, x2p], -l2p) * f(cr[y2, x2], l2, cr[y1p, x1p], -l1p)
    return s1, s2


def make_case(Ny, Nx, by, bx, seed, res_arcmin=2.0, car=False):
    """Axes of an (Ny, Nx) map and four even (a(-k) = a(k)) random full planes: wg, wh non-zero exactly on |ky| <= by, |kx| <= bx without
    the origin, cr and cpp positive everywhere (cpp 0 at the origin).  ``car``: the x axis decreases (lx[1] < 0), as FlatGeometry.from_res has it."""
    rng = np.random.default_rng(seed)
    res = res_arcmin * np.pi / 180 / 60
    ly, lx = 2 * np.pi * np.fft.fftfreq(Ny, res), 2 * np.pi * np.fft.fftfreq(Nx, -res if car else res)
    iy, ix = np.arange(Ny), np.arange(Nx)

    def even(a):
        return 0.5 * (a + a[np.ix_((-iy) % Ny, (-ix) % Nx)])
    fy, fx = np.minimum(iy, Ny - iy), np.minimum(ix, Nx - ix)
    band = ((fy[:, None] <= by) & (fx[None, :] <= bx)).astype(np.float64)
    band[0, 0] = 0.0
    wg = even(rng.uniform(0.5, 1.5, (Ny, Nx))) * band
    wh = even(rng.uniform(0.5, 1.5, (Ny, Nx))) * band
    cr = even(rng.uniform(0.5, 1.5, (Ny, Nx)))
    cpp = even(rng.uniform(0.5, 1.5, (Ny, Nx)))
    cpp[0, 0] = 0.0
    return dict(Ny=Ny, Nx=Nx, ly=ly, lx=lx, wg=wg, wh=wh, cr=cr, cpp=cpp, rows=by + 1, cols=bx + 1)


def reference(case, modes):
    out = [n1_statement(case["ly"], case["lx"], case["wg"], case["wh"], case["cr"], case["cpp"], case["rows"], case["cols"], y, x) for (y, x) in modes]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def hc_plane(a, kp, fill=np.nan):
    """full (Ny, Nx) plane -> (Ny, kp) hc-layout plane; the padding columns beyond Nx / 2 hold ``fill``"""
    Ny, Nx = a.shape
    out = np.full((Ny, kp), fill)
    out[:, :Nx // 2 + 1] = a[:, :Nx // 2 + 1]
    return out


# ---- the bodies under the emulator ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_n1.so")
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    deps = [os.path.join(EMUL, f) for f in ("emul_n1.cpp", "emul_fft.cpp")] + [os.path.join(csrc, h) for h in ("n1.hpp", "cx.hpp", "fft_kernels.hpp", "fft_plan.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, deps[0]])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_emu(emu, case, modes, tiles_per_launch=0):
    kp = case["Nx"] // 2 + 1 + 3
    planes = [hc_plane(case[k], kp) for k in ("wg", "wh", "cr", "cpp")]
    Ly = np.ascontiguousarray([m[0] for m in modes], dtype=np.int32)
    Lx = np.ascontiguousarray([m[1] for m in modes], dtype=np.int32)
    S = np.full(len(modes) + 1, -7.5)
    rc = emu.emu_n1_tt(*[_p(a) for a in planes], _p(case["ly"]), _p(case["lx"]), case["Ny"], case["Nx"], ctypes.c_long(kp), case["cols"], case["rows"],
                       len(modes), _p(Ly), _p(Lx), tiles_per_launch, _p(S))
    assert rc == 0 and S[-1] == -7.5
    return S[:-1]


# L on both axes, in all four quadrants (row index > Ny / 2, column index > Nx / 2), at 0, and one beyond twice the band (empty box)
MODES_32 = [(0, 0), (3, 0), (0, 4), (2, 3), (30, 5), (4, 29), (28, 27), (7, 8), (16, 16), (11, 0)]
MODES_48 = [(0, 0), (5, 0), (0, 37), (3, 4), (44, 2), (6, 35), (40, 33), (13, 11), (15, 0)]


@pytest.mark.parametrize("shape,band,modes", [((32, 32), (5, 5), MODES_32), ((48, 40), (7, 6), MODES_48)])
def test_bodies_against_the_statement(emu, shape, band, modes):
    case = make_case(*shape, *band, seed=shape[0], car=shape[0] == 48)
    S = run_emu(emu, case, modes)
    ref, scale = reference(case, modes)
    assert scale.max() > 0 and np.abs(ref).max() > 1e-3 * scale.max()          # the sums are not all cancellation
    assert S[0] == 0.0 and ref[0] == 0.0                                        # L = 0: g = 0
    assert S[-1] == 0.0 and scale[-1] == 0.0                                    # |L| beyond twice the band: no mode pair
    assert np.all(np.abs(S - ref) <= TOL * scale), (np.abs(S - ref) / np.maximum(scale, 1e-300)).max()
    # the same bits for a list cut in two, for one L at a time, and with the pair launches cut per tile
    again = np.concatenate([run_emu(emu, case, modes[1:2]), run_emu(emu, case, modes[2:4])])
    assert np.array_equal(S[1:4], again)
    assert np.array_equal(S[4:6], run_emu(emu, case, modes[4:6], tiles_per_launch=2))


def test_bodies_on_a_wide_box(emu):
    """32 x 4096 with band |ky| <= 1, |kx| <= 300: a box row of 601 modes is two l1 tiles (> 512 modes, 301 + 300: threads with two modes
    and with one) and five q chunks (> 128 modes) -- the paths no square box of a testable size reaches.  (0, 37): three box rows;
    (2, 250): one row of 351 modes."""
    case = make_case(32, 4096, 1, 300, seed=4096, car=True)
    modes = [(0, 37), (2, 250)]
    S = run_emu(emu, case, modes)
    ref, scale = reference(case, modes)
    assert np.all(scale > 0) and np.all(np.abs(S - ref) <= TOL * scale), np.abs(S - ref) / scale
    assert np.array_equal(S[1:], run_emu(emu, case, modes[1:], tiles_per_launch=1))


def test_box_of_L_and_parts(emu):
    """the box of L is the set of modes q with q and L - q inside the band; its cut into parts depends on the box alone"""
    out = (ctypes.c_int * 4)()
    assert emu.emu_n1_box(0, 0, 6, 6, out) >= 1 and list(out) == [-5, -5, 11, 11]
    assert emu.emu_n1_box(3, -4, 6, 6, out) >= 1 and list(out) == [-2, -5, 8, 7]
    assert emu.emu_n1_box(10, 0, 6, 6, out) >= 1 and list(out) == [5, -5, 1, 11]
    assert emu.emu_n1_box(11, 0, 6, 6, out) == 0
    # 1522 tiles of 381 modes, 6e10 pair terms per launch: 271 tiles per launch, cut into 8 parts for 2048 workgroups
    assert emu.emu_n1_box(0, 0, 381, 381, out) == 8 and list(out)[2:] == [761, 761]


# ---- properties of the statement -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case32():
    return make_case(32, 32, 5, 5, seed=32)


def _S(case, y, x, cpp=None):
    return n1_statement(case["ly"], case["lx"], case["wg"], case["wh"], case["cr"], case["cpp"] if cpp is None else cpp, case["rows"], case["cols"], y, x)


def test_statement_is_even_in_L(case32):
    for (y, x) in [(2, 3), (30, 5), (0, 4), (7, 8)]:
        a, sa = _S(case32, y, x)
        b, _ = _S(case32, (-y) % 32, (-x) % 32)
        assert abs(a - b) <= TOL * sa and sa > 0


def test_statement_is_linear_in_cpp_and_zero_without_it(case32):
    rng = np.random.default_rng(5)
    other = make_case(32, 32, 5, 5, seed=77)["cpp"]
    a, sa = _S(case32, 2, 3)
    b, sb = _S(case32, 2, 3, cpp=other)
    c, _ = _S(case32, 2, 3, cpp=2.0 * case32["cpp"] - 0.5 * other)
    assert abs(c - (2.0 * a - 0.5 * b)) <= TOL * (2.0 * sa + 0.5 * sb)
    assert _S(case32, 2, 3, cpp=np.zeros((32, 32))) == (0.0, 0.0)
    assert rng is not None


def test_each_bracket_term_against_scalar_loops():
    case = make_case(12, 12, 2, 2, seed=12)
    for (y, x) in [(1, 2), (11, 3), (0, 2)]:
        s1, s2, a1, a2 = n1_statement(case["ly"], case["lx"], case["wg"], case["wh"], case["cr"], case["cpp"], 3, 3, y, x, terms=True)
        r1, r2 = n1_scalar_terms(case["ly"], case["lx"], case["wg"], case["wh"], case["cr"], case["cpp"], y, x)
        assert a1 > 0 and a2 > 0
        assert abs(s1 - r1) <= TOL * a1 and abs(s2 - r2) <= TOL * a2


# ---- host surface --------------------------------------------------------------------------------------------------------------------------
def test_symbol_in_header_and_ctypes_table():
    from orphics_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    ver = int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION >= 416
    assert "oa_n1_tt" in _lib.SIGNATURES and re.search(r"\boa_n1_tt\s*\(", hdr)
    assert len(_lib.SIGNATURES["oa_n1_tt"][1]) == 12


def test_argument_checks_and_aliasing_refusal():
    from orphics_amd.engine import n1_check
    Ly, Lx = n1_check(64, 48, 10, 8, [0, 63], [47, 1])
    assert Ly.dtype == Lx.dtype == np.int32 and list(Ly) == [0, 63] and list(Lx) == [47, 1]
    n1_check(64, 48, 16, 12, [1], [1])                               # 4 * 15 = 60 < 64, 4 * 11 = 44 < 48: the widest band allowed
    for rows, cols in [(17, 12), (16, 13), (0, 5), (5, 0)]:         # one more row / column aliases; 0 = 'not band-limited'
        with pytest.raises(ValueError, match="un-aliased"):
            n1_check(64, 48, rows, cols, [1], [1])
    for Ly, Lx in [([], []), ([1, 2], [1]), ([[1]], [[1]])]:
        with pytest.raises(ValueError, match="one length"):
            n1_check(64, 48, 5, 5, Ly, Lx)
    for Ly, Lx in [([64], [0]), ([0], [48]), ([-1], [0])]:
        with pytest.raises(ValueError, match="outside"):
            n1_check(64, 48, 5, 5, Ly, Lx)
    with pytest.raises(TypeError, match="INDICES"):
        n1_check(64, 48, 5, 5, [1.5], [2.0])


def test_getN1_mode_selection():
    from orphics_amd.lensing import NlGenerator, n1_bin_modes
    res = 2.0 * np.pi / 180 / 60
    ly, lx = 2 * np.pi * np.fft.fftfreq(256, res), 2 * np.pi * np.fft.fftfreq(320, -res)      # CAR: x decreases, lx[1] < 0
    cents = np.linspace(100, 3000, 7)
    m = n1_bin_modes(ly, lx, cents, per_bin=4)
    assert np.array_equal(m, n1_bin_modes(ly, -lx, cents, per_bin=4))                           # a quadrant of indices
    assert m.shape == (7, 4, 2) and np.array_equal(m, n1_bin_modes(ly, lx, cents, per_bin=4))
    assert m.min() >= 0 and m[..., 0].max() <= 128 and m[..., 1].max() <= 160         # first quadrant
    L = np.hypot(ly[m[..., 0]], lx[m[..., 1]])
    assert np.all(np.abs(L - cents[:, None]) <= 0.75 * np.hypot(ly[1], lx[1]))         # nearest grid mode: within half a cell diagonal (+ slack)
    ang = np.arctan2(np.abs(ly[m[..., 0]]), np.abs(lx[m[..., 1]]))
    want = (np.arange(4) + 0.5) * np.pi / 8
    assert np.all(np.abs(ang[2:] - want[None, :]) < 0.1)
    assert np.all(np.diff(m[3, :, 0]) > 0) and np.all(np.diff(m[3, :, 1]) < 0)
    with pytest.raises(ValueError):
        n1_bin_modes(ly, lx, cents, per_bin=0)
    doc = " ".join(NlGenerator.getN1.__doc__.split())
    assert "SAMPLED annulus, not a full-annulus average" in doc
    g = NlGenerator.__new__(NlGenerator)
    with pytest.raises(NotImplementedError, match="follow-up"):
        g.getN1("EB")
