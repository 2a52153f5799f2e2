"""CPU: the realisation-dependent N0 (``oa_mc_run_rdn0`` / ``mc.RDN0MonteCarlo``) without a GPU -- its definition stated in NumPy with
the oracle estimator (the six-term identity, and the band grid: the sample computed on the inner (256, 512) plane equals the sample on
the (600, 750) map's grid), the combine -> bin -> moments tail (orphics_amd/csrc/rdn0.hpp) under the thread emulator
(tests/emul/emul_rdn0.cpp) against a float64 NumPy loop that repeats its arithmetic, and the host-only surface.

Tolerances: the identities 1e-12 of the largest value (float64 FFTs of ~5e5 points); the tail's S exact or 1e-14, its C 1e-13 of the
largest entry (the reference adds the same float64 numbers in the same order; only the compiler's contraction could differ)."""
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
NT, SEG, PARTS, FOLD_Q = 64, 8, 192, 4          # rdn0.hpp: RDN0_NT, RDN0_SEG, RDN0_PARTS, RDN0_FOLD_Q


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_rdn0.so")
    srcs = [os.path.join(EMUL, f) for f in ("emul_rdn0.cpp", "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("rdn0.hpp", "mc_pol.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp",
                                            "fft_mixed.hpp", "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _band_row(i, r, m):
    return i if (r == 0 or i < r) else i - (2 * r - 1) + m


# ---- the tail under the emulator ---------------------------------------------------------------------------------------------------------
def _tail_reference(k, ids, nids, pnorm, w, rb, nxh, mcounts, n, S, C):
    """rdn0_part_body + rdn0_fold_body in Python floats: runs of equal id per thread segment, added to the bin's accumulator in column
    order; groups of rows; Q interleaved sub-sums per bin, combined as (s0 + s1) + (s2 + s3); x_i; S, C in realisation order."""
    twoB, ny, _ = k.shape
    B = twoB // 2
    nrows = 2 * rb - 1 if rb else ny
    R = (nrows + PARTS - 1) // PARTS
    G = (nrows + R - 1) // R
    kr, ki = k.real.astype(np.float64), k.imag.astype(np.float64)
    part = np.zeros((B, G, 2, nids))
    for b in range(B):
        for g in range(G):
            acc = [[0.0] * nids, [0.0] * nids]
            for r in range(g * R, min((g + 1) * R, nrows)):
                y = _band_row(r, rb, ny)
                for step in range(0, w, NT * SEG):
                    for t in range(NT):
                        cur, sa, sb = -1, 0.0, 0.0
                        for x in range(step + t * SEG, min(step + (t + 1) * SEG, w)):
                            i = int(ids[y, x])
                            m = 1 if (x == 0 or x == nxh) else (2 if x < nxh else 0)
                            if i < 0 or i >= nids or m == 0:
                                continue
                            pa = (kr[2 * b, y, x] * kr[2 * b, y, x] + ki[2 * b, y, x] * ki[2 * b, y, x]) * pnorm * float(m)
                            pb = (kr[2 * b + 1, y, x] * kr[2 * b + 1, y, x] + ki[2 * b + 1, y, x] * ki[2 * b + 1, y, x]) * pnorm * float(m)
                            if i != cur:
                                if cur >= 0:
                                    acc[0][cur] += sa
                                    acc[1][cur] += sb
                                cur, sa, sb = i, pa, pb
                            else:
                                sa += pa
                                sb += pb
                        if cur >= 0:
                            acc[0][cur] += sa
                            acc[1][cur] += sb
            part[b, g, 0], part[b, g, 1] = acc[0], acc[1]
    d = nids - 2
    xs = np.zeros((B, 2 * d))
    for b in range(B):
        tot = np.zeros((2, nids))
        for pl in range(2):
            for kbin in range(nids):
                sub = [0.0] * FOLD_Q
                for q in range(FOLD_Q):
                    for g in range(q, G, FOLD_Q):
                        sub[q] += part[b, g, pl, kbin]
                tot[pl, kbin] = (sub[0] + sub[1]) + (sub[2] + sub[3])
        for j in range(d):
            cnt = float(mcounts[j + 1])
            half = 0.5 * (tot[1, j + 1] / cnt)
            xs[b, j] = tot[0, j + 1] / cnt - half
            xs[b, d + j] = half
    for b in range(B):
        S[:2 * d] += xs[b]
        C[:(2 * d) ** 2] += np.outer(xs[b], xs[b]).ravel()
    n[0] += B
    return part, xs


def _radial_ids(ny, pitch, w, rb, edges):
    """ids of |(x, ky)| on the band (columns < w, rows |ky| < rb), -1 elsewhere: 0 below the first edge, len(edges) above the last"""
    ids = np.full((ny, pitch), -1, dtype=np.int32)
    nrows = 2 * rb - 1 if rb else ny
    for r in range(nrows):
        y = _band_row(r, rb, ny)
        ky = y if y <= ny // 2 else y - ny
        ids[y, :w] = np.digitize(np.hypot(np.arange(w), ky), edges)
    return ids


def _run_tail(emu, prec, ny, pitch, w, rb, nxh, B, edges, seed, holes=True):
    cdt = np.complex128 if prec == "f64" else np.complex64
    rng = np.random.default_rng(seed)
    k = (rng.standard_normal((2 * B, ny, pitch)) + 1j * rng.standard_normal((2 * B, ny, pitch))).astype(cdt)
    nids = len(edges) + 1
    ids = _radial_ids(ny, pitch, w, 0 if 2 * rb - 1 >= ny else rb, edges)
    band = np.argwhere(ids >= 3)                        # (not among the few underflow modes: the tests want some to remain)
    if holes:                                           # modes without a bin inside the band: skipped, they do not end a run
        for y, x in band[rng.choice(len(band), size=min(5, len(band)), replace=False)]:
            ids[y, x] = -1
    mcounts = rng.integers(1, 50, nids).astype(np.int64)
    d = nids - 2
    nrows = 2 * rb - 1 if (rb > 0 and 2 * rb - 1 < ny) else ny
    G = emu.emu_rdn0_groups(nrows)
    part = np.full(B * G * 2 * nids + 3, SENT)
    n = np.array([5, int(SENT * 2)], dtype=np.int64)
    S = np.full(2 * d + 3, SENT)
    C = np.full((2 * d) ** 2 + 3, SENT)
    S[:2 * d] = rng.standard_normal(2 * d)
    C[:(2 * d) ** 2] = rng.standard_normal((2 * d) ** 2)
    rn, rS, rC = n.copy(), S.copy(), C.copy()
    fn = emu.emu_rdn0_tail_f64 if prec == "f64" else emu.emu_rdn0_tail_f32
    pnorm = 0.37
    for rep in range(2):                                # a second call adds again
        rc = fn(_p(k), ctypes.c_long(ny * pitch), B, ny, ctypes.c_long(pitch), nxh, _p(ids), nids, ctypes.c_double(pnorm), w, rb, _p(mcounts),
                _p(part), _p(n), _p(S), _p(C))
        assert rc == 0
        rpart, xs = _tail_reference(k, ids, nids, pnorm, w, rb if (rb > 0 and 2 * rb - 1 < ny) else 0, nxh, mcounts, rn, rS, rC)
        assert np.array_equal(part[:-3].reshape(rpart.shape), rpart)
        assert n[0] == rn[0] == 5 + B * (rep + 1)
        np.testing.assert_allclose(S[:2 * d], rS[:2 * d], rtol=0, atol=1e-14 * np.abs(rS[:2 * d]).max())
        np.testing.assert_allclose(C[:-3], rC[:-3], rtol=0, atol=1e-13 * np.abs(rC[:-3]).max())
    # nothing outside 2 d / (2 d)^2 / the partial block is written
    assert n[1] == int(SENT * 2) and np.all(S[2 * d:] == SENT) and np.all(C[(2 * d) ** 2:] == SENT) and np.all(part[-3:] == SENT)
    return ids, xs


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("w,r", [(13, 7), (16, 16), (17, 1)])
def test_tail_bodies_against_a_numpy_loop(emu, w, r, B, prec):
    """2 B inner 32 x 32 kappa planes -> n, S, C.  Bins of |(x, ky)| with edges (1.5, 2.05, 2.2, 4, 6.5, 9): id 0 (underflow: the modes at
    radius <= 1) and id nids - 1 (overflow: radius > 9) occur inside every band, the bin (2.05, 2.2] holds no integer radius and stays
    empty, five modes inside the band carry id -1.  r = 16 fills 31 of the 32 rows, w = 17 reaches the inner Nyquist column 16
    (multiplicity 1), r = 1 is one row."""
    edges = np.array([1.5, 2.05, 2.2, 4.0, 6.5, 9.0])
    ids, xs = _run_tail(emu, prec, 32, 32, w, r, 16, B, edges, seed=1000 * w + 10 * r + B)
    got = set(np.unique(ids[ids >= 0]))
    assert 0 in got and 2 not in got and (len(edges) in got or r == 1 and w <= 9)
    d = len(edges) - 1
    assert np.all(xs[:, 1] == 0) and np.all(xs[:, d + 1] == 0)                     # the empty bin: sum 0 over its (whole-plane) count
    assert np.all(xs[:, d:] >= 0)


@pytest.mark.parametrize("case", ["rows", "cols"])
def test_tail_bodies_beyond_one_row_group_and_one_tile_step(emu, case):
    """What 32 x 32 planes do not reach: a band of 401 rows is cut into groups of 3 rows (134 partial vectors, the last of 2 rows: more
    than the 192-group limit would give with one row each), and a band of 530 columns takes two tile steps of 512."""
    if case == "rows":
        assert emu.emu_rdn0_rows_per_group(401) == 3 and emu.emu_rdn0_groups(401) == 134
        _run_tail(emu, "f64", 401, 12, 9, 0, 6, 2, np.array([1.5, 30.0, 90.0, 150.0]), seed=7)
    else:
        _run_tail(emu, "f32", 5, 536, 530, 2, 520, 1, np.array([1.5, 100.0, 300.0, 515.0, 525.0]), seed=8)


# ---- the definition in NumPy ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_600x750():
    from oracle import maps_oracle as mo
    from oracle.qe_oracle import QEOracleTT
    from orphics_amd import cosmology
    shape, res = (600, 750), 1.0 * np.pi / 180 / 60
    ly, lx = mo.laxes(shape, res, res)
    modl = np.hypot(ly[:, None], lx[None, :])
    th = cosmology.default_theory()
    cl = th.lCl("TT", modl)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    beam = np.exp(-0.5 * (modl * 1.5 * np.pi / 180 / 60 / np.sqrt(8 * np.log(2))) ** 2)
    tmask = ((modl > 300) & (modl < 2000)).astype(np.float64)
    kmask = ((modl > 20) & (modl < 3500)).astype(np.float64)
    qo = QEOracleTT(shape, res, res, cl, cl, noise, beam, tmask, kmask_K=kmask)
    rng = np.random.default_rng(3)
    amp = np.sqrt(cl * beam ** 2 + noise)
    d, s, sp = (np.fft.fft2(rng.standard_normal(shape)) * amp for _ in range(3))
    return dict(shape=shape, res=res, ly=ly, lx=lx, modl=modl, qo=qo, d=d, s=s, sp=sp)


def test_six_term_identity(oracle_600x750):
    """|QE(d, s) + QE(s, d)|^2 is the sum of the four data-simulation terms C[ds, ds] + C[sd, sd] + C[ds, sd] + C[sd, ds] of the six-term
    RDN0, C[a, b] = Re(a conj b), per mode."""
    o = oracle_600x750
    qo, d, s = o["qo"], o["d"], o["s"]
    ds, sd = qo.kappa_ft(d, s), qo.kappa_ft(s, d)
    lhs = np.abs(ds + sd) ** 2
    c = lambda a, b: (a * np.conj(b)).real
    rhs = c(ds, ds) + c(sd, sd) + c(ds, sd) + c(sd, ds)
    assert lhs.max() > 0
    assert np.abs(lhs - rhs).max() <= 1e-12 * lhs.max()


def _embed(a, My, Mx, r, w):
    """the modes |ky index| < r, |kx index| < w of a full (ny, nx) plane at the same signed indices of a zero (My, Mx) plane"""
    out = np.zeros((My, Mx), dtype=a.dtype)
    ky = np.arange(-(r - 1), r)
    kx = np.arange(-(w - 1), w)
    out[np.ix_(ky % My, kx % Mx)] = a[np.ix_(ky % a.shape[0], kx % a.shape[1])]
    return out


def test_sample_on_the_inner_plane_equals_the_sample_on_the_maps_grid(oracle_600x750):
    """x_i = [p(A) - p(B) / 2, p(B) / 2] from the three sources' leg bands embedded in the (256, 512) plane of the band grid -- filters
    at the same modes, Fnorm times My Mx / (ny nx), the map grid's bin ids and mode counts -- equals x_i on the (600, 750) grid."""
    from oracle.qe_oracle import QEOracleTT
    o = oracle_600x750
    qo, (ny, nx) = o["qo"], o["shape"]

    def band(plane):
        yy, xx = np.nonzero(plane)
        return int(np.minimum(yy, ny - yy).max()) + 1, int(np.minimum(xx, nx - xx).max()) + 1
    rl, wl = band((qo.Wg != 0) | (qo.Wh != 0))
    rk, wk = band(qo.Fnorm != 0)
    My, Mx = 256, 512
    assert My >= max(2 * rl + rk, 2 * rk) and Mx >= max(2 * wl + wk, 2 * wk) and My // 2 < max(2 * rl + rk, 2 * rk)
    edges = np.linspace(20, 3500, 12)
    ids = np.digitize(o["modl"], edges)
    nids = edges.size + 1
    counts = np.bincount(ids.ravel(), minlength=nids).astype(np.float64)
    norm = 1.0

    def sample(A, B, idmap):
        pa = np.bincount(idmap.ravel(), weights=(np.abs(A) ** 2).ravel() * norm, minlength=nids + 1)[1:nids - 1] / counts[1:-1]
        pb = np.bincount(idmap.ravel(), weights=(np.abs(B) ** 2).ravel() * norm, minlength=nids + 1)[1:nids - 1] / counts[1:-1]
        return np.concatenate((pa - pb / 2, pb / 2))
    d, s, sp = o["d"], o["s"], o["sp"]
    x_map = sample(qo.kappa_ft(d, s) + qo.kappa_ft(s, d), qo.kappa_ft(s, sp) + qo.kappa_ft(sp, s), ids)
    qi = QEOracleTT.for_timing((My, Mx), o["res"] * ny / My, o["res"] * nx / Mx, _embed(qo.Wg, My, Mx, rl, wl), _embed(qo.Wh, My, Mx, rl, wl),
                               _embed(qo.Fnorm, My, Mx, rk, wk) * (My * Mx / float(ny * nx)))
    di, si, spi = (_embed(a, My, Mx, rl, wl) for a in (d, s, sp))
    ids_i = _embed(ids + 1, My, Mx, rk, wk) - 1                      # -1 outside kappa's band
    ids_i = np.where(ids_i < 0, nids, ids_i)                         # (np.bincount wants non-negative ids: one extra, unused bin)
    x_in = sample(qi.kappa_ft(di, si) + qi.kappa_ft(si, di), qi.kappa_ft(si, spi) + qi.kappa_ft(spi, si), ids_i)
    assert np.all(x_map[edges.size - 1:] > 0)
    assert np.abs(x_in - x_map).max() <= 1e-12 * np.abs(x_map).max()


# ---- host surface --------------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_docstring():
    from orphics_amd import _lib, lensing, mc
    hdr = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    ver = int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION >= 411
    for name in ("oa_rdn0_set_data", "oa_mc_run_rdn0"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr)
    doc = " ".join(mc.RDN0MonteCarlo.__doc__.split())
    for piece in ("A = QE(d, s) + QE(s, d)", "B = QE(s, s') + QE(s', s)", "x_i = [ p(A) - p(B) / 2 , p(B) / 2 ]", "stream ``2 i``", "``2 i + 1``",
                  "smaller variance", "no ``window`` argument", "one_call=False"):
        assert piece in doc, piece
    assert hasattr(mc.RDN0MonteCarlo, "debiased") and "QE(A, B) + QE(B, A)" in lensing.Estimator.reconstruct_tt_sym_hc.__doc__
