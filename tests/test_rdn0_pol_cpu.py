"""CPU: the realisation-dependent N0 of an estimator set (``oa_mc_run_rdn0_mv`` / ``mc.RDN0MonteCarloPol``) without a GPU -- the combine ->
bin -> moments tail (orphics_amd/csrc/rdn0_mv.hpp) under the thread emulator (tests/emul/emul_rdn0_mv.cpp) against a float64 NumPy loop
that repeats its arithmetic, its definition stated in NumPy with the oracle estimators on ``rng_oracle``'s statement of the ``grf_mix``
draws, and the host-only surface.

Tolerances: the tail's partial tables and x_i exact, its S exact or 1e-14, its C 1e-13 of the largest entry (the reference adds the same
float64 numbers in the same order; only the compiler's contraction could differ: tests/test_rdn0_cpu.py's bounds); the identities 1e-12
of the largest value (float64 FFTs of 8192 points)."""
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
NT, PARTS, FOLD_Q, FMAX = 64, 512, 4, 6         # rdn0_mv.hpp: RDN0MV_NT, RDN0MV_PARTS, RDN0MV_FOLD_Q; mc_pol.hpp: STACK_MULTI_MAX


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMUL, "libemul_rdn0_mv.so")
    srcs = [os.path.join(EMUL, f) for f in ("emul_rdn0_mv.cpp", "emul_fft.cpp")]
    csrc = os.path.join(ROOT, "orphics_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("rdn0_mv.hpp", "mc_pol.hpp", "fft_kernels.hpp", "fft_plan.hpp", "fft_r2c_w64.hpp", "fft_r2c_rs4096.hpp",
                                            "fft_mixed.hpp", "cx.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", so, srcs[0]])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _band_row(i, r, m):
    return i if (r == 0 or i < r) else i - (2 * r - 1) + m


def _spectra(nest, cross=True, mv=True):
    from orphics_amd import mc
    return mc.pol_spectrum_list(["E%d" % i for i in range(nest)], cross, mv)[1]


# ---- the tail under the emulator ---------------------------------------------------------------------------------------------------------
def _tail_reference(k, wt, pairs, ids, nids, pnorm, w, rb, nxh, mcounts, n, S, C):
    """rdn0mv_part_body + rdn0mv_fold_body + rdn0mv_moments_body in float64 NumPy.  Per mode the field values (MV: sum_e w_e Z_e added in
    estimator order from 0) and the products (ar br + ai bi) * (pnorm * m) are elementwise, so they are formed for the whole plane at once;
    the ORDER of the additions is what the loops repeat: a table entry (set, spectrum, bin) of a row group receives its modes in (row,
    column) order; the groups are folded as Q interleaved sub-sums combined as (s0 + s1) + (s2 + s3); then x_i, S, C."""
    nf2, ny, _ = k.shape
    nest = nf2 // 2
    nspec = len(pairs)
    nrows = 2 * rb - 1 if rb else ny
    R = (nrows + PARTS - 1) // PARTS
    G = (nrows + R - 1) // R
    kr, ki = k.real.astype(np.float64), k.imag.astype(np.float64)
    zr = np.zeros((2, nest + 1) + kr.shape[1:])
    zi = np.zeros_like(zr)
    for s_ in range(2):
        zr[s_, :nest], zi[s_, :nest] = kr[s_ * nest:(s_ + 1) * nest], ki[s_ * nest:(s_ + 1) * nest]
        if wt is not None:
            for e in range(nest):
                ww = wt[e].astype(np.float64)
                zr[s_, nest] = zr[s_, nest] + ww * zr[s_, e]
                zi[s_, nest] = zi[s_, nest] + ww * zi[s_, e]
    cols = np.arange(kr.shape[2])
    fac = pnorm * np.where((cols == 0) | (cols == nxh), 1.0, 2.0)
    prod = np.zeros((2, nspec) + kr.shape[1:])
    for s_ in range(2):
        for j, (a, b) in enumerate(pairs):
            prod[s_, j] = (zr[s_, a] * zr[s_, b] + zi[s_, a] * zi[s_, b]) * fac[None, :]
    part = np.zeros((G, 2, nspec, nids))
    for g in range(G):
        for r in range(g * R, min((g + 1) * R, nrows)):
            y = _band_row(r, rb, ny)
            for x in range(min(w, nxh + 1)):
                i = int(ids[y, x])
                if 0 <= i < nids:
                    part[g, :, :, i] += prod[:, :, y, x]
    sub = np.zeros((FOLD_Q, 2, nspec, nids))
    for q in range(FOLD_Q):
        for g in range(q, G, FOLD_Q):
            sub[q] += part[g]
    tot = (sub[0] + sub[1]) + (sub[2] + sub[3])
    cnt = mcounts[1:-1].astype(np.float64)
    half = 0.5 * (tot[1][:, 1:-1] / cnt)
    x = np.concatenate(((tot[0][:, 1:-1] / cnt - half).ravel(), half.ravel()))
    D = x.size
    S[:D] += x
    if C is not None:
        C[:D * D] += np.outer(x, x).ravel()
    n[0] += 1
    return part, x


def _radial_ids(ny, pitch, w, rb, edges):
    """ids of |(x, ky)| on the band (columns < w, rows |ky| < rb), -1 elsewhere: 0 below the first edge, len(edges) above the last"""
    ids = np.full((ny, pitch), -1, dtype=np.int32)
    nrows = 2 * rb - 1 if rb else ny
    for r in range(nrows):
        y = _band_row(r, rb, ny)
        ky = y if y <= ny // 2 else y - ny
        ids[y, :w] = np.digitize(np.hypot(np.arange(w), ky), edges)
    return ids


def _run_tail(emu, prec, nest, pairs, weights, ny, pitch, w, rb, nxh, edges, seed, holes=True, moments=True, reps=2):
    cdt, rdt = (np.complex128, np.float64) if prec == "f64" else (np.complex64, np.float32)
    rng = np.random.default_rng(seed)
    k = (rng.standard_normal((2 * nest, ny, pitch)) + 1j * rng.standard_normal((2 * nest, ny, pitch))).astype(cdt)
    wt = rng.uniform(0.1, 1.0, (nest, ny, pitch)).astype(rdt) if weights else None
    nids, nspec = len(edges) + 1, len(pairs)
    rbe = rb if (rb > 0 and 2 * rb - 1 < ny) else 0
    ids = _radial_ids(ny, pitch, w, rbe, edges)
    band = np.argwhere(ids >= 3)
    if holes:                                           # inside the band: modes without a bin (-1) and with an id beyond the table (nids + 3)
        pick = band[rng.choice(len(band), size=min(8, len(band)), replace=False)]
        for j, (y, x) in enumerate(pick):
            ids[y, x] = -1 if j % 2 else nids + 3
    mcounts = rng.integers(1, 50, nids).astype(np.int64)
    d = nids - 2
    D = 2 * nspec * d
    nrows = 2 * rbe - 1 if rbe else ny
    G = emu.emu_rdn0mv_groups(nrows)
    part = np.full(G * 2 * nspec * nids + 3, SENT)
    x = np.full(D + 3, SENT)
    n = np.array([5, int(SENT * 2)], dtype=np.int64)
    S = np.full(D + 3, SENT)
    C = np.full((D * D if moments else 0) + 3, SENT)
    S[:D] = rng.standard_normal(D)
    C[:len(C) - 3] = rng.standard_normal(len(C) - 3)
    rn, rS, rC = n.copy(), S.copy(), C.copy()
    fn = emu.emu_rdn0mv_tail_f64 if prec == "f64" else emu.emu_rdn0mv_tail_f32
    ha = (ctypes.c_int * nspec)(*[p[0] for p in pairs])
    hb = (ctypes.c_int * nspec)(*[p[1] for p in pairs])
    pnorm = 0.37
    for rep in range(reps):                             # a second call adds again
        rc = fn(_p(k), ctypes.c_long(ny * pitch), _p(wt), ctypes.c_long(ny * pitch), nest, nspec, ha, hb, ny, ctypes.c_long(pitch), nxh, _p(ids), nids,
                ctypes.c_double(pnorm), w, rb, _p(mcounts), _p(part), _p(x), _p(n), _p(S), _p(C), 3 if moments else 0)
        assert rc == 0
        if not moments:                                 # (no moment launch: S, C, n untouched; the reference's S, n are scratch)
            rpart, rx = _tail_reference(k, wt, pairs, ids, nids, pnorm, w, rbe, nxh, mcounts, rn.copy(), rS.copy(), None)
        else:
            rpart, rx = _tail_reference(k, wt, pairs, ids, nids, pnorm, w, rbe, nxh, mcounts, rn, rS, rC)
        assert np.array_equal(part[:-3].reshape(rpart.shape), rpart)
        assert np.array_equal(x[:D], rx)
        if moments:
            assert n[0] == rn[0] == 5 + rep + 1
            np.testing.assert_allclose(S[:D], rS[:D], rtol=0, atol=1e-14 * np.abs(rS[:D]).max())
            np.testing.assert_allclose(C[:-3], rC[:-3], rtol=0, atol=1e-13 * np.abs(rC[:-3]).max())
    # nothing outside D / D^2 / the partial block / x is written
    assert n[1] == int(SENT * 2) and np.all(S[D:] == SENT) and np.all(C[len(C) - 3:] == SENT) and np.all(part[-3:] == SENT) and np.all(x[D:] == SENT)
    if not moments:
        assert n[0] == 5 and np.array_equal(S, rS) and np.array_equal(C, rC)
    return ids, x[:D].copy()


EDGES6 = np.array([1.5, 2.05, 2.2, 4.0, 6.5, 9.0])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("w,r", [(13, 7), (16, 16), (17, 1), (17, 0)])
def test_tail_bodies_against_a_numpy_loop(emu, w, r, prec):
    """2 nest inner 32 x 32 kappa planes -> n, S, C, for nest = 1 without weights (one auto) and nest = 5 with weights and the 16 spectra
    of pol_spectrum_list (autos, crosses, MV auto).  Bins of |(x, ky)| with edges (1.5, 2.05, 2.2, 4, 6.5, 9): id 0 and id nids - 1 occur
    inside every band, the bin (2.05, 2.2] stays empty, eight modes inside the band carry an id outside [0, nids) (-1 and nids + 3).
    w = 13 ends at an odd column, w = 17 includes the Nyquist column 16 (multiplicity 1), r = 16 fills 31 of the 32 rows, r = 1 is one
    row, r = 0 every row."""
    _run_tail(emu, prec, 1, [(0, 0)], False, 32, 32, w, r, 16, EDGES6, seed=1000 * w + 10 * r + 1)
    pairs = _spectra(5)
    assert len(pairs) == 16 and pairs[-1] == (5, 5)
    ids, xs = _run_tail(emu, prec, 5, pairs, True, 32, 32, w, r, 16, EDGES6, seed=1000 * w + 10 * r + 5)
    got = set(np.unique(ids[(ids >= 0) & (ids < len(EDGES6) + 1)]))
    assert 0 in got and 2 not in got
    d = len(EDGES6) - 1
    x = xs.reshape(2, 16, d)
    assert np.all(x[:, :, 1] == 0)                                                 # the empty bin: sum 0 over its (whole-plane) count
    autos = [0, 1, 2, 3, 4, 15]
    assert np.all(x[1, autos] >= 0)                                                # p(B_a, B_a) / 2


def test_tail_at_the_table_limits(emu):
    """nest = 6 with the 22 spectra of its list and six more crosses with the MV field: nspec = 28, the spectrum table's limit, with 21 bin
    ids (D = 1064).  nids = 1024, the id limit, with one spectrum (D = 2044).  nspec * nids = 4088 of the 4096 the partial table holds
    (28 x 146): partial sums and x_i only -- its C would be 8064^2 doubles.  Just beyond each limit the launcher's checks refuse."""
    pairs = _spectra(6)
    assert len(pairs) == 22
    pairs = pairs + [(e, 6) for e in range(6)]
    _run_tail(emu, "f64", 6, pairs, True, 32, 32, 17, 12, 16, np.linspace(0.5, 20.0, 20), seed=61, reps=1)
    _run_tail(emu, "f32", 1, [(0, 0)], False, 32, 32, 17, 0, 16, np.linspace(0.5, 23.0, 1023), seed=62, reps=1)
    _run_tail(emu, "f64", 6, pairs, True, 32, 32, 17, 12, 16, np.linspace(0.5, 20.0, 145), seed=63, moments=False, reps=1)
    z = np.zeros(8)
    one = (ctypes.c_int * 29)(*([0] * 29))

    def rc(nest, nspec, nids, a=one, b=one, wt=None):
        return emu.emu_rdn0mv_tail_f64(_p(z), ctypes.c_long(4), _p(wt), ctypes.c_long(4), nest, nspec, a, b, 2, ctypes.c_long(2), 1, _p(z), nids,
                                       ctypes.c_double(1.0), 2, 0, _p(z), _p(z), _p(z), _p(z), _p(z), _p(z), 1)
    assert rc(1, 29, 21) == 2 and rc(1, 1, 1025) == 2 and rc(1, 28, 147) == 2 and rc(1, 1, 2) == 2 and rc(7, 1, 21) == 1
    assert rc(1, 1, 21, a=(ctypes.c_int * 1)(1)) == 3                              # the MV field without weights


@pytest.mark.parametrize("case", ["rows", "cols"])
def test_tail_bodies_beyond_one_row_group_and_one_tile_step(emu, case):
    """What 32 x 32 planes do not reach: a band of 1031 rows is cut into groups of 3 rows (344 partial tables, the last of 2 rows), and a
    band of 150 columns takes three tile steps of 64 (the last of 22 columns, three of them beyond the Nyquist column 146: skipped)."""
    pairs = _spectra(2)
    if case == "rows":
        assert emu.emu_rdn0mv_rows_per_group(1031) == 3 and emu.emu_rdn0mv_groups(1031) == 344
        _run_tail(emu, "f64", 2, pairs, True, 1031, 8, 5, 0, 6, np.array([1.5, 60.0, 200.0, 400.0]), seed=7, reps=1)
    else:
        _run_tail(emu, "f32", 2, pairs, True, 5, 152, 150, 2, 146, np.array([1.5, 30.0, 70.0, 100.0, 140.0]), seed=8, reps=1)


# ---- the definition in NumPy ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_64x128():
    from oracle import maps_oracle as mo
    from oracle import rng_oracle as ro
    from oracle.qe_oracle import QEOracle
    from orphics_amd import cosmology, mc
    shape, res = (64, 128), 4.0 * np.pi / 180 / 60
    ny, nx = shape
    ly, lx = mo.laxes(shape, res, res)
    modl = np.hypot(ly[:, None], lx[None, :])
    th = cosmology.default_theory()
    cl = {k: th.lCl(k, modl) for k in ("TT", "EE", "BB", "TE")}
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    nP = 2 * nT
    beam = np.exp(-0.5 * (modl * 1.5 * np.pi / 180 / 60 / np.sqrt(8 * np.log(2))) ** 2)
    tmask = ((modl > 300) & (modl < 2000)).astype(np.float64)
    kmask = ((modl > 20) & (modl < 2500)).astype(np.float64)
    qo = QEOracle(shape, res, res, cl, dict(T=nT, P=nP), beam, dict(T=tmask, P=tmask), kmask_K=kmask)
    for XY in ("TT", "EB"):
        qo.setup(XY)
    tot = dict(TT=cl["TT"] * beam ** 2 + nT, EE=cl["EE"] * beam ** 2 + nP, BB=cl["BB"] * beam ** 2 + nP, TE=cl["TE"] * beam ** 2)
    a, b, c, d = (x[:, :nx // 2 + 1] for x in mc.teb_covsqrt(tot))
    cs = [[a, None, None], [b, c, None], [None, None, d]]

    def draw(sid0):
        """the T, E, B draw of Engine.grf_mix(seed = 11, stream_id0 = sid0) as full (ny, nx) transforms"""
        return [ro.hermitian_expand(z, nx) for z in ro.grf_mix(ny, nx, 11, sid0, cs)]
    return dict(qo=qo, modl=modl, d=draw(6000), s=draw(6 * 2), sp=draw(6 * 2 + 3))


def _qe(qo, XY, X, Y):
    i = {"T": 0, "E": 1, "B": 2}
    return qo.kappa_ft(XY, X[i[XY[0]]], Y[i[XY[1]]])


def test_six_term_identity_of_a_cross_spectrum_and_the_two_halves(oracle_64x128):
    """(64, 128), float64, data and simulations from rng_oracle's grf_mix (realisation 2: streams 12 .. 14 and 15 .. 17; the data from
    streams 6000 ..).  Per mode, Re(A_a conj A_b) with A_e = QE_e(d; s) + QE_e(s; d) is the sum of the four data-simulation terms
    C[ds_a, ds_b] + C[ds_a, sd_b] + C[sd_a, ds_b] + C[sd_a, sd_b], C[u, v] = Re(u conj v), for (a, b) = (TT, EB); and the two halves of the
    sample sum to p(A_a, A_b) - p(B_a, B_b) / 2 + p(B_a, B_b) / 2 = p(A_a, A_b)."""
    o = oracle_64x128
    qo, d, s, sp = o["qo"], o["d"], o["s"], o["sp"]
    c = lambda u, v: (u * np.conj(v)).real
    ds = {XY: _qe(qo, XY, d, s) for XY in ("TT", "EB")}
    sd = {XY: _qe(qo, XY, s, d) for XY in ("TT", "EB")}
    A = {XY: ds[XY] + sd[XY] for XY in ds}
    B = {XY: _qe(qo, XY, s, sp) + _qe(qo, XY, sp, s) for XY in ds}
    lhs = c(A["TT"], A["EB"])
    rhs = c(ds["TT"], ds["EB"]) + c(ds["TT"], sd["EB"]) + c(sd["TT"], ds["EB"]) + c(sd["TT"], sd["EB"])
    scale = np.sqrt(c(A["TT"], A["TT"]).max() * c(A["EB"], A["EB"]).max())
    assert scale > 0 and np.abs(lhs).max() > 1e-3 * scale
    assert np.abs(lhs - rhs).max() <= 1e-12 * scale
    edges = np.linspace(100, 2400, 9)
    ids = np.digitize(o["modl"], edges)
    nids = edges.size + 1
    cnt = np.bincount(ids.ravel(), minlength=nids)[1:-1].astype(np.float64)
    p = lambda u, v: np.bincount(ids.ravel(), weights=c(u, v).ravel(), minlength=nids)[1:-1] / cnt
    for a, b in (("TT", "TT"), ("EB", "EB"), ("TT", "EB")):
        pa, pb = p(A[a], A[b]), p(B[a], B[b])
        x = np.concatenate((pa - pb / 2, pb / 2))
        assert np.abs(x[:8] + x[8:] - pa).max() <= 1e-12 * np.abs(pa).max()
        if a == b:
            assert np.all(x[8:] > 0)


# ---- host surface --------------------------------------------------------------------------------------------------------------------------
def test_abi_version_and_docstring():
    from orphics_amd import _lib, mc
    hdr = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    ver = int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION >= 412
    for name in ("oa_rdn0_set_data_mv", "oa_mc_run_rdn0_mv"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr)
    assert len(_lib.SIGNATURES["oa_mc_run_rdn0_mv"][1]) == len(_lib.SIGNATURES["oa_mc_run_mv"][1])
    doc = " ".join(mc.RDN0MonteCarloPol.__doc__.split())
    for piece in ("A_e = QE_e(d; s) + QE_e(s; d)", "B_e = QE_e(s; s') + QE_e(s'; s)", "A_MV = sum_e w_e A_e", "p(A_a, A_b) - p(B_a, B_b) / 2",
                  "stream_id0 = 6 i)", "stream_id0 = 6 i + 3)", "``2 i`` and ``2 i + 1``", "There is no window", "band-grid sides (2^a 3^b 5^c) run the "
                  "host loop for now", "one_call=False", "reconstruct_hc(XY, X[XY[0]], Y[XY[1]])", "accumulate=True"):
        assert piece in doc, piece
    for name in ("rdn0", "mcn0", "sem", "cov", "data_bandpowers", "debiased", "centers", "sample_host", "run_local", "run", "set_data"):
        assert hasattr(mc.RDN0MonteCarloPol, name), name
    import inspect
    sig = inspect.signature(mc.RDN0MonteCarloPol.__init__)
    assert list(sig.parameters)[1:] == ["qest", "data", "total_power_half", "bin_edges", "estimators", "cross", "mv", "comm", "base_seed", "one_call",
                                        "qu", "iau"]
    # the TT driver is as it was: no window argument, and its docstring says so
    assert "no ``window`` argument" in " ".join(mc.RDN0MonteCarlo.__doc__.split())
