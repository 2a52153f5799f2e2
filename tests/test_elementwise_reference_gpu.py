"""GPU: the kernels of csrc/elementwise.hip -- the flat kernels, the four layout conversions, oa_qe_legs / oa_qe_div and the flat-sky
lensing operator -- against the longdouble restatement of their contracts in oracle/ew_oracle.py, never against another kernel, at
the places where such kernels go wrong: the scalar tail behind the 16-byte vectors, a second step of the grid-stride loop, a second
x-block (nx/2 + 1 = 257) and a ragged one (nx = 320), ny != nx, mixed-radix and chirp-z plans, the y = 0 and Nyquist rows and
columns, the row padding of hc planes, shifts that wrap the map several times in either sign.

Tolerances, per element and per component, never against the plane maximum.  Single-rounding operations (oa_cmul_real, oa_mul_real,
the layouts, the integer shift of oa_lens_split) equal the same-precision NumPy result bit for bit.  Everything else obeys

    |got - ref| <= 1.01 c u_T A,      u_32 = 2^-24, u_64 = 2^-53, 1.01 for second-order terms,

ref the longdouble value on the stored inputs, A the sum of the magnitudes of the terms that are added, c the roundings on the
kernel's longest path (fused multiply-adds only shorten it; scalars are rounded to T by the entries and by the reference alike):

    oa_f2power 3      two products, their sum, the product with norm           A = (|ax bx| + |ay by|) |norm|
    oa_cmul 2         product, sum of two products                            A = |ar br| + |ai bi|, |ar bi| + |ai br|
    oa_axpby_real 2   product, sum                                            A = |alpha x| + |beta y|
    oa_rot2 2         product, sum                                            A = |i1 c| + |i2 s| per component
    oa_qe_legs        no phase: 2 (k F, times the axis) for Gx, Gy, 1 for H   A = the product's magnitude
                      phase: 10 / 9 -- each component of the unit-modulus phase (v^2 - u^2, 2 u v) / (u^2 + v^2) carries at most 6 u
                      (squares 1 + 1, their sum 2 relative, the reciprocal 3, the difference 2 (u^2 + v^2) absolute, the product 1),
                      the complex product 2, the stored k F 1, the axis 1                A = |F| (|k.re| + |k.im|) [|l|]
    oa_qe_div 3       two products, their sum, Fnorm; accumulate 4            A = (|Px lx| + |Py ly|) |F| [+ |out|]
    oa_lens_split 2   shift step, alpha - that                                A = |alpha| + |shift step|
    oa_lens_gather    1 + pow_x + pow_y [+ 1 accumulate]                      A = |coef src dx^px dy^py| [+ |out|]
    oa_hc_derivs      n = a + b: lx^a in a - 1, ly^b in b - 1, their product, times k
    oa_lens_taylor    2 order - 3 + order (order + 1) / 2 - 1: dx^a / a! in 2 (a - 1), the products, one per running sum
                                                                              A = sum |D_ab| |dx^a / a!| |dy^b / b!|

tests/test_elementwise_reference_cpu.py shows on these inputs that each bound holds for a step-by-step evaluation in the plane's
precision and fails for a wrong one."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import ew_oracle as eo  # noqa: E402

LD = np.longdouble
PRECS = ["f32", "f64"]
SENT = 777.0                      # sentinel of pre-filled outputs: no kernel result equals it
PLAN_SHAPES = eo.SHAPES_POW2 + eo.SHAPES_MIXED
WIDE = [(32, 64), (36, 40), (32, 512), (32, 320)]       # one and two x-blocks, whole and ragged


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_error(lib):
    return (lib.oa_last_error() or b"").decode()


def tdt(prec, cplx=False):
    return {("f32", False): torch.float32, ("f64", False): torch.float64, ("f32", True): torch.complex64, ("f64", True): torch.complex128}[prec, cplx]


def sentinel(shape, prec, cplx=False):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENT, dtype=tdt(prec, cplx), device="cuda")


def eng(ny, nx, prec):
    """the cached engine of this geometry with the axes of FlatGeometry.from_res bound"""
    from orphics_amd.engine import Engine
    from orphics_amd.geometry import FlatGeometry
    e = Engine.get(ny, nx, prec)
    assert e.kp == eo.kpitch(nx)
    if e._laxes is None:
        g = FlatGeometry.from_res((ny, nx), eo.RES_ARCMIN)
        ly, lx = g.laxes()
        assert (g.step_y, g.step_x) == eo.steps() and g.step_x < 0 < g.step_y
        ref = eo.laxes(ny, nx, g.step_y, g.step_x, "f64")
        assert np.array_equal(ly, ref[0]) and np.array_equal(lx, ref[1])
        e.set_laxes(ly, lx)
    return e


def assert_bound(got, R, c, prec, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == R.ref.shape, what
    bad = eo.violations(got, R, c, prec)
    if bad.size:
        i = np.unravel_index(bad[0], got.shape)
        b = eo.bound(R, c, prec)
        raise AssertionError("%s %s: element %s got %r ref %r bound %r; %d elements off" % (
            what, prec, i, got[i], complex(R.ref[i]) if np.iscomplexobj(R.ref) else float(R.ref[i]),
            complex(b[i]) if np.iscomplexobj(b) else float(b[i]), bad.size))


def assert_same(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = np.flatnonzero(~(got == ref).reshape(-1))
    assert bad.size == 0, "%s: element %s got %r want %r; %d elements differ" % (
        what, np.unravel_index(bad[0], got.shape), got.reshape(-1)[bad[0]], ref.reshape(-1)[bad[0]], bad.size)


def lib_code(prec):
    from orphics_amd import _lib
    return _lib.load(), {"f32": _lib.OA_F32, "f64": _lib.OA_F64}[prec]


# ---- flat kernels ------------------------------------------------------------------------------------------------------------------------
def run_flat(prec, n, d, which):
    """every flat entry on views of n elements of buffers of n + 8 (outputs pre-filled): {name: result of n elements}; the eight
    elements behind every output must still hold the sentinel"""
    lib, code = lib_code(prec)
    PAD = 8

    def up(a):
        t = torch.zeros(n + PAD, dtype=tdt(prec, np.iscomplexobj(a)), device="cuda")
        t[:n] = dev(a)
        return t
    k1, k2, f, a, b, c, s = (up(d[key]) for key in ("k1", "k2", "f", "a", "b", "c", "s"))
    out = {}

    def call(name, cplx, fn):
        o = [sentinel(n + PAD, prec, cplx) for _ in range(2 if name == "rot2" else 1)]
        rc = fn(*o)
        assert rc == 0, "%s n=%d: %s" % (name, n, last_error(lib))
        torch.cuda.synchronize()
        for t in o:
            tail = t[n:].cpu().numpy()
            assert np.all(tail == SENT), "%s n=%d wrote behind its end: %r" % (name, n, tail)
        out[name] = tuple(t[:n] for t in o) if len(o) > 1 else o[0][:n]
    if "f2power" in which:
        call("f2power", False, lambda o: lib.oa_f2power(code, P(k1), P(k2), P(o), eo.NORM, n, stream()))
    if "cmul_real" in which:
        call("cmul_real", True, lambda o: lib.oa_cmul_real(code, P(k1), P(f), P(o), n, stream()))
    if "mul_real" in which:
        call("mul_real", False, lambda o: lib.oa_mul_real(code, P(a), P(b), P(o), n, stream()))
    if "axpby" in which:
        call("axpby", False, lambda o: lib.oa_axpby_real(code, P(a), P(b), P(o), eo.ALPHA, eo.BETA, n, stream()))
    if "cmul" in which:
        call("cmul", True, lambda o: lib.oa_cmul(code, P(k1), P(k2), P(o), n, stream()))
    if "rot2" in which:
        call("rot2", True, lambda o1, o2: lib.oa_rot2(code, P(c), P(s), P(k1), P(k2), P(o1), P(o2), n, stream()))
    return out


def check_flat(prec, n, d, out):
    if "f2power" in out:
        assert_bound(out["f2power"], eo.f2power(d["k1"], d["k2"], eo.NORM, prec), eo.C_F2POWER, prec, "f2power n=%d" % n)
    if "cmul_real" in out:
        assert_same(out["cmul_real"], eo.cmul_real(d["k1"], d["f"]), "cmul_real n=%d" % n)
    if "mul_real" in out:
        assert_same(out["mul_real"], eo.mul_real(d["a"], d["b"]), "mul_real n=%d" % n)
    if "axpby" in out:
        assert_bound(out["axpby"], eo.axpby(d["a"], d["b"], eo.ALPHA, eo.BETA, prec), eo.C_AXPBY, prec, "axpby n=%d" % n)
    if "cmul" in out:
        assert_bound(out["cmul"], eo.cmul(d["k1"], d["k2"]), eo.C_CMUL, prec, "cmul n=%d" % n)
    if "rot2" in out:
        o1, o2 = eo.rot2(d["c"], d["s"], d["k1"], d["k2"])
        assert_bound(out["rot2"][0], o1, eo.C_ROT2, prec, "rot2 o1 n=%d" % n)
        assert_bound(out["rot2"][1], o2, eo.C_ROT2, prec, "rot2 o2 n=%d" % n)


ALL_FLAT = ("f2power", "cmul_real", "mul_real", "axpby", "cmul", "rot2")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", eo.FLAT_N)
def test_flat_kernels(prec, n):
    """every flat entry at 0, below / at / above one 16-byte vector and around 1024 elements: the vector body and the scalar tail;
    n = 0 leaves the output untouched; nothing is written behind element n"""
    d = eo.flat_inputs(eo.SEED, n, prec)
    out = run_flat(prec, n, d, ALL_FLAT)
    check_flat(prec, n, d, out)


@pytest.mark.parametrize("which,n", [(("f2power", "cmul_real", "mul_real", "axpby"), 4 * 256 * 8192 + 5), (("cmul", "rot2"), 256 * 8192 + 257)])
def test_flat_kernels_past_the_grid_cap(which, n):
    """one element count past 8192 blocks of 256 lanes (of four elements for the vectorised kernels): the grid-stride loop takes a
    second step, and the tail sits behind it.  float32 only (the loop is the same template)."""
    d = eo.flat_inputs(eo.SEED, n, "f32")
    out = run_flat("f32", n, d, which)
    check_flat("f32", n, d, out)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [5, 1027])
def test_in_place_calls_of_the_library(prec, n):
    """the in-place forms the library itself runs -- cmul(k, f, out=k) and cmul_real(k, f, out=k) (filter_map), mul_real(g, h, out=g),
    axpby(g, a, s, 1, out=a), axpby(g, g, s, 0, out=a) (the estimators) -- equal the out-of-place result bit for bit"""
    e = eng(32, 32, prec)
    d = eo.flat_inputs(eo.SEED, n, prec)
    k, k2, f, a, b = (dev(d[key]) for key in ("k1", "k2", "f", "a", "b"))
    for name, fn, first in (("cmul", lambda x, **kw: e.cmul(x, k2, **kw), k), ("cmul_real", lambda x, **kw: e.cmul_real(x, f, **kw), k),
                            ("mul_real", lambda x, **kw: e.mul_real(x, b, **kw), a)):
        want = fn(first).cpu().numpy()
        x = first.clone()
        got = fn(x, out=x)
        assert got is x
        assert_same(got, want, "%s in place n=%d" % (name, n))
    want = e.axpby(a, b, eo.ALPHA, 1.0).cpu().numpy()
    y = b.clone()
    assert_same(e.axpby(a, y, eo.ALPHA, 1.0, out=y), want, "axpby out=b")
    assert_bound(want, eo.axpby(d["a"], d["b"], eo.ALPHA, 1.0, prec), eo.C_AXPBY, prec, "axpby(a, b, alpha, 1)")
    o = sentinel(n, prec)
    assert_same(e.axpby(a, a, -1.0, 0.0, out=o), -d["a"], "axpby(a, a, -1, 0)")


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", PLAN_SHAPES + [eo.SHAPE_CZT])
def test_layouts(prec, ny, nx):
    """index-encoding planes with 1e6 on the hc padding: every element of every conversion, bit for bit; row 0, row ny/2, column 0
    and column nx/2 named; the entries that do not own the padding leave it alone, oa_fullreal_to_hc zeroes it"""
    e = eng(ny, nx, prec)
    kp, nxh, w = e.kp, nx // 2, nx // 2 + 1
    st = stream()
    hc, hr = eo.index_plane_hc(ny, nx, kp, prec), eo.index_plane_hc(ny, nx, kp, prec, real=True)
    fc, fr = eo.index_plane_full(ny, nx, prec), eo.index_plane_full(ny, nx, prec, real=True)

    def run(fn, src, oshape, cplx):
        o, s = sentinel(oshape, prec, cplx), dev(src)
        rc = fn(e.plan, P(s), P(o), st)
        assert rc == 0, last_error(e.lib)
        return o.cpu().numpy()
    for name, got, want in (("hc_to_full", run(e.lib.oa_hc_to_full, hc, (ny, nx), True), eo.hc_to_full(hc, nx)),
                            ("hcreal_to_full", run(e.lib.oa_hcreal_to_full, hr, (ny, nx), False), eo.hcreal_to_full(hr, nx))):
        for part, sl in (("row 0", np.s_[0, :]), ("row ny/2", np.s_[ny // 2, :]), ("column 0", np.s_[:, 0]), ("column nx/2", np.s_[:, nxh]),
                         ("row 1", np.s_[1, :]), ("column nx/2 + 1", np.s_[:, nxh + 1]), ("column nx - 1", np.s_[:, nx - 1])):
            assert_same(got[sl], want[sl], "%s %s %s" % (name, prec, part))
        assert_same(got, want, "%s %s" % (name, prec))
        assert np.abs(got).max() < 1e6, "%s read the padding" % name
    fill_c = np.full((ny, kp), SENT, dtype=hc.dtype)
    got = run(e.lib.oa_full_to_hc, fc, (ny, kp), True)
    want = eo.full_to_hc(fc, kp, fill_c)
    for part, sl in (("row 0", np.s_[0, :]), ("row ny/2", np.s_[ny // 2, :]), ("column 0", np.s_[:, 0]), ("column nx/2", np.s_[:, nxh])):
        assert_same(got[sl], want[sl], "full_to_hc %s %s" % (prec, part))
    assert_same(got, want, "full_to_hc %s" % prec)
    got = run(e.lib.oa_fullreal_to_hc, fr, (ny, kp), False)
    assert_same(got, eo.fullreal_to_hc(fr, kp), "fullreal_to_hc %s" % prec)
    assert np.all(got[:, w:] == 0) and np.array_equal(got[:, nxh], fr[:, nxh])
    # the engine wrappers hand out the same planes
    assert_same(e.hc_to_full(dev(hc)), eo.hc_to_full(hc, nx), "Engine.hc_to_full")
    assert_same(e.full_to_hc(dev(fc)), eo.full_to_hc(fc, kp, np.zeros_like(fill_c)), "Engine.full_to_hc")


# ---- legs and divergence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", PLAN_SHAPES)
def test_qe_legs_and_div(prec, ny, nx):
    """every combination of phase_g, phase_h in {0, +1, -1} and h_times_i on the rectangular axes of FlatGeometry.from_res; the l = 0
    mode (phase 1), the Nyquist row and column (Gx / Gy exactly zero where the derivative axis is, H not), the padding columns
    untouched; oa_qe_div with and without accumulate on a pre-filled plane"""
    e = eng(ny, nx, prec)
    kp, nxh, w = e.kp, nx // 2, nx // 2 + 1
    ly, lx, lyd, lxd = eo.laxes(ny, nx, *eo.steps(), prec)
    d = eo.legs_inputs(eo.SEED, ny, nx, kp, prec)
    kX, kY, FG, FH, Fn = (dev(d[key]) for key in ("kX", "kY", "FG", "FH", "Fn"))
    for pg in (0, 1, -1):
        for ph in (0, 1, -1):
            for hi in (False, True):
                outs = tuple(sentinel((ny, kp), prec, True) for _ in range(3))
                e.qe_legs(kX, kY, FG, FH, phase_g=pg, phase_h=ph, h_times_i=hi, out=outs)
                refs = eo.qe_legs(d["kX"], d["kY"], d["FG"], d["FH"], ly, lx, lyd, lxd, nx, pg, ph, hi)
                cg, ch = (eo.C_LEGS_PHASE_G if pg else eo.C_LEGS_PLAIN_G), (eo.C_LEGS_PHASE_H if ph else eo.C_LEGS_PLAIN_H)
                what = "pg %d ph %d i %d (%d, %d)" % (pg, ph, hi, ny, nx)
                got = [o.cpu().numpy() for o in outs]
                for name, g, R, c in zip(("Gx", "Gy", "H"), got, refs, (cg, cg, ch)):
                    assert np.all(g[:, w:] == SENT), "%s %s wrote the padding" % (name, what)
                    assert_bound(g[:, :w], R, c, prec, "%s %s" % (name, what))
                assert np.all(got[0][:, nxh] == 0) and np.all(got[1][ny // 2, :w] == 0), "Nyquist gradient " + what
                assert np.all(got[2][:, nxh] != 0) and np.all(got[2][ny // 2, :w] != 0), "Nyquist H " + what
                assert got[0][0, 0] == 0 and got[1][0, 0] == 0
                # l = 0: phase 1, so H there is k FH [times i], one rounding
                h00 = complex(d["kY"][0, 0]) * float(d["FH"][0, 0]) * (1j if hi else 1)
                assert abs(got[2][0, 0] - h00) <= 2 * eo.U[prec] * abs(h00), "l = 0 " + what
    for acc in (False, True):
        out = dev(d["out0"]).clone()
        e.qe_div(kX, kY, Fn, out=out, accumulate=acc)
        got = out.cpu().numpy()
        assert np.all(got[:, w:] == 1e6), "qe_div wrote the padding"
        assert_bound(got[:, :w], eo.qe_div(d["kX"], d["kY"], d["Fn"], lyd, lxd, nx, out0=d["out0"] if acc else None),
                     eo.C_DIV_ACC if acc else eo.C_DIV, prec, "qe_div acc %d (%d, %d)" % (acc, ny, nx))


# ---- lensing operator -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", [(32, 64), (36, 40), (32, 320)])
def test_lens_split(prec, ny, nx):
    """positive (y) and negative (x) step, |alpha / step| up to 40 and 2^-10 clear of the ties: the shifts are exact; ties, with a
    power-of-two step of either sign and m of both parities and signs, go to even with an exact remainder"""
    e = eng(ny, nx, prec)
    T = eo.RDT[prec]
    for step, seed in zip(eo.steps(), (1, 2)):
        alpha = eo.split_alpha(eo.SEED + seed, (ny, nx), step, prec)
        shift, delta = e.lens_split(dev(alpha), step)
        want, R = eo.lens_split(alpha, step, prec)
        assert shift.dtype == torch.int32 and want.min() < -30 and want.max() > 30
        assert_same(shift.cpu().numpy(), want.astype(np.int32), "lens_split shift step %g" % step)
        assert_bound(delta, R, eo.C_SPLIT, prec, "lens_split delta step %g" % step)
    m = np.resize(np.array([-6, -5, -2, -1, 0, 1, 2, 5, 6, 1023, -1024], dtype=np.float64), ny * nx).reshape(ny, nx)
    for step in (2.0 ** -11, -2.0 ** -11):
        alpha = ((m + 0.5) * step).astype(T)
        shift, delta = e.lens_split(dev(alpha), step)
        want = np.where(m % 2 == 0, m, m + 1)
        assert_same(shift.cpu().numpy(), want.astype(np.int32), "lens_split ties step %g" % step)
        assert_same(delta.cpu().numpy(), (alpha - want * step).astype(T), "lens_split tie remainders step %g" % step)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", WIDE)
def test_lens_gather(prec, ny, nx):
    """shifts from [-(3 n + 1), 3 n + 1] per axis with the exact multiples of the sides, powers (0, 0) .. (3, 2), coefficients of both
    signs, accumulate on and off; a constant shift is np.roll, bit for bit"""
    e = eng(ny, nx, prec)
    g = eo.gather_inputs(eo.SEED, ny, nx, prec)
    src, sx, sy, dx, dy = (dev(g[key]) for key in ("src", "sx", "sy", "dx", "dy"))
    assert g["sx"].min() == -(3 * nx + 1) and g["sx"].max() == 3 * nx + 1 and g["sy"].min() == -(3 * ny + 1)
    for px, py, coef in eo.GATHER_CASES:
        for acc in (False, True):
            out0 = eo.gather_out0(g, px, py, prec)
            out = dev(out0).clone()
            e.lens_gather(src, sx, sy, dx, dy, px, py, coef, out, acc)
            R = eo.lens_gather(g["src"], g["sx"], g["sy"], g["dx"], g["dy"], px, py, coef, prec, out0=out0 if acc else None)
            assert_bound(out, R, eo.c_gather(px, py, acc), prec, "lens_gather (%d, %d) coef %g acc %d" % (px, py, coef, acc))
    for s_y, s_x in [(1, -2), (ny + 1, -2 - 3 * nx), (-ny, nx), (-3 * ny - 1, 3 * nx + 1)]:
        cx_, cy_ = dev(np.full((ny, nx), s_x, dtype=np.int32)), dev(np.full((ny, nx), s_y, dtype=np.int32))
        out = sentinel((ny, nx), prec)
        e.lens_gather(src, cx_, cy_, dx, dy, 0, 0, 1.0, out, False)
        assert_same(out, np.roll(g["src"], (-(s_y % ny), -(s_x % nx)), axis=(0, 1)), "constant shift (%d, %d)" % (s_y, s_x))


def derivs_on_gpu(e, khc, order):
    nd = order * (order + 1) // 2 - 1
    dk = sentinel((nd, e.ny, e.kp), e.prec, True)
    rc = e.lib.oa_hc_derivs(e.plan, P(khc), order, P(dk), e.ny * e.kp, stream())
    assert rc == 0, last_error(e.lib)
    return dk


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", WIDE)
def test_hc_derivs(prec, ny, nx):
    """orders 2, 5, 8: every plane against (i lx)^a (i ly)^b k on the derivative axes; the Nyquist column of every a > 0 and the
    Nyquist row of every b > 0 exactly zero; the padding columns untouched"""
    e = eng(ny, nx, prec)
    w = nx // 2 + 1
    _, _, lyd, lxd = eo.laxes(ny, nx, *eo.steps(), prec)
    hc = eo.derivs_input(eo.SEED, ny, nx, prec)
    refs = eo.hc_derivs(hc, lyd, lxd, nx, 8)
    for order in (2, 5, 8):
        got = derivs_on_gpu(e, dev(hc), order).cpu().numpy()
        for (a, b), R in refs.items():
            if a + b >= order:
                continue
            pl = got[eo.plane_index(a, b)]
            assert np.all(pl[:, w:] == SENT)
            assert_bound(pl[:, :w], R, eo.c_derivs(a + b), prec, "hc_derivs order %d (a, b) = (%d, %d)" % (order, a, b))
            if a:
                assert np.all(pl[:, nx // 2] == 0)
            if b:
                assert np.all(pl[ny // 2, :w] == 0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", WIDE)
def test_lens_taylor(prec, ny, nx):
    """orders 1 .. 8 on derivative planes made by the oracle's side (only this kernel is under test), a deflection of up to 2.5
    pixels of both signs; order 1 is the plain gather, bit for bit"""
    e = eng(ny, nx, prec)
    t = eo.taylor_inputs(eo.SEED, ny, nx, prec)
    src, planes, sx, sy, dx, dy = (dev(t[key]) for key in ("src", "planes", "sx", "sy", "dx", "dy"))
    for order in range(1, 9):
        nd = order * (order + 1) // 2 - 1
        out = sentinel((ny, nx), prec)
        rc = e.lib.oa_lens_taylor(e.plan, P(src), P(planes) if nd else None, ny * nx, order, P(sx), P(sy), P(dx), P(dy), P(out), stream())
        assert rc == 0, last_error(e.lib)
        R = eo.lens_taylor(t["src"], t["planes"][:nd], t["sx"], t["sy"], t["dx"], t["dy"], order)
        assert_bound(out, R, eo.c_taylor(order), prec, "lens_taylor order %d (%d, %d)" % (order, ny, nx))
        if order == 1:
            assert_same(out, R.ref.astype(eo.RDT[prec]), "lens_taylor order 1")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", [(32, 64), (36, 40)])
def test_lens_maps(prec, ny, nx, capsys):
    """oa_lens_maps at orders 1, 2, 8 against (a) the fine-grained sequence oa_hc_derivs -> C2R per plane -> oa_lens_taylor and (b) the
    longdouble oracle of the whole operator (longdouble DFT matrices).  Margin per element: the Taylor bound 1.01 c u A plus the
    transforms' error, 4 eps sum_{a + b >= 1} rms(D_ab) |dx^a / a!| |dy^b / b!| with eps = max |irfft(rfft(x)) - x| / rms(x) MEASURED in this
    test on the same white map with this plan's own transforms -- a derivative plane passes one forward and one inverse transform like
    the round trip, its error is white like the map's (so the factors (i l)^n scale signal and error alike), and 4 covers the spread
    of a maximum over 35 planes against the one measured; (a) compares two transform paths and gets twice that.
    Measured on an MI355X: eps = 7.2e-7 (f32) and 1.1e-15 (f64) at (32, 64), 6.1e-7 and 1.0e-15 at (36, 40), about one u log2 N;
    the largest error / margin was 0.26 (order 2) and 0.13 (order 8) against the oracle, 0.12 between the two GPU paths."""
    from orphics_amd._lib import check
    e = eng(ny, nx, prec)
    T = eo.RDT[prec]
    sty, stx = eo.steps()
    t = eo.taylor_inputs(eo.SEED, ny, nx, prec)
    src, sx, sy, dx, dy = (dev(t[key]) for key in ("src", "sx", "sy", "dx", "dy"))
    rms = float(np.sqrt(np.mean(t["src"].astype(np.float64) ** 2)))
    eps = float((e.irfft(e.rfft(src)) - src).abs().max()) / rms
    with capsys.disabled():
        print("\nlens_maps %s (%d, %d): round trip eps = %.3g (%.2f u log2 N)" % (prec, ny, nx, eps, eps / eo.U[prec] / np.log2(ny * nx)))
    assert eps < 64 * eo.U[prec]                      # sanity only: a transform of ~2^11 points loses a few u log2 N
    k0 = e.rfft(src)
    for order in (1, 2, 8):
        nd = order * (order + 1) // 2 - 1
        out = sentinel((1, ny, nx), prec)
        check(e.lib.oa_lens_maps(e.plan, 1, P(src), ny * nx, order, P(sx), P(sy), P(dx), P(dy), P(out), ny * nx, stream()))
        fine = sentinel((ny, nx), prec)
        dr = torch.empty((max(nd, 1), ny, nx), dtype=e.rdt, device=e.device)
        if nd:
            dk = derivs_on_gpu(e, k0, order)
            dk[:, :, nx // 2 + 1:] = 0
            for i in range(nd):
                e.irfft(dk[i], out=dr[i])
        check(e.lib.oa_lens_taylor(e.plan, P(src), P(dr), ny * nx, order, P(sx), P(sy), P(dx), P(dy), P(fine), stream()))
        R, planes = eo.flat_taylens(t["src"], t["sx"], t["sy"], t["dx"], t["dy"], sty, stx, order, prec)
        fft_margin = np.zeros((ny, nx), dtype=LD)
        for n in range(1, order):
            for b in range(n + 1):
                a = n - b
                pr = np.sqrt(np.mean(planes[eo.plane_index(a, b)] ** 2))
                fft_margin += 4 * LD(eps) * pr * np.abs(t["dx"].astype(LD) ** a * t["dy"].astype(LD) ** b) / LD(eo.factorial(a) * eo.factorial(b))
        margin = eo.bound(R, max(eo.c_taylor(order), 1), prec) + fft_margin
        got, fin = out[0].cpu().numpy().astype(LD), fine.cpu().numpy().astype(LD)
        for name, err, lim in (("oa_lens_maps vs oracle", np.abs(got - R.ref), margin), ("fine-grained vs oracle", np.abs(fin - R.ref), margin),
                               ("oa_lens_maps vs fine-grained", np.abs(got - fin), 2 * margin)):
            bad = np.flatnonzero(~(err <= lim).reshape(-1))
            with capsys.disabled():
                print("  order %d %s: max err / margin = %.3g" % (order, name, float((err / lim).max())))
            assert bad.size == 0, "%s %s order %d (%d, %d): %d pixels off, worst err / margin %.3g" % (
                name, prec, order, ny, nx, bad.size, float((err / lim).max()))
        if order == 1:
            assert_same(out[0], R.ref.astype(T), "oa_lens_maps order 1 is the gather")


# ---- refusals: nothing is launched --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_refusals_launch_nothing(prec):
    """each refused call returns non-zero with oa_last_error set and leaves its pre-filled output untouched"""
    ny, nx = 32, 64
    e = eng(ny, nx, prec)
    lib, st = e.lib, stream()
    t = eo.taylor_inputs(eo.SEED, ny, nx, prec)
    src, planes, sx, sy, dx, dy = (dev(t[key]) for key in ("src", "planes", "sx", "sy", "dx", "dy"))
    khc = e.rfft(src)
    dk = sentinel((35, ny, e.kp), prec, True)
    out = sentinel((ny, nx), prec)

    def refused(rc, word, *untouched):
        assert rc != 0 and word in last_error(lib), (rc, last_error(lib))
        torch.cuda.synchronize()
        for u in untouched:
            assert bool((u == SENT).all()), "a refused call wrote its output (%s)" % word
    for order in (1, 9, 0, -1):
        refused(lib.oa_hc_derivs(e.plan, P(khc), order, P(dk), ny * e.kp, st), "order", dk)
    refused(lib.oa_hc_derivs(e.plan, P(khc), 5, P(dk), ny * e.kp - 1, st), "plane_stride", dk)
    for order in (0, 9, -1):
        refused(lib.oa_lens_taylor(e.plan, P(src), P(planes), ny * nx, order, P(sx), P(sy), P(dx), P(dy), P(out), st), "order", out)
    refused(lib.oa_lens_taylor(e.plan, P(src), None, ny * nx, 2, P(sx), P(sy), P(dx), P(dy), P(out), st), "order", out)
    refused(lib.oa_lens_taylor(e.plan, P(src), P(planes), ny * nx - 1, 5, P(sx), P(sy), P(dx), P(dy), P(out), st), "plane_stride", out)
    keep = src.clone()
    refused(lib.oa_lens_taylor(e.plan, P(src), P(planes), ny * nx, 5, P(sx), P(sy), P(dx), P(dy), P(src), st), "in-place")
    assert torch.equal(src, keep)
    for px, py in ((9, 8), (17, 0), (0, 17), (-1, 0)):
        refused(lib.oa_lens_gather(e.plan, P(src), P(sx), P(sy), P(dx), P(dy), px, py, 1.0, P(out), 0, st), "powers", out)
    refused(lib.oa_lens_gather(e.plan, P(src), P(sx), P(sy), P(dx), P(dy), 0, 0, 1.0, P(src), 0, st), "in-place")
    assert torch.equal(src, keep)
    with pytest.raises(ValueError):
        e.lens_gather(src, sx, sy, dx, dy, 0, 0, 1.0, src, False)
    refused(lib.oa_lens_split(e.code, P(src), 0.0, P(sx), P(out), ny * nx, st), "oa_lens_split", out)
    # legs, divergence and derivatives on a plan without axes
    from orphics_amd._lib import OrphicsAmdError
    from orphics_amd.engine import Engine
    bare = Engine(ny, nx, prec)
    outs = tuple(sentinel((ny, bare.kp), prec, True) for _ in range(3))
    fr = sentinel((ny, bare.kp), prec)
    with pytest.raises(OrphicsAmdError, match="set_laxes"):
        bare.qe_legs(outs[0].clone(), outs[0].clone(), fr.clone(), fr.clone(), out=outs)
    with pytest.raises(OrphicsAmdError, match="set_laxes"):
        bare.qe_div(outs[0].clone(), outs[0].clone(), fr.clone(), out=outs[0])
    refused(lib.oa_hc_derivs(bare.plan, P(khc), 5, P(dk), ny * bare.kp, st), "set_laxes", dk, *outs)


class NoLibrary(object):
    """stands in for the loaded library: any call into it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


@pytest.mark.parametrize("prec", PRECS)
def test_engine_validates_out_before_the_library(prec):
    """a short, wrongly typed, host-side or strided ``out=`` (and such operands of rot2 / lens_gather) raises ValueError before
    anything is passed to the library"""
    from orphics_amd.engine import Engine
    ny, nx = 32, 32
    e = Engine(ny, nx, prec)
    n = 64
    d = eo.flat_inputs(eo.SEED, n, prec)
    k, k2, f, a, b, c, s = (dev(d[key]) for key in ("k1", "k2", "f", "a", "b", "c", "s"))
    other = "f64" if prec == "f32" else "f32"
    real_lib = e.lib
    e.lib = NoLibrary()
    try:
        calls = {"f2power": (lambda o: e.f2power(k, k2, eo.NORM, out=o), False), "cmul_real": (lambda o: e.cmul_real(k, f, out=o), True),
                 "cmul": (lambda o: e.cmul(k, k2, out=o), True), "mul_real": (lambda o: e.mul_real(a, b, out=o), False),
                 "axpby": (lambda o: e.axpby(a, b, 1.0, 2.0, out=o), False)}
        for name, (fn, cplx) in calls.items():
            bad = {"short": sentinel(n - 1, prec, cplx), "long": sentinel(n + 1, prec, cplx), "other precision": sentinel(n, other, cplx),
                   "real for complex": sentinel(n, prec, not cplx), "host": sentinel(n, prec, cplx).cpu(),
                   "strided": sentinel(2 * n, prec, cplx)[::2], "no tensor": np.zeros(n)}
            for why, o in bad.items():
                with pytest.raises(ValueError):
                    fn(o)
                    pytest.fail("%s accepted an out= that is %s" % (name, why))
        for args in ((c[:-1], s, k, k2), (c, s.cpu(), k, k2), (c, s, k, k2[:-1]), (c, s, k.real.contiguous(), k2), (c.double() if prec == "f32" else c.float(), s, k, k2)):
            with pytest.raises(ValueError):
                e.rot2(*args)
        src, dxp = torch.zeros((ny, nx), dtype=e.rdt, device="cuda"), torch.zeros((ny, nx), dtype=e.rdt, device="cuda")
        si = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
        o = sentinel((ny, nx), prec)
        for args in ((src, si, si, dxp, dxp, 0, 0, 1.0, o[:-1], False), (src, si, si, dxp, dxp, 0, 0, 1.0, o.cpu(), False),
                     (src, si.cpu(), si, dxp, dxp, 0, 0, 1.0, o, False), (src, si, si.long(), dxp, dxp, 0, 0, 1.0, o, False),
                     (src, si, si[:-1], dxp, dxp, 0, 0, 1.0, o, False), (src, si, si, dxp.cpu(), dxp, 0, 0, 1.0, o, False),
                     (src, si, si, dxp, dxp, 0, 0, 1.0, sentinel((ny, nx), other), False),
                     (src, si.t().contiguous().t(), si, dxp, dxp, 0, 0, 1.0, o, False)):
            with pytest.raises(ValueError):
                e.lens_gather(*args)
    finally:
        e.lib = real_lib


@pytest.mark.parametrize("prec", PRECS)
def test_vector_entries_refuse_misaligned_pointers(prec):
    """oa_f2power, oa_cmul_real, oa_mul_real and oa_axpby_real move 16 bytes per access: a pointer one element into an allocation that
    is not 16-byte aligned is refused with oa_last_error set, and nothing is launched (no vector kernel ever runs misaligned)"""
    from orphics_amd._lib import OrphicsAmdError
    lib, code = lib_code(prec)
    n = 16
    kc = [torch.ones(n + 8, dtype=tdt(prec, True), device="cuda") for _ in range(2)]
    fr = [torch.ones(n + 8, dtype=tdt(prec), device="cuda") for _ in range(2)]
    oc, orl = sentinel(n + 8, prec, True), sentinel(n + 8, prec)
    st = stream()
    entries = {"oa_f2power": (lambda o: lib.oa_f2power(code, P(kc[0], o[0]), P(kc[1], o[1]), P(orl, o[2]), 1.0, n, st), (kc[0], kc[1], orl)),
               "oa_cmul_real": (lambda o: lib.oa_cmul_real(code, P(kc[0], o[0]), P(fr[0], o[1]), P(oc, o[2]), n, st), (kc[0], fr[0], oc)),
               "oa_mul_real": (lambda o: lib.oa_mul_real(code, P(fr[0], o[0]), P(fr[1], o[1]), P(orl, o[2]), n, st), (fr[0], fr[1], orl)),
               "oa_axpby_real": (lambda o: lib.oa_axpby_real(code, P(fr[0], o[0]), P(fr[1], o[1]), P(orl, o[2]), 1.0, 1.0, n, st), (fr[0], fr[1], orl))}
    tried = 0
    for name, (fn, tensors) in entries.items():
        for which in range(3):
            off = [0, 0, 0]
            off[which] = 1
            if (tensors[which].data_ptr() + tensors[which].element_size()) % 16 == 0:
                continue                                  # one complex128 element is 16 bytes: still aligned, a valid call
            rc = fn(off)
            assert rc != 0 and "16-byte aligned" in last_error(lib) and name in last_error(lib), (name, which, rc, last_error(lib))
            tried += 1
    torch.cuda.synchronize()
    assert tried == (12 if prec == "f32" else 8) and bool((oc == SENT).all()) and bool((orl == SENT).all())
    e = eng(32, 32, prec)
    a = torch.ones(n + 1, dtype=e.rdt, device="cuda")
    with pytest.raises(OrphicsAmdError, match="16-byte aligned"):
        e.mul_real(a[1:], a[1:])
