"""Plain NumPy restatement, at np.longdouble, of the contracts of the flat elementwise entries, the four layout conversions,
oa_qe_legs / oa_qe_div and the flat-sky lensing operator (include/orphics_amd.h) -- written from the header's formulas, not from
the kernels.  Every bounded operation returns ``Ref(ref, A)``: the longdouble value on inputs taken as stored (already rounded to
the plane's precision) and the per-element sum of the magnitudes of the terms that are added; for complex results both are complex
arrays whose real / imaginary part belongs to the real / imaginary component.  The tests assert, per element and per component,

    |got - ref| <= 1.01 c u_T A

with c the number of roundings on the kernel's longest path (``C_*`` below, each with its count).  The input generators of the
GPU tests live here too, so the CPU tests show on the same inputs that the bounds hold for a step-by-step evaluation in the plane's
precision and fail for a wrong one."""
from collections import namedtuple
from math import factorial

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
RDT = {"f32": np.float32, "f64": np.float64}
CDT = {"f32": np.complex64, "f64": np.complex128}
PI = LD(4) * np.arctan(LD(1))

Ref = namedtuple("Ref", "ref A")
I_POW = [CLD(1), CLD(1j), CLD(-1), CLD(-1j)]          # i^n, exact

# ---- rounding counts (longest path, fused multiply-adds only shorten it) ---------------------------------------------------------
C_F2POWER = 3        # product, sum (the second product may fuse), product with the norm already rounded to T
C_CMUL = 2           # product, difference / sum of two products
C_AXPBY = 2          # product, sum (alpha, beta already rounded to T)
C_ROT2 = 2           # product, difference / sum
C_LEGS_PLAIN_G = 2   # k FG, times the derivative axis
C_LEGS_PLAIN_H = 1   # k FH
# phase: u^2, v^2 (1 each), r2 = u^2 + v^2 (2 relative), 1 / r2 (3), v^2 - u^2 (absolute 2 r2), product (1): each component of the
# unit-modulus phase is off by at most 6 u; the complex product adds 2 and the stored k F carries 1: 9 relative to |F| (|k.re| + |k.im|)
C_LEGS_PHASE_H = 9
C_LEGS_PHASE_G = 10  # ... times the derivative axis
C_DIV = 3            # two products and their sum (2 relative to the magnitude sum), times Fnorm
C_DIV_ACC = 4        # ... and the sum with the plane's previous content
C_SPLIT = 2          # shift * step, alpha - that


def c_gather(px, py, accumulate):
    """coef * src (1), dx^px by repeated products times v (px roundings: the first product is by 1), likewise dy, the final sum"""
    return 1 + px + py + (1 if accumulate else 0)


def c_derivs(n):
    """(i lx)^a (i ly)^b k, a + b = n: lx^a in a - 1 roundings, ly^b in b - 1, their product 1, times k 1 (a product by 1 is exact)"""
    return n


def c_taylor(order):
    """dx^a / a! in 2 (a - 1) roundings (product and quotient per step, the first step exact), likewise dy; their product and the one
    with D_ab: at most 2 n - 1 per term with n = order - 1; then one rounding per running sum over the order (order + 1) / 2 terms"""
    return 0 if order == 1 else 2 * order - 3 + order * (order + 1) // 2 - 1


def ld(a):
    a = np.asarray(a)
    return a.astype(CLD) if np.iscomplexobj(a) else a.astype(LD)


def cpack(re, im):
    out = np.empty(np.shape(re), dtype=CLD)
    out.real, out.imag = re, im
    return out


def bound(R, c, prec):
    """per element (and per component) 1.01 c u_T A"""
    return (LD(1.01) * LD(c) * LD(U[prec])) * R.A


def violations(got, R, c, prec):
    """indices (flat) where got leaves the bound; complex: either component"""
    got, b = ld(got), bound(R, c, prec)
    if np.iscomplexobj(R.ref):
        bad = ~(np.abs(got.real - R.ref.real) <= b.real) | ~(np.abs(got.imag - R.ref.imag) <= b.imag)
    else:
        bad = ~(np.abs(got - R.ref) <= b)
    return np.flatnonzero(bad)


# ---- inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
def mixed_real(rng, shape, prec):
    """magnitudes 1e-3 .. 1e3, uniform in the exponent, both signs: cancellation shows per element"""
    return (10.0 ** rng.uniform(-3, 3, shape) * rng.choice([-1.0, 1.0], shape)).astype(RDT[prec])


def mixed_complex(rng, shape, prec):
    return (mixed_real(rng, shape, "f64") + 1j * mixed_real(rng, shape, "f64")).astype(CDT[prec])


def flat_inputs(seed, n, prec):
    rng = np.random.default_rng([seed, n])
    return dict(k1=mixed_complex(rng, n, prec), k2=mixed_complex(rng, n, prec), f=mixed_real(rng, n, prec), a=mixed_real(rng, n, prec),
                b=mixed_real(rng, n, prec), c=mixed_real(rng, n, prec), s=mixed_real(rng, n, prec))


NORM, ALPHA, BETA = 0.37, 1.7, -0.3          # no powers of two: the float32 entries round them
SEED = 20
# 0, below / at / above one vector of four, a ragged and a whole number of 256-lane blocks of vectors
FLAT_N = [0, 1, 3, 4, 5, 1023, 1024, 1027]
# (32, 512): nx/2 + 1 = 257, one column into the second x-block; (32, 320): a ragged second block of the full-width kernels
SHAPES_POW2 = [(32, 32), (32, 64), (64, 32), (32, 512)]
SHAPES_MIXED = [(36, 40), (32, 320)]
SHAPE_CZT = (34, 38)
RES_ARCMIN = 2.0


def kpitch(nx):
    """row pitch of an hc plane (oa_plan_kpitch)"""
    return nx // 2 + 16


def steps():
    """(step_y, step_x) of FlatGeometry.from_res(shape, RES_ARCMIN): x decreasing"""
    r = RES_ARCMIN * np.pi / 180. / 60.
    return r, -r


def index_plane_hc(ny, nx, kp, prec, real=False):
    """an hc plane whose values encode their own index (exact in float32 up to 512 x 512), 1e6 on the padding columns"""
    y, x = np.mgrid[0:ny, 0:kp]
    v = (y + 1 + 1000.0 * x) if real else (y + 1 + 1000.0 * x) + 1j * (0.5 + x + 1000.0 * y)
    v = v.astype(RDT[prec] if real else CDT[prec])
    v[:, nx // 2 + 1:] = 1e6
    return v


def index_plane_full(ny, nx, prec, real=False):
    y, x = np.mgrid[0:ny, 0:nx]
    v = (y + 1 + 1000.0 * x) if real else (y + 1 + 1000.0 * x) + 1j * (0.5 + x + 1000.0 * y)
    return v.astype(RDT[prec] if real else CDT[prec])


def laxes(ny, nx, step_y, step_x, prec):
    """ly, lx as the plan stores them (float64 axes rounded to the plan's precision) and the derivative axes (Nyquist entry zero)"""
    ly = (np.fft.fftfreq(ny, step_y) * 2 * np.pi).astype(RDT[prec])
    lx = (np.fft.fftfreq(nx, step_x) * 2 * np.pi).astype(RDT[prec])
    lyd, lxd = ly.copy(), lx.copy()
    lyd[ny // 2] = 0
    lxd[nx // 2] = 0
    return ly, lx, lyd, lxd


def legs_inputs(seed, ny, nx, kp, prec):
    rng = np.random.default_rng([seed, ny, nx])
    d = dict(kX=mixed_complex(rng, (ny, kp), prec), kY=mixed_complex(rng, (ny, kp), prec), FG=mixed_real(rng, (ny, kp), prec),
             FH=mixed_real(rng, (ny, kp), prec), Fn=mixed_real(rng, (ny, kp), prec), out0=mixed_complex(rng, (ny, kp), prec))
    for v in d.values():
        v[:, nx // 2 + 1:] = 1e6          # the padding must never be read into a valid column
    return d


def split_alpha(seed, shape, step, prec, qmax=40.0):
    """displacements whose longdouble quotient by the (rounded) step stays 2^-10 away from every half-integer: the nearest-pixel
    shift is then the same in float32, float64 and longdouble (|q| u_32 < 2^-18)"""
    rng = np.random.default_rng([seed, shape[0], shape[1]])
    st = LD(RDT[prec](step))
    a = (rng.uniform(-qmax, qmax, shape) * float(st)).astype(RDT[prec])
    for _ in range(64):
        q = a.astype(LD) / st
        near = np.abs(np.abs(q - np.floor(q)) - LD(0.5)) < LD(2.0) ** -10
        if not near.any():
            return a
        a[near] = (rng.uniform(-qmax, qmax, int(near.sum())) * float(st)).astype(RDT[prec])
    raise AssertionError("split_alpha: no draw clear of the ties")


def white_map(seed, ny, nx, prec):
    return np.random.default_rng([seed, ny, nx]).standard_normal((ny, nx)).astype(RDT[prec])


def gather_inputs(seed, ny, nx, prec):
    """a white map, shifts from [-(3 n + 1), 3 n + 1] per axis (they wrap the map up to three times in either sign) with the exact
    multiples 0, +-n, +-2 n, +-3 n and the ends of the range first, remainders within half a pixel, a pre-filled output"""
    rng = np.random.default_rng([seed, ny, nx, 1])
    sty, stx = steps()

    def shifts(n):
        s = rng.integers(-(3 * n + 1), 3 * n + 2, (ny, nx)).astype(np.int32)
        edge = np.array([0, n, -n, 2 * n, -2 * n, 3 * n, -3 * n, 3 * n + 1, -(3 * n + 1), n - 1, 1 - n, -1, 1], dtype=np.int32)
        s.reshape(-1)[:edge.size] = edge
        s.reshape(-1)[-edge.size:] = edge[::-1]
        return s
    return dict(src=white_map(seed, ny, nx, prec), sx=shifts(nx), sy=shifts(ny),
                dx=(rng.uniform(-0.5, 0.5, (ny, nx)) * stx).astype(RDT[prec]), dy=(rng.uniform(-0.5, 0.5, (ny, nx)) * sty).astype(RDT[prec]),
                out0=mixed_real(rng, (ny, nx), prec))


def derivs_input(seed, ny, nx, prec):
    """an hc plane of mixed magnitudes, 1e6 on the padding (the input of the oa_hc_derivs tests)"""
    hc = mixed_complex(np.random.default_rng([seed, ny, nx, 2]), (ny, kpitch(nx)), prec)
    hc[:, nx // 2 + 1:] = 1e6
    return hc


def gather_out0(g, px, py, prec):
    """the pre-filled plane of an accumulating gather, scaled to the size of the term (step^(px + py)): a plane of order one would
    hide a wrong term of a high power inside its own rounding"""
    return (g["out0"].astype(np.float64) * abs(steps()[0]) ** (px + py)).astype(RDT[prec])


GATHER_CASES = [(0, 0, 1.0), (1, 0, -1.0), (0, 1, 0.5), (1, 1, -0.37), (2, 0, 0.5), (0, 2, -0.5), (2, 1, 0.37), (3, 0, 1.0 / 6), (3, 2, -1.0 / 12)]


def real_derivs_fft(imap, order):
    """float64 FFT form of :func:`real_derivs` on the axes of :func:`steps` (inputs of the oa_lens_taylor tests; the check of
    real_derivs)"""
    ny, nx = imap.shape
    _, _, lyd, lxd = laxes(ny, nx, *steps(), "f64")
    k = np.fft.fft2(np.asarray(imap, dtype=np.float64))
    planes = [None] * (order * (order + 1) // 2 - 1)
    for n in range(1, order):
        for b in range(n + 1):
            a = n - b
            planes[plane_index(a, b)] = np.fft.ifft2(k * (1j * lxd[None, :]) ** a * (1j * lyd[:, None]) ** b).real
    return planes


def taylor_inputs(seed, ny, nx, prec):
    """a white map, its 35 derivative planes for order 8 (plane_index order: the first order (order + 1) / 2 - 1 serve a lower
    order), a deflection of up to 2.5 pixels split by :func:`lens_split`, everything stored in the plane's precision"""
    src = white_map(seed, ny, nx, prec)
    sty, stx = steps()
    T = RDT[prec]
    planes = np.stack([p.astype(T) for p in real_derivs_fft(src, 8)])
    ay = split_alpha(seed + 1, (ny, nx), sty, prec, qmax=2.5)
    ax = split_alpha(seed + 2, (ny, nx), stx, prec, qmax=2.5)
    sy, dy = lens_split(ay, sty, prec)
    sx, dx = lens_split(ax, stx, prec)
    return dict(src=src, planes=planes, ax=ax, ay=ay, sx=sx.astype(np.int32), sy=sy.astype(np.int32), dx=dx.ref.astype(T), dy=dy.ref.astype(T))


# ---- flat kernels ----------------------------------------------------------------------------------------------------------------------
def f2power(k1, k2, norm, prec):
    a, b, nm = ld(k1), ld(k2), LD(RDT[prec](norm))
    t1, t2 = a.real * b.real, a.imag * b.imag
    return Ref((t1 + t2) * nm, (np.abs(t1) + np.abs(t2)) * np.abs(nm))


def cmul_real(k, f):
    """single rounding per component: the result in the operands' own precision"""
    k, f = np.asarray(k), np.asarray(f)
    out = np.empty_like(k)
    out.real, out.imag = k.real * f, k.imag * f
    return out


def cmul(k, f):
    a, b = ld(k), ld(f)
    rr, ii, ri, ir = a.real * b.real, a.imag * b.imag, a.real * b.imag, a.imag * b.real
    return Ref(cpack(rr - ii, ri + ir), cpack(np.abs(rr) + np.abs(ii), np.abs(ri) + np.abs(ir)))


def mul_real(a, b):
    return np.asarray(a) * np.asarray(b)


def axpby(a, b, alpha, beta, prec):
    t1, t2 = LD(RDT[prec](alpha)) * ld(a), LD(RDT[prec](beta)) * ld(b)
    return Ref(t1 + t2, np.abs(t1) + np.abs(t2))


def rot2(c, s, i1, i2, sign=1):
    """[o1; o2] = [[c, -s], [s, c]] [i1; i2]; returns (Ref o1, Ref o2).  sign = -1: the wrong rotation of the bite tests"""
    c, s, a, b = ld(c), LD(sign) * ld(s), ld(i1), ld(i2)

    def comb(p, q, sg):
        return Ref(cpack(p.real + sg * q.real, p.imag + sg * q.imag), cpack(np.abs(p.real) + np.abs(q.real), np.abs(p.imag) + np.abs(q.imag)))
    ac, bs, as_, bc = a * c, b * s, a * s, b * c
    return comb(ac, bs, -1), comb(as_, bc, 1)


# ---- layouts (index maps only: exact in any dtype) ------------------------------------------------------------------------------------------
def hc_to_full(hc, nx, conj=True):
    ny = hc.shape[0]
    y, x = np.mgrid[0:ny, 0:nx]
    low = x <= nx // 2
    src = hc[np.where(low, y, (ny - y) % ny), np.where(low, x, nx - x)]
    if conj and np.iscomplexobj(hc):
        src = np.where(low, src, np.conj(src))
    return src


def full_to_hc(full, kp, fill):
    """the valid columns 0 .. nx/2; the padding keeps ``fill`` (the entry does not write it)"""
    ny, nx = full.shape
    out = np.array(fill, dtype=full.dtype, copy=True)
    assert out.shape == (ny, kp)
    out[:, :nx // 2 + 1] = full[:, :nx // 2 + 1]
    return out


def hcreal_to_full(hc, nx):
    return hc_to_full(hc, nx, conj=False)


def fullreal_to_hc(full, kp):
    ny, nx = full.shape
    out = np.zeros((ny, kp), dtype=full.dtype)
    out[:, :nx // 2 + 1] = full[:, :nx // 2 + 1]
    return out


# ---- legs and divergence -----------------------------------------------------------------------------------------------------------------
def phase(lx, ly, sgn):
    """e^{sgn 2 i psi}, psi = atan2(-lx, ly) on the (ny, len(lx)) grid; 1 at l = 0"""
    LX, LY = np.meshgrid(ld(lx), ld(ly))
    psi = np.arctan2(-LX, LY)
    p = cpack(np.cos(2 * psi), LD(sgn) * np.sin(2 * psi))
    p[(LX == 0) & (LY == 0)] = 1
    return p


def qe_legs(kX, kY, FG, FH, ly, lx, lyd, lxd, nx, phase_g=0, phase_h=0, h_times_i=False):
    """(Gx, Gy, H) as Refs on the valid columns 0 .. nx/2 of the (ny, kp) planes.  ``lxd`` / ``lyd`` multiply the gradient; pass
    lx / ly there for the wrong form of the bite tests."""
    w = nx // 2 + 1
    kx, ky, fg, fh = ld(kX)[:, :w], ld(kY)[:, :w], ld(FG)[:, :w], ld(FH)[:, :w]
    lxw, lxdw = np.asarray(lx)[:w], ld(lxd)[None, :w]
    lydc = ld(lyd)[:, None]

    def leg(k, f, ph):
        g = k * f
        if not ph:
            return g, cpack(np.abs(g.real), np.abs(g.imag))
        m = np.abs(g.real) + np.abs(g.imag)
        return g * phase(lxw, ly, ph), cpack(m, m)
    g, Ag = leg(kx, fg, phase_g)
    h, Ah = leg(ky, fh, phase_h)
    if h_times_i:
        h, Ah = h * CLD(1j), cpack(Ah.imag, Ah.real)
    ig, Aig = g * CLD(1j), cpack(Ag.imag, Ag.real)
    return (Ref(ig * lxdw, cpack(Aig.real * np.abs(lxdw), Aig.imag * np.abs(lxdw))),
            Ref(ig * lydc, cpack(Aig.real * np.abs(lydc), Aig.imag * np.abs(lydc))), Ref(h, Ah))


def qe_div(Px, Py, Fn, lyd, lxd, nx, out0=None):
    """Fnorm (i lx Px + i ly Py) on the derivative axes, plus ``out0`` when accumulating"""
    w = nx // 2 + 1
    px, py, fn = ld(Px)[:, :w], ld(Py)[:, :w], ld(Fn)[:, :w]
    tx, ty = px * ld(lxd)[None, :w], py * ld(lyd)[:, None]
    d = (tx + ty) * CLD(1j) * fn
    A = cpack((np.abs(tx.imag) + np.abs(ty.imag)) * np.abs(fn), (np.abs(tx.real) + np.abs(ty.real)) * np.abs(fn))
    if out0 is not None:
        o = ld(out0)[:, :w]
        d, A = d + o, cpack(A.real + np.abs(o.real), A.imag + np.abs(o.imag))
    return Ref(d, A)


# ---- flat-sky lensing operator ----------------------------------------------------------------------------------------------------------------
def lens_split(alpha, step, prec):
    """(shift int64, Ref delta): shift = rint(alpha / step) (ties to even), delta = alpha - shift step, step rounded to T"""
    a, st = ld(alpha), LD(RDT[prec](step))
    r = np.rint(a / st)
    return r.astype(np.int64), Ref(a - r * st, np.abs(a) + np.abs(r * st))


def gather_index(sy, sx):
    ny, nx = sy.shape
    iy, ix = np.mgrid[0:ny, 0:nx]
    return (iy + np.asarray(sy, dtype=np.int64)) % ny, (ix + np.asarray(sx, dtype=np.int64)) % nx


def lens_gather(src, sx, sy, dx, dy, px, py, coef, prec, out0=None):
    yy, xx = gather_index(sy, sx)
    v = LD(RDT[prec](coef)) * ld(src)[yy, xx] * ld(dx) ** px * ld(dy) ** py
    if out0 is None:
        return Ref(v, np.abs(v))
    return Ref(ld(out0) + v, np.abs(ld(out0)) + np.abs(v))


def plane_index(a, b):
    n = a + b
    return n * (n + 1) // 2 - 1 + b


def hc_derivs(k, lyd, lxd, nx, order):
    """{(a, b): Ref of (i lx)^a (i ly)^b k on the valid columns} for 1 <= a + b < order"""
    w = nx // 2 + 1
    kk, lxw, lyc = ld(k)[:, :w], ld(lxd)[None, :w], ld(lyd)[:, None]
    out = {}
    for n in range(1, order):
        for b in range(n + 1):
            a = n - b
            m = lxw ** a * lyc ** b
            v = kk * I_POW[n % 4] * m
            out[(a, b)] = Ref(v, cpack(np.abs(v.real), np.abs(v.imag)))
    return out


def lens_taylor(src, planes, sx, sy, dx, dy, order, drop=None):
    """sum_{a + b < order} dx^a dy^b / (a! b!) D_ab[(y + sy) % ny, (x + sx) % nx], D_00 = src, D_ab = planes[plane_index(a, b)].
    drop = (a, b): that term left out (the wrong form of the bite tests)"""
    yy, xx = gather_index(sy, sx)
    ddx, ddy = ld(dx), ld(dy)
    ref = ld(src)[yy, xx].copy()
    A = np.abs(ref)
    for n in range(1, order):
        for b in range(n + 1):
            a = n - b
            if drop == (a, b):
                continue
            t = ld(planes[plane_index(a, b)])[yy, xx] * (ddx ** a / LD(factorial(a))) * (ddy ** b / LD(factorial(b)))
            ref = ref + t
            A = A + np.abs(t)
    return Ref(ref, A)


def dft_matrix(n, inverse=False):
    jk = np.outer(np.arange(n), np.arange(n)) % n
    ang = (LD(2) * PI / LD(n)) * jk.astype(LD)
    return cpack(np.cos(ang), (1 if inverse else -1) * np.sin(ang))


def real_derivs(imap, step_y, step_x, order, prec="f64"):
    """the real derivative planes of a map, [plane_index(a, b)] = IDFT[(i lx)^a (i ly)^b DFT(map)] / (ny nx), by longdouble DFT
    matrices (small maps only) on the axes as a plan of precision ``prec`` stores them, the Nyquist entry zeroed (the conventions of
    qe_oracle.flat_taylens)"""
    ny, nx = imap.shape
    _, _, lyd, lxd = laxes(ny, nx, step_y, step_x, prec)
    Wy, Wx, Vy, Vx = dft_matrix(ny), dft_matrix(nx), dft_matrix(ny, True), dft_matrix(nx, True)
    k = Wy @ ld(imap).astype(CLD) @ Wx.T
    planes = [None] * (order * (order + 1) // 2 - 1)
    for n in range(1, order):
        for b in range(n + 1):
            a = n - b
            s = k * I_POW[n % 4] * (ld(lxd)[None, :] ** a * ld(lyd)[:, None] ** b)
            planes[plane_index(a, b)] = (Vy @ s @ Vx.T).real / LD(ny * nx)
    return planes


def flat_taylens(imap, sx, sy, dx, dy, step_y, step_x, order, prec="f64"):
    """the whole operator from a map and an already split deflection: (Ref, planes)"""
    planes = real_derivs(imap, step_y, step_x, order, prec)
    return lens_taylor(imap, planes, sx, sy, dx, dy, order), planes
