"""NumPy statement of what a Gaussian draw of ``orphics_amd/csrc/rng.hip`` IS.

TEST INFRASTRUCTURE ONLY, written from the header contract (``include/orphics_amd.h``: "Counter-based Philox4x32-10,
key = (seed, stream_id)") and the published definition of Philox (Salmon, Moraes, Dror & Shaw, SC'11; the Random123
known-answer vectors pin :func:`philox4x32_10` in ``tests/test_rng_oracle_cpu.py``).  It imports nothing from ``orphics_amd``.

A draw, in words:

* four 32-bit words per counter: ``philox4x32_10((idx lo, idx hi, stream lo, stream hi), (seed lo, seed hi))``;
* the words pair as (x, y) and (z, w); per pair ``u = (float32(word) + 0.5f) * 2^-32`` in float32 (exact IEEE operations, so
  NumPy reproduces the uniforms bit for bit), then Box-Muller ``r = sqrt(-2 ln u1)``, ``n0 = r cos(2 pi u2)``,
  ``n1 = r sin(2 pi u2)``.  The kernels evaluate these in float32 (``logf``, ``sqrtf``, ``sincospif``); the oracle evaluates
  them in float64 from the same float32 uniforms, so the two differ by the float32 error of those functions alone;
* ``randn``: element ``4 i + j`` is normal ``j`` of counter ``i``;
* the half plane ``(ny, nx/2 + 1)``: column ``x`` belongs to the column pair ``p = x // 2``, slot ``j = x % 2``, counter
  ``ys * npair + p`` with ``npair = (nx/2)/2 + 1``; ``(re, im) = (n[2j], n[2j+1]) / sqrt 2``.  On the self-conjugate columns
  ``x in {0, nx/2}`` the rows ``y > ny/2`` take ``ys = ny - y`` and are conjugated (everywhere else ``ys = y``), and at
  ``ys in {0, ny/2}`` the mode is real: ``re = n[2j]``, ``im = 0``.

ERROR MODEL (:func:`normal_bound`, used by every GPU comparison).  ``logf``, ``sqrtf`` and ``sincospif`` are each taken as
within 2 ulp, and two float32 roundings of products are added:
``n = r * c`` with ``r = sqrtf(-2 * logf(u))``.  In units of 2^-23: r carries (2 [logf] + 0.5 [the product -2 * l, counted
although a power of two is exact]) / 2 [the square root halves a relative error] + 2 [sqrtf] = 3.25, c carries 2 of 1 >= |c|, the
product r * c rounds once more (0.5): at most ``5.75 * 2^-23 * r ~ 6.9e-7 r``.  The bound used is ``1e-6 * max(1, r)`` per
normal; the floor of 1 covers logf's absolute error where u1 is near 1 and r is small.  A wrong word, counter or branch is off
by O(1).  Scale factors (1 / sqrt 2, covsqrt, mix coefficients) propagate linearly; the plan's own roundings of the products
and sums behind the normals add ``4 * eps`` of the sum of the absolute values of the terms, eps = 2^-24 (float32 plans) or
2^-53 (float64 plans: negligible, kept for symmetry).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
NORMAL_TOL = 1e-6
ROUNDINGS = 4
PLAN_EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(ctr4, key2):
    """Philox4x32 with 10 rounds.  ``ctr4``: four, ``key2``: two broadcastable uint64 arrays holding 32-bit words;
    returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.array(np.broadcast_arrays(*[_u64(c) & M32 for c in ctr4])[i]) for i in range(4))
    k0, k1 = _u64(key2[0]) & M32, _u64(key2[1]) & M32
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> s, p0 & M32, p1 >> s, p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniform01(word):
    """(0, 1] float32 uniform of a 32-bit word, with the float32 operations of the kernel."""
    f = _u64(word).astype(np.uint32).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def box_muller(a, b):
    """two normals (float64) and their radius from two 32-bit words"""
    u1, u2 = uniform01(a), uniform01(b)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    t = 2.0 * u2.astype(np.float64)
    return r * np.cos(np.pi * t), r * np.sin(np.pi * t), r


def normals4(seed, stream_id, idx):
    """The four normals of counter ``idx`` (array) of stream (seed, stream_id): ``(n, r)``, float64 arrays of shape
    ``idx.shape + (4,)``; ``r[..., k]`` is the Box-Muller radius behind ``n[..., k]``."""
    seed, sid = int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1)
    idx = _u64(idx)
    s = np.uint64(32)
    w = philox4x32_10((idx & M32, idx >> s, np.uint64(sid & 0xFFFFFFFF), np.uint64(sid >> 32)),
                      (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))
    n0, n1, ra = box_muller(w[0], w[1])
    n2, n3, rb = box_muller(w[2], w[3])
    return np.stack([n0, n1, n2, n3], axis=-1), np.stack([ra, ra, rb, rb], axis=-1)


def normal_bound(r):
    """float32 evaluation error allowed per normal of radius r (module docstring)"""
    return NORMAL_TOL * np.maximum(1.0, r)


def randn(seed, stream_id, n, with_bound=False):
    n = int(n)
    v, r = normals4(seed, stream_id, np.arange((n + 3) // 4, dtype=np.uint64))
    v, r = v.reshape(-1)[:n], r.reshape(-1)[:n]
    return (v, normal_bound(r)) if with_bound else v


def hc_counters(ny, nx):
    """(counter, slot, mirrored) of every mode of the (ny, nx/2 + 1) half plane"""
    nxh = nx // 2
    npair = nxh // 2 + 1
    y, x = np.meshgrid(np.arange(ny), np.arange(nxh + 1), indexing="ij")
    edge = (x == 0) | (x == nxh)
    mirrored = edge & (y > ny // 2)
    ys = np.where(mirrored, ny - y, y)
    ctr = ys.astype(np.uint64) * np.uint64(npair) + (x // 2).astype(np.uint64)
    return ctr, x % 2, mirrored


def white_hc(ny, nx, seed, stream_id):
    """Unit white Hermitian-consistent field on the half plane: ``(w complex128, e float64)``; ``e`` bounds the error of the real
    and of the imaginary part of a float32 evaluation of the normals."""
    nxh = nx // 2
    ctr, slot, mirrored = hc_counters(ny, nx)
    uniq, inv = np.unique(ctr, return_inverse=True)
    n, r = normals4(seed, stream_id, uniq)
    n, r = n[inv.reshape(ctr.shape)], r[inv.reshape(ctr.shape)]
    re = np.take_along_axis(n, (2 * slot)[..., None], -1)[..., 0]
    im = np.take_along_axis(n, (2 * slot + 1)[..., None], -1)[..., 0]
    e = normal_bound(np.take_along_axis(r, (2 * slot)[..., None], -1)[..., 0])
    y, x = np.meshgrid(np.arange(ny), np.arange(nxh + 1), indexing="ij")
    real_mode = ((x == 0) | (x == nxh)) & ((y == 0) | (2 * y == ny))
    rs2 = np.where(real_mode, 1.0, np.sqrt(0.5))
    re, im, e = re * rs2, np.where(real_mode, 0.0, im * rs2), e * rs2
    im = np.where(mirrored, -im, im)
    return re + 1j * im, e


def _parts(z):
    return np.stack([np.abs(z.real), np.abs(z.imag)], axis=-1)


def grf_hc(ny, nx, seed, stream_id, covsqrt=None, with_bound=False, prec="f64"):
    """``oa_grf_hc`` on the (ny, nx/2 + 1) grid.  ``with_bound``: also the allowed |error| of (re, im), shape + (2,)."""
    w, e = white_hc(ny, nx, seed, stream_id)
    if covsqrt is not None:
        cs = np.asarray(covsqrt, dtype=np.float64)
        w, e = w * cs, e * np.abs(cs)
    if not with_bound:
        return w
    return w, e[..., None] + ROUNDINGS * PLAN_EPS[prec] * _parts(w)


def rot2(p, q, c, s):
    """oa_rot2's convention: (p c - q s, p s + q c)"""
    return p * c - q * s, p * s + q * c


def grf_mix(ny, nx, seed, stream_id0, covsqrt, rot=None, inputs=None, filt=None, scale=1.0, with_bound=False, prec="f64"):
    """``oa_grf_mix``: white fields of streams stream_id0 + c mixed by the n x n table ``covsqrt`` (None = zero block), rotated on
    components 1, 2; without inputs ``scale * rot(v)``, with inputs ``rot(in * filt) + scale * v``.  Returns the list of planes
    (and, ``with_bound``, the list of allowed |error| of (re, im))."""
    n = len(covsqrt)
    ws = [white_hc(ny, nx, seed, (int(stream_id0) + c) & (2 ** 64 - 1)) for c in range(n)]
    shape = ws[0][0].shape
    v, ev, av = [], [], []                       # value, normal-error bound, sum of |terms| per (re, im)
    for i in range(n):
        vi, ei, ai = np.zeros(shape, complex), np.zeros(shape), np.zeros(shape + (2,))
        for j in range(n):
            if covsqrt[i][j] is None:
                continue
            cs = np.asarray(covsqrt[i][j], dtype=np.float64)
            vi, ei, ai = vi + cs * ws[j][0], ei + np.abs(cs) * ws[j][1], ai + _parts(cs * ws[j][0])
        v.append(vi); ev.append(ei); av.append(ai)

    def rotate(z, e, a):
        if rot is None:
            return z, e, a
        c, s = (np.asarray(t, dtype=np.float64) for t in rot)
        ac, as_ = np.abs(c), np.abs(s)
        z1, z2 = rot2(z[1], z[2], c, s)
        return ([z[0], z1, z2], [e[0], ac * e[1] + as_ * e[2], as_ * e[1] + ac * e[2]],
                [a[0], ac[..., None] * a[1] + as_[..., None] * a[2], as_[..., None] * a[1] + ac[..., None] * a[2]])

    sc = abs(float(scale))
    if inputs is None:
        v, ev, av = rotate(v, ev, av)
        out, eo, ao = [float(scale) * z for z in v], [sc * e for e in ev], [sc * a for a in av]
    else:
        f = 1.0 if filt is None else np.asarray(filt, dtype=np.float64)
        u = [np.asarray(k, dtype=np.complex128) * f for k in inputs]
        u, eu, au = rotate(u, [np.zeros(shape) for _ in u], [_parts(k) for k in u])
        out = [u[i] + float(scale) * v[i] for i in range(n)]
        eo = [eu[i] + sc * ev[i] for i in range(n)]
        ao = [au[i] + sc * av[i] for i in range(n)]
    if not with_bound:
        return out
    return out, [eo[i][..., None] + ROUNDINGS * PLAN_EPS[prec] * ao[i] for i in range(n)]


def hermitian_expand(hc, nx):
    """full (ny, nx) plane of a half plane (ny, nx/2 + 1): F[y, x] = conj(F[-y, -x])"""
    ny, nxh = hc.shape[0], nx // 2
    full = np.empty((ny, nx), dtype=np.complex128)
    full[:, :nxh + 1] = hc
    x = np.arange(nxh + 1, nx)
    full[:, nxh + 1:] = np.conj(hc[(-np.arange(ny)) % ny][:, nx - x])
    return full


def _as_parts(z):
    z = np.asarray(z)
    if np.iscomplexobj(z):
        return np.stack([z.real, z.imag], axis=-1).astype(np.float64)
    return z.astype(np.float64)


def draw_ratios(got, ref, bound):
    """|got - ref| / bound per real number (complex arrays: per real and imaginary part, trailing axis 2; ``bound`` has either
    that shape or the shape of the complex array).  A zero bound demands equality: ratio 0 or inf.  NaN counts as inf."""
    g, r = _as_parts(got), _as_parts(ref)
    if g.shape != r.shape:
        raise ValueError("draw_ratios: shapes %s and %s differ" % (g.shape, r.shape))
    b = np.asarray(bound, dtype=np.float64)
    if np.iscomplexobj(np.asarray(got)) and b.ndim == g.ndim - 1:
        b = b[..., None]
    b = np.broadcast_to(b, g.shape)
    if np.any(b < 0) or np.any(np.isnan(b)):
        raise ValueError("draw_ratios: bounds must be non-negative numbers")
    d = np.abs(g - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d == 0, 0.0, np.inf))
    return np.where(np.isnan(q), np.inf, q)


def draw_mismatch(got, ref, bound):
    """The worst |got - ref| / bound: the comparison is met when this is <= 1."""
    q = draw_ratios(got, ref, bound)
    return float(q.max()) if q.size else 0.0
