"""CPU: oracle/ew_oracle.py -- the longdouble restatement that tests/test_elementwise_reference_gpu.py holds the kernels of
csrc/elementwise.hip against -- checked here against independent NumPy forms (np.fft expansions for the layouts, np.roll for constant
shifts, qe_oracle.flat_taylens for the Taylor sum), and its error bounds shown to BITE on the GPU tests' own inputs: for every bounded
kernel a step-by-step evaluation in the plane's precision (float32 / float64, every operation rounded) stays inside
1.01 c u_T A per element, and a wrong evaluation leaves it on at least one element."""
import numpy as np
import pytest

from oracle import ew_oracle as eo
from oracle import qe_oracle as qo

LD = np.longdouble
PRECS = ["f32", "f64"]
SMALL = [(32, 64), (36, 40), (64, 32)]


def inside(got, R, c, prec):
    return eo.violations(got, R, c, prec).size == 0


# ---- the oracle against independent forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx", eo.SHAPES_POW2[:3] + eo.SHAPES_MIXED[:1] + [eo.SHAPE_CZT])
def test_layouts_against_fft_expansions(ny, nx):
    rng = np.random.default_rng(1)
    kp, w = eo.kpitch(nx), nx // 2 + 1
    x = rng.standard_normal((ny, nx))
    full, half = np.fft.fft2(x), np.fft.rfft2(x)
    hc = np.full((ny, kp), 1e6 + 0j)
    hc[:, :w] = half
    scale = np.abs(full).max()
    assert np.abs(eo.hc_to_full(hc, nx) - full).max() < 1e-13 * scale          # what the C2C of a real map holds
    assert np.array_equal(eo.full_to_hc(full, kp, hc)[:, :w], full[:, :w]) and np.all(eo.full_to_hc(full, kp, hc)[:, w:] == 1e6)
    # an exactly Hermitian plane (z + conj z(-l)) comes back bit for bit from its half
    z = rng.standard_normal((ny, nx)) + 1j * rng.standard_normal((ny, nx))
    herm = z + np.conj(np.roll(z[::-1, ::-1], (1, 1), axis=(0, 1)))
    hc[:, :w] = herm[:, :w]
    assert np.array_equal(eo.hc_to_full(hc, nx), herm)
    assert not np.array_equal(eo.hc_to_full(hc, nx, conj=False), herm)
    # real even-symmetric planes: the transform of a real even map
    ev = x + np.roll(x[::-1, ::-1], (1, 1), axis=(0, 1))
    hr = np.full((ny, kp), 1e6)
    hr[:, :w] = ev[:, :w]
    assert np.array_equal(eo.hcreal_to_full(hr, nx), ev)
    back = eo.fullreal_to_hc(ev, kp)
    assert np.array_equal(back[:, :w], ev[:, :w]) and np.all(back[:, w:] == 0)
    # the marked rows and columns: row 0 and ny/2 map onto themselves, column nx/2 is its own mirror
    f = eo.hc_to_full(eo.index_plane_hc(ny, nx, kp, "f64"), nx)
    ih = eo.index_plane_hc(ny, nx, kp, "f64")
    assert np.array_equal(f[0, w:], np.conj(ih[0, 1:nx // 2][::-1])) and np.array_equal(f[ny // 2, w:], np.conj(ih[ny // 2, 1:nx // 2][::-1]))
    assert np.array_equal(f[1, w:], np.conj(ih[ny - 1, 1:nx // 2][::-1])) and np.array_equal(f[:, :w], ih[:, :w])


def test_flat_refs_against_numpy():
    d = eo.flat_inputs(eo.SEED, 1027, "f64")
    assert np.allclose(eo.f2power(d["k1"], d["k2"], eo.NORM, "f64").ref.astype(float), np.real(np.conj(d["k1"]) * d["k2"]) * eo.NORM, rtol=0,
                       atol=1e-15 * float(eo.f2power(d["k1"], d["k2"], eo.NORM, "f64").A.max()))
    R = eo.cmul(d["k1"], d["k2"])
    assert np.abs(R.ref.astype(complex) - d["k1"] * d["k2"]).max() <= 4e-16 * float(max(R.A.real.max(), R.A.imag.max()))
    assert np.array_equal(eo.cmul_real(d["k1"], d["f"]), d["k1"] * d["f"])
    R = eo.axpby(d["a"], d["b"], eo.ALPHA, eo.BETA, "f64")
    assert np.abs(R.ref.astype(float) - (eo.ALPHA * d["a"] + eo.BETA * d["b"])).max() <= 4e-16 * float(R.A.max())
    o1, o2 = eo.rot2(d["c"], d["s"], d["k1"], d["k2"])
    assert np.abs(o1.ref.astype(complex) - (d["k1"] * d["c"] - d["k2"] * d["s"])).max() <= 4e-16 * float(o1.A.real.max() + o1.A.imag.max())
    assert np.abs(o2.ref.astype(complex) - (d["k1"] * d["s"] + d["k2"] * d["c"])).max() <= 4e-16 * float(o2.A.real.max() + o2.A.imag.max())


def test_phase_and_legs_against_closed_forms():
    ny, nx = 36, 40
    ly, lx, lyd, lxd = eo.laxes(ny, nx, *eo.steps(), "f64")
    p = eo.phase(lx, ly, +1).astype(complex)
    LX, LY = np.meshgrid(lx, ly)
    with np.errstate(invalid="ignore", divide="ignore"):
        closed = ((LY - 1j * LX) / np.hypot(LX, LY)) ** 2          # e^{i psi} = (ly - i lx) / l
    closed[0, 0] = 1
    assert np.abs(p - closed).max() < 1e-15 and p[0, 0] == 1
    assert np.abs(eo.phase(lx, ly, -1).astype(complex) - np.conj(closed)).max() < 1e-15
    kp = eo.kpitch(nx)
    d = eo.legs_inputs(eo.SEED, ny, nx, kp, "f64")
    w = nx // 2 + 1
    Gx, Gy, H = eo.qe_legs(d["kX"], d["kY"], d["FG"], d["FH"], ly, lx, lyd, lxd, nx, phase_g=1, phase_h=-1, h_times_i=True)
    g = d["kX"][:, :w] * d["FG"][:, :w] * closed[:, :w]
    assert np.abs(Gx.ref.astype(complex) - 1j * lxd[None, :w] * g).max() <= 1e-14 * float(Gx.A.real.max())
    assert np.abs(Gy.ref.astype(complex) - 1j * lyd[:, None] * g).max() <= 1e-14 * float(Gy.A.real.max())
    assert np.abs(H.ref.astype(complex) - 1j * d["kY"][:, :w] * d["FH"][:, :w] * np.conj(closed[:, :w])).max() <= 1e-14 * float(H.A.real.max())
    assert np.all(Gx.ref[:, nx // 2] == 0) and np.all(Gy.ref[ny // 2] == 0) and np.all(H.ref[:, nx // 2] != 0) and np.all(H.ref[ny // 2] != 0)
    D = eo.qe_div(d["kX"], d["kY"], d["Fn"], lyd, lxd, nx, out0=d["out0"])
    direct = d["out0"][:, :w] + d["Fn"][:, :w] * (1j * lxd[None, :w] * d["kX"][:, :w] + 1j * lyd[:, None] * d["kY"][:, :w])
    assert np.abs(D.ref.astype(complex) - direct).max() <= 1e-14 * float(max(D.A.real.max(), D.A.imag.max()))


@pytest.mark.parametrize("ny,nx", SMALL)
def test_lensing_refs_against_roll_and_flat_taylens(ny, nx):
    sty, stx = eo.steps()
    t = eo.taylor_inputs(eo.SEED, ny, nx, "f64")
    # a constant shift is np.roll, whatever multiple of the side is added
    for s_y, s_x in [(1, -2), (ny + 1, -2 - 3 * nx), (-ny, nx), (0, 0)]:
        R = eo.lens_gather(t["src"], np.full((ny, nx), s_x), np.full((ny, nx), s_y), t["dx"], t["dy"], 0, 0, 1.0, "f64")
        assert np.array_equal(R.ref.astype(float), np.roll(t["src"], (-(s_y % ny), -(s_x % nx)), axis=(0, 1)))
    # the split and the Taylor sum: qe_oracle.flat_taylens restates the whole operator in float64
    sy, dy = eo.lens_split(t["ay"], sty, "f64")
    sx, dx = eo.lens_split(t["ax"], stx, "f64")
    assert np.array_equal(sy, np.rint(t["ay"] / sty).astype(int)) and np.array_equal(sx, np.rint(t["ax"] / stx).astype(int))
    assert np.abs(dx.ref.astype(float) - (t["ax"] - sx * stx)).max() <= 4e-16 * float(dx.A.max())
    assert sx.min() < 0 < sx.max() and sy.min() < 0 < sy.max()
    for order in (1, 2, 5, 8):
        R, planes = eo.flat_taylens(t["src"], sx, sy, dx.ref, dy.ref, sty, stx, order)
        ref = qo.flat_taylens((t["ay"], t["ax"]), t["src"], sty, stx, taylor_order=order)
        assert np.abs(R.ref.astype(float) - ref).max() <= 1e-12 * float(R.A.max()), order
        fast = eo.real_derivs_fft(t["src"], order)
        for a, b in zip(planes, fast):
            assert np.abs(a.astype(float) - b).max() <= 1e-12 * np.abs(b).max()
    # hc_derivs: plane n (n + 1) / 2 - 1 + b of the full-plane form, restricted to the half plane
    k = np.fft.fft2(t["src"])
    _, _, lyd, lxd = eo.laxes(ny, nx, sty, stx, "f64")
    kp = eo.kpitch(nx)
    hc = np.full((ny, kp), 1e6 + 0j)
    hc[:, :nx // 2 + 1] = k[:, :nx // 2 + 1]
    D = eo.hc_derivs(hc, lyd, lxd, nx, 8)
    assert sorted(eo.plane_index(a, b) for a, b in D) == list(range(35))
    for (a, b), R in D.items():
        full = (1j * lxd[None, :]) ** a * (1j * lyd[:, None]) ** b * k
        assert np.abs(R.ref.astype(complex) - full[:, :nx // 2 + 1]).max() <= 1e-13 * np.abs(full).max()
        if a:
            assert np.all(R.ref[:, nx // 2] == 0)
        if b:
            assert np.all(R.ref[ny // 2] == 0)


def test_split_ties_go_to_even():
    for step in (2.0 ** -11, -2.0 ** -11):
        m = np.array([-6, -5, -2, -1, 0, 1, 2, 5, 6, 1023, -1024], dtype=np.float64)
        alpha = (m + 0.5) * step
        sh, d = eo.lens_split(alpha.astype(np.float32), step, "f32")
        expect = np.where(m % 2 == 0, m, m + 1).astype(int)
        assert np.array_equal(sh, expect)
        assert np.array_equal(d.ref.astype(float), alpha - expect * step)


# ---- step-by-step evaluations in the plane's precision: inside the bound; wrong ones: outside ---------------------------------------------
def emu_f2power(k1, k2, norm, T):
    return (k1.real * k2.real + k1.imag * k2.imag) * T(norm)


def emu_cmul(a, b):
    out = np.empty_like(a)
    out.real, out.imag = a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real
    return out


def emu_cscale(a, s):
    out = np.empty_like(a)
    out.real, out.imag = a.real * s, a.imag * s
    return out


def emu_muli(a):
    out = np.empty_like(a)
    out.real, out.imag = -a.imag, a.real
    return out


def emu_phase(lx, ly, sgn, T, C):
    u, v = np.meshgrid(-lx, ly)
    r2 = u * u + v * v
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = T(1) / r2
        p = np.empty(r2.shape, dtype=C)
        p.real, p.imag = (v * v - u * u) * inv, T(sgn) * T(2) * u * v * inv
    p[r2 == 0] = 1
    return p


def emu_legs(d, ly, lx, gy_axis, gx_axis, nx, pg, ph, hi, prec):
    T, C, w = eo.RDT[prec], eo.CDT[prec], nx // 2 + 1
    g, h = emu_cscale(d["kX"][:, :w], d["FG"][:, :w]), emu_cscale(d["kY"][:, :w], d["FH"][:, :w])
    if pg:
        g = emu_cmul(g, emu_phase(lx[:w], ly, pg, T, C))
    if ph:
        h = emu_cmul(h, emu_phase(lx[:w], ly, ph, T, C))
    if hi:
        h = emu_muli(h)
    return emu_cscale(emu_muli(g), gx_axis[None, :w]), emu_cscale(emu_muli(g), gy_axis[:, None]), h


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [5, 1027])
def test_flat_bounds_bite(prec, n):
    T = eo.RDT[prec]
    d = eo.flat_inputs(eo.SEED, n, prec)
    R = eo.f2power(d["k1"], d["k2"], eo.NORM, prec)
    assert inside(emu_f2power(d["k1"], d["k2"], eo.NORM, T), R, eo.C_F2POWER, prec)
    assert not inside((d["k1"].real * d["k2"].real - d["k1"].imag * d["k2"].imag) * T(eo.NORM), R, eo.C_F2POWER, prec)      # Re(k1 k2)
    R = eo.cmul(d["k1"], d["k2"])
    assert inside(emu_cmul(d["k1"], d["k2"]), R, eo.C_CMUL, prec)
    assert not inside(emu_cmul(d["k1"], np.conj(d["k2"])), R, eo.C_CMUL, prec)
    R = eo.axpby(d["a"], d["b"], eo.ALPHA, eo.BETA, prec)
    assert inside(T(eo.ALPHA) * d["a"] + T(eo.BETA) * d["b"], R, eo.C_AXPBY, prec)
    assert not inside(T(eo.BETA) * d["a"] + T(eo.ALPHA) * d["b"], R, eo.C_AXPBY, prec)
    if prec == "f32":                                   # alpha not rounded as the entry rounds it: visible
        assert not inside((eo.ALPHA * d["a"].astype(np.float64) + eo.BETA * d["b"].astype(np.float64)) * (1 + 3e-7), R, eo.C_AXPBY, prec)
    o1, o2 = eo.rot2(d["c"], d["s"], d["k1"], d["k2"])

    def emu_rot(sign):
        s = T(sign) * d["s"]
        e1, e2 = np.empty_like(d["k1"]), np.empty_like(d["k1"])
        e1.real, e1.imag = d["k1"].real * d["c"] - d["k2"].real * s, d["k1"].imag * d["c"] - d["k2"].imag * s
        e2.real, e2.imag = d["k1"].real * s + d["k2"].real * d["c"], d["k1"].imag * s + d["k2"].imag * d["c"]
        return e1, e2
    e1, e2 = emu_rot(1)
    assert inside(e1, o1, eo.C_ROT2, prec) and inside(e2, o2, eo.C_ROT2, prec)
    w1, w2 = emu_rot(-1)                                # the sign of s flipped
    assert not inside(w1, o1, eo.C_ROT2, prec) and not inside(w2, o2, eo.C_ROT2, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", [(32, 64), (36, 40)])
def test_layout_errors_are_unmistakable(prec, ny, nx):
    """the layouts are exact, so anything wrong differs; with index-encoding planes: a missing conj, the row guard y -> ny - y
    without the wrap, the padding read instead of the mirror column"""
    kp = eo.kpitch(nx)
    hc = eo.index_plane_hc(ny, nx, kp, prec)
    good = eo.hc_to_full(hc, nx)
    assert not np.array_equal(eo.hc_to_full(hc, nx, conj=False), good)
    y, x = np.mgrid[0:ny, 0:nx]
    wrong_row = np.where(x <= nx // 2, hc[y, np.minimum(x, nx // 2)], np.conj(hc[(ny - 1 - y) % ny, (nx - x) % kp]))
    assert not np.array_equal(wrong_row, good)
    assert np.abs(good).max() < 1e6                       # no padding value reaches the full plane


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", [(32, 64), (36, 40)])
def test_legs_and_div_bounds_bite(prec, ny, nx):
    kp = eo.kpitch(nx)
    ly, lx, lyd, lxd = eo.laxes(ny, nx, *eo.steps(), prec)
    d = eo.legs_inputs(eo.SEED, ny, nx, kp, prec)
    w = nx // 2 + 1
    for pg in (0, 1, -1):
        for ph in (0, 1, -1):
            for hi in (False, True):
                Gx, Gy, H = eo.qe_legs(d["kX"], d["kY"], d["FG"], d["FH"], ly, lx, lyd, lxd, nx, pg, ph, hi)
                cg, ch = (eo.C_LEGS_PHASE_G if pg else eo.C_LEGS_PLAIN_G), (eo.C_LEGS_PHASE_H if ph else eo.C_LEGS_PLAIN_H)
                ex, ey, eh = emu_legs(d, ly, lx, lyd, lxd, nx, pg, ph, hi, prec)
                assert inside(ex, Gx, cg, prec) and inside(ey, Gy, cg, prec) and inside(eh, H, ch, prec), (pg, ph, hi)
                wx, wy, _ = emu_legs(d, ly, lx, ly, lx, nx, pg, ph, hi, prec)            # lx in place of lxd: the Nyquist column and row
                bx, by = eo.violations(wx, Gx, cg, prec), eo.violations(wy, Gy, cg, prec)
                assert bx.size == ny and np.all(bx % w == nx // 2) and by.size == w and np.all(by // w == ny // 2)
                if pg:                                                                     # the opposite phase
                    ox, _, _ = emu_legs(d, ly, lx, lyd, lxd, nx, -pg, ph, hi, prec)
                    assert not inside(ox, Gx, cg, prec)
                _, _, nh = emu_legs(d, ly, lx, lyd, lxd, nx, pg, ph, not hi, prec)
                assert not inside(nh, H, ch, prec)
    for acc in (False, True):
        R = eo.qe_div(d["kX"], d["kY"], d["Fn"], lyd, lxd, nx, out0=d["out0"] if acc else None)

        def emu_div(ax_y, ax_x):
            px, py = emu_cscale(d["kX"][:, :w], ax_x[None, :w]), emu_cscale(d["kY"][:, :w], ax_y[:, None])
            s = np.empty_like(px)
            s.real, s.imag = px.real + py.real, px.imag + py.imag
            v = emu_cscale(emu_muli(s), d["Fn"][:, :w])
            if acc:
                v.real, v.imag = d["out0"][:, :w].real + v.real, d["out0"][:, :w].imag + v.imag
            return v
        c = eo.C_DIV_ACC if acc else eo.C_DIV
        assert inside(emu_div(lyd, lxd), R, c, prec)
        assert not inside(emu_div(ly, lx), R, c, prec)
        assert not inside(emu_div(lyd, -lxd), R, c, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ny,nx", [(32, 64), (36, 40)])
def test_lensing_bounds_bite(prec, ny, nx):
    T = eo.RDT[prec]
    sty, stx = eo.steps()
    # split: both signs of the step
    for step, seed in ((sty, 1), (stx, 2)):
        alpha = eo.split_alpha(eo.SEED + seed, (ny, nx), step, prec)
        sh, R = eo.lens_split(alpha, step, prec)
        r = np.rint(alpha / T(step))
        assert np.array_equal(r.astype(np.int64), sh)
        assert inside(alpha - r * T(step), R, eo.C_SPLIT, prec)
        assert not inside(alpha - np.trunc(alpha / T(step)) * T(step), R, eo.C_SPLIT, prec)
    # gather
    g = eo.gather_inputs(eo.SEED, ny, nx, prec)
    yy, xx = eo.gather_index(g["sy"], g["sx"])
    for px, py, coef in eo.GATHER_CASES:
        for acc in (False, True):
            out0 = eo.gather_out0(g, px, py, prec)
            R = eo.lens_gather(g["src"], g["sx"], g["sy"], g["dx"], g["dy"], px, py, coef, prec, out0=out0 if acc else None)

            def emu(px_, py_, xx_):
                v = T(coef) * g["src"][yy, xx_]
                for p, dd in ((px_, g["dx"]), (py_, g["dy"])):
                    if p:
                        r = np.ones_like(dd)
                        for _ in range(p):
                            r = r * dd
                        v = v * r
                return out0 + v if acc else v
            c = eo.c_gather(px, py, acc)
            assert inside(emu(px, py, xx), R, c, prec), (px, py, acc)
            assert not inside(emu(px, py, (xx + 1) % nx), R, c, prec)                       # the neighbouring pixel
            assert not inside(emu(py, px, xx), R, c, prec) or px == py                        # the powers swapped
    # derivatives and the Taylor sum
    t = eo.taylor_inputs(eo.SEED, ny, nx, prec)
    _, _, lyd, lxd = eo.laxes(ny, nx, sty, stx, prec)
    kp, w = eo.kpitch(nx), nx // 2 + 1
    hc = eo.derivs_input(eo.SEED, ny, nx, prec)
    D = eo.hc_derivs(hc, lyd, lxd, nx, 8)

    def emu_deriv(a, b):
        kn = hc[:, :w]
        xp, yp = np.ones(w, dtype=T), np.ones(ny, dtype=T)
        for _ in range(a + b):
            kn = emu_muli(kn)
        for _ in range(a):
            xp = xp * lxd[:w]
        for _ in range(b):
            yp = yp * lyd
        return emu_cscale(kn, xp[None, :] * yp[:, None])
    for (a, b), R in D.items():
        assert inside(emu_deriv(a, b), R, eo.c_derivs(a + b), prec), (a, b)
        if a != b:
            assert not inside(emu_deriv(b, a), R, eo.c_derivs(a + b), prec), (a, b)
    yy, xx = eo.gather_index(t["sy"], t["sx"])
    for order in range(1, 9):
        nd = order * (order + 1) // 2 - 1
        R = eo.lens_taylor(t["src"], t["planes"][:nd], t["sx"], t["sy"], t["dx"], t["dy"], order)

        def emu_taylor(swap=False, drop=None):
            xa, ya = [np.ones_like(t["dx"])], [np.ones_like(t["dy"])]
            for n in range(1, order):
                xa.append(xa[-1] * t["dx"] / T(n))
                ya.append(ya[-1] * t["dy"] / T(n))
            acc = t["src"][yy, xx]
            for n in range(1, order):
                for b in range(n + 1):
                    if drop == (n - b, b):
                        continue
                    pw = (xa[b] * ya[n - b]) if swap else (xa[n - b] * ya[b])
                    acc = acc + t["planes"][eo.plane_index(n - b, b)][yy, xx] * pw
            return acc
        c = eo.c_taylor(order)
        assert inside(emu_taylor(), R, c, prec), order
        if order == 1:
            assert np.array_equal(emu_taylor(), R.ref.astype(T))
            continue
        assert not inside(emu_taylor(swap=True), R, c, prec), order                          # dx^a / a! and dy^b / b! swapped
        for drop in [(order - 1, 0), (0, order - 1), ((order - 1) // 2, order - 1 - (order - 1) // 2)]:
            assert not inside(emu_taylor(drop=drop), R, c, prec), (order, drop)                # one term of the highest order dropped
        assert np.abs(R.ref.astype(float) - eo.lens_taylor(t["src"], t["planes"][:nd], t["sx"], t["sy"], t["dx"], t["dy"], order,
                                                           drop=(order - 1, 0)).ref.astype(float)).max() > 0
