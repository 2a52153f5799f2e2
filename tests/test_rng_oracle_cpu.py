"""The NumPy statement of a Gaussian draw (oracle/rng_oracle.py) checked on its own: Philox4x32-10 against the Random123
known-answer vectors, the uniform edge words, the Hermitian / distinct-counter / unit-variance properties of the plane layout,
and the resolving power of the one comparison helper the GPU parity tests use."""
import numpy as np
import pytest

from oracle import rng_oracle as ro

SHAPES = [(32, 36), (36, 250), (66, 98), (32, 64)]      # nx/2 even and odd; chirp-z, mixed-radix and power-of-two plans
SEED, STREAM = 0x9E3779B97F4A7C15, 2 ** 40 + 3


def test_module_stands_alone():
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(ro))
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods == {"numpy"}


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    got = ro.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], [np.uint64(k) for k in key])
    assert tuple(int(g[0]) for g in got) == out


def test_philox_is_vectorised():
    ctr = np.arange(7, dtype=np.uint64)
    got = ro.philox4x32_10((ctr, 0, 5, 0), (9, 1))
    for i in range(7):
        one = ro.philox4x32_10((np.uint64(i), 0, 5, 0), (9, 1))
        assert [int(g[i]) for g in got] == [int(o) for o in one]


def test_uniform_edge_words():
    words = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    u = ro.uniform01(words)
    assert u.dtype == np.float32
    assert np.all(u > 0) and np.all(u <= 1)
    assert u[0] == np.float32(2.0 ** -33) and u[3] == np.float32(1.0)
    a, b = np.meshgrid(words, words, indexing="ij")
    n0, n1, r = ro.box_muller(a, b)
    assert np.all(np.isfinite(n0)) and np.all(np.isfinite(n1))
    assert np.all(r >= 0) and r.max() <= 6.77
    assert np.all(np.abs(n0 ** 2 + n1 ** 2 - r ** 2) <= 1e-14 * np.maximum(1.0, r ** 2))


def test_randn_layout():
    v = ro.randn(SEED, STREAM, 11)
    n, _ = ro.normals4(SEED, STREAM, np.arange(3, dtype=np.uint64))
    assert v.shape == (11,) and np.array_equal(v, n.reshape(-1)[:11])
    # the counter's upper word and both halves of key and stream take part
    base = ro.normals4(SEED, STREAM, np.array([5], dtype=np.uint64))[0]
    for other in (ro.normals4(SEED, STREAM, np.array([5 + 2 ** 32], dtype=np.uint64))[0],
                  ro.normals4(SEED ^ (1 << 40), STREAM, np.array([5], dtype=np.uint64))[0],
                  ro.normals4(SEED, STREAM ^ (1 << 40), np.array([5], dtype=np.uint64))[0],
                  ro.normals4(SEED ^ 1, STREAM, np.array([5], dtype=np.uint64))[0]):
        assert np.all(np.abs(other - base) > 1e-6)


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_plane_is_hermitian(ny, nx):
    k = ro.grf_hc(ny, nx, SEED, STREAM)
    assert k.shape == (ny, nx // 2 + 1)
    m = np.fft.ifft2(ro.hermitian_expand(k, nx))
    assert np.abs(m.imag).max() < 1e-13
    for y, x in ((0, 0), (ny // 2, 0), (0, nx // 2), (ny // 2, nx // 2)):
        assert k[y, x].imag == 0.0
    # a covsqrt plane is a plain product
    cs = np.random.default_rng(1).uniform(0.5, 2.0, size=k.shape)
    assert np.array_equal(ro.grf_hc(ny, nx, SEED, STREAM, cs), k * cs)


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_counters_are_distinct(ny, nx):
    ctr, slot, mirrored = ro.hc_counters(ny, nx)
    nxh = nx // 2
    assert int(mirrored.sum()) == 2 * (ny - ny // 2 - 1) and set(np.nonzero(mirrored)[1]) <= {0, nxh}
    own = 2 * ctr[~mirrored] + slot[~mirrored].astype(np.uint64)
    assert np.unique(own).size == own.size
    # the intended reuse: a mirrored row reads the normals of its partner row ny - y of the same column
    for y, x in zip(*np.nonzero(mirrored)):
        assert ctr[y, x] == ctr[ny - y, x] and slot[y, x] == slot[ny - y, x] and not mirrored[ny - y, x]


@pytest.mark.parametrize("ny,nx", SHAPES)
def test_unit_variance_per_pixel(ny, nx):
    K = 300
    maps = np.empty((K, ny, nx))
    for s in range(K):
        m = np.fft.ifft2(ro.hermitian_expand(ro.grf_hc(ny, nx, SEED + s, STREAM), nx)) * np.sqrt(ny * nx)
        maps[s] = m.real
    v = maps.var(axis=0, ddof=1).mean()
    tol = 5 * np.sqrt(2.0 / (K * ny * nx))
    print("shape %dx%d: mean per-pixel variance - 1 = %+.2e (%.2f sigma)" % (ny, nx, v - 1, (v - 1) / (tol / 5)))
    assert abs(v - 1.0) < tol


def test_mix_is_the_sum_of_its_planes():
    ny, nx = 32, 36
    rng = np.random.default_rng(2)
    shp = (ny, nx // 2 + 1)
    cs = [[rng.uniform(0.5, 2, shp) if (i + j) % 2 == 0 else None for j in range(3)] for i in range(3)]
    ang = rng.uniform(0, 2 * np.pi, shp)
    rot = (np.cos(ang), np.sin(ang))
    w = [ro.grf_hc(ny, nx, 7, STREAM + c) for c in range(3)]
    v = [sum(cs[i][j] * w[j] for j in range(3) if cs[i][j] is not None) for i in range(3)]
    out, bound = ro.grf_mix(ny, nx, 7, STREAM, cs, rot=rot, scale=0.5, with_bound=True, prec="f32")
    ref = [0.5 * v[0], 0.5 * (v[1] * rot[0] - v[2] * rot[1]), 0.5 * (v[1] * rot[1] + v[2] * rot[0])]
    for i in range(3):
        assert np.allclose(out[i], ref[i], rtol=0, atol=1e-14)
        assert bound[i].shape == shp + (2,) and np.all(bound[i] >= 0) and bound[i].max() < 1e-4
    ins = [rng.standard_normal(shp) + 1j * rng.standard_normal(shp) for _ in range(3)]
    f = rng.uniform(0.5, 1, shp)
    out2 = ro.grf_mix(ny, nx, 7, STREAM, cs, rot=rot, inputs=ins, filt=f, scale=0.5)
    u = [k * f for k in ins]
    ref2 = [u[0] + 0.5 * v[0], u[1] * rot[0] - u[2] * rot[1] + 0.5 * v[1], u[1] * rot[1] + u[2] * rot[0] + 0.5 * v[2]]
    for i in range(3):
        assert np.allclose(out2[i], ref2[i], rtol=0, atol=1e-14)


def test_draw_mismatch_helper():
    ref = np.array([1.0, -2.0, 3.0])
    assert ro.draw_mismatch(ref, ref, 1e-6) == 0.0
    assert ro.draw_mismatch(ref + np.array([0, 5e-7, 0]), ref, 1e-6) == pytest.approx(0.5)
    assert ro.draw_mismatch(ref + np.array([0, 0, 2e-6]), ref, np.array([1e-6, 1e-6, 4e-6])) == pytest.approx(0.5)
    # zero bound: equality or nothing; NaN never passes
    assert ro.draw_mismatch(ref, ref, 0.0) == 0.0
    assert ro.draw_mismatch(np.nextafter(ref, 9.0), ref, np.array([0.0, 1.0, 1.0])) == np.inf
    assert ro.draw_mismatch(np.array([np.nan, 0, 0]), np.zeros(3), 1.0) == np.inf
    # complex: real and imaginary parts are compared one by one, with a per-mode or a per-part bound
    z = np.array([1 + 1j, 2 - 1j])
    assert ro.draw_mismatch(z + 3e-6j, z, 1e-6) == pytest.approx(3.0)
    assert ro.draw_mismatch(z + 3e-6j, z, np.array([[1e-6, 6e-6], [1e-6, 6e-6]])) == pytest.approx(0.5)
    assert ro.draw_ratios(z, z, 1e-6).shape == (2, 2)
    with pytest.raises(ValueError):
        ro.draw_mismatch(np.zeros(3), np.zeros(4), 1.0)
    with pytest.raises(ValueError):
        ro.draw_mismatch(np.zeros(3), np.zeros(3), -1.0)


def _wrong_counters(name):
    """a layout mistake, as a replacement for the oracle's hc_counters"""
    true = ro.hc_counters

    def bad(ny, nx):
        ctr, slot, mirrored = true(ny, nx)
        if name == "no_conj":                    # the mirrored rows read their partner's normals but are not conjugated
            return ctr, slot, np.zeros_like(mirrored)
        if name == "counter_plus_one":
            return ctr + np.uint64(1), slot, mirrored
        npair = np.uint64(nx // 2 // 2 + 1)      # npair_nx4: row stride nx / 4 instead of (nx/2)/2 + 1
        return (ctr // npair) * np.uint64(nx // 4) + ctr % npair, slot, mirrored
    return bad


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["key_high", "stream_high", "swap_sincos", "no_conj", "counter_plus_one", "npair_nx4"])
@pytest.mark.parametrize("ny,nx", [(36, 250), (66, 98), (32, 64)])
def test_draw_mismatch_resolves_a_wrong_draw(ny, nx, name, prec, monkeypatch):
    """Six wrong draws, each made by replacing one piece of the oracle for the length of the test, against the bounds of the GPU
    parity tests: draw_mismatch > 1, and more than 99 % of the modes the mistake touches sit above their bound.  "Touches" is
    computed, not listed: a mode whose (counter, slot, conjugation) is the true one draws the true value and must compare equal;
    for the three layout mistakes EVERY other mode must exceed its bound.  (Omitted conjugation can only touch the mirrored rows
    of the two self-conjugate columns, a wrong npair leaves row ys = 0 alone; the other four touch every mode.)"""
    seed, sid = 0xC0FFEE123456789A, STREAM
    cs = np.random.default_rng(5).uniform(0.5, 2.0, size=(ny, nx // 2 + 1))
    ref, bound = ro.grf_hc(ny, nx, seed, sid, cs, with_bound=True, prec=prec)
    assert ro.draw_mismatch(ref, ref, bound) == 0.0
    touched = np.ones((ny, nx // 2 + 1), dtype=bool)
    layout = name in ("no_conj", "counter_plus_one", "npair_nx4")
    if name == "key_high":
        bad = ro.grf_hc(ny, nx, seed & 0xFFFFFFFF, sid, cs)
    elif name == "stream_high":
        bad = ro.grf_hc(ny, nx, seed, sid & 0xFFFFFFFF, cs)
    elif name == "swap_sincos":
        true_bm = ro.box_muller
        monkeypatch.setattr(ro, "box_muller", lambda a, b: (lambda n0, n1, r: (n1, n0, r))(*true_bm(a, b)))
        bad = ro.grf_hc(ny, nx, seed, sid, cs)
    else:
        wrong = _wrong_counters(name)
        touched = np.zeros_like(touched)
        for t, w in zip(ro.hc_counters(ny, nx), wrong(ny, nx)):
            touched |= t != w
        monkeypatch.setattr(ro, "hc_counters", wrong)
        bad = ro.grf_hc(ny, nx, seed, sid, cs)
    monkeypatch.undo()
    assert np.array_equal(ro.grf_hc(ny, nx, seed, sid, cs), ref)
    assert ro.draw_mismatch(bad, ref, bound) > 1.0
    mode_off = ro.draw_ratios(bad, ref, bound).max(axis=-1) > 1.0
    assert touched.sum() >= ny - 2
    frac = mode_off[touched].mean()
    assert frac > 0.99, "%s: only %.2f %% of the touched modes exceed the bound" % (name, 100 * frac)
    if layout:
        assert mode_off[touched].all()
        assert np.array_equal(bad[~touched], ref[~touched])
