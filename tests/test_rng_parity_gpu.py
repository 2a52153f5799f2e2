"""The draw kernels of csrc/rng.hip (oa_randn, oa_grf_hc, oa_grf_hc_band, oa_grf_mix) against oracle/rng_oracle.py: every number
of every plane, through the one helper ``draw_mismatch``.

BOUND (oracle/rng_oracle.py, ERROR MODEL): per normal ``1e-6 * max(1, r)`` with r the Box-Muller radius from the oracle --
``logf``, ``sqrtf`` and ``sincospif`` each taken as within 2 ulp, plus the float32 roundings of the products: at most
5.75 * 2^-23 r ~ 6.9e-7 r.
Scale factors (1 / sqrt 2, covsqrt, mix coefficients, rotation, scale) propagate linearly, and the plan's own roundings add
4 eps of the sum of the absolute values of the terms (eps = 2^-24 float32 plans, 2^-53 float64 plans).  A wrong Philox word,
counter, key half or branch is off by O(1) (tests/test_rng_oracle_cpu.py shows that this bound rejects six such mistakes), so the
bound hides nothing.

NOT COVERED: the upper 32 bits of the counter (the element index): a stream needs more than 2^34 normals (a plane of more
than 2^33 modes) to reach them.  The upper halves of seed and stream id ARE covered (SEEDS[1]; the seed is >= 2^63)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import rng_oracle as ro   # noqa: E402

PLANS = [(64, 64), (32, 128), (128, 32),      # power of two
         (36, 250), (96, 160),                # mixed radix
         (66, 98)]                            # chirp-z
SEEDS = [(1234, 2), (0xC0FFEE123456789A, 2 ** 40 + 3)]
NPDT = {"f32": np.float32, "f64": np.float64}
FILL = complex(7.25, -3.5)


def eng(ny, nx, prec):
    from orphics_amd.engine import Engine
    return Engine.get(ny, nx, prec)


def lib():
    from orphics_amd import _lib
    return _lib.load()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def covsqrt_host(ny, nx, kp, prec):
    """random positive amplitude plane (ny, kp), symmetric under y -> ny - y like every physical one (the exact conjugacy of the
    self-conjugate columns needs equal amplitudes on the two rows of a pair)"""
    rng = np.random.default_rng(ny * 1000 + nx)
    cs = rng.uniform(0.25, 4.0, size=(ny, kp)).astype(NPDT[prec])
    cs[ny // 2 + 1:] = cs[1:ny - ny // 2][::-1]
    cs.setflags(write=False)
    return cs


@pytest.mark.parametrize("seed,sid", SEEDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 3, 4, 4099])
def test_randn(n, prec, seed, sid):
    from orphics_amd._lib import OA_F32, OA_F64, check
    dt = torch.float32 if prec == "f32" else torch.float64
    code = OA_F32 if prec == "f32" else OA_F64
    guard = 8
    bufs = []
    for _ in range(2):
        buf = torch.full((n + guard,), -77.0, dtype=dt, device="cuda")
        check(lib().oa_randn(code, seed, sid, ptr(buf), n, stream()))
        bufs.append(buf.cpu().numpy())
    ref, bound = ro.randn(seed, sid, n, with_bound=True)
    worst = ro.draw_mismatch(bufs[0][:n], ref, bound)
    print("randn n=%d %s: worst |err| / bound = %.3f" % (n, prec, worst))
    assert worst <= 1.0
    assert np.all(bufs[0][n:] == -77.0), "oa_randn wrote behind its n elements"
    assert bufs[0].tobytes() == bufs[1].tobytes(), "two launches differ"


@pytest.mark.parametrize("seed,sid", SEEDS)
@pytest.mark.parametrize("with_cov", [False, True])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("ny,nx", PLANS)
def test_grf_hc(ny, nx, prec, with_cov, seed, sid):
    e = eng(ny, nx, prec)
    nxh = nx // 2
    csh = covsqrt_host(ny, nx, e.kp, prec) if with_cov else None
    cs = torch.as_tensor(np.array(csh), device=e.device) if with_cov else None
    out = torch.full((ny, e.kp), FILL, dtype=e.cdt, device=e.device)
    e.grf_hc(seed, sid, cs, out=out)
    k = out.cpu().numpy()
    ref, bound = ro.grf_hc(ny, nx, seed, sid, None if csh is None else csh[:, :nxh + 1].astype(np.float64), with_bound=True, prec=prec)
    worst = ro.draw_mismatch(k[:, :nxh + 1], ref, bound)
    print("grf_hc %dx%d %s cov=%s: worst |err| / bound = %.3f" % (ny, nx, prec, with_cov, worst))
    assert worst <= 1.0
    assert np.all(k[:, nxh + 1:] == np.asarray(FILL, dtype=k.dtype)), "pad columns written"
    for x in (0, nxh):                         # both self-conjugate columns: exact conjugate pairs, real at y = 0, ny/2
        a, b = k[1:ny // 2, x], k[:ny // 2:-1, x][:ny // 2 - 1]
        assert a.shape == b.shape == (ny // 2 - 1,)
        assert np.array_equal(a.real, b.real) and np.array_equal(a.imag, -b.imag), "column %d is not Hermitian" % x
        assert k[0, x].imag == 0.0 and k[ny // 2, x].imag == 0.0
    again = torch.full((ny, e.kp), FILL, dtype=e.cdt, device=e.device)
    e.grf_hc(seed, sid, cs, out=again)
    assert torch.equal(out, again)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("width,rband", [(1, 1), (7, 5), (125, 0), (0, 17)])
@pytest.mark.parametrize("ny,nx", [(36, 250), (66, 98)])
def test_grf_hc_band(ny, nx, width, rband, prec):
    """Region draw: columns < width, rows y < rband or y > ny - rband (0 = all) hold the full-plane draw; the rest of the plane is
    not written.  Whole column pairs are drawn: an odd width may (not must) also fill column ``width`` -- exactly that one."""
    seed, sid = SEEDS[1]
    e = eng(ny, nx, prec)
    nxh = nx // 2
    csh = covsqrt_host(ny, nx, e.kp, prec)
    out = torch.full((ny, e.kp), FILL, dtype=e.cdt, device=e.device)
    e.grf_hc(seed, sid, torch.as_tensor(np.array(csh), device=e.device), out=out, width=width, rband=rband)
    k = out.cpu().numpy()
    ref, bound = ro.grf_hc(ny, nx, seed, sid, csh[:, :nxh + 1].astype(np.float64), with_bound=True, prec=prec)
    ncols = width if 0 < width < nxh + 1 else nxh + 1
    y = np.arange(ny)
    rows = ((y < rband) | (y > ny - rband)) if (rband > 0 and 2 * rband - 1 < ny) else np.ones(ny, dtype=bool)
    assert rows.sum() == (2 * rband - 1 if rband > 0 else ny)
    fill = np.asarray(FILL, dtype=k.dtype)
    worst = ro.draw_mismatch(k[rows][:, :ncols], ref[rows][:, :ncols], bound[rows][:, :ncols])
    print("grf_hc_band %dx%d w=%d rb=%d %s: worst |err| / bound = %.3f" % (ny, nx, width, rband, prec, worst))
    assert worst <= 1.0
    assert np.all(k[~rows] == fill), "rows outside the band written"
    first_free = ncols
    if ncols % 2 == 1 and ncols <= nxh:        # the round-up of an odd width: the pair's second column, drawn or left alone
        extra = k[rows][:, ncols]
        if not np.all(extra == fill):
            assert ro.draw_mismatch(extra, ref[rows][:, ncols], bound[rows][:, ncols]) <= 1.0
        first_free = ncols + 1
    assert np.all(k[:, first_free:] == fill), "columns outside the band written"


# nx/2 odd makes the row pitch kp = nx/2 + 16 odd: the kernel then moves its column pairs one column at a time, and the last pair
# of a row has no second column; (36, 250) and (66, 98) take that path, (64, 64) the paired loads and stores
MIX_PLANS = [(36, 250, "f64"), (64, 64, "f32"), (66, 98, "f32")]


def _mix_case(ny, nx, prec, case):
    e = eng(ny, nx, prec)
    rng = np.random.default_rng({"n1": 1, "n2": 2, "n3rot": 3, "n3in": 4}[case] + ny)
    rd = NPDT[prec]
    shp = (ny, e.kp)

    def amp():
        return rng.uniform(0.25, 2.0, size=shp).astype(rd) * rng.choice([-1.0, 1.0], size=shp).astype(rd)
    if case == "n1":
        cs, rot, scale = [[amp()]], None, 1.0
    elif case == "n2":
        cs, rot, scale = [[amp(), None], [amp(), amp()]], None, 0.75
    else:
        cs = [[amp(), None, None], [amp(), amp(), None], [None, amp(), amp()]]
        ang = rng.uniform(0, 2 * np.pi, size=shp)
        rot = (np.cos(ang).astype(rd), np.sin(ang).astype(rd))
        scale = 1.0 if case == "n3rot" else 0.5
    ins = filt = None
    if case == "n3in":
        ins = [(rng.standard_normal(shp) + 1j * rng.standard_normal(shp)).astype(np.complex64 if prec == "f32" else np.complex128)
               for _ in range(3)]
        filt = rng.uniform(0.2, 1.0, size=shp).astype(rd)
    return e, cs, rot, ins, filt, scale


@pytest.mark.parametrize("case", ["n1", "n2", "n3rot", "n3in"])
@pytest.mark.parametrize("ny,nx,prec", MIX_PLANS)
def test_grf_mix(ny, nx, prec, case):
    """ncomp 1, 2; 3 with rotation; 3 with inputs, filter, rotation and scale = 0.5 written over the inputs."""
    seed, sid0 = SEEDS[1]
    e, cs, rot, ins, filt, scale = _mix_case(ny, nx, prec, case)
    nxh, n = nx // 2, len(cs)

    def dev(a):
        return None if a is None else torch.as_tensor(a, device=e.device)
    cs_d = [[dev(c) for c in row] for row in cs]
    rot_d = None if rot is None else (dev(rot[0]), dev(rot[1]))
    if ins is None:
        outs = [torch.full((ny, e.kp), FILL, dtype=e.cdt, device=e.device) for _ in range(n)]
        got = e.grf_mix(seed, cs_d, rot=rot_d, scale=scale, out=outs, stream_id0=sid0)
    else:
        ins_d = [dev(k) for k in ins]
        got = e.grf_mix(seed, cs_d, rot=rot_d, inputs=ins_d, filt=dev(filt), scale=scale, out=ins_d, stream_id0=sid0)
        assert all(g.data_ptr() == k.data_ptr() for g, k in zip(got, ins_d))

    def cut(a):
        return None if a is None else a[:, :nxh + 1].astype(np.complex128 if np.iscomplexobj(a) else np.float64)
    ref, bound = ro.grf_mix(ny, nx, seed, sid0, [[cut(c) for c in row] for row in cs], rot=None if rot is None else (cut(rot[0]), cut(rot[1])),
                            inputs=None if ins is None else [cut(k) for k in ins], filt=cut(filt), scale=scale, with_bound=True, prec=prec)
    for i in range(n):
        k = got[i].cpu().numpy()
        worst = ro.draw_mismatch(k[:, :nxh + 1], ref[i], bound[i])
        print("grf_mix %dx%d %s %s plane %d: worst |err| / bound = %.3f" % (ny, nx, prec, case, i, worst))
        assert worst <= 1.0
        assert np.all(k[:, nxh + 1:] == 0), "pad columns of plane %d are not zero" % i
