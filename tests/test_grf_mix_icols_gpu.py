"""GPU: ``oa_grf_mix_icols`` -- the mixed T, Q, U draw evaluated inside the load of inverse column pass 1, each Philox counter once per
triple -- is bit for bit ``oa_grf_mix(rot_c = c, rot_s = -s)`` followed by ``oa_fft_cols(inverse = 1, scale = 1, width = nx/2 + 1)`` per
component: ``torch.equal``, no tolerance.

Shapes, where the single-field kernel can still go wrong: (32, 32) -- 17 columns, one partly filled tile, N1 = 8 (workgroups of 16
threads); (64, 256) -- 129 columns, the Nyquist column alone in the last tile (its lane partner draws nothing); (512, 64) -- a tall plane
(N1 = 32: radix-16 x 2); (2048, 128) -- log2 Ny odd, so N1 = 64 != N2 = 32.  Column 0 and column nx/2 read the mirrored row's counter
above the middle row in every one of them.  Amplitude and rotation planes have no symmetry in y or x."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [(32, 32), (64, 256), (512, 64), (2048, 128)]
SEED = 0xABCDEF0123
_ENG = {}


def _engine(shape, prec):
    from orphics_amd.engine import Engine
    if (shape, prec) not in _ENG:
        _ENG[(shape, prec)] = Engine(shape[0], shape[1], prec)
    return _ENG[(shape, prec)]


def _plane(e, a, b, m, lo=0.5):
    y = torch.arange(e.ny, device=e.device, dtype=e.rdt)[:, None]
    x = torch.arange(e.kp, device=e.device, dtype=e.rdt)[None, :]
    return (lo + ((a * y + b * x) % m) / float(m)).contiguous()


def _blocks(e, full=False):
    """the four blocks the driver uses (TT, ET, EE, BB), or all nine"""
    cs = [[None] * 3 for _ in range(3)]
    cs[0][0] = _plane(e, 3, 7, 11)
    cs[1][0] = _plane(e, 5, 3, 13, lo=-0.4)
    cs[1][1] = _plane(e, 7, 5, 17)
    cs[2][2] = _plane(e, 11, 9, 19, lo=0.25)
    if full:
        k = 0
        for i in range(3):
            for j in range(3):
                if cs[i][j] is None:
                    cs[i][j] = _plane(e, 2 + k, 13 - k, 23, lo=-0.3)
                    k += 1
    return cs


def _rot(e):
    ang = 2.0 * torch.pi * _plane(e, 3, 5, 29, lo=0.1)
    return torch.cos(ang).contiguous(), torch.sin(ang).contiguous()


def _reference(e, cs, rot, sid):
    w = e.nx // 2 + 1
    draw = e.grf_mix(SEED, cs, rot=None if rot is None else (rot[0], (-rot[1]).contiguous()), stream_id0=sid)
    return [e.fft_cols(k, inverse=True, scale=1.0, width=w) for k in draw]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_mixed_draw_is_bit_for_bit_the_draw_then_the_column_transform(shape, prec):
    e = _engine(shape, prec)
    assert e.pow2
    w = e.nx // 2 + 1
    rot = _rot(e)
    # (ntriples, first stream id, all nine blocks, with the rotation)
    cases = [(1, 5, False, True), (2, 2 ** 32 + 7, False, True), (2, 11, True, True), (1, 4, False, False)]
    for ntriples, sid, full, with_rot in cases:
        cs = _blocks(e, full)
        r = rot if with_rot else None
        got = e.grf_mix_icols(SEED, cs, r, stream_id0=sid, ntriples=ntriples)
        assert tuple(got.shape) == (3 * ntriples, e.ny, e.kp)
        for t in range(ntriples):
            ref = _reference(e, cs, r, sid + 3 * t)
            for c in range(3):
                assert torch.equal(got[3 * t + c, :, :w], ref[c][:, :w]), (shape, prec, ntriples, sid, full, with_rot, t, c)
                assert float(got[3 * t + c, :, :w].abs().min()) > 0
        assert not bool(got[:, :, w:].any())                                # the row padding is not written
    # rotation off: the planes are T, E, B -- E and B differ from Q and U
    cs = _blocks(e)
    teb = e.grf_mix_icols(SEED, cs, None, stream_id0=5)
    tqu = e.grf_mix_icols(SEED, cs, rot, stream_id0=5)
    assert torch.equal(teb[0], tqu[0]) and not torch.equal(teb[1], tqu[1]) and not torch.equal(teb[2], tqu[2])
    # triples of a launch do not depend on the launch: triple 1 of two == a single triple of its streams
    two = e.grf_mix_icols(SEED, cs, rot, stream_id0=11, ntriples=2)
    assert torch.equal(two[3:6], e.grf_mix_icols(SEED, cs, rot, stream_id0=14, ntriples=1))


def test_other_plans_and_counts_are_refused_by_name():
    from orphics_amd._lib import OrphicsAmdError
    from orphics_amd.engine import Engine
    e = Engine(600, 750, "f32")
    assert e.mixed
    with pytest.raises(OrphicsAmdError, match="oa_grf_mix_icols.*not powers of two"):
        e.grf_mix_icols(1, _blocks(e), None)
    p = _engine((32, 32), "f32")
    with pytest.raises(OrphicsAmdError, match="oa_grf_mix_icols.*ntriples"):
        p.grf_mix_icols(1, _blocks(p), None, ntriples=0)
