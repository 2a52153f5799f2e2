"""GPU: ``oa_grf_hc_icols`` -- the Gaussian draw evaluated inside the load of inverse column pass 1 -- is bit for bit ``oa_grf_hc``
followed by ``oa_fft_cols(inverse = 1, scale = 1, width = nx/2 + 1)``: ``torch.equal``, no tolerance.

Shapes, where the kernel can still go wrong: (32, 32) -- 17 columns, one partly filled tile, N1 = 8 (workgroups of 16 threads, two
butterflies per thread); (64, 256) -- 129 columns, the Nyquist column alone in the last tile (its lane partner draws nothing);
(512, 64) -- a tall plane (N1 = 32: radix-16 x 2); (2048, 128) -- log2 Ny odd, so N1 = 64 != N2 = 32.  Column 0 and column nx/2 read the
mirrored row's counter above the middle row in every one of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = [(32, 32), (64, 256), (512, 64), (2048, 128)]
_ENG = {}


def _engine(shape, prec):
    from orphics_amd.engine import Engine
    if (shape, prec) not in _ENG:
        _ENG[(shape, prec)] = Engine(shape[0], shape[1], prec)
    return _ENG[(shape, prec)]


def _amp(e):
    """an amplitude plane with no symmetry in y or x"""
    y = torch.arange(e.ny, device=e.device, dtype=e.rdt)[:, None]
    x = torch.arange(e.kp, device=e.device, dtype=e.rdt)[None, :]
    return (0.5 + ((3 * y + 7 * x) % 11) / 11.0).contiguous()


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_draw_is_bit_for_bit_the_draw_then_the_column_transform(shape, prec):
    e = _engine(shape, prec)
    assert e.pow2
    w = e.nx // 2 + 1
    cases = [(1, 5, True), (3, 2 ** 32 + 7, True), (3, 11, False)]          # (nreal, first stream id, with an amplitude plane)
    for nreal, sid, with_cs in cases:
        cs = _amp(e) if with_cs else None
        got = e.grf_hc_icols(0xABCDEF0123, sid, cs, nreal=nreal)
        assert tuple(got.shape) == (nreal, e.ny, e.kp)
        for z in range(nreal):
            ref = e.fft_cols(e.grf_hc(0xABCDEF0123, sid + z, cs), inverse=True, scale=1.0, width=w)
            assert torch.equal(got[z, :, :w], ref[:, :w]), (shape, prec, nreal, sid, z)
            assert float(got[z, :, :w].abs().min()) > 0
        assert not bool(got[:, :, w:].any())                                # the row padding is not written
    # planes of a batch do not depend on the batch: plane 1 of three == a single draw of its stream
    one = e.grf_hc_icols(0xABCDEF0123, 12, None, nreal=1)
    assert torch.equal(one[0], e.grf_hc_icols(0xABCDEF0123, 11, None, nreal=3)[1])


def test_other_plans_are_refused_by_name():
    from orphics_amd._lib import OrphicsAmdError
    from orphics_amd.engine import Engine
    e = Engine(600, 750, "f32")
    assert e.mixed
    with pytest.raises(OrphicsAmdError, match="oa_grf_hc_icols.*not powers of two"):
        e.grf_hc_icols(1, 0, None)
    p = _engine((32, 32), "f32")
    with pytest.raises(ValueError):
        p.grf_hc_icols(1, 0, None, nreal=0)
