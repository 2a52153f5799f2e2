"""CPU: the host side of the band-grid dispatch of the general estimators (lensing.Estimator.one_call_pol / pol_band_grid): which
band numbers go to the grid rule for an estimator set, and for which geometries the one-call path is taken."""
import types

import numpy as np

from orphics_amd import engine, lensing


def test_widest_band_and_zero_poisons_the_set():
    assert lensing.widest([56, 70, 42]) == 70
    assert lensing.widest([56, 0, 42]) == 0          # 0 = all columns / rows: no pruning for the whole set
    gens = [dict(wl=56, wk=84, rl=56, rk=84), dict(wl=70, wk=60, rl=42, rk=90)]
    assert lensing.pol_bands(gens) == (70, 84, 56, 90)
    assert lensing.pol_bands(gens, wK=(122, 98)) == (70, 122, 56, 98)        # external normalisation planes: the kappa mask's support
    assert lensing.pol_bands(gens + [dict(wl=0, wk=84, rl=56, rk=84)]) == (0, 84, 56, 90)
    assert lensing.pol_bands(gens + [dict(wl=10, wk=84, rl=0, rk=0)], wK=(122, 98)) == (70, 122, 0, 98)


class _Eng(object):
    """the attributes of engine.Engine the dispatch reads, without a device"""

    def __init__(self, ny, nx):
        self.ny, self.nx = ny, nx
        self.pow2 = (ny & (ny - 1)) == 0 and (nx & (nx - 1)) == 0

        def smooth(n):
            for r in (2, 3, 5):
                while n % r == 0:
                    n //= r
            return n == 1
        self.mixed = (not self.pow2) and ny % 2 == 0 and nx % 2 == 0 and smooth(ny) and smooth(nx)
        self.calls = []

    def band_grid(self, *a):
        self.calls.append(a)
        return engine.Engine.band_grid(self, *a)


def _bands(shape, res_arcmin, lmax_leg, lmax_kappa):
    """support of a circular ell cut on the hc grid: (columns, rows) as Estimator._support_cols / _support_rows count them"""
    ny, nx = shape
    dly, dlx = 21600.0 / (ny * res_arcmin), 21600.0 / (nx * res_arcmin)
    return (int(lmax_leg // dlx) + 1, int(lmax_kappa // dlx) + 1), (int(lmax_leg // dly) + 1, int(lmax_kappa // dly) + 1)


def _fake(shape, res, legs, lmax_kappa, mrow=-1, mcol=-1, unbounded=()):
    q = lensing.Estimator.__new__(lensing.Estimator)
    q.eng = _Eng(*shape)
    q.mrow, q.mcol = mrow, mcol
    q._gen = {}
    for XY, lmax in legs.items():
        (wl, wk), (rl, rk) = _bands(shape, res, lmax, lmax_kappa)
        q._gen[XY] = dict(wl=0 if XY in unbounded else wl, wk=wk, rl=0 if XY in unbounded else rl, rk=rk, pieces=[])
    (_, wk), (_, rk) = _bands(shape, res, 0, lmax_kappa)
    q._wK = (wk, rk)
    return q


ESTS = ("TT", "TE", "EE", "EB", "TB")


def test_one_call_pol_per_geometry():
    T = {XY: 2000 for XY in ESTS}
    # 600 x 750 at 1': 256 x 512; the MV set hands the grid rule the widest leg band and the kappa mask's support
    q = _fake((600, 750), 1.0, T, 3500)
    assert q.one_call_pol(ESTS) and q.pol_band_grid(ESTS) == (256, 512) and q.pol_band_grid("EB") == (256, 512)
    assert q.eng.calls[-1] == (70, 122, 56, 98, -1, -1)
    # 1200^2 at 0.5': the notebook's patch on 256^2
    q = _fake((1200, 1200), 0.5, T, 3000)
    assert q.one_call_pol("EB") and q.pol_band_grid(ESTS) == (256, 256)
    # a polarisation mask to 1500: EE / EB on 256 x 256, anything with a T leg (and the MV set: the widest band) on 256 x 512
    q = _fake((600, 750), 1.0, dict(TT=2000, TE=2000, TB=2000, EE=1500, EB=1500), 3500)
    assert q.pol_band_grid("EB") == (256, 256) and q.pol_band_grid("EE") == (256, 256)
    assert q.pol_band_grid("TE") == (256, 512) and q.pol_band_grid(ESTS) == (256, 512)
    assert q.pol_band_grid(("EE", "EB")) == (256, 256)
    assert q.eng.calls[-1] == (53, 122, 42, 98, -1, -1)
    # an explicit row / column grid one step above the automatic one; one below aliases
    q = _fake((1200, 1200), 0.5, T, 3000, mrow=512, mcol=512)
    assert q.pol_band_grid(ESTS) == (512, 512) and q.one_call_pol("TE")
    q = _fake((1200, 1200), 0.5, T, 3000, mrow=128, mcol=-1)
    assert q.pol_band_grid(ESTS) is None and not q.one_call_pol("EB")
    # the map's own grid, unbounded filters (one estimator poisons the set it is in, not the others), a grid not smaller than the map
    q = _fake((600, 750), 1.0, T, 3500, mrow=0, mcol=0)
    assert not q.one_call_pol(ESTS) and not q.one_call_pol("EB")
    q = _fake((600, 750), 1.0, T, 3500, unbounded=("TB",))
    assert not q.one_call_pol(ESTS) and not q.one_call_pol("TB") and q.one_call_pol("EB") and q.one_call_pol(("TE", "EB"))
    q = _fake((480, 600), 2.0, T, 3500)
    assert not q.one_call_pol(ESTS) and not q.one_call_pol("EB")
    # chirp-z sides never; power-of-two sides always (no band grid there: the fused kernels run on the map's grid)
    q = _fake((700, 700), 1.0, T, 3500)
    assert not q.eng.mixed and not q.one_call_pol("EB") and q.pol_band_grid("EB") is None
    q = _fake((512, 512), 2.0, T, 3000)
    assert q.one_call_pol(ESTS) and q.pol_band_grid(ESTS) is None


def test_external_norm_uses_the_kappa_mask_support():
    q = _fake((600, 750), 1.0, dict(EB=1500), 3500)
    q._gen["EB"]["wk"], q._gen["EB"]["rk"] = 100, 80         # the estimator's own normalisation vanishes earlier than the mask
    q.pol_band_grid("EB")
    assert q.eng.calls[-1] == (53, 100, 42, 80, -1, -1)
    q.pol_band_grid("EB", ext_norm=True)                     # reconstruct_hc(norm=...): an MV weight plane reaches the mask's edge
    assert q.eng.calls[-1] == (53, 122, 42, 98, -1, -1)
    assert np.all(np.array(q.eng.calls[-1][:4]) > 0)
