"""CPU: the BAND GRID identity behind the one-call TT entries on map sides 2^a 3^b 5^c (include/orphics_amd.h, oa_plan_band_grid),
checked in NumPy, and the host-side mirror of the C grid rule (orphics_amd.engine.band_grid)."""
import numpy as np
import pytest

from oracle import qe_oracle as qo


def _notebook(shape, res_arcmin, tl=(300, 2000), kl=(20, 3500)):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res_arcmin)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=tl[0], lmax=tl[1])
    kmask = maps.mask_kspace(shape, g, lmin=kl[0], lmax=kl[1])
    return g, th.lCl("TT", ml), beam, noise, tmask, kmask


def _band(*planes):
    """(columns, rows) outside which all the FULL planes vanish: columns |kx index| < w, rows |ky index| < r
    (lensing.Estimator._support_cols / _support_rows on the half plane)."""
    nz = np.zeros(planes[0].shape, dtype=bool)
    for a in planes:
        nz |= a != 0
    ny, nx = nz.shape
    y, x = np.nonzero(nz)
    return int(np.minimum(x, nx - x).max()) + 1, int(np.minimum(y, ny - y).max()) + 1


def _signed(n):
    return np.fft.fftfreq(n, 1.0 / n).astype(int)


def _crop(a, my, mx, w, r):
    """modes |ky| < r, |kx| < w of an (Ny, Nx) full plane at rows ky mod my, columns kx mod mx of an (my, mx) plane"""
    ny, nx = a.shape
    ky, kx = _signed(ny), _signed(nx)
    ys, xs = np.nonzero(np.abs(ky) < r)[0], np.nonzero(np.abs(kx) < w)[0]
    out = np.zeros((my, mx), dtype=a.dtype)
    out[np.ix_(ky[ys] % my, kx[xs] % mx)] = a[np.ix_(ys, xs)]
    return out


@pytest.mark.parametrize("shape,res,grid", [((1200, 1200), 0.5, (256, 256)), ((600, 750), 1.0, (256, 512))])
def test_band_grid_identity_numpy(shape, res, grid):
    """The oracle TT estimator on the notebook's N-grid equals the same estimator on the inner power-of-two grid (filters
    cropped to their bands, rows remapped ky mod My, Fnorm times My Mx / (Ny Nx)) on every kappa mode, to 1e-12."""
    from orphics_amd.engine import band_grid
    g, cl, beam, noise, tmask, kmask = _notebook(shape, res)
    ny, nx = shape
    full = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    wl, rl = _band(full.Wg, full.Wh)
    wk, rk = _band(full.Fnorm)
    my, mx = band_grid(ny, nx, wl, wk, rl, rk)
    assert (my, mx) == grid
    rng = np.random.default_rng(7)
    tmap = rng.standard_normal(shape)
    kX = np.fft.fft2(tmap)
    kref = full.kappa_ft(kX)
    # the inner estimator: same ell lattice (the N-grid's ell at the same signed index), Nyquist derivative entries zeroed as on any grid
    ly, lx = full.ly[_signed(my) % ny], full.lx[_signed(mx) % nx]
    inner = qo.QEOracleTT.for_timing((my, mx), g.step_y, g.step_x, _crop(full.Wg, my, mx, wl, rl), _crop(full.Wh, my, mx, wl, rl),
                                     _crop(full.Fnorm, my, mx, wk, rk) * (my * mx) / float(ny * nx))
    lyd, lxd = ly.copy(), lx.copy()
    lyd[my // 2] = 0.0
    lxd[mx // 2] = 0.0
    inner.LYd = lyd[:, None] * np.ones((1, mx))
    inner.LXd = np.ones((my, 1)) * lxd[None, :]
    got = inner.kappa_ft(_crop(kX, my, mx, wl, rl))
    # kappa_hat vanishes outside its band on the N grid; inside it the two grids agree
    assert np.array_equal(_crop(_crop(kref, ny, nx, wk, rk), my, mx, wk, rk), _crop(kref, my, mx, wk, rk))
    assert np.abs(kref).sum() == pytest.approx(np.abs(_crop(kref, my, mx, wk, rk)).sum(), rel=1e-14)
    ref_in = _crop(kref, my, mx, wk, rk)
    assert np.abs(got - ref_in).max() <= 1e-12 * np.abs(ref_in).max()


def test_band_grid_rule():
    """engine.band_grid mirrors oa_plan_set_filters' rule on sides 2^a 3^b 5^c."""
    from orphics_amd.engine import BAND_MIN, band_grid
    # notebook filters at 1200^2 / 0.5' (Delta ell = 36): legs 56 x 56, kappa 98 x 98 -> bound 210 -> 256
    assert band_grid(1200, 1200, 56, 98, 56, 98) == (256, 256)
    assert band_grid(2400, 2400, 112, 195, 112, 195) == (512, 512)
    assert band_grid(600, 750, 70, 122, 56, 98) == (256, 512)
    # explicit powers of two: checked against the bound
    assert band_grid(1200, 1200, 56, 98, 56, 98, mrow=512, mcol=1024) == (1024, 512)
    assert band_grid(1200, 1200, 56, 98, 56, 98, mrow=128) is None          # 128 < 210 would alias
    assert band_grid(1200, 1200, 56, 98, 56, 98, mrow=384) is None          # not a power of two
    # the map's own grid, unbounded filters
    assert band_grid(1200, 1200, 56, 98, 56, 98, mrow=0) is None
    assert band_grid(1200, 1200, 56, 98, 56, 98, mcol=0) is None
    assert band_grid(1200, 1200, 0, 98, 56, 98) is None
    assert band_grid(1200, 1200, 56, 98, 56, 0) is None
    # a band too wide for its side: the 480 x 600 patch at 2' (rows: 2 * 118 + 98 = 334 -> 512 >= 480)
    assert band_grid(480, 600, 57, 98, 118, 98) is None
    # at least BAND_MIN points
    assert band_grid(1200, 1200, 10, 10, 10, 10) == (BAND_MIN, BAND_MIN)


def test_band_grid_rule_on_notebook_supports():
    """The supports the estimator derives from the notebook's masks give the inner grids the one-call path runs on."""
    from orphics_amd.engine import band_grid
    for shape, res, grid in (((1200, 1200), 0.5, (256, 256)), ((2400, 2400), 0.5, (512, 512)), ((600, 750), 1.0, (256, 512))):
        g, cl, beam, noise, tmask, kmask = _notebook(shape, res)
        wl, rl = _band(tmask)
        wk, rk = _band(kmask)
        assert band_grid(shape[0], shape[1], wl, wk, rl, rk) == grid, shape
    g, cl, beam, noise, tmask, kmask = _notebook((480, 600), 2.0)
    wl, rl = _band(tmask)
    wk, rk = _band(kmask)
    assert 2 * rl + rk > 256 and band_grid(480, 600, wl, wk, rl, rk) is None


def test_band_grid_rule_keeps_kappa_inside_the_inner_plane():
    """Wherever engine.band_grid returns a grid, it is alias-free AND holds kappa's columns: Mx >= 2 wl + wk, Mx >= 2 wk (so
    Mx // 2 + 1 >= wk: the inner copies of Fnorm / the bin ids and the inner kappa_hat fit the inner hc plane), My >= max(2 rl + rk,
    2 rk), both powers of two below the side.  Swept over band widths and explicit grids on the notebook sides."""
    from orphics_amd.engine import BAND_MIN, band_grid
    widths = (1, 15, 16, 17, 20, 56, 84, 98, 150, 300, 700)
    grids = (-1, 128, 256, 512, 1024, 2048)
    n = 0
    for ny, nx in ((1200, 1200), (2400, 2400), (600, 750), (750, 600)):
        for wl in widths:
            for wk in widths:
                for mrow in grids:
                    for rl, rk, mcol in ((wl, wk, -1), (wk, wl, -1), (wl, wk, 512), (17, 300, -1)):
                        got = band_grid(ny, nx, wl, wk, rl, rk, mrow, mcol)
                        if got is None:
                            continue
                        my, mx = got
                        n += 1
                        assert mx >= 2 * wl + wk and mx >= 2 * wk and mx // 2 + 1 >= wk, (ny, nx, wl, wk, mrow, got)
                        assert my >= 2 * rl + rk and my >= 2 * rk, (ny, nx, rl, rk, mcol, got)
                        for m, side in ((my, ny), (mx, nx)):
                            assert m >= BAND_MIN and m & (m - 1) == 0 and m < side
                        if mrow > 0:
                            assert mx == mrow
                        if mcol > 0:
                            assert my == mcol
    assert n > 500
    # the narrow-leg / wide-kappa filters of the 1200^2 patch at 0.5' with T 100-700, kappa 20-3000 (wl = 20, wk = 84): 2 wl + wk = 124
    # alone would give Mx = 128, whose 65 hc columns cannot hold 84 kappa columns
    assert band_grid(1200, 1200, 20, 84, 20, 84) == (256, 256)
    assert band_grid(1200, 1200, 20, 84, 20, 84, mrow=128) is None


@pytest.mark.parametrize("shape,res,tl,kl,bands,grid", [((1200, 1200), 0.5, (100, 700), (20, 3000), (20, 84), (256, 256)),
                                                       ((2400, 2400), 0.5, (300, 1900), (20, 5400), (106, 300), (1024, 1024))])
def test_band_grid_rule_on_wide_kappa_bands(shape, res, tl, kl, bands, grid):
    """The two geometries whose kappa band is wider than the hc plane of the smallest alias-free grid (the power of two >= 2 wl + wk
    has fewer than wk columns): the grid the rule picks holds kappa's columns."""
    from orphics_amd.engine import band_grid
    g, cl, beam, noise, tmask, kmask = _notebook(shape, res, tl=tl, kl=kl)
    wl, rl = _band(tmask)
    wk, rk = _band(kmask)
    assert (wl, wk) == bands
    alias_only = max(128, 1 << (2 * wl + wk - 1).bit_length())
    assert alias_only // 2 + 1 < wk
    my, mx = band_grid(shape[0], shape[1], wl, wk, rl, rk)
    assert (my, mx) == grid and mx // 2 + 1 >= wk
