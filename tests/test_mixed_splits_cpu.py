"""CPU: the identity behind oa_qe_tt_split_power (include/orphics_amd.h) in NumPy: the split-based 4-point combination is per Fourier
mode and vanishes outside kappa's band, so combining the n^2 pairwise reconstructions on the band grid's inner plane and mapping the
real result back gives what the reference's ordering of the estimator gives on the map's own grid."""
import numpy as np

from oracle import maps_oracle as mo
from oracle import qe_oracle as qo


def _signed(n):
    return np.fft.fftfreq(n, 1.0 / n).astype(int)


def _band(*planes):
    """(columns, rows) outside which all the FULL planes vanish: columns |kx index| < w, rows |ky index| < r"""
    nz = np.zeros(planes[0].shape, dtype=bool)
    for a in planes:
        nz |= a != 0
    ny, nx = nz.shape
    y, x = np.nonzero(nz)
    return int(np.minimum(x, nx - x).max()) + 1, int(np.minimum(y, ny - y).max()) + 1


def _band_index(shape, my, mx, w, r):
    """rows / columns of the band on the (Ny, Nx) plane, and where they sit on the (my, mx) plane"""
    ky, kx = _signed(shape[0]), _signed(shape[1])
    ys, xs = np.nonzero(np.abs(ky) < r)[0], np.nonzero(np.abs(kx) < w)[0]
    return np.ix_(ys, xs), np.ix_(ky[ys] % my, kx[xs] % mx)


def _combine(K, norm):
    """split_cross_mode (csrc/split_power.hpp) per mode, K[i][j] complex planes of one shape"""
    n = len(K)
    fn = float(n)
    diag = [K[i][i] for i in range(n)]
    rc = [2.0 * diag[i] for i in range(n)]
    tot = sum(diag)
    pij = 0.0
    for i in range(n):
        for j in range(i + 1, n):
            s = K[i][j] + K[j][i]
            rc[i] = rc[i] + s
            rc[j] = rc[j] + s
            tot = tot + s
            pij = pij + np.abs(s) ** 2
    pic = sum(np.abs(rc[i] / (2.0 * fn) - diag[i] / fn) ** 2 for i in range(n))
    kc = (tot - sum(diag)) / fn ** 2
    return (fn ** 4 * np.abs(kc) ** 2 - 4.0 * fn ** 2 * pic + pij) * norm / (fn * (fn - 1.0) * (fn - 2.0) * (fn - 3.0))


def test_split_combination_on_the_inner_grid_equals_the_full_grid_numpy():
    from orphics_amd import cosmology, maps
    from orphics_amd.engine import band_grid
    from orphics_amd.geometry import FlatGeometry
    shape, res, n = (600, 750), 1.0, 4
    g = FlatGeometry.from_res(shape, res)
    ml = g.modlmap()
    cl = cosmology.default_theory().lCl("TT", ml)
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    qr = qo.QEOracleTT(shape, g.step_y, g.step_x, cl, cl, noise, beam, tmask, kmask_K=kmask)
    fo = mo.FourierCalc(shape, g.step_y, g.step_x)
    wl, rl = _band(qr.Wg, qr.Wh)
    wk, rk = _band(qr.Fnorm)
    my, mx = band_grid(shape[0], shape[1], wl, wk, rl, rk)
    assert (my, mx) == (256, 512)
    assert 2 * rk - 1 <= my and wk <= mx // 2 + 1                       # kappa's band fits the inner plane without wrapping onto itself
    rng = np.random.default_rng(21)
    tk = np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cl * beam ** 2 + noise) / g.pixarea)
    tmap = np.fft.ifft2(tk).real
    splits = np.array([np.fft.fft2(tmap + 0.3 * rng.standard_normal(shape)) for _ in range(n)])

    def qfrag(a, b):
        return qr.kappa_from_map("TT", a, T2DDataY=b, alreadyFTed=True, returnFt=True)

    # (i) the reference's ordering on the map's own grid (reconstructions of the mean split included)
    ref = qo.split_cross_estimator(qfrag, fo.f2power, splits)
    # (ii) the n^2 pairwise reconstructions, kappa's band of each on the inner plane (row ky mod My, column kx mod Mx), combined per mode
    # there, the real result mapped back
    on_map, on_inner = _band_index(shape, my, mx, wk, rk)
    K = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            kij = qfrag(splits[i], splits[j])
            inner = np.zeros((my, mx), dtype=kij.dtype)
            inner[on_inner] = kij[on_map]
            K[i][j] = inner
    p_inner = _combine(K, fo.normfact)
    got = np.zeros(shape)
    got[on_map] = p_inner[on_inner]
    outside = np.ones(shape, dtype=bool)
    outside[on_map] = False
    assert np.all(ref[outside] == 0.0) and np.all(got[outside] == 0.0)
    assert np.abs(ref).max() > 0
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
