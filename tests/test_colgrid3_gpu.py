"""The from-map TT path on a 3 x 2^k column grid (include/orphics_amd.h, COLUMN GRID / FROM-MAP GRID): 8192^2 maps run the coarse side of
the R-split path on 1536 rows, 4096^2 maps on 768, where the band limits fit.  Same kappa_hat as on the power-of-two grid and on the
map's own rows, same moments from the one- and two-map entries; every other entry of the plan keeps the power-of-two grid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(N, tlmax=2000, seed=5):
    from orphics_amd import cosmology, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (N, N)
    g = FlatGeometry.from_res(shape, 0.5)
    th = cosmology.default_theory()
    ml = g.modlmap()
    kw = dict(noise2d=np.full(shape, cosmology.white_noise_power(1.0)), beam2d=maps.gauss_beam(ml, 1.5),
              kmask=maps.mask_kspace(shape, g, lmin=300, lmax=tlmax), kmask_K=maps.mask_kspace(shape, g, lmin=20, lmax=3500),
              unlensed_equals_lensed=True)
    rng = np.random.default_rng(seed)
    return shape, g, th, kw, rng


@pytest.mark.parametrize("N,my3", [(4096, 768), (8192, 1536)])
def test_from_map_grid_is_exact(N, my3):
    """automatic grid (3 x 2^k) == col_grid = the power of two == col_grid="full", from a map into a dirty plane (1e-12 / 2e-6 of the plane's
    maximum, as test_column_grid_is_exact); the plan reports 3 x 2^k rows, R = 4, the fused divergence"""
    from orphics_amd import lensing
    shape, g, th, kw, rng = _setup(N)
    my2 = my3 // 3 * 4
    for prec, tol in (("f64", 1e-12), ("f32", 2e-6)):
        qa = lensing.qest(shape, g, th, dtype=prec, **kw)
        q2 = lensing.qest(shape, g, th, dtype=prec, col_grid=my2, **kw)
        q3 = lensing.qest(shape, g, th, dtype=prec, col_grid=my3, **kw)
        qf = lensing.qest(shape, g, th, dtype=prec, col_grid="full", **kw)
        e = qa.eng
        x = e.to_real(rng.standard_normal(shape))
        rl, rk = qa.leg_rows, qa.kappa_rows
        assert max(2 * rl + rk, 2 * rk) <= my3
        full = qf.reconstruct_tt_from_map(x).clone()
        assert qf.col_grid == 0
        scale = float(full.abs().max())
        ref2 = q2.reconstruct_tt_from_map(x).clone()
        assert q2.col_grid == my2
        assert int(e.lib.oa_plan_rsplit(e.plan)) == 4
        dirty = e.hc(); dirty[:] = 3.0
        rec = qa.reconstruct_tt_from_map(x, out=dirty).clone()
        assert qa.col_grid == my3
        assert int(e.lib.oa_plan_rsplit(e.plan)) == 4
        for other in (full, ref2):
            err = float((rec - other).abs().max()) / scale
            print("N = %d %s: automatic grid %d vs %s: %.3g" % (N, prec, my3, "full" if other is full else my2, err))
            assert err < tol
        assert bool((rec[rk:N - rk + 1] == 0).all()) and bool((rec[:, qa.kappa_cols:] == 0).all())
        rec3 = q3.reconstruct_tt_from_map(x)
        assert q3.col_grid == my3
        assert float((rec3 - full).abs().max()) / scale < tol
        # Fourier-space legs on the same plan: the power-of-two grid, output unchanged from the explicit power-of-two handle's
        kX = e.rfft(x)
        a = qa.reconstruct_tt_hc(kX).clone()
        b = q2.reconstruct_tt_hc(kX).clone()
        assert bool((a == b).all())
        assert float((a - full).abs().max()) / scale < tol
        del qa, q2, q3, qf


@pytest.mark.parametrize("N", [4096, 8192])
def test_from_map_grid_moments(N):
    """tt_moments2 == per-map tt_moments == bandpowers of the stored kappa_hat (1e-9 / 2e-6 relative, the bench's check), on the
    automatic 3 x 2^k grid and against the power-of-two grid; the fused divergence + binning launch is the one that runs"""
    from orphics_amd import lensing
    shape, g, th, kw, rng = _setup(N, seed=6)
    edges = np.linspace(20, 3500, 20)
    d = len(edges) - 1
    for prec, tol in (("f64", 1e-9), ("f32", 2e-6)):
        res = {}
        for grid in ("auto", N // 4):
            q = lensing.qest(shape, g, th, dtype=prec, col_grid=grid, **kw)
            e = q.eng
            if "x0" not in res:
                res["x0"] = e.to_real(rng.standard_normal(shape)); res["x1"] = e.to_real(rng.standard_normal(shape))
            x0, x1 = res["x0"], res["x1"]
            ids = e.modl_digitize(torch.as_tensor(edges, device=e.device), half=True)
            pn = g.area / float(N * N) ** 2
            q.bind_bins(ids, len(edges) + 1, pn)
            assert q.col_grid == (3 * N // 16 if grid == "auto" else N // 4)
            eb = q._bind_bins()                      # (bind_bins is lazy: the plan learns its bins here)
            assert int(eb.lib.oa_plan_div_fused(eb.plan)) == 1
            n = torch.zeros(1, dtype=torch.int64, device=e.device)
            S = torch.zeros(d, dtype=torch.float64, device=e.device)
            C = torch.zeros(d, d, dtype=torch.float64, device=e.device)
            q.tt_moments2(x0, x1, n, S, C)
            n1 = torch.zeros_like(n); S1 = torch.zeros_like(S); C1 = torch.zeros_like(C)
            q.tt_moments(x0, n1, S1, C1)
            q.tt_moments(x1, n1, S1, C1)
            bs = []
            for x in (x0, x1):
                kk = q.reconstruct_tt_from_map(x)
                sums, _ = e.bin_power(kk, kk, pn, ids, len(edges) + 1, herm=True, active_cols=q.kappa_cols, active_rows=q.kappa_rows)
                bs.append((sums[1:-1] / q.bin_counts()[1:-1].double()).cpu().numpy())
            torch.cuda.synchronize()
            assert int(n.item()) == 2 and int(n1.item()) == 2
            S_, S1_, C_, C1_ = (t.cpu().numpy() for t in (S, S1, C, C1))
            eS, eC = np.max(np.abs(S_ / S1_ - 1)), np.max(np.abs(C_ / C1_ - 1))
            eB = np.max(np.abs(S_ / (bs[0] + bs[1]) - 1))
            print("N = %d %s grid %s: moments2 vs moments %.3g %.3g, vs bandpowers %.3g" % (N, prec, grid, eS, eC, eB))
            assert eS < tol and eC < 2 * tol and eB < tol
            res[grid] = S_
            del q
        eG = np.max(np.abs(res["auto"] / res[N // 4] - 1))
        print("N = %d %s: 3 x 2^k grid vs power of two: %.3g" % (N, prec, eG))
        assert eG < tol


def test_from_map_grid_falls_back_and_refuses():
    """a band whose alias-free bound exceeds 1536 rows keeps 2048; an explicit 3 x 2^k grid below the bound, or on a geometry without the
    path, is refused with a message"""
    from orphics_amd import lensing
    from orphics_amd._lib import OrphicsAmdError
    N = 8192
    shape, g, th, kw, rng = _setup(N, tlmax=2400)
    q = lensing.qest(shape, g, th, dtype="f32", **kw)
    x = q.eng.to_real(rng.standard_normal(shape))
    q.reconstruct_tt_from_map(x)
    need = max(2 * q.leg_rows + q.kappa_rows, 2 * q.kappa_rows)
    assert need > 1536 and q.col_grid == 2048, (need, q.col_grid)
    qbad = lensing.qest(shape, g, th, dtype="f32", col_grid=1536, **kw)
    with pytest.raises(OrphicsAmdError):
        qbad.reconstruct_tt_from_map(x)
    del q, qbad, x
    # 2048^2: no R-split from-map path -> no 3 x 2^k grid (the automatic grid is the power of two, as before)
    N = 2048
    shape, g, th, kw, rng = _setup(N)
    q = lensing.qest(shape, g, th, dtype="f64", **kw)
    x = q.eng.to_real(rng.standard_normal(shape))
    q.reconstruct_tt_from_map(x)
    assert q.col_grid == 0 or (q.col_grid & (q.col_grid - 1)) == 0
    qbad = lensing.qest(shape, g, th, dtype="f64", col_grid=384, **kw)
    with pytest.raises(OrphicsAmdError):
        qbad.reconstruct_tt_from_map(x)


def test_other_entries_keep_the_power_of_two_grid():
    """pol, MV and the N0 Monte-Carlo entry on a plan whose from-map path runs on 1536 rows: bit-identical to the same calls on a handle with
    the explicit power-of-two grid"""
    from orphics_amd import cosmology, lensing, maps
    N = 8192
    shape, g, th, kw, rng = _setup(N, seed=8)
    kw = dict(kw, noise2d_P=2 * kw["noise2d"], kmask_P=kw["kmask"], pol=True)
    qa = lensing.qest(shape, g, th, dtype="f32", **kw)
    q2 = lensing.qest(shape, g, th, dtype="f32", col_grid=2048, **kw)
    e = qa.eng
    x = e.to_real(rng.standard_normal(shape))
    qa.reconstruct_tt_from_map(x)
    assert qa.col_grid == 1536
    kT, kE, kB = [e.rfft(e.to_real(rng.standard_normal(shape))) for _ in range(3)]
    for XY, f in (("TE", (kT, kE)), ("EB", (kE, kB))):
        a = qa.reconstruct_hc(XY, *f).clone()
        b = q2.reconstruct_hc(XY, *f).clone()
        assert bool((a == b).all()), XY
    a = qa.reconstruct_mv_hc(kT, kE, kB).clone()
    b = q2.reconstruct_mv_hc(kT, kE, kB).clone()
    assert bool((a == b).all())
    del kT, kE, kB, a, b
    # N0 Monte Carlo (oa_mc_run): the same realisations, bit-identical bandpower moments
    from orphics_amd import mc
    ml = g.modlmap()[:, :N // 2 + 1]
    tot_h = th.lCl("TT", ml) * kw["beam2d"][:, :N // 2 + 1] ** 2 + kw["noise2d"][:, :N // 2 + 1]
    edges = np.linspace(20, 3500, 20)
    sa = mc.GaussianN0MonteCarlo(qa, tot_h, edges, base_seed=3).run(6)
    assert qa.col_grid == 1536
    sb = mc.GaussianN0MonteCarlo(q2, tot_h, edges, base_seed=3).run(6)
    assert sa.count("n0") == 6 and np.array_equal(sa.mean("n0"), sb.mean("n0")) and np.array_equal(sa.cov("n0"), sb.cov("n0"))
