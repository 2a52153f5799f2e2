#!/usr/bin/env python
"""Every one-call Monte-Carlo entry through its Python driver at a fixed seed, n / S / C and every mean-field stack written to one .npz:
the bit-identity evidence of a change that must not alter what the sequencers launch (csrc/pipeline.hip).  Run it on the two builds
(ORPHICS_AMD_LIB selects the library) and compare:

    python tools/mc_entries_dump.py --out a.npz          # build A
    python tools/mc_entries_dump.py --out b.npz          # build B
    python tools/mc_entries_dump.py --compare a.npz b.npz    # one line per case, exit status 1 on any difference

Cases (8 realisations, f32 and f64): oa_mc_run / oa_mc_run_windowed on 2048^2 at 1' (batched row stage; batches of 1, 4, 6 / fused row
pass on and off) and 512^2 at 2' (falls back to one by one), and on the band grids of 300 x 1200 (batched) and 300 x 360 (not batched) at
2'; oa_mc_run_rdn0 / oa_mc_run_rdn0_windowed (mc.RDN0MonteCarlo, one_call=True) on the same four geometries, without a window and with the
taper at the same batch sizes, and with the taper at OA_OPT_WIN_FUSED 1 / 0 and, on the power-of-two sides, OA_OPT_DRAW_FUSED 1 / 0, each
with oa_plan_rdn0_batched + 1 as one more array; oa_mc_run_rdn0_mv on 256^2 at 2'; oa_mc_run_mv / oa_mc_run_mv_windowed on 256^2 and 128 x 256 at 2' and on the band grids of 300 x 360 and 300 x 750 at 1', windowed
with the taper + stacks and without a window + stacks."""
import argparse
import sys

import numpy as np

NS, SEED = 8, 4242


def compare(a, b):
    A, B = np.load(a), np.load(b)
    cases, bad = sorted({k.rsplit("/", 1)[0] for k in A.files} | {k.rsplit("/", 1)[0] for k in B.files}), 0
    for c in cases:
        ka, kb = [k for k in A.files if k.rsplit("/", 1)[0] == c], [k for k in B.files if k.rsplit("/", 1)[0] == c]
        ok = sorted(ka) == sorted(kb) and all(np.array_equal(A[k], B[k]) and np.any(A[k]) for k in ka)      # (an all-zero array proves nothing)
        bad += not ok
        print("%-44s %2d arrays %s" % (c, len(ka), "equal" if ok else "DIFFERENT"))
    print("%d cases, %d different" % (len(cases), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from orphics_amd import _lib, cosmology, lensing, maps, mc
    from orphics_amd.geometry import FlatGeometry
    print("library:", _lib.LIB_PATH, flush=True)
    out = {}

    def geometry(shape, res, kmax):
        g = FlatGeometry.from_res(shape, res)
        th, ml = cosmology.default_theory(), g.modlmap()
        beam, nT = maps.gauss_beam(ml, 1.5), np.full(shape, cosmology.white_noise_power(1.0))
        tmask, kmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000), maps.mask_kspace(shape, g, lmin=20, lmax=kmax)
        tot = dict(TT=th.lCl("TT", ml) * beam ** 2 + nT, EE=th.lCl("EE", ml) * beam ** 2 + 2 * nT, BB=th.lCl("BB", ml) * beam ** 2 + 2 * nT,
                   TE=th.lCl("TE", ml) * beam ** 2)
        tot_h = {k: np.ascontiguousarray(v[:, :shape[1] // 2 + 1]) for k, v in tot.items()}
        return g, th, beam, nT, tmask, kmask, tot_h, np.asarray(maps.get_taper(shape, g, 12.0, 3.0)[0], dtype=np.float64)

    def keep(case, drv, labels, label="n0", dim=None):
        n, S, C = drv.acc.device_moments(label, dim or getattr(drv, "D", getattr(drv, "d", None)))
        out[case + "/n"], out[case + "/S"], out[case + "/C"] = n.cpu().numpy(), S.cpu().numpy(), C.cpu().numpy()
        e = drv.eng
        for lab in labels:
            out[case + "/" + lab] = drv.acc.device_stack(lab, (e.ny, e.kp, 2)).cpu().numpy()
        print(case, int(n.item()), flush=True)

    # ---- oa_mc_run, oa_mc_run_windowed
    edges = np.linspace(100, 3000, 12)
    for shape, res, batches in (((2048, 2048), 1.0, (1, 4, 6)), ((512, 512), 2.0, (0,)), ((300, 1200), 2.0, (0,)), ((300, 360), 2.0, (0,))):
        g, th, beam, nT, tmask, kmask, tot_h, taper = geometry(shape, res, 3500)
        for prec in ("f32", "f64"):
            q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype=prec)
            name = "tt %dx%d %s" % (shape + (prec,))
            for b in batches:
                q.eng.set_option("mc_batch", b)
                keep("%s batch %d" % (name, b), mc.GaussianN0MonteCarlo(q, tot_h["TT"], edges, base_seed=SEED, mean_field=True).run_local(range(NS)), ["mf"])
            q.eng.set_option("mc_batch", 0)
            for fused in (1, 0):
                q.eng.set_option("win_fused", fused)
                drv = mc.GaussianN0MonteCarlo(q, tot_h["TT"], edges, base_seed=SEED, mean_field=True, window=taper, one_call=True)
                keep("%s windowed fused %d" % (name, fused), drv.run_local(range(NS)), ["mf"])
            q.eng.set_option("win_fused", -1)
            # ---- oa_mc_run_rdn0, oa_mc_run_rdn0_windowed on the same plan: which path the call took (+ 1) is one more array
            e = q.eng
            draw = e.grf_hc(17, 10 ** 6, q._hcreal(e, np.sqrt(tot_h["TT"] * float(e.npix) ** 2 / g.area)))
            pow2 = bool(e.pow2)

            def rdn0(case, w, **opts):
                for k, v in opts.items():
                    e.set_option(k, v)
                data = draw if w is None else e.rfft(e.irfft(draw) * e.to_real(w))          # the data as analysed: apodised
                drv = mc.RDN0MonteCarlo(q, data, tot_h["TT"], edges, base_seed=SEED, one_call=True, window=w).run_local(range(NS))
                keep("rdn0 " + name[3:] + " " + case, drv, [], "rdn0", 2 * drv.d)
                out["rdn0 " + name[3:] + " " + case + "/batched"] = np.array([1 + e.lib.oa_plan_rdn0_batched(q._bind_bins().plan)])
                for k in opts:
                    e.set_option(k, 0 if k == "mc_batch" else -1)
            for wname, w in (("plain", None), ("windowed", taper)):
                for b in batches:
                    rdn0("%s batch %d" % (wname, b), w, mc_batch=b)
            for fused in (1, 0):
                rdn0("windowed fused %d" % fused, taper, win_fused=fused)
                if pow2:
                    rdn0("windowed draw_fused %d" % fused, taper, draw_fused=fused)
            del q, e
    # ---- oa_mc_run_rdn0_mv: not touched by a change to the TT entries, and shown so
    g, th, beam, nT, tmask, kmask, tot_h, taper = geometry((256, 256), 2.0, 3000)
    for prec in ("f32", "f64"):
        q = lensing.qest((256, 256), g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=2 * nT, kmask_P=tmask, kmask_K=kmask, pol=True,
                         unlensed_equals_lensed=True, dtype=prec)
        drv = mc.RDN0MonteCarloPol(q, [q.eng.hc()] * 3, tot_h, np.linspace(100, 2900, 12), base_seed=SEED, one_call=True)
        keep("rdn0 mv 256x256 %s" % prec, drv.set_data(q.eng.grf_mix(17, drv.cs, stream_id0=10 ** 6)).run_local(range(NS)), [], "rdn0")
        del q
    # ---- oa_mc_run_mv, oa_mc_run_mv_windowed
    edges = np.linspace(100, 2900, 12)
    for shape, res in (((256, 256), 2.0), ((128, 256), 2.0), ((300, 360), 1.0), ((300, 750), 1.0)):
        g, th, beam, nT, tmask, kmask, tot_h, taper = geometry(shape, res, 3000)
        band = not (shape[0] & (shape[0] - 1) == 0 and shape[1] & (shape[1] - 1) == 0)
        for prec in ("f32", "f64"):
            q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=2 * nT, kmask_P=tmask, kmask_K=kmask, pol=True,
                             unlensed_equals_lensed=True, dtype=prec)
            name = "mv %dx%d %s" % (shape + (prec,))
            kw = dict(base_seed=SEED, one_call="band" if band else None)
            keep(name, mc.GaussianN0MonteCarloPol(q, tot_h, edges, **kw).run_local(range(NS)), [])
            for fused in ((1, 0) if band else (-1,)):
                q.eng.set_option("win_fused", fused)
                for w in (taper, None):
                    drv = mc.GaussianN0MonteCarloPol(q, tot_h, edges, window=w, mean_field=True, **kw).run_local(range(NS))
                    keep("%s %s fused %d" % (name, "windowed" if w is not None else "stacks only", fused), drv, drv.mf_labels)
            q.eng.set_option("win_fused", -1)
            del q
    np.savez_compressed(a.out, **out)             # (the stacks vanish outside kappa's band)


if __name__ == "__main__":
    main()
