#!/usr/bin/env python
"""Every one-call Monte-Carlo entry through its Python driver at a fixed seed, n / S / C and every mean-field stack written to one .npz:
the bit-identity evidence of a change that must not alter what the sequencers launch (csrc/pipeline.hip).  Run it on the two builds
(ORPHICS_AMD_LIB selects the library) and compare:

    python tools/mc_entries_dump.py --out a.npz          # build A
    python tools/mc_entries_dump.py --out b.npz          # build B
    python tools/mc_entries_dump.py --compare a.npz b.npz    # one line per case, exit status 1 on any difference

Cases (8 realisations, f32 and f64): oa_mc_run / oa_mc_run_windowed on 2048^2 at 1' (batched row stage; batches of 1, 4, 6 / fused row
pass on and off) and 512^2 at 2' (falls back to one by one), and on the band grids of 300 x 1200 (batched) and 300 x 360 (not batched) at
2'; oa_mc_run_mv / oa_mc_run_mv_windowed on 256^2 and 128 x 256 at 2' and on the band grids of 300 x 360 and 300 x 750 at 1', windowed
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

    def keep(case, drv, labels):
        n, S, C = drv.acc.device_moments("n0", getattr(drv, "D", getattr(drv, "d", None)))
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
