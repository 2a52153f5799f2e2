"""Timing of the realisation-dependent N0 Monte Carlo of an estimator set and its MV combination (mc.RDN0MonteCarloPol): the one-call
path (oa_rdn0_set_data_mv once, then oa_mc_run_rdn0_mv: per realisation two band draws, one batched leg launch per triple, the chain row
stage over the 2 nest chains, two batched divergences and the three launches of the combine -> bin -> moments tail) against the host loop
of existing entries on the same plan (one_call=False: Engine.grf_mix twice, four Estimator.reconstruct_hc calls per estimator -- the
data's legs filtered and transformed again every time --, the weighted sums in torch, Engine.bin_power per spectrum for A and for B,
Statistics.add) -- the way this job is done without the entry, so it is the baseline.

tools/rdn0_bench.py's protocol: both paths in ONE process on the same estimator, ALTERNATED block by block after a warm-up of each; a
block is --iters consecutive realisations timed with HIP events; per path the median and the 10th .. 90th percentile of --reps blocks (at
least 7), in ms per realisation.  One JSON line per (geometry, precision), appended to --out if given.  The two paths' mean sample
vectors of the timed realisations are compared as well (largest difference over the largest |mean|).
--mode onecall N / --mode hostloop N: N realisations of one path and nothing else (the workload for a kernel trace).
--geoms: comma-separated NYxNX@RES entries, RES in arcmin (default: 2048x2048@1 and 4096x4096@0.5).  Five estimators, their ten
crosses, the MV auto; 19 bins."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ESTS = ("TT", "TE", "EE", "EB", "TB")


def setup(shape, res):
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    nP = 2 * nT
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask,
                     kmask_K=maps.mask_kspace(shape, g, lmin=20, lmax=3500), pol=True, unlensed_equals_lensed=True, dtype="f64")
    nxh = shape[1] // 2
    cl = {k: th.lCl(k, ml) for k in ("TT", "EE", "BB", "TE")}
    tot = dict(TT=cl["TT"] * beam ** 2 + nT, EE=cl["EE"] * beam ** 2 + nP, BB=cl["BB"] * beam ** 2 + nP, TE=cl["TE"] * beam ** 2)
    return q, {k: np.ascontiguousarray(v[:, :nxh + 1]) for k, v in tot.items()}


def block_ms(drv, lo, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    drv.run_local(range(lo, lo + iters))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", nargs="+", default=["compare"], help="compare | onecall N | hostloop N")
    ap.add_argument("--geoms", default="2048x2048@1,4096x4096@0.5")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--iters", type=int, default=6, help="realisations per timed block")
    ap.add_argument("--reps", type=int, default=7, help="timed blocks per path (>= 7)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    from orphics_amd import mc
    mode = args.mode[0]
    if mode == "compare" and args.reps < 7:
        ap.error("--reps must be at least 7")
    edges = np.linspace(20, 3500, 20)
    for spec in args.geoms.split(","):
        sides, res = spec.split("@")
        shape = tuple(int(s) for s in sides.split("x"))
        q64, tot = setup(shape, float(res))
        for prec in args.precs.split(","):
            q = q64 if prec == "f64" else q64.astype("f32")
            e = q.eng
            one = mc.RDN0MonteCarloPol(q, [e.hc(), e.hc(), e.hc()], tot, edges, estimators=ESTS, base_seed=5, one_call=True)
            data = e.grf_mix(17, one.cs, stream_id0=10 ** 6)
            one.set_data(data)
            host = mc.RDN0MonteCarloPol(q, data, tot, edges, estimators=ESTS, base_seed=5, one_call=False)
            if mode in ("onecall", "hostloop"):
                (one if mode == "onecall" else host).run_local(range(int(args.mode[1])))
                torch.cuda.synchronize()
                continue
            it = args.iters
            for drv in (one, host):                   # warm-up of each path: allocations, first-use tables, clocks
                drv.run_local(range(0, it))
            torch.cuda.synchronize()
            t1, t0 = [], []
            for r in range(args.reps):                # alternated block by block, the same realisations for both
                lo = (r + 1) * it
                t1.append(block_ms(one, lo, it))
                t0.append(block_ms(host, lo, it))
            one.acc.allreduce(); host.acc.allreduce()
            m1, m0 = one.acc.mean("rdn0"), host.acc.mean("rdn0")
            wl, wk, rl, rk = one._set._bands
            line = dict(tool="rdn0_pol_bench", shape=list(shape), prec=prec, res_arcmin=float(res), estimators=list(ESTS), nspec=one.nspec,
                        bins=int(one.d), iters=it, reps=args.reps, leg_band=[int(wl), int(rl)], kappa_band=[int(wk), int(rk)],
                        onecall_ms=round(float(np.median(t1)), 4),
                        onecall_p10_p90=[round(float(np.percentile(t1, 10)), 4), round(float(np.percentile(t1, 90)), 4)],
                        hostloop_ms=round(float(np.median(t0)), 4),
                        hostloop_p10_p90=[round(float(np.percentile(t0, 10)), 4), round(float(np.percentile(t0, 90)), 4)],
                        speedup=round(float(np.median(t0) / np.median(t1)), 2),
                        max_diff_mean_over_max_mean=float(np.max(np.abs(m1 - m0)) / np.max(np.abs(m0))))
            txt = json.dumps(line)
            print(txt, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(txt + "\n")
            del one, host
            e.release_pools()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
