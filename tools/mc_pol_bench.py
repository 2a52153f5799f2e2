"""Timing of the polarisation / MV N0 Monte Carlo (mc.GaussianN0MonteCarloPol): the one-call path (oa_mc_run_mv: leg-band draw, the
oa_qe_mv launch sequence, one oa_bin_power_multi pass, one moment launch per realisation) against the host loop of existing entries
(Engine.grf_mix on three full planes, reconstruct_hc per estimator, the weighted sum, Engine.bin_power per spectrum, Statistics.add) --
the way this job was done before the entry existed, so it is the baseline.  Full spectrum list: TT, TE, EE, EB, TB autos, their ten
crosses and the MV auto (16 spectra).

--mode compare (default): both paths in ONE process on the same estimator, ALTERNATED block by block after a warm-up of each; a block
    is --iters consecutive realisations timed with HIP events; per path the median and the 10th .. 90th percentile of --reps blocks
    (at least 7), in ms per realisation.  One JSON line per (side, precision), appended to --out if given.  The two paths' moments of
    the timed realisations are compared as well (max relative difference of the mean sample vector).
--mode onecall N / --mode hostloop N: N realisations of one path and nothing else (the workload for a kernel trace).
--windowed [--mean-field]: every realisation's T, Q, U maps are multiplied by ``maps.get_taper(shape, g, 12.0, 3.0)[0]`` (12 % taper, 3 % pad)
    before their transforms, and -- with --mean-field -- the six kappa_hat stacks are kept: the one call is then oa_mc_run_mv_windowed (full-plane
    draw rotated to T, Q, U, batched inverse columns, one fused C2R x window -> R2C row launch over the three planes, batched forward
    columns, band rotation), the baseline the host loop on the same library and plan (one_call=False: Engine.grf_mix with the rotation,
    Engine.irfft(window=...), Engine.rfft and Engine.rot2, then the sequence above, the stacks added with torch).  The JSON line
    carries "windowed" and "mean_field"; profiles/mc_pol_windowed.jsonl collects these lines."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ESTS = ("TT", "TE", "EE", "EB", "TB")


def setup(n, res):
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (n, n)
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    nP = 2 * nT
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3000)
    q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=nP, kmask_P=tmask, kmask_K=kmask, pol=True,
                     unlensed_equals_lensed=True, dtype="f64")
    cl = {k: th.lCl(k, ml)[:, :n // 2 + 1] for k in ("TT", "EE", "BB", "TE")}
    b2, nTh, nPh = beam[:, :n // 2 + 1] ** 2, nT[:, :n // 2 + 1], nP[:, :n // 2 + 1]
    tot = dict(TT=cl["TT"] * b2 + nTh, EE=cl["EE"] * b2 + nPh, BB=cl["BB"] * b2 + nPh, TE=cl["TE"] * b2)
    return q, tot


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
    ap.add_argument("--sides", default="2048,4096")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--res", type=float, default=0.5, help="pixel size in arcmin")
    ap.add_argument("--iters", type=int, default=8, help="realisations per timed block")
    ap.add_argument("--reps", type=int, default=9, help="timed blocks per path (>= 7)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--windowed", action="store_true", help="apply the 12 %% / 3 %% taper to T, Q, U (oa_mc_run_mv_windowed against its host loop)")
    ap.add_argument("--mean-field", action="store_true", help="with --windowed: keep the mean-field stacks of every estimator and of MV")
    args = ap.parse_args()
    import torch
    from orphics_amd import maps, mc
    mode = args.mode[0]
    if args.mean_field and not args.windowed:
        ap.error("--mean-field goes with --windowed")
    if mode == "compare" and args.reps < 7:
        ap.error("--reps must be at least 7")
    edges = np.linspace(100, 2900, 12)
    for n in [int(s) for s in args.sides.split(",")]:
        q64, tot = setup(n, args.res)
        extra = dict(window=maps.get_taper((n, n), q64.geom, 12.0, 3.0)[0], mean_field=args.mean_field) if args.windowed else {}
        for prec in args.precs.split(","):
            q = q64 if prec == "f64" else q64.astype("f32")
            one = mc.GaussianN0MonteCarloPol(q, tot, edges, estimators=ESTS, base_seed=5, one_call=True, **extra)
            host = mc.GaussianN0MonteCarloPol(q, tot, edges, estimators=ESTS, base_seed=5, one_call=False, **extra)
            if not one.one_call:
                raise SystemExit("side %d has no one-call path" % n)
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
            m1, m0 = one.acc.mean("n0"), host.acc.mean("n0")
            line = dict(tool="mc_pol_bench", side=n, prec=prec, windowed=bool(args.windowed), mean_field=bool(args.mean_field), res_arcmin=args.res, spectra=len(one.spectra), bins=int(one.d),
                        iters=it, reps=args.reps, leg_band=[int(one.wl), int(one.rl)], kappa_band=[int(one.wk), int(one.rk)],
                        onecall_ms=round(float(np.median(t1)), 4),
                        onecall_p10_p90=[round(float(np.percentile(t1, 10)), 4), round(float(np.percentile(t1, 90)), 4)],
                        hostloop_ms=round(float(np.median(t0)), 4),
                        hostloop_p10_p90=[round(float(np.percentile(t0, 10)), 4), round(float(np.percentile(t0, 90)), 4)],
                        speedup=round(float(np.median(t0) / np.median(t1)), 2),
                        max_rel_diff_mean=float(np.max(np.abs(m1 - m0)) / np.max(np.abs(m0))))
            txt = json.dumps(line)
            print(txt, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(txt + "\n")
            del one, host
            q.eng.release_pools()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
