"""Timing of the realisation-dependent N0 Monte Carlo of the TT estimator (mc.RDN0MonteCarlo): the one-call path (oa_rdn0_set_data once,
then oa_mc_run_rdn0: per batch one draw launch of 2 B leg bands, two leg launches over the simulations' fields only, one chain row-stage
launch, one divergence launch and the two launches of the combine -> bin -> moments tail) against the host loop of existing entries on the
same plan (one_call=False: Engine.grf_hc twice on the leg band, Estimator.reconstruct_tt_sym_hc twice -- four oa_qe_tt calls and two sums,
the data's legs filtered and transformed again every time --, Engine.bin_power twice, Statistics.add) -- the way this job is done without
the entry, so it is the baseline.

--mode compare (default): both paths in ONE process on the same estimator, ALTERNATED block by block after a warm-up of each; a block is
    --iters consecutive realisations timed with HIP events; per path the median and the 10th .. 90th percentile of --reps blocks (at
    least 7), in ms per realisation.  One JSON line per (geometry, precision), appended to --out if given.  The two paths' mean sample
    vectors of the timed realisations are compared as well (largest difference over the largest mean p(A) bandpower).
--mode onecall N / --mode hostloop N: N realisations of one path and nothing else (the workload for a kernel trace).
--geoms: comma-separated NYxNX@RES entries, RES in arcmin (default: 2048x2048@1, 4096x4096@0.5 and the band grid 1200x1200@1).
--windowed: the same protocol for the windowed driver (mc.RDN0MonteCarlo(window=taper): oa_mc_run_rdn0_windowed against the host loop
    Engine.grf_hc -> irfft -> x window -> rfft for both draws, then the sequence above), blocks of 6 realisations, 7 blocks per path;
    default geometries 2048x2048@1, 4096x4096@0.5 (power of two) and 1200x1200@0.5, 2400x2400@0.5 (band grid).  On power-of-two sides the one
    call is timed with OA_OPT_DRAW_FUSED = 1 and = 0 (alternated with the host loop), and oa_grf_hc_icols alone (two planes per launch)
    against oa_grf_hc + oa_fft_cols alone (per plane), alternated blocks of HIP-event-timed launches, in microseconds per drawn plane."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(shape, res):
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=maps.mask_kspace(shape, g, lmin=300, lmax=2000),
                     kmask_K=maps.mask_kspace(shape, g, lmin=20, lmax=3500), unlensed_equals_lensed=True, dtype="f64")
    return q, (th.lCl("TT", ml) * beam ** 2 + noise)[:, :shape[1] // 2 + 1]


def block_ms(drv, lo, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    drv.run_local(range(lo, lo + iters))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def pct(t):
    return [round(float(np.percentile(t, 10)), 4), round(float(np.percentile(t, 90)), 4)]


def events_us(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def windowed(args, shape, res, q64, tot):
    """one JSON line per precision: one call (draw_fused 1 / 0 on power-of-two sides) against the host loop, and the draw kernels alone"""
    import torch
    from orphics_amd import maps, mc
    edges = np.linspace(20, 3500, 20)
    taper = maps.get_taper(shape, q64.geom, 12.0, 3.0)[0]
    it, reps = args.iters or 6, args.reps or 7
    for prec in args.precs.split(","):
        q = q64 if prec == "f64" else q64.astype("f32")
        e = q.eng
        cs = q._hcreal(e, np.sqrt(tot * float(e.npix) ** 2 / q.geom.area))
        data = e.rfft(e.irfft(e.grf_hc(17, 10 ** 6, cs)) * e.to_real(taper))              # the data as analysed: apodised
        one = mc.RDN0MonteCarlo(q, data, tot, edges, base_seed=5, one_call=True, window=taper)
        host = mc.RDN0MonteCarlo(q, data, tot, edges, base_seed=5, one_call=False, window=taper)
        paths = [("onecall_draw_fused1", one, 1), ("onecall_draw_fused0", one, 0)] if e.pow2 else [("onecall", one, -1)]
        paths.append(("hostloop", host, -1))
        for _, drv, dfu in paths:                     # warm-up of each path: allocations, first-use tables, clocks
            e.set_option("draw_fused", dfu)
            drv.run_local(range(0, it))
        torch.cuda.synchronize()
        t = {name: [] for name, _, _ in paths}
        for r in range(reps):                         # alternated block by block, the same realisations for every path
            for name, drv, dfu in paths:
                e.set_option("draw_fused", dfu)
                t[name].append(block_ms(drv, (r + 1) * it, it))
        e.set_option("draw_fused", -1)
        one.acc.allreduce(); host.acc.allreduce()
        m1, m0 = one.acc.mean("rdn0"), host.acc.mean("rdn0")
        d = one.d
        line = dict(tool="rdn0_bench", windowed=True, shape=list(shape), prec=prec, res_arcmin=float(res), bins=int(d), band_grid=list(q.band_grid),
                    iters=it, reps=reps, leg_band=[int(q.leg_cols), int(q.leg_rows)], kappa_band=[int(q.kappa_cols), int(q.kappa_rows)],
                    batched=int(e.lib.oa_plan_rdn0_batched(q._bind_bins().plan)))
        for name in t:
            line[name + "_ms"] = round(float(np.median(t[name])), 4)
            line[name + "_p10_p90"] = pct(t[name])
        best = min(float(np.median(t[name])) for name in t if name != "hostloop")
        line["speedup"] = round(float(np.median(t["hostloop"])) / best, 2)
        line["max_diff_mean_over_pA"] = float(np.max(np.abs(m1 - m0)) / np.max(m0[:d] + m0[d:]))
        if e.pow2:                                    # the draw kernels alone, microseconds per drawn plane
            w = e.nx // 2 + 1
            buf, dr, co = e.hc(2), e.hc(), e.hc()
            fused = lambda: e.grf_hc_icols(5, 0, cs, nreal=2, out=buf)
            def unfused():
                for z in range(2):
                    e.grf_hc(5, z, cs, out=dr)
                    e.fft_cols(dr, inverse=True, out=co, width=w)
            draw_only = lambda: (e.grf_hc(5, 0, cs, out=dr), e.grf_hc(5, 1, cs, out=dr))
            k = {"icols_us": [], "grf_then_cols_us": [], "grf_only_us": []}
            for f in (fused, unfused, draw_only):
                events_us(f, 5)
            for r in range(reps):
                k["icols_us"].append(events_us(fused, 20) / 2)
                k["grf_then_cols_us"].append(events_us(unfused, 20) / 2)
                k["grf_only_us"].append(events_us(draw_only, 20) / 2)
            for name in k:
                line[name] = round(float(np.median(k[name])), 2)
                line[name + "_p10_p90"] = [round(x, 2) for x in pct(k[name])]
            del buf, dr, co
        txt = json.dumps(line)
        print(txt, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(txt + "\n")
        del one, host
        e.release_pools()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", nargs="+", default=["compare"], help="compare | onecall N | hostloop N")
    ap.add_argument("--geoms", default=None)
    ap.add_argument("--windowed", action="store_true", help="the windowed driver (see above)")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--iters", type=int, default=None, help="realisations per timed block (default 12; --windowed: 6)")
    ap.add_argument("--reps", type=int, default=None, help="timed blocks per path (>= 7; default 9; --windowed: 7)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    from orphics_amd import mc
    mode = args.mode[0]
    if mode == "compare" and args.reps is not None and args.reps < 7:
        ap.error("--reps must be at least 7")
    if args.geoms is None:
        args.geoms = "2048x2048@1,4096x4096@0.5,1200x1200@0.5,2400x2400@0.5" if args.windowed else "2048x2048@1,4096x4096@0.5,1200x1200@1"
    edges = np.linspace(20, 3500, 20)
    for spec in args.geoms.split(","):
        sides, res = spec.split("@")
        shape = tuple(int(s) for s in sides.split("x"))
        q64, tot = setup(shape, float(res))
        if args.windowed:
            windowed(args, shape, res, q64, tot)
            continue
        args.iters, args.reps = args.iters or 12, args.reps or 9
        for prec in args.precs.split(","):
            q = q64 if prec == "f64" else q64.astype("f32")
            e = q.eng
            data = e.grf_hc(17, 10 ** 6, q._hcreal(e, np.sqrt(tot * float(e.npix) ** 2 / q.geom.area)))
            one = mc.RDN0MonteCarlo(q, data, tot, edges, base_seed=5, one_call=True)
            host = mc.RDN0MonteCarlo(q, data, tot, edges, base_seed=5, one_call=False)
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
            d = one.d
            line = dict(tool="rdn0_bench", shape=list(shape), prec=prec, res_arcmin=float(res), bins=int(d), band_grid=list(q.band_grid),
                        iters=it, reps=args.reps, leg_band=[int(q.leg_cols), int(q.leg_rows)], kappa_band=[int(q.kappa_cols), int(q.kappa_rows)],
                        onecall_ms=round(float(np.median(t1)), 4),
                        onecall_p10_p90=[round(float(np.percentile(t1, 10)), 4), round(float(np.percentile(t1, 90)), 4)],
                        hostloop_ms=round(float(np.median(t0)), 4),
                        hostloop_p10_p90=[round(float(np.percentile(t0, 10)), 4), round(float(np.percentile(t0, 90)), 4)],
                        speedup=round(float(np.median(t0) / np.median(t1)), 2),
                        max_diff_mean_over_pA=float(np.max(np.abs(m1 - m0)) / np.max(m0[:d] + m0[d:])))
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
