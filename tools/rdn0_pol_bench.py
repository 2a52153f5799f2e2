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
crosses, the MV auto; 19 bins.
--windowed: the same protocol for the windowed driver (RDN0MonteCarloPol.set_window(taper)), every path in one process on the same plan,
    blocks of --iters (6) realisations alternated, 7 blocks per path: oa_mc_run_rdn0_mv_windowed with OA_OPT_DRAW_FUSED = 1 and = 0, the
    windowed host loop (Engine.grf_mix(rot) -> irfft x window -> rfft -> rot2 for both triples, then the sequence above), and the
    unwindowed oa_mc_run_rdn0_mv as the cost of everything behind the source stage.  Stand-alone, in microseconds per triple:
    oa_grf_mix_icols (two triples per launch), oa_grf_mix(rot) + the batched inverse columns of its three planes, and that draw alone.
--band: the same protocol on map sides 2^a 3^b 5^c (default --geoms 1200x1200@1,2400x2400@0.5): one_call="band" (oa_qe_band_bind,
    oa_mc_mv_band_bind and oa_rdn0_set_data_mv once, then oa_mc_run_rdn0_mv on the band grid) against one_call=False on the same plan,
    blocks alternated, the bindings of each path re-made by its own first block after the other's (that set-up is inside the block: it is
    what alternating costs, and a production run pays it once); "onecall_steady" is the one call in blocks of its own with nothing in
    between.
    Stand-alone on the inner grid, in microseconds per realisation: the six planes of s and s' by ONE oa_grf_mix_band_inner_triples launch
    and by TWO oa_grf_mix_band_inner launches; "onecall_two_draws_ms" is the one call's time with the difference added -- the
    per-realisation time had the shard kept two single-triple launches (derived: the library has no switch for it)."""
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


def pct(t, nd=4):
    return [round(float(np.percentile(t, 10)), nd), round(float(np.percentile(t, 90)), nd)]


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
    """one JSON line per precision: the windowed one call (draw_fused 1 / 0), the windowed host loop, the unwindowed one call; the draw
    kernels alone"""
    import ctypes
    import torch
    from orphics_amd import maps, mc
    from orphics_amd._lib import check
    from orphics_amd.engine import _ptr, _stream
    edges = np.linspace(20, 3500, 20)
    taper = np.asarray(maps.get_taper(shape, q64.geom, 12.0, 3.0)[0], dtype=np.float64)
    it, reps = args.iters, args.reps
    for prec in args.precs.split(","):
        q = q64 if prec == "f64" else q64.astype("f32")
        e = q.eng
        mk = lambda one_call, win: mc.RDN0MonteCarloPol(q, [e.hc(), e.hc(), e.hc()], tot, edges, estimators=ESTS, base_seed=5, one_call=one_call)
        one, host, plain = mk(True, True).set_window(taper), mk(False, True).set_window(taper), mk(True, False)
        # the data as analysed: an apodised triple (the windowed draw of stream 10^6)
        draw, real = [e.hc() for _ in range(3)], [e.real() for _ in range(3)]
        data = [k.clone() for k in mc._windowed_teb(e, 17, one.cs, one.rot, one.window, draw, real, 10 ** 6)]
        for drv in (one, host, plain):
            drv.set_data(data)
        paths = [("onecall_draw_fused1", one, 1), ("onecall_draw_fused0", one, 0), ("hostloop", host, -1), ("unwindowed_onecall", plain, -1)]
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
        wl, wk, rl, rk = one._set._bands
        line = dict(tool="rdn0_pol_bench", windowed=True, shape=list(shape), prec=prec, res_arcmin=float(res), estimators=list(ESTS),
                    nspec=one.nspec, bins=int(one.d), iters=it, reps=reps, leg_band=[int(wl), int(rl)], kappa_band=[int(wk), int(rk)])
        for name in t:
            line[name + "_ms"] = round(float(np.median(t[name])), 4)
            line[name + "_p10_p90"] = pct(t[name])
        best = min(float(np.median(t[name])) for name in ("onecall_draw_fused1", "onecall_draw_fused0"))
        line["speedup"] = round(float(np.median(t["hostloop"])) / best, 2)
        line["source_stage_ms"] = {name: round(float(np.median(t[name]) - np.median(t["unwindowed_onecall"])), 4)
                                   for name in ("onecall_draw_fused1", "onecall_draw_fused0")}
        line["max_diff_mean_over_max_mean"] = float(np.max(np.abs(m1 - m0)) / np.max(np.abs(m0)))
        # the draw kernels alone, microseconds per triple
        w = e.nx // 2 + 1
        rot = (one.rot[0], one.rot[2])
        buf = torch.empty((6, e.ny, e.kp), dtype=e.cdt, device=e.device)
        dr = torch.empty((3, e.ny, e.kp), dtype=e.cdt, device=e.device)
        co = torch.empty((3, e.ny, e.kp), dtype=e.cdt, device=e.device)
        drl = [dr[j] for j in range(3)]
        fused = lambda: e.grf_mix_icols(5, one.cs, one.rot[:2], stream_id0=0, ntriples=2, out=buf)
        def unfused():
            for z in range(2):
                e.grf_mix(5, one.cs, rot=rot, out=drl, stream_id0=3 * z)
                for j in range(3):
                    e.fft_cols(dr[j], inverse=True, out=co[j], width=w)
        draw_only = lambda: (e.grf_mix(5, one.cs, rot=rot, out=drl, stream_id0=0), e.grf_mix(5, one.cs, rot=rot, out=drl, stream_id0=3))
        k = {"mix_icols_us": [], "mix_then_cols_us": [], "mix_only_us": []}
        for f in (fused, unfused, draw_only):
            events_us(f, 5)
        for r in range(reps):
            k["mix_icols_us"].append(events_us(fused, 20) / 2)
            k["mix_then_cols_us"].append(events_us(unfused, 20) / 2)
            k["mix_only_us"].append(events_us(draw_only, 20) / 2)
        for name in k:
            line[name] = round(float(np.median(k[name])), 2)
            line[name + "_p10_p90"] = pct(k[name], 2)
        line["cols_launches_note"] = "mix_then_cols: one oa_fft_cols call per plane (the entry batches the three planes in one launch pair)"
        del buf, dr, co, drl
        txt = json.dumps(line)
        print(txt, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(txt + "\n")
        del one, host, plain
        e.release_pools()
        torch.cuda.empty_cache()


def band(args, shape, res, q64, tot):
    """one JSON line per precision: one_call="band" against the host loop on the same plan; the two draw variants alone"""
    import torch
    from orphics_amd import mc
    edges = np.linspace(20, 3500, 20)
    it, reps = args.iters, args.reps
    for prec in args.precs.split(","):
        q = q64 if prec == "f64" else q64.astype("f32")
        e = q.eng
        one = mc.RDN0MonteCarloPol(q, [e.hc(), e.hc(), e.hc()], tot, edges, estimators=ESTS, base_seed=5, one_call="band")
        data = e.grf_mix(17, one.cs, stream_id0=10 ** 6)
        one.set_data(data)
        host = mc.RDN0MonteCarloPol(q, data, tot, edges, estimators=ESTS, base_seed=5, one_call=False)
        for drv in (one, host):                       # warm-up of each path: allocations, first-use tables, clocks
            drv.run_local(range(0, it))
        torch.cuda.synchronize()
        t1, t0, ts = [], [], []
        for r in range(reps):                         # alternated block by block, the same realisations for both
            lo = (r + 1) * it
            t1.append(block_ms(one, lo, it))          # (its first realisation re-binds the plan and sets the data again: the host loop
            t0.append(block_ms(host, lo, it))         #  bound the plan per estimator in between)
        # ... and the one call in blocks of its own, nothing in between: the steady state of a production shard
        one.run_local(range((reps + 1) * it, (reps + 2) * it))
        for r in range(reps):
            ts.append(block_ms(one, (reps + 2 + r) * it, it))
        one.acc.allreduce(); host.acc.allreduce()
        wl, wk, rl, rk = one._bands
        my, mx = q.pol_bound_grid
        line = dict(tool="rdn0_pol_bench", band=True, shape=list(shape), prec=prec, res_arcmin=float(res), estimators=list(ESTS), nspec=one.nspec,
                    bins=int(one.d), iters=it, reps=reps, band_grid=[int(my), int(mx)], leg_band=[int(wl), int(rl)], kappa_band=[int(wk), int(rk)],
                    onecall_ms=round(float(np.median(t1)), 4), onecall_p10_p90=pct(t1),
                    onecall_steady_ms=round(float(np.median(ts)), 4), onecall_steady_p10_p90=pct(ts),
                    hostloop_ms=round(float(np.median(t0)), 4), hostloop_p10_p90=pct(t0),
                    speedup=round(float(np.median(t0) / np.median(t1)), 2), speedup_steady=round(float(np.median(t0) / np.median(ts)), 2))
        # same realisations in both paths up to (reps + 1) * it; the one call ran more after that, so compare the sample means loosely:
        # the tests pin the equality, this is a sanity figure
        m1, m0 = one.acc.mean("rdn0"), host.acc.mean("rdn0")
        line["max_diff_mean_over_max_mean"] = float(np.max(np.abs(m1 - m0)) / np.max(np.abs(m0)))
        line["mean_diff_note"] = "the one call accumulated %d more realisations than the host loop: a sanity figure, not an equality" % ((reps + 1) * it)
        # the two draw variants alone, on the inner grid's planes
        pitch = mx // 2 + 16
        planes = torch.zeros((6, my, pitch), dtype=e.cdt, device=e.device)
        pl = [planes[j] for j in range(6)]
        both = lambda: e.grf_mix_band_inner_triples(5, one.cs, pl, my, pitch, wl, rl, stream_id0=0)
        def twice():
            e.grf_mix_band_inner(5, one.cs, pl[:3], my, pitch, wl, rl, stream_id0=0)
            e.grf_mix_band_inner(5, one.cs, pl[3:], my, pitch, wl, rl, stream_id0=3)
        k = {"draw_triples_us": [], "draw_two_singles_us": []}
        for f in (both, twice):
            events_us(f, 20)
        for r in range(reps):
            k["draw_triples_us"].append(events_us(both, 200))
            k["draw_two_singles_us"].append(events_us(twice, 200))
        for name in k:
            line[name] = round(float(np.median(k[name])), 2)
            line[name + "_p10_p90"] = pct(k[name], 2)
        extra = (np.median(k["draw_two_singles_us"]) - np.median(k["draw_triples_us"])) / 1e3
        line["onecall_two_draws_ms"] = round(float(np.median(ts) + extra), 4)
        line["two_draws_note"] = ("derived: onecall_steady_ms + (draw_two_singles_us - draw_triples_us); the draws are timed through the Python "
                                  "wrappers, back to back on one stream")
        del planes, pl
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
    ap.add_argument("--geoms", default=None, help="default: 2048x2048@1,4096x4096@0.5; with --band 1200x1200@1,2400x2400@0.5")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--iters", type=int, default=6, help="realisations per timed block")
    ap.add_argument("--reps", type=int, default=7, help="timed blocks per path (>= 7)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--windowed", action="store_true", help="the windowed driver (see above)")
    ap.add_argument("--band", action="store_true", help="one_call=\"band\" on sides 2^a 3^b 5^c (see above)")
    args = ap.parse_args()
    if args.geoms is None:
        args.geoms = "1200x1200@1,2400x2400@0.5" if args.band else "2048x2048@1,4096x4096@0.5"
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
        if args.windowed:
            windowed(args, shape, res, q64, tot)
            continue
        if args.band:
            band(args, shape, res, q64, tot)
            continue
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
