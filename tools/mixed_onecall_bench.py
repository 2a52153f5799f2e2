"""Timing of the one-call TT path on map sides 2^a 3^b 5^c (BAND GRID, include/orphics_amd.h oa_plan_band_grid) against the
modular chain on the same plan, on the reference notebooks' patches (tutorials/tt_verification.ipynb: 1200^2 at 0.5'; mapwork.ipynb:
2400^2), both precisions.  One JSON line per (side, precision):
    onecall_ms / modular_ms : qe_TT per map (kappa_from_map("TT") from a real device map), median of --reps timed blocks of --iters
    mc_sims_per_s           : GaussianN0MonteCarlo.run_local (oa_mc_run, bandpower moments, no mean field)
    map_bytes               : bytes of the real map the band input transform reads
--only-onecall N: run N one-call reconstructions per geometry and nothing else (the workload for
    rocprofv3 --kernel-trace --stats -- python tools/mixed_onecall_bench.py --only-onecall 200).
--pol: the polarisation half instead (oa_qe_pol / oa_qe_mv behind oa_qe_band_bind): qe_EB (reconstruct_hc) and the MV of TT, TE, EE,
    EB, TB (reconstruct_mv_hc) from Fourier-space legs into an estimator-owned plane, one call on the band grid against the modular
    chain (fused=False) of the same object on the same inputs, in one process.  Per cell the median of --reps timed blocks of --iters
    calls (HIP events) and the spread of the blocks (10th .. 90th percentile).
--splits: the split-based 4-point estimator (SplitLensing.cross_estimator, TT) on n = 4 and 8 splits held as one HalfPlane: the device
    path (one oa_qe_tt_split_power call on the band grid) against the generic pairwise loop on the same plan (n^2 kappa_from_map calls +
    host-side power evaluations: what a duck-typed qest gets, and what every qest got on these sides before), in one process on the
    same inputs.  Per cell the median of --reps timed blocks (HIP events) of --iters device-path / --loop-iters generic-loop estimates and
    the spread of the blocks.
--from-maps: the polarisation entries from REAL T, Q, U maps resident on the device (oa_qe_mv_maps): (a) ONE reconstruct_mv_from_maps(T, Q, U,
    qu=True) call for the MV of five / ONE reconstruct_from_maps("EB", (T, Q, U), qu=True) call, against (b) what the same inputs cost
    without the entry: Engine.rfft of T, Q, U (EB: of Q, U only) into resident planes, rot2, reconstruct_mv_hc / reconstruct_hc -- in one
    process on the same plan and maps, the two paths ALTERNATED block by block after a warm-up of every shape.  Per cell the median and
    the 10th .. 90th percentile of --reps blocks of --iters calls (HIP events; the issue's setting: --reps 50 --iters 10) and the maximum
    relative difference of the two outputs.  --precs picks the precisions; with --only-onecall N: N calls of path (a) and nothing else.
--windowed: the windowed N0 / mean-field Monte Carlo, GaussianN0MonteCarlo(window=taper, mean_field=True): one_call=True (oa_mc_run_windowed
    on the band grid) with the fused row pass (win_fused = 1) and with the unfused flow (win_fused = 0), against the one_call=False host loop
    of existing entries on the same plan -- the three paths ALTERNATED block by block in one process after a warm-up of each.  A block is
    --sims realisations (host loop: --loop-sims); per path the median and the 10th .. 90th percentile of --reps blocks, in sims/s.
    --out appends the raw lines to a file.  With --only-onecall N: N realisations of the fused one call per cell and nothing else.
--pol --windowed: the same for the polarisation set, GaussianN0MonteCarloPol(TT, TE, EE, EB, TB + MV, window=taper, mean_field=True: all
    six stacks): one_call="band" (oa_mc_run_mv_windowed on the band grid) with win_fused = 1 and 0 against the one_call=False host loop on
    the same library and plan, alternated block by block with HIP events.  speedup_vs_host_loop takes the flow the entry picks by itself
    (auto_flow).  With --only-onecall N: per cell N realisations of the one call with win_fused = 1 (one batched inverse column launch
    over three planes per realisation), then N with win_fused = 0 (three single-plane launches per realisation), and nothing else."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(n, res, prec):
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (n, n)
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    noise = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    cl = th.lCl("TT", ml)
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=tmask, kmask_K=kmask, unlensed_equals_lensed=True, dtype=prec)
    rng = np.random.default_rng(1)
    tmap = np.fft.ifft2(np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((cl * beam ** 2 + noise) / g.pixarea)).real
    return q, tmap, (cl * beam ** 2 + noise)[:, :n // 2 + 1]


def setup_pol(n, res):
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    shape = (n, n)
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    beam = maps.gauss_beam(ml, 1.5)
    nT = np.full(shape, cosmology.white_noise_power(1.0))
    tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
    kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
    q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=2 * nT, kmask_P=tmask, kmask_K=kmask, pol=True,
                     unlensed_equals_lensed=True, dtype="f64")
    rng = np.random.default_rng(1)
    k = {X: np.fft.fft2(rng.standard_normal(shape)) * np.sqrt((th.lCl(X + X, ml) * beam ** 2 + nT) / g.pixarea) for X in "TEB"}
    return q, k


def timed_spread(fn, iters, reps):
    """median and (p10, p90) over `reps` blocks of `iters` calls, ms per call"""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), float(np.percentile(out, 10)), float(np.percentile(out, 90))


def main_pol(args):
    import torch
    ests = ("TT", "TE", "EE", "EB", "TB")
    for n in [int(s) for s in args.sides.split(",")]:
        q64, k = setup_pol(n, 0.5)
        q64.mv_weights(ests)
        for prec in ("f32", "f64"):
            q = q64 if prec == "f64" else q64.astype("f32")
            e = q.eng
            hk = {X: e.full_to_hc(e.to_complex(k[X])) for X in "TEB"}
            out, mod_out = q.new_output(), e.hc()
            cells = {
                "EB": (lambda: q.reconstruct_hc("EB", hk["E"], hk["B"], out=out),
                       lambda: q._reconstruct_hc_modular("EB", hk["E"], hk["B"], out=mod_out)),
                "MV": (lambda: q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"], out=out),
                       lambda: q.reconstruct_mv_hc(hk["T"], hk["E"], hk["B"], out=mod_out, fused=False)),
            }
            for name, (one, mod) in cells.items():
                grid = q.pol_band_grid("EB" if name == "EB" else ests)
                if args.only_onecall:
                    for _ in range(args.only_onecall):
                        one()
                    torch.cuda.synchronize()
                    continue
                t1 = timed_spread(one, args.iters, args.reps)
                t0 = timed_spread(mod, args.iters, args.reps)
                diff = float((out - mod_out)[:, :e.nxh + 1].abs().max() / mod_out.abs().max())
                print(json.dumps(dict(side=n, prec=prec, call=name, band_grid=list(grid) if grid else None, onecall_ms=round(t1[0], 4),
                                      onecall_p10_p90=[round(t1[1], 4), round(t1[2], 4)], modular_ms=round(t0[0], 4),
                                      modular_p10_p90=[round(t0[1], 4), round(t0[2], 4)], speedup=round(t0[0] / t1[0], 2),
                                      max_rel_diff=diff)), flush=True)


def timed_alternating(fa, fb, iters, reps, *more):
    """blocks of `iters` calls of fa, of fb (and of every further function) in turn: (median, p10, p90) ms per call of each"""
    import torch
    fns = (fa, fb) + tuple(more)
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = tuple([] for _ in fns)
    for _ in range(reps):
        for fn, acc in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b) / iters)
    return tuple((float(np.median(o)), float(np.percentile(o, 10)), float(np.percentile(o, 90))) for o in out)


def main_frommaps(args):
    import torch
    from orphics_amd import maps
    ests = ("TT", "TE", "EE", "EB", "TB")
    sides = [int(s) for s in args.sides.split(",")]
    precs = args.precs.split(",")
    cells = []
    for n in sides:
        q64, k = setup_pol(n, 0.5)
        q64.mv_weights(ests)
        rot = maps.queb_rotmat(q64.geom.lmap())
        c, s = rot[0, 0], rot[1, 0]
        real = [np.fft.ifft2(a).real for a in (k["T"], c * k["E"] + s * k["B"], -s * k["E"] + c * k["B"])]        # T, Q, U
        for prec in precs:
            q = q64 if prec == "f64" else q64.astype("f32")
            e = q.eng
            T, Q, U = (e.to_real(a) for a in real)
            kb = [e.hc(), e.hc(), e.hc()]
            out, ref_out = q.new_output(), e.hc()
            rc, rs = q._qu_rot(False)

            def mv_ref(q=q, e=e, T=T, Q=Q, U=U, kb=kb, ref_out=ref_out, rc=rc, rs=rs):
                e.rfft(T, out=kb[0]); e.rfft(Q, out=kb[1]); e.rfft(U, out=kb[2])
                kE, kB = e.rot2(rc, rs, kb[1], kb[2])
                return q.reconstruct_mv_hc(kb[0], kE, kB, out=ref_out)

            def eb_ref(q=q, e=e, Q=Q, U=U, kb=kb, ref_out=ref_out, rc=rc, rs=rs):
                e.rfft(Q, out=kb[1]); e.rfft(U, out=kb[2])
                kE, kB = e.rot2(rc, rs, kb[1], kb[2])
                return q.reconstruct_hc("EB", kE, kB, out=ref_out)
            cells.append((n, prec, "MV", q, e, out, ref_out, lambda q=q, T=T, Q=Q, U=U, out=out: q.reconstruct_mv_from_maps(T, Q, U, qu=True, out=out), mv_ref))
            cells.append((n, prec, "EB", q, e, out, ref_out, lambda q=q, T=T, Q=Q, U=U, out=out: q.reconstruct_from_maps("EB", (T, Q, U), qu=True, out=out), eb_ref))
    for cell in cells:                                 # warm-up of every shape before anything is timed
        cell[7](); cell[8]()
    torch.cuda.synchronize()
    for n, prec, name, q, e, out, ref_out, one, ref in cells:
        if args.only_onecall:
            for _ in range(args.only_onecall):
                one()
            torch.cuda.synchronize()
            continue
        ta, tb = timed_alternating(one, ref, args.iters, args.reps)
        one(); ref()
        diff = float((out - ref_out)[:, :e.nxh + 1].abs().max() / ref_out.abs().max())
        grid = q.pol_band_grid("EB" if name == "EB" else ests)
        print(json.dumps(dict(side=n, prec=prec, call=name, band_grid=list(grid) if grid else None, frommaps_ms=round(ta[0], 4),
                              frommaps_p10_p90=[round(ta[1], 4), round(ta[2], 4)], transforms_ms=round(tb[0], 4),
                              transforms_p10_p90=[round(tb[1], 4), round(tb[2], 4)], speedup=round(tb[0] / ta[0], 2), max_rel_diff=diff)),
              flush=True)


def main_windowed(args):
    import torch
    from orphics_amd import maps, mc
    edges = np.linspace(100, 3000, 12)
    lines = []
    for n in [int(s) for s in args.sides.split(",")]:
        for prec in args.precs.split(","):
            q, _, tot_h = setup(n, 0.5, prec)
            e = q.eng
            taper, _ = maps.get_taper((n, n), q.geom, taper_percent=12.0, pad_percent=3.0)
            kw = dict(base_seed=3, mean_field=True, window=taper)
            one = mc.GaussianN0MonteCarlo(q, tot_h, edges, one_call=True, **kw)
            host = mc.GaussianN0MonteCarlo(q, tot_h, edges, one_call=False, **kw)
            state = {"lo": 1000}

            def block(drv, fused, count):
                e.set_option("win_fused", fused)
                drv.run_local(range(state["lo"], state["lo"] + count))
                state["lo"] += count
            if args.only_onecall:
                block(one, 1, args.only_onecall)
                torch.cuda.synchronize()
                continue
            # one "call" of timed_alternating is a block of realisations (the drivers bind their own bin ids when they take turns: a
            # set-up launch per block, inside the timed window of each path alike)
            names = ("onecall_fused", "onecall_unfused", "host_loop")
            counts = (args.sims, args.sims, args.loop_sims)
            ms = timed_alternating(lambda: block(one, 1, args.sims), lambda: block(one, 0, args.sims), 1, args.reps,
                                   lambda: block(host, 1, args.loop_sims))
            rates = {name: [c / (t / 1e3) for t in (m[0], m[2], m[1])] for name, c, m in zip(names, counts, ms)}      # median, p10, p90 of the rate
            e.set_option("win_fused", -1)
            rec = dict(side=n, prec=prec, call="windowed_n0_mean_field", band_grid=list(q.band_grid), reps=args.reps, sims_per_block=args.sims,
                       loop_sims_per_block=args.loop_sims)
            for name, r in rates.items():
                rec[name + "_sims_per_s"] = round(r[0], 1)
                rec[name + "_p10_p90"] = [round(r[1], 1), round(r[2], 1)]
            rec["speedup_vs_host_loop"] = round(rec["onecall_fused_sims_per_s"] / rec["host_loop_sims_per_s"], 2)
            rec["fused_vs_unfused"] = round(rec["onecall_fused_sims_per_s"] / rec["onecall_unfused_sims_per_s"], 3)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            e.release_pools()
    if args.out and lines:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main_pol_windowed(args):
    import torch
    from orphics_amd import cosmology, lensing, maps, mc
    from orphics_amd.geometry import FlatGeometry
    ests = ("TT", "TE", "EE", "EB", "TB")
    edges = np.linspace(100, 3000, 12)
    lines = []
    for n in [int(s) for s in args.sides.split(",")]:
        shape = (n, n)
        g = FlatGeometry.from_res(shape, 0.5)
        th = cosmology.default_theory()
        ml = g.modlmap()
        beam = maps.gauss_beam(ml, 1.5)
        nT = np.full(shape, cosmology.white_noise_power(1.0))
        tmask = maps.mask_kspace(shape, g, lmin=300, lmax=2000)
        kmask = maps.mask_kspace(shape, g, lmin=20, lmax=3500)
        cl = {k: th.lCl(k, ml) for k in ("TT", "EE", "BB", "TE")}
        tot = dict(TT=cl["TT"] * beam ** 2 + nT, EE=cl["EE"] * beam ** 2 + 2 * nT, BB=cl["BB"] * beam ** 2 + 2 * nT, TE=cl["TE"] * beam ** 2)
        tot_h = {k: np.ascontiguousarray(v[:, :n // 2 + 1]) for k, v in tot.items()}
        taper, _ = maps.get_taper(shape, g, taper_percent=12.0, pad_percent=3.0)
        for prec in args.precs.split(","):
            q = lensing.qest(shape, g, th, noise2d=nT, beam2d=beam, kmask=tmask, noise2d_P=2 * nT, kmask_P=tmask, kmask_K=kmask, pol=True,
                             unlensed_equals_lensed=True, dtype=prec)
            e = q.eng
            kw = dict(estimators=ests, base_seed=3, mean_field=True, window=taper)
            one = mc.GaussianN0MonteCarloPol(q, tot_h, edges, one_call="band", **kw)
            host = mc.GaussianN0MonteCarloPol(q, tot_h, edges, one_call=False, **kw)
            state = {"lo": 1000}

            def block(drv, fused, count):
                e.set_option("win_fused", fused)
                drv.run_local(range(state["lo"], state["lo"] + count))
                state["lo"] += count
            if args.only_onecall:
                for fused in (1, 0):
                    block(one, fused, args.only_onecall)
                torch.cuda.synchronize()
                e.set_option("win_fused", -1)
                continue
            # a block of the one call binds the plan again after the host loop's per-estimator bindings: two set-up calls per block,
            # inside its timed window
            names = ("onecall_fused", "onecall_unfused", "host_loop")
            counts = (args.sims, args.sims, args.loop_sims)
            ms = timed_alternating(lambda: block(one, 1, args.sims), lambda: block(one, 0, args.sims), 1, args.reps,
                                   lambda: block(host, 1, args.loop_sims))
            rates = {name: [c / (t / 1e3) for t in (m[0], m[2], m[1])] for name, c, m in zip(names, counts, ms)}      # median, p10, p90 of the rate
            e.set_option("win_fused", -1)
            rec = dict(side=n, prec=prec, call="pol_windowed_n0_mean_field", estimators=list(ests), nstacks=len(one.mf_labels),
                       band_grid=list(q.pol_band_grid(ests, ext_norm=True)), reps=args.reps, sims_per_block=args.sims, loop_sims_per_block=args.loop_sims)
            for name, r in rates.items():
                rec[name + "_sims_per_s"] = round(r[0], 2)
                rec[name + "_p10_p90"] = [round(r[1], 2), round(r[2], 2)]
            auto = "onecall_fused" if n > 1200 else "onecall_unfused"                  # what the entry runs until win_fused is set
            rec["auto_flow"] = auto
            rec["speedup_vs_host_loop"] = round(rec[auto + "_sims_per_s"] / rec["host_loop_sims_per_s"], 2)
            rec["fused_vs_unfused"] = round(rec["onecall_fused_sims_per_s"] / rec["onecall_unfused_sims_per_s"], 3)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            e.release_pools()
    if args.out and lines:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


class _Duck(object):
    """a qest that is not this package's Estimator: SplitLensing takes the generic pairwise loop"""

    def __init__(self, q):
        self.q = q

    def kappa_from_map(self, XY, T2DData=None, T2DDataY=None, alreadyFTed=False, returnFt=False, **unused):
        return self.q.kappa_from_map(XY, T2DData=T2DData, T2DDataY=T2DDataY, alreadyFTed=alreadyFTed, returnFt=returnFt)


def main_splits(args):
    import torch
    from orphics_amd import lensing
    from orphics_amd.stats import HalfPlane
    for n in [int(s) for s in args.sides.split(",")]:
        q64, tmap, _ = setup(n, 0.5, "f64")
        rng = np.random.default_rng(2)
        smaps = [tmap + 0.3 * rng.standard_normal(tmap.shape) for _ in range(8)]
        for prec in ("f32", "f64"):
            q = q64 if prec == "f64" else q64.astype("f32")
            e = q.eng
            hcs = torch.stack([e.rfft(e.to_real(m)) for m in smaps])
            dev_sl = lensing.SplitLensing(tmap.shape, q.geom, q, "TT")
            gen_sl = lensing.SplitLensing(tmap.shape, q.geom, _Duck(q), "TT")
            for ns in (4, 8):
                half = HalfPlane(hcs[:ns], e)
                res = {}
                t1 = timed_spread(lambda: res.__setitem__("dev", dev_sl.cross_estimator(half)), args.iters, args.reps)
                t0 = timed_spread(lambda: res.__setitem__("gen", gen_sl.cross_estimator(half)), args.loop_iters, args.reps)
                a, b = res["dev"].t.double()[:, :e.nxh + 1], res["gen"].t.double()[:, :e.nxh + 1]
                diff = float((a - b).abs().max() / b.abs().max())
                print(json.dumps(dict(side=n, prec=prec, call="splits", nsplits=ns, band_grid=list(q.band_grid), device_ms=round(t1[0], 4),
                                      device_p10_p90=[round(t1[1], 4), round(t1[2], 4)], loop_ms=round(t0[0], 4),
                                      loop_p10_p90=[round(t0[1], 4), round(t0[2], 4)], speedup=round(t0[0] / t1[0], 2),
                                      max_rel_diff=diff)), flush=True)
            e.release_pools()


def timed(fn, iters, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="1200,2400")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sims", type=int, default=600)
    ap.add_argument("--only-onecall", type=int, default=0)
    ap.add_argument("--pol", action="store_true")
    ap.add_argument("--splits", action="store_true")
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--from-maps", action="store_true")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--windowed", action="store_true")
    ap.add_argument("--loop-sims", type=int, default=60)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orphics_amd import mc
    torch.cuda.set_device(0)
    if args.pol and args.windowed:
        return main_pol_windowed(args)
    if args.pol:
        return main_pol(args)
    if args.splits:
        return main_splits(args)
    if args.from_maps:
        return main_frommaps(args)
    if args.windowed:
        return main_windowed(args)
    for n in [int(s) for s in args.sides.split(",")]:
        for prec in ("f32", "f64"):
            q, tmap, tot_h = setup(n, 0.5, prec)
            e = q.eng
            tm = e.to_real(tmap)
            out = q.new_output()
            if args.only_onecall:
                for _ in range(args.only_onecall):
                    q.reconstruct_tt_from_map(tm, out=out)
                torch.cuda.synchronize()
                continue
            one = timed(lambda: q.reconstruct_tt_from_map(tm, out=out), args.iters, args.reps)
            kbuf = e.hc()
            mod = timed(lambda: q.reconstruct_tt_hc(e.rfft(tm, out=kbuf), out=out, fused=False), args.iters, args.reps)
            drv = mc.GaussianN0MonteCarlo(q, tot_h, np.linspace(100, 3000, 12), base_seed=3)
            drv.run_local(range(12))
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            drv.run_local(range(100, 100 + args.sims))
            b.record()
            b.synchronize()
            sims = args.sims / (a.elapsed_time(b) / 1e3)
            print(json.dumps(dict(side=n, prec=prec, band_grid=list(q.band_grid), onecall_ms=round(one, 4), modular_ms=round(mod, 4),
                                  speedup=round(mod / one, 2), mc_sims_per_s=round(sims, 1), map_bytes=n * n * e.rdt.itemsize)), flush=True)


if __name__ == "__main__":
    main()
