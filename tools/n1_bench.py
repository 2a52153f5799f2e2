"""Timing of the analytic N1 pair sums of the TT estimator (oa_n1_tt, csrc/n1.hpp) with the notebook filters (l_T in (300, 2000), 1.5'
beam, 1 uK-arcmin noise).

Per geometry (--geoms, default 1024x1024@2, 4096x4096@0.5, 8192x8192@0.5) a few modes L are timed one oa_n1_tt call each with HIP
events: a warm-up call, then --reps calls per L; median and 10th .. 90th percentile in seconds per L.  Pair counts per L:
  pairs_box  : (modes of the box of L)^2 -- every (l1, q) the definition sums over on the kernel's box;
  pairs_exec : what the kernel evaluates: (l1 with G != 0) x (q in chunks of <= 128 box modes that hold some H != 0).
Rates are pairs_exec / s; the kernel spends 17 float64 instructions (23 floating-point operations: 6 of them are fused multiply-adds)
per evaluated pair.  In the same run oa_probe_fma64 gives the attainable float64 vector rate (fused multiply-adds / s), and the kernel
is expressed as a fraction of it by instruction count (17 instructions per pair against one per fused multiply-add).
The vectorised NumPy statement of one L is timed on the host at the first geometry over a slice of --numpy-l1 l1 modes against the
whole box and scaled to the box (the full statement at 1024^2 is 2e10 pair terms).
One JSON line per geometry, one for the probe, one for NumPy; appended to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OPS_PER_PAIR = 17


def setup(shape, res):
    from orphics_amd import cosmology, lensing, maps
    from orphics_amd.geometry import FlatGeometry
    g = FlatGeometry.from_res(shape, res)
    th = cosmology.default_theory()
    ml = g.modlmap()
    return lensing.qest(shape, g, th, noise2d=np.full(shape, cosmology.white_noise_power(1.0)), beam2d=maps.gauss_beam(ml, 1.5),
                        kmask=maps.mask_kspace(shape, g, lmin=300, lmax=2000), kmask_K=maps.mask_kspace(shape, g, lmin=20, lmax=3500),
                        unlensed_equals_lensed=True, dtype="f64")


def box_arrays(q, Lyi, Lxi):
    """(G, H, l vectors, C, indices) on the box of L, NumPy, as csrc/n1.hpp's prologue makes them"""
    Ny, Nx = q.shape[-2:]
    rows, cols = q.n1_band()
    kLy = Lyi - Ny if Lyi > Ny // 2 else Lyi
    kLx = Lxi - Nx if Lxi > Nx // 2 else Lxi
    y = np.arange(max(kLy, 0) - (rows - 1), min(kLy, 0) + rows)
    x = np.arange(max(kLx, 0) - (cols - 1), min(kLx, 0) + cols)
    ky, kx = np.meshgrid(y, x, indexing="ij")
    ly, lx = q.geom.laxes()

    def at(half, yy, xx):
        neg = xx < 0
        return half[np.where(neg, -yy, yy) % Ny, np.abs(xx)]
    k2y, k2x = kLy - ky, kLx - kx
    l1 = (ly[ky % Ny], lx[kx % Nx])
    l2 = (ly[k2y % Ny], lx[k2x % Nx])
    G = (ly[Lyi] * l1[0] + lx[Lxi] * l1[1]) * at(q.wg_tt, ky, kx) * at(q.wh_tt, k2y, k2x)
    G2 = (ly[Lyi] * l2[0] + lx[Lxi] * l2[1]) * at(q.wg_tt, k2y, k2x) * at(q.wh_tt, ky, kx)
    return dict(G=G, H=G + G2, l1=l1, l2=l2, C1=at(q.cl_grad["TT"], ky, kx), C2=at(q.cl_grad["TT"], k2y, k2x), ky=ky, kx=kx)


def pair_counts(b):
    bh, bw = b["G"].shape
    nseg = -(-bw // 128)
    qlen = -(-bw // nseg)
    nq = 0
    for s in range(nseg):
        blk = b["H"][:, s * qlen:min(bw, (s + 1) * qlen)]
        nq += int((np.any(blk != 0, axis=1) * blk.shape[1]).sum())
    return float(bh * bw) ** 2, float(np.count_nonzero(b["G"])) * nq


def numpy_slice_seconds(q, b, n_l1):
    """the statement's fused form, broadcast: n_l1 l1 modes with G != 0 against every q of the box"""
    Ny, Nx = q.shape[-2:]
    cpp = q.n1_clpp()
    idx = np.flatnonzero(b["G"].ravel() != 0)[:n_l1]
    f = lambda a: a.ravel()
    t0 = time.perf_counter()
    ay, ax, a2y, a2x = f(b["l1"][0])[idx, None], f(b["l1"][1])[idx, None], f(b["l2"][0])[idx, None], f(b["l2"][1])[idx, None]
    qy, qx, q2y, q2x = f(b["l1"][0])[None, :], f(b["l1"][1])[None, :], f(b["l2"][0])[None, :], f(b["l2"][1])[None, :]
    my, mx = ay - qy, ax - qx
    f1 = f(b["C1"])[idx, None] * (my * ay + mx * ax) - f(b["C1"])[None, :] * (my * qy + mx * qx)
    f2 = f(b["C2"])[None, :] * (my * q2y + mx * q2x) - f(b["C2"])[idx, None] * (my * a2y + mx * a2x)
    dy = f(b["ky"])[idx, None] - f(b["ky"])[None, :]
    dx = f(b["kx"])[idx, None] - f(b["kx"])[None, :]
    cp = cpp[np.where(dx < 0, -dy, dy) % Ny, np.abs(dx)]
    s = float((f(b["G"])[idx, None] * f(b["H"])[None, :] * cp * f1 * f2).sum())
    return time.perf_counter() - t0, idx.size, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geoms", default="1024x1024@2,4096x4096@0.5,8192x8192@0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-l1", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from orphics_amd import _lib
    lib = _lib.load()
    lines = []

    def ev_seconds(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e-3
    # float64 FMA probe: 8 workgroups per CU of 256, ~0.1 s
    blocks, iters = 2048, 1 << 18
    sink = torch.empty(blocks * 256, dtype=torch.float64, device="cuda")
    probe = lambda: _lib.check(lib.oa_probe_fma64(blocks, iters, 0.999999, 1e-9, ctypes.c_void_p(sink.data_ptr()),
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    probe()
    torch.cuda.synchronize()
    pt = [ev_seconds(probe) for _ in range(7)]
    fma_rate = blocks * 256 * iters * 8 / float(np.median(pt))
    lines.append(dict(what="probe_fma64", fma_per_s=fma_rate, tflops=2 * fma_rate / 1e12, seconds_median=float(np.median(pt)),
                      seconds_p10_p90=[float(np.percentile(pt, 10)), float(np.percentile(pt, 90))]))
    print(json.dumps(lines[-1]), flush=True)
    first = True
    for spec in a.geoms.split(","):
        dims, res = spec.split("@")
        shape = tuple(int(v) for v in dims.split("x"))
        q = setup(shape, float(res))
        ly, lx = q.geom.laxes()
        rows, cols = q.n1_band()
        per_L = []
        for Lmod in (200.0, 1000.0, 2500.0):                     # one mode per |L| on the diagonal
            m = (int(round(Lmod / np.sqrt(2) / abs(ly[1]))), int(round(Lmod / np.sqrt(2) / abs(lx[1]))))
            b = box_arrays(q, *m)
            pbox, pexec = pair_counts(b)
            q.n1_sums([m])                                        # warm-up: pool, planes
            wg, wh, cr, cp = (q._hcreal(q.eng64, p) for p in (q.wg_tt, q.wh_tt, q.cl_grad["TT"], q.n1_clpp()))
            Ly, Lx = [m[0]], [m[1]]
            out = torch.empty(1, dtype=torch.float64, device="cuda")
            t = [ev_seconds(lambda: q.eng64.n1_tt(wg, wh, cr, cp, cols, rows, Ly, Lx, out=out)) for _ in range(a.reps)]
            med = float(np.median(t))
            per_L.append(dict(L=float(np.hypot(ly[m[0]], lx[m[1]])), mode=list(m), S=float(out.cpu()[0]), box=list(b["G"].shape), pairs_box=pbox,
                              pairs_exec=pexec, seconds_median=med, seconds_p10_p90=[float(np.percentile(t, 10)), float(np.percentile(t, 90))],
                              pairs_exec_per_s=pexec / med, frac_of_fma_rate=pexec * OPS_PER_PAIR / med / fma_rate))
            if first and Lmod == 1000.0:
                sec, n, _ = numpy_slice_seconds(q, b, a.numpy_l1)
                lines.append(dict(what="numpy_statement", geom=spec, L=per_L[-1]["L"], l1_modes_timed=n, seconds_slice=sec,
                                  seconds_per_L_scaled=sec * np.count_nonzero(b["G"]) / n, note="one slice timed, scaled to every l1 with G != 0"))
                print(json.dumps(lines[-1]), flush=True)
        lines.append(dict(what="n1_tt", geom=spec, leg_rows=rows, leg_cols=cols, ops_per_pair=OPS_PER_PAIR, reps=a.reps, per_L=per_L))
        print(json.dumps(lines[-1]), flush=True)
        first = False
        del q
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
