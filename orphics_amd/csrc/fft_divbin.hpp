// Tail of the single-pass divergence kernel (col_div_body<.., DivBinTail>): radial binning of |kappa|^2 and the moment update,
// GPU only (wave-level reductions).  Replaces bin_kernel<POWER> + bin_final_kernel on the one-call paths: the kappa plane is
// not re-read (14 MB per 8192^2 reconstruction) and two dependent launches (15 us) go away.
//
// Per value the arithmetic is bin_kernel's: v = (double)((re^2 + im^2) * (T)pnorm) * multiplicity, multiplicity 1 on the columns
// 0 and nx/2 of the half plane, 2 between.  Per wave-step the lanes that share an id are summed in a fixed order (DPP inside rows of 16 lanes, then the row totals) and the
// lowest such lane adds the total to the wave's private LDS row (no atomics, fixed order); the rows are summed per workgroup
// in wave order, the workgroups' partials by divbin_fold_kernel, the next launch on the stream, in workgroup order: deterministic.
#pragma once
#include "fft_launch.hpp"

namespace oa {

// Sum of v over the 64 lanes, returned in every lane (wave-uniform): four DPP steps inside each row of 16 lanes (pairs, quads,
// half-row mirror, row mirror: 2 v_mov_dpp + 1 v_add_f64 each -- float64 has no DPP add), then the four row totals in row
// order through v_readlane.  Fixed order: deterministic.  (64-lane butterflies through ds_bpermute were a chain of six LDS
// round trips per step: the tail took longer than the divergence itself.)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | (unsigned long long)lo);
}
__device__ __forceinline__ double wave_total_f64(double v) {
    v += dpp_f64<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);     // row_half_mirror
    v += dpp_f64<0x140>(v);     // row_mirror
    return ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
}

// What every tail ends with: this workgroup's partial of id i is partial(i) (a fixed-order sum in the tail's LDS, complete and
// visible before the call).  The partials go to f.part with plain vector stores and the workgroup ends: no acknowledge wait, no
// barrier, no ticket.  divbin_fold_kernel, launched right behind the divergence kernel on the same stream (HipLauncher::go_fused),
// folds them: the kernel boundary is the only ordering between the workgroups and the fold, on any target.  `part` belongs to the
// plan: the next call's divergence launch on the same stream is ordered behind this call's fold, so back-to-back calls need nothing else.
template <class Partial>
__device__ __forceinline__ void divbin_handover(const DivBinFuse& f, Partial partial) {
    const int nids = f.nids;
    double* mine = f.part + ((long)blockIdx.z * gridDim.x + blockIdx.x) * nids;
    for (int i = threadIdx.x; i < nids; i += blockDim.x) mine[i] = partial(i);
}

// LDS of the fold: [G][NI] group sums (G NI <= nt), then the nids - 2 bandpowers of every map behind them
__host__ __device__ inline int divbin_fold_ni(int nids, int nt) {
    int NI = 1;
    while (NI < nids && 2 * NI <= nt) NI <<= 1;      // (a power of two of at most nt threads: 384- and 768-thread launches too)
    return NI;
}
inline size_t divbin_fold_lds_bytes(int nids, int nt, int gz) { return ((size_t)nt + (size_t)gz * nids) * sizeof(double); }

// The fold: ONE workgroup of as many threads as the divergence launch had (the order of the additions below depends on it), gx
// workgroups' partials per map, gz maps.  Per map: sums[i] = the workgroups' partials in a fixed two-level order -- thread (g, i),
// i = t mod NI, g = t / NI, adds the partials of workgroups b = g, g + G, ... in fours, (p0 + p1) + (p2 + p3), and what is left over
// one by one; then the G group sums are added in group order; b = sums[1 .. nids-2] / mode counts.  Then the moments, every element
// in map order.  It is a chain of memory round trips, so each trip carries all it can: sixteen partials of a thread are requested
// together (133 workgroups at 19 bins: all of a thread's in one trip; the order of the additions is not the order of the loads), the
// mode count of the id with them, and the thread's first elements of S, C and n before anything else; an element of S or C is read
// and written once for all maps.  (One thread per id walking all workgroups was a chain of ~100 dependent L2-miss loads: 30-50 us.)
__global__ __launch_bounds__(1024) void divbin_fold_kernel(DivBinFuse f, int gz) {
    extern __shared__ double oa_fold_red[];
    double* red = oa_fold_red;
    const int t = threadIdx.x, nt = blockDim.x, nids = f.nids, d = nids - 2, gx = f.gx, dd = d * d;
    const int NI = divbin_fold_ni(nids, nt);
    const int G = nt / NI, gi = t / NI, ii = t - gi * NI;      // (threads behind G NI idle in the group sums)
    double* bv = red + G * NI;                                 // [gz][d]
    const bool mom = f.S != nullptr;
    const double S0 = (mom && t < d) ? f.S[t] : 0.0, C0 = (mom && t < dd) ? f.C[t] : 0.0;
    const int64_t n0 = (t == 0 && f.n) ? f.n[0] : 0;
    for (int z = 0; z < gz; ++z) {
        for (int i0 = 0; i0 < nids; i0 += NI) {          // (one round unless nids > NI)
            const int i = i0 + ii;
            const bool isb = gi == 0 && i >= 1 && i <= d;
            const int64_t mc = isb ? f.mcounts[i] : 1;
            __syncthreads();
            if (gi < G) {
                double s = 0.0;
                if (i < nids) {
                    const double* pz = f.part + ((long)z * gx) * nids + i;
                    for (int b = gi; b < gx; b += 16 * G) {
                        double p[16];
#pragma unroll
                        for (int k = 0; k < 16; ++k) p[k] = pz[(long)(b + k * G < gx ? b + k * G : gx - 1) * nids];     // (clamped: branch-free)
#pragma unroll
                        for (int j = 0; j < 16; j += 4) {
                            if (b + (j + 3) * G < gx) s += (p[j] + p[j + 1]) + (p[j + 2] + p[j + 3]);
                            else {
#pragma unroll
                                for (int k = j; k < j + 4; ++k)
                                    if (b + k * G < gx) s += p[k];
                            }
                        }
                    }
                }
                red[gi * NI + ii] = s;
            }
            __syncthreads();
            if (gi == 0 && i < nids) {
                double tot = 0.0;
                for (int k = 0; k < G; ++k) tot += red[k * NI + ii];
                f.sums[(long)z * nids + i] = tot;
                if (isb) bv[z * d + i - 1] = tot / (double)mc;
            }
        }
    }
    __syncthreads();
    if (mom) {
        for (int a = t; a < d; a += nt) {
            double s = a == t ? S0 : f.S[a];
            for (int z = 0; z < gz; ++z) s += bv[z * d + a];
            f.S[a] = s;
        }
        for (int e = t; e < dd; e += nt) {
            const int ra = e / d, cb = e - ra * d;
            double c = e == t ? C0 : f.C[e];
            for (int z = 0; z < gz; ++z) c += bv[z * d + ra] * bv[z * d + cb];
            f.C[e] = c;
        }
    }
    if (t == 0 && f.n) f.n[0] = n0 + (int64_t)gz;
}

template <typename T>
struct DivBinTail {
    static constexpr bool active = true, needs_ids = true;
    DivBinFuse f;
    double* rows = nullptr;     // LDS: [waves][nids]

    __device__ __forceinline__ void begin(GpuCtx&, void* lds, int, int, int) {
        rows = reinterpret_cast<double*>(lds);
        const int nw = blockDim.x >> 6;
        for (int i = threadIdx.x; i < nw * f.nids; i += blockDim.x) rows[i] = 0.0;
    }
    __device__ __forceinline__ int id_at(unsigned yfull, int col) const { return f.ids[(long)yfull * f.ipitch + col]; }
    // tile-major copy of the ids on the coarse grid ([tile][coarse row][C], DivBinFuse::ids_t): contiguous per tile instead of 16- /
    // 32-byte row segments of the full-pitch plane (7.3 / 15.3 MB fetched for 3.5 MB: profiles/r04_overfetch.txt)
    __device__ __forceinline__ bool packed_ids() const { return f.ids_t != nullptr; }
    __device__ __forceinline__ int id_at_t(long i) const { return f.ids_t[i]; }
    // id < 0: this lane has no value in this step; pw = re^2 + im^2 of kappa
    __device__ __forceinline__ void add(GpuCtx&, int id, T pw, int col, int) {
        const int m = (col == 0 || col == f.nxh) ? 1 : (col < f.nxh ? 2 : 0);
        const bool ok = id >= 0 && id < f.nids && m > 0;
        const double v = ok ? (double)(pw * (T)f.pnorm) * (double)m : 0.0;
        const int lane = threadIdx.x & 63;
        double* row = rows + (threadIdx.x >> 6) * f.nids;
        unsigned long long act = __ballot(ok);
        while (act) {
            const int leader = __ffsll((long long)act) - 1;
            const int lid = __shfl(id, leader, 64);
            const bool mine = ok && id == lid;
            const unsigned long long mm = __ballot(mine);
            const double sv = wave_total_f64(mine ? v : 0.0);
            if (lane == leader) row[lid] += sv;
            act &= ~mm;
        }
    }
    __device__ __forceinline__ void finish(GpuCtx&) {
        const int nw = blockDim.x >> 6, nids = f.nids;
        const double* r = rows;
        __syncthreads();
        divbin_handover(f, [=](int i) {
            double s = 0.0;
            for (int k = 0; k < nw; ++k) s += r[k * nids + i];
            return s;
        });
    }
};

// The same tail without an id in sight (the one-call entries' choice whenever the binding has a run table: divbin_runs.hpp).  The bin
// id of a mode is known when the bins are bound and is piecewise constant down a column, so the tile's runs (column, first row,
// length, id), sorted by id, replace the id reads, the ballot / leader loop and the per-wave histogram rows:
//   add:     v (DivBinTail's expression) goes to P[column][row] in the tile's LDS;
//   finish:  thread e adds the values of run e in row order (R[e]); thread i adds R over the entries of id i in table order: the
//            workgroup's partial of id i.  Then the shared hand-over.
// Every sum has a fixed order that no wave timing enters: bit-reproducible; against DivBinTail only the order of the additions inside
// a workgroup differs.
// LDS: row y of a column sits at y + (y >> 6), columns divrun_col_stride() doubles apart.  The lanes of a wave in finish() mostly hold the
// 64-row chunks of one long run, 64 rows apart: the skew puts them on consecutive banks (unskewed, in either layout, all of them hit one
// bank: the float32 tail then took longer than DivBinTail's); the stride keeps the stores of add() -- C columns x 32 / C rows per half
// wave -- apart.  P takes a little over half a float64 tile, R sits behind it; in float32 P is the tile and a few KB behind it
// (divrun_lds_bytes: the launcher asks for them), and R lies over P's first entries, behind one more barrier.  The entries and
// offsets of this thread are requested in begin(), ahead of the kernel's own Fnorm / axis loads: they have long arrived when finish()
// looks at them.
__host__ __device__ inline int divrun_col_stride(int rows, int logc) {
    const int want = (32 >> logc) > 0 ? (32 >> logc) : 1;
    const int s = rows + (rows >> 6) + 1;
    return s + (((want - s) % 32) + 32) % 32;
}
// dynamic LDS the tail needs from the start of the tile: P, and in float64 R (two entries per thread) behind it
inline size_t divrun_lds_bytes(int rows, int logc, int nt, bool f64) {
    return ((size_t)divrun_col_stride(rows, logc) << logc) * sizeof(double) + (f64 ? (size_t)2 * nt * sizeof(double) : 0);
}
template <typename T>
struct DivRunTail {
    static constexpr bool active = true, needs_ids = false;
    static constexpr bool r_behind = sizeof(T) == 8;
    DivBinFuse f;
    double* P = nullptr;
    double* R = nullptr;
    const int32_t* offp = nullptr;
    int base = 0, cnt = 0, logc = 0, cs = 0, o0 = 0, o1 = 0;
    unsigned e0 = 0, e1 = 0;      // this thread's entries (t, t + nt): their low words -- the id word is the builder's and the offsets' business

    __device__ __forceinline__ void begin(GpuCtx&, void* lds, int tile, int logc_, int rows) {
        P = reinterpret_cast<double*>(lds);
        logc = logc_;
        cs = divrun_col_stride(rows, logc);
        R = r_behind ? P + ((long)cs << logc) : P;
        const int t = threadIdx.x, nt = blockDim.x;
        const int32_t* off = offp = f.run_off + (long)tile * (f.nids + 1);
        base = off[0];
        cnt = off[f.nids] - base;
        if (cnt > 2 * nt) cnt = 2 * nt;                          // (the builder's cap; R holds no more)
        const unsigned* ew = reinterpret_cast<const unsigned*>(f.run_ent + base);
        e0 = t < cnt ? ew[2 * t] : 0u;
        e1 = t + nt < cnt ? ew[2 * (t + nt)] : 0u;
        if (t < f.nids) { o0 = off[t] - base; o1 = off[t + 1] - base; }
    }
    __device__ __forceinline__ int id_at(unsigned, int) const { return -1; }
    __device__ __forceinline__ bool packed_ids() const { return false; }
    __device__ __forceinline__ int id_at_t(long) const { return -1; }
    // slot = coarse row * C + column in tile
    __device__ __forceinline__ void add(GpuCtx&, int, T pw, int col, int slot) {
        const int m = (col == 0 || col == f.nxh) ? 1 : (col < f.nxh ? 2 : 0);
        const int y = slot >> logc, c = slot & ((1 << logc) - 1);
        P[c * cs + y + (y >> 6)] = (double)(pw * (T)f.pnorm) * (double)m;
    }
    __device__ __forceinline__ double run_sum(unsigned w) const {
        const int first = (int)(w & 0xffffu), len = (int)((w >> 16) & 0xffu), col = (int)(w >> 24);
        const double* p = P + col * cs;
        double s = 0.0;
#pragma unroll 4
        for (int y = first; y < first + len; ++y) s += p[y + (y >> 6)];
        return s;
    }
    __device__ __forceinline__ void finish(GpuCtx&) {
        const int t = threadIdx.x, nt = blockDim.x;
        __syncthreads();
        const double s0 = run_sum(e0), s1 = run_sum(e1);          // (no entry: length 0)
        if (!r_behind) __syncthreads();                           // R lies over P: every run has been read
        if (t < cnt) R[t] = s0;
        if (t + nt < cnt) R[t + nt] = s1;
        __syncthreads();
        const double* r = R;
        const int32_t* off = offp;
        const int a0 = o0, a1 = o1, b0 = base, n = cnt;
        divbin_handover(f, [=](int i) {
            int k = a0, k1 = a1;
            if (i != t) { k = off[i] - b0; k1 = off[i + 1] - b0; }     // (more ids than threads)
            if (k1 > n) k1 = n;
            double s = 0.0;
            for (; k < k1; ++k) s += r[k];
            return s;
        });
    }
};

}  // namespace oa
