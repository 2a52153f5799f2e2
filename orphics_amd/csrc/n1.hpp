// Analytic N1 bias of the TT estimator by direct mode-pair summation (oa_n1_tt, n1.hip).  For ONE reconstructed mode L
//     S(L) = sum_{l1} sum_{l1'} g_L(l1, l2) g_L(l1', l2') [ Cpp(l1 - l1') f(l1, -l1') f(l2, -l2') + Cpp(l1 - l2') f(l1, -l2') f(l2, -l1') ],
//     l2 = L - l1,  l2' = L - l1',  g_L(a, b) = (L.a) wg(a) wh(b),  f(a, b) = C_a (m.a) + C_b (m.b),  m = a + b.
// Renaming l1' <-> l2' in the second term gives both terms the kernel Cpp(l1 - q) f(l1, -q) f(l2, -(L - q)), so
//     S(L) = sum_{l1} G(l1) sum_{q} H(q) Cpp(l1 - q) f(l1, -q) f(l2, -(L - q)),      G(q) = g_L(q, L - q),   H(q) = G(q) + G(L - q):
// one pair term per (l1, q), evaluated in float64 over the BOX of L: the modes q with q and L - q both inside |ky| < leg_rows,
// |kx| < leg_cols (outside it wh(L - q) = 0 and G vanishes), row-major, bh rows of bw modes.
// THREE bodies, shared by the HIP launchers (n1.hip) and the CPU emulator (tests/emul/emul_n1.cpp):
//   n1_prologue_body : the box-ordered mode table N1Q (q, L - q, C(q), C(L - q), H(q)) and G(q) of one L;
//   n1_pair_body     : workgroup (tile, part) owns a TILE of l1 -- a segment of at most N1_SEG modes of one box row, N1_R1 per thread, in
//                      registers -- and walks part `part` of the q CHUNKS (segments of at most N1_TQ modes of one box row), each staged in
//                      LDS with the ONE vector of Cpp values the (tile row, chunk row) pair can meet: Cpp(dy, dx) for the single dy and
//                      the contiguous dx range of the pair (lanes of a wave read consecutive entries, the q entry is a broadcast);
//   n1_fold_body     : ONE workgroup adds the (tile, part) partials.
// Every sum has an order fixed by (box, tile constants) alone, no atomics: S is the same bit for bit on every run and for every nL.
#pragma once
#include <cmath>
#include "cx.hpp"

namespace oa {

constexpr int N1_NT = 256;             // threads of a pair / fold workgroup
constexpr int N1_R1 = 2;               // l1 modes per thread (columns x0 + t and x0 + t + N1_NT of the tile)
constexpr int N1_SEG = N1_NT * N1_R1;  // most l1 modes of a tile
constexpr int N1_TQ = 128;             // most q modes of a chunk
constexpr int N1_PARTS_MAX = 16;       // most parts the chunks of one L are cut into (grid y)
constexpr int N1_WG_TARGET = 2048;     // workgroups per launch the cut aims at (8 per CU of 256)
constexpr double N1_PAIRS_PER_LAUNCH = 6e10;   // most pair terms of one launch

struct alignas(16) N1Q {               // one box mode q for the primed side
    double y, x;                       // l(q)
    double y2, x2;                     // l(L - q)
    double c, c2;                      // C(q), C(L - q)
    double h, pad;                     // H(q)
};

// the box of L (signed mode indices): rows y0 .. y0 + bh - 1, columns x0 .. x0 + bw - 1; bh or bw <= 0: empty
struct N1Box { int y0, x0, bh, bw; };
OA_HD N1Box n1_box(int kLy, int kLx, int leg_rows, int leg_cols) {
    const int r = leg_rows - 1, w = leg_cols - 1;
    N1Box b;
    b.y0 = (kLy > 0 ? kLy : 0) - r;
    b.x0 = (kLx > 0 ? kLx : 0) - w;
    b.bh = (kLy < 0 ? kLy : 0) + r - b.y0 + 1;
    b.bw = (kLx < 0 ? kLx : 0) + w - b.x0 + 1;
    return b;
}
// tiles of l1 and chunks of q per box row: balanced segments
OA_HD int n1_nseg(int bw, int cap) { return (bw + cap - 1) / cap; }
OA_HD int n1_seglen(int bw, int cap) { const int n = n1_nseg(bw, cap); return (bw + n - 1) / n; }
OA_HD long n1_ntiles(N1Box b) { return (long)b.bh * n1_nseg(b.bw, N1_SEG); }
OA_HD long n1_nchunks(N1Box b) { return (long)b.bh * n1_nseg(b.bw, N1_TQ); }
// tiles per pair launch: a launch evaluates at most N1_PAIRS_PER_LAUNCH pair terms (tens of milliseconds at the measured rate),
// whatever the map's size; and the parts the chunks are cut into, so that a LAUNCH brings N1_WG_TARGET workgroups where the box allows
OA_HD long n1_tiles_per_launch(N1Box b) {
    const long per = (long)(N1_PAIRS_PER_LAUNCH / ((double)b.bh * b.bw * n1_seglen(b.bw, N1_SEG)));
    const long nt = n1_ntiles(b);
    return per < 1 ? 1 : (per > nt ? nt : per);
}
OA_HD int n1_parts(N1Box b) {
    const long nt = n1_tiles_per_launch(b), nc = n1_nchunks(b);
    long p = (N1_WG_TARGET + nt - 1) / nt;
    if (p > N1_PARTS_MAX) p = N1_PARTS_MAX;
    if (p > nc) p = nc;
    return p < 1 ? 1 : (int)p;
}
inline size_t n1_pair_lds() { return (size_t)N1_TQ * sizeof(N1Q) + (size_t)(N1_SEG + N1_TQ) * 8 + 64; }

OA_HD double n1_fma(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fma(a, b, c);
#else
    return std::fma(a, b, c);
#endif
}
OA_HD long n1_wrap(long k, long n) { const long m = k % n; return m < 0 ? m + n : m; }
// real hc-layout plane (ny rows of pitch kp) at the signed mode (ky, kx), |kx| <= nx / 2: negative kx through the Hermitian partner
OA_HD double n1_hc_at(const double* pl, int ny, long kp, int ky, int kx) {
    if (kx < 0) { ky = -ky; kx = -kx; }
    return pl[n1_wrap(ky, ny) * kp + kx];
}

/* THE PAIR TERM of the TT estimator without its weights: f(l1, -q) f(l2, -(L - q)) for l1 = (ay, ax), l2 = (a2y, a2x) with their
 * response spectra ca, ca2, and the primed mode q.  With m = l1 - q:
 *     f(l1, -q) = C(l1) (m.l1) - C(q) (m.q),        f(l2, -(L - q)) = -C(l2) (m.l2) + C(L - q) (m.(L - q)).
 * 14 float64 operations (2 sub, 6 mul, 6 fma); the caller spends 3 more on Cpp H and the accumulation: 17 per pair. */
OA_HD void n1_pair_tt(double ay, double ax, double a2y, double a2x, double ca, double ca2, const N1Q& q, double& f1, double& f2) {
    const double my = ay - q.y, mx = ax - q.x;
    const double ma = n1_fma(my, ay, mx * ax);
    const double mq = n1_fma(my, q.y, mx * q.x);
    const double ma2 = n1_fma(my, a2y, mx * a2x);
    const double mq2 = n1_fma(my, q.y2, mx * q.x2);
    f1 = n1_fma(ca, ma, -(q.c * mq));
    f2 = n1_fma(q.c2, mq2, -(ca2 * ma2));
}

/* PROLOGUE.  Any grid of N1_NT-thread workgroups (x), grid-stride over the bh bw box modes. */
struct N1ProArgs {
    const double* wg; const double* wh; const double* cr;   // real hc planes (ny, kp)
    const double* ly; const double* lx;                     // the plan's axes (ny, nx doubles)
    int ny, nx; long kp;
    int kLy, kLx;                                           // L: signed mode indices
    N1Box box;
    N1Q* q; double* g;                                      // [bh bw] each
};
template <class Ctx>
OA_HD void n1_prologue_body(Ctx& ctx, const N1ProArgs& a) {
    const long n = (long)a.box.bh * a.box.bw;
    const double Ly = a.ly[n1_wrap(a.kLy, a.ny)], Lx = a.lx[n1_wrap(a.kLx, a.nx)];
    for (long i = (long)ctx.bid_x() * ctx.nthreads() + ctx.tid(); i < n; i += (long)ctx.grid_x() * ctx.nthreads()) {
        const int ky = a.box.y0 + (int)(i / a.box.bw), kx = a.box.x0 + (int)(i % a.box.bw);
        const int k2y = a.kLy - ky, k2x = a.kLx - kx;
        N1Q e;
        e.y = a.ly[n1_wrap(ky, a.ny)];   e.x = a.lx[n1_wrap(kx, a.nx)];
        e.y2 = a.ly[n1_wrap(k2y, a.ny)]; e.x2 = a.lx[n1_wrap(k2x, a.nx)];
        e.c = n1_hc_at(a.cr, a.ny, a.kp, ky, kx);
        e.c2 = n1_hc_at(a.cr, a.ny, a.kp, k2y, k2x);
        const double g1 = (Ly * e.y + Lx * e.x) * n1_hc_at(a.wg, a.ny, a.kp, ky, kx) * n1_hc_at(a.wh, a.ny, a.kp, k2y, k2x);
        const double g2 = (Ly * e.y2 + Lx * e.x2) * n1_hc_at(a.wg, a.ny, a.kp, k2y, k2x) * n1_hc_at(a.wh, a.ny, a.kp, ky, kx);
        e.h = g1 + g2;
        e.pad = 0.0;
        a.q[i] = e;
        a.g[i] = g1;
    }
}

/* PAIR SUMS.  Grid (tiles of this launch, parts), N1_NT threads, n1_pair_lds() bytes.  part[(tile0 + bid_x) parts + bid_y] is written by
 * every workgroup (0 where the tile carries no weight). */
struct N1PairArgs {
    const N1Q* q; const double* g;     // the prologue's table
    const double* cpp; int ny; long kp;                     // C^phiphi: real hc plane
    N1Box box;
    long tile0; int parts;
    double* part;                      // [ntiles][parts]
};
template <class Ctx>
OA_HD void n1_pair_body(Ctx& ctx, const N1PairArgs& a) {
    const int tid = ctx.tid();
    char* sm = (char*)ctx.smem();
    N1Q* const qs = (N1Q*)sm;                                           // [N1_TQ]
    double* const cp = (double*)(qs + N1_TQ);                           // [N1_SEG + N1_TQ]
    int* const any = (int*)(cp + N1_SEG + N1_TQ);                       // [2] chunk flags, [2] the tile's
    double* const red = (double*)sm;                                    // [N1_NT] (the final reduction, over qs)
    const int bw = a.box.bw;
    const long tile = a.tile0 + ctx.bid_x();
    const int nseg = n1_nseg(bw, N1_SEG), seglen = n1_seglen(bw, N1_SEG);
    const int trow = (int)(tile / nseg), tseg = (int)(tile % nseg);
    const int x0 = tseg * seglen, x1 = x0 + seglen < bw ? x0 + seglen : bw;
    const int nqseg = n1_nseg(bw, N1_TQ), qlen = n1_seglen(bw, N1_TQ);
    // the l1 side: registers
    double ay[N1_R1], ax[N1_R1], a2y[N1_R1], a2x[N1_R1], ca[N1_R1], ca2[N1_R1], g[N1_R1], acc[N1_R1];
    bool on[N1_R1];
    bool mine = false;
    // thread t owns the columns x0 + t + e N1_NT: the fewest wave-instructions for the tile (co-resident workgroups fill the waves that
    // carry one mode or none; cutting the tile into N1_R1 equal runs instead measured 15 to 35 % slower on boxes 312 and 211 wide)
    for (int e = 0; e < N1_R1; ++e) {
        const int x = x0 + tid + e * N1_NT;
        on[e] = x < x1;
        const N1Q v = a.q[(long)trow * bw + (on[e] ? x : x0)];
        ay[e] = v.y; ax[e] = v.x; a2y[e] = v.y2; a2x[e] = v.x2; ca[e] = v.c; ca2[e] = v.c2;
        g[e] = on[e] ? a.g[(long)trow * bw + x] : 0.0;
        on[e] = on[e] && g[e] != 0.0;
        mine = mine || on[e];
        acc[e] = 0.0;
    }
    if (tid < 4) any[tid] = 0;
    ctx.sync();
    if (mine) any[2] = 1;
    ctx.sync();
    const bool tile_on = any[2] != 0;
    const long nc = n1_nchunks(a.box);
    const long c0 = nc * ctx.bid_y() / a.parts, c1 = nc * (ctx.bid_y() + 1) / a.parts;
    for (long c = tile_on ? c0 : c1; c < c1; ++c) {
        const int qrow = (int)(c / nqseg), qseg = (int)(c % nqseg);
        const int q0 = qseg * qlen, nq = (q0 + qlen < bw ? q0 + qlen : bw) - q0;
        const int slot = (int)((c - c0) & 1);
        // stage the chunk, and Cpp(dy, dx) for dy = tile row - chunk row, dx = x0 - q0 - nq + 1 + i, i < (x1 - x0) + nq - 1
        if (tid == 0) any[slot ^ 1] = 0;
        if (tid < nq) {
            const N1Q v = a.q[(long)qrow * bw + q0 + tid];
            qs[tid] = v;
            if (v.h != 0.0) any[slot] = 1;
        }
        const int dy = trow - qrow, dx0 = x0 - q0 - nq + 1, ncp = (x1 - x0) + nq - 1;
        for (int i = tid; i < ncp; i += N1_NT) cp[i] = n1_hc_at(a.cpp, a.ny, a.kp, dy, dx0 + i);
        ctx.sync();
        if (any[slot]) {
            for (int e = 0; e < N1_R1; ++e) {
                if (!on[e]) continue;
                const double* const cpe = cp + tid + e * N1_NT + nq - 1;   // Cpp(l1 - q_j) = cpe[-j]
                double s = acc[e];
                for (int j = 0; j < nq; ++j) {
                    const N1Q& v = qs[j];
                    double f1, f2;
                    n1_pair_tt(ay[e], ax[e], a2y[e], a2x[e], ca[e], ca2[e], v, f1, f2);
                    s = n1_fma((cpe[-j] * v.h) * f1, f2, s);
                }
                acc[e] = s;
            }
        }
        ctx.sync();
    }
    double t = 0.0;
    for (int e = 0; e < N1_R1; ++e) t += g[e] * acc[e];
    red[tid] = t;
    ctx.sync();
    for (int s = N1_NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        ctx.sync();
    }
    if (tid == 0) a.part[tile * a.parts + ctx.bid_y()] = red[0];
}

/* FOLD.  ONE workgroup of N1_NT threads: thread t adds the partials t, t + N1_NT, ... in that order, then a fixed tree. */
struct N1FoldArgs { const double* part; long n; double* out; };
template <class Ctx>
OA_HD void n1_fold_body(Ctx& ctx, const N1FoldArgs& a) {
    const int tid = ctx.tid();
    double* const red = (double*)ctx.smem();
    double t = 0.0;
    for (long i = tid; i < a.n; i += N1_NT) t += a.part[i];
    red[tid] = t;
    ctx.sync();
    for (int s = N1_NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        ctx.sync();
    }
    if (tid == 0) a.out[0] = red[0];
}

}  // namespace oa
