// Per-mode bodies of oa_mc_run_mv_windowed (pipeline.hip) that are not FFT passes: the Q,U -> E,B rotation on the leg band and the
// mean-field stack of an estimator set, on the plan's own grid and from the inner planes of a band grid.  Shared by the HIP launchers
// (elementwise.hip) and the CPU emulator (tests/emul/emul_win3.cpp, tests/emul/emul_band_mf.cpp).
#pragma once
#include "cx.hpp"

namespace oa {

constexpr int STACK_MULTI_MAX = 6;     // estimators per call (oa_mc_run_mv: nest <= 6)

// row y of the band row index b (b < 2 rb - 1; rb = 0: every row, b = y)
OA_HD int band_row_of(int b, int rb, int ny) { return (rb > 0 && b >= rb) ? b + ny - (2 * rb - 1) : b; }

// Q, U -> E, B in place on the leg band (columns < w, rows y < rb or y > ny - rb) of two hc planes: oa_rot2's combination
// E = Q c - U s, B = Q s + U c, with c, s read from the caller's (ny, pitch) planes at the same mode.  Arithmetic in double, one
// rounding to T (band_cols_fold_body's convention).  One thread per mode: grid (ceil(w / nthreads), band rows).
template <typename T>
struct BandRotArgs {
    const T* c;
    const T* s;
    cx<T>* q;        // in: Q, out: E
    cx<T>* u;        // in: U, out: B
    long pitch;      // row pitch of all four planes (elements of their own type)
    int ny, w, rb;
};
template <typename T, class Ctx>
OA_HD void band_rot2_body(Ctx& ctx, const BandRotArgs<T>& a) {
    const int x = ctx.bid_x() * ctx.nthreads() + ctx.tid();
    if (x >= a.w) return;
    const long at = (long)band_row_of(ctx.bid_y(), a.rb, a.ny) * a.pitch + x;
    const double cc = (double)a.c[at], ss = (double)a.s[at];
    const cx<T> Q = a.q[at], U = a.u[at];
    const double qr = (double)Q.x, qi = (double)Q.y, ur = (double)U.x, ui = (double)U.y;
    a.q[at] = mk<T>((T)(qr * cc - ur * ss), (T)(qi * cc - ui * ss));
    a.u[at] = mk<T>((T)(qr * ss + ur * cc), (T)(qi * ss + ui * cc));
}

// Mean-field stacks of an estimator set: a thread owns ONE mode of kappa's band (columns < w, rows y < rb or y > ny - rb), loads the
// nest kappa_hat values once, adds each into its float64 stack plane and -- wt != nullptr -- adds sum_e w_e kappa_hat_e, formed in
// double in registers in estimator order, into the MV stack.  Every mode has one owner: no atomics, the same sums on every run.
template <typename T>
struct StackMultiArgs {
    const cx<T>* k;  long kstride;     // nest kappa_hat planes, kstride complex elements apart
    const T* wt;     long wstride;     // nest MV weight planes (real), wstride elements apart; nullptr: no MV stack
    cx<double>* acc[STACK_MULTI_MAX];  // the estimators' stacks (indexed by unrolled constants only: the struct stays in registers)
    cx<double>* acc_mv;                // the MV stack (with wt)
    long pitch;                        // row pitch of every plane (elements of its own type)
    int nest, ny, w, rb;
};
template <typename T, class Ctx>
OA_HD void stack_add_region_multi_body(Ctx& ctx, const StackMultiArgs<T>& a) {
    const int x = ctx.bid_x() * ctx.nthreads() + ctx.tid();
    if (x >= a.w) return;
    const long at = (long)band_row_of(ctx.bid_y(), a.rb, a.ny) * a.pitch + x;
    double mr = 0.0, mi = 0.0;
#pragma unroll
    for (int e = 0; e < STACK_MULTI_MAX; ++e) {
        if (e < a.nest) {
            const cx<T> v = a.k[at + e * a.kstride];
            const double vr = (double)v.x, vi = (double)v.y;
            const cx<double> s = a.acc[e][at];
            a.acc[e][at] = mk<double>(s.x + vr, s.y + vi);
            if (a.wt) {
                const double ww = (double)a.wt[at + e * a.wstride];
                mr += ww * vr;
                mi += ww * vi;
            }
        }
    }
    if (a.wt) {
        const cx<double> s = a.acc_mv[at];
        a.acc_mv[at] = mk<double>(s.x + mr, s.y + mi);
    }
}

// The same stacks when kappa_hat lives on the INNER grid of a band grid (oa_mc_run_mv_windowed on map sides 2^a 3^b 5^c): the nest
// kappa_hat planes and the weights (the Monte-Carlo binding's inner-layout copies) are read at the inner pitch and row -- band row i of
// 0 .. 2 r - 2 sits at row i (i < r) or i - (2 r - 1) + rows of either grid --, the float64 stacks are the N grid's.  One thread per mode
// of kappa's band, lanes along columns; one owner per mode: no atomics, the same sums however a range of realisations is cut into calls.
template <typename T>
struct BandStackMultiArgs {
    const cx<T>* k;  long kstride;     // nest inner kappa_hat planes, kstride complex elements apart
    const T* wt;     long wstride;     // nest inner MV weight planes (real), wstride elements apart; nullptr: no MV stack
    cx<double>* acc[STACK_MULTI_MAX];  // the estimators' N-grid stacks
    cx<double>* acc_mv;                // the N-grid MV stack (with wt)
    long ipitch;     int iny;          // inner planes: row pitch (elements of their own type), rows
    long apitch;     int any;          // N-grid stacks: row pitch (complex elements), rows
    int nest, w, r;                    // band: columns < w, rows |ky| < r (r >= 1)
};
template <typename T, class Ctx>
OA_HD void band_stack_add_multi_body(Ctx& ctx, const BandStackMultiArgs<T>& a) {
    const int x = ctx.bid_x() * ctx.nthreads() + ctx.tid();
    if (x >= a.w) return;
    const int i = ctx.bid_y();
    const long src = (long)band_row_of(i, a.r, a.iny) * a.ipitch + x, dst = (long)band_row_of(i, a.r, a.any) * a.apitch + x;
    double mr = 0.0, mi = 0.0;
#pragma unroll
    for (int e = 0; e < STACK_MULTI_MAX; ++e) {
        if (e < a.nest) {
            const cx<T> v = a.k[src + e * a.kstride];
            const double vr = (double)v.x, vi = (double)v.y;
            const cx<double> s = a.acc[e][dst];
            a.acc[e][dst] = mk<double>(s.x + vr, s.y + vi);
            if (a.wt) {
                const double ww = (double)a.wt[src + e * a.wstride];
                mr += ww * vr;
                mi += ww * vi;
            }
        }
    }
    if (a.wt) {
        const cx<double> s = a.acc_mv[dst];
        a.acc_mv[dst] = mk<double>(s.x + mr, s.y + mi);
    }
}

}  // namespace oa
