// BATCHED BAND INPUT STAGE of oa_qe_mv_maps on map sides 2^a 3^b 5^c (band.hip, pipeline.hip): up to BAND_MAPS_MAX real maps -> the leg
// band (columns < w, rows |ky| < rl) of their transforms, written in the hc layout of the inner power-of-two grid, optionally with the
// per-mode Q,U -> E,B rotation; and the FUSED WINDOWED ROW PASS of oa_mc_run_windowed on these sides, which feeds the same column bodies
// with realisations in the place of maps.  Four kernel bodies, templated on the context type so that the CPU thread emulator
// (tests/emul/emul_band.cpp, emul_band_win.cpp) runs the same code as the GPU:
//   * band_rows_body      : grid (row, map); one map row per workgroup: packed N/2-point mixed-radix transform (mr_transform) + untangle,
//                           store of columns < w only into the row plane of its map (the arithmetic of band_row_kernel);
//   * band_rows_win_body  : grid (row, realisation); C2R of an inverse-column-transformed spectrum row -> x window / Npix -> R2C, the real
//                           row in LDS only, store of columns < w into the row plane of its realisation;
//   * band_cols_body      : grid (column tile, output-row tile, segment); the pruned-output column DFT of band_cols_kernel -- same
//                           segments, same 32-row chunks, double accumulation, same fma order per output -- for all maps of the call: the
//                           twiddle tile W[16][32] (with its (k y) mod ny index arithmetic) is staged once per chunk and applied to the
//                           operand tiles of every map, one accumulator pair per map and thread;
//   * band_cols_fold_body : grid (column block, band row); the sum over the segments in segment order (deterministic, no atomics), the
//                           rotation E = Q c - U s, B = Q s + U c in double on the double sums, ONE rounding to T, store to the inner
//                           planes at row band_row(ki, rl, My).
// Only plain C++ and vector stores.
#pragma once
#include <cmath>
#include "fft_mixed.hpp"

namespace oa {

constexpr int BAND_MAPS_MAX = 6;               // T, Q, U and the Y-leg maps of a split call (POL_SRC_MAX of pipeline.hip)

// band row i of 0 .. 2 r - 2 -> signed ky (0 .. r - 1, then -(r - 1) .. -1) -> row of a grid of m rows
OA_HD int band_row(int i, int r, int m) { return i < r ? i : i - (2 * r - 1) + m; }

// tiles of the pruned-output column DFT: 16 columns x 16 output rows per workgroup, chunks of 32 input rows; the input rows are split
// into SEGMENTS so that one map's band gives the chip a few hundred workgroups (the same rule for one map and for a batch: a map's
// partial sums, and so its result, do not depend on how many maps travel with it)
constexpr int BC_TX = 16, BC_TK = 16, BC_YC = 32, BC_TARGET_WG = 512;
inline int band_cols_segments(int ny, int w, int rl, int* yseg) {
    const long tiles = (long)((w + BC_TX - 1) / BC_TX) * ((2 * rl - 1 + BC_TK - 1) / BC_TK);
    long nseg = (ny + BC_YC - 1) / BC_YC;
    if (nseg > BC_TARGET_WG / tiles) nseg = BC_TARGET_WG / tiles;
    if (nseg < 1) nseg = 1;
    int ys = (int)((ny + nseg - 1) / nseg);
    ys = (ys + BC_YC - 1) / BC_YC * BC_YC;
    *yseg = ys;
    return (ny + ys - 1) / ys;
}

// the map pointers of one call travel by value in the kernel arguments; entry m by compares (m is uniform over a workgroup), so the
// argument block is never indexed dynamically
template <typename T> struct BandMapPtrs { const T* m[BAND_MAPS_MAX]; };
template <typename T> OA_HD const T* band_map_ptr(const BandMapPtrs<T>& t, int m) {
    const T* r = t.m[0];
#pragma unroll
    for (int k = 1; k < BAND_MAPS_MAX; ++k) if (k == m) r = t.m[k];
    return r;
}

template <typename T>
struct BandRowsArgs {
    BandMapPtrs<T> maps;             // real planes, in_pitch reals per row
    cx<T>* out;                      // row planes: map m at out + m * out_mstride, w complex per row
    long in_pitch, out_mstride;
    int w, N;                        // stored columns; packed transform length nx / 2
    MrFactors f;
    const cx<T>* tw;                 // W_N^e
    const cx<T>* tw2;                // W_2N^e (untangle)
};
template <typename T> inline size_t band_rows_lds(int N) { return 2 * ((size_t)N + 1) * sizeof(cx<T>); }

template <typename T, class Ctx>
OA_HD void band_rows_body(Ctx& c, const BandRowsArgs<T>& a) {
    const int N = a.N, w = a.w;
    cx<T>* b0 = reinterpret_cast<cx<T>*>(c.smem());
    cx<T>* b1 = b0 + N + 1;
    const int tid = c.tid(), NT = c.nthreads(), m = c.bid_y();
    const long row = c.bid_x();
    const cx<T>* src = reinterpret_cast<const cx<T>*>(band_map_ptr(a.maps, m) + row * a.in_pitch);
    for (int n = tid; n < N; n += NT) b0[n] = src[n];
    c.sync();
    const cx<T>* r = mr_transform<T>(c, b0, b1, N, a.f, 0, a.tw, tid, NT);
    cx<T>* dst = a.out + m * a.out_mstride + row * w;
    for (int k = tid; k < w; k += NT) {
        const cx<T> Zk = r[k == N ? 0 : k], Zm = conj(r[k == 0 ? 0 : N - k]);
        const cx<T> E = (Zk + Zm) * (T)0.5, O = mul_mi(Zk - Zm) * (T)0.5;
        dst[k] = E + a.tw2[k] * O;
    }
}

// FUSED WINDOWED ROW PASS of oa_mc_run_windowed on these sides (the mixed-radix counterpart of the pow2 ROW_WIN pass, fft_kernels.hpp):
// grid (map row, realisation); per row C2R of the inverse-column-transformed spectrum -> x window x scale -> R2C, the real row in LDS
// only, store of columns < w into the row plane of its realisation.  A thread owns the packed elements n = tid + q NT, q < BRW_MAXQ
// (256 threads: N <= 4096), and keeps its window values in registers across the inverse transform: every global load of the row --
// spectrum and window -- is issued before the first barrier, none between the transforms.
constexpr int BRW_NT = 256, BRW_MAXQ = 16;
inline bool band_rows_win_fits(int N) { return N >= 1 && N <= BRW_NT * BRW_MAXQ; }

template <typename T>
struct BandRowsWinArgs {
    const cx<T>* in;                 // inverse-column-transformed spectra: realisation b at in + b * in_bstride, in_pitch complex per row
    long in_pitch, in_bstride;
    const T* win;                    // (ny, 2 N) real window, rows back to back
    cx<T>* out;                      // row planes: realisation b at out + b * out_bstride, w complex per row
    long out_bstride;
    int w, N;                        // stored columns (<= N); packed transform length nx / 2
    T scale;                         // 1 / Npix of the inverse transform, applied with the window
    MrFactors f;
    const cx<T>* tw;                 // W_N^e
    const cx<T>* tw2;                // W_2N^e ((un)tangle)
};

template <typename T, class Ctx>
OA_HD void band_rows_win_body(Ctx& c, const BandRowsWinArgs<T>& a) {
    const int N = a.N, w = a.w;
    cx<T>* b0 = reinterpret_cast<cx<T>*>(c.smem());
    cx<T>* b1 = b0 + N + 1;
    const int tid = c.tid(), NT = c.nthreads(), b = c.bid_y();
    const long row = c.bid_x();
    const cx<T>* src = a.in + b * a.in_bstride + row * a.in_pitch;
    const cx<T>* wrow = reinterpret_cast<const cx<T>*>(a.win + row * 2 * (long)N);
    // all loads of the row, back to back: N window pairs (kept in registers across the inverse transform), N + 1 spectrum columns
    // (to LDS: nothing reads them before the barrier, so the loop's loads are issued together)
    cx<T> wv[BRW_MAXQ];
#pragma unroll
    for (int q = 0; q < BRW_MAXQ; ++q) { const int n = tid + q * NT; wv[q] = n < N ? wrow[n] : mk<T>((T)0, (T)0); }
#pragma unroll
    for (int q = 0; q < BRW_MAXQ; ++q) { const int n = tid + q * NT; if (n < N) b1[n] = src[n]; }
    if (tid == 0) b1[N] = src[N];
    c.sync();
    // C2R pre-twist (mr_row_body, MR_C2R): Z'[k] = (X[k] + conj X[N - k]) + i conj(W_2N^k) (X[k] - conj X[N - k]); the self-conjugate
    // columns k = 0 and k = N keep their real part only; inverse as the forward transform of the swapped data
    for (int k = tid; k < N; k += NT) {
        cx<T> A = b1[k], B = b1[N - k];
        if (k == 0) { A.y = (T)0; B.y = (T)0; }
        const cx<T> z = (A + conj(B)) + mul_pi(conj(a.tw2[k]) * (A - conj(B)));
        b0[k] = swp(z);
    }
    c.sync();
    cx<T>* r = mr_transform<T>(c, b0, b1, N, a.f, 0, a.tw, tid, NT);
    cx<T>* other = r == b0 ? b1 : b0;
    // packed real row z[n] = x[2 n] + i x[2 n + 1] (the swapped result): x window x scale, in place -- a thread touches its own n only
#pragma unroll
    for (int q = 0; q < BRW_MAXQ; ++q) {
        const int n = tid + q * NT;
        if (n < N) { const cx<T> v = swp(r[n]); r[n] = mk<T>(v.x * (wv[q].x * a.scale), v.y * (wv[q].y * a.scale)); }
    }
    c.sync();
    const cx<T>* z = mr_transform<T>(c, r, other, N, a.f, 0, a.tw, tid, NT);
    cx<T>* dst = a.out + b * a.out_bstride + row * w;
    for (int k = tid; k < w; k += NT) {
        const cx<T> Zk = z[k == N ? 0 : k], Zm = conj(z[k == 0 ? 0 : N - k]);
        const cx<T> E = (Zk + Zm) * (T)0.5, O = mul_mi(Zk - Zm) * (T)0.5;
        dst[k] = E + a.tw2[k] * O;
    }
}

template <typename T>
struct BandColsArgs {
    const cx<T>* rows;               // row planes of band_rows_body, map m at rows + m * rows_mstride
    long rows_mstride;
    int ny, w, rl, yseg, nseg;
    const cx<T>* tw;                 // W_ny^e
    cx<double>* part;                // partial sums [map][segment][band row][w]
};
// LDS: the operand tiles A[NM][32][16] and the twiddle tile W[16][32], doubles (57 344 bytes for six maps)
template <int NM> constexpr size_t band_cols_lds() { return ((size_t)NM * BC_YC * BC_TX + (size_t)BC_TK * BC_YC) * sizeof(cx<double>); }

// 256 threads: thread (tx, tk) owns column x0 + tx of output row k0 + tk for every map
template <typename T, int NM, class Ctx>
OA_HD void band_cols_body(Ctx& c, const BandColsArgs<T>& a) {
    cx<double>* A = reinterpret_cast<cx<double>*>(c.smem());          // [NM][BC_YC][BC_TX]
    cx<double>* W = A + NM * BC_YC * BC_TX;                           // [BC_TK][BC_YC]
    const int tid = c.tid(), NT = c.nthreads(), tx = tid & (BC_TX - 1), tk = tid / BC_TX;
    const int x0 = c.bid_x() * BC_TX, k0 = c.bid_y() * BC_TK, seg = c.bid_z();
    const int ny = a.ny, w = a.w, rl = a.rl, nk = 2 * rl - 1;
    double ar[NM], ai[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) { ar[m] = 0.0; ai[m] = 0.0; }
    const int ybeg = seg * a.yseg, yend = ybeg + a.yseg < ny ? ybeg + a.yseg : ny;
    for (int y0 = ybeg; y0 < yend; y0 += BC_YC) {
        for (int e = tid; e < NM * BC_YC * BC_TX; e += NT) {
            const int m = e / (BC_YC * BC_TX), yy = (e / BC_TX) % BC_YC, cc = e % BC_TX, y = y0 + yy, x = x0 + cc;
            cx<double> v = mk<double>(0.0, 0.0);
            if (y < ny && x < w) { const cx<T> s = a.rows[m * a.rows_mstride + (long)y * w + x]; v = mk<double>((double)s.x, (double)s.y); }
            A[e] = v;
        }
        for (int e = tid; e < BC_TK * BC_YC; e += NT) {
            const int kk = e / BC_YC, yy = e % BC_YC, y = y0 + yy, ki = k0 + kk;
            cx<double> v = mk<double>(0.0, 0.0);
            if (y < ny && ki < nk) {
                const int kmod = band_row(ki, rl, ny);                                   // ky mod ny
                const cx<T> t = a.tw[(int)(((long)kmod * y) % ny)];
                v = mk<double>((double)t.x, (double)t.y);
            }
            W[e] = v;
        }
        c.sync();
#pragma unroll 8
        for (int yy = 0; yy < BC_YC; ++yy) {
            const cx<double> t = W[tk * BC_YC + yy];
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const cx<double> v = A[(m * BC_YC + yy) * BC_TX + tx];
                ar[m] = fma(v.x, t.x, fma(-v.y, t.y, ar[m]));
                ai[m] = fma(v.x, t.y, fma(v.y, t.x, ai[m]));
            }
        }
        c.sync();
    }
    const int x = x0 + tx, ki = k0 + tk;
    if (x < w && ki < nk) {
#pragma unroll
        for (int m = 0; m < NM; ++m) a.part[(((long)m * a.nseg + seg) * nk + ki) * w + x] = mk<double>(ar[m], ai[m]);
    }
}

template <typename T>
struct BandFoldArgs {
    const cx<double>* part;          // [map][segment][band row][w]
    int nmaps, nseg, w, rl;
    const T* rot_c;                  // both nullptr, or the N-grid (ny, rot_pitch) planes cos / sin 2 phi_ell: only their band is read
    const T* rot_s;
    long rot_pitch;
    int ny;
    cx<T>* out;                      // inner hc planes, map m at out + m * out_mstride, okp complex per row, my rows
    long out_mstride, okp;
    int my;
};

// one thread per (column, band row): every map's sum over the segments in segment order, then the rotation of the pairs (1, 2) and
// (4, 5) in double, one rounding to T
template <typename T, class Ctx>
OA_HD void band_cols_fold_body(Ctx& c, const BandFoldArgs<T>& a) {
    const int x = c.bid_x() * c.nthreads() + c.tid(), ki = c.bid_y(), nk = 2 * a.rl - 1;
    if (x >= a.w) return;
    double sr[BAND_MAPS_MAX], si[BAND_MAPS_MAX];
#pragma unroll
    for (int m = 0; m < BAND_MAPS_MAX; ++m) {
        double r = 0.0, i = 0.0;
        if (m < a.nmaps)
            for (int s = 0; s < a.nseg; ++s) { const cx<double> v = a.part[(((long)m * a.nseg + s) * nk + ki) * a.w + x]; r += v.x; i += v.y; }
        sr[m] = r; si[m] = i;
    }
    if (a.rot_c) {
        const long at = (long)band_row(ki, a.rl, a.ny) * a.rot_pitch + x;
        const double cc = (double)a.rot_c[at], ss = (double)a.rot_s[at];
#pragma unroll
        for (int q = 1; q + 1 < BAND_MAPS_MAX; q += 3) {
            if (q + 1 < a.nmaps) {
                const double qr = sr[q], qi = si[q], ur = sr[q + 1], ui = si[q + 1];
                sr[q] = qr * cc - ur * ss;     si[q] = qi * cc - ui * ss;
                sr[q + 1] = qr * ss + ur * cc; si[q + 1] = qi * ss + ui * cc;
            }
        }
    }
    const long o = (long)band_row(ki, a.rl, a.my) * a.okp + x;
#pragma unroll
    for (int m = 0; m < BAND_MAPS_MAX; ++m)
        if (m < a.nmaps) a.out[m * a.out_mstride + o] = mk<T>((T)sr[m], (T)si[m]);
}

}  // namespace oa
