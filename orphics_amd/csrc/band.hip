// BAND GRID of the one-call entries (TT, and oa_qe_pol / oa_qe_mv / oa_qe_mv_maps behind oa_qe_band_bind) on map sides 2^a 3^b 5^c (pipeline.hip, include/orphics_amd.h): the estimator is
// band-limited, so after the input transform everything runs on a small power-of-two (My, Mx) grid through the fused pow2
// pipeline of an inner plan.  The kernels here move data between the map's N-grid and that inner grid:
//   * band_map_r2c   : real map -> the leg band of its transform (columns < wl, rows |ky| < rl), written in the inner hc layout.
//                      Row pass: the mixed-radix packed N/2 R2C of mixed.hip (fft_mixed.hpp) with only the columns < wl stored
//                      (ny x wl complex instead of ny x (nx/2+1)); column pass: an ny-point DFT evaluated only at the 2 rl - 1 kept
//                      rows (pruned-output DFT, double accumulation, split over row segments + an ordered sum) into the inner plane;
//   * band_maps_r2c  : the same for the <= 6 real maps of one oa_qe_mv_maps call (T, Q, U [, the Y-leg T, Q, U]) in THREE launches
//                      (bodies in fft_band.hpp: band_rows on grid (row, map); band_cols with the twiddle tile staged once and applied to
//                      every map's operand tile; band_cols_fold = the ordered sum + the Q,U -> E,B rotation in double before the one
//                      rounding), straight into the inner source planes of the oa_qe_band_bind binding; map pointers by value;
//   * band_win_r2c   : the front end of oa_mc_run_windowed: <= 6 inverse-column-transformed spectra -> fused C2R x window -> R2C rows
//                      (band_rows_win, fft_band.hpp; the real map in LDS only, the leg columns stored) -> the same pruned column DFT;
//   * band_copy      : band region (rows |ky| < r, columns < w) of one grid's hc-layout plane -> the other grid's (filters, bin ids,
//                      Fourier-space legs N -> inner; kappa_hat inner -> N), optionally scaled;
//   * band_stack_add : the mean-field stack update of oa_mc_run (f64 interleaved N-grid accumulator += inner kappa_hat planes);
//   * band_embed     : the leg band of n Fourier-space source planes (T, E, B [, the Y-leg sources of a split call]) of oa_qe_pol /
//                      oa_qe_mv -> n inner planes, ONE launch through a device table of sources (planes on grid z);
//   * band_scatter   : kappa_hat's band, inner -> N grid, overwriting, adding (accumulate) or with the zero-fill of the complement
//                      in the same launch;
//   * band_scatter_batch : the same for the n^2 evenly spaced inner kappa planes of oa_qe_tt_splits -> n^2 N-grid planes through a
//                      device table of destinations, ONE launch (planes on grid z);
//   * band_split_power : the split-based 4-point combination (split_power.hpp) of those n^2 inner planes per mode, stored to the
//                      N-grid real half-plane -- the K_ij never exist on the N grid.
// A mode of signed index ky sits at row ky mod ny on one grid and ky mod My on the other; the columns are the same.
#include <algorithm>
#include "fft_launch.hpp"
#include "fft_mixed.hpp"
#include "fft_band.hpp"
#include "split_power.hpp"

namespace oa {

// one map row per workgroup: packed N/2-point mixed-radix transform + untangle (mr_row_body, MR_R2C), store of columns < w only
template <typename T>
struct BandRowArgs {
    const T* in;
    cx<T>* out;
    long in_pitch;                   // reals per map row
    int w, N;                        // stored columns; packed transform length nx / 2
    MrFactors f;
    const cx<T>* tw;                 // W_N^e
    const cx<T>* tw2;                // W_2N^e (untangle)
};
template <typename T>
__global__ __launch_bounds__(256) void band_row_kernel(BandRowArgs<T> a) {
    const T* __restrict__ in = a.in;
    cx<T>* __restrict__ out = a.out;
    const long in_pitch = a.in_pitch;
    const int w = a.w, N = a.N;
    const cx<T>* __restrict__ tw = a.tw;
    const cx<T>* __restrict__ tw2 = a.tw2;
    GpuCtx c{oa_dyn_smem};
    cx<T>* b0 = reinterpret_cast<cx<T>*>(c.smem());
    cx<T>* b1 = b0 + N + 1;
    const int tid = threadIdx.x, NT = blockDim.x;
    const long row = blockIdx.x;
    const cx<T>* src = reinterpret_cast<const cx<T>*>(in + row * in_pitch);
    for (int n = tid; n < N; n += NT) b0[n] = src[n];
    c.sync();
    const cx<T>* r = mr_transform<T>(c, b0, b1, N, a.f, 0, tw, tid, NT);
    cx<T>* dst = out + row * w;
    for (int k = tid; k < w; k += NT) {
        const cx<T> Zk = r[k == N ? 0 : k], Zm = conj(r[k == 0 ? 0 : N - k]);
        const cx<T> E = (Zk + Zm) * (T)0.5, O = mul_mi(Zk - Zm) * (T)0.5;
        dst[k] = E + tw2[k] * O;
    }
}

// pruned-output column DFT: out[ky, x] = sum_y rows[y, x] W_ny^(ky y) for |ky| < rl, x < w; a workgroup owns 16 columns x 16 output
// rows x one SEGMENT of yseg rows and walks it in chunks of 32 (operands and twiddles staged in LDS as doubles; accumulation in double
// for both precisions); its partial sums go to part[seg][k][x], which band_cols_sum adds in segment order (deterministic).  With one
// segment per tile the 1200^2 leg band is 28 workgroups of 1200 rows each (~100 us); segments give the chip a few hundred
// (band_cols_segments, fft_band.hpp).
size_t band_map_scratch_bytes(const oa_plan* p, int wl, int rl) {
    int ys = 0;
    const int nseg = band_cols_segments(p->ny, wl, rl, &ys);
    return (size_t)p->ny * wl * 2 * (p->dtype == OA_F32 ? 4 : 8) + (size_t)nseg * (2 * rl - 1) * wl * sizeof(double2);
}
template <typename T>
__global__ __launch_bounds__(256) void band_cols_kernel(const cx<T>* __restrict__ rows, int ny, int w, int rl, const cx<T>* __restrict__ tw,
                                                        double2* __restrict__ part, int yseg) {
    __shared__ double2 A[BC_YC][BC_TX];
    __shared__ double2 W[BC_TK][BC_YC];
    const int tid = threadIdx.x, tx = tid & (BC_TX - 1), tk = tid / BC_TX;
    const int x0 = blockIdx.x * BC_TX, k0 = blockIdx.y * BC_TK;
    const int nk = 2 * rl - 1;
    double ar = 0.0, ai = 0.0;
    const int ybeg = blockIdx.z * yseg, yend = std::min(ny, ybeg + yseg);
    for (int y0 = ybeg; y0 < yend; y0 += BC_YC) {
        for (int e = tid; e < BC_YC * BC_TX; e += 256) {
            const int yy = e / BC_TX, cc = e % BC_TX, y = y0 + yy, x = x0 + cc;
            double2 v = make_double2(0.0, 0.0);
            if (y < ny && x < w) { const cx<T> s = rows[(long)y * w + x]; v = make_double2((double)s.x, (double)s.y); }
            A[yy][cc] = v;
        }
        for (int e = tid; e < BC_TK * BC_YC; e += 256) {
            const int kk = e / BC_YC, yy = e % BC_YC, y = y0 + yy, ki = k0 + kk;
            double2 v = make_double2(0.0, 0.0);
            if (y < ny && ki < nk) {
                const int kmod = band_row(ki, rl, ny);                                   // ky mod ny
                const cx<T> t = tw[(int)(((long)kmod * y) % ny)];
                v = make_double2((double)t.x, (double)t.y);
            }
            W[kk][yy] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int yy = 0; yy < BC_YC; ++yy) {
            const double2 a = A[yy][tx], t = W[tk][yy];
            ar = fma(a.x, t.x, fma(-a.y, t.y, ar));
            ai = fma(a.x, t.y, fma(a.y, t.x, ai));
        }
        __syncthreads();
    }
    const int x = x0 + tx, ki = k0 + tk;
    if (x < w && ki < nk) part[((long)blockIdx.z * nk + ki) * w + x] = make_double2(ar, ai);
}
template <typename T>
__global__ __launch_bounds__(256) void band_cols_sum(const double2* __restrict__ part, int nseg, int w, int rl, cx<T>* __restrict__ out, int my,
                                                     long okp) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, ki = blockIdx.y, nk = 2 * rl - 1;
    if (x >= w) return;
    double ar = 0.0, ai = 0.0;
    for (int s = 0; s < nseg; ++s) { const double2 v = part[((long)s * nk + ki) * w + x]; ar += v.x; ai += v.y; }
    out[(long)band_row(ki, rl, my) * okp + x] = mk<T>((T)ar, (T)ai);
}

// the column stage of ONE row plane (rowbuf: ny x wl complex, then the partial sums: band_map_scratch_bytes) -> the inner plane dst
template <typename T>
static int cols_single_t(oa_plan* p, void* rowbuf, int wl, int rl, void* dst, int dny, long dkp, hipStream_t st) {
    int yseg = 0;
    const int nseg = band_cols_segments(p->ny, wl, rl, &yseg);
    double2* part = reinterpret_cast<double2*>((char*)rowbuf + (size_t)p->ny * wl * sizeof(cx<T>));     // (band_map_scratch_bytes)
    dim3 grid((wl + BC_TX - 1) / BC_TX, (2 * rl - 1 + BC_TK - 1) / BC_TK, nseg);
    hipLaunchKernelGGL(band_cols_kernel<T>, grid, dim3(256), 0, st, (const cx<T>*)rowbuf, p->ny, wl, rl, (const cx<T>*)p->mr_twy, part, yseg);
    OA_LAUNCH_CHECK();
    hipLaunchKernelGGL(band_cols_sum<T>, dim3((wl + 255) / 256, 2 * rl - 1), dim3(256), 0, st, (const double2*)part, nseg, wl, rl, (cx<T>*)dst, dny, dkp);
    OA_LAUNCH_CHECK();
    return 0;
}
template <typename T>
static int map_r2c_t(oa_plan* p, const void* map, void* rowbuf, int wl, int rl, void* dst, int dny, long dkp, hipStream_t st) {
    const int N = p->nx / 2;
    int rc = 0;
    BandRowArgs<T> a{(const T*)map, (cx<T>*)rowbuf, (long)p->nx, wl, N, mixed_factor(N), (const cx<T>*)p->mr_twxh, (const cx<T>*)p->mr_twx};
    launch_go(rc, st, band_row_kernel<T>, dim3(p->ny), 256, 2 * ((size_t)N + 1) * sizeof(cx<T>), a);
    if (rc) return rc;
    return cols_single_t<T>(p, rowbuf, wl, rl, dst, dny, dkp, st);
}
int band_map_r2c(oa_plan* p, const void* map, void* rowbuf, int wl, int rl, void* dst, int dny, long dkp, hipStream_t st) {
    OA_REQUIRE(p->mixed && wl >= 1 && wl <= p->nx / 2 && rl >= 1 && 2 * rl - 1 <= std::min(p->ny, dny), "band input transform: bad band");
    return p->dtype == OA_F32 ? map_r2c_t<float>(p, map, rowbuf, wl, rl, dst, dny, dkp, st)
                              : map_r2c_t<double>(p, map, rowbuf, wl, rl, dst, dny, dkp, st);
}

// BATCHED band input transform of oa_qe_mv_maps (bodies: fft_band.hpp): nmaps real maps -> the leg band of their transforms in nmaps
// inner planes dstride elements apart, with the Q,U -> E,B rotation of the pairs (1, 2) / (4, 5) when rot_c / rot_s are given.  Three
// launches whatever nmaps is; the map pointers travel by value.  scratch: band_maps_scratch_bytes(p, nmaps, wl, rl) bytes -- the row
// planes of all maps, then (256-byte aligned) the partial sums of all maps, each sized as in band_map_scratch_bytes.
template <typename T>
__global__ __launch_bounds__(256) void band_rows_kernel(BandRowsArgs<T> a) {
    GpuCtx c{oa_dyn_smem};
    band_rows_body<T>(c, a);
}
template <typename T, int NM>
__global__ __launch_bounds__(256) void band_colsn_kernel(BandColsArgs<T> a) {
    __shared__ __attribute__((aligned(16))) char lds[band_cols_lds<NM>()];
    GpuCtx c{lds};
    band_cols_body<T, NM>(c, a);
}
template <typename T>
__global__ __launch_bounds__(256) void band_cols_fold_kernel(BandFoldArgs<T> a) {
    GpuCtx c{nullptr};
    band_cols_fold_body<T>(c, a);
}
static size_t band_maps_rows_bytes(const oa_plan* p, int nmaps, int wl) {
    const size_t b = (size_t)nmaps * p->ny * wl * 2 * (p->dtype == OA_F32 ? 4 : 8);
    return (b + 255) / 256 * 256;
}
size_t band_maps_scratch_bytes(const oa_plan* p, int nmaps, int wl, int rl) {
    int ys = 0;
    const int nseg = band_cols_segments(p->ny, wl, rl, &ys);
    return band_maps_rows_bytes(p, nmaps, wl) + (size_t)nmaps * nseg * (2 * rl - 1) * wl * sizeof(cx<double>);
}
// the column stage of n row planes (scratch: the planes ny x wl complex each, then -- 256-byte aligned -- their partial sums:
// band_maps_scratch_bytes) -> n inner planes dstride elements apart, with the rotation of the pairs (1, 2) / (4, 5) when rot_c / rot_s
// are given: the pruned column DFT of all planes in one launch, then the ordered fold
template <typename T>
static int cols_batched_t(oa_plan* p, int n, void* scratch, int wl, int rl, const void* rot_c, const void* rot_s, void* dst, long dstride, int dny,
                          long dkp, hipStream_t st) {
    BandColsArgs<T> ca{};
    ca.rows = (const cx<T>*)scratch; ca.rows_mstride = (long)p->ny * wl; ca.ny = p->ny; ca.w = wl; ca.rl = rl;
    ca.nseg = band_cols_segments(p->ny, wl, rl, &ca.yseg);
    ca.tw = (const cx<T>*)p->mr_twy;
    ca.part = reinterpret_cast<cx<double>*>((char*)scratch + band_maps_rows_bytes(p, n, wl));
    const dim3 grid((wl + BC_TX - 1) / BC_TX, (2 * rl - 1 + BC_TK - 1) / BC_TK, ca.nseg);
    switch (n) {
        case 1: hipLaunchKernelGGL((band_colsn_kernel<T, 1>), grid, dim3(256), 0, st, ca); break;
        case 2: hipLaunchKernelGGL((band_colsn_kernel<T, 2>), grid, dim3(256), 0, st, ca); break;
        case 3: hipLaunchKernelGGL((band_colsn_kernel<T, 3>), grid, dim3(256), 0, st, ca); break;
        case 4: hipLaunchKernelGGL((band_colsn_kernel<T, 4>), grid, dim3(256), 0, st, ca); break;
        case 5: hipLaunchKernelGGL((band_colsn_kernel<T, 5>), grid, dim3(256), 0, st, ca); break;
        default: hipLaunchKernelGGL((band_colsn_kernel<T, 6>), grid, dim3(256), 0, st, ca); break;
    }
    OA_LAUNCH_CHECK();
    BandFoldArgs<T> fa{};
    fa.part = ca.part; fa.nmaps = n; fa.nseg = ca.nseg; fa.w = wl; fa.rl = rl;
    fa.rot_c = (const T*)rot_c; fa.rot_s = (const T*)rot_s; fa.rot_pitch = p->kp; fa.ny = p->ny;
    fa.out = (cx<T>*)dst; fa.out_mstride = dstride; fa.okp = dkp; fa.my = dny;
    hipLaunchKernelGGL(band_cols_fold_kernel<T>, dim3((wl + 255) / 256, 2 * rl - 1), dim3(256), 0, st, fa);
    OA_LAUNCH_CHECK();
    return 0;
}
template <typename T>
static int maps_r2c_t(oa_plan* p, int nmaps, const void* const* maps, const void* rot_c, const void* rot_s, void* scratch, int wl, int rl, void* dst,
                      long dstride, int dny, long dkp, hipStream_t st) {
    const int N = p->nx / 2;
    int rc = 0;
    BandRowsArgs<T> ra{};
    for (int m = 0; m < BAND_MAPS_MAX; ++m) ra.maps.m[m] = (const T*)maps[m < nmaps ? m : 0];
    ra.out = (cx<T>*)scratch; ra.in_pitch = p->nx; ra.out_mstride = (long)p->ny * wl; ra.w = wl; ra.N = N; ra.f = mixed_factor(N);
    ra.tw = (const cx<T>*)p->mr_twxh; ra.tw2 = (const cx<T>*)p->mr_twx;
    launch_go(rc, st, band_rows_kernel<T>, dim3(p->ny, nmaps), 256, band_rows_lds<T>(N), ra);
    if (rc) return rc;
    return cols_batched_t<T>(p, nmaps, scratch, wl, rl, rot_c, rot_s, dst, dstride, dny, dkp, st);
}
// FRONT END of oa_mc_run_windowed on these sides (body: fft_band.hpp band_rows_win_body): the fused windowed row pass of B realisations in one
// launch, then the pruned column DFT with the realisations in the place of maps and no rotation (batched: band_colsn_kernel +
// band_cols_fold_kernel on the layout of band_maps_scratch_bytes; single: band_cols_kernel + band_cols_sum on band_map_scratch_bytes').
// oa_mc_run_mv_windowed passes the T, Q, U planes of ONE realisation as the batch (B = 3) and rot_c / rot_s: the fold then rotates the
// pair (1, 2) Q, U -> E, B, as for band_maps_r2c.
template <typename T>
__global__ __launch_bounds__(BRW_NT, waves_per_eu<T>()) void band_rows_win_kernel(BandRowsWinArgs<T> a) {
    GpuCtx c{oa_dyn_smem};
    band_rows_win_body<T>(c, a);
}
template <typename T>
static int win_r2c_t(oa_plan* p, int B, const void* hc_in, long in_bstride, const void* window, double scale, void* scratch, int single, int wl,
                     int rl, const void* rot_c, const void* rot_s, void* dst, long dstride, int dny, long dkp, hipStream_t st) {
    const int N = p->nx / 2;
    int rc = 0;
    BandRowsWinArgs<T> ra{};
    ra.in = (const cx<T>*)hc_in; ra.in_pitch = p->kp; ra.in_bstride = in_bstride; ra.win = (const T*)window;
    ra.out = (cx<T>*)scratch; ra.out_bstride = (long)p->ny * wl; ra.w = wl; ra.N = N; ra.scale = (T)scale; ra.f = mixed_factor(N);
    ra.tw = (const cx<T>*)p->mr_twxh; ra.tw2 = (const cx<T>*)p->mr_twx;
    launch_go(rc, st, band_rows_win_kernel<T>, dim3(p->ny, B), BRW_NT, band_rows_lds<T>(N), ra);
    if (rc) return rc;
    if (single) return cols_single_t<T>(p, scratch, wl, rl, dst, dny, dkp, st);
    return cols_batched_t<T>(p, B, scratch, wl, rl, rot_c, rot_s, dst, dstride, dny, dkp, st);
}
bool band_rows_win_ok(const oa_plan* p) { return band_rows_win_fits(p->nx / 2); }
int band_win_r2c(oa_plan* p, int B, const void* hc_in, long in_bstride, const void* window, double scale, void* scratch, int single, int wl, int rl,
                 const void* rot_c, const void* rot_s, void* dst, long dstride, int dny, long dkp, hipStream_t st) {
    OA_REQUIRE(p->mixed && wl >= 1 && wl <= p->nx / 2 && rl >= 1 && 2 * rl - 1 <= std::min(p->ny, dny), "band windowed front end: bad band");
    OA_REQUIRE(B >= 1 && B <= BAND_MAPS_MAX && (!single || B == 1) && wl <= dkp && (B == 1 || (long)dny * dkp <= dstride) &&
               (B == 1 || (long)p->ny * p->kp <= in_bstride), "band windowed front end: bad planes");
    OA_REQUIRE(band_rows_win_fits(p->nx / 2), "band windowed front end: map rows longer than 8192 points");
    OA_REQUIRE((!rot_c && !rot_s) || (rot_c && rot_s && !single && (B == 3 || B == 6) && wl <= p->kp), "band windowed front end: bad rotation planes");
    return p->dtype == OA_F32 ? win_r2c_t<float>(p, B, hc_in, in_bstride, window, scale, scratch, single, wl, rl, rot_c, rot_s, dst, dstride, dny, dkp, st)
                              : win_r2c_t<double>(p, B, hc_in, in_bstride, window, scale, scratch, single, wl, rl, rot_c, rot_s, dst, dstride, dny, dkp, st);
}
int band_maps_r2c(oa_plan* p, int nmaps, const void* const* maps, const void* rot_c, const void* rot_s, void* scratch, int wl, int rl, void* dst,
                  long dstride, int dny, long dkp, hipStream_t st) {
    OA_REQUIRE(p->mixed && wl >= 1 && wl <= p->nx / 2 && rl >= 1 && 2 * rl - 1 <= std::min(p->ny, dny), "band input transform: bad band");
    OA_REQUIRE(nmaps >= 1 && nmaps <= BAND_MAPS_MAX && wl <= dkp && wl <= p->kp && (long)dny * dkp <= dstride, "band input transform: bad planes");
    OA_REQUIRE((!rot_c && !rot_s) || (rot_c && rot_s && (nmaps == 3 || nmaps == 6)), "band input transform: bad rotation planes");
    return p->dtype == OA_F32 ? maps_r2c_t<float>(p, nmaps, maps, rot_c, rot_s, scratch, wl, rl, dst, dstride, dny, dkp, st)
                              : maps_r2c_t<double>(p, nmaps, maps, rot_c, rot_s, scratch, wl, rl, dst, dstride, dny, dkp, st);
}

template <typename E> OA_D E band_scaled(E v, double) { return v; }
OA_D float band_scaled(float v, double s) { return (float)((double)v * s); }
OA_D double band_scaled(double v, double s) { return v * s; }
template <typename E>
__global__ __launch_bounds__(256) void band_copy_kernel(const E* __restrict__ src, long spitch, int sny, E* __restrict__ dst, long dpitch, int dny,
                                                        int w, int r, double scale) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= w) return;
    const int i = blockIdx.y;
    dst[(long)band_row(i, r, dny) * dpitch + x] = band_scaled(src[(long)band_row(i, r, sny) * spitch + x], scale);
}
// kind: 0 f32, 1 f64, 2 int32 (real planes), 3 complex f32, 4 complex f64; scale applies to the real float kinds only
int band_copy(int kind, const void* src, long spitch, int sny, void* dst, long dpitch, int dny, int w, int r, double scale, hipStream_t st) {
    OA_REQUIRE(w >= 1 && r >= 1 && 2 * r - 1 <= std::min(sny, dny), "band copy: bad band");
    OA_REQUIRE(w <= spitch && w <= dpitch, "band copy: band wider than a plane's row pitch");
    dim3 grid((w + 255) / 256, 2 * r - 1);
    switch (kind) {
        case 0: hipLaunchKernelGGL(band_copy_kernel<float>, grid, dim3(256), 0, st, (const float*)src, spitch, sny, (float*)dst, dpitch, dny, w, r, scale); break;
        case 1: hipLaunchKernelGGL(band_copy_kernel<double>, grid, dim3(256), 0, st, (const double*)src, spitch, sny, (double*)dst, dpitch, dny, w, r, scale); break;
        case 2: hipLaunchKernelGGL(band_copy_kernel<int32_t>, grid, dim3(256), 0, st, (const int32_t*)src, spitch, sny, (int32_t*)dst, dpitch, dny, w, r, scale); break;
        case 3: hipLaunchKernelGGL(band_copy_kernel<cx<float>>, grid, dim3(256), 0, st, (const cx<float>*)src, spitch, sny, (cx<float>*)dst, dpitch, dny, w, r, scale); break;
        case 4: hipLaunchKernelGGL(band_copy_kernel<cx<double>>, grid, dim3(256), 0, st, (const cx<double>*)src, spitch, sny, (cx<double>*)dst, dpitch, dny, w, r, scale); break;
        default: return fail("band copy: bad kind");
    }
    OA_LAUNCH_CHECK();
    return 0;
}

// zero every element of an (ny, kp) hc plane outside kappa's band (columns < w of the rows |ky| < r), element by element: on these sides
// kp = nx / 2 + 16 may be odd, so rows are not 16-byte units (pipeline.hip's zero_complement assumes they are)
template <typename T>
__global__ __launch_bounds__(256) void band_zero_kernel(cx<T>* __restrict__ out, int ny, long kp, int w, int r) {
    const int y = blockIdx.y;
    const bool band = y < r || y > ny - r;
    for (long x = (band ? w : 0) + blockIdx.x * (long)blockDim.x + threadIdx.x; x < kp; x += (long)gridDim.x * blockDim.x)
        out[(long)y * kp + x] = mk<T>((T)0, (T)0);
}
int band_zero_outside(int dtype, void* out, int ny, long kp, int w, int r, hipStream_t st) {
    OA_REQUIRE(w >= 1 && w <= kp && r >= 1 && 2 * r - 1 <= ny, "band zero: bad band");
    dim3 grid((unsigned)std::min<long>(4, (kp + 255) / 256), ny);
    if (dtype == OA_F32) hipLaunchKernelGGL(band_zero_kernel<float>, grid, dim3(256), 0, st, (cx<float>*)out, ny, kp, w, r);
    else hipLaunchKernelGGL(band_zero_kernel<double>, grid, dim3(256), 0, st, (cx<double>*)out, ny, kp, w, r);
    OA_LAUNCH_CHECK();
    return 0;
}

// n source planes (device table `srcs`, N-grid hc layout) -> n inner planes dstride elements apart, band rows |ky| < r, columns < w.
// A workgroup is 4 band rows x 64 columns: each wave reads and writes one contiguous row segment.
template <typename T>
__global__ __launch_bounds__(256) void band_embed_kernel(const cx<T>* const* __restrict__ srcs, long spitch, int sny, cx<T>* __restrict__ dst,
                                                         long dstride, long dpitch, int dny, int w, int r) {
    const int x = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || i >= 2 * r - 1) return;
    const cx<T>* __restrict__ src = srcs[blockIdx.z];
    dst[blockIdx.z * dstride + (long)band_row(i, r, dny) * dpitch + x] = src[(long)band_row(i, r, sny) * spitch + x];
}
int band_embed(int dtype, const void* const* dev_srcs, int n, long spitch, int sny, void* dst, long dstride, long dpitch, int dny, int w, int r,
               hipStream_t st) {
    OA_REQUIRE(n >= 1 && w >= 1 && r >= 1 && 2 * r - 1 <= std::min(sny, dny), "band embed: bad band");
    OA_REQUIRE(w <= spitch && w <= dpitch && (long)dny * dpitch <= dstride, "band embed: band wider than a plane's row pitch");
    dim3 grid((w + 63) / 64, (2 * r - 1 + 3) / 4, n), block(64, 4);
    if (dtype == OA_F32)
        hipLaunchKernelGGL(band_embed_kernel<float>, grid, block, 0, st, (const cx<float>* const*)dev_srcs, spitch, sny, (cx<float>*)dst, dstride, dpitch, dny, w, r);
    else
        hipLaunchKernelGGL(band_embed_kernel<double>, grid, block, 0, st, (const cx<double>* const*)dev_srcs, spitch, sny, (cx<double>*)dst, dstride, dpitch, dny, w, r);
    OA_LAUNCH_CHECK();
    return 0;
}

// kappa_hat's band of the inner plane -> the N-grid plane `out`: mode 0 overwrites the band, mode 1 (accumulate) reads, adds and
// writes the band only.  Mode 2 (zero_outside) SHARES ITS LAUNCH with the zero-fill: the workgroups walk every row of `out` and store
// either the band value or zero, element by element over all okp columns (what band_zero_outside + a band copy wrote in two launches).
template <typename T>
__global__ __launch_bounds__(256) void band_scatter_kernel(const cx<T>* __restrict__ src, long spitch, int sny, cx<T>* __restrict__ out, long okp,
                                                           int ony, int w, int r, int accumulate) {
    const int x = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || i >= 2 * r - 1) return;
    const cx<T> v = src[(long)band_row(i, r, sny) * spitch + x];
    cx<T>* o = out + (long)band_row(i, r, ony) * okp + x;
    *o = accumulate ? *o + v : v;
}
template <typename T>
__global__ __launch_bounds__(256) void band_scatter_zero_kernel(const cx<T>* __restrict__ src, long spitch, int sny, cx<T>* __restrict__ out,
                                                                long okp, int ony, int w, int r) {
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (y >= ony) return;
    const bool band = y < r || y > ony - r;
    const cx<T>* __restrict__ srow = src + (long)(y < r ? y : y - ony + sny) * spitch;      // (read on band rows only)
    cx<T>* __restrict__ orow = out + (long)y * okp;
    for (long x = blockIdx.x * 64 + threadIdx.x; x < okp; x += (long)gridDim.x * 64)
        orow[x] = (band && x < w) ? srow[x] : mk<T>((T)0, (T)0);
}
int band_scatter(int dtype, const void* src, long spitch, int sny, void* out, long okp, int ony, int w, int r, int mode, hipStream_t st) {
    OA_REQUIRE(w >= 1 && r >= 1 && 2 * r - 1 <= std::min(sny, ony), "band scatter: bad band");
    OA_REQUIRE(w <= spitch && w <= okp, "band scatter: band wider than a plane's row pitch");
    const dim3 block(64, 4);
    if (mode == 2) {
        dim3 grid((unsigned)std::min<long>(4, (okp + 63) / 64), (ony + 3) / 4);
        if (dtype == OA_F32) hipLaunchKernelGGL(band_scatter_zero_kernel<float>, grid, block, 0, st, (const cx<float>*)src, spitch, sny, (cx<float>*)out, okp, ony, w, r);
        else hipLaunchKernelGGL(band_scatter_zero_kernel<double>, grid, block, 0, st, (const cx<double>*)src, spitch, sny, (cx<double>*)out, okp, ony, w, r);
    } else {
        dim3 grid((w + 63) / 64, (2 * r - 1 + 3) / 4);
        if (dtype == OA_F32) hipLaunchKernelGGL(band_scatter_kernel<float>, grid, block, 0, st, (const cx<float>*)src, spitch, sny, (cx<float>*)out, okp, ony, w, r, mode);
        else hipLaunchKernelGGL(band_scatter_kernel<double>, grid, block, 0, st, (const cx<double>*)src, spitch, sny, (cx<double>*)out, okp, ony, w, r, mode);
    }
    OA_LAUNCH_CHECK();
    return 0;
}

// band_scatter for nplanes inner planes sstride elements apart -> the N-grid planes of the device table `outs` (oa_qe_tt_splits on a band
// grid: all n^2 kappa planes in one launch, plane on grid z).  Same workgroup shape as band_scatter: 4 rows x 64 columns, each wave one
// contiguous row segment.  Without `zero` only the band of each destination is written; with it the workgroups walk every row of the
// destination and store the band value or zero over all okp columns.
template <typename T>
__global__ __launch_bounds__(256) void band_scatter_batch_kernel(const cx<T>* __restrict__ src, long sstride, long spitch, int sny,
                                                                 cx<T>* const* __restrict__ outs, long okp, int ony, int w, int r) {
    const int x = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || i >= 2 * r - 1) return;
    cx<T>* __restrict__ out = outs[blockIdx.z];
    out[(long)band_row(i, r, ony) * okp + x] = src[blockIdx.z * sstride + (long)band_row(i, r, sny) * spitch + x];
}
template <typename T>
__global__ __launch_bounds__(256) void band_scatter_batch_zero_kernel(const cx<T>* __restrict__ src, long sstride, long spitch, int sny,
                                                                      cx<T>* const* __restrict__ outs, long okp, int ony, int w, int r) {
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (y >= ony) return;
    const bool band = y < r || y > ony - r;
    const cx<T>* __restrict__ srow = src + blockIdx.z * sstride + (long)(y < r ? y : y - ony + sny) * spitch;      // (read on band rows only)
    cx<T>* __restrict__ orow = outs[blockIdx.z] + (long)y * okp;
    for (long x = blockIdx.x * 64 + threadIdx.x; x < okp; x += (long)gridDim.x * 64)
        orow[x] = (band && x < w) ? srow[x] : mk<T>((T)0, (T)0);
}
int band_scatter_batch(int dtype, const void* src, long sstride, int nplanes, long spitch, int sny, void* const* dev_outs, long okp, int ony, int w,
                       int r, int zero, hipStream_t st) {
    OA_REQUIRE(nplanes >= 1 && nplanes <= 65535 && w >= 1 && r >= 1 && 2 * r - 1 <= std::min(sny, ony), "band scatter: bad band");
    OA_REQUIRE(w <= spitch && w <= okp && (long)sny * spitch <= sstride, "band scatter: band wider than a plane's row pitch");
    const dim3 block(64, 4);
    if (zero) {
        dim3 grid((unsigned)std::min<long>(4, (okp + 63) / 64), (ony + 3) / 4, nplanes);
        if (dtype == OA_F32) hipLaunchKernelGGL(band_scatter_batch_zero_kernel<float>, grid, block, 0, st, (const cx<float>*)src, sstride, spitch, sny, (cx<float>* const*)dev_outs, okp, ony, w, r);
        else hipLaunchKernelGGL(band_scatter_batch_zero_kernel<double>, grid, block, 0, st, (const cx<double>*)src, sstride, spitch, sny, (cx<double>* const*)dev_outs, okp, ony, w, r);
    } else {
        dim3 grid((w + 63) / 64, (2 * r - 1 + 3) / 4, nplanes);
        if (dtype == OA_F32) hipLaunchKernelGGL(band_scatter_batch_kernel<float>, grid, block, 0, st, (const cx<float>*)src, sstride, spitch, sny, (cx<float>* const*)dev_outs, okp, ony, w, r);
        else hipLaunchKernelGGL(band_scatter_batch_kernel<double>, grid, block, 0, st, (const cx<double>*)src, sstride, spitch, sny, (cx<double>* const*)dev_outs, okp, ony, w, r);
    }
    OA_LAUNCH_CHECK();
    return 0;
}

// The split-based 4-point combination (split_cross_mode: the arithmetic of split_cross_power_kernel, f64 per mode) of the N^2 inner kappa
// planes K[i*N+j] (sstride elements apart) -> the REAL N-grid half-plane `out` (okp reals per row).  Lanes run along columns: every one of
// the N^2 loads of a wave is one contiguous row segment of its plane.  ZERO = false writes kappa's band only (grid: band rows x band
// columns); ZERO = true walks every row of `out` over all okp columns and stores the combination or zero.
template <typename T>
struct SplitBlockLoad {                            // plane k of an evenly spaced block at this mode
    const cx<T>* at; long sstride;
    OA_D cx<T> operator()(int k) const { return at[k * sstride]; }
};
template <typename T, int N, bool ZERO>
__global__ __launch_bounds__(256) void band_split_power_kernel(const cx<T>* __restrict__ src, long sstride, long spitch, int sny, T* __restrict__ out,
                                                               long okp, int ony, int w, int r, double norm) {
    if (ZERO) {
        const int y = blockIdx.y * 4 + threadIdx.y;
        if (y >= ony) return;
        const bool band = y < r || y > ony - r;
        const cx<T>* __restrict__ srow = src + (long)(y < r ? y : y - ony + sny) * spitch;      // (read on band rows only)
        T* __restrict__ orow = out + (long)y * okp;
        for (long x = blockIdx.x * 64 + threadIdx.x; x < okp; x += (long)gridDim.x * 64) {
            double v = 0.0;
            if (band && x < w) v = split_cross_mode<N>(SplitBlockLoad<T>{srow + x, sstride}, norm);
            orow[x] = (T)v;
        }
    } else {
        const int x = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
        if (x >= w || i >= 2 * r - 1) return;
        const double v = split_cross_mode<N>(SplitBlockLoad<T>{src + (long)band_row(i, r, sny) * spitch + x, sstride}, norm);
        out[(long)band_row(i, r, ony) * okp + x] = (T)v;
    }
}
template <typename T, bool ZERO>
static int split_power_t(int n, const void* src, long sstride, long spitch, int sny, void* out, long okp, int ony, int w, int r, double norm,
                         hipStream_t st) {
    const dim3 block(64, 4);
    const dim3 grid = ZERO ? dim3((unsigned)std::min<long>(8, (okp + 63) / 64), (ony + 3) / 4) : dim3((w + 63) / 64, (2 * r - 1 + 3) / 4);
#define OA_BSPLIT_CASE(NN) \
    case NN: hipLaunchKernelGGL((band_split_power_kernel<T, NN, ZERO>), grid, block, 0, st, (const cx<T>*)src, sstride, spitch, sny, (T*)out, okp, ony, w, r, norm); break
    switch (n) {
        OA_BSPLIT_CASE(4); OA_BSPLIT_CASE(5); OA_BSPLIT_CASE(6); OA_BSPLIT_CASE(7); OA_BSPLIT_CASE(8);
        default: return fail("band split power: 4 <= nsplits <= 8");
    }
#undef OA_BSPLIT_CASE
    OA_LAUNCH_CHECK();
    return 0;
}
int band_split_power(int dtype, int nsplits, const void* src, long sstride, long spitch, int sny, void* out_real, long okp, int ony, int w, int r,
                     double norm, int zero, hipStream_t st) {
    OA_REQUIRE(nsplits >= 4 && nsplits <= 8, "band split power: 4 <= nsplits <= 8");
    OA_REQUIRE(w >= 1 && r >= 1 && 2 * r - 1 <= std::min(sny, ony), "band split power: bad band");
    OA_REQUIRE(w <= spitch && w <= okp && (long)sny * spitch <= sstride, "band split power: band wider than a plane's row pitch");
    if (dtype == OA_F32)
        return zero ? split_power_t<float, true>(nsplits, src, sstride, spitch, sny, out_real, okp, ony, w, r, norm, st)
                    : split_power_t<float, false>(nsplits, src, sstride, spitch, sny, out_real, okp, ony, w, r, norm, st);
    return zero ? split_power_t<double, true>(nsplits, src, sstride, spitch, sny, out_real, okp, ony, w, r, norm, st)
                : split_power_t<double, false>(nsplits, src, sstride, spitch, sny, out_real, okp, ony, w, r, norm, st);
}

// acc (N grid, interleaved re / im doubles, apitch complex elements per row) += the nbatch inner planes (sstride complex elements apart), in
// plane order -- the order of stack_add_region
template <typename T>
__global__ __launch_bounds__(256) void band_stack_kernel(const T* __restrict__ src, long spitch, int sny, int nbatch, long sstride,
                                                         double* __restrict__ acc, long apitch, int any, int w, int r) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;      // real-valued element within the row (2 per complex column)
    if (c >= 2 * w) return;
    const int i = blockIdx.y;
    const long si = 2 * (long)band_row(i, r, sny) * spitch + c, ai = 2 * (long)band_row(i, r, any) * apitch + c;
    double a = acc[ai];
    for (int b = 0; b < nbatch; ++b) a += (double)src[si + 2 * b * sstride];
    acc[ai] = a;
}
int band_stack_add(int dtype, const void* src, long spitch, int sny, int nbatch, long sstride, double* acc, long apitch, int any, int w, int r,
                   hipStream_t st) {
    OA_REQUIRE(w >= 1 && r >= 1 && 2 * r - 1 <= std::min(sny, any), "band stack: bad band");
    OA_REQUIRE(w <= spitch && w <= apitch, "band stack: band wider than a plane's row pitch");
    dim3 grid((2 * w + 255) / 256, 2 * r - 1);
    if (dtype == OA_F32)
        hipLaunchKernelGGL(band_stack_kernel<float>, grid, dim3(256), 0, st, (const float*)src, spitch, sny, nbatch, sstride, acc, apitch, any, w, r);
    else
        hipLaunchKernelGGL(band_stack_kernel<double>, grid, dim3(256), 0, st, (const double*)src, spitch, sny, nbatch, sstride, acc, apitch, any, w, r);
    OA_LAUNCH_CHECK();
    return 0;
}

}  // namespace oa
