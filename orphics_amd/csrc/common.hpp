// Shared host-side helpers for the C-ABI implementation files.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include "../../include/orphics_amd.h"
#include "cx.hpp"

namespace oa {

std::string& last_error_ref();

inline int fail(const std::string& msg) {
    last_error_ref() = msg;
    return 1;
}

#define OA_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return ::oa::fail(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + \
                              ":" + std::to_string(__LINE__) + ")");                              \
    } while (0)

#define OA_REQUIRE(cond, msg)                         \
    do {                                              \
        if (!(cond)) return ::oa::fail(std::string(msg)); \
    } while (0)

#define OA_LAUNCH_CHECK() OA_HIP(hipGetLastError())

template <typename T, int N>
struct alignas(sizeof(T) * N > 16 ? 16 : sizeof(T) * N) Arr {
    T v[N];
};

// Request to fold the radial histogram of |kappa|^2 and the moment update (n += maps, S += b, C += b b^T, b = sums / mode
// counts) into the single-pass divergence launch and the one-workgroup fold launched behind it (fft_divbin.hpp).  Filled by pipeline.hip, honoured by HipLauncher::col_div_sp
// when the geometry runs that kernel (`done` set); otherwise the caller runs bin_power_moments as before.  Device pointers.
struct DivBinFuse {
    const int32_t* ids; long ipitch;      // radial ids of the full-resolution half plane, row pitch
    const int32_t* ids_t;                 // tile-major copy on the coarse grid of the single-pass divergence launch, or nullptr
    const void* fn_t;                     // ... and of Fnorm (handed to ColDivArgs::Fn_t by the launcher)
    int tab_logc, tab_rows;               // tile shape the two copies were made for: log2 columns per tile, coarse rows
    // run table of the same tile shape (divbin_runs.hpp), or run_ent == nullptr: this binding has none.  It was made for a band of
    // run_w columns and run_rb rows (ColDivArgs::width / rband) and holds at most run_cap entries per tile
    const unsigned long long* run_ent; const int32_t* run_off;
    int run_w, run_rb, run_cap;
    double pnorm; int nids, nxh;
    double* part;                         // [maps][workgroups][nids] partial sums (capacity part_cap doubles)
    long part_cap;
    double* sums;                         // [maps][nids]
    const int64_t* mcounts; int64_t* n; double* S; double* C;
    int store;                            // != 0: kappa is also written to `out`
    int gx;                               // (set by the launcher) workgroups per map
    bool done;                            // (set by the launcher)
};

inline int flat_grid(long units, int block = 256, int cap = 8192) {
    long g = (units + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

}  // namespace oa

struct oa_plan {
    int ny, nx, logNy, logNx, dtype, device;
    long kp;
    void* tw_x;      // cx<T>[nx]
    void* tw_y;      // cx<T>[ny]
    void* scratch;   // FFT scratch plane(s)
    size_t scratch_bytes;
    void* ly;        // T[ny]
    void* lx;        // T[nx]
    void* lyd;       // T[ny]  derivative axis: Nyquist entry zeroed
    void* lxd;       // T[nx]
    double* ly64;    // double[ny]
    double* lx64;    // double[nx]
    bool have_laxes;
    // sides that are not powers of two: chirp-z (Bluestein) state, see czt.hip.  pow2 == false then.
    bool pow2;
    oa_plan* inner;            // (My, Mx) power-of-two plan
    int My, Mx;
    void* chirp_y; void* chirp_x;            // cx<T>[ny], cx<T>[nx]
    void* cz_bhat; void* cz_a; void* cz_f;   // cx<T>[My*Mx]: chirp-kernel transform, two work planes
    void* cz_full;                           // cx<T>[ny*nx]
    bool mixed;                              // sides 2^a 3^b 5^c: mixed-radix transforms (mixed.hip) instead of the chirp-z path
    void* mr_twx; void* mr_twxh; void* mr_twy;   // cx<T>[nx + 1], [nx / 2], [ny]
    void* pipe;                              // oa::Pipeline* (pipeline.hip): filters, bins, work planes of the one-call entries
    void* rq8c[5];                           // per-thread constants of the fused row stage's grids of 1024, 1536, 2048, 4096, 8192 points (fft_rowqe8.hpp: RQ8_NGRIDS)
    void* tw_y_small[16];                    // COLUMN GRID: cx<T>[my] = W_my^k for my = 2^i (made on first use, kept: estimators
                                             // with different row bands may alternate on one plan)
    void* tw_y_m3[16];                       // ... and for the 3 x 2^i grids of the from-map R-split path (slot i)
};

namespace oa {
int plan_ensure_scratch(oa_plan* p, size_t bytes);
int czt_setup(oa_plan* p);
void czt_release(oa_plan* p);
int czt_c2c(oa_plan* p, const void* in, void* out, int inverse, double scale, hipStream_t st);
int czt_r2c(oa_plan* p, const void* real_in, void* hc_out, double scale, hipStream_t st);
int czt_c2r(oa_plan* p, const void* hc_in, void* real_out, double scale, hipStream_t st);
bool mixed_sides_ok(int ny, int nx);
int mixed_setup(oa_plan* p);
void mixed_release(oa_plan* p);
int mixed_c2c(oa_plan* p, const void* in, void* out, int inverse, double scale, hipStream_t st);
int mixed_r2c(oa_plan* p, const void* real_in, void* hc_out, double scale, hipStream_t st);
int mixed_c2r(oa_plan* p, const void* hc_in, void* real_out, double scale, hipStream_t st);
int mixed_c2r_windowed(oa_plan* p, const void* hc_in, void* real_out, double scale, const void* window, hipStream_t st);
int mixed_cols_inverse(oa_plan* p, const void* hc_in, void* hc_out, hipStream_t st);      // unscaled, nx / 2 + 1 columns; in place allowed
int mixed_lens_derivs(oa_plan* p, int nmaps, const void* real_in, long in_stride, void* k0, void* hc_pool, void* real_pool, int nd, hipStream_t st,
                      const void* hc_in, long hc_stride, double hc_scale);
void pipeline_release(oa_plan* p);
// oa_n1_tt (n1.hip): its plan-owned pool (pipeline.hip: grown on demand, oa_plan_release_pools frees it)
int n1_pool_reserve(oa_plan* p, size_t bytes, char** out);
// fused estimator passes on the plan's compact work planes (fft.hip)
long work_pitch(const oa_plan* p, int w);
int bin_power_moments(int dtype, const void* k, double norm, const int32_t* ids, long n, int nids, long hp, int nxh, double* sums,
                      int64_t* counts, void* scratch, int active_cols, int active_rows, unsigned* ticket,
                      const int64_t* mcounts, int64_t* mn, double* S, double* C, hipStream_t st, int nbatch = 1, long kstride = 0);
int stack_add_region(int dtype, const void* x, double* acc, int ny, long kp, int w, int rb, hipStream_t st, int nbatch = 1, long xstride = 0);
// oa_mc_run_mv_windowed (mc_pol.hpp, elementwise.hip; rng.hip): Q, U -> E, B in place on the leg band of two hc planes by the caller's
// (ny, kp) cos / sin planes; the nest kappa_hat planes of an estimator set (kstride complex elements apart) added into nest float64 stacks
// and -- acc_mv -- their weighted sum into one more, over kappa's band; the full-plane T, E, B draw rotated to T, Q, U in the same pass
int band_rot2(int dtype, const void* c, const void* s, void* q, void* u, int ny, long kp, int w, int rb, hipStream_t st);
int stack_add_region_multi(int dtype, const void* k, long kstride, const void* wt, long wstride, int nest, double* const* acc, double* acc_mv,
                           int ny, long kp, int w, int rb, hipStream_t st);
int grf_mix_teb_to_tqu(oa_plan* p, uint64_t seed, uint64_t sid0, const void* const* cs, const void* rot_c, const void* rot_s, void* const* out,
                       hipStream_t st);
// ... on a band grid: k and wt are inner-layout planes (iny rows, ipitch elements per row), the stacks N-grid planes (any rows, apitch
// complex per row); band: columns < w, rows |ky| < r
int band_stack_add_multi(int dtype, const void* k, long kstride, const void* wt, long wstride, int nest, double* const* acc, double* acc_mv,
                         int iny, long ipitch, int any, long apitch, int w, int r, hipStream_t st);
// oa_mc_run_rdn0's combine -> bin -> moments tail over the 2 B kappa_hat planes of a batch (elementwise.hip, rdn0.hpp): two launches
size_t rdn0_part_bytes(int ny, int rb, int nids, int B);
int rdn0_tail_check(const char* who, int nids, int B);
int rdn0_tail(int dtype, const void* k, long kstride, int B, int ny, long kp, int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb,
              const int64_t* mcounts, double* part, int64_t* n, double* S, double* C, hipStream_t st);
// oa_mc_run_rdn0_mv's tail over the 2 nest kappa_hat planes of one realisation of an estimator set (elementwise.hip, rdn0_mv.hpp): three launches
size_t rdn0mv_scratch_bytes(int ny, int rb, int nspec, int nids);
int rdn0mv_tail_check(const char* who, int nest, bool have_w, int nspec, const int* host_a, const int* host_b, int nids);
int rdn0mv_tail(int dtype, const void* k, long kstride, const void* wt, long wstride, int nest, int nspec, const int* host_a, const int* host_b, int ny,
                long kp, int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb, const int64_t* mcounts, void* scratch, int64_t* n, double* S,
                double* C, hipStream_t st);
// the unscaled inverse column transform of nplanes hc planes pstride complex elements apart, in place, ONE launch (grid y = plane)
int mixed_cols_inverse_batch(oa_plan* p, int nplanes, void* hc, long pstride, hipStream_t st);
// my > 0: COLUMN GRID -- legs, row stage and divergence run on my < ny rows (plan_ensure_col_grid(p, my) first)
int plan_ensure_col_grid(oa_plan* p, int my);
// lr > 0 (qe_rsplit_lr): R-SPLIT path -- row R2C with the first radix-R column butterfly, then one single-pass column kernel;
// the leg planes are then in the R-LAYOUT and qe_rows_w must be told so (same lr)
int qe_rsplit_lr(const oa_plan* p, int my, int width, int wout, int mrow);
// fgh (lr > 0 only): the packed (FG, FH) table of this binding made by qe_fband_pack_w (qe_fband_table_entries complex entries), or
// nullptr: the column kernel reads the filter planes
int qe_map_legs_cols_w(oa_plan* p, const void* map, const void* FG, const void* FH, void* gx, void* gy, void* h, int width,
                       int rband, long pl, hipStream_t st, int stages = 7, int my = 0, int lr = 0, const void* fgh = nullptr);
long qe_fband_table_entries(const oa_plan* p, int width, int my);
int qe_fband_pack_w(oa_plan* p, const void* FG, const void* FH, void* out, int width, int rband, int my, hipStream_t st);
int qe_legs_cols_w(oa_plan* p, const void* kX, const void* kY, const void* FG, const void* FH, void* gx, void* gy, void* h,
                   int width, int rband, long pl, hipStream_t st, int my = 0);
// flat-sky Taylor lensing, FFT part: R2C of nmaps maps, then all nmaps * nd derivative fields inverse-transformed in three launches
// tile-major copy of a full-pitch real / int32 hc-layout plane on the coarse grid of `rows` rows: dst[(tile * rows + k) * C + c] =
// src[(k + (k >= rows / 2 ? ny - rows : 0)) * kp + tile * C + c], zero beyond `width` columns (elem_bytes 4 or 8)
int pack_tiles(const oa_plan* p, const void* src, void* dst, int rows, int logc, int width, int elem_bytes, hipStream_t st);
int div_tile_logc(const oa_plan* p, int rows);          // log2 columns per tile of the single-pass divergence launch on `rows` coarse rows
int qe_lens_derivs_w(oa_plan* p, int nmaps, const void* real_in, long in_stride, void* k0, void* hc_pool, void* real_pool, int nd, hipStream_t st,
                     const void* hc_in = nullptr, long hc_stride = 0, double hc_scale = 1.0);
// windowed simulation front end: hc spectrum -> inverse columns -> fused C2R x window -> R2C rows onto the plan's scratch plane
// (then qe_map_legs_cols_w with stages = 6, lr = 0)
// nz > 0: that many spectra per launch (one batched inverse column launch, one row launch with grid y = plane; the window is shared):
// plane z of hc_in and of cols_tmp sits z * in_moff, its row-transformed plane z * out_moff complex elements behind the first
int qe_windowed_rows_w(oa_plan* p, const void* hc_in, void* cols_tmp, const void* window, int width, long pl, double scale, hipStream_t st,
                       void* out = nullptr, int nz = 0, long in_moff = 0, long out_moff = 0);
int qe_win_rows_w(oa_plan* p, const void* cols_in, const void* window, int width, long pl, double scale, hipStream_t st, void* out, int nz,
                  long in_moff, long out_moff);
int qe_fwd_cols_batch_w(oa_plan* p, const void* in, long pin, void* out, int B, long in_moff, long out_moff, int width, int rband, hipStream_t st);
// one filtered field (subset 1: H plane into a; 2: gradient pair into a, b), inverse pass 1 only; then pass 2 over a pool of planes
int qe_legs_subset_w(oa_plan* p, const void* src, const void* F, void* a, void* b, int subset, int width, int rband, long pl,
                     hipStream_t st, int my = 0);
// divergence of nmaps estimators in one launch: product planes (A_e, B_e adjacent: B_e = A_e + in_moff / 2) in_moff apart, Fn planes
// fn_moff apart, outputs out_moff apart (offsets in elements of the respective plane type); tmp: 2 nmaps compact planes
int qe_cols_div_batch_w(oa_plan* p, const void* pa, const void* pb, const void* Fn, void* out, void* tmp, int nmaps, long in_moff,
                        long fn_moff, long out_moff, int width, int rband, long pk, hipStream_t st, int my = 0, DivBinFuse* fuse = nullptr);
int sum_region(int dtype, const void* parts, long part_stride, int nparts, void* out, int accumulate, int ny, long kp, int w, int rb,
               hipStream_t st);
// all leg planes of several estimators in one inverse pass-1 launch (ColLegsArgs::batch); offsets in complex elements
int qe_legs_batch_w(oa_plan* p, const void* src0, long off1, long off2, unsigned long long srcsel, const void* const* ftab,
                    int ngrad, int nh, void* pool, long ostride, int width, int rband, long pl, hipStream_t st, int my = 0, int selbits = 2,
                    int* finished = nullptr);      // *finished = 1: single pass (col_legs_sp), the planes need no inverse pass 2
// row stage of nmaps maps in one launch; -1: this geometry's row stage is not the two-rows-per-transform kernel
int qe_rows_batch_w(oa_plan* p, const void* gx, const void* gy, const void* h, void* px, void* py, double scale, int win, int wout, int mrow,
                    long pl, long pk, hipStream_t st, int my, int nmaps, long in_moff, long h_moff, long out_moff);
int qe_rows_table_w(oa_plan* p, int n, const void* const* gx, const void* const* gy, const void* const* h, void* const* px, void* const* py,
                    const double* scales, void* dev_tab, int upload, int accumulate, int win, int wout, int mrow, long pl, long pk, hipStream_t st,
                    int my);
size_t qe_rows_table_entry_bytes(const oa_plan* p);
int qe_rows_chain_w(oa_plan* p, int nest, int total, const void* const* gx, const void* const* gy, const void* const* h, void* const* px,
                    void* const* py, const double* scales, const int* first, const int* count, void* dev_tab, int upload, int win, int wout, int mrow,
                    long pl, long pk, hipStream_t st, int my);
// nreal full-plane draws (streams stream_id ...) straight into their inverse column transform: oa_grf_hc_icols without its checks (fft.hip)
int grf_icols_w(oa_plan* p, uint64_t seed, uint64_t stream_id, int nreal, const void* cs, void* out, long zstride, hipStream_t st);
// ntriples mixed T, Q, U draws (streams sid0 + 3 t + k) straight into their inverse column transform: oa_grf_mix_icols without its checks
int grf_mix_icols_w(oa_plan* p, uint64_t seed, uint64_t sid0, int ntriples, const void* const* cs, const void* rc, const void* rs, void* out,
                    long zstride, hipStream_t st);
// the plans its kernel exists for: power of two, and not float64 with a pass-1 sub-length of 256 (ny >= 32768: fft.hip, col_mix)
inline bool grf_mix_icols_serves(const oa_plan* p) { return p->pow2 && !(p->dtype != OA_F32 && p->logNy >= 15); }
bool qe_rows_chain_ok(const oa_plan* p, int win, int wout, int mrow, int my);
int grf_hc_band_batch(oa_plan* p, uint64_t seed, uint64_t stream_id, int nreal, const void* covsqrt_hc, void* hc_out, long zstride,
                      int width, int rband, hipStream_t stream);
// oa_mc_run_mv: the interior bins of nspec binned spectra (oa_bin_power_multi's layout) over the mode counts -> n += 1, S += x, C += x x^T (rng.hip);
// the argument checks of oa_bin_power_multi without its launches (bin.hip): 0, or the failure already reported
int moments_add_binned_multi(const double* sums, const int64_t* counts, int nspec, int nids, int64_t* n, double* S, double* C, hipStream_t st);
int bin_power_multi_check(const char* who, int dtype, int nfields, bool have_w, int nspec, const int* host_a, const int* host_b, int nids);
int qe_legs_pass2_w(oa_plan* p, void* pool, int nplanes, long stride, int width, long pl, hipStream_t st, int my = 0);
int qe_rows_w(oa_plan* p, const void* gx, const void* gy, const void* h, void* px, void* py, double scale, int accumulate,
              int win, int wout, int mrow, long pl, long pk, hipStream_t st, int my = 0, int lr = 0);
int qe_cols_div_w(oa_plan* p, const void* pa, const void* pb, const void* Fn, void* out, int accumulate, int width, int rband,
                  long pk, hipStream_t st, int my = 0, DivBinFuse* fuse = nullptr);
// two maps at once (fft.hip); -1 = not available for this geometry
int qe_tt_pair_w(oa_plan* p, const void* map0, const void* map1, const void* FG, const void* FH, const void* Fn, void* c0, void* c1,
                 void* c2, void* g0, void* g1, void* out0, void* out1, int wl, int wk, int rl, int rk, int mrow, int my, long pl, long pk,
                 hipStream_t st, DivBinFuse* fuse = nullptr, const void* fgh = nullptr);
// BAND GRID of the one-call TT entries on map sides 2^a 3^b 5^c (band.hip, pipeline.hip): N-grid <-> inner power-of-two grid
// rowbuf: band_map_scratch_bytes(p, wl, rl) bytes (row pass + the column pass's per-segment partial sums)
int band_map_r2c(oa_plan* p, const void* map, void* rowbuf, int wl, int rl, void* dst, int dny, long dkp, hipStream_t st);
size_t band_map_scratch_bytes(const oa_plan* p, int wl, int rl);
// the same for the nmaps <= 6 real maps of oa_qe_mv_maps in three launches (map pointers by value), into inner planes dstride elements apart,
// with the Q,U -> E,B rotation of the pairs (1, 2) / (4, 5) by the band of the N-grid planes rot_c / rot_s (both or neither)
int band_maps_r2c(oa_plan* p, int nmaps, const void* const* maps, const void* rot_c, const void* rot_s, void* scratch, int wl, int rl, void* dst,
                  long dstride, int dny, long dkp, hipStream_t st);
size_t band_maps_scratch_bytes(const oa_plan* p, int nmaps, int wl, int rl);
// FRONT END of oa_mc_run_windowed on these sides: B <= 6 inverse-column-transformed spectra (N-grid hc planes in_bstride elements apart)
// -> fused C2R x window x scale -> R2C rows (the real map in LDS only) -> pruned column DFT onto B inner planes dstride elements apart.
// single = 0: the batched kernels, scratch of band_maps_scratch_bytes(p, B, wl, rl); single != 0 (B = 1): band_map_r2c's column
// kernels, scratch of band_map_scratch_bytes(p, wl, rl).  rot_c / rot_s (both or neither; batched, B = 3 or 6): the planes are T, Q, U
// and the fold rotates the pairs (1, 2) / (4, 5) Q, U -> E, B as band_maps_r2c does (oa_mc_run_mv_windowed)
int band_win_r2c(oa_plan* p, int B, const void* hc_in, long in_bstride, const void* window, double scale, void* scratch, int single, int wl, int rl,
                 const void* rot_c, const void* rot_s, void* dst, long dstride, int dny, long dkp, hipStream_t st);
bool band_rows_win_ok(const oa_plan* p);                 // the fused windowed row kernel holds a row of this plan (nx <= 8192)
int band_copy(int kind, const void* src, long spitch, int sny, void* dst, long dpitch, int dny, int w, int r, double scale, hipStream_t st);
int band_zero_outside(int dtype, void* out, int ny, long kp, int w, int r, hipStream_t st);
int band_stack_add(int dtype, const void* src, long spitch, int sny, int nbatch, long sstride, double* acc, long apitch, int any, int w, int r,
                   hipStream_t st);
// oa_qe_pol / oa_qe_mv on the band grid: n source planes through a device table -> inner planes (one launch); kappa's band back
// (mode 0 overwrite, 1 accumulate, 2 overwrite + zero-fill of the complement in the same launch)
int band_embed(int dtype, const void* const* dev_srcs, int n, long spitch, int sny, void* dst, long dstride, long dpitch, int dny, int w, int r,
               hipStream_t st);
int band_scatter(int dtype, const void* src, long spitch, int sny, void* out, long okp, int ony, int w, int r, int mode, hipStream_t st);
// oa_qe_tt_splits / oa_qe_tt_split_power on the band grid: nplanes inner kappa planes sstride elements apart -> the N-grid planes of a
// device table, one launch (zero: + the zero-fill of each destination's complement); the 4-point combination of n^2 such planes per mode
// -> the real N-grid half-plane (okp reals per row)
int band_scatter_batch(int dtype, const void* src, long sstride, int nplanes, long spitch, int sny, void* const* dev_outs, long okp, int ony, int w,
                       int r, int zero, hipStream_t st);
int band_split_power(int dtype, int nsplits, const void* src, long sstride, long spitch, int sny, void* out_real, long okp, int ony, int w, int r,
                     double norm, int zero, hipStream_t st);
// the leg band of oa_grf_hc's N-grid draw (same Philox counters) into the hc layout of an (my, okp) grid, nreal planes zstride elements apart
int grf_band_inner(oa_plan* p, uint64_t seed, uint64_t stream_id, int nreal, const void* covsqrt_hc, void* out, int my, long okp, long zstride,
                   int width, int rband, hipStream_t stream);
}
#define OA_NEED_POW2(p, what) \
    OA_REQUIRE((p)->pow2, what ": needs power-of-two map sides (other sizes: oa_fft_r2c / oa_fft_c2r / oa_fft_c2c and the modular oa_qe_legs / oa_mul_real / oa_qe_div calls)")
