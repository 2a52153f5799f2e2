// One-call entry points of the C-ABI: a plan that knows its estimator filters and its
// radial bins runs a whole reconstruction -- or a whole Monte-Carlo shard -- per call, stream-ordered, without the
// host touching intermediate planes.  They are thin sequencers over the fused passes of fft.hip / bin.hip /
// rng.hip (the same kernels the fine-grained calls launch), plus an RCCL all-reduce for hosts that do not bring
// torch.distributed (librccl is dlopen'ed on first use, so the library has no link-time dependency on it).
#include <dlfcn.h>
#include <cstdlib>
#include <algorithm>
#include <functional>
#include <string>
#include <utility>
#include <vector>
#include "common.hpp"
#include "fft_plan.hpp"
#include "divbin_runs.hpp"

namespace oa {

constexpr int MC_BATCH_MAX = 6;      // realisations per launch in oa_mc_run (kappa planes: the six plan-owned work planes in front of kk)

// A grow-only device buffer.  reserve() on a buffer that is already large enough does NOTHING -- no HIP call: the steady-state one-call
// entries stay free of allocation and synchronisation.  Otherwise it synchronises the device before it frees a live allocation (launches
// in flight may still use it), allocates, and zero-fills when asked.  A plain value: nothing is freed implicitly, pipeline_release is
// where a plan's device memory is returned.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int reserve(size_t need, bool zero = false) {
        if (bytes >= need) return 0;
        if (p) { OA_HIP(hipDeviceSynchronize()); release(); }
        OA_HIP(hipMalloc(&p, need));
        bytes = need;
        if (zero) OA_HIP(hipMemset(p, 0, need));
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    char* at(size_t off = 0) const { return (char*)p + off; }
};

struct Pipeline {
    // filters (caller-owned device planes) + active region of the TT estimator
    const void* FG = nullptr; const void* FH = nullptr; const void* Fn = nullptr;
    int wl = 0, wk = 0, rl = 0, rk = 0, mrow = -1;
    int mcol = -1;   // requested column grid (-1 auto, 0 = the map's own ny rows, > 0 explicit)
    int my = 0;      // resolved: rows the legs / row stage / divergence run on (0 = ny)
    int my3 = 0;     // FROM-MAP GRID: 3 my / 4 when the from-map R-split path runs its coarse side there (include/orphics_amd.h), else 0 = my
    int map_grid() const { return my3 ? my3 : my; }
    // plan-owned work planes (hc): legs x3, products x2, input transform, kappa
    void* work = nullptr;
    void* c[3] = {nullptr, nullptr, nullptr};
    void* g[2] = {nullptr, nullptr};
    void* kT = nullptr;
    void* kk = nullptr;
    // bins
    const int32_t* ids = nullptr;
    int nids = 0;
    double norm = 1.0;
    void* bin_scratch = nullptr;
    double* sums = nullptr;
    int64_t* counts_full = nullptr;   // data-independent mode counts over the whole plane
    int64_t* counts_tmp = nullptr;
    unsigned* ticket = nullptr;       // last-workgroup ticket of the fused bin + moments launch (bin.hip, BinTail)
    DevBuf split_legs;                // oa_qe_tt_splits / oa_qe_mv: pool of compact leg planes (grown on demand)
    void* mv_rtab = nullptr;          // oa_qe_mv: device table of per-piece row-stage operands (RowQeMap), 64 entries
    std::vector<unsigned long long> mv_rkey;
    DevBuf mc_src;                    // oa_mc_run: MC_BATCH_MAX hc planes, a batch of realisations
    DevBuf lens_pool;                 // oa_lens_maps: transforms + derivative planes (hc and real) of the maps of one call
    DevBuf mvmc;                      // oa_mc_run_mv: the three drawn hc planes | per-estimator kappa planes (only when the one-launch divergence
                                      // is not engaged) | oa_bin_power_multi's partials | its sums
    DevBuf mvwin;                     // oa_mc_run_mv_windowed: the three full-plane T, Q, U draws | one column temporary per plane (the real maps of
                                      // the unfused flow) | the three compact row-transformed planes; oa_mc_run_rdn0_mv_windowed's fused-draw
                                      // arm: six full planes (T, Q, U of s, then of s') | six compact row-transformed planes
    // oa_rdn0_set_data / oa_mc_run_rdn0.  On a band grid the two buffers are the inner plan's, the key is the map's plan's
    DevBuf rdn0_legs;                 // the data map's three compact leg planes gx, gy, h, as the leg stage of oa_qe_tt(kX = d) leaves them
    DevBuf rdn0_pool;                 // 2 MC_BATCH_MAX drawn hc planes | 2 MC_BATCH_MAX kappa planes | the partial sums of the tail (rdn0.hpp)
    unsigned long rdn0_gen = 0;       // bind_gen the data legs were made under (0: no data set) ...
    int rdn0_my = 0;                  // ... and the column grid
    int rdn0_ran_batched = 0;         // whether the last oa_mc_run_rdn0 / oa_mc_run_rdn0_windowed call ran a batch to its tail (oa_plan_rdn0_batched)
    // oa_rdn0_set_data_mv / oa_mc_run_rdn0_mv (the estimator set comes with every call, so the key is its description)
    DevBuf rdn0mv_legs;               // the data triple's distinct leg planes in Rdn0MvSlots' numbering
    DevBuf rdn0mv_pool;               // the 6 drawn hc planes (T, E, B of s, then of s') | the 2 nest kappa planes (A_e, then B_e) | the tail's scratch
    DevBuf n1_pool;                   // oa_n1_tt (n1.hip): the box-ordered mode table and G of one L | the (tile, part) partial sums
    std::vector<const void*> rdn0mv_key;   // Rdn0MvSlots::key() the data legs were made for (empty: no data set) ...
    int rdn0mv_band[5] = {0, 0, 0, 0, 0};  // ... their leg_cols, kappa_cols, leg_rows, kappa_rows, mrow ...
    int rdn0mv_my = 0;                     // ... and their column grid
    // on a band grid (oa_qe_band_bind + oa_mc_mv_band_bind first) the two buffers are those of the inner plan of the binding, the key, the
    // bands and the (inner) column grid are kept here, on the map's plan, with ...
    unsigned long rdn0mv_gen = 0;          // ... PolBind::gen of the binding the data legs were made on
    // tile-major copies of Fnorm and of the bin ids on the coarse grid of the fused divergence + binning launch (what they were
    // made from: rebuilt when the filters / bins / column grid change)
    // (one set per grid a plan can carry: [0] the column grid `my`, [1] the from-map grid `my3`)
    struct DivTabs {
        DevBuf fn_t, ids_t;
        unsigned long tab_gen = 0;
        int tab_rows = 0, tab_logc = 0, tab_wk = 0;
        // the run table of the ids (divbin_runs.hpp) on the same tiles, for kappa's band as the divergence launch clamps it
        DevBuf run_ent, run_off;
        bool has_runs = false;
        int run_w = 0, run_rb = 0, run_cap = 0;
    } dt[2];
    DivTabs& tabs_of(int rows) { return (my3 && rows == my3) ? dt[1] : dt[0]; }
    const DivTabs& tabs_of(int rows) const { return (my3 && rows == my3) ? dt[1] : dt[0]; }
    // keyed on a GENERATION bumped by every oa_plan_set_filters / oa_plan_set_bins call, not on the planes' addresses: a caching
    // allocator hands a new estimator the addresses of a freed one, and a caller may refill Fnorm or the ids in place
    unsigned long bind_gen = 1;
    // the packed (FG, FH) table of the R-split column stage (ColFBandArgs::fgh), same generation key
    DevBuf fb_t;
    unsigned long fb_gen = 0;
    int fb_my = 0, fb_wl = 0, fb_rl = 0;
    void** mv_ftab = nullptr;         // oa_qe_mv: device table of the distinct filter planes (gradient fields, then H fields)
    std::vector<const void*> mv_fkey; // what the table holds
    // oa_plan_set_option (include/orphics_amd.h): which of the equivalent launch sequences the one-call entries run
    int opt_mc_batch = MC_BATCH_MAX;  // realisations per launch in oa_mc_run
    bool opt_mv_batch = true;         // oa_qe_mv / oa_qe_tt_splits: all leg planes / all divergences in one launch each
    bool opt_mv_rowbatch = true;      // oa_qe_mv: the row stage of several pieces per launch
    bool opt_mv_chain = true;         // oa_qe_mv: estimator chains (pieces summed in real space inside one row-stage launch)
    bool opt_divbin = true;           // moment entries: radial binning + moments in the tail of the single-pass divergence launch
    bool opt_win_fused = true;        // oa_mc_run_windowed: C2R x window -> R2C as one row pass (the real map stays in LDS)
    bool opt_win_fused_set = false;   // ... set by the caller (until then a band-grid plan picks by row length: mixed_mc_run_windowed)
    int opt_draw_fused = -1;          // oa_mc_run_rdn0_windowed (power-of-two plans): the draws inside inverse column pass 1 (1), oa_grf_hc and
                                      // the column transform (0), or the measured default (< 0: DRAW_FUSED_DEFAULT)
    // BAND GRID (map sides 2^a 3^b 5^c, p->mixed; include/orphics_amd.h): the one-call TT entries run on an inner power-of-two plan of
    // (bmy, bmx) points that holds inner-layout copies of the filters and bin ids; made by oa_plan_set_filters / oa_plan_set_col_grid
    oa_plan* band = nullptr;
    int bmy = 0, bmx = 0;
    DevBuf bplanes;                   // inner layout: FG, FH, Fnorm (real planes), then the two input-transform planes kX, kY (hc)
    DevBuf bids;                      // inner-layout bin ids (int32, -1 outside kappa's band)
    DevBuf brows;                     // band input transform: row pass (ny x leg_cols complex) + column-pass partial sums
    // ... oa_mc_run_windowed there: MC_BATCH_MAX N-grid hc planes (the full-plane draws, inverse-column-transformed in place; plane 1
    // holds the real map of the unfused flow) | the row planes and column partial sums of a batch (band_maps_scratch_bytes); taken on
    // the first windowed call, regrown when the band widens
    DevBuf bwin;
    // ... oa_qe_tt_splits / oa_qe_tt_split_power there: bs_cap inner source planes (hc, zero outside the leg band) | the evenly spaced
    // (n, n, My, kp_inner) block of the inner kappa planes; allocated on first use, grown when a call brings more splits
    DevBuf bsplit;
    int bs_cap = 0;
    DevBuf bs_tab;                    // device table (void*): the n N-grid source planes, then the n^2 N-grid output planes of the batched scatter
    std::vector<const void*> bs_key;  // what it holds
    // ... and oa_qe_pol / oa_qe_mv there: a PRIVATE inner plan (their bands differ from the TT binding's: kmask_P, the widest band of
    // an estimator set) with inner-layout copies of the planes handed to oa_qe_band_bind, looked up by their N-grid address
    struct PolBind {
        bool bound = false;
        unsigned long gen = 0;                 // bumped by every oa_qe_band_bind call: it rewrites the inner filter copies and may remake the
                                               // inner plan, so whatever was made from them (the data legs of oa_rdn0_set_data_mv) is stale
        oa_plan* plan = nullptr;
        int my = 0, mx = 0;
        int wl = 0, wk = 0, rl = 0, rk = 0, mrow = -1;
        std::vector<const void*> fkey, nkey;   // the bound N-grid filter / normalisation planes; inner plane i belongs to key i
        DevBuf planes;                         // inner layout: nf filter planes | nn normalisation planes, stacked in the bound order |
                                               //               POL_SRC_MAX source planes (hc)
        DevBuf stab;                           // device table (void*) of the N-grid source planes of the batched embed
        std::vector<const void*> skey;         // what it holds
        DevBuf mrows;                          // oa_qe_mv_maps: row planes + column partial sums of the batched band input transform
                                               // (band_maps_scratch_bytes; taken on the first from-maps call, grown on demand)
        DevBuf mwin;                           // oa_mc_run_mv_windowed: the three N-grid hc planes of a realisation's T, Q, U draw | three planes
                                               // for the real maps of the unfused flow | band_maps_scratch_bytes(p, 3, wl, rl) (first windowed call)
        // oa_mc_run_mv on this binding (oa_mc_mv_band_bind; dropped by the next oa_qe_band_bind): what the caller's shard calls must
        // bring again (the key), and one pool in the inner layout: nest weight planes (real; none without weights) | bin ids (-1 outside
        // kappa's band) | the three drawn hc planes (zero outside the leg band) | nest kappa planes (for when the one-launch divergence
        // is not engaged) | oa_bin_power_multi's partials | its sums
        struct McBind {
            bool bound = false;
            const void* w = nullptr; long wstride = 0;
            const int32_t* ids = nullptr;
            int nids = 0, nest = 0, nspec_max = 0;
            DevBuf pool;
            size_t off_ids = 0, off_draw = 0, off_kappa = 0, off_scratch = 0, off_sums = 0;
        } mc;
    } pb;
    // what is sized by the band plan's planes: returned when the band grid changes (mixed_bind) and with the plan
    void release_band() { for (DevBuf* b : {&bplanes, &bids, &bsplit, &bwin}) b->release(); bs_cap = 0; }
};
constexpr int POL_SRC_MAX = 6;                 // T, E, B and the Y-leg sources of a split call

static size_t elem_bytes(const oa_plan* p) { return 2 * (size_t)(p->dtype == OA_F32 ? 4 : 8); }       // one complex element
static size_t plane_bytes(const oa_plan* p) { return (size_t)p->ny * p->kp * elem_bytes(p); }
static long plane_elems(const oa_plan* p) { return (long)p->ny * p->kp; }                               // complex elements per hc plane

static Pipeline* pipe_of(oa_plan* p) {
    if (!p->pipe) p->pipe = new Pipeline();
    return (Pipeline*)p->pipe;
}

int n1_pool_reserve(oa_plan* p, size_t bytes, char** out) {
    Pipeline* q = pipe_of(p);
    if (int rc = q->n1_pool.reserve(bytes)) return rc;
    *out = q->n1_pool.at();
    return 0;
}

void pipeline_release(oa_plan* p) {
    if (!p || !p->pipe) return;
    Pipeline* q = (Pipeline*)p->pipe;
    if (q->work) (void)hipFree(q->work);
    if (q->bin_scratch) (void)hipFree(q->bin_scratch);
    if (q->sums) (void)hipFree(q->sums);
    if (q->counts_full) (void)hipFree(q->counts_full);
    if (q->counts_tmp) (void)hipFree(q->counts_tmp);
    if (q->ticket) (void)hipFree(q->ticket);
    if (q->mv_ftab) (void)hipFree(q->mv_ftab);
    if (q->mv_rtab) (void)hipFree(q->mv_rtab);
    for (DevBuf* b : {&q->split_legs, &q->mc_src, &q->lens_pool, &q->mvmc, &q->mvwin, &q->rdn0_legs, &q->rdn0_pool, &q->rdn0mv_legs, &q->rdn0mv_pool, &q->n1_pool, &q->dt[0].fn_t, &q->dt[0].ids_t,
                      &q->dt[1].fn_t, &q->dt[1].ids_t, &q->dt[0].run_ent, &q->dt[0].run_off, &q->dt[1].run_ent, &q->dt[1].run_off, &q->fb_t}) b->release();
    if (q->band) (void)oa_plan_destroy(q->band);
    q->release_band();
    q->brows.release();
    q->bs_tab.release();
    if (q->pb.plan) (void)oa_plan_destroy(q->pb.plan);
    for (DevBuf* b : {&q->pb.planes, &q->pb.stab, &q->pb.mrows, &q->pb.mwin, &q->pb.mc.pool}) b->release();
    delete q;
    p->pipe = nullptr;
}

static int ensure_work(oa_plan* p, Pipeline* q) {
    if (q->work) return 0;
    const size_t pb = plane_bytes(p);
    OA_HIP(hipMalloc(&q->work, 7 * pb));
    OA_HIP(hipMemset(q->work, 0, 7 * pb));          // kappa plane zero outside its active region from the start
    char* b = (char*)q->work;
    for (int i = 0; i < 3; ++i) q->c[i] = b + i * pb;
    for (int i = 0; i < 2; ++i) q->g[i] = b + (3 + i) * pb;
    q->kT = b + 5 * pb;
    q->kk = b + 6 * pb;
    return plan_ensure_scratch(p, 2 * pb);          // never reallocated inside a stream-ordered call afterwards
}

// pool of compact planes of the multi-map entries (grown on demand; growing synchronises the device once)
static int ensure_pool(Pipeline* q, size_t bytes) { return q->split_legs.reserve(bytes); }

// zero the part of a caller-supplied output plane that the pruned divergence kernel never writes: every 16-byte unit of
// the plane outside (columns < wk) x (band rows), in one streaming launch (two hipMemset2DAsync calls ran at 1.2 TB/s:
// 365 us per 8192^2 plane, a third of an MV reconstruction into a caller-owned plane)
__global__ __launch_bounds__(256) void zero_complement_kernel(uint4* __restrict__ out, int ny, int units_per_row, int wk_units,
                                                              int rk, int odd_col) {
    const int y = blockIdx.y;
    const bool band = (rk <= 0) || y < rk || y > ny - rk;      // rows that hold kappa's active columns
    const int x0 = band ? wk_units : 0;
    uint4* row = out + (size_t)y * units_per_row;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int x = x0 + blockIdx.x * blockDim.x + threadIdx.x; x < units_per_row; x += gridDim.x * blockDim.x) row[x] = z;
    // f32 planes with an odd number of active columns: column wk shares its 16-byte unit with the last active column
    if (band && odd_col >= 0 && blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<uint2*>(row)[odd_col] = make_uint2(0u, 0u);
}

static int zero_complement(oa_plan* p, void* out, int wk, int rk, hipStream_t st) {
    const size_t es = elem_bytes(p);
    const int per16 = (int)(16 / es);                           // complex elements per 16-byte unit (2 in f32, 1 in f64)
    if (!(wk > 0 && wk < p->kp)) wk = (int)p->kp;
    if (!(rk > 0 && 2L * rk - 1 < p->ny)) rk = 0;
    if (wk >= p->kp && rk == 0) return 0;
    const int units = (int)(p->kp / per16);                     // kp is a multiple of 16 elements
    const int wk_units = (wk + per16 - 1) / per16;              // first unit wholly outside the active columns
    const int odd_col = (wk < p->kp && wk % per16) ? wk : -1;
    hipLaunchKernelGGL(zero_complement_kernel, dim3(4, p->ny), dim3(256), 0, st, (uint4*)out, p->ny, units, wk_units, rk, odd_col);
    OA_LAUNCH_CHECK();
    return 0;
}

// COLUMN GRID.  Legs confined to rows |ky| < rl have real-space products confined to |ky| <= 2 (rl - 1); sampled on
// my >= 2 rl + rk rows no aliased product frequency reaches the kept kappa rows |ky| < rk (same argument as the row
// grid, include/orphics_amd.h), so the inverse column transforms, the row stage and the forward column transforms run
// on my instead of ny rows and return the same kappa_hat rows.
static int resolve_my(oa_plan* p, int mcol, int rl, int rk, int* my_out) {
    *my_out = 0;
    if (mcol == 0 || rl <= 0 || rk <= 0) return 0;
    if (mcol > 0 && is_m3(mcol)) mcol = m3_pow2(mcol);          // a 3 x 2^k request concerns the from-map path only (resolve_col_grid)
    const long need = std::max(2L * rl + rk, 2L * rk);
    int my = mcol;
    if (my < 0) { my = 64; while (my < need && my < p->ny) my <<= 1; }
    else if (my < need) return fail("column grid < max(2*leg_rows + kappa_rows, 2*kappa_rows) would alias the leg products into the kept rows");
    if (my >= p->ny) return 0;
    if (int rc = plan_ensure_col_grid(p, my)) return rc;
    *my_out = my;
    return 0;
}
// ... and the FROM-MAP GRID: three quarters of `my` when that many rows satisfy the same bound and this geometry's from-map path is the
// R = 4 R-split one with the 3 x 2^k kernels built (8192 rows -> 1536, 4096 rows -> 768); chosen automatically, or asked for by
// an explicit 3 x 2^k column grid, which is refused where it would alias or where no such path exists.  Every other entry (Fourier-space
// legs, pol, MV, Monte Carlo) keeps `my`.
static int resolve_col_grid(oa_plan* p, Pipeline* q) {
    q->my3 = 0;
    const bool want3 = q->mcol > 0 && is_m3(q->mcol);
    const long need = std::max(2L * q->rl + q->rk, 2L * q->rk);
    if (want3 && q->rl > 0 && q->rk > 0 && q->mcol < need)
        return fail("column grid < max(2*leg_rows + kappa_rows, 2*kappa_rows) would alias the leg products into the kept rows");
    if (int rc = resolve_my(p, q->mcol, q->rl, q->rk, &q->my)) return rc;
    const int my3 = want3 ? q->mcol : (q->mcol < 0 && q->my > 0 && q->my % 4 == 0 ? q->my / 4 * 3 : 0);
    bool ok = my3 > 0 && q->my == m3_pow2(my3) && my3 >= need && qe_rsplit_lr(p, q->my, q->wl, q->wk, q->mrow) == 2;
    if (ok) {
        if (int rc = plan_ensure_col_grid(p, my3)) return rc;
        ok = qe_rsplit_lr(p, my3, q->wl, q->wk, q->mrow) == 2;
    }
    if (ok) q->my3 = my3;
    else if (want3) return fail("oa_plan_set_col_grid: this geometry has no from-map path on a 3 x 2^k column grid (built for 8192-row maps on 1536 "
                                "rows and 4096-row maps on 768 rows, R-split from-map path)");
    return 0;
}

}  // namespace oa

using namespace oa;

static int ensure_div_tables(oa_plan* p, oa::Pipeline* q, hipStream_t st);
static int ensure_div_tables(oa_plan* p, oa::Pipeline* q, hipStream_t st, int rows);
// BAND GRID (map sides 2^a 3^b 5^c), defined below the Monte-Carlo helpers
namespace oa {
static int band_grid_rule(const oa_plan* p, int mrow, int mcol, int wl, int wk, int rl, int rk, int* my, int* mx);
static int mixed_bind(oa_plan* p, Pipeline* q);
static int mixed_bins(oa_plan* p, Pipeline* q, hipStream_t st);
static int mixed_qe_tt(oa_plan* p, Pipeline* q, const void* map, const void* kX, const void* kY, void* out, int zero_outside, hipStream_t st);
static int mixed_moments(oa_plan* p, Pipeline* q, const void* map, int64_t* n, double* S, double* C, hipStream_t st);
struct MvCall {            // the arguments of oa_qe_mv (oa_qe_pol: nest = 1 and pol set)
    int nest; const int* npieces; const double* signs; const void* const* FG; const void* const* FH; const int* swap;
    const void* const* kX; const void* const* kY; const void* const* Fn; bool pol;
    // oa_qe_mv_maps (nmaps > 0): the sources are real maps, the estimators name them by index; kX / kY are unused
    int nmaps; const void* const* maps; const void* rot_c; const void* rot_s; const int* xsrc; const int* ysrc;
};
static int mixed_qe_mv(oa_plan* p, Pipeline* q, const MvCall& c, void* out, int accumulate, int wl, int wk, int rl, int rk, int mrow, int zero_outside,
                       hipStream_t st);
static int mixed_qe_tt_splits(oa_plan* p, Pipeline* q, const char* who, int nsplits, const void* const* host_kmaps, void* const* host_out,
                              void* out_power, double norm, int zero_outside, hipStream_t st);
}  // namespace oa
#define OA_NOT_MIXED(p, what) \
    OA_REQUIRE(!(p)->mixed, what ": not available on map sides that are not powers of two (one-call TT entries there: oa_qe_tt, oa_qe_tt_moments(2), oa_mc_run)")

extern "C" {

int oa_plan_set_col_grid(oa_plan* p, int mcol) {
    OA_REQUIRE(p, "oa_plan_set_col_grid: NULL plan");
    OA_REQUIRE(p->pow2 || p->mixed, "oa_plan_set_col_grid: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path");
    OA_REQUIRE(mcol <= 0 || is_pow2(mcol) || (is_m3(mcol) && p->pow2),
               "oa_plan_set_col_grid: mcol must be -1 (auto), 0 (off), a power of two, or 3 x 2^k (from-map path of power-of-two plans)");
    Pipeline* q = pipe_of(p);
    q->mcol = mcol;
    if (p->mixed) {                                // the band grid's rows: re-resolved, the inner plan remade only if they change
        if (!q->FG) return 0;
        int my = 0, mx = 0;
        int rc = band_grid_rule(p, q->mrow, q->mcol, q->wl, q->wk, q->rl, q->rk, &my, &mx);
        if (!rc && q->band && my == q->bmy && mx == q->bmx) return 0;
        if (!rc) rc = mixed_bind(p, q);
        if (rc) q->FG = nullptr;                   // nothing is bound after a refused grid
        return rc;
    }
    return q->FG ? resolve_col_grid(p, q) : 0;     // oa_qe_pol resolves it per call from its own row bands
}

int oa_plan_col_grid(const oa_plan* p) { return (p && p->pipe) ? ((Pipeline*)p->pipe)->map_grid() : 0; }

int oa_plan_band_grid(const oa_plan* p, int* my, int* mx) {
    OA_REQUIRE(p && my && mx, "oa_plan_band_grid: NULL argument");
    const Pipeline* q = (const Pipeline*)p->pipe;
    const bool bound = q && q->FG && q->band;
    *my = bound ? q->bmy : 0;
    *mx = bound ? q->bmx : 0;
    return 0;
}

int oa_plan_set_option(oa_plan* p, int option, int value) {
    OA_REQUIRE(p, "oa_plan_set_option: NULL plan");
    Pipeline* q = pipe_of(p);
    switch (option) {
        case OA_OPT_MC_BATCH:
            OA_REQUIRE(value >= 0 && value <= MC_BATCH_MAX, "oa_plan_set_option: OA_OPT_MC_BATCH takes 0 (default) .. 6");
            q->opt_mc_batch = value ? value : MC_BATCH_MAX; return 0;
        case OA_OPT_MV_BATCH: q->opt_mv_batch = value != 0; return 0;
        case OA_OPT_MV_ROWBATCH: q->opt_mv_rowbatch = value != 0; return 0;
        case OA_OPT_MV_CHAIN: q->opt_mv_chain = value != 0; return 0;
        case OA_OPT_DIV_BIN: q->opt_divbin = value != 0; return 0;
        case OA_OPT_WIN_FUSED:                     // (< 0: back to the automatic choice of a band-grid plan; pow2 plans: the fused pass)
            q->opt_win_fused = value != 0; q->opt_win_fused_set = value >= 0; return 0;
        case OA_OPT_DRAW_FUSED: q->opt_draw_fused = value < 0 ? -1 : (value != 0); return 0;
        default: return fail("oa_plan_set_option: unknown option");
    }
}
}  // extern "C"
namespace oa {
// the band plan runs the one-call launches of a mixed plan: it follows the options set on the outer plan
static void band_options(Pipeline* q) {
    for (oa_plan* inner : {q->band, q->pb.plan}) {
        if (!inner || !inner->pipe) continue;
        Pipeline* b = (Pipeline*)inner->pipe;
        b->opt_mc_batch = q->opt_mc_batch; b->opt_mv_batch = q->opt_mv_batch; b->opt_mv_rowbatch = q->opt_mv_rowbatch;
        b->opt_mv_chain = q->opt_mv_chain; b->opt_divbin = q->opt_divbin; b->opt_win_fused = q->opt_win_fused;
    }
}
}  // namespace oa
extern "C" {
int oa_plan_rdn0_batched(const oa_plan* p) { return (p && p->pipe) ? ((const Pipeline*)p->pipe)->rdn0_ran_batched : 0; }
int oa_plan_rsplit(const oa_plan* p) {
    if (!p || !p->pipe) return 0;
    const Pipeline* q = (const Pipeline*)p->pipe;
    return q->FG ? (1 << qe_rsplit_lr(p, q->map_grid(), q->wl, q->wk, q->mrow)) & ~1 : 0;
}

int oa_plan_div_fused(const oa_plan* p) {
    if (!p || !p->pipe) return 0;
    const Pipeline* q = (const Pipeline*)p->pipe;
    if (p->mixed) { band_options((Pipeline*)q); return (q->FG && q->ids && q->band) ? oa_plan_div_fused(q->band) : 0; }
    if (!q->FG || !q->ids || !q->opt_divbin) return 0;
    const int rows = q->map_grid() ? q->map_grid() : p->ny;     // rows of the grid the from-map divergence runs on
    const bool sp = p->dtype == OA_F32 ? Fft2dPlan<float>::single_pass_div() : Fft2dPlan<double>::single_pass_div();
    if (!(sp && (rows == 1024 || rows == 2048 || rows == 4096 || (q->my3 && rows == q->my3)))) return 0;
    const int logc = div_tile_logc(p, rows);           // columns per 128 KB tile of this grid and precision
    const long tiles = ((long)(q->wk > 0 ? q->wk : p->nx / 2 + 1) + (1 << logc) - 1) >> logc;
    return (tiles * MC_BATCH_MAX * q->nids <= (long)(oa_bin_scratch_bytes(q->nids) / 8) * MC_BATCH_MAX) ? 1 : 0;
}

int oa_plan_set_filters(oa_plan* p, const void* FG, const void* FH, const void* Fnorm, int leg_cols, int kappa_cols,
                        int leg_rows, int kappa_rows, int mrow) {
    OA_REQUIRE(p && FG && FH && Fnorm, "oa_plan_set_filters: NULL argument");
    OA_REQUIRE(p->pow2 || p->mixed, "oa_plan_set_filters: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no "
               "one-call path (use the modular oa_qe_legs / oa_mul_real / oa_qe_div calls)");
    OA_REQUIRE(p->have_laxes, "oa_plan_set_filters: call oa_plan_set_laxes first");
    if (p->pow2) {                             // a band wider than the plane would run the column / row loops past the hc planes
        const int hw = p->nx / 2 + 1;
        OA_REQUIRE(leg_cols <= hw && kappa_cols <= hw, "oa_plan_set_filters: leg / kappa columns beyond the hc plane (> nx / 2 + 1)");
        OA_REQUIRE(2L * leg_rows - 1 <= p->ny && 2L * kappa_rows - 1 <= p->ny, "oa_plan_set_filters: leg / kappa rows beyond the plane (2 rows - 1 > ny)");
    }
    Pipeline* q = pipe_of(p);
    q->FG = FG; q->FH = FH; q->Fn = Fnorm;
    ++q->bind_gen;                             // the tile-major copy of Fnorm is repacked by the next call that uses it
    q->wl = leg_cols; q->wk = kappa_cols; q->rl = leg_rows; q->rk = kappa_rows; q->mrow = mrow;
    q->mcol = mrow == 0 ? 0 : -1;             // the map's own grid in x means the map's own grid in y too
    if (int rc = ensure_work(p, q)) { if (p->mixed) q->FG = nullptr; return rc; }
    if (p->mixed) {                            // BAND GRID: inner plan + inner-layout copies of the filters (and of the bins, if bound)
        int rc = mixed_bind(p, q);
        if (rc) q->FG = nullptr;
        return rc;
    }
    return resolve_col_grid(p, q);
}

int oa_plan_set_bins(oa_plan* p, const int32_t* ids_hc, int nids, double norm, void* stream) {
    OA_REQUIRE(p && ids_hc && nids >= 3, "oa_plan_set_bins: bad argument");
    Pipeline* q = pipe_of(p);
    if (int rc = ensure_work(p, q)) return rc;
    if (q->nids != nids) {
        if (q->bin_scratch) { OA_HIP(hipDeviceSynchronize()); (void)hipFree(q->bin_scratch); (void)hipFree(q->sums); (void)hipFree(q->counts_full); (void)hipFree(q->counts_tmp); }
        const long sb = oa_bin_scratch_bytes(nids);
        OA_REQUIRE(sb > 0, "oa_plan_set_bins: bad nids");
        // (x MC_BATCH_MAX: oa_mc_run bins a batch of realisations per launch)
        OA_HIP(hipMalloc(&q->bin_scratch, (size_t)sb * MC_BATCH_MAX));
        OA_HIP(hipMalloc((void**)&q->sums, MC_BATCH_MAX * nids * sizeof(double)));
        OA_HIP(hipMalloc((void**)&q->counts_full, nids * sizeof(int64_t)));
        OA_HIP(hipMalloc((void**)&q->counts_tmp, MC_BATCH_MAX * nids * sizeof(int64_t)));
    }
    if (!q->ticket) {
        OA_HIP(hipMalloc((void**)&q->ticket, sizeof(unsigned)));
        OA_HIP(hipMemset(q->ticket, 0, sizeof(unsigned)));
    }
    q->ids = ids_hc; q->nids = nids; q->norm = norm;
    ++q->bind_gen;
    // mode counts per bin over the WHOLE plane (the per-call binning visits only kappa's active region)
    if (p->kp % 4 == 0) {
        if (int rc = oa_bin_power(p->dtype, q->c[0], q->c[0], norm, ids_hc, nullptr, (long)p->ny * p->kp, nids, p->kp, p->nx / 2, q->sums,
                                  q->counts_full, nullptr, q->bin_scratch, 0, 0, stream)) return rc;
    } else {
        // nx / 2 odd (750 -> kp = 391): oa_bin_power moves four columns per lane and refuses such a pitch; the counts are taken from
        // copies padded to the next multiple of 4, the padding ignored (id -1) -- what Engine.bin_power does.  Set-up call: the
        // temporaries are released after a stream synchronisation
        const long kp4 = (p->kp + 3) / 4 * 4;
        const size_t es = elem_bytes(p);
        int32_t* ids4 = nullptr;
        void* z4 = nullptr;
        OA_HIP(hipMalloc((void**)&ids4, (size_t)p->ny * kp4 * sizeof(int32_t)));
        hipError_t e = hipMalloc(&z4, (size_t)p->ny * kp4 * es);
        if (e == hipSuccess) e = hipMemsetAsync(ids4, 0xFF, (size_t)p->ny * kp4 * sizeof(int32_t), (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(z4, 0, (size_t)p->ny * kp4 * es, (hipStream_t)stream);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(ids4, kp4 * sizeof(int32_t), ids_hc, p->kp * sizeof(int32_t), p->kp * sizeof(int32_t), p->ny, hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream);
        int rc = e == hipSuccess ? oa_bin_power(p->dtype, z4, z4, norm, ids4, nullptr, (long)p->ny * kp4, nids, kp4, p->nx / 2, q->sums, q->counts_full,
                                                nullptr, q->bin_scratch, 0, 0, stream)
                                 : fail(std::string("oa_plan_set_bins: padded bin ids: ") + hipGetErrorString(e));
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipFree(ids4);
        if (z4) (void)hipFree(z4);
        if (rc) return rc;
    }
    if (p->mixed) return (q->FG && q->band) ? mixed_bins(p, q, (hipStream_t)stream) : 0;     // (else: when the filters are bound)
    return ensure_div_tables(p, q, (hipStream_t)stream);
}

void* oa_plan_kappa(oa_plan* p) { return (p && p->pipe) ? ((Pipeline*)p->pipe)->kk : nullptr; }
const int64_t* oa_plan_bin_counts(oa_plan* p) { return (p && p->pipe) ? ((Pipeline*)p->pipe)->counts_full : nullptr; }

// Binning + moments in the tail of the single-pass divergence launch (fft_divbin.hpp): the request the one-call entries hand to
// the divergence wrappers.  OA_OPT_DIV_BIN = 0: always the separate histogram launches (the path of the other geometries).
static bool divbin_enabled(const Pipeline* q) { return q->opt_divbin; }
// (re)build the tile-major copies of Fnorm / ids for the single-pass divergence launch on this plan's column grid.  Called where the
// filters, the bins and the grid are known (oa_plan_set_bins, and again by make_fuse_tabs if any of them changed since): the first
// build of a size allocates (one device synchronisation), later rebuilds are two small launches -- and the run table of the ids
// (divbin_runs.hpp), which is made on the host from the packed copy: one read-back and one upload per binding, the stream waited for.
static int build_run_table(const oa_plan* p, Pipeline* q, Pipeline::DivTabs* t, int rows, int logc, long tiles, hipStream_t st) {
    t->has_runs = false;
    const int nxh = p->nx / 2;
    const int w = q->wk > nxh + 1 ? nxh + 1 : q->wk;                            // Fft2dPlan::clampw / clampr on the coarse grid
    const int rb = (q->rk <= 0 || 2L * q->rk - 1 >= rows) ? 0 : q->rk;
    const int cap = 2 * ((rows << logc) / 16);                                  // two entries per thread of the launch
    std::vector<int32_t> host((size_t)(tiles * rows) << logc);
    OA_HIP(hipMemcpyAsync(host.data(), t->ids_t.p, host.size() * 4, hipMemcpyDeviceToHost, st));
    OA_HIP(hipStreamSynchronize(st));
    DivRunTable tab;
    if (!divbin_build_runs(host.data(), (int)tiles, rows, logc, w, rb, q->nids, nxh, cap, &tab)) return 0;     // no run table: DivBinTail
    if (int rc = t->run_ent.reserve((tab.ent.size() + 1) * 8)) return rc;
    if (int rc = t->run_off.reserve(tab.off.size() * 4)) return rc;
    OA_HIP(hipMemcpyAsync(t->run_ent.p, tab.ent.data(), tab.ent.size() * 8, hipMemcpyHostToDevice, st));
    OA_HIP(hipMemcpyAsync(t->run_off.p, tab.off.data(), tab.off.size() * 4, hipMemcpyHostToDevice, st));
    OA_HIP(hipStreamSynchronize(st));
    t->has_runs = true; t->run_w = w; t->run_rb = rb; t->run_cap = cap;
    return 0;
}
static int ensure_div_tables(oa_plan* p, Pipeline* q, hipStream_t st, int rows) {
    Pipeline::DivTabs* const t = &q->tabs_of(rows);
    if (!(q->Fn && q->ids && (rows == 1024 || rows == 2048 || rows == 4096 || (q->my3 && rows == q->my3)) && q->wk > 0)) { t->tab_rows = 0; return 0; }
    const int logc = div_tile_logc(p, rows);
    if (t->tab_gen == q->bind_gen && t->tab_rows == rows && t->tab_logc == logc && t->tab_wk == q->wk) return 0;
    const size_t rs = p->dtype == OA_F32 ? 4 : 8;
    const long tiles = ((long)q->wk + (1 << logc) - 1) >> logc, total = (tiles * rows) << logc;
    if (int rc = t->fn_t.reserve((size_t)total * rs)) return rc;
    if (int rc = t->ids_t.reserve((size_t)total * 4)) return rc;
    if (int rc = pack_tiles(p, q->Fn, t->fn_t.p, rows, logc, q->wk, (int)rs, st)) return rc;
    if (int rc = pack_tiles(p, q->ids, t->ids_t.p, rows, logc, q->wk, 4, st)) return rc;
    if (int rc = build_run_table(p, q, t, rows, logc, tiles, st)) return rc;
    t->tab_gen = q->bind_gen; t->tab_rows = rows; t->tab_logc = logc; t->tab_wk = q->wk;
    return 0;
}
// both grids of the plan (the from-map grid's tables only where it differs)
static int ensure_div_tables(oa_plan* p, Pipeline* q, hipStream_t st) {
    if (int rc = ensure_div_tables(p, q, st, q->my)) return rc;
    return q->my3 ? ensure_div_tables(p, q, st, q->my3) : 0;
}
// the packed filter table of the R-split column stage for the bound filters on this plan's column grid, (re)made when the filters, the
// band or the grid changed: nullptr when this geometry does not take the R-split path (or on failure: the kernel then reads the planes)
static const void* fband_table(oa_plan* p, Pipeline* q, hipStream_t st) {
    static const bool off = exp_env("OA_NO_FBAND_TABLE") != nullptr;        // A/B switch
    const int my = q->map_grid();                  // (the R-split column stage exists on the from-map path only)
    if (off || !q->FG || my <= 0 || !qe_rsplit_lr(p, my, q->wl, q->wk, q->mrow)) return nullptr;
    if (q->fb_t.p && q->fb_gen == q->bind_gen && q->fb_my == my && q->fb_wl == q->wl && q->fb_rl == q->rl) return q->fb_t.p;
    if (q->fb_t.reserve((size_t)qe_fband_table_entries(p, q->wl, my) * elem_bytes(p))) { (void)hipGetLastError(); return nullptr; }
    if (qe_fband_pack_w(p, q->FG, q->FH, q->fb_t.p, q->wl, q->rl, my, st)) return nullptr;
    q->fb_gen = q->bind_gen; q->fb_my = my; q->fb_wl = q->wl; q->fb_rl = q->rl;
    return q->fb_t.p;
}
// rows: the grid of the divergence launch the request goes to (-1: the column grid `my`)
static DivBinFuse make_fuse(const oa_plan* p, const Pipeline* q, int64_t* n, double* S, double* C, int store, int rows = -1) {
    DivBinFuse f{};
    if (rows < 0) rows = q->my;
    const Pipeline::DivTabs& t = q->tabs_of(rows);
    if (t.tab_rows && t.tab_gen == q->bind_gen && t.tab_rows == rows && t.tab_wk == q->wk) {
        f.ids_t = (const int32_t*)t.ids_t.p; f.fn_t = t.fn_t.p; f.tab_logc = t.tab_logc; f.tab_rows = t.tab_rows;
        if (t.has_runs) {
            f.run_ent = (const unsigned long long*)t.run_ent.p; f.run_off = (const int32_t*)t.run_off.p;
            f.run_w = t.run_w; f.run_rb = t.run_rb; f.run_cap = t.run_cap;
        }
    }
    f.ids = q->ids; f.ipitch = p->kp; f.pnorm = q->norm; f.nids = q->nids; f.nxh = p->nx / 2;
    f.part = (double*)q->bin_scratch; f.part_cap = (long)(oa_bin_scratch_bytes(q->nids) / (long)sizeof(double)) * MC_BATCH_MAX;
    f.sums = q->sums; f.mcounts = q->counts_full; f.n = n; f.S = S; f.C = C; f.store = store; f.done = false;
    return f;
}

static int qe_tt_impl(oa_plan* p, const void* real_map, const void* kX, const void* kY, void* out_kappa_hc, int zero_outside,
                      void* stream, DivBinFuse* fuse, int rows_done = 0);
static int qe_mv_pow2(oa_plan* p, Pipeline* q, const MvCall& c, void* out, int accumulate, int leg_cols, int kappa_cols, int leg_rows,
                      int kappa_rows, int mrow, int zero_outside, hipStream_t st, bool keep_planes);
int oa_qe_tt(oa_plan* p, const void* real_map, const void* kX, const void* kY, void* out_kappa_hc, int zero_outside,
             void* stream) {
    if (p && p->mixed) {
        OA_REQUIRE(p->pipe && ((Pipeline*)p->pipe)->FG, "oa_qe_tt: call oa_plan_set_filters first");
        OA_REQUIRE((real_map != nullptr) != (kX != nullptr), "oa_qe_tt: pass either a real map or the Fourier-space leg(s)");
        return mixed_qe_tt(p, (Pipeline*)p->pipe, real_map, kX, kY, out_kappa_hc, zero_outside, (hipStream_t)stream);
    }
    return qe_tt_impl(p, real_map, kX, kY, out_kappa_hc, zero_outside, stream, nullptr);
}
// rows_done: the row-transformed map already sits on the plan's scratch plane (qe_windowed_rows_w): column stages only, multi-pass
static int qe_tt_impl(oa_plan* p, const void* real_map, const void* kX, const void* kY, void* out_kappa_hc, int zero_outside,
                      void* stream, DivBinFuse* fuse, int rows_done) {
    OA_REQUIRE(p && p->pipe && ((Pipeline*)p->pipe)->FG, "oa_qe_tt: call oa_plan_set_filters first");
    OA_REQUIRE((real_map != nullptr) != (kX != nullptr), "oa_qe_tt: pass either a real map or the Fourier-space leg(s)");
    Pipeline* q = (Pipeline*)p->pipe;
    void* out = out_kappa_hc ? out_kappa_hc : q->kk;
    if (out_kappa_hc && zero_outside)
        if (int rc = zero_complement(p, out, q->wk, q->rk, (hipStream_t)stream)) return rc;
    // intermediates live on the plan's compact work planes (Fft2dPlan::work_pitch): only `out` has the caller's pitch
    const long pl = work_pitch(p, q->wl), pk = work_pitch(p, q->wk);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    // from a map: R-split row pass + one column kernel, on the from-map grid where the plan carries one
    const int my = (real_map && !rows_done) ? q->map_grid() : q->my;
    const int lr = (real_map && !rows_done) ? qe_rsplit_lr(p, my, q->wl, q->wk, q->mrow) : 0;
    if (real_map) rc = qe_map_legs_cols_w(p, real_map, q->FG, q->FH, q->c[0], q->c[1], q->c[2], q->wl, q->rl, pl, st, rows_done ? 6 : 7, my, lr,
                                          lr ? fband_table(p, q, st) : nullptr);
    else rc = qe_legs_cols_w(p, kX, kY ? kY : kX, q->FG, q->FH, q->c[0], q->c[1], q->c[2], q->wl, q->rl, pl, st, my);
    if (rc) return rc;
    const double s = 1.0 / ((double)p->ny * p->nx), sy = my ? (double)p->ny / my : 1.0;   // DFT on my rows = my/ny x the full one
    if ((rc = qe_rows_w(p, q->c[0], q->c[1], q->c[2], q->g[0], q->g[1], s * s * sy, 0, q->wl, q->wk, q->mrow, pl, pk, st, my, lr))) return rc;
    return qe_cols_div_w(p, q->g[0], q->g[1], q->Fn, out, 0, q->wk, q->rk, pk, st, my, fuse);
}

int oa_qe_pol(oa_plan* p, int npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH,
              const int* host_swap, const void* kX, const void* kY, const void* Fnorm, void* out, int accumulate,
              int leg_cols, int kappa_cols, int leg_rows, int kappa_rows, int mrow, int zero_outside, void* stream) {
    OA_REQUIRE(p && npieces >= 1 && host_signs && host_FG && host_FH && kX && kY && Fnorm && out, "oa_qe_pol: bad argument");
    OA_REQUIRE(p->pow2 || p->mixed, "oa_qe_pol: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path "
               "(use the modular oa_qe_legs / oa_mul_real / oa_qe_div calls)");
    Pipeline* q = pipe_of(p);
    if (p->mixed) {                                 // BAND GRID: the planes bound by oa_qe_band_bind, on the inner plan
        const MvCall c{1, &npieces, host_signs, host_FG, host_FH, host_swap, &kX, &kY, &Fnorm, true};
        return mixed_qe_mv(p, q, c, out, accumulate, leg_cols, kappa_cols, leg_rows, kappa_rows, mrow, zero_outside, (hipStream_t)stream);
    }
    if (int rc = ensure_work(p, q)) return rc;
    if (!accumulate && zero_outside && out != q->kk)
        if (int rc = zero_complement(p, out, kappa_cols, kappa_rows, (hipStream_t)stream)) return rc;
    const long pl = work_pitch(p, leg_cols), pk = work_pitch(p, kappa_cols);
    hipStream_t st = (hipStream_t)stream;
    int my = 0;                                     // column grid from this call's row bands (policy: oa_plan_set_col_grid)
    if (int rc = resolve_my(p, mrow == 0 ? 0 : q->mcol, leg_rows, kappa_rows, &my)) return rc;
    const double s = 1.0 / ((double)p->ny * p->nx), sy = my ? (double)p->ny / my : 1.0;
    // products accumulate in g[0], g[1] over the separable pieces (compact work planes)
    for (int i = 0; i < npieces; ++i) {
        const bool sw = host_swap && host_swap[i];
        int rc = qe_legs_cols_w(p, sw ? kY : kX, sw ? kX : kY, host_FG[i], host_FH[i], q->c[0], q->c[1], q->c[2], leg_cols, leg_rows, pl, st, my);
        if (rc) return rc;
        if ((rc = qe_rows_w(p, q->c[0], q->c[1], q->c[2], q->g[0], q->g[1], host_signs[i] * s * s * sy, i > 0, leg_cols, kappa_cols, mrow, pl, pk, st, my))) return rc;
    }
    return qe_cols_div_w(p, q->g[0], q->g[1], Fnorm, out, accumulate, kappa_cols, kappa_rows, pk, st, my);
}

/* flat_taylens (lensing.py:395-440) of nmaps real maps by ONE deflection field, given as its nearest-pixel shifts and sub-pixel
 * remainders (oa_lens_split): out_m(x) = sum_{a + b < order} dx^a dy^b / (a! b!) D_ab[m](x + shift).  Per call: nmaps R2Cs, then the
 * inverse transforms of all nmaps * nd derivative fields (nd = order (order + 1) / 2 - 1), separably (lens_derivs_impl, fft.hip): per
 * (map, y-derivative order b) the column transform of (i ly)^b k on ONE hc plane and a row launch that takes every x-derivative at
 * its load -- and one gather pass per map.  The planes live in a plan-owned pool (allocated / grown on first use: that call
 * synchronises the device once; oa_plan_release_pools frees it). */
static int lens_maps_impl(oa_plan* p, int nmaps, const void* real_in, long in_stride, const void* hc_in, long hc_stride, double hc_scale, int order,
                          const int32_t* shift_x, const int32_t* shift_y, const void* dx, const void* dy, void* real_out, long out_stride, void* stream) {
    const long rplane = (long)p->ny * p->nx;
    Pipeline* q = pipe_of(p);
    const size_t rs = p->dtype == OA_F32 ? 4 : 8;
    const int nd = order * (order + 1) / 2 - 1;
    const int d00 = hc_in ? 1 : 0;               // transforms in: the undisplaced map is a pool plane too (the first of each map's nd + 1)
    hipStream_t st = (hipStream_t)stream;
    char* realp = nullptr;
    if (nd + d00 > 0) {
        const size_t hcb = plane_bytes(p), rb = (size_t)rplane * rs;
        const int chunk = 1;                      // ONE hc plane: the column-transformed field of the current (map, y-derivative order)
        const size_t nk0 = hc_in ? 0 : (size_t)nmaps;
        if (int rc = q->lens_pool.reserve(nk0 * hcb + (size_t)chunk * hcb + (size_t)nmaps * (nd + d00) * rb)) return rc;
        char* k0 = q->lens_pool.at();
        char* hcp = k0 + nk0 * hcb;
        realp = hcp + (size_t)chunk * hcb;
        if (int rc = qe_lens_derivs_w(p, nmaps, real_in, in_stride, k0, hcp, realp, nd, st, hc_in, hc_stride, hc_scale)) return rc;
    }
    for (int m = 0; m < nmaps; ++m) {
        const char* pm = realp + (size_t)m * (nd + d00) * rplane * rs;
        const void* src = hc_in ? (const void*)pm : (const void*)((const char*)real_in + (size_t)m * in_stride * rs);
        void* dst = (char*)real_out + (size_t)m * out_stride * rs;
        if (int rc = oa_lens_taylor(p, src, nd > 0 ? pm + (size_t)d00 * rplane * rs : nullptr, rplane, order, shift_x, shift_y, dx, dy, dst, stream)) return rc;
    }
    return 0;
}

int oa_lens_maps(oa_plan* p, int nmaps, const void* real_in, long in_stride, int order, const int32_t* shift_x, const int32_t* shift_y,
                 const void* dx, const void* dy, void* real_out, long out_stride, void* stream) {
    OA_REQUIRE(p && real_in && shift_x && shift_y && dx && dy && real_out && nmaps >= 1, "oa_lens_maps: bad argument");
    OA_REQUIRE(p->pow2 || p->mixed, "oa_lens_maps: needs map sides of the form 2^a 3^b 5^c");
    OA_REQUIRE(p->have_laxes, "oa_lens_maps: call oa_plan_set_laxes first");
    OA_REQUIRE(order >= 1 && order <= 8, "oa_lens_maps: order must be 1..8");
    OA_REQUIRE(real_in != real_out, "oa_lens_maps: in-place not supported");
    const long rplane = (long)p->ny * p->nx;
    OA_REQUIRE(in_stride >= rplane && out_stride >= rplane, "oa_lens_maps: plane stride smaller than a plane");
    return lens_maps_impl(p, nmaps, real_in, in_stride, nullptr, 0, 1.0, order, shift_x, shift_y, dx, dy, real_out, out_stride, stream);
}

int oa_lens_maps_hc(oa_plan* p, int nmaps, const void* hc_in, long hc_stride, double scale, int order, const int32_t* shift_x,
                    const int32_t* shift_y, const void* dx, const void* dy, void* real_out, long out_stride, void* stream) {
    OA_REQUIRE(p && hc_in && shift_x && shift_y && dx && dy && real_out && nmaps >= 1, "oa_lens_maps_hc: bad argument");
    OA_REQUIRE(p->pow2 || p->mixed, "oa_lens_maps_hc: needs map sides of the form 2^a 3^b 5^c");
    OA_REQUIRE(p->have_laxes, "oa_lens_maps_hc: call oa_plan_set_laxes first");
    OA_REQUIRE(order >= 1 && order <= 8, "oa_lens_maps_hc: order must be 1..8");
    OA_REQUIRE(hc_stride >= (long)p->ny * p->kp && out_stride >= (long)p->ny * p->nx, "oa_lens_maps_hc: plane stride smaller than a plane");
    return lens_maps_impl(p, nmaps, nullptr, 0, hc_in, hc_stride, scale, order, shift_x, shift_y, dx, dy, real_out, out_stride, stream);
}

/* frees the plan-owned pools that the multi-map entries grow on demand (oa_lens_maps, oa_qe_mv / oa_qe_tt_splits, oa_mc_run, oa_mc_run_mv, oa_mc_run_mv_windowed): they
 * are reallocated by the next call that needs them.  Synchronises the device. */
int oa_plan_release_pools(oa_plan* p) {
    OA_REQUIRE(p, "oa_plan_release_pools: NULL plan");
    if (!p->pipe) return 0;
    Pipeline* q = (Pipeline*)p->pipe;
    OA_HIP(hipDeviceSynchronize());
    // band grid: the split entries' inner source planes and kappa block (bsplit), the draw and row planes of oa_mc_run_windowed (bwin), the
    // map-side scratch of oa_qe_mv_maps (mrows) and the N-grid planes of oa_mc_run_mv_windowed (mwin): all retaken by the next call
    for (DevBuf* b : {&q->lens_pool, &q->split_legs, &q->mc_src, &q->mvmc, &q->mvwin, &q->bsplit, &q->bwin, &q->pb.mrows, &q->pb.mwin, &q->rdn0_legs,
                      &q->rdn0_pool, &q->rdn0mv_legs, &q->rdn0mv_pool, &q->n1_pool}) b->release();
    q->bs_cap = 0;
    q->rdn0_gen = 0;                 // the data legs of oa_rdn0_set_data are gone: oa_mc_run_rdn0 asks for them again
    q->rdn0mv_key.clear();           // ... and those of oa_rdn0_set_data_mv
    // ... the pool the split entries' inner call grew (regrown on demand), and the inner planes of oa_rdn0_set_data / oa_mc_run_rdn0
    if (q->band && q->band->pipe)
        for (DevBuf* b : {&((Pipeline*)q->band->pipe)->split_legs, &((Pipeline*)q->band->pipe)->rdn0_legs, &((Pipeline*)q->band->pipe)->rdn0_pool}) b->release();
    // ... the inner planes of oa_rdn0_set_data_mv / oa_mc_run_rdn0_mv on the oa_qe_band_bind binding (its leg pool is the binding's: kept)
    if (q->pb.plan && q->pb.plan->pipe)
        for (DevBuf* b : {&((Pipeline*)q->pb.plan->pipe)->rdn0mv_legs, &((Pipeline*)q->pb.plan->pipe)->rdn0mv_pool}) b->release();
    // ... and the Monte-Carlo binding with its pool: oa_mc_mv_band_bind makes it again
    q->pb.mc.pool.release();
    q->pb.mc = Pipeline::PolBind::McBind();
    return 0;
}

int oa_filter_map(oa_plan* p, const void* real_in, const void* filt_hcreal, void* real_out, void* stream) {
    OA_REQUIRE(p && real_in && filt_hcreal && real_out, "oa_filter_map: NULL argument");
    Pipeline* q = pipe_of(p);
    if (int rc = ensure_work(p, q)) return rc;
    int rc = oa_fft_r2c(p, real_in, q->kT, 1.0, 0, 0, stream);
    if (rc) return rc;
    if ((rc = oa_cmul_real(p->dtype, q->kT, filt_hcreal, q->kT, (long)p->ny * p->kp, stream))) return rc;
    return oa_fft_c2r(p, q->kT, real_out, 1.0 / ((double)p->ny * p->nx), 0, stream);
}

// kappa_hat (plan-owned plane) -> bandpower sums over its active region -> n += 1, S += b, C += b b^T (b = bin means)
static int bandpower_moments(oa_plan* p, Pipeline* q, int64_t* n, double* S, double* C, void* stream, const void* kappa = nullptr) {
    // one launch: the last workgroup of the histogram reduces the partials and adds the bandpower vector to n, S, C
    return bin_power_moments(p->dtype, kappa ? kappa : q->kk, q->norm, q->ids, (long)p->ny * p->kp, q->nids, p->kp, p->nx / 2, q->sums, q->counts_tmp,
                             q->bin_scratch, q->wk, q->rk, q->ticket, q->counts_full, n, S, C, (hipStream_t)stream);
}

int oa_qe_tt_moments(oa_plan* p, const void* real_map, int64_t* n, double* S, double* C, void* stream) {
    OA_REQUIRE(p && p->pipe && ((Pipeline*)p->pipe)->FG && ((Pipeline*)p->pipe)->ids, "oa_qe_tt_moments: call oa_plan_set_filters and oa_plan_set_bins first");
    OA_REQUIRE(real_map && n && S && C, "oa_qe_tt_moments: NULL argument");
    Pipeline* q = (Pipeline*)p->pipe;
    if (p->mixed) return mixed_moments(p, q, real_map, n, S, C, (hipStream_t)stream);
    if (int rc = ensure_div_tables(p, q, (hipStream_t)stream)) return rc;
    DivBinFuse f = make_fuse(p, q, n, S, C, 0, q->map_grid());
    if (int rc = qe_tt_impl(p, real_map, nullptr, nullptr, nullptr, 0, stream, divbin_enabled(q) ? &f : nullptr)) return rc;
    if (f.done) return 0;                      // binned and accumulated in the divergence launch
    return bandpower_moments(p, q, n, S, C, stream);
}

/* oa_qe_mv from REAL MAPS on a 2^a 3^b 5^c plan (include/orphics_amd.h): the arguments are checked here, everything behind the source
 * stage is mixed_qe_mv's. */
int oa_qe_mv_maps(oa_plan* p, int nmaps, const void* const* host_maps, const void* rot_c, const void* rot_s, int nest, const int* host_npieces,
                  const double* host_signs, const void* const* host_FG, const void* const* host_FH, const int* host_swap, const int* host_xsrc,
                  const int* host_ysrc, const void* const* host_Fnorm, void* out, int accumulate, int leg_cols, int kappa_cols, int leg_rows,
                  int kappa_rows, int mrow, int zero_outside, void* stream) {
    OA_REQUIRE(p && host_maps && nest >= 1 && host_npieces && host_signs && host_FG && host_FH && host_xsrc && host_ysrc && host_Fnorm && out,
               "oa_qe_mv_maps: bad argument");
    OA_REQUIRE(!p->pow2, "oa_qe_mv_maps: a power-of-two plan has no band grid: oa_fft_r2c per map, oa_rot2 for Q, U and oa_qe_mv are the same "
               "steps there");
    OA_REQUIRE(p->mixed, "oa_qe_mv_maps: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path "
               "(use the modular oa_qe_legs / oa_mul_real / oa_qe_div calls)");
    OA_REQUIRE(nmaps >= 1 && nmaps <= POL_SRC_MAX, "oa_qe_mv_maps: 1 <= nmaps <= 6 real maps per call");
    for (int i = 0; i < nmaps; ++i) OA_REQUIRE(host_maps[i], "oa_qe_mv_maps: NULL map");
    OA_REQUIRE((rot_c != nullptr) == (rot_s != nullptr), "oa_qe_mv_maps: rot_c and rot_s are given together or not at all");
    OA_REQUIRE(!rot_c || nmaps == 3 || nmaps == 6, "oa_qe_mv_maps: the rotation planes need nmaps = 3 (T, Q, U) or 6 (and the Y-leg T, Q, U)");
    for (int e = 0; e < nest; ++e)
        OA_REQUIRE(host_xsrc[e] >= 0 && host_xsrc[e] < nmaps && host_ysrc[e] >= 0 && host_ysrc[e] < nmaps,
                   "oa_qe_mv_maps: source index outside [0, nmaps)");
    const MvCall c{nest, host_npieces, host_signs, host_FG, host_FH, host_swap, nullptr, nullptr, host_Fnorm, false,
                   nmaps, host_maps, rot_c, rot_s, host_xsrc, host_ysrc};
    return mixed_qe_mv(p, pipe_of(p), c, out, accumulate, leg_cols, kappa_cols, leg_rows, kappa_rows, mrow, zero_outside, (hipStream_t)stream);
}

/* Several estimators accumulated into one kappa plane (minimum-variance combination) with every distinct filtered field
 * transformed once: a leg plane is identified by (source transform, filter plane) pointers, so estimators that share a
 * filter plane object share the transform (TE / TB: the gradient of W^TE T cos, sin; EE / EB; TE / EE: E / C^EE cos, sin ...). */
int oa_qe_mv(oa_plan* p, int nest, const int* host_npieces, const double* host_signs, const void* const* host_FG,
             const void* const* host_FH, const int* host_swap, const void* const* host_kX, const void* const* host_kY,
             const void* const* host_Fnorm, void* out, int accumulate, int leg_cols, int kappa_cols, int leg_rows, int kappa_rows,
             int mrow, int zero_outside, void* stream) {
    OA_REQUIRE(p && nest >= 1 && host_npieces && host_signs && host_FG && host_FH && host_kX && host_kY && host_Fnorm && out,
               "oa_qe_mv: bad argument");
    OA_REQUIRE(p->pow2 || p->mixed, "oa_qe_mv: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path "
               "(use the modular oa_qe_legs / oa_mul_real / oa_qe_div calls)");
    Pipeline* q = pipe_of(p);
    if (p->mixed) {                                 // BAND GRID: the planes bound by oa_qe_band_bind, on the inner plan
        const MvCall c{nest, host_npieces, host_signs, host_FG, host_FH, host_swap, host_kX, host_kY, host_Fnorm, false};
        return mixed_qe_mv(p, q, c, out, accumulate, leg_cols, kappa_cols, leg_rows, kappa_rows, mrow, zero_outside, (hipStream_t)stream);
    }
    const MvCall c{nest, host_npieces, host_signs, host_FG, host_FH, host_swap, host_kX, host_kY, host_Fnorm, false};
    return qe_mv_pow2(p, q, c, out, accumulate, leg_cols, kappa_cols, leg_rows, kappa_rows, mrow, zero_outside, (hipStream_t)stream, false);
}

// the one-launch divergence of oa_qe_mv: 2 .. 6 estimators whose normalisation planes are evenly spaced (one stacked allocation)
static bool mv_div_batched(const Pipeline* q, int nest, const void* const* host_Fnorm, size_t rs, long* fn_moff) {
    bool dbatch = nest >= 2 && nest <= 6 && q->opt_mv_batch;
    if (dbatch) {
        const long d = (long)((const char*)host_Fnorm[1] - (const char*)host_Fnorm[0]);
        dbatch = d > 0 && d % (long)rs == 0;
        for (int e = 2; e < nest && dbatch; ++e) dbatch = ((const char*)host_Fnorm[e] - (const char*)host_Fnorm[0]) == e * d;
        *fn_moff = d / (long)rs;
    }
    return dbatch;
}

/* The body of oa_qe_mv on a power-of-two plan, shared with oa_mc_run_mv.  keep_planes (the caller has checked mv_div_batched): the
 * estimators' kappa_hat stay in the plan-owned planes c[0] + e planes, where the one-launch divergence writes them; they are not summed
 * and `out` is not touched. */
static int qe_mv_pow2(oa_plan* p, Pipeline* q, const MvCall& c, void* out, int accumulate, int leg_cols, int kappa_cols, int leg_rows,
                      int kappa_rows, int mrow, int zero_outside, hipStream_t st, bool keep_planes) {
    const int nest = c.nest;
    const int* const host_npieces = c.npieces;
    const double* const host_signs = c.signs;
    const void* const* const host_FG = c.FG;
    const void* const* const host_FH = c.FH;
    const int* const host_swap = c.swap;
    const void* const* const host_kX = c.kX;
    const void* const* const host_kY = c.kY;
    const void* const* const host_Fnorm = c.Fn;
    if (int rc = ensure_work(p, q)) return rc;
    if (!keep_planes && !accumulate && zero_outside && out != q->kk)
        if (int rc = zero_complement(p, out, kappa_cols, kappa_rows, st)) return rc;
    const long pl = work_pitch(p, leg_cols), pk = work_pitch(p, kappa_cols);
    int my = 0;
    if (int rc = resolve_my(p, mrow == 0 ? 0 : q->mcol, leg_rows, kappa_rows, &my)) return rc;
    // distinct leg planes: gradient pairs (source, FG) and H planes (source, FH)
    struct Key { const void* src; const void* f; };
    std::vector<Key> grad, hpl;
    std::vector<int> gslot, hslot;
    auto slot_of = [](std::vector<Key>& v, const void* src, const void* f) {
        for (size_t i = 0; i < v.size(); ++i) if (v[i].src == src && v[i].f == f) return (int)i;
        v.push_back(Key{src, f});
        return (int)v.size() - 1;
    };
    int total = 0;
    for (int e = 0; e < nest; ++e) {
        OA_REQUIRE(host_npieces[e] >= 1 && host_kX[e] && host_kY[e] && host_Fnorm[e], "oa_qe_mv: bad estimator entry");
        for (int i = 0; i < host_npieces[e]; ++i, ++total) {
            OA_REQUIRE(host_FG[total] && host_FH[total], "oa_qe_mv: NULL filter plane");
            const bool sw = host_swap && host_swap[total];
            gslot.push_back(slot_of(grad, sw ? host_kY[e] : host_kX[e], host_FG[total]));
            hslot.push_back(slot_of(hpl, sw ? host_kX[e] : host_kY[e], host_FH[total]));
        }
    }
    const int ng = (int)grad.size(), nh = (int)hpl.size(), nplanes = 2 * ng + nh;
    const size_t es = elem_bytes(p);
    const size_t lb = (size_t)pl * p->ny * es;                      // one compact leg plane
    // pool: leg planes | 2 product planes per estimator | 2 pass-1 planes per estimator (two-pass divergence)
    const size_t lbk = (size_t)pk * p->ny * es;                     // one compact product plane
    if (int rc = ensure_pool(q, nplanes * lb + 4 * (size_t)nest * lbk)) return rc;
    char* const prod = q->split_legs.at(nplanes * lb);
    char* const tmp = prod + 2 * (size_t)nest * lbk;
    auto plane = [&](int k) { return (void*)q->split_legs.at((size_t)k * lb); };      // gradient pair g: 2g, 2g + 1; H plane h: 2 ng + h
    // all leg planes in ONE inverse pass-1 launch when the fields come from at most three sources (T, E, B)
    std::vector<const void*> srcs;
    unsigned long long srcsel = 0;
    bool batch = ng + nh <= 32 && q->opt_mv_batch;                  // (OA_OPT_MV_BATCH = 0: one launch per field)
    int legs_done = 0;
    for (int f = 0; f < ng + nh && batch; ++f) {
        const void* sp = f < ng ? grad[f].src : hpl[f - ng].src;
        size_t k = 0;
        while (k < srcs.size() && srcs[k] != sp) ++k;
        if (k == srcs.size()) srcs.push_back(sp);
        if (srcs.size() > 3) batch = false;
        srcsel |= (unsigned long long)k << (2 * f);
    }
    if (batch) {
        std::vector<const void*> key;
        for (int g = 0; g < ng; ++g) key.push_back(grad[g].f);
        for (int h = 0; h < nh; ++h) key.push_back(hpl[h].f);
        if (!q->mv_ftab) OA_HIP(hipMalloc((void**)&q->mv_ftab, 32 * sizeof(void*)));
        if (key != q->mv_fkey) {       // (pageable source: staged before the call returns; ordered on this stream)
            OA_HIP(hipMemcpyAsync(q->mv_ftab, key.data(), key.size() * sizeof(void*), hipMemcpyHostToDevice, st));
            q->mv_fkey = key;
        }
        const long off1 = srcs.size() > 1 ? (long)(((const char*)srcs[1] - (const char*)srcs[0]) / (long)es) : 0;
        const long off2 = srcs.size() > 2 ? (long)(((const char*)srcs[2] - (const char*)srcs[0]) / (long)es) : 0;
        bool aligned = true;
        for (size_t k = 1; k < srcs.size(); ++k) aligned = aligned && (((const char*)srcs[k] - (const char*)srcs[0]) % (long)es == 0);
        if (aligned) {
            if (int rc = qe_legs_batch_w(p, srcs[0], off1, off2, srcsel, (const void* const*)q->mv_ftab, ng, nh, q->split_legs.p, (long)(lb / es),
                                         leg_cols, leg_rows, pl, st, my, 2, &legs_done)) return rc;
        } else batch = false;
    }
    if (!batch) {
        for (int g = 0; g < ng; ++g)
            if (int rc = qe_legs_subset_w(p, grad[g].src, grad[g].f, plane(2 * g), plane(2 * g + 1), 2, leg_cols, leg_rows, pl, st, my)) return rc;
        for (int h = 0; h < nh; ++h)
            if (int rc = qe_legs_subset_w(p, hpl[h].src, hpl[h].f, plane(2 * ng + h), nullptr, 1, leg_cols, leg_rows, pl, st, my)) return rc;
    }
    if (!legs_done)                  // (single-pass leg kernel on 1024- / 2048-row column grids: nothing left to do)
        if (int rc = qe_legs_pass2_w(p, q->split_legs.p, nplanes, (long)(lb / es), leg_cols, pl, st, my)) return rc;
    const double s = 1.0 / ((double)p->ny * p->nx), sy = my ? (double)p->ny / my : 1.0;
    // divergence of all estimators in ONE launch when their Fnorm planes are evenly spaced (one stacked allocation): each
    // estimator's weighted kappa goes to its own plan-owned plane (c[0..2], g[0..1], kT are contiguous and unused here),
    // then one pass sums them in estimator order
    const size_t rs = es / 2;
    long fn_moff = 0;
    bool dbatch = mv_div_batched(q, nest, host_Fnorm, rs, &fn_moff);
    // ROW STAGE: the k-th separable piece of every estimator in ONE launch (they write different product planes; a launch
    // of one piece is 1024 workgroups of two waves and leaves most of the chip's wave slots empty), per-piece planes and
    // scales through a device table; pieces k > 0 accumulate.  Same arithmetic per piece, same order per estimator.
    bool rbatch = dbatch && total <= 64 && q->opt_mv_rowbatch;
    if (rbatch) {
        int maxp = 0;
        for (int e = 0; e < nest; ++e) maxp = std::max(maxp, host_npieces[e]);
        std::vector<const void*> tgx, tgy, th;
        std::vector<void*> tpx, tpy;
        std::vector<double> tsc;
        std::vector<int> count(maxp, 0);
        for (int k = 0; k < maxp; ++k) {
            int base = 0;
            for (int e = 0; e < nest; base += host_npieces[e], ++e) {
                if (host_npieces[e] <= k) continue;
                const int idx = base + k;
                tgx.push_back(plane(2 * gslot[idx])); tgy.push_back(plane(2 * gslot[idx] + 1)); th.push_back(plane(2 * ng + hslot[idx]));
                tpx.push_back(prod + 2 * (size_t)e * lbk); tpy.push_back(prod + (2 * (size_t)e + 1) * lbk);
                tsc.push_back(host_signs[idx] * s * s * sy);
                ++count[k];
            }
        }
        std::vector<unsigned long long> key;
        for (size_t i = 0; i < tgx.size(); ++i) {
            unsigned long long bits;
            memcpy(&bits, &tsc[i], sizeof bits);
            key.insert(key.end(), {(unsigned long long)(uintptr_t)tgx[i], (unsigned long long)(uintptr_t)tgy[i], (unsigned long long)(uintptr_t)th[i],
                                   (unsigned long long)(uintptr_t)tpx[i], (unsigned long long)(uintptr_t)tpy[i], bits});
        }
        key.push_back((unsigned long long)my); key.push_back((unsigned long long)(unsigned)mrow); key.push_back((unsigned long long)p->dtype);
        const size_t eb = qe_rows_table_entry_bytes(p);
        if (!q->mv_rtab) OA_HIP(hipMalloc(&q->mv_rtab, 64 * 64 + 1024));
        const int upload = key != q->mv_rkey;
        size_t off = 0;
        // ESTIMATOR CHAINS: one launch for all estimators, each workgroup loops over its estimator's pieces and keeps the
        // summed products in registers (3 n + 2 transforms per row pair instead of 5 n; no read-modify-write of the product
        // planes).  OA_OPT_MV_CHAIN = 0: the piece-by-piece launches below
        bool chained = false;
        if (q->opt_mv_chain) {
            std::vector<const void*> cgx, cgy, chh;
            std::vector<void*> cpx, cpy;
            std::vector<double> csc;
            std::vector<int> first(nest), cnt(nest);
            int base = 0;
            for (int e = 0; e < nest; base += host_npieces[e], ++e) {
                first[e] = (int)cgx.size(); cnt[e] = host_npieces[e];
                for (int i = 0; i < host_npieces[e]; ++i) {
                    const int idx = base + i;
                    cgx.push_back(plane(2 * gslot[idx])); cgy.push_back(plane(2 * gslot[idx] + 1)); chh.push_back(plane(2 * ng + hslot[idx]));
                    cpx.push_back(prod + 2 * (size_t)e * lbk); cpy.push_back(prod + (2 * (size_t)e + 1) * lbk);
                    csc.push_back(host_signs[idx] * s * s * sy);
                }
            }
            std::vector<unsigned long long> ckey = key;
            ckey.push_back(0xC4A1ull);
            const int up = ckey != q->mv_rkey;
            int rc = qe_rows_chain_w(p, nest, total, cgx.data(), cgy.data(), chh.data(), cpx.data(), cpy.data(), csc.data(), first.data(), cnt.data(),
                                     q->mv_rtab, up, leg_cols, kappa_cols, mrow, pl, pk, st, my);
            if (rc > 0) return rc;
            if (rc == 0) { chained = true; q->mv_rkey = ckey; }
        }
        for (int k = 0; k < maxp && rbatch && !chained; ++k) {
            int rc = qe_rows_table_w(p, count[k], tgx.data() + off, tgy.data() + off, th.data() + off, tpx.data() + off, tpy.data() + off,
                                     tsc.data() + off, (char*)q->mv_rtab + off * eb, upload, k > 0, leg_cols, kappa_cols, mrow, pl, pk, st, my);
            if (rc < 0) { rbatch = false; break; }      // (only possible at k = 0: nothing launched yet)
            if (rc) return rc;
            off += count[k];
        }
        if (rbatch && !chained) q->mv_rkey = key;
    }
    int at = 0;
    for (int e = 0; e < nest && !rbatch; ++e) {
        void* g0 = dbatch ? (void*)(prod + 2 * (size_t)e * lbk) : q->g[0];
        void* g1 = dbatch ? (void*)(prod + (2 * (size_t)e + 1) * lbk) : q->g[1];
        for (int i = 0; i < host_npieces[e]; ++i, ++at) {
            int rc = qe_rows_w(p, plane(2 * gslot[at]), plane(2 * gslot[at] + 1), plane(2 * ng + hslot[at]), g0, g1,
                               host_signs[at] * s * s * sy, i > 0, leg_cols, kappa_cols, mrow, pl, pk, st, my);
            if (rc) return rc;
        }
        if (!dbatch)
            if (int rc = qe_cols_div_w(p, g0, g1, host_Fnorm[e], out, (accumulate || e > 0) ? 1 : 0, kappa_cols, kappa_rows, pk, st, my)) return rc;
    }
    if (dbatch) {
        if (int rc = qe_cols_div_batch_w(p, prod, prod + lbk, host_Fnorm[0], q->c[0], tmp, nest, (long)(2 * lbk / es), fn_moff, plane_elems(p),
                                         kappa_cols, kappa_rows, pk, st, my)) return rc;
        if (keep_planes) return 0;
        // (the divergence writes columns <= nx/2 only: the planes' row padding beyond holds whatever the work planes held)
        const int wsum = (kappa_cols > 0 && kappa_cols <= p->nx / 2 + 1) ? kappa_cols : p->nx / 2 + 1;
        return sum_region(p->dtype, q->c[0], plane_elems(p), nest, out, accumulate ? 1 : 0, p->ny, p->kp, wsum, kappa_rows, st);
    }
    return 0;
}

int oa_qe_tt_splits(oa_plan* p, int nsplits, const void* const* host_kmaps, void* const* host_out, int zero_outside, void* stream) {
    OA_REQUIRE(p && p->pipe && ((Pipeline*)p->pipe)->FG, "oa_qe_tt_splits: call oa_plan_set_filters first");
    OA_REQUIRE(nsplits >= 1 && nsplits <= 64 && host_kmaps && host_out, "oa_qe_tt_splits: bad argument");
    Pipeline* q = (Pipeline*)p->pipe;
    hipStream_t st = (hipStream_t)stream;
    if (p->mixed) return mixed_qe_tt_splits(p, q, "oa_qe_tt_splits", nsplits, host_kmaps, host_out, nullptr, 0.0, zero_outside, st);
    const long pl = work_pitch(p, q->wl), pk = work_pitch(p, q->wk);
    const size_t lb = (size_t)pl * p->ny * elem_bytes(p);      // one compact leg plane
    const size_t es = elem_bytes(p), lbk = (size_t)pk * p->ny * es;
    const int npairs = nsplits * nsplits;
    // evenly spaced output planes (one (n, n, Ny, kp) block): the divergence of all pairs runs as ONE launch
    bool dbatch = npairs >= 2 && q->opt_mv_batch;
    long out_moff = 0;
    if (dbatch) {
        const long d = (long)((char*)host_out[1] - (char*)host_out[0]);
        dbatch = d > 0 && d % (long)es == 0;
        for (int k = 2; k < npairs && dbatch; ++k) dbatch = host_out[k] && ((char*)host_out[k] - (char*)host_out[0]) == k * d;
        out_moff = d / (long)es;
    }
    // pool: 3 leg planes per split | 2 product planes per pair | 2 pass-1 planes per pair (two-pass divergence)
    if (int rc = ensure_pool(q, 3 * lb * nsplits + (dbatch ? 4 * (size_t)npairs * lbk : 0))) return rc;
    char* const prod = q->split_legs.at(3 * lb * nsplits);
    const int my = q->my;
    auto leg = [&](int i, int c) { return (void*)q->split_legs.at((3 * (size_t)i + c) * lb); };
    for (int i = 0; i < nsplits; ++i) {
        OA_REQUIRE(host_kmaps[i], "oa_qe_tt_splits: NULL split plane");
        if (int rc = qe_legs_cols_w(p, host_kmaps[i], host_kmaps[i], q->FG, q->FH, leg(i, 0), leg(i, 1), leg(i, 2), q->wl, q->rl, pl, st, my)) return rc;
    }
    const double s = 1.0 / ((double)p->ny * p->nx), sy = my ? (double)p->ny / my : 1.0;
    for (int i = 0; i < nsplits; ++i)
        for (int j = 0; j < nsplits; ++j) {
            const int k = i * nsplits + j;
            void* out = host_out[k];
            OA_REQUIRE(out, "oa_qe_tt_splits: NULL output plane");
            int rc;
            if (zero_outside && (rc = zero_complement(p, out, q->wk, q->rk, st))) return rc;
            void* g0 = dbatch ? (void*)(prod + 2 * (size_t)k * lbk) : q->g[0];
            void* g1 = dbatch ? (void*)(prod + (2 * (size_t)k + 1) * lbk) : q->g[1];
            if ((rc = qe_rows_w(p, leg(i, 0), leg(i, 1), leg(j, 2), g0, g1, s * s * sy, 0, q->wl, q->wk, q->mrow, pl, pk, st, my))) return rc;
            if (!dbatch && (rc = qe_cols_div_w(p, g0, g1, q->Fn, out, 0, q->wk, q->rk, pk, st, my))) return rc;
        }
    if (dbatch)
        return qe_cols_div_batch_w(p, prod, prod + lbk, q->Fn, host_out[0], prod + 2 * (size_t)npairs * lbk, npairs, (long)(2 * lbk / es), 0,
                                   out_moff, q->wk, q->rk, pk, st, my);
    return 0;
}

/* The split-based 4-point estimate of the kappa power straight from the splits' transforms, on a band-grid plan: the n^2 pairwise
 * reconstructions run on the inner grid and are combined there per mode; only the real result is written on the map's grid. */
int oa_qe_tt_split_power(oa_plan* p, int nsplits, const void* const* host_kmaps, void* out_hcreal, double norm, int zero_outside, void* stream) {
    OA_REQUIRE(p && host_kmaps && out_hcreal, "oa_qe_tt_split_power: bad argument");
    OA_REQUIRE(nsplits >= 4 && nsplits <= 8, "oa_qe_tt_split_power: 4 <= nsplits <= 8");
    OA_REQUIRE(!p->pow2, "oa_qe_tt_split_power: a power-of-two plan has no band grid; there the estimate is oa_qe_tt_splits + oa_split_cross_power");
    OA_REQUIRE(p->pipe && ((Pipeline*)p->pipe)->FG, "oa_qe_tt_split_power: call oa_plan_set_filters first");
    return mixed_qe_tt_splits(p, (Pipeline*)p->pipe, "oa_qe_tt_split_power", nsplits, host_kmaps, nullptr, out_hcreal, norm, zero_outside,
                              (hipStream_t)stream);
}

/* Two Monte-Carlo steps in one call: both maps share every launch behind their row transforms (fft.hip qe_tt_pair_impl);
 * geometries without that path run the two steps one after the other.  n += 2, S += b0 + b1, C += b0 b0^T + b1 b1^T. */
int oa_qe_tt_moments2(oa_plan* p, const void* real_map0, const void* real_map1, int64_t* n, double* S, double* C, void* stream) {
    OA_REQUIRE(p && p->pipe && ((Pipeline*)p->pipe)->FG && ((Pipeline*)p->pipe)->ids, "oa_qe_tt_moments2: call oa_plan_set_filters and oa_plan_set_bins first");
    OA_REQUIRE(real_map0 && real_map1 && n && S && C, "oa_qe_tt_moments2: NULL argument");
    Pipeline* q = (Pipeline*)p->pipe;
    if (p->mixed) {                            // two steps on the band grid, map order
        if (int rc = mixed_moments(p, q, real_map0, n, S, C, (hipStream_t)stream)) return rc;
        return mixed_moments(p, q, real_map1, n, S, C, (hipStream_t)stream);
    }
    const long pl = work_pitch(p, q->wl), pk = work_pitch(p, q->wk);
    // second kappa plane: the plan-owned input-transform plane (unused on the from-map path); only kappa's active region of
    // it is ever read back (binning)
    if (int rc = ensure_div_tables(p, q, (hipStream_t)stream)) return rc;
    DivBinFuse f = make_fuse(p, q, n, S, C, 0, q->map_grid());
    int rc = qe_tt_pair_w(p, real_map0, real_map1, q->FG, q->FH, q->Fn, q->c[0], q->c[1], q->c[2], q->g[0], q->g[1], q->kk, q->kT, q->wl,
                          q->wk, q->rl, q->rk, q->mrow, q->map_grid(), pl, pk, (hipStream_t)stream, divbin_enabled(q) ? &f : nullptr,
                          fband_table(p, q, (hipStream_t)stream));
    if (rc > 0) return rc;
    if (rc == 0 && f.done) return 0;           // both maps binned and accumulated (map order) in the divergence launch
    if (rc < 0) {
        if ((rc = oa_qe_tt_moments(p, real_map0, n, S, C, stream))) return rc;
        return oa_qe_tt_moments(p, real_map1, n, S, C, stream);
    }
    // both kappa planes binned in one launch pair (grid y = map; kT sits one plane IN FRONT of kk: stride -1 plane), the moment
    // tail adds the two bandpower vectors in map order
    const long es = elem_bytes(p);
    const long back = ((const char*)q->kT - (const char*)q->kk) / es;
    return bin_power_moments(p->dtype, q->kk, q->norm, q->ids, (long)p->ny * p->kp, q->nids, p->kp, p->nx / 2, q->sums, q->counts_tmp,
                             q->bin_scratch, q->wk, q->rk, q->ticket, q->counts_full, n, S, C, (hipStream_t)stream, 2, back);
}

/* One stage of oa_qe_tt_moments on the plan's own work planes, for per-kernel timing (bench.py):
 * 0 = row R2C of the map, 1 = forward column pass 1, 2 = fused forward pass 2 + leg filters + inverse pass 1 and the
 * 3-plane inverse pass 2, 3 = fused row stage, 4 = 2-plane forward pass 1 + divergence kernel, 5 = binned power +
 * moment accumulation (into plan-owned dummies).  Stages read what the previous ones left in the work planes. */
int oa_qe_tt_stage(oa_plan* p, int stage, const void* real_map, void* stream) {
    OA_REQUIRE(p && p->pipe && ((Pipeline*)p->pipe)->FG, "oa_qe_tt_stage: call oa_plan_set_filters first");
    OA_NOT_MIXED(p, "oa_qe_tt_stage");
    Pipeline* q = (Pipeline*)p->pipe;
    const long pl = work_pitch(p, q->wl), pk = work_pitch(p, q->wk);
    hipStream_t st = (hipStream_t)stream;
    const int my = q->map_grid();
    const double s = 1.0 / ((double)p->ny * p->nx), sy = my ? (double)p->ny / my : 1.0;
    const int lr = qe_rsplit_lr(p, my, q->wl, q->wk, q->mrow);
    switch (stage) {
        case 0: case 1: case 2:
            OA_REQUIRE(real_map, "oa_qe_tt_stage: stages 0-2 need the map");
            return qe_map_legs_cols_w(p, real_map, q->FG, q->FH, q->c[0], q->c[1], q->c[2], q->wl, q->rl, pl, st, 1 << stage, my, lr,
                                      lr ? fband_table(p, q, st) : nullptr);
        case 3: return qe_rows_w(p, q->c[0], q->c[1], q->c[2], q->g[0], q->g[1], s * s * sy, 0, q->wl, q->wk, q->mrow, pl, pk, st, my, lr);
        case 4: {
            if (q->ids && divbin_enabled(q)) {      // as the one-call entries: binning + moments (into dummies) in the divergence launch
                DivBinFuse f = make_fuse(p, q, (int64_t*)q->kT, (double*)q->kT + 8, (double*)q->kT + 8 + q->nids, 0, my);
                return qe_cols_div_w(p, q->g[0], q->g[1], q->Fn, q->kk, 0, q->wk, q->rk, pk, st, my, &f);
            }
            return qe_cols_div_w(p, q->g[0], q->g[1], q->Fn, q->kk, 0, q->wk, q->rk, pk, st, my);
        }
        case 5: {
            OA_REQUIRE(q->ids, "oa_qe_tt_stage: stage 5 needs oa_plan_set_bins");
            if (oa_plan_div_fused(p)) return 0;    // nothing left to do: stage 4 binned
            // dummies: the tail of the (nids-long) sums / counts_tmp buffers is not large enough for C: use the kT plane
            int64_t* n = (int64_t*)q->kT;
            double* S = (double*)q->kT + 8;
            double* C = S + q->nids;
            return bandpower_moments(p, q, n, S, C, stream);
        }
        default: return fail("oa_qe_tt_stage: stage must be 0..5");
    }
}

}  // extern "C"

namespace oa {
static int ensure_mc_src(oa_plan* p, Pipeline* q, bool zero = false) { return q->mc_src.reserve((size_t)MC_BATCH_MAX * plane_bytes(p), zero); }
// pool bytes of a batch of B realisations: 3 B leg planes (gx_b, gy_b at 2b, 2b + 1; h_b at 2B + b) | 2 B product planes | 2 B pass-1 planes
static size_t mc_pool_bytes(const oa_plan* p, const Pipeline* q, int B) {
    const size_t es = elem_bytes(p);
    return 3 * (size_t)B * work_pitch(p, q->wl) * p->ny * es + 4 * (size_t)B * work_pitch(p, q->wk) * p->ny * es;
}
// B realisations through the bound (FG, FH) in one qe_legs_batch_w launch: its filter pointer table (FG x B, FH x B in q->mv_ftab, which the
// caller has allocated; uploaded when it differs from the table there) and its field selector
static int batch_filters(Pipeline* q, int B, hipStream_t st, unsigned long long* sel) {
    std::vector<const void*> key(2 * (size_t)B, q->FH);
    std::fill_n(key.begin(), B, q->FG);
    if (key != q->mv_fkey) {
        OA_HIP(hipMemcpyAsync(q->mv_ftab, key.data(), key.size() * sizeof(void*), hipMemcpyHostToDevice, st));
        q->mv_fkey = key;
    }
    *sel = 0;                                         // field f (gradient fields 0..B-1, H fields B..2B-1) reads source plane f mod B
    for (int f = 0; f < 2 * B; ++f) *sel |= (unsigned long long)(f % B) << (4 * f);
    return 0;
}
/* Everything behind the transforms of a BATCH of B realisations (q->mc_src: their hc planes, leg band filled): leg planes, row
 * stage, divergence, binned power + moments in realisation order, mean-field stack -- each ONE launch for the batch (oa_mc_run and,
 * behind its windowed front end, oa_mc_run_windowed).  *fallback = 1: this geometry's row stage takes one map per launch (nothing
 * was launched). */
static int mc_batch_tail(oa_plan* p, Pipeline* q, int B, int64_t* n, double* S, double* C, double* meanfield_acc, hipStream_t st, int* fallback,
                         bool keep_kappa = false) {     // keep_kappa: the kappa planes are stored (c[0] ...) even without a stack here
    *fallback = 0;
    const long pl = work_pitch(p, q->wl), pk = work_pitch(p, q->wk);
    const size_t es = elem_bytes(p);
    const size_t lb = (size_t)pl * p->ny * es, lbk = (size_t)pk * p->ny * es;
    const int my = q->my;
    if (int rc = ensure_pool(q, mc_pool_bytes(p, q, B))) return rc;
    char* const legs = q->split_legs.at();
    char* const prod = legs + 3 * (size_t)B * lb;
    char* const tmp = prod + 2 * (size_t)B * lbk;
    unsigned long long sel;
    if (!q->mv_ftab) OA_HIP(hipMalloc((void**)&q->mv_ftab, 32 * sizeof(void*)));
    if (int rc = batch_filters(q, B, st, &sel)) return rc;
    // (the row stage's geometry check first: nothing may have been launched when this batch falls back)
    const double s = 1.0 / ((double)p->ny * p->nx), sy = my ? (double)p->ny / my : 1.0;
    int legs_done = 0, rc;
    if ((rc = qe_legs_batch_w(p, q->mc_src.p, plane_elems(p), 0, sel, (const void* const*)q->mv_ftab, B, B, legs, (long)(lb / es), q->wl, q->rl,
                              pl, st, my, 4, &legs_done))) return rc;
    if (!legs_done && (rc = qe_legs_pass2_w(p, legs, 3 * B, (long)(lb / es), q->wl, pl, st, my))) return rc;
    rc = qe_rows_batch_w(p, legs, legs + lb, legs + 2 * (size_t)B * lb, prod, prod + lbk, s * s * sy, q->wl, q->wk, q->mrow, pl, pk, st, my, B,
                         (long)(2 * lb / es), (long)(lb / es), (long)(2 * lbk / es));
    if (rc < 0) { *fallback = 1; return 0; }          // this geometry's row stage takes one map per launch: one-by-one loop
    if (rc) return rc;
    if ((rc = ensure_div_tables(p, q, st))) return rc;
    DivBinFuse f = make_fuse(p, q, n, S, C, (meanfield_acc || keep_kappa) ? 1 : 0);
    if ((rc = qe_cols_div_batch_w(p, prod, prod + lbk, q->Fn, q->c[0], tmp, B, (long)(2 * lbk / es), 0, plane_elems(p), q->wk, q->rk, pk, st, my,
                                  divbin_enabled(q) ? &f : nullptr)))
        return rc;
    // binned power of the B kappa planes + their moment updates in realisation order: in the divergence launch, else two
    // launches; the mean-field stack: one
    if (!f.done && (rc = bin_power_moments(p->dtype, q->c[0], q->norm, q->ids, (long)p->ny * p->kp, q->nids, p->kp, p->nx / 2, q->sums, q->counts_tmp,
                                q->bin_scratch, q->wk, q->rk, q->ticket, q->counts_full, n, S, C, st, B, plane_elems(p)))) return rc;
    if (meanfield_acc && (rc = stack_add_region(p->dtype, q->c[0], meanfield_acc, p->ny, p->kp, q->wk, q->rk, st, B, 2 * plane_elems(p)))) return rc;
    return 0;
}

/* ---- BAND GRID: the one-call TT entries on map sides 2^a 3^b 5^c (include/orphics_amd.h) ---------------------------------------
 * Legs confined to columns < wl and rows |ky| < rl, kappa to columns < wk and rows |ky| < rk: on any (My, Mx) grid with
 * My >= max(2 rl + rk, 2 rk), Mx >= max(2 wl + wk, 2 wk) the estimator returns the same kappa modes as on the map's own (ny, nx) grid
 * (same ell lattice; a mode of signed index ky at row ky mod My), times (ny nx) / (My Mx): each inverse transform carries its own grid's
 * 1 / Npix and the forward transform sums over its own grid.  That factor is folded into the inner copy of Fnorm.  Mx >= 2 wk keeps
 * kappa's wk columns inside the inner plane's Mx / 2 + 1 (its Fnorm, bin ids and kappa_hat are stored there, as on a power-of-two
 * plan).  With My, Mx powers of two the inner computation IS the fused pipeline of a power-of-two plan fed with Fourier-space legs; only the input
 * transform (band_map_r2c), the GRF draw and the kappa scatter see the map's grid. */
constexpr int BAND_MIN = 128;                  // smallest inner side (the fused estimator kernels are exercised from 128 points up)
static int band_side(int mreq, long need, int side, const char* axis, int* out) {
    *out = 0;
    int m = mreq;
    if (m < 0) { m = BAND_MIN; while (m < need) m <<= 1; }
    else if (!is_pow2(m)) return fail(std::string("oa_plan_set_filters: band grid ") + axis + " must be a power of two");
    else if (m < need) return fail(std::string("oa_plan_set_filters: band grid ") + axis + " of " + std::to_string(m) + " points < " +
                                   std::to_string(need) + " would alias the leg products into the kept kappa modes");
    if (m >= side)
        return fail(std::string("oa_plan_set_filters: band too wide for the map: the band grid needs ") + std::to_string(m) + " points in " + axis +
                    " (alias-free bound " + std::to_string(need) + "), not fewer than the map's " + std::to_string(side) +
                    " -- no one-call path on this geometry (use the modular chain)");
    *out = m;
    return 0;
}
static int band_grid_rule(const oa_plan* p, int mrow, int mcol, int wl, int wk, int rl, int rk, int* my, int* mx) {
    *my = *mx = 0;
    if (mrow == 0 || mcol == 0)
        return fail("oa_plan_set_filters: sides that are not powers of two have no fused path on the map's own grid (mrow = 0 / column grid 0): "
                    "the one-call entries run on a band grid (mrow, column grid -1 or a power of two)");
    if (wl <= 0 || wk <= 0 || rl <= 0 || rk <= 0)
        return fail("oa_plan_set_filters: sides that are not powers of two need band-limited filters (leg / kappa columns and rows > 0; "
                    "0 = all has no band grid)");
    if (int rc = band_side(mrow, std::max(2L * wl + wk, 2L * wk), p->nx, "x", mx)) return rc;
    return band_side(mcol, std::max(2L * rl + rk, 2L * rk), p->ny, "y", my);
}
// an inner power-of-two plan of (my, mx) points on the ell lattice of p
static int band_inner_plan(const oa_plan* p, int my, int mx, oa_plan** out) {
    *out = nullptr;
    oa_plan* b = nullptr;
    if (int rc = oa_plan_create(my, mx, p->dtype, &b)) return rc;
    std::vector<double> ly(p->ny), lx(p->nx), bly(my), blx(mx);
    hipError_t e = hipMemcpy(ly.data(), p->ly64, p->ny * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(lx.data(), p->lx64, p->nx * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { (void)oa_plan_destroy(b); return fail(std::string("band grid: reading the ell axes: ") + hipGetErrorString(e)); }
    for (int i = 0; i < my; ++i) bly[i] = ly[i < my / 2 ? i : i - my + p->ny];    // the N grid's ell at the same signed index
    for (int i = 0; i < mx; ++i) blx[i] = lx[i < mx / 2 ? i : i - mx + p->nx];
    if (int rc = oa_plan_set_laxes(b, bly.data(), blx.data())) { (void)oa_plan_destroy(b); return rc; }
    *out = b;
    return 0;
}
static size_t band_real_bytes(const oa_plan* b) { return (size_t)b->ny * b->kp * (b->dtype == OA_F32 ? 4 : 8); }
// (re)make the band plan for the bound filters, copy the filters (and the bins) into its layout and bind them there.  Set-up call:
// synchronises the device (the caller's planes may have been written on any stream)
static int mixed_bind(oa_plan* p, Pipeline* q) {
    int my = 0, mx = 0;
    if (int rc = band_grid_rule(p, q->mrow, q->mcol, q->wl, q->wk, q->rl, q->rk, &my, &mx)) return rc;
    OA_HIP(hipDeviceSynchronize());
    if (!q->band || q->bmy != my || q->bmx != mx) {
        if (q->band) { (void)oa_plan_destroy(q->band); q->band = nullptr; }
        q->release_band();           // (bsplit, bwin: sized by the inner plane, retaken by the next call that needs them)
        q->bmy = q->bmx = 0;
        if (int rc = band_inner_plan(p, my, mx, &q->band)) return rc;
        if (int rc = q->bplanes.reserve(3 * band_real_bytes(q->band) + 2 * plane_bytes(q->band))) return rc;
        if (int rc = q->bids.reserve((size_t)my * q->band->kp * sizeof(int32_t))) return rc;
        q->bmy = my; q->bmx = mx;
        band_options(q);
    }
    oa_plan* b = q->band;
    const size_t rb = band_real_bytes(b);
    if (int rc = q->brows.reserve(band_map_scratch_bytes(p, q->wl, q->rl))) return rc;
    char* f = q->bplanes.at();
    OA_HIP(hipMemset(f, 0, 3 * rb + 2 * plane_bytes(b)));          // zero outside the bands (the input planes: only their band is written)
    const int kind = p->dtype == OA_F32 ? 0 : 1;
    const double fscale = (double)b->ny * b->nx / ((double)p->ny * p->nx);
    int rc = band_copy(kind, q->FG, p->kp, p->ny, f, b->kp, my, q->wl, q->rl, 1.0, nullptr);
    if (!rc) rc = band_copy(kind, q->FH, p->kp, p->ny, f + rb, b->kp, my, q->wl, q->rl, 1.0, nullptr);
    if (!rc) rc = band_copy(kind, q->Fn, p->kp, p->ny, f + 2 * rb, b->kp, my, q->wk, q->rk, fscale, nullptr);
    if (rc) return rc;
    OA_HIP(hipDeviceSynchronize());
    if (int rc2 = oa_plan_set_filters(b, f, f + rb, f + 2 * rb, q->wl, q->wk, q->rl, q->rk, -1)) return rc2;
    if (q->ids) {
        if (int rc2 = mixed_bins(p, q, nullptr)) return rc2;
        OA_HIP(hipDeviceSynchronize());
    }
    return 0;
}
// the bound bin ids in the band plan's layout; the band plan's mode counts are replaced by the WHOLE N-plane ones (a bandpower divides
// by the full grid's count).  Also takes the band plan's Monte-Carlo planes now (set-up time), zero-filled
static int mixed_bins(oa_plan* p, Pipeline* q, hipStream_t st) {
    oa_plan* b = q->band;
    OA_HIP(hipMemsetAsync(q->bids.p, 0xFF, (size_t)b->ny * b->kp * sizeof(int32_t), st));
    if (int rc = band_copy(2, q->ids, p->kp, p->ny, q->bids.p, b->kp, b->ny, q->wk, q->rk, 1.0, st)) return rc;
    if (int rc = oa_plan_set_bins(b, (const int32_t*)q->bids.p, q->nids, q->norm, st)) return rc;
    Pipeline* qb = (Pipeline*)b->pipe;
    OA_HIP(hipMemcpyAsync(qb->counts_full, q->counts_full, q->nids * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (int rc = ensure_mc_src(b, qb, true)) return rc;
    return ensure_pool(qb, mc_pool_bytes(b, qb, MC_BATCH_MAX));
}
static void* band_in(const Pipeline* q, int which) { return q->bplanes.at(3 * band_real_bytes(q->band) + which * plane_bytes(q->band)); }
static int band_cx_kind(const oa_plan* p) { return p->dtype == OA_F32 ? 3 : 4; }

// oa_qe_tt: input band -> band plan's fused pipeline (kappa on its plan-owned plane) -> scatter into the N-grid output
static int mixed_qe_tt(oa_plan* p, Pipeline* q, const void* map, const void* kX, const void* kY, void* out, int zero_outside, hipStream_t st) {
    oa_plan* b = q->band;
    void* bx = band_in(q, 0);
    void* by = nullptr;
    int rc;
    if (map) rc = band_map_r2c(p, map, q->brows.p, q->wl, q->rl, bx, b->ny, b->kp, st);
    else {
        rc = band_copy(band_cx_kind(p), kX, p->kp, p->ny, bx, b->kp, b->ny, q->wl, q->rl, 1.0, st);
        if (!rc && kY && kY != kX) { by = band_in(q, 1); rc = band_copy(band_cx_kind(p), kY, p->kp, p->ny, by, b->kp, b->ny, q->wl, q->rl, 1.0, st); }
    }
    if (rc) return rc;
    if ((rc = qe_tt_impl(b, nullptr, bx, by, nullptr, 0, st, nullptr))) return rc;
    void* o = out ? out : q->kk;
    if (out && zero_outside && (rc = band_zero_outside(p->dtype, o, p->ny, p->kp, q->wk, q->rk, st))) return rc;
    return band_copy(band_cx_kind(p), ((Pipeline*)b->pipe)->kk, b->kp, b->ny, o, p->kp, p->ny, q->wk, q->rk, 1.0, st);
}
// one Monte-Carlo step of a real map: input band, then oa_qe_tt_moments' sequence on the band plan (its bins carry the N-plane counts)
static int mixed_moments(oa_plan* p, Pipeline* q, const void* map, int64_t* n, double* S, double* C, hipStream_t st) {
    oa_plan* b = q->band;
    Pipeline* qb = (Pipeline*)b->pipe;
    band_options(q);
    void* bx = band_in(q, 0);
    if (int rc = band_map_r2c(p, map, q->brows.p, q->wl, q->rl, bx, b->ny, b->kp, st)) return rc;
    if (int rc = ensure_div_tables(b, qb, st)) return rc;
    DivBinFuse f = make_fuse(b, qb, n, S, C, 0);
    if (int rc = qe_tt_impl(b, nullptr, bx, nullptr, nullptr, 0, st, divbin_enabled(qb) ? &f : nullptr)) return rc;
    if (f.done) return 0;
    return bandpower_moments(b, qb, n, S, C, st);
}
/* ---- the shard loop of oa_mc_run / oa_mc_run_windowed, both plan kinds --------------------------------------------------------------
 * `grid` is the map's plan (Philox counters, the window and the mean-field stack are its), `run` the plan the estimator and the binning
 * run on: `grid` itself (power of two) or the inner plan of its band grid; `rq` is run's Pipeline.
 * BATCHES of realisations: at 4096^2 a realisation is ~60 MB of traffic behind ~10 launches, i.e. launch latency; with B realisations per
 * launch (grid z) the column and row stages fill the chip (OA_OPT_MC_BATCH 1 / 2 / 4 / 6 per launch at 4096^2: 16.5 / 26.0 / 37.6 / 40.3 k
 * realisations/s).  A batch of ONE goes through the same launches, so the moments do not depend on the batch size.  `source_batch(i, B)`
 * leaves the leg bands of realisations i .. i + B - 1 in run's mc_src, mc_batch_tail does the rest.  A geometry whose row stage takes one
 * map per launch reports `fallback` from its first batch, after the source stage and the leg launches (plan-owned planes only: harmless)
 * have run; the one-by-one loop then starts from the same i and draws that realisation again with the same counters.
 * ONE BY ONE: `source_one(i)` leaves realisation i in `one_map` (a real map; rows_done: its row transform on the plan's scratch plane
 * instead, qe_windowed_rows_w) or on the leg band of `one_k` (Fourier plane); then the estimator -- with `fuse`, binning + moments in the
 * divergence launch where the geometry has that kernel --, the bandpower moments, the stack. */
struct McTtLoop {
    oa_plan* grid; oa_plan* run; Pipeline* rq;
    bool batched;                                   // whether batching may start
    size_t pool_extra;                              // bytes per realisation of a batch behind the tail's region of run's pool
    std::function<int(long, int)> source_batch;
    std::function<int(long)> source_one;
    const void* one_map; const void* one_k; int rows_done; bool fuse;
    // oa_mc_run_rdn0: what stands in for mc_batch_tail (B realisations; *fallback as there) and for the estimator + binning of the
    // one-by-one loop; the sources then leave 2 B draws in run's rdn0_pool, not in mc_src
    std::function<int(int, int*)> tail_batch = nullptr;
    std::function<int()> tail_one = nullptr;
};
static int mc_tt_loop(const McTtLoop& T, long sim_lo, long sim_hi, int64_t* n, double* S, double* C, double* meanfield_acc, hipStream_t st) {
    oa_plan* const r = T.run;
    Pipeline* const rq = T.rq;
    const bool inner = T.grid != r;                 // the stack is grid's plane: kappa's band goes from the inner rows and pitch to the N grid's
    auto stack = [&](const void* kappa, int B, long stride) {
        if (!meanfield_acc) return 0;
        if (inner) return band_stack_add(T.grid->dtype, kappa, r->kp, r->ny, B, stride, meanfield_acc, T.grid->kp, T.grid->ny, rq->wk, rq->rk, st);
        // kappa_hat vanishes outside its active region (the plan-owned plane was zero-filled once): stack only that
        return stack_add_region(r->dtype, kappa, meanfield_acc, r->ny, r->kp, rq->wk, rq->rk, st);
    };
    const int BMAX = std::max(1, std::min(MC_BATCH_MAX, rq->opt_mc_batch));
    long i = sim_lo;
    bool batched = T.batched;
    while (batched && i < sim_hi) {
        const int B = (int)std::min<long>(BMAX, sim_hi - i);
        // before the first draw: growing either synchronises the device (a band plan's were taken by oa_plan_set_bins: no allocation here)
        if (!T.tail_batch)
            if (int rc = ensure_mc_src(r, rq)) return rc;
        if (int rc = ensure_pool(rq, mc_pool_bytes(r, rq, B) + (size_t)B * T.pool_extra)) return rc;
        int rc = T.source_batch(i, B), fallback = 0;
        if (rc) return rc;
        // the power-of-two plans' stack is added inside the tail, in the batch's launch; a band plan's from the kappa planes it keeps
        if ((rc = T.tail_batch ? T.tail_batch(B, &fallback)
                               : mc_batch_tail(r, rq, B, n, S, C, inner ? nullptr : meanfield_acc, st, &fallback, inner && meanfield_acc))) return rc;
        if (fallback) break;
        if (inner && (rc = stack(rq->c[0], B, plane_elems(r)))) return rc;
        i += B;
    }
    for (; i < sim_hi; ++i) {
        int rc = T.source_one(i);
        if (rc) return rc;
        if (T.tail_one) {
            if ((rc = T.tail_one())) return rc;
            continue;
        }
        DivBinFuse f = make_fuse(r, rq, n, S, C, meanfield_acc ? 1 : 0);     // (kappa_hat still stored when the stack needs it)
        if ((rc = qe_tt_impl(r, T.one_map, T.one_k, nullptr, nullptr, 0, st, T.fuse && divbin_enabled(rq) ? &f : nullptr, T.rows_done))) return rc;
        if (!f.done && (rc = bandpower_moments(r, rq, n, S, C, st))) return rc;
        if ((rc = stack(rq->kk, 1, 0))) return rc;
    }
    return 0;
}
// oa_mc_run on a band grid: the leg band of each realisation's N-grid draw straight into the band plan's layout
static int mixed_mc_run(oa_plan* p, Pipeline* q, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, int64_t* n, double* S,
                        double* C, double* meanfield_acc, hipStream_t st) {
    oa_plan* b = q->band;
    Pipeline* qb = (Pipeline*)b->pipe;
    band_options(q);
    void* const bx = band_in(q, 0);
    McTtLoop T{p, b, qb, true, 0, nullptr, nullptr, nullptr, bx, 0, false};
    T.source_batch = [=](long i, int B) { return grf_band_inner(p, base_seed, (uint64_t)i, B, covsqrt_hc, qb->mc_src.p, b->ny, b->kp, plane_elems(b), q->wl, q->rl, st); };
    T.source_one = [=](long i) { return grf_band_inner(p, base_seed, (uint64_t)i, 1, covsqrt_hc, bx, b->ny, b->kp, 0, q->wl, q->rl, st); };
    return mc_tt_loop(T, sim_lo, sim_hi, n, S, C, meanfield_acc, st);
}
/* ---- WINDOWED TT DRAWS: the source stage of oa_mc_run_windowed (realisation i = Philox stream i) and of oa_mc_run_rdn0_windowed (s, s' of
 * realisation i = streams 2 i, 2 i + 1).  A draw is the full-plane draw of its stream on the map's grid (oa_grf_hc: key (seed, stream), the
 * counters of every other draw) -> C2R / Npix -> x window -> R2C, of which only the leg band is kept, on a plane of the plan the estimator
 * runs on.  FUSED (one method per plan kind, `nd` consecutive streams onto planes a fixed stride apart, the full-plane part in groups of
 * at most MC_BATCH_MAX = the work planes there are): the real map exists in LDS only.
 *   band():  per draw oa_grf_hc into an N-grid plane of bwin + its inverse column transform in place (mixed_cols_inverse); per group ONE
 *     fused row launch (C2R x window -> R2C, columns < wl stored: band_rows_win_kernel) and the pruned column DFT onto the inner planes
 *     (band_win_r2c).  band_open() first: it owns bwin and the fused / unfused rule.
 *   pow2():  on c[0..2], g[0..1], kT, the plan's six contiguous work planes, free until the tail -- dfused: ONE inverse pass-1 launch that
 *     evaluates the group's draws at its load + the in-place pass 2 (oa_grf_hc_icols), then ONE fused row launch (grid y = draw); else per
 *     draw oa_grf_hc into kT, inverse columns into c[0], the fused row pass -- onto compact row planes at `rowT` (the caller's place in the
 *     pool); then per group ONE forward column transform onto the leg band of the destination planes.
 * UNFUSED (band_map(), pow2_map(): one draw): oa_grf_hc -> C2R with the window at the row store -> real map in HBM -> its transform. */
// the default of OA_OPT_DRAW_FUSED: oa_grf_hc_icols alone measured 5 - 14 us per plane below oa_grf_hc + oa_fft_cols, beyond both 10th - 90th
// spreads at every measured geometry (profiles/rdn0_windowed.jsonl); the 0 arm is also one by one, so a realisation differs by more
constexpr bool DRAW_FUSED_DEFAULT = true;
struct WinDraws {
    oa_plan* p; Pipeline* q; uint64_t seed; const void* cs; const void* window; hipStream_t st;
    bool fused = false, dfused = false;             // the fused row pass; the draw inside the column pass (pow2() only)
    double inv() const { return 1.0 / ((double)p->ny * p->nx); }
    char* rows() const { return q->bwin.at((size_t)MC_BATCH_MAX * plane_bytes(p)); }      // bwin: MC_BATCH_MAX N-grid planes | row scratch

    int band_open() {
        // entry-owned planes, taken on the first windowed call of either entry (and regrown when the band widens): that call synchronises
        // the device once
        if (int rc = q->bwin.reserve((size_t)MC_BATCH_MAX * plane_bytes(p) + std::max(band_maps_scratch_bytes(p, MC_BATCH_MAX, q->wl, q->rl),
                                                                                     band_map_scratch_bytes(p, q->wl, q->rl)))) return rc;
        // fused row pass or the unfused flow: the caller's OA_OPT_WIN_FUSED; until it is set, what measured faster (DESIGN 5a,
        // profiles/band_grid_windowed.jsonl): the unfused flow at 1200^2 (by 1 % f32, 5 % f64), the fused pass at 2400^2 (by up to 1 %)
        // (rows the fused kernel does not hold -- more than 8192 points -- take the unfused flow, whose row passes have an in-place form)
        fused = q->opt_win_fused_set ? q->opt_win_fused : (p->nx > 1200 && band_rows_win_ok(p));
        return 0;
    }
    // `single` (nd = 1): band_win_r2c's column kernels of one map
    int band(uint64_t s0, int nd, void* dst, long dstride, int single = 0) const {
        const oa_plan* b = q->band;
        const size_t pb = plane_bytes(p);
        char* const full = q->bwin.at();
        for (int z0 = 0; z0 < nd; z0 += MC_BATCH_MAX) {
            const int nz = std::min(MC_BATCH_MAX, nd - z0);
            for (int k = 0; k < nz; ++k) {
                void* pl = full + (size_t)k * pb;
                if (int rc = oa_grf_hc(p, seed, s0 + (uint64_t)(z0 + k), cs, pl, st)) return rc;
                if (int rc = mixed_cols_inverse(p, pl, pl, st)) return rc;
            }
            if (int rc = band_win_r2c(p, nz, full, plane_elems(p), window, inv(), rows(), single, q->wl, q->rl, nullptr, nullptr,
                                      (char*)dst + (size_t)z0 * dstride * elem_bytes(b), dstride, b->ny, b->kp, st)) return rc;
        }
        return 0;
    }
    int band_map(uint64_t s, void* dst) const {
        char* const full = q->bwin.at();
        void* tmap = full + plane_bytes(p);                                      // ny x nx reals fit an hc plane
        if (int rc = oa_grf_hc(p, seed, s, cs, full, st)) return rc;
        if (int rc = oa_fft_c2r_windowed(p, full, tmap, inv(), window, st)) return rc;
        return band_map_r2c(p, tmap, rows(), q->wl, q->rl, dst, q->band->ny, q->band->kp, st);
    }
    // dst = nullptr (one draw, not dfused): no Fourier plane -- the row transform stays on the plan's scratch plane, for qe_tt_impl(rows_done)
    int pow2(uint64_t s0, int nd, char* rowT, void* dst) const {
        const long pl = work_pitch(p, q->wl), pe = plane_elems(p);
        const size_t es = elem_bytes(p), lb = (size_t)pl * p->ny * es;
        char* const full = (char*)q->c[0];
        for (int z0 = 0; z0 < nd; z0 += MC_BATCH_MAX) {
            const int nz = std::min(MC_BATCH_MAX, nd - z0);
            if (dfused) {
                if (int rc = grf_icols_w(p, seed, s0 + (uint64_t)z0, nz, cs, full, pe, st)) return rc;
                if (int rc = qe_win_rows_w(p, full, window, q->wl, pl, inv(), st, rowT + (size_t)z0 * lb, nz, pe, (long)(lb / es))) return rc;
            } else {
                for (int k = 0; k < nz; ++k) {
                    if (int rc = oa_grf_hc(p, seed, s0 + (uint64_t)(z0 + k), cs, q->kT, st)) return rc;
                    if (int rc = qe_windowed_rows_w(p, q->kT, full, window, q->wl, pl, inv(), st, dst ? rowT + (size_t)(z0 + k) * lb : nullptr)) return rc;
                }
            }
            if (!dst) continue;
            if (int rc = qe_fwd_cols_batch_w(p, rowT + (size_t)z0 * lb, pl, (char*)dst + (size_t)z0 * pe * es, nz, (long)(lb / es), pe, q->wl, q->rl, st))
                return rc;
        }
        return 0;
    }
    // dst = nullptr: the real map stays in c[0] (the first leg plane, which the from-map estimator overwrites only after its row pass)
    int pow2_map(uint64_t s, void* dst) const {
        if (int rc = oa_grf_hc(p, seed, s, cs, q->kT, st)) return rc;
        if (int rc = oa_fft_c2r_windowed(p, q->kT, q->c[0], inv(), window, st)) return rc;
        return dst ? oa_fft_r2c(p, q->c[0], dst, 1.0, q->wl, q->rl, st) : 0;
    }
};
// oa_mc_run_windowed on a band grid: WinDraws::band onto the band plan's source planes, batched where the row pass is fused
static int mixed_mc_run_windowed(oa_plan* p, Pipeline* q, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, const void* window,
                                 int64_t* n, double* S, double* C, double* meanfield_acc, hipStream_t st) {
    oa_plan* b = q->band;
    Pipeline* qb = (Pipeline*)b->pipe;
    band_options(q);
    WinDraws W{p, q, base_seed, covsqrt_hc, window, st};
    if (int rc = W.band_open()) return rc;
    void* const bx = band_in(q, 0);
    // (an inner plan whose row stage takes one map per launch -- row grids below 1024 points -- abandons its first batch of every call
    // after the front end has run: about 1 % of a 300-realisation call)
    McTtLoop T{p, b, qb, W.fused, 0, nullptr, nullptr, nullptr, bx, 0, false};
    T.source_batch = [=](long i, int B) { return W.band((uint64_t)i, B, qb->mc_src.p, plane_elems(b)); };
    T.source_one = [=](long i) { return W.fused ? W.band((uint64_t)i, 1, bx, 0, 1) : W.band_map((uint64_t)i, bx); };
    return mc_tt_loop(T, sim_lo, sim_hi, n, S, C, meanfield_acc, st);
}
/* ---- oa_rdn0_set_data / oa_mc_run_rdn0: the realisation-dependent N0 shard (include/orphics_amd.h) ------------------------------------
 * Realisation i pairs the data d with the draws s (Philox stream 2 i) and s' (stream 2 i + 1) through the two legs of the TT estimator:
 *     A = QE(d, s) + QE(s, d),   B = QE(s, s') + QE(s', s)       (QE(X, Y): gradient leg from X, the other from Y).
 * The real-space products are linear in the pieces, so A and B are two-piece estimators over the sources d, s, s' in oa_qe_mv's sense:
 * (gx_d, gy_d, h_s) + (gx_s, gy_s, h_d) and (gx_s, gy_s, h_s') + (gx_s', gy_s', h_s), one divergence each.  d's three leg planes never
 * change: oa_rdn0_set_data makes them once (rdn0_legs).  `r` is the plan the estimator runs on -- the map's plan, or the inner plan of
 * its band grid -- and `rq` its Pipeline.  PER BATCH of B realisations (r's pool: 6 B leg planes | 4 B product planes | 4 B pass-1 planes;
 * rdn0_pool: the 2 B draws, draw z = stream 2 i + z | the 2 B kappa planes, A_b and B_b at 2 b, 2 b + 1 | the tail's partials):
 *   1 draw launch (2 B leg bands)  ->  2 leg launches (B gradient + B H fields each: the selector holds 16 fields) [+ 1 inverse pass 2 over
 *   the 6 B planes where the leg kernel is not single-pass]  ->  1 chain row-stage launch (2 B estimators of two pieces)  ->  the batched
 *   divergence of 2 B planes  ->  the tail's 2 launches (rdn0.hpp).
 * ONE BY ONE, where the row stage takes one map per launch (rdn0_one): 1 draw launch (2 planes), 2 leg-stage calls, 4 row-stage launches
 * (the second piece of an estimator accumulates), 2 divergences, the same tail with B = 1. */
static size_t rdn0_pool_bytes(const oa_plan* r, const Pipeline* rq) {
    return 4 * (size_t)MC_BATCH_MAX * plane_bytes(r) + rdn0_part_bytes(r->ny, rq->rk, rq->nids, MC_BATCH_MAX);
}
// everything a shard needs beyond the data legs; allocates (and synchronises) only when something is missing or too small
static int rdn0_reserve(oa_plan* r, Pipeline* rq) {
    if (int rc = ensure_work(r, rq)) return rc;
    if (int rc = rq->rdn0_pool.reserve(rdn0_pool_bytes(r, rq), true)) return rc;          // draws and kappa planes: only their band is ever written
    if (int rc = ensure_pool(rq, 2 * mc_pool_bytes(r, rq, MC_BATCH_MAX))) return rc;
    if (!rq->mv_ftab) OA_HIP(hipMalloc((void**)&rq->mv_ftab, 32 * sizeof(void*)));
    if (!rq->mv_rtab) OA_HIP(hipMalloc(&rq->mv_rtab, 64 * 64 + 1024));
    return 0;
}
struct Rdn0Planes {                       // where a batch of B lives
    char *legs, *prod, *tmp, *draw, *kappa; double* part; const char* data;
    size_t lb, lbk, pb;
};
static Rdn0Planes rdn0_planes(const oa_plan* r, const Pipeline* rq, int B) {
    Rdn0Planes P;
    const size_t es = elem_bytes(r);
    P.lb = (size_t)work_pitch(r, rq->wl) * r->ny * es; P.lbk = (size_t)work_pitch(r, rq->wk) * r->ny * es; P.pb = plane_bytes(r);
    P.legs = rq->split_legs.at(); P.prod = P.legs + 6 * (size_t)B * P.lb; P.tmp = P.prod + 4 * (size_t)B * P.lbk;
    P.draw = rq->rdn0_pool.at(); P.kappa = P.draw + 2 * (size_t)MC_BATCH_MAX * P.pb; P.part = (double*)(P.kappa + 2 * (size_t)MC_BATCH_MAX * P.pb);
    P.data = rq->rdn0_legs.at();
    return P;
}
static int rdn0_tail_of(oa_plan* r, Pipeline* rq, const Rdn0Planes& P, int B, int64_t* n, double* S, double* C, hipStream_t st) {
    return rdn0_tail(r->dtype, P.kappa, plane_elems(r), B, r->ny, r->kp, r->nx / 2, rq->ids, rq->nids, rq->norm, rq->wk, rq->rk, rq->counts_full, P.part,
                     n, S, C, st);
}
static int rdn0_batch(oa_plan* r, Pipeline* rq, int B, int64_t* n, double* S, double* C, hipStream_t st, int* fallback) {
    *fallback = 0;
    const Rdn0Planes P = rdn0_planes(r, rq, B);
    const long pl = work_pitch(r, rq->wl), pk = work_pitch(r, rq->wk);
    const size_t es = elem_bytes(r), lb = P.lb, lbk = P.lbk;
    const int my = rq->my;
    unsigned long long sel;                           // (the table itself is rdn0_reserve's)
    int legs_done = 0, rc;
    if ((rc = batch_filters(rq, B, st, &sel))) return rc;
    for (int c = 0; c < 2; ++c)                      // draws [c B, (c + 1) B) -> leg planes [3 c B, 3 (c + 1) B): gx, gy of draw z' at 2 z', 2 z' + 1, h at 2 B + z'
        if ((rc = qe_legs_batch_w(r, P.draw + (size_t)c * B * P.pb, plane_elems(r), 0, sel, (const void* const*)rq->mv_ftab, B, B,
                                  P.legs + 3 * (size_t)c * B * lb, (long)(lb / es), rq->wl, rq->rl, pl, st, my, 4, &legs_done))) return rc;
    if (!legs_done && (rc = qe_legs_pass2_w(r, P.legs, 6 * B, (long)(lb / es), rq->wl, pl, st, my))) return rc;
    auto gx = [&](int z) { return (const void*)(P.legs + (3 * (size_t)(z / B) * B + 2 * (size_t)(z % B)) * lb); };
    auto hh = [&](int z) { return (const void*)(P.legs + (3 * (size_t)(z / B) * B + 2 * (size_t)B + (size_t)(z % B)) * lb); };
    const double s = 1.0 / ((double)r->ny * r->nx), sy = my ? (double)r->ny / my : 1.0;
    std::vector<const void*> cgx, cgy, chh;
    std::vector<void*> cpx, cpy;
    std::vector<double> csc(4 * B, s * s * sy);
    std::vector<int> first(2 * B), cnt(2 * B, 2);
    for (int b = 0; b < B; ++b) {
        const int zs = 2 * b, zt = 2 * b + 1;         // s, s'
        const void* const pg[4] = {P.data, gx(zs), gx(zs), gx(zt)};                 // A: (d, s) + (s, d);  B: (s, s') + (s', s)
        const void* const ph[4] = {hh(zs), P.data + 2 * lb, hh(zt), hh(zs)};
        for (int k = 0; k < 4; ++k) {
            const int e = 2 * b + k / 2;
            if (k % 2 == 0) first[e] = (int)cgx.size();
            cgx.push_back(pg[k]); cgy.push_back((const char*)pg[k] + lb); chh.push_back(ph[k]);
            cpx.push_back(P.prod + 2 * (size_t)e * lbk); cpy.push_back(P.prod + (2 * (size_t)e + 1) * lbk);
        }
    }
    std::vector<unsigned long long> key;
    for (size_t i = 0; i < cgx.size(); ++i)
        key.insert(key.end(), {(unsigned long long)(uintptr_t)cgx[i], (unsigned long long)(uintptr_t)chh[i], (unsigned long long)(uintptr_t)cpx[i]});
    unsigned long long bits;
    memcpy(&bits, &csc[0], sizeof bits);
    key.insert(key.end(), {bits, (unsigned long long)my, (unsigned long long)(unsigned)rq->mrow, (unsigned long long)r->dtype, 0x4D01ull});
    rc = qe_rows_chain_w(r, 2 * B, 4 * B, cgx.data(), cgy.data(), chh.data(), cpx.data(), cpy.data(), csc.data(), first.data(), cnt.data(), rq->mv_rtab,
                         key != rq->mv_rkey, rq->wl, rq->wk, rq->mrow, pl, pk, st, my);
    if (rc < 0) { *fallback = 1; return 0; }          // this geometry's row stage takes one map per launch: one-by-one loop
    if (rc) return rc;
    rq->mv_rkey = key;
    if ((rc = qe_cols_div_batch_w(r, P.prod, P.prod + lbk, rq->Fn, P.kappa, P.tmp, 2 * B, (long)(2 * lbk / es), 0, plane_elems(r), rq->wk, rq->rk, pk,
                                  st, my))) return rc;
    return rdn0_tail_of(r, rq, P, B, n, S, C, st);
}
// one realisation whose draws s, s' sit on the first two planes of rdn0_pool
static int rdn0_one(oa_plan* r, Pipeline* rq, int64_t* n, double* S, double* C, hipStream_t st) {
    const Rdn0Planes P = rdn0_planes(r, rq, 1);
    const long pl = work_pitch(r, rq->wl), pk = work_pitch(r, rq->wk);
    const size_t lb = P.lb;
    const int my = rq->my;
    char* const L = P.legs;                           // gx, gy, h of s, then of s'
    int rc;
    for (int z = 0; z < 2; ++z)
        if ((rc = qe_legs_cols_w(r, P.draw + (size_t)z * P.pb, P.draw + (size_t)z * P.pb, rq->FG, rq->FH, L + 3 * (size_t)z * lb, L + (3 * (size_t)z + 1) * lb,
                                 L + (3 * (size_t)z + 2) * lb, rq->wl, rq->rl, pl, st, my))) return rc;
    const double s = 1.0 / ((double)r->ny * r->nx), sy = my ? (double)r->ny / my : 1.0, sc = s * s * sy;
    const void* const pg[4] = {P.data, L, L, L + 3 * lb};
    const void* const ph[4] = {L + 2 * lb, P.data + 2 * lb, L + 5 * lb, L + 2 * lb};
    for (int e = 0; e < 2; ++e) {
        for (int k = 0; k < 2; ++k)
            if ((rc = qe_rows_w(r, pg[2 * e + k], (const char*)pg[2 * e + k] + lb, ph[2 * e + k], rq->g[0], rq->g[1], sc, k, rq->wl, rq->wk, rq->mrow, pl, pk,
                                st, my))) return rc;
        if ((rc = qe_cols_div_w(r, rq->g[0], rq->g[1], rq->Fn, P.kappa + (size_t)e * P.pb, 0, rq->wk, rq->rk, pk, st, my))) return rc;
    }
    return rdn0_tail_of(r, rq, P, 1, n, S, C, st);
}
static const char* const RDN0_HOW = "run the host loop of the existing entries (mc.RDN0MonteCarlo with one_call=False)";
/* The opening of entry `who` (oa_mc_run_rdn0, oa_mc_run_rdn0_windowed): every refusal -- `refuse`, where not NULL, is the entry's own, said
 * right after the argument check --, then the plan the estimator runs on and its planes (rdn0_reserve: nothing to do after the first call, or
 * after oa_rdn0_set_data with bins bound), and *T = a batched McTtLoop on that plan with rdn0_batch / rdn0_one as its tail; the entry adds
 * its source stage.  Nothing has been launched when it refuses. */
static int rdn0_tt_open(const char* who, const char* refuse, oa_plan* p, long sim_lo, long sim_hi, const void* covsqrt_hc, int64_t* n, double* S,
                        double* C, hipStream_t st, McTtLoop* T) {
    auto msg = [who](const char* what, bool how = true) { return std::string(who) + ": " + what + (how ? std::string("; or ") + RDN0_HOW : ""); };
    OA_REQUIRE(p && covsqrt_hc && n && S && C && sim_hi >= sim_lo, msg("bad argument", false));
    OA_REQUIRE(!refuse, msg(refuse, false));
    OA_REQUIRE(p->pow2 || p->mixed, msg("map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path"));
    OA_REQUIRE(p->pipe && ((Pipeline*)p->pipe)->FG, msg("no filters bound: call oa_plan_set_filters, oa_plan_set_bins and oa_rdn0_set_data first"));
    Pipeline* q = (Pipeline*)p->pipe;
    OA_REQUIRE(q->ids, msg("no bins bound: call oa_plan_set_bins, then oa_rdn0_set_data"));
    OA_REQUIRE(!p->mixed || (q->band && q->band->pipe), msg("the bound filters have no band grid on this plan (oa_plan_set_filters reports why)"));
    oa_plan* r = p->mixed ? q->band : p;
    Pipeline* rq = (Pipeline*)r->pipe;
    OA_REQUIRE(q->rdn0_gen, msg("no data set: call oa_rdn0_set_data (after oa_plan_set_filters and oa_plan_set_bins)"));
    OA_REQUIRE(q->rdn0_gen == q->bind_gen && q->rdn0_my == rq->my && rq->rdn0_legs.p,
               msg("the data legs are stale -- oa_plan_set_filters, oa_plan_set_bins or oa_plan_set_col_grid was called since they were made: "
                   "call oa_rdn0_set_data again"));
    if (int rc = rdn0_tail_check(who, rq->nids, MC_BATCH_MAX)) return rc;
    if (p->mixed) band_options(q);
    if (int rc = rdn0_reserve(r, rq)) return rc;
    *T = McTtLoop{p, r, rq, true, mc_pool_bytes(r, rq, 1), nullptr, nullptr, nullptr, nullptr, 0, false};
    q->rdn0_ran_batched = 0;
    T->tail_batch = [=](int B, int* fallback) {
        const int rc = rdn0_batch(r, rq, B, n, S, C, st, fallback);
        if (!rc && !*fallback) q->rdn0_ran_batched = 1;
        return rc;
    };
    T->tail_one = [=]() { return rdn0_one(r, rq, n, S, C, st); };
    return 0;
}
/* ---- oa_qe_pol / oa_qe_mv on the band grid -------------------------------------------------------------------------------------------
 * These entries take their filter planes per call, so the inner-layout copies are made by a set-up entry (oa_qe_band_bind, which may
 * allocate and synchronise) and a call only looks its pointers up: ONE inner plane per distinct N-grid plane, so that the inner
 * oa_qe_mv's sharing of leg transforms by (source, filter) address is the caller's; the normalisation planes stacked in the bound
 * order, so that a call that passes them in that order keeps the one-launch divergence.  A call embeds its distinct source transforms
 * in one launch, runs the inner oa_qe_pol / oa_qe_mv into the inner plan's kappa plane and scatters kappa's band back: no allocation,
 * no synchronisation (pool, tables and column-grid twiddles of the inner plan are taken at set-up). */
static int pol_bind(oa_plan* p, Pipeline* q, int nf, const void* const* filters, int nn, const void* const* norms, int wl, int wk, int rl, int rk,
                    int mrow, int mcol, int max_leg_planes) {
    Pipeline::PolBind& B = q->pb;
    B.bound = false;
    ++B.gen;
    B.mc.bound = false;                             // the Monte-Carlo binding belongs to the binding it was made on
    int my = 0, mx = 0;
    if (int rc = band_grid_rule(p, mrow, mcol, wl, wk, rl, rk, &my, &mx)) return rc;
    OA_HIP(hipDeviceSynchronize());                 // the caller's planes may have been written on any stream; the old copies may be in use
    if (!B.plan || B.my != my || B.mx != mx) {
        if (B.plan) { (void)oa_plan_destroy(B.plan); B.plan = nullptr; }
        B.mrows.release();                          // (the from-maps calls' scratch: retaken on demand)
        B.mwin.release();                           // (the windowed Monte Carlo's planes: likewise)
        B.my = B.mx = 0;
        if (int rc = band_inner_plan(p, my, mx, &B.plan)) return rc;
        B.my = my; B.mx = mx;
    }
    oa_plan* b = B.plan;
    Pipeline* qb = pipe_of(b);
    band_options(q);
    const size_t rb = band_real_bytes(b), cb = plane_bytes(b), need = (size_t)(nf + nn) * rb + (size_t)POL_SRC_MAX * cb;
    if (int rc = B.planes.reserve(need)) return rc;
    OA_HIP(hipMemset(B.planes.p, 0, need));         // zero outside the bands (source planes: only their band is ever written)
    if (int rc = B.stab.reserve(POL_SRC_MAX * sizeof(void*))) return rc;
    B.skey.clear();
    const int kind = p->dtype == OA_F32 ? 0 : 1;
    const double fscale = (double)b->ny * b->nx / ((double)p->ny * p->nx);
    char* f = B.planes.at();
    for (int i = 0; i < nf; ++i)
        if (int rc = band_copy(kind, filters[i], p->kp, p->ny, f + (size_t)i * rb, b->kp, my, wl, rl, 1.0, nullptr)) return rc;
    for (int i = 0; i < nn; ++i)
        if (int rc = band_copy(kind, norms[i], p->kp, p->ny, f + (size_t)(nf + i) * rb, b->kp, my, wk, rk, fscale, nullptr)) return rc;
    // everything the inner entries would otherwise take on first use
    if (int rc = ensure_work(b, qb)) return rc;
    const size_t es = elem_bytes(b);
    const size_t lb = (size_t)work_pitch(b, wl) * b->ny * es, lbk = (size_t)work_pitch(b, wk) * b->ny * es;
    if (int rc = ensure_pool(qb, (size_t)(max_leg_planes > 0 ? max_leg_planes : 3 * nf) * lb + 4 * (size_t)nn * lbk)) return rc;
    if (!qb->mv_ftab) OA_HIP(hipMalloc((void**)&qb->mv_ftab, 32 * sizeof(void*)));
    if (!qb->mv_rtab) OA_HIP(hipMalloc(&qb->mv_rtab, 64 * 64 + 1024));
    int imy = 0;
    if (int rc = resolve_my(b, qb->mcol, rl, rk, &imy)) return rc;      // (an explicit grid above the automatic one: the inner column grid's table)
    OA_HIP(hipDeviceSynchronize());
    B.fkey.assign(filters, filters + nf);
    B.nkey.assign(norms, norms + nn);
    B.wl = wl; B.wk = wk; B.rl = rl; B.rk = rk; B.mrow = mrow;
    B.bound = true;
    return 0;
}
static void* pol_inner(const std::vector<const void*>& key, const void* ptr, char* base, size_t stride) {
    for (size_t i = 0; i < key.size(); ++i) if (key[i] == ptr) return base + i * stride;
    return nullptr;
}
// SOURCE STAGE of oa_qe_pol / oa_qe_mv: the leg band of the distinct N-grid source transforms -> the inner source planes, one launch
// through the device table (re-uploaded only when the caller's pointers change)
static int mv_sources_embed(oa_plan* p, Pipeline::PolBind& B, const std::vector<const void*>& srcs, char* sbase, size_t cb, int wl, int rl,
                            hipStream_t st) {
    const oa_plan* b = B.plan;
    if (srcs != B.skey) {                             // (pageable source: staged before the call returns; ordered on this stream)
        OA_HIP(hipMemcpyAsync(B.stab.p, srcs.data(), srcs.size() * sizeof(void*), hipMemcpyHostToDevice, st));
        B.skey = srcs;
    }
    return band_embed(p->dtype, (const void* const*)B.stab.p, (int)srcs.size(), p->kp, p->ny, sbase, plane_elems(b), b->kp, b->ny, wl, rl, st);
}
// SOURCE STAGE of oa_qe_mv_maps: the batched band input transform of the call's real maps (with the Q,U -> E,B rotation) straight into
// the inner source planes -- no N-grid hc plane, no embed, no device table.  The map-side scratch belongs to the binding: taken on the
// first from-maps call and regrown when a call brings more maps or a wider band than any before (that call synchronises the device
// once); later calls neither allocate nor synchronise
static int mv_sources_maps(oa_plan* p, Pipeline::PolBind& B, const MvCall& c, char* sbase, size_t cb, int wl, int rl, hipStream_t st) {
    const oa_plan* b = B.plan;
    if (int rc = B.mrows.reserve(band_maps_scratch_bytes(p, c.nmaps, wl, rl))) return rc;
    return band_maps_r2c(p, c.nmaps, c.maps, c.rot_c, c.rot_s, B.mrows.p, wl, rl, sbase, plane_elems(b), b->ny, b->kp, st);
}
static int mixed_qe_mv(oa_plan* p, Pipeline* q, const MvCall& c, void* out, int accumulate, int wl, int wk, int rl, int rk, int mrow, int zero_outside,
                       hipStream_t st) {
    const bool from_maps = c.nmaps > 0;
    const char* who = from_maps ? "oa_qe_mv_maps" : (c.pol ? "oa_qe_pol" : "oa_qe_mv");
    Pipeline::PolBind& B = q->pb;
    if (!B.bound)
        return fail(std::string(who) + ": on map sides that are not powers of two the filter and normalisation planes are bound first (oa_qe_band_bind)");
    if (wl != B.wl || wk != B.wk || rl != B.rl || rk != B.rk || mrow != B.mrow)
        return fail(std::string(who) + ": leg / kappa columns and rows or the row grid differ from the bound ones (call oa_qe_band_bind for this band)");
    oa_plan* b = B.plan;
    Pipeline* qb = (Pipeline*)b->pipe;
    band_options(q);
    const size_t rb = band_real_bytes(b), cb = plane_bytes(b), es = elem_bytes(b);
    char* const fbase = B.planes.at();
    char* const nbase = fbase + B.fkey.size() * rb;
    char* const sbase = nbase + B.nkey.size() * rb;
    int total = 0;
    for (int e = 0; e < c.nest; ++e) {
        OA_REQUIRE(c.npieces[e] >= 1 && (from_maps || (c.kX[e] && c.kY[e])) && c.Fn[e], "oa_qe_mv: bad estimator entry");
        total += c.npieces[e];
    }
    std::vector<const void*> iFG(total), iFH(total), iFn(c.nest), ikX(c.nest), ikY(c.nest), srcs;
    for (int i = 0; i < total; ++i) {
        iFG[i] = pol_inner(B.fkey, c.FG[i], fbase, rb);
        iFH[i] = pol_inner(B.fkey, c.FH[i], fbase, rb);
        if (!iFG[i] || !iFH[i]) return fail(std::string(who) + ": a filter plane of this call is not bound (oa_qe_band_bind binds every distinct plane)");
    }
    auto source = [&](const void* s) {
        size_t k = 0;
        while (k < srcs.size() && srcs[k] != s) ++k;
        if (k == srcs.size()) srcs.push_back(s);
        return (const void*)(sbase + k * cb);
    };
    for (int e = 0; e < c.nest; ++e) {
        iFn[e] = pol_inner(B.nkey, c.Fn[e], nbase, rb);
        if (!iFn[e]) return fail(std::string(who) + ": a normalisation plane of this call is not bound (oa_qe_band_bind)");
        if (from_maps) {                              // source i IS map i (checked by the entry: 0 <= index < nmaps <= 6)
            ikX[e] = sbase + (size_t)c.xsrc[e] * cb;
            ikY[e] = sbase + (size_t)c.ysrc[e] * cb;
        } else {
            ikX[e] = source(c.kX[e]);
            ikY[e] = source(c.kY[e]);
        }
    }
    if ((int)srcs.size() > POL_SRC_MAX) return fail(std::string(who) + ": more than 6 distinct source transforms in one call on a band grid");
    if (!c.pol) {                                     // the inner entry's pool: sized by oa_qe_band_bind, never grown here
        std::vector<std::pair<const void*, const void*>> grad, hpl;
        auto add = [](std::vector<std::pair<const void*, const void*>>& v, const void* s, const void* f) {
            for (auto& k : v) if (k.first == s && k.second == f) return;
            v.emplace_back(s, f);
        };
        int at = 0;
        for (int e = 0; e < c.nest; ++e)
            for (int i = 0; i < c.npieces[e]; ++i, ++at) {
                const bool sw = c.swap && c.swap[at];
                add(grad, sw ? ikY[e] : ikX[e], iFG[at]);
                add(hpl, sw ? ikX[e] : ikY[e], iFH[at]);
            }
        const size_t lb = (size_t)work_pitch(b, wl) * b->ny * es, lbk = (size_t)work_pitch(b, wk) * b->ny * es;
        if ((2 * grad.size() + hpl.size()) * lb + 4 * (size_t)c.nest * lbk > qb->split_legs.bytes)
            return fail(std::string(who) + ": this call needs " + std::to_string(2 * grad.size() + hpl.size()) + " leg planes and " + std::to_string(c.nest) +
                        " estimators, more than oa_qe_band_bind was told (max_leg_planes, normalisation planes)");
    }
    int rc = from_maps ? mv_sources_maps(p, B, c, sbase, cb, wl, rl, st) : mv_sources_embed(p, B, srcs, sbase, cb, wl, rl, st);
    if (rc) return rc;
    if (c.pol) rc = oa_qe_pol(b, c.npieces[0], c.signs, iFG.data(), iFH.data(), c.swap, ikX[0], ikY[0], iFn[0], qb->kk, 0, wl, wk, rl, rk, -1, 0, st);
    else rc = oa_qe_mv(b, c.nest, c.npieces, c.signs, iFG.data(), iFH.data(), c.swap, ikX.data(), ikY.data(), iFn.data(), qb->kk, 0, wl, wk, rl, rk,
                       -1, 0, st);
    if (rc) return rc;
    return band_scatter(p->dtype, qb->kk, b->kp, b->ny, out, p->kp, p->ny, wk, rk, accumulate ? 1 : (zero_outside ? 2 : 0), st);
}
/* ---- oa_qe_tt_splits / oa_qe_tt_split_power on the band grid ---------------------------------------------------------------------------
 * The leg band of the n splits' transforms is embedded into n inner source planes in one launch (device table of sources, re-uploaded
 * only when the caller's pointers change), the inner plan's own oa_qe_tt_splits writes the n^2 kappa planes into an evenly spaced
 * plan-owned block (so its divergence stays one batched launch), and ONE launch either scatters kappa's band of all n^2 planes to the
 * caller's N-grid planes (host_out) or combines them per mode into the real N-grid half-plane (out_power: the K_ij never exist on the
 * N grid).  The source planes and the block are taken on first use and grown when a call brings more splits than any before: that call
 * synchronises the device once (the inner plan's pool likewise), later calls with as many splits or fewer neither allocate nor
 * synchronise. */
static int mixed_qe_tt_splits(oa_plan* p, Pipeline* q, const char* who, int nsplits, const void* const* host_kmaps, void* const* host_out,
                              void* out_power, double norm, int zero_outside, hipStream_t st) {
    if (!(p->mixed && q->FG && q->band)) return fail(std::string(who) + ": call oa_plan_set_filters first");
    oa_plan* b = q->band;
    band_options(q);
    const int n = nsplits, npairs = n * n, nout = host_out ? npairs : 0;
    for (int i = 0; i < n; ++i)
        if (!host_kmaps[i]) return fail(std::string(who) + ": NULL split plane");
    for (int k = 0; k < nout; ++k)
        if (!host_out[k]) return fail(std::string(who) + ": NULL output plane");
    const size_t cb = plane_bytes(b);
    if (n > q->bs_cap) {
        q->bs_cap = 0;
        if (int rc = q->bsplit.reserve(((size_t)n + (size_t)npairs) * cb)) return rc;
        q->bs_cap = n;
        OA_HIP(hipMemsetAsync(q->bsplit.p, 0, (size_t)n * cb, st));  // source planes: zero outside the leg band (only the band is ever written)
    }
    if ((size_t)(n + nout) * sizeof(void*) > q->bs_tab.bytes) {
        if (int rc = q->bs_tab.reserve((size_t)std::max(n + nout, 8 + 64) * sizeof(void*))) return rc;
        q->bs_key.clear();
    }
    std::vector<const void*> key(host_kmaps, host_kmaps + n);
    if (nout) key.insert(key.end(), host_out, host_out + nout);
    if (key != q->bs_key) {                           // (pageable source: staged before the call returns; ordered on this stream)
        q->bs_key = key;
        OA_HIP(hipMemcpyAsync(q->bs_tab.p, q->bs_key.data(), key.size() * sizeof(void*), hipMemcpyHostToDevice, st));
    }
    char* const sbase = q->bsplit.at();
    char* const kbase = sbase + (size_t)q->bs_cap * cb;
    const long pe = plane_elems(b);                   // complex elements per inner plane
    int rc = band_embed(p->dtype, (const void* const*)q->bs_tab.p, n, p->kp, p->ny, sbase, pe, b->kp, b->ny, q->wl, q->rl, st);
    if (rc) return rc;
    std::vector<const void*> ins(n);
    std::vector<void*> outs(npairs);
    for (int i = 0; i < n; ++i) ins[i] = sbase + (size_t)i * cb;
    for (int k = 0; k < npairs; ++k) outs[k] = kbase + (size_t)k * cb;
    if ((rc = oa_qe_tt_splits(b, n, ins.data(), outs.data(), 0, st))) return rc;
    if (out_power)
        return band_split_power(p->dtype, n, kbase, pe, b->kp, b->ny, out_power, p->kp, p->ny, q->wk, q->rk, norm, zero_outside, st);
    return band_scatter_batch(p->dtype, kbase, pe, npairs, b->kp, b->ny, (void* const*)q->bs_tab.p + n, p->kp, p->ny, q->wk, q->rk, zero_outside, st);
}
/* ---- oa_mc_run_mv on the band grid ----------------------------------------------------------------------------------------------------
 * The shard's per-call planes that are not filters -- the MV weights and the bin ids -- get their inner-layout copies from a second set-up
 * entry, oa_mc_mv_band_bind, which also takes every plane the shard would otherwise allocate on first use.  A shard call then looks its
 * pointers up (pol_inner, and the key below) and runs the loop of the power-of-two plans on the inner plan: no allocation, no
 * synchronisation. */
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
static int mc_mv_bind(oa_plan* p, Pipeline* q, const void* w, long wstride, int nest, const int32_t* ids, int nids, int nspec_max) {
    Pipeline::PolBind& B = q->pb;
    Pipeline::PolBind::McBind& M = B.mc;
    M.bound = false;
    if (!B.bound) return fail("oa_mc_mv_band_bind: bind the filter and normalisation planes first (oa_qe_band_bind)");
    const long sbl = oa_bin_power_multi_scratch_bytes(nspec_max, nids);
    if (sbl < 0) return fail("oa_mc_mv_band_bind: nspec_max outside 1..28, nids outside 1..1024 or nspec_max * nids > 4096 (oa_bin_power_multi)");
    oa_plan* b = B.plan;
    const size_t rb = band_real_bytes(b), cb = plane_bytes(b), rs = b->dtype == OA_F32 ? 4 : 8;
    const size_t ib = (size_t)b->ny * b->kp * sizeof(int32_t), ub = (size_t)nspec_max * nids * sizeof(double);
    const size_t off_ids = up256(w ? (size_t)nest * rb : 0), off_draw = up256(off_ids + ib), off_kappa = off_draw + 3 * cb;
    const size_t off_scratch = up256(off_kappa + (size_t)nest * cb), off_sums = up256(off_scratch + (size_t)sbl), need = off_sums + ub;
    OA_HIP(hipDeviceSynchronize());                 // the caller's planes may have been written on any stream; the old copies may be in use
    if (int rc = M.pool.reserve(need)) return rc;
    char* const base = M.pool.at();
    OA_HIP(hipMemset(base, 0, need));               // weights, draws and kappa planes: only their band is ever written
    OA_HIP(hipMemset(base + off_ids, 0xFF, ib));
    if (w)
        for (int e = 0; e < nest; ++e)
            if (int rc = band_copy(p->dtype == OA_F32 ? 0 : 1, (const char*)w + (size_t)e * wstride * rs, p->kp, p->ny, base + (size_t)e * rb, b->kp, b->ny,
                                   B.wk, B.rk, 1.0, nullptr)) return rc;
    if (int rc = band_copy(2, ids, p->kp, p->ny, base + off_ids, b->kp, b->ny, B.wk, B.rk, 1.0, nullptr)) return rc;
    OA_HIP(hipDeviceSynchronize());
    M.w = w; M.wstride = wstride; M.ids = ids; M.nids = nids; M.nest = nest; M.nspec_max = nspec_max;
    M.off_ids = off_ids; M.off_draw = off_draw; M.off_kappa = off_kappa; M.off_scratch = off_scratch; M.off_sums = off_sums;
    M.bound = true;
    return 0;
}

/* The per-realisation loop of oa_mc_run_mv, shared by both plan kinds.  `grid` is the map's plan: Philox counters, self-conjugate edge
 * rules and the covsqrt planes are its.  `run` is the plan the estimators and the binning run on -- `grid` itself (power of two), or
 * the inner plan of its band grid, into whose layout the draw then goes directly (oa_grf_mix_band_inner); every plane below is in `run`'s
 * layout.  Nothing here allocates or synchronises once the pools exist.
 * SOURCE STAGE HOOK: `source` (when set) replaces the band draw -- it leaves realisation i's T, E, B on the leg band of `draw`
 * (oa_mc_run_mv_windowed's windowed front end).  `mf` (when set): nest host-side pointers to float64 stack planes, and `mf_mv` the MV
 * stack or nullptr -- one stack_add_region_multi launch per realisation over kappa's band (band_stack_add_multi when `run` is an inner
 * plan: the stacks are always `grid`'s planes). */
struct McMvLoop {
    oa_plan* grid; oa_plan* run; Pipeline* rq;
    bool engaged;                                   // the one-launch divergence: kappa planes = run's work planes c[0] + e
    void* draw[3]; char* own; void* scratch; double* sums;
    const void* w; long wstride; const int32_t* ids;
    int mrow;
    const void* const* FG; const void* const* FH; const void* const* Fn;    // the call's filter / normalisation planes in run's layout
    std::function<int(long)> source;
    double* const* mf = nullptr; double* mf_mv = nullptr;
};
// the arguments of oa_mc_run_mv and (the last four) oa_mc_run_mv_windowed, as the entries receive them (include/orphics_amd.h)
struct McMvArgs {
    uint64_t base_seed; long sim_lo, sim_hi; const void* const* covsqrt; int nest; const int* npieces; const double* signs;
    const void* const* FG; const void* const* FH; const int* swap; const int* xsrc; const int* ysrc; const void* const* Fn;
    const void* w; long wstride; int nspec; const int* a; const int* b; const int32_t* ids; int nids; const int64_t* counts; double norm;
    int wl, wk, rl, rk, mrow; int64_t* n; double* S; double* C; hipStream_t st;
    const void* window; const void* rot_c; const void* rot_s; double* const* mf;
};
static int mc_mv_loop(const McMvLoop& L, const McMvArgs& a) {
    oa_plan* r = L.run;
    hipStream_t st = a.st;
    const size_t pb = plane_bytes(r);
    const long pe = plane_elems(r);
    const void* const block = L.engaged ? L.rq->c[0] : (const void*)L.own;
    std::vector<const void*> kX(a.nest), kY(a.nest);
    for (int e = 0; e < a.nest; ++e) { kX[e] = L.draw[a.xsrc[e]]; kY[e] = L.draw[a.ysrc[e]]; }
    for (long i = a.sim_lo; i < a.sim_hi; ++i) {
        int rc = L.source    ? L.source(i)
               : L.grid == r ? oa_grf_mix_band(r, a.base_seed, 3 * (uint64_t)i, 3, a.covsqrt, 1.0, L.draw, a.wl, a.rl, st)
                             : oa_grf_mix_band_inner(L.grid, a.base_seed, 3 * (uint64_t)i, 3, a.covsqrt, 1.0, L.draw, r->ny, r->kp, a.wl, a.rl, st);
        if (rc) return rc;
        if (L.engaged) {
            const MvCall c{a.nest, a.npieces, a.signs, L.FG, L.FH, a.swap, kX.data(), kY.data(), L.Fn, false};
            if ((rc = qe_mv_pow2(r, L.rq, c, nullptr, 0, a.wl, a.wk, a.rl, a.rk, L.mrow, 0, st, true))) return rc;
        } else {
            for (int e = 0, at = 0; e < a.nest; at += a.npieces[e], ++e) {       // one at a time, each into its plane of the entry's block
                const MvCall c{1, a.npieces + e, a.signs + at, L.FG + at, L.FH + at, a.swap ? a.swap + at : nullptr,
                               kX.data() + e, kY.data() + e, L.Fn + e, false};
                if ((rc = qe_mv_pow2(r, L.rq, c, L.own + (size_t)e * pb, 0, a.wl, a.wk, a.rl, a.rk, L.mrow, 0, st, false))) return rc;
            }
        }
        if ((rc = oa_bin_power_multi(r->dtype, a.nest, block, pe, L.w, L.wstride, a.nspec, a.a, a.b, a.norm, L.ids, a.nids,
                                     r->ny, r->kp, r->nx / 2, a.wk, a.rk, L.sums, L.scratch, st))) return rc;
        if ((rc = moments_add_binned_multi(L.sums, a.counts, a.nspec, a.nids, a.n, a.S, a.C, st))) return rc;
        if (!L.mf) continue;
        // the stacks are the map's planes: on a band grid kappa_hat's band goes from the inner rows and pitch to the N grid's
        rc = L.grid == r ? stack_add_region_multi(r->dtype, block, pe, L.w, L.wstride, a.nest, L.mf, L.mf_mv, r->ny, r->kp, a.wk, a.rk, st)
                         : band_stack_add_multi(r->dtype, block, pe, L.w, L.wstride, a.nest, L.mf, L.mf_mv, r->ny, r->kp, L.grid->ny,
                                                L.grid->kp, a.wk, a.rk, st);
        if (rc) return rc;
    }
    return 0;
}

/* oa_mc_run_mv on a 2^a 3^b 5^c plan: every pointer of the call is looked up in the two bindings and everything is refused before the
 * first launch; then the loop above on the inner plan.  kappa_hat per mode is the same on both grids (the bound normalisations carry
 * My Mx / (ny nx)), the inner ids are the N grid's at the same mode, and since Mx >= 2 kappa_cols the inner Nyquist column is never
 * visited: column 0 is the only visited one of Hermitian multiplicity 1, as on the N grid.  The caller's counts are the N plane's. */
// what a shard call resolves before its first launch: the loop's description and, on a band grid, the inner-layout planes of the call's pointers
struct MvShard {
    std::vector<const void*> iFG, iFH, iFn;
    McMvLoop L;
};
// `who`: the entry's name.  `how_all`: every refusal ends with the way out (oa_mc_run_mv_windowed names the driver and one_call=False in
// each of its refusals); oa_mc_run_mv's messages are as they were.  `how_rdn0` (oa_mc_run_rdn0_mv): that entry's way out in the place of `how`,
// in every refusal; the inner plan's pool is then not checked here (oa_rdn0_set_data_mv grew it: the entry checks the data legs next).
static int mixed_mc_mv_lookup(const std::string& who, bool how_all, oa_plan* p, Pipeline* q, const McMvArgs& a, MvShard* out,
                              const char* how_rdn0 = nullptr) {
    static const char* const how_mc = " -- bind the estimator set with oa_qe_band_bind, then oa_mc_mv_band_bind, or run the host loop of the "
                                      "existing entries (mc.GaussianN0MonteCarloPol with one_call=False)";
    const char* const how = how_rdn0 ? how_rdn0 : how_mc;
    const std::string tail = (how_all || how_rdn0) ? how : "";
    Pipeline::PolBind& B = q->pb;
    const Pipeline::PolBind::McBind& M = B.mc;
    if (!B.bound) return fail(who + ": on map sides 2^a 3^b 5^c the filter and normalisation planes are bound first" + how);
    if (a.wl != B.wl || a.wk != B.wk || a.rl != B.rl || a.rk != B.rk || a.mrow != B.mrow)
        return fail(who + ": leg / kappa columns and rows or the row grid differ from the bound ones" + how);
    if (!M.bound) return fail(who + ": no Monte-Carlo binding on the current oa_qe_band_bind binding" + how);
    if (a.w != M.w || (a.w && a.wstride != M.wstride) || a.ids != M.ids || a.nids != M.nids || a.nest != M.nest || a.nspec > M.nspec_max)
        return fail(who + ": the weights, their stride, the bin ids, nids, nest or nspec differ from the Monte-Carlo binding's" + how);
    std::vector<const void*>&iFG = out->iFG, &iFH = out->iFH, &iFn = out->iFn;
    oa_plan* b = B.plan;
    Pipeline* qb = (Pipeline*)b->pipe;
    band_options(q);
    const size_t rb = band_real_bytes(b), es = elem_bytes(b);
    char* const fbase = B.planes.at();
    char* const nbase = fbase + B.fkey.size() * rb;
    int total = 0;
    for (int e = 0; e < a.nest; ++e) total += a.npieces[e];
    iFG.assign(total, nullptr); iFH.assign(total, nullptr); iFn.assign(a.nest, nullptr);
    for (int i = 0; i < total; ++i) {
        iFG[i] = pol_inner(B.fkey, a.FG[i], fbase, rb);
        iFH[i] = pol_inner(B.fkey, a.FH[i], fbase, rb);
        if (!iFG[i] || !iFH[i]) return fail(who + ": a filter plane of this call is not bound (oa_qe_band_bind binds every distinct plane)" + tail);
    }
    for (int e = 0; e < a.nest; ++e) {
        iFn[e] = pol_inner(B.nkey, a.Fn[e], nbase, rb);
        if (!iFn[e]) return fail(who + ": a normalisation plane of this call is not bound (oa_qe_band_bind)" + tail);
    }
    if (!how_rdn0) {                                // the inner plan's leg pool: sized by oa_qe_band_bind, never grown here
        std::vector<std::pair<int, const void*>> grad, hpl;
        auto add = [](std::vector<std::pair<int, const void*>>& v, int s, const void* f) {
            for (auto& k : v) if (k.first == s && k.second == f) return;
            v.emplace_back(s, f);
        };
        for (int e = 0, at = 0; e < a.nest; ++e)
            for (int i = 0; i < a.npieces[e]; ++i, ++at) {
                const bool sw = a.swap && a.swap[at];
                add(grad, sw ? a.ysrc[e] : a.xsrc[e], iFG[at]);
                add(hpl, sw ? a.xsrc[e] : a.ysrc[e], iFH[at]);
            }
        const size_t lb = (size_t)work_pitch(b, a.wl) * b->ny * es, lbk = (size_t)work_pitch(b, a.wk) * b->ny * es;
        if ((2 * grad.size() + hpl.size()) * lb + 4 * (size_t)a.nest * lbk > qb->split_legs.bytes)
            return fail(who + ": this call needs " + std::to_string(2 * grad.size() + hpl.size()) + " leg planes and " + std::to_string(a.nest) +
                        " estimators, more than oa_qe_band_bind was told (max_leg_planes, normalisation planes)" + tail);
    }
    char* const base = M.pool.at();
    const size_t cb = plane_bytes(b);
    long fn_moff = 0;
    out->L = McMvLoop{p, b, qb, mv_div_batched(qb, a.nest, iFn.data(), es / 2, &fn_moff),
                      {base + M.off_draw, base + M.off_draw + cb, base + M.off_draw + 2 * cb}, base + M.off_kappa, base + M.off_scratch,
                      (double*)(base + M.off_sums), a.w ? (const void*)base : nullptr, (long)(rb / (es / 2)),
                      (const int32_t*)(base + M.off_ids), -1, iFG.data(), iFH.data(), iFn.data()};
    return 0;
}
// the argument checks oa_mc_run_mv and oa_mc_run_mv_windowed share, under the caller's name; `plan_msg`: what a chirp-z plan is told
static int mc_mv_check(const std::string& who, const char* plan_msg, const oa_plan* p, const McMvArgs& a) {
    OA_REQUIRE(p && a.covsqrt && a.npieces && a.signs && a.FG && a.FH && a.xsrc && a.ysrc && a.Fn && a.ids && a.counts &&
               a.n && a.S && a.C && a.sim_hi >= a.sim_lo, who + ": bad argument");
    OA_REQUIRE(p->pow2 || p->mixed, who + plan_msg);
    OA_REQUIRE(a.nest >= 1 && a.nest <= 6, who + ": 1 <= nest <= 6 estimators");
    OA_REQUIRE(a.nids >= 3, who + ": nids must be at least 3 (two outer bins around the bandpowers)");
    if (int rc = bin_power_multi_check(who.c_str(), p->dtype, a.nest, a.w != nullptr, a.nspec, a.a, a.b, a.nids)) return rc;
    const int hw = p->nx / 2 + 1;
    OA_REQUIRE(a.wl >= 0 && a.wk >= 0 && a.rl >= 0 && a.rk >= 0 && a.wl <= hw && a.wk <= hw && 2L * a.rl - 1 <= p->ny && 2L * a.rk - 1 <= p->ny,
               who + ": leg / kappa band beyond the hc plane");
    int total = 0;
    for (int e = 0; e < a.nest; ++e) {
        OA_REQUIRE(a.npieces[e] >= 1 && a.Fn[e], who + ": bad estimator entry");
        OA_REQUIRE(a.xsrc[e] >= 0 && a.xsrc[e] < 3 && a.ysrc[e] >= 0 && a.ysrc[e] < 3, who + ": source index outside [0, 3) (0 T, 1 E, 2 B)");
        total += a.npieces[e];
    }
    for (int i = 0; i < total; ++i) OA_REQUIRE(a.FG[i] && a.FH[i], who + ": NULL filter plane");
    return 0;
}
// the entry-owned pool of a power-of-two plan, taken on the first call (and regrown when a call needs more): that call synchronises the
// device once; and the loop's description on it
static int mc_mv_pow2_loop(oa_plan* p, Pipeline* q, const McMvArgs& a, McMvLoop* L) {
    if (int rc = ensure_work(p, q)) return rc;
    const size_t pb = plane_bytes(p);
    long fn_moff = 0;
    const bool engaged = mv_div_batched(q, a.nest, a.Fn, elem_bytes(p) / 2, &fn_moff);
    const size_t sb = (size_t)oa_bin_power_multi_scratch_bytes(a.nspec, a.nids), ub = (size_t)a.nspec * a.nids * sizeof(double);
    if (int rc = q->mvmc.reserve((3 + (engaged ? 0 : (size_t)a.nest)) * pb + sb + ub, true)) return rc;
    char* const base = q->mvmc.at();
    *L = McMvLoop{p, p, q, engaged, {base, base + pb, base + 2 * pb}, base + 3 * pb /* per-estimator kappa planes when the plan's are not used */,
                  base + q->mvmc.bytes - sb - ub, (double*)(base + q->mvmc.bytes - ub), a.w, a.wstride, a.ids, a.mrow, a.FG, a.FH, a.Fn};
    return 0;
}
/* SOURCE STAGE of a windowed realisation (oa_mc_run_mv_windowed; L->source): the full-plane T, E, B draw rotated to T, Q, U in the same
 * pass (grf_mix_teb_to_tqu, the counters of the band draw), the window in real space, and T, E, B on the leg band of the loop's three
 * source planes.  The planes of the front end are taken on the first windowed call (regrown when the leg band widens).
 * POWER OF TWO, fused: one fused row launch over the three planes (inverse columns, C2R / Npix -> x window -> R2C, the real maps in LDS only,
 * leg columns stored at the compact pitch), one batched forward column launch, Q, U -> E, B on the band.  Unfused (A/B): the window at
 * the C2R's store, the real map in HBM, the R2C on the leg band. */
// ONE windowed triple (both entries' per-triple body): streams sid0 .. sid0 + 2 -> T, E, B on the leg band of dst[0..2] (full-pitch hc planes
// one plane apart).  wb: 3 full T, Q, U planes | 3 column temporaries | 3 compact row planes
static int mv_window_triple_pow2(oa_plan* p, const McMvArgs& a, bool fused, uint64_t sid0, char* wb, void* const* dst) {
    const size_t es = elem_bytes(p), pb = plane_bytes(p);
    const long pl = work_pitch(p, a.wl);
    const size_t lb = (size_t)pl * p->ny * es;
    char* const tmp = wb + 3 * pb;
    char* const rowT = wb + 6 * pb;
    const double inv = 1.0 / ((double)p->ny * p->nx);
    void* tqu[3] = {wb, wb + pb, wb + 2 * pb};
    int rc = grf_mix_teb_to_tqu(p, a.base_seed, sid0, a.covsqrt, a.rot_c, a.rot_s, tqu, a.st);
    if (rc) return rc;
    if (fused) {
        if ((rc = qe_windowed_rows_w(p, wb, tmp, a.window, a.wl, pl, inv, a.st, rowT, 3, plane_elems(p), (long)(lb / es)))) return rc;
        if ((rc = qe_fwd_cols_batch_w(p, rowT, pl, dst[0], 3, (long)(lb / es), plane_elems(p), a.wl, a.rl, a.st))) return rc;
    } else {
        for (int f = 0; f < 3; ++f) {
            if ((rc = oa_fft_c2r_windowed(p, tqu[f], tmp + (size_t)f * pb, inv, a.window, a.st))) return rc;
            if ((rc = oa_fft_r2c(p, tmp + (size_t)f * pb, dst[f], 1.0, a.wl, a.rl, a.st))) return rc;
        }
    }
    return band_rot2(p->dtype, a.rot_c, a.rot_s, dst[1], dst[2], p->ny, p->kp, a.wl, a.rl, a.st);
}
static size_t mv_window_triple_bytes(const oa_plan* p, int wl) {
    return 6 * plane_bytes(p) + 3 * (size_t)work_pitch(p, wl) * p->ny * elem_bytes(p);
}
static int mv_window_source_pow2(oa_plan* p, Pipeline* q, const McMvArgs& a, bool fused, McMvLoop* L) {
    if (int rc = q->mvwin.reserve(mv_window_triple_bytes(p, a.wl))) return rc;
    char* const wb = q->mvwin.at();
    void* const* const dst = L->draw;
    L->source = [=](long i) -> int { return mv_window_triple_pow2(p, a, fused, 3 * (uint64_t)i, wb, dst); };
    return 0;
}
/* BAND GRID, fused: ONE batched inverse column launch over the three N-grid planes (in place), ONE fused row launch, the pruned column DFT
 * of the three planes and the fold with the Q, U -> E, B rotation onto the loop's three inner source planes (band_win_r2c with rot_c /
 * rot_s: mixed_mc_run_windowed's front end with planes in the place of realisations).  Unfused: oa_fft_c2r_windowed per plane onto a real
 * map in an entry-owned plane, then ONE band_maps_r2c(3, rot_c, rot_s) -- what oa_qe_mv_maps runs. */
static int mv_window_source_band(oa_plan* p, Pipeline* q, const McMvArgs& a, bool fused, McMvLoop* L) {
    Pipeline::PolBind& B = q->pb;
    const size_t pb = plane_bytes(p);
    if (int rc = B.mwin.reserve(6 * pb + band_maps_scratch_bytes(p, 3, a.wl, a.rl))) return rc;
    char* const wb = B.mwin.at();
    char* const tmp = wb + 3 * pb;                  // ny x nx reals fit an hc plane
    void* const rows = wb + 6 * pb;
    const long pne = plane_elems(p), pbe = plane_elems(B.plan);
    const double inv = 1.0 / ((double)p->ny * p->nx);
    void* const dst = L->draw[0];                   // the three inner source planes are contiguous, one inner plane apart (oa_mc_mv_band_bind)
    const int dny = B.plan->ny;
    const long dkp = B.plan->kp;
    L->source = [=](long i) -> int {
        void* tqu[3] = {wb, wb + pb, wb + 2 * pb};
        int rc = grf_mix_teb_to_tqu(p, a.base_seed, 3 * (uint64_t)i, a.covsqrt, a.rot_c, a.rot_s, tqu, a.st);
        if (rc) return rc;
        if (fused) {
            if ((rc = mixed_cols_inverse_batch(p, 3, wb, pne, a.st))) return rc;
            return band_win_r2c(p, 3, wb, pne, a.window, inv, rows, 0, a.wl, a.rl, a.rot_c, a.rot_s, dst, pbe, dny, dkp, a.st);
        }
        const void* maps[3] = {tmp, tmp + pb, tmp + 2 * pb};
        for (int f = 0; f < 3; ++f)
            if ((rc = oa_fft_c2r_windowed(p, tqu[f], tmp + (size_t)f * pb, inv, a.window, a.st))) return rc;
        return band_maps_r2c(p, 3, maps, a.rot_c, a.rot_s, rows, a.wl, a.rl, dst, pbe, dny, dkp, a.st);
    };
    return 0;
}
/* The body of oa_mc_run_mv and oa_mc_run_mv_windowed behind their argument checks.  Power of two: the loop on the plan itself, with the
 * call's planes.  2^a 3^b 5^c: on the inner plan of the band grid behind oa_qe_band_bind + oa_mc_mv_band_bind, the windowed source stage on
 * the N grid in front of it and the stacks on the N grid behind it. */
static int mc_mv_shard(const std::string& who, bool how_all, oa_plan* p, const McMvArgs& a) {
    Pipeline* q = pipe_of(p);
    MvShard c;
    McMvLoop& L = c.L;
    if (int rc = p->mixed ? mixed_mc_mv_lookup(who, how_all, p, q, a, &c) : mc_mv_pow2_loop(p, q, a, &L)) return rc;
    if (a.mf) { L.mf = a.mf; L.mf_mv = a.w ? a.mf[a.nest] : nullptr; }
    if (a.window) {
        // fused row pass or the unfused flow: OA_OPT_WIN_FUSED; a band-grid plan, until the option is set, picks by row length
        // (mixed_mc_run_windowed's rule), and rows its fused kernel does not hold take the unfused flow
        const bool fused = p->mixed ? band_rows_win_ok(p) && (q->opt_win_fused_set ? q->opt_win_fused : p->nx > 1200) : q->opt_win_fused;
        if (int rc = p->mixed ? mv_window_source_band(p, q, a, fused, &L) : mv_window_source_pow2(p, q, a, fused, &L)) return rc;
    }
    return mc_mv_loop(L, a);
}

/* ---- oa_rdn0_set_data_mv / oa_mc_run_rdn0_mv: RDN0 of an estimator set (a plan pointer: the map's power-of-two plan, or the inner plan of a band grid) ----------------------------------------------
 * SLOTS.  The distinct leg planes of a field triple X = (X_T, X_E, X_B) under an estimator set: one gradient pair per distinct
 * (source index, FG), one H plane per distinct (source index, FH) -- qe_mv_pow2's sharing rule with source INDICES in the place of source
 * pointers, so that the data triple d and the draws s, s' number their planes alike.  In a pool of compact planes gradient pair g sits at
 * planes 2 g, 2 g + 1 and H plane h at 2 ng + h.  Piece idx of estimator e in QE_e(X; Y) reads its gradient pair from (swap ? Y : X) at
 * gslot[idx] and its H plane from (swap ? X : Y) at hslot[idx].  BOTH entries number through rdn0mv_slots. */
constexpr size_t MV_RTAB_BYTES = 64 * 64 + 1024;    // the device table mv_rtab of the table / chain row stage
struct Rdn0MvSlots {
    std::vector<std::pair<int, const void*>> grad, hpl;     // (source index, filter plane)
    std::vector<int> gslot, hslot;                          // per piece
    int total = 0;
    int ng() const { return (int)grad.size(); }
    int nh() const { return (int)hpl.size(); }
    int nplanes() const { return 2 * ng() + nh(); }
    std::vector<const void*> key() const {                  // what the data legs depend on besides the bands
        std::vector<const void*> k;
        for (const auto& g : grad) { k.push_back((const void*)(uintptr_t)(g.first + 1)); k.push_back(g.second); }
        k.push_back(nullptr);
        for (const auto& h : hpl) { k.push_back((const void*)(uintptr_t)(h.first + 1)); k.push_back(h.second); }
        return k;
    }
};
static Rdn0MvSlots rdn0mv_slots(int nest, const int* npieces, const void* const* FG, const void* const* FH, const int* swap, const int* xsrc,
                                const int* ysrc) {
    Rdn0MvSlots S;
    auto slot_of = [](std::vector<std::pair<int, const void*>>& v, int src, const void* f) {
        for (size_t i = 0; i < v.size(); ++i) if (v[i].first == src && v[i].second == f) return (int)i;
        v.emplace_back(src, f);
        return (int)v.size() - 1;
    };
    for (int e = 0; e < nest; ++e)
        for (int i = 0; i < npieces[e]; ++i, ++S.total) {
            const bool sw = swap && swap[S.total];
            S.gslot.push_back(slot_of(S.grad, sw ? ysrc[e] : xsrc[e], FG[S.total]));
            S.hslot.push_back(slot_of(S.hpl, sw ? xsrc[e] : ysrc[e], FH[S.total]));
        }
    return S;
}
// the checks of the estimator-set description both entries make, under the caller's name
static int rdn0mv_set_check(const std::string& who, const oa_plan* p, int nest, const int* npieces, const void* const* FG, const void* const* FH,
                            const int* xsrc, const int* ysrc, int wl, int wk, int rl, int rk) {
    OA_REQUIRE(nest >= 1 && nest <= 6, who + ": 1 <= nest <= 6 estimators");
    const int hw = p->nx / 2 + 1;
    OA_REQUIRE(wl >= 0 && wk >= 0 && rl >= 0 && rk >= 0 && wl <= hw && wk <= hw && 2L * rl - 1 <= p->ny && 2L * rk - 1 <= p->ny,
               who + ": leg / kappa band beyond the hc plane");
    int total = 0;
    for (int e = 0; e < nest; ++e) {
        OA_REQUIRE(npieces[e] >= 1, who + ": bad estimator entry");
        OA_REQUIRE(xsrc[e] >= 0 && xsrc[e] < 3 && ysrc[e] >= 0 && ysrc[e] < 3, who + ": source index outside [0, 3) (0 T, 1 E, 2 B)");
        total += npieces[e];
    }
    for (int i = 0; i < total; ++i) OA_REQUIRE(FG[i] && FH[i], who + ": NULL filter plane");
    return 0;
}
/* The leg planes of ONE field triple into `pool` (nplanes compact planes lb bytes apart): qe_mv_pow2's leg stage -- ONE inverse pass-1
 * launch over all fields where it applies (at most 32 fields, sources a whole number of complex elements apart; OA_OPT_MV_BATCH), else one
 * launch per field.  *done = 1: the planes need no inverse pass 2. */
static int rdn0mv_legs_of(oa_plan* p, Pipeline* q, const Rdn0MvSlots& S, const void* const src[3], char* pool, size_t lb, int wl, int rl, long pl,
                          int my, hipStream_t st, int* done) {
    const size_t es = elem_bytes(p);
    const int ng = S.ng(), nh = S.nh();
    *done = 0;
    std::vector<const void*> srcs;
    unsigned long long srcsel = 0;
    bool batch = ng + nh <= 32 && q->opt_mv_batch;
    for (int f = 0; f < ng + nh; ++f) {
        const void* sp = src[f < ng ? S.grad[f].first : S.hpl[f - ng].first];
        size_t k = 0;
        while (k < srcs.size() && srcs[k] != sp) ++k;
        if (k == srcs.size()) srcs.push_back(sp);
        if (f < 32) srcsel |= (unsigned long long)k << (2 * f);
    }
    for (size_t k = 1; k < srcs.size(); ++k) batch = batch && (((const char*)srcs[k] - (const char*)srcs[0]) % (long)es == 0);
    if (batch) {
        std::vector<const void*> key;
        for (int g = 0; g < ng; ++g) key.push_back(S.grad[g].second);
        for (int h = 0; h < nh; ++h) key.push_back(S.hpl[h].second);
        if (key != q->mv_fkey) {       // (pageable source: staged before the call returns; ordered on this stream)
            OA_HIP(hipMemcpyAsync(q->mv_ftab, key.data(), key.size() * sizeof(void*), hipMemcpyHostToDevice, st));
            q->mv_fkey = key;
        }
        const long off1 = srcs.size() > 1 ? (long)(((const char*)srcs[1] - (const char*)srcs[0]) / (long)es) : 0;
        const long off2 = srcs.size() > 2 ? (long)(((const char*)srcs[2] - (const char*)srcs[0]) / (long)es) : 0;
        return qe_legs_batch_w(p, srcs[0], off1, off2, srcsel, (const void* const*)q->mv_ftab, ng, nh, pool, (long)(lb / es), wl, rl, pl, st, my, 2, done);
    }
    for (int g = 0; g < ng; ++g)
        if (int rc = qe_legs_subset_w(p, src[S.grad[g].first], S.grad[g].second, pool + 2 * (size_t)g * lb, pool + (2 * (size_t)g + 1) * lb, 2, wl, rl, pl,
                                      st, my)) return rc;
    for (int h = 0; h < nh; ++h)
        if (int rc = qe_legs_subset_w(p, src[S.hpl[h].first], S.hpl[h].second, pool + (2 * (size_t)ng + h) * lb, nullptr, 1, wl, rl, pl, st, my)) return rc;
    return 0;
}
// where a shard lives: leg planes of s and s', product and pass-1 planes of the 2 nest chains in the plan's pool of compact planes
// (split_legs); draws, kappa block and tail scratch in rdn0mv_pool
struct Rdn0MvPlanes {
    size_t lb, lbk, pb;
    char *legs[3];                     // the leg pools of d, s, s'
    char *prod, *tmp, *draw, *kappa, *scratch;
};
static size_t rdn0mv_split_bytes(const oa_plan* p, const Rdn0MvSlots& S, int nest, int wl, int wk) {
    const size_t es = elem_bytes(p);
    return 2 * (size_t)S.nplanes() * work_pitch(p, wl) * p->ny * es + 8 * (size_t)nest * work_pitch(p, wk) * p->ny * es;
}
static Rdn0MvPlanes rdn0mv_planes(const oa_plan* p, const Pipeline* q, const Rdn0MvSlots& S, int nest, int wl, int wk) {
    Rdn0MvPlanes P;
    const size_t es = elem_bytes(p);
    P.lb = (size_t)work_pitch(p, wl) * p->ny * es; P.lbk = (size_t)work_pitch(p, wk) * p->ny * es; P.pb = plane_bytes(p);
    P.legs[0] = q->rdn0mv_legs.at(); P.legs[1] = q->split_legs.at(); P.legs[2] = P.legs[1] + (size_t)S.nplanes() * P.lb;
    P.prod = P.legs[2] + (size_t)S.nplanes() * P.lb; P.tmp = P.prod + 4 * (size_t)nest * P.lbk;
    P.draw = q->rdn0mv_pool.at(); P.kappa = P.draw + 6 * P.pb; P.scratch = P.kappa + 2 * (size_t)nest * P.pb;
    return P;
}
/* One realisation whose draws s, s' sit on the six planes of P.draw: leg planes of s and of s' (one batched launch per triple [+ ONE
 * inverse pass 2 over both]), the row stage of the 2 nest chains -- A_e = pieces of QE_e(d; s), then of QE_e(s; d); B_e = pieces of
 * QE_e(s; s'), then of QE_e(s'; s); chain e and nest + e --, their divergences into the kappa block, the tail. */
static int rdn0mv_one(oa_plan* p, Pipeline* q, const McMvArgs& a, const Rdn0MvSlots& S, const Rdn0MvPlanes& P, int my) {
    hipStream_t st = a.st;
    const size_t es = elem_bytes(p), lb = P.lb, lbk = P.lbk;
    const long pl = work_pitch(p, a.wl), pk = work_pitch(p, a.wk);
    const int nest = a.nest, np = S.nplanes(), ng = S.ng();
    int rc, done = 0;
    for (int z = 0; z < 2; ++z) {
        const void* const src[3] = {P.draw + 3 * (size_t)z * P.pb, P.draw + (3 * (size_t)z + 1) * P.pb, P.draw + (3 * (size_t)z + 2) * P.pb};
        if ((rc = rdn0mv_legs_of(p, q, S, src, P.legs[1 + z], lb, a.wl, a.rl, pl, my, st, &done))) return rc;
    }
    if (!done && (rc = qe_legs_pass2_w(p, P.legs[1], 2 * np, (long)(lb / es), a.wl, pl, st, my))) return rc;
    const double s = 1.0 / ((double)p->ny * p->nx), sy = my ? (double)p->ny / my : 1.0;
    // the chains' pieces: triples 0 = d, 1 = s, 2 = s'
    std::vector<const void*> cgx, cgy, chh;
    std::vector<void*> cpx, cpy;
    std::vector<double> csc;
    std::vector<int> first(2 * nest), cnt(2 * nest);
    static const int pairs[2][2][2] = {{{0, 1}, {1, 0}}, {{1, 2}, {2, 1}}};       // [A | B][half][X, Y]
    for (int set = 0; set < 2; ++set)
        for (int e = 0, base = 0; e < nest; base += a.npieces[e], ++e) {
            const int c = set * nest + e;
            first[c] = (int)cgx.size(); cnt[c] = 2 * a.npieces[e];
            for (int half = 0; half < 2; ++half)
                for (int i = 0; i < a.npieces[e]; ++i) {
                    const int idx = base + i, X = pairs[set][half][0], Y = pairs[set][half][1];
                    const bool sw = a.swap && a.swap[idx];
                    const char* const G = P.legs[sw ? Y : X] + 2 * (size_t)S.gslot[idx] * lb;
                    cgx.push_back(G); cgy.push_back(G + lb);
                    chh.push_back(P.legs[sw ? X : Y] + (2 * (size_t)ng + S.hslot[idx]) * lb);
                    cpx.push_back(P.prod + 2 * (size_t)c * lbk); cpy.push_back(P.prod + (2 * (size_t)c + 1) * lbk);
                    csc.push_back(a.signs[idx] * s * s * sy);
                }
        }
    const int total = (int)cgx.size();                                            // 4 x the set's pieces
    const size_t eb = qe_rows_table_entry_bytes(p);
    auto fits = [&](int pieces, int chains) { return ((size_t)pieces * eb + 15) / 16 * 16 + 2 * (size_t)chains * sizeof(int) <= MV_RTAB_BYTES; };
    bool chained = false;
    if (q->opt_mv_chain && fits(total / 2, nest)) {
        // ONE launch over the 2 nest chains where the table holds them, else the A chains and the B chains in a launch each
        const int nl = fits(total, 2 * nest) ? 1 : 2, nc = 2 * nest / nl;
        for (int l = 0; l < nl; ++l) {
            const int c0 = l * nc, p0 = first[c0], npc = (l + 1 < nl ? first[c0 + nc] : total) - p0;
            std::vector<int> fl(nc);
            for (int c = 0; c < nc; ++c) fl[c] = first[c0 + c] - p0;
            std::vector<unsigned long long> key;
            for (int i = p0; i < p0 + npc; ++i) {
                unsigned long long bits;
                memcpy(&bits, &csc[i], sizeof bits);
                key.insert(key.end(), {(unsigned long long)(uintptr_t)cgx[i], (unsigned long long)(uintptr_t)chh[i], (unsigned long long)(uintptr_t)cpx[i], bits});
            }
            for (int c = 0; c < nc; ++c) key.push_back((unsigned long long)cnt[c0 + c]);
            key.insert(key.end(), {(unsigned long long)my, (unsigned long long)(unsigned)a.mrow, (unsigned long long)p->dtype, 0x4D02ull});
            rc = qe_rows_chain_w(p, nc, npc, cgx.data() + p0, cgy.data() + p0, chh.data() + p0, cpx.data() + p0, cpy.data() + p0, csc.data() + p0, fl.data(),
                                 cnt.data() + c0, q->mv_rtab, key != q->mv_rkey, a.wl, a.wk, a.mrow, pl, pk, st, my);
            if (rc < 0) break;                         // (only at l = 0, before anything is launched: this geometry's row stage is another kernel)
            if (rc) return rc;
            q->mv_rkey = key;
            chained = l + 1 == nl;
        }
    }
    if (!chained)                                      // piece by piece; the second and later pieces of a chain accumulate
        for (int c = 0; c < 2 * nest; ++c)
            for (int i = first[c]; i < first[c] + cnt[c]; ++i)
                if ((rc = qe_rows_w(p, cgx[i], cgy[i], chh[i], cpx[i], cpy[i], csc[i], i > first[c], a.wl, a.wk, a.mrow, pl, pk, st, my))) return rc;
    long fn_moff = 0;
    if (mv_div_batched(q, nest, a.Fn, es / 2, &fn_moff)) {
        for (int set = 0; set < 2; ++set)
            if ((rc = qe_cols_div_batch_w(p, P.prod + 2 * (size_t)set * nest * lbk, P.prod + (2 * (size_t)set * nest + 1) * lbk, a.Fn[0],
                                          P.kappa + (size_t)set * nest * P.pb, P.tmp + 2 * (size_t)set * nest * lbk, nest, (long)(2 * lbk / es), fn_moff,
                                          plane_elems(p), a.wk, a.rk, pk, st, my))) return rc;
    } else {
        for (int c = 0; c < 2 * nest; ++c)
            if ((rc = qe_cols_div_w(p, P.prod + 2 * (size_t)c * lbk, P.prod + (2 * (size_t)c + 1) * lbk, a.Fn[c % nest], P.kappa + (size_t)c * P.pb, 0, a.wk,
                                    a.rk, pk, st, my))) return rc;
    }
    return rdn0mv_tail(p->dtype, P.kappa, plane_elems(p), a.w, a.wstride, nest, a.nspec, a.a, a.b, p->ny, p->kp, p->nx / 2, a.ids, a.nids, a.norm, a.wk,
                       a.rk, a.counts, P.scratch, a.n, a.S, a.C, st);
}
}  // namespace oa

extern "C" {

int oa_mc_mv_band_bind(oa_plan* p, const void* mv_weights, long mv_wstride, int nest, const int32_t* ids_hc, int nids, int nspec_max) {
    OA_REQUIRE(p && ids_hc, "oa_mc_mv_band_bind: NULL argument");
    OA_REQUIRE(nest >= 1 && nest <= 6, "oa_mc_mv_band_bind: 1 <= nest <= 6 estimators");
    OA_REQUIRE(nids >= 3, "oa_mc_mv_band_bind: nids must be at least 3 (two outer bins around the bandpowers)");
    OA_REQUIRE(!mv_weights || mv_wstride >= (long)p->ny * p->kp, "oa_mc_mv_band_bind: weight planes closer than one hc-real plane");
    if (p->pow2) return 0;                          // power-of-two plans take their planes per call
    OA_REQUIRE(p->mixed, "oa_mc_mv_band_bind: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path "
               "(mc.GaussianN0MonteCarloPol with one_call=False runs the host loop of the existing entries)");
    return mc_mv_bind(p, pipe_of(p), mv_weights, mv_wstride, nest, ids_hc, nids, nspec_max);
}

int oa_qe_band_bind(oa_plan* p, int nfilters, const void* const* host_filters, int nnorms, const void* const* host_Fnorm, int leg_cols,
                    int kappa_cols, int leg_rows, int kappa_rows, int mrow, int mcol, int max_leg_planes) {
    OA_REQUIRE(p && host_filters && host_Fnorm && nfilters >= 1 && nfilters <= 256 && nnorms >= 1 && nnorms <= 64 && max_leg_planes >= 0,
               "oa_qe_band_bind: bad argument");
    for (int i = 0; i < nfilters; ++i) OA_REQUIRE(host_filters[i], "oa_qe_band_bind: NULL filter plane");
    for (int i = 0; i < nnorms; ++i) OA_REQUIRE(host_Fnorm[i], "oa_qe_band_bind: NULL normalisation plane");
    if (p->pow2) return 0;                          // power-of-two plans take their planes per call
    OA_REQUIRE(p->mixed, "oa_qe_band_bind: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path "
               "(use the modular oa_qe_legs / oa_mul_real / oa_qe_div calls)");
    OA_REQUIRE(p->have_laxes, "oa_qe_band_bind: call oa_plan_set_laxes first");
    return pol_bind(p, pipe_of(p), nfilters, host_filters, nnorms, host_Fnorm, leg_cols, kappa_cols, leg_rows, kappa_rows, mrow, mcol, max_leg_planes);
}

int oa_qe_band_grid(const oa_plan* p, int* my, int* mx) {
    OA_REQUIRE(p && my && mx, "oa_qe_band_grid: NULL argument");
    const Pipeline* q = (const Pipeline*)p->pipe;
    const bool bound = q && q->pb.bound;
    *my = bound ? q->pb.my : 0;
    *mx = bound ? q->pb.mx : 0;
    return 0;
}

int oa_mc_run(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, int64_t* n, double* S, double* C,
              double* meanfield_acc, void* stream) {
    OA_REQUIRE(p && p->pipe && ((Pipeline*)p->pipe)->FG && ((Pipeline*)p->pipe)->ids, "oa_mc_run: call oa_plan_set_filters and oa_plan_set_bins first");
    OA_REQUIRE(covsqrt_hc && n && S && C && sim_hi >= sim_lo, "oa_mc_run: bad argument");
    Pipeline* q = (Pipeline*)p->pipe;
    hipStream_t st = (hipStream_t)stream;
    if (p->mixed) return mixed_mc_run(p, q, base_seed, sim_lo, sim_hi, covsqrt_hc, n, S, C, meanfield_acc, st);
    // only the leg band of a realisation is ever read (col_legs: columns < wl, rows |ky index| < rl)
    McTtLoop T{p, p, q, p->pow2, 0, nullptr, nullptr, nullptr, q->kT, 0, false};
    T.source_batch = [=](long i, int B) { return grf_hc_band_batch(p, base_seed, (uint64_t)i, B, covsqrt_hc, q->mc_src.p, plane_elems(p), q->wl, q->rl, st); };
    T.source_one = [=](long i) { return oa_grf_hc_band(p, base_seed, (uint64_t)i, covsqrt_hc, q->kT, q->wl, q->rl, st); };
    return mc_tt_loop(T, sim_lo, sim_hi, n, S, C, meanfield_acc, st);
}

/* oa_rdn0_set_data (include/orphics_amd.h): the data map's three leg planes on the plan's coarse grid, kept for oa_mc_run_rdn0.  Set-up
 * entry: may allocate and synchronise.  On a band grid the leg band of kD goes to the inner plan's first input plane first. */
int oa_rdn0_set_data(oa_plan* p, const void* kD_hc, void* stream) {
    OA_REQUIRE(p && kD_hc, "oa_rdn0_set_data: NULL argument");
    OA_REQUIRE(p->pow2 || p->mixed, std::string("oa_rdn0_set_data: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no "
                                                "one-call path; ") + RDN0_HOW);
    OA_REQUIRE(p->pipe && ((Pipeline*)p->pipe)->FG, "oa_rdn0_set_data: call oa_plan_set_filters first");
    Pipeline* q = (Pipeline*)p->pipe;
    hipStream_t st = (hipStream_t)stream;
    q->rdn0_gen = 0;
    oa_plan* r = p;
    const void* src = kD_hc;
    if (p->mixed) {
        OA_REQUIRE(q->band && q->band->pipe, "oa_rdn0_set_data: the bound filters have no band grid on this plan (oa_plan_set_filters reports why)");
        band_options(q);
        r = q->band;
        void* bx = band_in(q, 0);
        if (int rc = band_copy(band_cx_kind(p), kD_hc, p->kp, p->ny, bx, r->kp, r->ny, q->wl, q->rl, 1.0, st)) return rc;
        src = bx;
    }
    Pipeline* rq = (Pipeline*)r->pipe;
    const long pl = work_pitch(r, rq->wl);
    const size_t lb = (size_t)pl * r->ny * elem_bytes(r);
    if (int rc = ensure_work(r, rq)) return rc;
    if (int rc = rq->rdn0_legs.reserve(3 * lb)) return rc;
    if (rq->ids)                                   // the shard's planes now, where the bins are known: its first call then allocates nothing
        if (int rc = rdn0_reserve(r, rq)) return rc;
    char* const L = rq->rdn0_legs.at();
    if (int rc = qe_legs_cols_w(r, src, src, rq->FG, rq->FH, L, L + lb, L + 2 * lb, rq->wl, rq->rl, pl, st, rq->my)) return rc;
    q->rdn0_gen = q->bind_gen;
    q->rdn0_my = rq->my;
    return 0;
}

/* oa_mc_run_rdn0 (include/orphics_amd.h): the RDN0 shard [sim_lo, sim_hi) on oa_mc_run's loop (mc_tt_loop) with its own source stage
 * (two draws per realisation) and its own tail (rdn0_batch / rdn0_one above).  Everything is refused before the first launch. */
int oa_mc_run_rdn0(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, int64_t* n, double* S, double* C,
                   void* stream) {
    hipStream_t st = (hipStream_t)stream;
    McTtLoop T;
    if (int rc = rdn0_tt_open("oa_mc_run_rdn0", nullptr, p, sim_lo, sim_hi, covsqrt_hc, n, S, C, st, &T)) return rc;
    Pipeline* q = (Pipeline*)p->pipe;
    oa_plan* r = T.run;
    void* const draw = T.rq->rdn0_pool.p;
    auto source = [=](long i, int nreal) {          // draws 2 i .. 2 i + nreal - 1: the leg band of oa_grf_hc's plane, oa_mc_run's counters
        if (p->mixed) return grf_band_inner(p, base_seed, 2 * (uint64_t)i, nreal, covsqrt_hc, draw, r->ny, r->kp, plane_elems(r), q->wl, q->rl, st);
        return grf_hc_band_batch(p, base_seed, 2 * (uint64_t)i, nreal, covsqrt_hc, draw, plane_elems(p), q->wl, q->rl, st);
    };
    T.source_batch = [=](long i, int B) { return source(i, 2 * B); };
    T.source_one = [=](long i) { return source(i, 2); };
    return mc_tt_loop(T, sim_lo, sim_hi, n, S, C, nullptr, st);
}

/* oa_mc_run_rdn0_windowed (include/orphics_amd.h): oa_mc_run_rdn0 with the WINDOWED draws of oa_mc_run_windowed as s and s' -- the shard
 * loop and the tail are oa_mc_run_rdn0's (rdn0_tt_open), the source stage is that entry's (WinDraws above) with streams 2 i .. 2 i + 2 B - 1
 * of a batch onto the draw planes of rdn0_pool.  No mean field: s, s' and d are independent and zero-mean, so neither A nor B has an
 * ensemble mean to subtract.
 * POWER-OF-TWO PLANS: WinDraws::pow2 with OA_OPT_DRAW_FUSED (default: on), the 2 B compact row planes behind the tail's region of the pool.
 * BAND GRID: WinDraws::band, the batch's two halves of B draws each through the six N-grid planes of bwin.
 * OA_OPT_WIN_FUSED = 0 (on a band grid: also its rule by row length): one by one, both draws through the unfused flow. */
int oa_mc_run_rdn0_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, const void* window_real, int64_t* n,
                            double* S, double* C, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    McTtLoop T;
    if (int rc = rdn0_tt_open("oa_mc_run_rdn0_windowed", window_real ? nullptr : "NULL window (oa_mc_run_rdn0 is the entry without one)", p, sim_lo,
                              sim_hi, covsqrt_hc, n, S, C, st, &T)) return rc;
    Pipeline* q = (Pipeline*)p->pipe;
    oa_plan* r = T.run;
    Pipeline* rq = T.rq;
    char* const draw = rq->rdn0_pool.at();
    const size_t pbr = plane_bytes(r);
    WinDraws W{p, q, base_seed, covsqrt_hc, window_real, st};
    // a batch is started only where the chain row stage finishes it: with a window the source stage is most of a realisation, and a batch
    // abandoned at the row stage (mc_tt_loop's fallback) would have run it for up to six realisations in vain
    const bool chain = qe_rows_chain_ok(r, rq->wl, rq->wk, rq->mrow, rq->my);
    if (p->mixed) {
        if (int rc = W.band_open()) return rc;
        T.batched = W.fused && chain;
        T.source_batch = [=](long i, int B) {           // (a launch of its own for each half, B <= 6 planes)
            if (int rc = W.band(2 * (uint64_t)i, B, draw, plane_elems(r))) return rc;
            return W.band(2 * (uint64_t)i + B, B, draw + (size_t)B * pbr, plane_elems(r));
        };
        T.source_one = [=](long i) {
            if (W.fused) return W.band(2 * (uint64_t)i, 2, draw, plane_elems(r));
            if (int rc = W.band_map(2 * (uint64_t)i, draw)) return rc;
            return W.band_map(2 * (uint64_t)i + 1, draw + pbr);
        };
        return mc_tt_loop(T, sim_lo, sim_hi, n, S, C, nullptr, st);
    }
    W.fused = q->opt_win_fused;
    W.dfused = W.fused && (q->opt_draw_fused < 0 ? DRAW_FUSED_DEFAULT : q->opt_draw_fused != 0);
    T.batched = W.fused && chain;
    T.pool_extra = mc_pool_bytes(p, q, 1) + 2 * work_pitch(p, q->wl) * p->ny * elem_bytes(p);      // the tail's region, then the batch's 2 B compact row planes
    if (int rc = ensure_pool(q, (size_t)MC_BATCH_MAX * T.pool_extra + mc_pool_bytes(p, q, MC_BATCH_MAX))) return rc;      // (first call only)
    auto source = [=](long i, int B) { return W.pow2(2 * (uint64_t)i, 2 * B, q->split_legs.at(2 * mc_pool_bytes(p, q, B)), draw); };
    T.source_batch = source;
    T.source_one = [=](long i) {
        if (W.fused) return source(i, 1);
        if (int rc = W.pow2_map(2 * (uint64_t)i, draw)) return rc;
        return W.pow2_map(2 * (uint64_t)i + 1, draw + pbr);
    };
    return mc_tt_loop(T, sim_lo, sim_hi, n, S, C, nullptr, st);
}

/* oa_mc_run_mv (include/orphics_amd.h): the Gaussian N0 Monte-Carlo shard of an estimator SET.  Per realisation (mc_mv_loop): the leg band
 * of oa_grf_mix's T, E, B draw (streams 3 i, 3 i + 1, 3 i + 2) into three entry-owned planes -- not the plan's work planes: c[0..2], g[0..1]
 * and kT are where the one-launch divergence puts the per-estimator kappa_hat --, the launch sequence of oa_qe_mv with the sum left out
 * (qe_mv_pow2), one oa_bin_power_multi pass over the estimators' planes, one moment launch.  On a 2^a 3^b 5^c plan the same loop runs on
 * the inner plan of the band grid (mc_mv_shard). */
int oa_mc_run_mv(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest, const int* host_npieces,
                 const double* host_signs, const void* const* host_FG, const void* const* host_FH, const int* host_swap, const int* host_xsrc,
                 const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights, long mv_wstride, int nspec, const int* host_a,
                 const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts, double norm, int leg_cols, int kappa_cols,
                 int leg_rows, int kappa_rows, int mrow, int64_t* n, double* S, double* C, void* stream) {
    const McMvArgs a{base_seed, sim_lo, sim_hi, host_covsqrt, nest, host_npieces, host_signs, host_FG, host_FH, host_swap, host_xsrc, host_ysrc,
                     host_Fnorm, mv_weights, mv_wstride, nspec, host_a, host_b, ids_hc, nids, counts, norm, leg_cols, kappa_cols, leg_rows,
                     kappa_rows, mrow, n, S, C, (hipStream_t)stream, nullptr, nullptr, nullptr, nullptr};
    if (int rc = mc_mv_check("oa_mc_run_mv", ": map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path; "
                             "run the host loop of the existing entries (mc.GaussianN0MonteCarloPol with one_call=False: Engine.grf_mix, reconstruct_hc per "
                             "estimator, Engine.bin_power, Statistics.add)", p, a))
        return rc;
    return mc_mv_shard("oa_mc_run_mv", false, p, a);
}

/* oa_mc_run_mv_windowed (include/orphics_amd.h): oa_mc_run_mv with a real-space window on T, Q, U and the mean-field stacks of the estimator
 * set.  The window multiplies Q and U, not E and B -- a taper leaks E into B, which is what the EB and TB noise on an apodised patch is made
 * of -- so the source stage of a windowed realisation is: full-plane draw of T, E, B rotated to T, Q, U in the same pass (the counters of the
 * band draw) -> one batched inverse column launch -> one fused row launch over the three planes (C2R / Npix -> x window -> R2C, the real maps
 * in LDS only, leg_cols columns stored at the compact pitch) -> one batched forward column launch onto the leg band of the loop's three
 * source planes -> Q, U -> E, B on that band.  OA_OPT_WIN_FUSED = 0: oa_fft_c2r_windowed -> real maps in HBM (the column temporaries) ->
 * oa_fft_r2c on the band.  Then mc_mv_loop's estimator, binning and moment steps, and one stack launch.
 * On a 2^a 3^b 5^c plan the loop runs on the inner plan of the band grid behind oa_qe_band_bind + oa_mc_mv_band_bind, with the windowed
 * source stage on the N grid in front of it and the stacks on the N grid behind it (mc_mv_shard, mv_window_source_band). */
int oa_mc_run_mv_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest,
                          const int* host_npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH,
                          const int* host_swap, const int* host_xsrc, const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights,
                          long mv_wstride, int nspec, const int* host_a, const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts,
                          double norm, int leg_cols, int kappa_cols, int leg_rows, int kappa_rows, int mrow, const void* window_real,
                          const void* rot_c, const void* rot_s, int64_t* n, double* S, double* C, double* const* host_meanfield, void* stream) {
    const McMvArgs a{base_seed, sim_lo, sim_hi, host_covsqrt, nest, host_npieces, host_signs, host_FG, host_FH, host_swap, host_xsrc, host_ysrc,
                     host_Fnorm, mv_weights, mv_wstride, nspec, host_a, host_b, ids_hc, nids, counts, norm, leg_cols, kappa_cols, leg_rows,
                     kappa_rows, mrow, n, S, C, (hipStream_t)stream, window_real, rot_c, rot_s, host_meanfield};
    if (int rc = mc_mv_check("oa_mc_run_mv_windowed", ": map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path; run "
                             "the host loop of the existing entries (mc.GaussianN0MonteCarloPol with one_call=False: Engine.grf_mix, Engine.irfft with "
                             "the window, Engine.rfft, Engine.rot2, reconstruct_hc per estimator, Engine.bin_power, Statistics.add)", p, a))
        return rc;
    OA_REQUIRE(!window_real || (rot_c && rot_s), "oa_mc_run_mv_windowed: a window acts on Q and U and needs both rotation planes rot_c, rot_s (cos / sin "
               "2 phi_l on the half plane, oa_qe_mv_maps' convention: what mc.GaussianN0MonteCarloPol passes, and what its one_call=False host "
               "loop rotates with)");
    if (host_meanfield)
        for (int e = 0; e < nest + (mv_weights ? 1 : 0); ++e) OA_REQUIRE(host_meanfield[e], "oa_mc_run_mv_windowed: NULL mean-field stack plane");
    return mc_mv_shard("oa_mc_run_mv_windowed", true, p, a);
}

/* oa_rdn0_set_data_mv (include/orphics_amd.h): the data triple's distinct leg planes (rdn0mv_slots) on the column grid of the set's bands,
 * transformed once and kept for oa_mc_run_rdn0_mv.  Set-up entry: may allocate and synchronise.  On a 2^a 3^b 5^c plan: on the inner plan of
 * the current oa_qe_band_bind binding (rdn0mv_set_data_band). */
static const char* const RDN0MV_HOW = "; run the host loop of the existing entries (mc.RDN0MonteCarloPol with one_call=False)";
static const char* const RDN0MV_CZT = ": map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call path -- the one-call "
                                      "RDN0 of an estimator set runs on power-of-two sides and on the band grid of sides 2^a 3^b 5^c";
static const char* const RDN0MV_BIND = ": on map sides that are not power-of-two the estimator set is bound first (oa_qe_band_bind, then "
                                       "oa_mc_mv_band_bind) and the entry runs on that binding's band grid";
// ... on the band grid of the current oa_qe_band_bind binding (whose bands and row grid are the call's: checked by the caller)
static int rdn0mv_set_data_band(const std::string& who, oa_plan* p, Pipeline* q, const void* const* host_kD, int nest, const int* host_npieces,
                                const void* const* host_FG, const void* const* host_FH, const int* host_swap, const int* host_xsrc,
                                const int* host_ysrc, int wl, int wk, int rl, int rk, int mrow, hipStream_t st) {
    Pipeline::PolBind& B = q->pb;
    oa_plan* b = B.plan;
    Pipeline* qb = (Pipeline*)b->pipe;
    band_options(q);
    const size_t rb = band_real_bytes(b), cb = plane_bytes(b), es = elem_bytes(b);
    char* const fbase = B.planes.at();
    char* const sbase = fbase + (B.fkey.size() + B.nkey.size()) * rb;
    int total = 0;
    for (int e = 0; e < nest; ++e) total += host_npieces[e];
    std::vector<const void*> iFG(total), iFH(total);
    for (int i = 0; i < total; ++i) {
        iFG[i] = pol_inner(B.fkey, host_FG[i], fbase, rb);
        iFH[i] = pol_inner(B.fkey, host_FH[i], fbase, rb);
        if (!iFG[i] || !iFH[i])
            return fail(who + ": a filter plane of this call is not bound (oa_qe_band_bind binds every distinct plane)" + RDN0MV_HOW);
    }
    // the caller's planes number the slots and make the key; the inner copies (one per distinct bound plane) number alike
    const Rdn0MvSlots S = rdn0mv_slots(nest, host_npieces, host_FG, host_FH, host_swap, host_xsrc, host_ysrc);
    const Rdn0MvSlots Si = rdn0mv_slots(nest, host_npieces, iFG.data(), iFH.data(), host_swap, host_xsrc, host_ysrc);
    OA_REQUIRE(Si.ng() == S.ng() && Si.nh() == S.nh(), who + ": a filter plane is bound twice (oa_qe_band_bind binds every DISTINCT plane)" + RDN0MV_HOW);
    const void* any = nullptr;
    for (const auto& g : S.grad) { OA_REQUIRE(host_kD[g.first], who + ": NULL data plane of a source an estimator reads"); any = host_kD[g.first]; }
    for (const auto& h : S.hpl) OA_REQUIRE(host_kD[h.first], who + ": NULL data plane of a source an estimator reads");
    int my = 0;
    if (int rc = resolve_my(b, qb->mcol, rl, rk, &my)) return rc;                  // (pol_bind's resolution: the table exists)
    const long pl = work_pitch(b, wl);
    const size_t lb = (size_t)pl * b->ny * es;
    // everything the shard would otherwise take: the leg planes of d, the pool of s, s' and the chains, the draw / kappa / tail planes
    // (the tail's scratch for the Monte-Carlo binding's nspec_max x nids where that binding exists already), the device tables
    if (int rc = qb->rdn0mv_legs.reserve((size_t)S.nplanes() * lb)) return rc;
    if (int rc = ensure_pool(qb, rdn0mv_split_bytes(b, Si, nest, wl, wk))) return rc;
    const Pipeline::PolBind::McBind& M = B.mc;
    const size_t tail = M.bound ? rdn0mv_scratch_bytes(b->ny, rk, M.nspec_max, M.nids) : 0;     // (nspec_max <= 28, nids >= 3: checked by that entry)
    if (int rc = qb->rdn0mv_pool.reserve((6 + 2 * (size_t)nest) * cb + tail, true)) return rc;
    if (!qb->mv_ftab) OA_HIP(hipMalloc((void**)&qb->mv_ftab, 32 * sizeof(void*)));
    if (!qb->mv_rtab) OA_HIP(hipMalloc(&qb->mv_rtab, MV_RTAB_BYTES));
    // the leg band of the data transforms -> the binding's first three inner source planes (zero outside the band), source index = plane
    std::vector<const void*> srcs(3);
    for (int i = 0; i < 3; ++i) srcs[i] = host_kD[i] ? host_kD[i] : any;
    if (int rc = mv_sources_embed(p, B, srcs, sbase, cb, wl, rl, st)) return rc;
    const void* const isrc[3] = {sbase, sbase + cb, sbase + 2 * cb};
    int done = 0;
    if (int rc = rdn0mv_legs_of(b, qb, Si, isrc, qb->rdn0mv_legs.at(), lb, wl, rl, pl, my, st, &done)) return rc;
    if (!done)
        if (int rc = qe_legs_pass2_w(b, qb->rdn0mv_legs.p, Si.nplanes(), (long)(lb / es), wl, pl, st, my)) return rc;
    q->rdn0mv_key = S.key();
    const int band[5] = {wl, wk, rl, rk, mrow};
    std::copy(band, band + 5, q->rdn0mv_band);
    q->rdn0mv_my = my;
    q->rdn0mv_gen = B.gen;
    return 0;
}
int oa_rdn0_set_data_mv(oa_plan* p, const void* const* host_kD, int nest, const int* host_npieces, const void* const* host_FG,
                        const void* const* host_FH, const int* host_swap, const int* host_xsrc, const int* host_ysrc, int leg_cols, int kappa_cols,
                        int leg_rows, int kappa_rows, int mrow, void* stream) {
    const std::string who = "oa_rdn0_set_data_mv";
    OA_REQUIRE(p && host_kD && host_npieces && host_FG && host_FH && host_xsrc && host_ysrc, who + ": NULL argument");
    OA_REQUIRE(p->pow2 || p->mixed, who + RDN0MV_CZT + RDN0MV_HOW);
    if (p->mixed) {
        Pipeline* q = pipe_of(p);
        q->rdn0mv_key.clear();
        OA_REQUIRE(q->pb.bound, who + RDN0MV_BIND + RDN0MV_HOW);
    }
    if (int rc = rdn0mv_set_check(who, p, nest, host_npieces, host_FG, host_FH, host_xsrc, host_ysrc, leg_cols, kappa_cols, leg_rows, kappa_rows)) return rc;
    OA_REQUIRE(p->have_laxes, who + ": call oa_plan_set_laxes first");
    Pipeline* q = pipe_of(p);
    hipStream_t st = (hipStream_t)stream;
    q->rdn0mv_key.clear();
    if (p->mixed) {
        const Pipeline::PolBind& B = q->pb;
        OA_REQUIRE(leg_cols == B.wl && kappa_cols == B.wk && leg_rows == B.rl && kappa_rows == B.rk && mrow == B.mrow,
                   who + ": leg / kappa columns and rows or the row grid differ from the bound ones (call oa_qe_band_bind for this band)" + RDN0MV_HOW);
        return rdn0mv_set_data_band(who, p, q, host_kD, nest, host_npieces, host_FG, host_FH, host_swap, host_xsrc, host_ysrc, leg_cols, kappa_cols,
                                    leg_rows, kappa_rows, mrow, st);
    }
    const Rdn0MvSlots S = rdn0mv_slots(nest, host_npieces, host_FG, host_FH, host_swap, host_xsrc, host_ysrc);
    for (const auto& g : S.grad) OA_REQUIRE(host_kD[g.first], who + ": NULL data plane of a source an estimator reads");
    for (const auto& h : S.hpl) OA_REQUIRE(host_kD[h.first], who + ": NULL data plane of a source an estimator reads");
    if (int rc = ensure_work(p, q)) return rc;
    int my = 0;
    if (int rc = resolve_my(p, mrow == 0 ? 0 : q->mcol, leg_rows, kappa_rows, &my)) return rc;
    const long pl = work_pitch(p, leg_cols);
    const size_t es = elem_bytes(p), lb = (size_t)pl * p->ny * es;
    if (int rc = q->rdn0mv_legs.reserve((size_t)S.nplanes() * lb)) return rc;
    // the shard's planes that do not depend on the bins, now: its first call then takes the tail's scratch only
    if (int rc = ensure_pool(q, rdn0mv_split_bytes(p, S, nest, leg_cols, kappa_cols))) return rc;
    if (!q->mv_ftab) OA_HIP(hipMalloc((void**)&q->mv_ftab, 32 * sizeof(void*)));
    if (!q->mv_rtab) OA_HIP(hipMalloc(&q->mv_rtab, MV_RTAB_BYTES));
    int done = 0;
    if (int rc = rdn0mv_legs_of(p, q, S, host_kD, q->rdn0mv_legs.at(), lb, leg_cols, leg_rows, pl, my, st, &done)) return rc;
    if (!done)
        if (int rc = qe_legs_pass2_w(p, q->rdn0mv_legs.p, S.nplanes(), (long)(lb / es), leg_cols, pl, st, my)) return rc;
    q->rdn0mv_key = S.key();
    const int band[5] = {leg_cols, kappa_cols, leg_rows, kappa_rows, mrow};
    std::copy(band, band + 5, q->rdn0mv_band);
    q->rdn0mv_my = my;
    return 0;
}

// the default of OA_OPT_DRAW_FUSED for oa_mc_run_rdn0_mv_windowed (its own constant: the rule is the TT entry's, the kernel is another):
// 1 only once oa_grf_mix_icols has measured faster per triple than grf_mix_teb_to_tqu + the batched inverse columns beyond both 10th - 90th
// spreads at every measured geometry (tools/rdn0_pol_bench.py --windowed).  No such measurement is recorded yet, so the default
// is the per-triple sequence; OA_OPT_DRAW_FUSED = 1 opts in, and the moments are bit-equal either way
constexpr bool DRAW_FUSED_DEFAULT_RDN0_MV = false;
/* oa_mc_run_rdn0_mv on a 2^a 3^b 5^c plan (the caller has checked the arguments and that oa_qe_band_bind bound the plan): every pointer of
 * the call is looked up in the two bindings (mixed_mc_mv_lookup's checks under this entry's name), the data legs must be those of the current
 * binding, and everything is refused before the first launch.  Then, per realisation, ONE draw launch puts T, E, B of s and of s' on the leg
 * band of six contiguous inner planes (oa_grf_mix_band_inner_triples: the N grid's counters, edge rules and covsqrt) and rdn0mv_one runs on
 * the inner plan with the inner filters, normalisations (they carry My Mx / (ny nx)), weights and ids, mrow and column grid as pol_bind
 * resolved them, and the caller's counts, those of the N plane.  As in oa_mc_run_mv there, the tail's note holds: since Mx >= 2 kappa_cols the
 * inner Nyquist column is never visited, so column 0 is the only visited one of Hermitian multiplicity 1, as on the N grid.  Nothing is
 * allocated here after oa_rdn0_set_data_mv behind both bindings (the reservations below find their planes), nothing synchronises. */
static int rdn0mv_shard_band(const std::string& who, oa_plan* p, const McMvArgs& a) {
    static const std::string how = std::string(" -- bind the estimator set with oa_qe_band_bind, then oa_mc_mv_band_bind, then call oa_rdn0_set_data_mv") +
                                   RDN0MV_HOW;
    Pipeline* q = pipe_of(p);
    MvShard c;
    if (int rc = mixed_mc_mv_lookup(who, true, p, q, a, &c, how.c_str())) return rc;
    Pipeline::PolBind& B = q->pb;
    oa_plan* b = B.plan;
    Pipeline* qb = (Pipeline*)b->pipe;
    OA_REQUIRE(!q->rdn0mv_key.empty(), who + ": no data set: call oa_rdn0_set_data_mv with this estimator set first" + RDN0MV_HOW);
    const Rdn0MvSlots SL = rdn0mv_slots(a.nest, a.npieces, a.FG, a.FH, a.swap, a.xsrc, a.ysrc);
    const Rdn0MvSlots Si = rdn0mv_slots(a.nest, a.npieces, c.iFG.data(), c.iFH.data(), a.swap, a.xsrc, a.ysrc);
    const int band[5] = {a.wl, a.wk, a.rl, a.rk, a.mrow};
    int my = 0;
    if (int rc = resolve_my(b, qb->mcol, a.rl, a.rk, &my)) return rc;
    OA_REQUIRE(q->rdn0mv_gen == B.gen && qb->rdn0mv_legs.p && SL.key() == q->rdn0mv_key && Si.nplanes() == SL.nplanes() && std::equal(band, band + 5, q->rdn0mv_band) &&
               my == q->rdn0mv_my,
               who + ": the data legs are stale -- oa_qe_band_bind was called since they were made, or the filter planes, the bands, the row grid or "
               "the inner column grid differ from those of oa_rdn0_set_data_mv: call oa_rdn0_set_data_mv again" + RDN0MV_HOW);
    const size_t cb = plane_bytes(b);
    if (int rc = qb->rdn0mv_pool.reserve((6 + 2 * (size_t)a.nest) * cb + rdn0mv_scratch_bytes(b->ny, a.rk, a.nspec, a.nids), true)) return rc;
    if (int rc = ensure_pool(qb, rdn0mv_split_bytes(b, Si, a.nest, a.wl, a.wk))) return rc;
    McMvArgs ai = a;                                // the call in the inner plan's layout
    ai.FG = c.iFG.data(); ai.FH = c.iFH.data(); ai.Fn = c.iFn.data();
    ai.w = c.L.w; ai.wstride = c.L.wstride; ai.ids = c.L.ids; ai.mrow = c.L.mrow;
    const Rdn0MvPlanes P = rdn0mv_planes(b, qb, Si, a.nest, a.wl, a.wk);
    void* out[6];
    for (int i = 0; i < 6; ++i) out[i] = P.draw + (size_t)i * cb;
    for (long i = a.sim_lo; i < a.sim_hi; ++i) {
        if (int rc = oa_grf_mix_band_inner_triples(p, a.base_seed, 6 * (uint64_t)i, 2, a.covsqrt, 1.0, out, b->ny, b->kp, a.wl, a.rl, a.st)) return rc;
        if (int rc = rdn0mv_one(b, qb, ai, Si, P, my)) return rc;
    }
    return 0;
}
/* The body of oa_mc_run_rdn0_mv and oa_mc_run_rdn0_mv_windowed: every refusal under the caller's name before the first launch, then one
 * realisation at a time -- the source stage puts T, E, B of s and of s' on the leg band of the six planes of P.draw, then rdn0mv_one.
 * No window: the two band draws (streams 6 i .. 6 i + 2 and 6 i + 3 .. 6 i + 5).  Window (a.window, a.rot_c, a.rot_s), on planes of
 * q->mvwin (6 full hc planes | 6 compact row planes; the per-triple arms use mv_window_triple_pow2's layout inside it):
 *   OA_OPT_WIN_FUSED = 1, OA_OPT_DRAW_FUSED = 1: ONE pass-1 launch with both triples' draws at its load + ONE in-place pass 2
 *     (oa_grf_mix_icols, ntriples = 2), ONE fused row launch over the six planes, ONE forward column launch over six, Q, U -> E, B per pair;
 *   OA_OPT_DRAW_FUSED = 0: oa_mc_run_mv_windowed's fused sequence per triple;   OA_OPT_WIN_FUSED = 0: its unfused flow per triple. */
static int rdn0mv_shard(const std::string& who, oa_plan* p, const McMvArgs& a) {
    const long sim_lo = a.sim_lo, sim_hi = a.sim_hi;
    OA_REQUIRE(p && a.covsqrt && a.npieces && a.signs && a.FG && a.FH && a.xsrc && a.ysrc && a.Fn && a.ids && a.counts && a.n && a.S && a.C &&
               a.sim_hi >= a.sim_lo, who + ": bad argument");
    // (the windowed entry is not on the band grid: its power-of-two form has not been timed against the host loop yet)
    if (a.window)
        OA_REQUIRE(p->pow2, who + ": the one-call RDN0 of an estimator set runs on power-of-two map sides only (not on the band grid of sides 2^a 3^b 5^c "
                   "yet, nor on chirp-z sides)" + RDN0MV_HOW);
    OA_REQUIRE(p->pow2 || p->mixed, who + RDN0MV_CZT + RDN0MV_HOW);
    if (p->mixed) OA_REQUIRE(pipe_of(p)->pb.bound, who + RDN0MV_BIND + RDN0MV_HOW);
    if (int rc = rdn0mv_set_check(who, p, a.nest, a.npieces, a.FG, a.FH, a.xsrc, a.ysrc, a.wl, a.wk, a.rl, a.rk)) return rc;
    for (int e = 0; e < a.nest; ++e) OA_REQUIRE(a.Fn[e], who + ": NULL normalisation plane");
    OA_REQUIRE(!a.w || a.wstride >= (long)p->ny * p->kp, who + ": weight planes closer than one hc-real plane");
    if (int rc = rdn0mv_tail_check(who.c_str(), a.nest, a.w != nullptr, a.nspec, a.a, a.b, a.nids)) return rc;
    if (p->mixed) return rdn0mv_shard_band(who, p, a);
    Pipeline* q = pipe_of(p);
    OA_REQUIRE(!q->rdn0mv_key.empty() && q->rdn0mv_legs.p, who + ": no data set: call oa_rdn0_set_data_mv with this estimator set first" + RDN0MV_HOW);
    const Rdn0MvSlots SL = rdn0mv_slots(a.nest, a.npieces, a.FG, a.FH, a.swap, a.xsrc, a.ysrc);
    const int band[5] = {a.wl, a.wk, a.rl, a.rk, a.mrow};
    int my = 0;
    if (int rc = resolve_my(p, a.mrow == 0 ? 0 : q->mcol, a.rl, a.rk, &my)) return rc;
    OA_REQUIRE(SL.key() == q->rdn0mv_key && std::equal(band, band + 5, q->rdn0mv_band) && my == q->rdn0mv_my,
               who + ": the data legs are stale -- the filter planes, the bands, the row grid or the column grid (oa_plan_set_col_grid) differ from those "
               "of oa_rdn0_set_data_mv: call it again" + RDN0MV_HOW);
    if (int rc = ensure_work(p, q)) return rc;     // (nothing to do after oa_rdn0_set_data_mv)
    const size_t pb = plane_bytes(p), es = elem_bytes(p);
    if (int rc = q->rdn0mv_pool.reserve((6 + 2 * (size_t)a.nest) * pb + rdn0mv_scratch_bytes(p->ny, a.rk, a.nspec, a.nids), true)) return rc;
    if (int rc = ensure_pool(q, rdn0mv_split_bytes(p, SL, a.nest, a.wl, a.wk))) return rc;
    const long pl = work_pitch(p, a.wl), pe = plane_elems(p);
    const size_t lb = (size_t)pl * p->ny * es;
    if (a.window)
        if (int rc = q->mvwin.reserve(std::max(6 * pb + 6 * lb, mv_window_triple_bytes(p, a.wl)))) return rc;
    const bool fused = q->opt_win_fused;
    // (float64 plans of 32768 rows and more have no fused-draw kernel: the per-triple sequence, which is bit-equal)
    const bool dfused = fused && grf_mix_icols_serves(p) && (q->opt_draw_fused < 0 ? DRAW_FUSED_DEFAULT_RDN0_MV : q->opt_draw_fused != 0);
    const Rdn0MvPlanes P = rdn0mv_planes(p, q, SL, a.nest, a.wl, a.wk);
    for (long i = sim_lo; i < sim_hi; ++i) {
        if (a.window && dfused) {
            char* const wb = q->mvwin.at();
            char* const rowT = wb + 6 * pb;
            if (int rc = grf_mix_icols_w(p, a.base_seed, 6 * (uint64_t)i, 2, a.covsqrt, a.rot_c, a.rot_s, wb, pe, a.st)) return rc;
            if (int rc = qe_win_rows_w(p, wb, a.window, a.wl, pl, 1.0 / ((double)p->ny * p->nx), a.st, rowT, 6, pe, (long)(lb / es))) return rc;
            if (int rc = qe_fwd_cols_batch_w(p, rowT, pl, P.draw, 6, (long)(lb / es), pe, a.wl, a.rl, a.st)) return rc;
            for (int z = 0; z < 2; ++z)
                if (int rc = band_rot2(p->dtype, a.rot_c, a.rot_s, P.draw + (3 * (size_t)z + 1) * pb, P.draw + (3 * (size_t)z + 2) * pb, p->ny, p->kp,
                                       a.wl, a.rl, a.st)) return rc;
        } else {
            for (int z = 0; z < 2; ++z) {
                void* const out[3] = {P.draw + 3 * (size_t)z * pb, P.draw + (3 * (size_t)z + 1) * pb, P.draw + (3 * (size_t)z + 2) * pb};
                if (int rc = a.window ? mv_window_triple_pow2(p, a, fused, 6 * (uint64_t)i + 3 * z, q->mvwin.at(), out)
                                      : oa_grf_mix_band(p, a.base_seed, 6 * (uint64_t)i + 3 * z, 3, a.covsqrt, 1.0, out, a.wl, a.rl, a.st)) return rc;
            }
        }
        if (int rc = rdn0mv_one(p, q, a, SL, P, my)) return rc;
    }
    return 0;
}
/* oa_mc_run_rdn0_mv (include/orphics_amd.h): the RDN0 shard [sim_lo, sim_hi) of an estimator set, one realisation at a time (as mc_mv_loop):
 * the two band draws (streams 6 i .. 6 i + 2 and 6 i + 3 .. 6 i + 5) into entry-owned planes, then rdn0mv_one.  Everything is refused before
 * the first launch. */
int oa_mc_run_rdn0_mv(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest, const int* host_npieces,
                      const double* host_signs, const void* const* host_FG, const void* const* host_FH, const int* host_swap, const int* host_xsrc,
                      const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights, long mv_wstride, int nspec, const int* host_a,
                      const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts, double norm, int leg_cols, int kappa_cols,
                      int leg_rows, int kappa_rows, int mrow, int64_t* n, double* S, double* C, void* stream) {
    const McMvArgs a{base_seed, sim_lo, sim_hi, host_covsqrt, nest, host_npieces, host_signs, host_FG, host_FH, host_swap, host_xsrc, host_ysrc,
                     host_Fnorm, mv_weights, mv_wstride, nspec, host_a, host_b, ids_hc, nids, counts, norm, leg_cols, kappa_cols, leg_rows,
                     kappa_rows, mrow, n, S, C, (hipStream_t)stream, nullptr, nullptr, nullptr, nullptr};
    return rdn0mv_shard("oa_mc_run_rdn0_mv", p, a);
}

/* oa_mc_run_rdn0_mv_windowed (include/orphics_amd.h): oa_mc_run_rdn0_mv whose s and s' are the windowed triples of oa_mc_run_mv_windowed's
 * source stage (streams 6 i + 3 z .. + 2).  The window and its rotation planes are checked first, then rdn0mv_shard. */
int oa_mc_run_rdn0_mv_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest,
                               const int* host_npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH,
                               const int* host_swap, const int* host_xsrc, const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights,
                               long mv_wstride, int nspec, const int* host_a, const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts,
                               double norm, int leg_cols, int kappa_cols, int leg_rows, int kappa_rows, int mrow, const void* window_real,
                               const void* rot_c, const void* rot_s, int64_t* n, double* S, double* C, void* stream) {
    const std::string who = "oa_mc_run_rdn0_mv_windowed";
    const McMvArgs a{base_seed, sim_lo, sim_hi, host_covsqrt, nest, host_npieces, host_signs, host_FG, host_FH, host_swap, host_xsrc, host_ysrc,
                     host_Fnorm, mv_weights, mv_wstride, nspec, host_a, host_b, ids_hc, nids, counts, norm, leg_cols, kappa_cols, leg_rows,
                     kappa_rows, mrow, n, S, C, (hipStream_t)stream, window_real, rot_c, rot_s, nullptr};
    OA_REQUIRE(window_real, who + ": NULL window -- oa_mc_run_rdn0_mv is the entry without one" + RDN0MV_HOW);
    OA_REQUIRE(rot_c && rot_s, who + ": a window acts on Q and U and needs both rotation planes rot_c, rot_s (cos / sin 2 phi_l on the half plane, "
               "oa_mc_run_mv_windowed's convention: what mc.RDN0MonteCarloPol.set_window binds)" + RDN0MV_HOW);
    return rdn0mv_shard(who, p, a);
}

/* Monte-Carlo shard with a REAL-SPACE WINDOW (the reference's analysis flow multiplies every map by its apodisation taper
 * before any transform: maps.py:1873-1878 get_taper, maps.py:1350-1361 binned_power(imap * mask) / mean(mask^2)): per
 * realisation a FULL-plane Philox draw (key = (base_seed, sim), the same counters as oa_mc_run's band draw) -> C2R / Npix ->
 * x window -> TT estimator from the real map (row R2C on the active columns ...) -> bandpower moments (+ mean-field stack:
 * with a window the ensemble mean of kappa_hat no longer vanishes -- that is the mean field Statistics.add_stack exists
 * for, stats.py:1123-1150).  The real map lives in the plan's first leg plane, which the estimator overwrites only after its
 * row pass has consumed the map. */
int oa_mc_run_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, const void* window_real,
                       int64_t* n, double* S, double* C, double* meanfield_acc, void* stream) {
    OA_REQUIRE(p, "oa_mc_run_windowed: NULL plan");
    OA_REQUIRE(p->pow2 || p->mixed, "oa_mc_run_windowed: map sides with a prime factor other than 2, 3 and 5 (chirp-z transforms) have no one-call "
               "path; run the host loop of the existing entries (mc.GaussianN0MonteCarlo with one_call=False: Engine.grf_hc, Engine.irfft, "
               "x window, Estimator.tt_moments)");
    OA_REQUIRE(p->pipe && ((Pipeline*)p->pipe)->FG && ((Pipeline*)p->pipe)->ids, "oa_mc_run_windowed: call oa_plan_set_filters and oa_plan_set_bins first");
    OA_REQUIRE(covsqrt_hc && window_real && n && S && C && sim_hi >= sim_lo, "oa_mc_run_windowed: bad argument");
    Pipeline* q = (Pipeline*)p->pipe;
    hipStream_t st = (hipStream_t)stream;
    if (p->mixed) {
        OA_REQUIRE(q->band && q->band->pipe, "oa_mc_run_windowed: the bound filters have no band grid on this plan (oa_plan_set_filters reports why)");
        return mixed_mc_run_windowed(p, q, base_seed, sim_lo, sim_hi, covsqrt_hc, window_real, n, S, C, meanfield_acc, st);
    }
    // FUSED ROW PASS (default; WinDraws::pow2 without the draw inside the column pass): inverse columns of the drawn spectrum (into the
    // first leg plane, free until the leg stage), then C2R x window -> R2C per row in ONE kernel -- the real map exists in LDS only.
    // OA_OPT_WIN_FUSED = 0: C2R with the window at its store -> real map in HBM -> the from-map estimator path.
    WinDraws W{p, q, base_seed, covsqrt_hc, window_real, st, (bool)q->opt_win_fused};
    const size_t lb = (size_t)work_pitch(p, q->wl) * p->ny * elem_bytes(p);
    // BATCHES (fused row pass only): per realisation the full-plane part onto a compact row plane behind the tail's region of the pool,
    // then for the batch ONE forward column transform onto the leg band of its hc planes and the launches of oa_mc_run's batches behind
    // it: the latency-bound coarse-grid work of a realisation (70 of its 205 us at 4096^2 float) is shared by up to six.  ONE BY ONE: the
    // row transform on the scratch plane the column stages read (rows_done), or the real map in c[0].
    McTtLoop T{p, p, q, W.fused && p->pow2, lb, nullptr, nullptr, q->c[0], nullptr, W.fused ? 1 : 0, true};
    T.source_batch = [=](long i, int B) { return W.pow2((uint64_t)i, B, q->split_legs.at(mc_pool_bytes(p, q, B)), q->mc_src.p); };
    T.source_one = [=](long i) { return W.fused ? W.pow2((uint64_t)i, 1, nullptr, nullptr) : W.pow2_map((uint64_t)i, nullptr); };
    return mc_tt_loop(T, sim_lo, sim_hi, n, S, C, meanfield_acc, st);
}

// ---- device memory for hosts that bring no GPU array library (the reference is NumPy) -----------------------------
int oa_malloc(void** out, size_t bytes) {
    OA_REQUIRE(out, "oa_malloc: NULL");
    *out = nullptr;
    OA_HIP(hipMalloc(out, bytes ? bytes : 1));
    return 0;
}
int oa_free(void* dptr) {
    if (dptr) OA_HIP(hipFree(dptr));
    return 0;
}
/* kind: 1 = host -> device, 2 = device -> host, 3 = device -> device; stream-ordered (pageable host memory makes the
 * copy synchronous with respect to the host, as hipMemcpyAsync documents) */
int oa_memcpy(void* dst, const void* src, size_t bytes, int kind, void* stream) {
    OA_REQUIRE(dst && src, "oa_memcpy: NULL");
    const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : (kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    OA_REQUIRE(kind >= 1 && kind <= 3, "oa_memcpy: kind must be 1 (h2d), 2 (d2h) or 3 (d2d)");
    OA_HIP(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
    return 0;
}
int oa_memset(void* dptr, int value, size_t bytes, void* stream) {
    OA_REQUIRE(dptr, "oa_memset: NULL");
    OA_HIP(hipMemsetAsync(dptr, value, bytes, (hipStream_t)stream));
    return 0;
}
int oa_stream_synchronize(void* stream) {
    OA_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// ---- RCCL all-reduce (Statistics.allreduce, stats.py:1209-1230) for hosts without torch.distributed -------------
typedef struct { char internal[128]; } oa_rccl_id;
struct OaComm { void* comm; };
static void* rccl_sym(const char* name) {
    static void* lib = nullptr;
    if (!lib) {
        lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return nullptr;
    }
    return dlsym(lib, name);
}
#define OA_RCCL(fn, ...)                                                                          \
    do {                                                                                          \
        auto f_ = (int (*)(...))rccl_sym(#fn);                                                    \
        if (!f_) return fail("oa_comm: librccl.so / " #fn " not found");                          \
        int e_ = f_(__VA_ARGS__);                                                                 \
        if (e_ != 0) return fail(std::string(#fn ": RCCL error ") + std::to_string(e_));         \
    } while (0)

int oa_comm_unique_id(void* id128) {
    OA_REQUIRE(id128, "oa_comm_unique_id: NULL");
    OA_RCCL(ncclGetUniqueId, id128);
    return 0;
}
int oa_comm_init(int nranks, int rank, const void* id128, void** comm_out) {
    OA_REQUIRE(id128 && comm_out && nranks >= 1 && rank >= 0 && rank < nranks, "oa_comm_init: bad argument");
    oa_rccl_id id;
    memcpy(&id, id128, sizeof(id));
    void* c = nullptr;
    auto f = (int (*)(void**, int, oa_rccl_id, int))rccl_sym("ncclCommInitRank");
    if (!f) return fail("oa_comm_init: librccl.so / ncclCommInitRank not found");
    int e = f(&c, nranks, id, rank);
    if (e != 0) return fail("ncclCommInitRank: RCCL error " + std::to_string(e));
    *comm_out = c;
    return 0;
}
int oa_comm_destroy(void* comm) {
    if (!comm) return 0;
    OA_RCCL(ncclCommDestroy, comm);
    return 0;
}
/* in-place SUM over the ranks of `comm`; dtype_code: 0 = float64, 1 = int64, 2 = float32 */
int oa_allreduce(void* comm, void* buf, long count, int dtype_code, void* stream) {
    OA_REQUIRE(comm && buf && count >= 0, "oa_allreduce: bad argument");
    const int nccl_type = dtype_code == 0 ? 8 /* ncclFloat64 */ : (dtype_code == 1 ? 4 /* ncclInt64 */ : 7 /* ncclFloat32 */);
    auto f = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))rccl_sym("ncclAllReduce");
    if (!f) return fail("oa_allreduce: librccl.so / ncclAllReduce not found");
    int e = f(buf, buf, (size_t)count, nccl_type, 0 /* ncclSum */, comm, (hipStream_t)stream);
    if (e != 0) return fail("ncclAllReduce: RCCL error " + std::to_string(e));
    return 0;
}

}  // extern "C"
