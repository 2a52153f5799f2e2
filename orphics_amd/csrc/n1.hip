// oa_n1_tt: the analytic N1 bias sums of the TT estimator by direct mode-pair summation (bodies and definition: n1.hpp).
#include <algorithm>
#include "common.hpp"
#include "n1.hpp"

namespace oa {

struct N1Ctx {
    char* sm;
    OA_D int tid() const { return threadIdx.x; }
    OA_D int nthreads() const { return blockDim.x; }
    OA_D int bid_x() const { return blockIdx.x; }
    OA_D int bid_y() const { return blockIdx.y; }
    OA_D int grid_x() const { return gridDim.x; }
    OA_D void sync() const { __syncthreads(); }
    OA_D void* smem() const { return sm; }
};
extern __shared__ __attribute__((aligned(16))) char n1_smem[];
__global__ __launch_bounds__(N1_NT) void n1_prologue_kernel(N1ProArgs a) {
    N1Ctx c{n1_smem};
    n1_prologue_body(c, a);
}
__global__ __launch_bounds__(N1_NT) void n1_pair_kernel(N1PairArgs a) {
    N1Ctx c{n1_smem};
    n1_pair_body(c, a);
}
__global__ __launch_bounds__(N1_NT) void n1_fold_kernel(N1FoldArgs a) {
    N1Ctx c{n1_smem};
    n1_fold_body(c, a);
}

// the attainable float64 vector rate, for tools/n1_bench.py: 8 independent v_fma_f64 chains per thread, no memory traffic in the loop
__global__ __launch_bounds__(N1_NT) void probe_fma64_kernel(long iters, double a, double b, double* out) {
    double x[8];
    for (int k = 0; k < 8; ++k) x[k] = (double)(threadIdx.x + k) * 1e-3;
    for (long i = 0; i < iters; ++i)
        for (int k = 0; k < 8; ++k) x[k] = __builtin_fma(x[k], a, b);
    double s = 0.0;
    for (int k = 0; k < 8; ++k) s += x[k];
    out[(long)blockIdx.x * N1_NT + threadIdx.x] = s;
}

static int signed_index(int i, int n) { return i > n / 2 ? i - n : i; }

}  // namespace oa

using namespace oa;

extern "C" int oa_probe_fma64(int blocks, long iters, double a, double b, double* out, void* stream) {
    OA_REQUIRE(blocks >= 1 && blocks <= 65536 && iters >= 1 && iters <= (1L << 24) && out, "oa_probe_fma64: bad argument");
    hipLaunchKernelGGL(probe_fma64_kernel, dim3(blocks), dim3(N1_NT), 0, (hipStream_t)stream, iters, a, b, out);
    OA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oa_n1_tt(oa_plan* p, const void* wg_hc, const void* wh_hc, const void* cr_hc, const void* cpp_hc, int leg_cols, int leg_rows, int nL,
                        const int32_t* host_Ly, const int32_t* host_Lx, double* S_out, void* stream) {
    OA_REQUIRE(p && wg_hc && wh_hc && cr_hc && cpp_hc && host_Ly && host_Lx && S_out, "oa_n1_tt: NULL argument");
    OA_REQUIRE(p->dtype == OA_F64, "oa_n1_tt: needs a float64 plan (the pair sums are float64 throughout)");
    OA_REQUIRE(p->have_laxes, "oa_n1_tt: call oa_plan_set_laxes first");
    OA_REQUIRE(leg_rows >= 1 && leg_cols >= 1 && 4L * (leg_rows - 1) < p->ny && 4L * (leg_cols - 1) < p->nx,
               "oa_n1_tt: the legs are not band-limited enough: all four modes of a pair must be un-aliased, which needs "
               "4 (leg_rows - 1) < ny and 4 (leg_cols - 1) < nx");
    OA_REQUIRE(nL >= 1, "oa_n1_tt: nL must be >= 1");
    for (int i = 0; i < nL; ++i)
        OA_REQUIRE(host_Ly[i] >= 0 && host_Ly[i] < p->ny && host_Lx[i] >= 0 && host_Lx[i] < p->nx, "oa_n1_tt: an L index is outside the plane");
    hipStream_t st = (hipStream_t)stream;
    // scratch: the mode table and G of the widest box (L = 0), then the partials of the box with the most (tile, part) pairs
    const N1Box full = n1_box(0, 0, leg_rows, leg_cols);
    const size_t nfull = (size_t)full.bh * full.bw;
    size_t npart = 1;
    for (int i = 0; i < nL; ++i) {
        const N1Box b = n1_box(signed_index(host_Ly[i], p->ny), signed_index(host_Lx[i], p->nx), leg_rows, leg_cols);
        if (b.bh > 0 && b.bw > 0) npart = std::max(npart, (size_t)n1_ntiles(b) * n1_parts(b));
    }
    const size_t off_g = nfull * sizeof(N1Q), off_part = off_g + ((nfull * 8 + 255) & ~(size_t)255);
    char* pool = nullptr;
    if (int rc = n1_pool_reserve(p, off_part + npart * 8, &pool)) return rc;
    N1Q* const qtab = (N1Q*)pool;
    double* const gtab = (double*)(pool + off_g);
    double* const part = (double*)(pool + off_part);
    for (int i = 0; i < nL; ++i) {
        const int kLy = signed_index(host_Ly[i], p->ny), kLx = signed_index(host_Lx[i], p->nx);
        const N1Box b = n1_box(kLy, kLx, leg_rows, leg_cols);
        long np = 0;
        if (b.bh > 0 && b.bw > 0) {
            const long n = (long)b.bh * b.bw;
            N1ProArgs pa{(const double*)wg_hc, (const double*)wh_hc, (const double*)cr_hc, p->ly64, p->lx64, p->ny, p->nx, p->kp, kLy, kLx,
                         b, qtab, gtab};
            hipLaunchKernelGGL(n1_prologue_kernel, dim3(flat_grid(n, N1_NT)), dim3(N1_NT), 0, st, pa);
            OA_LAUNCH_CHECK();
            const long ntiles = n1_ntiles(b);
            const int parts = n1_parts(b);
            const long per = n1_tiles_per_launch(b);
            for (long t0 = 0; t0 < ntiles; t0 += per) {
                N1PairArgs a{qtab, gtab, (const double*)cpp_hc, p->ny, p->kp, b, t0, parts, part};
                hipLaunchKernelGGL(n1_pair_kernel, dim3((unsigned)std::min(per, ntiles - t0), parts), dim3(N1_NT), n1_pair_lds(), st, a);
                OA_LAUNCH_CHECK();
            }
            np = ntiles * parts;
        }
        N1FoldArgs f{part, np, S_out + i};
        hipLaunchKernelGGL(n1_fold_kernel, dim3(1), dim3(N1_NT), N1_NT * sizeof(double), st, f);
        OA_LAUNCH_CHECK();
    }
    return 0;
}
