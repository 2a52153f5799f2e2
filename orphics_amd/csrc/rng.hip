// K8: on-device Gaussian random fields (Philox4x32-10 counter RNG + Box-Muller)
// K9: device-side moment accumulation for Monte-Carlo ensembles.
#include <algorithm>
#include "common.hpp"
#include "philox.hpp"

namespace oa {

// Hermitian-consistent unit white noise on the hc grid, times covsqrt.
// One Philox call serves 2 modes: (row y', column pair p) -> columns 2p, 2p+1.
template <typename T>
__global__ __launch_bounds__(256) void grf_hc_kernel(uint64_t seed, uint64_t sid, const T* __restrict__ cs,
                                                     cx<T>* __restrict__ out, int ny, int nx, long kp, int wpairs, int rband,
                                                     long zstride) {
    // grid z = realisation: stream id sid + z into the plane z * zstride elements behind `out` (oa_mc_run's batches)
    sid += blockIdx.z;
    out += (long)blockIdx.z * zstride;
    const int nxh = nx / 2;
    const int npair = nxh / 2 + 1;  // pairs cover columns 0..nxh(+1)
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    // region draws (oa_grf_hc_band): grid y enumerates the band rows y < rband, y > ny - rband; every mode keeps the
    // Philox counter of the full-plane draw, so the region is a bit-identical subset of it
    int y = blockIdx.y;
    if (rband > 0 && y >= rband) y += ny - (2 * rband - 1);
    if (pr >= (wpairs > 0 ? wpairs : npair)) return;
    const T rs2 = (T)0.70710678118654752440;
    float n[4];
    int cur_ys = -1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int x = 2 * pr + j;
        if (x > nxh) break;
        // self-conjugate columns: rows y and ny-y must be conjugates
        const bool edgecol = (x == 0 || x == nxh);
        int ys = y;
        bool cj = false;
        if (edgecol && y > ny / 2) { ys = ny - y; cj = true; }
        // columns 2p, 2p + 1 share a counter (and its four normals) unless one of them is a self-conjugate column read at the
        // mirrored row: ONE Philox evaluation per thread, not one per column
        if (ys != cur_ys) { normals4(seed, sid, (uint64_t)ys * (uint64_t)npair + (uint64_t)pr, n); cur_ys = ys; }
        T re = (T)n[2 * j], im = (T)n[2 * j + 1];
        if (edgecol && (ys == 0 || ys == ny / 2)) { im = (T)0; }  // real mode, variance 1
        else { re *= rs2; im *= rs2; }
        if (cj) im = -im;
        const long i = (long)y * kp + x;
        const T s = cs ? cs[i] : (T)1;
        out[i] = mk<T>(re * s, im * s);
    }
}

// BAND GRID draw of oa_mc_run on map sides 2^a 3^b 5^c (pipeline.hip): the leg band (columns < 2 wpairs, rows y < rband or
// y > ny - rband) of grf_hc_kernel's N-grid draw -- same Philox counters, same self-conjugate edge rules, amplitude from the N-grid
// covsqrt -- written into the hc layout of the inner (my, okp) grid, row ky mod my instead of ky mod ny
template <typename T>
__global__ __launch_bounds__(256) void grf_band_inner_kernel(uint64_t seed, uint64_t sid, const T* __restrict__ cs, cx<T>* __restrict__ out,
                                                             int ny, int nx, long kp, int wpairs, int rband, int my, long okp, long zstride) {
    sid += blockIdx.z;
    out += (long)blockIdx.z * zstride;
    const int nxh = nx / 2;
    const int npair = nxh / 2 + 1;
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y, yo = y;
    if (y >= rband) { y += ny - (2 * rband - 1); yo += my - (2 * rband - 1); }
    if (pr >= wpairs) return;
    const T rs2 = (T)0.70710678118654752440;
    float n[4];
    int cur_ys = -1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int x = 2 * pr + j;
        if (x > nxh) break;
        const bool edgecol = (x == 0 || x == nxh);
        int ys = y;
        bool cj = false;
        if (edgecol && y > ny / 2) { ys = ny - y; cj = true; }
        if (ys != cur_ys) { normals4(seed, sid, (uint64_t)ys * (uint64_t)npair + (uint64_t)pr, n); cur_ys = ys; }
        T re = (T)n[2 * j], im = (T)n[2 * j + 1];
        if (edgecol && (ys == 0 || ys == ny / 2)) { im = (T)0; }
        else { re *= rs2; im *= rs2; }
        if (cj) im = -im;
        const T s = cs ? cs[(long)y * kp + x] : (T)1;
        out[(long)yo * okp + x] = mk<T>(re * s, im * s);
    }
}
int grf_band_inner(oa_plan* p, uint64_t seed, uint64_t stream_id, int nreal, const void* covsqrt_hc, void* out, int my, long okp, long zstride,
                   int width, int rband, hipStream_t stream) {
    OA_REQUIRE(p && out && nreal >= 1 && width >= 1 && rband >= 1 && 2 * rband - 1 <= std::min(p->ny, my) && 2 * ((width + 1) / 2) <= okp,
               "band draw: bad argument");
    const int wpairs = (width + 1) / 2;
    const int bs = wpairs >= 256 ? 256 : 64;
    dim3 grid((wpairs + bs - 1) / bs, 2 * rband - 1, nreal);
    if (p->dtype == OA_F32)
        hipLaunchKernelGGL(grf_band_inner_kernel<float>, grid, dim3(bs), 0, stream, seed, stream_id, (const float*)covsqrt_hc, (cx<float>*)out,
                           p->ny, p->nx, p->kp, wpairs, rband, my, okp, zstride);
    else
        hipLaunchKernelGGL(grf_band_inner_kernel<double>, grid, dim3(bs), 0, stream, seed, stream_id, (const double*)covsqrt_hc, (cx<double>*)out,
                           p->ny, p->nx, p->kp, wpairs, rband, my, okp, zstride);
    OA_LAUNCH_CHECK();
    return 0;
}

// MapGen.get_map in one pass (maps.py:1579-1587): up to three white fields of streams (seed, sid0 + j) -- the counters and the
// Hermitian rules of grf_hc_kernel, so every w_j is bit-identical to a separate oa_grf_hc draw -- mixed by the covariance square
// root, v_i = sum_j cs[i][j] w_j (terms formed and added in the order of the per-plane path: cmul_real, then +), optionally
// rotated (E, B <-> Q, U on components 1, 2) and optionally ADDED to filtered input planes:
//   in == nullptr : out_i = rot(v)_i * scale                          (the unlensed T, Q, U transforms; kappa)
//   in != nullptr : out_i = rot(in * filt)_i + scale * v_i            (beam x lensed transforms -> E, B, + noise)
template <typename T>
struct GrfMixArgs {
    uint64_t seed, sid0;
    const T* cs[9];
    const T* rc;
    const T* rs;
    const cx<T>* in[3];
    const T* filt;
    cx<T>* out[3];
    cx<T>* out2[3];                // INNER launches with two triples (oa_grf_mix_band_inner_triples): the planes of triple 1 (grid z = 1)
    T scale;
    int ncomp, ny, nx;
    long kp;
    int wpairs, width, rband;      // BAND launches (oa_grf_mix_band): column pairs / columns drawn, row band (0 = every row)
    int my;                        // INNER launches (oa_grf_mix_band_inner): rows and row pitch of the output planes
    long okp;
    int rneg;                      // != 0: the rotation runs with -rs (E, B -> Q, U by the planes that take Q, U -> E, B: oa_mc_run_mv_windowed)
};
// NC and the input mode are compile-time: every loop unrolls, the pointer tables and the per-component values stay in registers
// (with run-time indices they went through scratch: 400-660 us per call at 4096^2 float64 instead of 100-250).  A thread owns the
// column pair (2p, 2p + 1) of one row and, where kp = nx/2 + 16 is even (VEC), moves it with ONE load / store per plane (32 B
// float64, 16 B float32: pairs are aligned and in bounds, row padding included).  nx/2 odd makes kp odd: the pairs of every other
// row are then misaligned and the last pair of a row has no second column (it would be column 0 of the next row, or one element
// behind the plane), so those plans move the two columns one by one and skip the missing one.  All loads are issued before the
// Philox / Box-Muller arithmetic.
template <typename T> struct alignas(2 * sizeof(T)) Pair { T a, b; };
template <bool VEC, typename E>
OA_D Pair<E> load_pair(const E* p, long i0, bool second) {
    if constexpr (VEC) {
        return *reinterpret_cast<const Pair<E>*>(p + i0);
    } else {
        Pair<E> r;
        r.a = p[i0];
        r.b = second ? p[i0 + 1] : p[i0];
        return r;
    }
}
template <bool VEC, typename E>
OA_D void store_pair(E* p, long i0, bool second, const Pair<E>& v) {
    if constexpr (VEC) {
        *reinterpret_cast<Pair<E>*>(p + i0) = v;
    } else {
        p[i0] = v.a;
        if (second) p[i0 + 1] = v.b;
    }
}
// BAND (oa_grf_mix_band; HAS_IN and VEC off): the same thread body on the leg band only -- grid y enumerates the band rows as
// grf_hc_kernel does, the columns stop at a.width (<= nx/2 + 1), and nothing else of the output planes is written.  Every mode keeps
// its Philox counter and goes through the same expressions as the full draw: a bit-identical subset of it.
// INNER (oa_grf_mix_band_inner; with BAND, a.rband >= 1): counters, edge rules and the cs loads are those of N-grid row y as before, the
// stores go to row yo = ky mod a.my of (a.my, a.okp) planes -- the band in the hc layout of an inner grid (grf_band_inner_kernel's
// mapping).  Only the store offset differs: the values are those of the BAND launch.  Grid z = the TRIPLE of an INNER launch
// (oa_grf_mix_band_inner_triples): workgroups of z = 1 draw streams sid0 + 3 .. into a.out2 -- the body, and with it every value, is that
// of a launch of its own with those streams and planes; a thread still evaluates each Philox counter once for its triple.
template <typename T, int NC, bool HAS_IN, bool VEC, bool BAND = false, bool INNER = false>
__global__ __launch_bounds__(256) void grf_mix_kernel(GrfMixArgs<T> a) {
    static_assert(!INNER || (BAND && !VEC && !HAS_IN), "the inner layout is a BAND launch");
    const int nxh = a.nx / 2, npair = nxh / 2 + 1, ny = a.ny;
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    [[maybe_unused]] int yo = y;
    uint64_t sid0 = a.sid0;
    if constexpr (INNER) {
        if (blockIdx.z) sid0 += 3;
    }
    if constexpr (BAND) {
        if (a.rband > 0 && y >= a.rband) {
            y += ny - (2 * a.rband - 1);
            if constexpr (INNER) yo += a.my - (2 * a.rband - 1);
        }
        if (pr >= a.wpairs) return;
    } else {
        if (2L * pr >= a.kp) return;
    }
    const long i0 = (long)y * a.kp + 2 * pr;
    const bool second = BAND ? 2 * pr + 1 < a.width : 2L * pr + 1 < a.kp;       // always true with VEC
    typedef Pair<T> R2;
    typedef Pair<cx<T>> C2;
    // ---- loads ----
    R2 sv[NC * NC];
#pragma unroll
    for (int k = 0; k < NC * NC; ++k) { sv[k].a = (T)0; sv[k].b = (T)0; if (a.cs[k]) sv[k] = load_pair<VEC>(a.cs[k], i0, second); }
    R2 rc{(T)1, (T)1}, rs{(T)0, (T)0}, fl{(T)1, (T)1};
    if (NC == 3 && a.rc) {
        rc = load_pair<VEC>(a.rc, i0, second); rs = load_pair<VEC>(a.rs, i0, second);
        if (a.rneg) { rs.a = -rs.a; rs.b = -rs.b; }
    }
    C2 u[NC];
    if constexpr (HAS_IN) {
        if (a.filt) fl = load_pair<VEC>(a.filt, i0, second);
#pragma unroll
        for (int c = 0; c < NC; ++c) u[c] = load_pair<VEC>(a.in[c], i0, second);
    }
    // ---- draws: columns 2p, 2p + 1 share a counter unless one of them is a self-conjugate column read at the mirrored row ----
    const T rs2 = (T)0.70710678118654752440;
    cx<T> w[2][NC];
    float n[NC][4] = {};                        // a pair that lies in the row padding draws nothing and stores zeros
    int cur_ys = -1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int x = 2 * pr + j;
        const bool edgecol = (x == 0 || x == nxh);
        int ys = y;
        bool cj = false;
        if (edgecol && y > ny / 2) { ys = ny - y; cj = true; }
        if (ys != cur_ys && x <= nxh) {
#pragma unroll
            for (int c = 0; c < NC; ++c) normals4(a.seed, sid0 + c, (uint64_t)ys * (uint64_t)npair + (uint64_t)pr, n[c]);
            cur_ys = ys;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            T re = (T)n[c][2 * j], im = (T)n[c][2 * j + 1];
            if (edgecol && (ys == 0 || ys == ny / 2)) { im = (T)0; }
            else { re *= rs2; im *= rs2; }
            if (cj) im = -im;
            w[j][c] = mk<T>(re, im);
        }
    }
    // ---- mix, rotate, add: per column of the pair ----
    C2 o[NC];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int x = 2 * pr + j;
        cx<T> v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            bool any = false;
            v[c] = mk<T>((T)0, (T)0);
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if (!a.cs[c * NC + k]) continue;
                const T q = j ? sv[c * NC + k].b : sv[c * NC + k].a;
                const cx<T> term = mk<T>(w[j][k].x * q, w[j][k].y * q);
                v[c] = any ? v[c] + term : term;
                any = true;
            }
        }
        const T cc = j ? rc.b : rc.a, ss = j ? rs.b : rs.a;
        cx<T> r[NC];
        if constexpr (HAS_IN) {
            const T f = j ? fl.b : fl.a;
#pragma unroll
            for (int c = 0; c < NC; ++c) { const cx<T> t = j ? u[c].b : u[c].a; r[c] = a.filt ? mk<T>(t.x * f, t.y * f) : t; }
            if constexpr (NC == 3) {
                if (a.rc) { const cx<T> p = r[1], q = r[2]; r[1] = p * cc - q * ss; r[2] = p * ss + q * cc; }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) r[c] = r[c] + v[c] * a.scale;
        } else {
            if constexpr (NC == 3) {
                if (a.rc) { const cx<T> p = v[1], q = v[2]; v[1] = p * cc - q * ss; v[2] = p * ss + q * cc; }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) r[c] = a.scale == (T)1 ? v[c] : v[c] * a.scale;
        }
        // the row padding of the outputs (columns nx/2 + 1 .. kp - 1) is written as zero: callers pass torch.empty planes
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const cx<T> z = x > nxh ? mk<T>((T)0, (T)0) : r[c];
            if (j) o[c].b = z; else o[c].a = z;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if constexpr (INNER) store_pair<VEC>(blockIdx.z ? a.out2[c] : a.out[c], (long)yo * a.okp + 2 * pr, second, o[c]);
        else store_pair<VEC>(a.out[c], i0, second, o[c]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void randn_kernel(uint64_t seed, uint64_t sid, T* __restrict__ out, long n) {
    const long n4 = (n + 3) / 4;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float v[4];
        normals4(seed, sid, (uint64_t)i, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * i + j < n) out[4 * i + j] = (T)v[j];
    }
}

__global__ __launch_bounds__(256) void moments_add_kernel(const double* __restrict__ x, int d, int64_t* __restrict__ n,
                                                          double* __restrict__ S, double* __restrict__ C) {
    const long tot = (long)d * d;
    const long stride = (long)gridDim.x * blockDim.x;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = gid; i < tot; i += stride) {
        const int a = (int)(i / d), b = (int)(i % d);
        C[i] += x[a] * x[b];
    }
    for (long i = gid; i < d; i += stride) S[i] += x[i];
    if (gid == 0) n[0] += 1;
}

// x_a = sums[a] / counts[a] formed on the fly: bin means (bin2D.bin) straight into the ensemble moments
__global__ __launch_bounds__(256) void moments_add_binned_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts,
                                                                 int d, int64_t* __restrict__ n, double* __restrict__ S,
                                                                 double* __restrict__ C) {
    const long tot = (long)d * d;
    const long stride = (long)gridDim.x * blockDim.x;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = gid; i < tot; i += stride) {
        const int a = (int)(i / d), b = (int)(i % d);
        C[i] += (sums[a] / (double)counts[a]) * (sums[b] / (double)counts[b]);
    }
    for (long i = gid; i < d; i += stride) S[i] += sums[i] / (double)counts[i];
    if (gid == 0) n[0] += 1;
}

template <typename T>
static int grf_mix_launch(oa_plan* p, uint64_t seed, uint64_t sid0, int ncomp, const void* const* cs, const void* rc, const void* rs,
                          const void* const* in, const void* filt, double scale, void* const* out, hipStream_t st, int rneg = 0) {
    GrfMixArgs<T> a;
    a.seed = seed; a.sid0 = sid0; a.rneg = rneg;
    for (int i = 0; i < 9; ++i) a.cs[i] = i < ncomp * ncomp ? (const T*)cs[i] : nullptr;
    a.rc = (const T*)rc; a.rs = (const T*)rs;
    for (int i = 0; i < 3; ++i) { a.in[i] = (in && i < ncomp) ? (const cx<T>*)in[i] : nullptr; a.out[i] = i < ncomp ? (cx<T>*)out[i] : nullptr; a.out2[i] = nullptr; }
    a.filt = (const T*)filt;
    a.scale = (T)scale;
    a.ncomp = ncomp; a.ny = p->ny; a.nx = p->nx; a.kp = p->kp;
    a.wpairs = 0; a.width = 0; a.rband = 0; a.my = 0; a.okp = 0;
    const int npair = (int)((p->kp + 1) / 2), bs = npair >= 256 ? 256 : 64;          // pairs of columns, the row padding included
    const dim3 grid((npair + bs - 1) / bs, p->ny);
    // the pair moves (grf_mix_kernel, VEC) need an even pitch and planes that start on a pair boundary; anything else goes column by column
    auto on_pair = [](const void* q, size_t unit) { return q == nullptr || (uintptr_t)q % unit == 0; };
    bool vec = p->kp % 2 == 0 && on_pair(rc, 2 * sizeof(T)) && on_pair(rs, 2 * sizeof(T)) && on_pair(filt, 2 * sizeof(T));
    for (int i = 0; i < ncomp * ncomp; ++i) vec = vec && on_pair(cs[i], 2 * sizeof(T));
    for (int i = 0; i < ncomp; ++i) vec = vec && on_pair(out[i], 4 * sizeof(T)) && (!in || on_pair(in[i], 4 * sizeof(T)));
#define OA_MIX(NC) \
    do { \
        if (in && vec) hipLaunchKernelGGL((grf_mix_kernel<T, NC, true, true>), grid, dim3(bs), 0, st, a); \
        else if (in) hipLaunchKernelGGL((grf_mix_kernel<T, NC, true, false>), grid, dim3(bs), 0, st, a); \
        else if (vec) hipLaunchKernelGGL((grf_mix_kernel<T, NC, false, true>), grid, dim3(bs), 0, st, a); \
        else hipLaunchKernelGGL((grf_mix_kernel<T, NC, false, false>), grid, dim3(bs), 0, st, a); \
    } while (0)
    if (ncomp == 1) OA_MIX(1);
    else if (ncomp == 2) OA_MIX(2);
    else OA_MIX(3);
#undef OA_MIX
    OA_LAUNCH_CHECK();
    return 0;
}

// the leg band of grf_mix_launch's draw (no inputs, no rotation): columns < width, rows y < rband or y > ny - rband
template <typename T>
static int grf_mix_band_launch(oa_plan* p, uint64_t seed, uint64_t sid0, int ncomp, const void* const* cs, double scale, void* const* out,
                               int width, int rband, hipStream_t st) {
    GrfMixArgs<T> a;
    a.seed = seed; a.sid0 = sid0;
    for (int i = 0; i < 9; ++i) a.cs[i] = i < ncomp * ncomp ? (const T*)cs[i] : nullptr;
    a.rc = nullptr; a.rs = nullptr; a.filt = nullptr;
    for (int i = 0; i < 3; ++i) { a.in[i] = nullptr; a.out[i] = i < ncomp ? (cx<T>*)out[i] : nullptr; a.out2[i] = nullptr; }
    a.scale = (T)scale;
    a.ncomp = ncomp; a.ny = p->ny; a.nx = p->nx; a.kp = p->kp;
    const int hw = p->nx / 2 + 1;
    a.width = (width > 0 && width < hw) ? width : hw;
    a.wpairs = (a.width + 1) / 2;
    a.rband = (rband > 0 && 2L * rband - 1 < p->ny) ? rband : 0;
    a.my = 0; a.okp = 0; a.rneg = 0;
    const int bs = a.wpairs >= 256 ? 256 : 64;
    const dim3 grid((a.wpairs + bs - 1) / bs, a.rband ? 2 * a.rband - 1 : p->ny);
    if (ncomp == 1) hipLaunchKernelGGL((grf_mix_kernel<T, 1, false, false, true>), grid, dim3(bs), 0, st, a);
    else if (ncomp == 2) hipLaunchKernelGGL((grf_mix_kernel<T, 2, false, false, true>), grid, dim3(bs), 0, st, a);
    else hipLaunchKernelGGL((grf_mix_kernel<T, 3, false, false, true>), grid, dim3(bs), 0, st, a);
    OA_LAUNCH_CHECK();
    return 0;
}

// the same band into the hc layout of an inner (my, okp) grid (the caller has checked the band against both grids).  ntriples = 2 (ncomp = 3
// only): `out` holds six planes and grid z = 1 draws streams sid0 + 3 .. sid0 + 5 into planes 3 .. 5, in the same launch
template <typename T>
static int grf_mix_band_inner_launch(oa_plan* p, uint64_t seed, uint64_t sid0, int ncomp, const void* const* cs, double scale, void* const* out,
                                     int my, long okp, int width, int rband, hipStream_t st, int ntriples = 1) {
    GrfMixArgs<T> a;
    a.seed = seed; a.sid0 = sid0;
    for (int i = 0; i < 9; ++i) a.cs[i] = i < ncomp * ncomp ? (const T*)cs[i] : nullptr;
    a.rc = nullptr; a.rs = nullptr; a.filt = nullptr;
    for (int i = 0; i < 3; ++i) {
        a.in[i] = nullptr; a.out[i] = i < ncomp ? (cx<T>*)out[i] : nullptr;
        a.out2[i] = ntriples == 2 ? (cx<T>*)out[3 + i] : nullptr;
    }
    a.scale = (T)scale;
    a.ncomp = ncomp; a.ny = p->ny; a.nx = p->nx; a.kp = p->kp;
    a.width = width; a.wpairs = (width + 1) / 2; a.rband = rband;
    a.my = my; a.okp = okp; a.rneg = 0;
    const int bs = a.wpairs >= 256 ? 256 : 64;
    const dim3 grid((a.wpairs + bs - 1) / bs, 2 * rband - 1, ntriples);
    if (ncomp == 1) hipLaunchKernelGGL((grf_mix_kernel<T, 1, false, false, true, true>), grid, dim3(bs), 0, st, a);
    else if (ncomp == 2) hipLaunchKernelGGL((grf_mix_kernel<T, 2, false, false, true, true>), grid, dim3(bs), 0, st, a);
    else hipLaunchKernelGGL((grf_mix_kernel<T, 3, false, false, true, true>), grid, dim3(bs), 0, st, a);
    OA_LAUNCH_CHECK();
    return 0;
}

// oa_mc_run_mv_windowed: oa_grf_mix's full-plane T, E, B draw with E, B -> Q, U in the same pass -- Q = E c + B s, U = -E s + B c, the
// inverse of oa_rot2's combination, by the caller's Q, U -> E, B planes (the sine enters negated: the values of
// oa_grf_mix(rot_c = c, rot_s = -s) bit for bit)
int grf_mix_teb_to_tqu(oa_plan* p, uint64_t seed, uint64_t sid0, const void* const* cs, const void* rot_c, const void* rot_s, void* const* out,
                       hipStream_t st) {
    return p->dtype == OA_F32 ? grf_mix_launch<float>(p, seed, sid0, 3, cs, rot_c, rot_s, nullptr, nullptr, 1.0, out, st, 1)
                              : grf_mix_launch<double>(p, seed, sid0, 3, cs, rot_c, rot_s, nullptr, nullptr, 1.0, out, st, 1);
}

// x[s * d + j] = sums[s * nids + j + 1] / counts[j + 1], d = nids - 2 (the interior bins of nspec binned spectra, oa_bin_power_multi's
// layout, over the data-independent mode counts): n += 1, S += x, C += x x^T with D = nspec * d (oa_mc_run_mv)
__global__ __launch_bounds__(256) void moments_add_binned_multi_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts,
                                                                       int nspec, int nids, int64_t* __restrict__ n, double* __restrict__ S,
                                                                       double* __restrict__ C) {
    const int d = nids - 2;
    const long D = (long)nspec * d, tot = D * D;
    const long stride = (long)gridDim.x * blockDim.x;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    auto x = [&](long i) { const int s = (int)(i / d), j = (int)(i - (long)s * d); return sums[(long)s * nids + j + 1] / (double)counts[j + 1]; };
    for (long i = gid; i < tot; i += stride) {
        const long a = i / D, b = i - a * D;
        C[i] += x(a) * x(b);
    }
    for (long i = gid; i < D; i += stride) S[i] += x(i);
    if (gid == 0) n[0] += 1;
}
int moments_add_binned_multi(const double* sums, const int64_t* counts, int nspec, int nids, int64_t* n, double* S, double* C, hipStream_t st) {
    OA_REQUIRE(sums && counts && n && S && C && nspec >= 1 && nids >= 3, "moments_add_binned_multi: bad argument");
    const long D = (long)nspec * (nids - 2);
    const int g = flat_grid(D * D, 256, 64);
    hipLaunchKernelGGL(moments_add_binned_multi_kernel, dim3(g), dim3(256), 0, st, sums, counts, nspec, nids, n, S, C);
    OA_LAUNCH_CHECK();
    return 0;
}

}  // namespace oa

using namespace oa;

extern "C" {

int oa_grf_mix_band(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ncomp, const void* const* covsqrt_hc, double scale, void* const* hc_out,
                    int width, int rband, void* stream) {
    OA_REQUIRE(p && covsqrt_hc && hc_out && ncomp >= 1 && ncomp <= 3, "oa_grf_mix_band: bad argument (1 <= ncomp <= 3)");
    OA_REQUIRE(width >= 0 && rband >= 0, "oa_grf_mix_band: negative band");
    for (int i = 0; i < ncomp; ++i) OA_REQUIRE(hc_out[i], "oa_grf_mix_band: NULL output plane");
    return p->dtype == OA_F32 ? grf_mix_band_launch<float>(p, seed, stream_id0, ncomp, covsqrt_hc, scale, hc_out, width, rband, (hipStream_t)stream)
                              : grf_mix_band_launch<double>(p, seed, stream_id0, ncomp, covsqrt_hc, scale, hc_out, width, rband, (hipStream_t)stream);
}

int oa_grf_mix_band_inner(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ncomp, const void* const* covsqrt_hc, double scale,
                          void* const* hc_out, int my, long out_pitch, int width, int rband, void* stream) {
    OA_REQUIRE(p && covsqrt_hc && hc_out, "oa_grf_mix_band_inner: NULL argument");
    OA_REQUIRE(ncomp >= 1 && ncomp <= 3, "oa_grf_mix_band_inner: bad argument (1 <= ncomp <= 3)");
    OA_REQUIRE(my >= 1 && out_pitch >= 1 && width >= 1 && rband >= 1, "oa_grf_mix_band_inner: the inner grid and the band must be positive");
    OA_REQUIRE(2L * rband - 1 <= std::min(p->ny, my), "oa_grf_mix_band_inner: row band beyond the rows of the map's or the inner grid (2 rband - 1 <= min(ny, my))");
    OA_REQUIRE(width <= p->nx / 2 + 1, "oa_grf_mix_band_inner: width beyond the hc columns (width <= nx/2 + 1)");
    OA_REQUIRE(2L * ((width + 1) / 2) <= out_pitch, "oa_grf_mix_band_inner: the band's column pairs do not fit the output row pitch");
    for (int i = 0; i < ncomp; ++i) OA_REQUIRE(hc_out[i], "oa_grf_mix_band_inner: NULL output plane");
    return p->dtype == OA_F32 ? grf_mix_band_inner_launch<float>(p, seed, stream_id0, ncomp, covsqrt_hc, scale, hc_out, my, out_pitch, width, rband, (hipStream_t)stream)
                              : grf_mix_band_inner_launch<double>(p, seed, stream_id0, ncomp, covsqrt_hc, scale, hc_out, my, out_pitch, width, rband, (hipStream_t)stream);
}

int oa_grf_mix_band_inner_triples(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ntriples, const void* const* covsqrt_hc, double scale,
                                  void* const* hc_out, int my, long out_pitch, int width, int rband, void* stream) {
    OA_REQUIRE(p && covsqrt_hc && hc_out, "oa_grf_mix_band_inner_triples: NULL argument");
    OA_REQUIRE(ntriples >= 1 && ntriples <= 2, "oa_grf_mix_band_inner_triples: bad argument (1 <= ntriples <= 2)");
    OA_REQUIRE(my >= 1 && out_pitch >= 1 && width >= 1 && rband >= 1, "oa_grf_mix_band_inner_triples: the inner grid and the band must be positive");
    OA_REQUIRE(2L * rband - 1 <= std::min(p->ny, my), "oa_grf_mix_band_inner_triples: row band beyond the rows of the map's or the inner grid (2 rband - 1 <= min(ny, my))");
    OA_REQUIRE(width <= p->nx / 2 + 1, "oa_grf_mix_band_inner_triples: width beyond the hc columns (width <= nx/2 + 1)");
    OA_REQUIRE(2L * ((width + 1) / 2) <= out_pitch, "oa_grf_mix_band_inner_triples: the band's column pairs do not fit the output row pitch");
    for (int i = 0; i < 3 * ntriples; ++i) OA_REQUIRE(hc_out[i], "oa_grf_mix_band_inner_triples: NULL output plane");
    return p->dtype == OA_F32 ? grf_mix_band_inner_launch<float>(p, seed, stream_id0, 3, covsqrt_hc, scale, hc_out, my, out_pitch, width, rband, (hipStream_t)stream, ntriples)
                              : grf_mix_band_inner_launch<double>(p, seed, stream_id0, 3, covsqrt_hc, scale, hc_out, my, out_pitch, width, rband, (hipStream_t)stream, ntriples);
}

int oa_grf_hc_band(oa_plan* p, uint64_t seed, uint64_t stream_id, const void* covsqrt_hc, void* hc_out, int width, int rband,
                   void* stream) {
    return oa::grf_hc_band_batch(p, seed, stream_id, 1, covsqrt_hc, hc_out, 0, width, rband, (hipStream_t)stream);
}
}  // extern "C"

namespace oa {
int grf_hc_band_batch(oa_plan* p, uint64_t seed, uint64_t stream_id, int nreal, const void* covsqrt_hc, void* hc_out, long zstride,
                      int width, int rband, hipStream_t stream) {
    OA_REQUIRE(p && hc_out && nreal >= 1, "oa_grf_hc: NULL argument");
    const int npair = p->nx / 4 + 1;
    int wpairs = (width > 0 && width < p->nx / 2 + 1) ? (width + 1) / 2 : 0;          // column pairs drawn (0 = all)
    if (wpairs >= npair) wpairs = 0;
    const int rb = (rband > 0 && 2L * rband - 1 < p->ny) ? rband : 0;
    const int np = wpairs ? wpairs : npair;
    const int bs = np >= 256 ? 256 : 64;
    dim3 grid((np + bs - 1) / bs, rb ? 2 * rb - 1 : p->ny, nreal);
    if (p->dtype == OA_F32)
        hipLaunchKernelGGL(grf_hc_kernel<float>, grid, dim3(bs), 0, stream, seed, stream_id,
                           (const float*)covsqrt_hc, (cx<float>*)hc_out, p->ny, p->nx, p->kp, wpairs, rb, zstride);
    else
        hipLaunchKernelGGL(grf_hc_kernel<double>, grid, dim3(bs), 0, stream, seed, stream_id,
                           (const double*)covsqrt_hc, (cx<double>*)hc_out, p->ny, p->nx, p->kp, wpairs, rb, zstride);
    OA_LAUNCH_CHECK();
    return 0;
}
}  // namespace oa

extern "C" {

int oa_grf_hc(oa_plan* p, uint64_t seed, uint64_t stream_id, const void* covsqrt_hc, void* hc_out, void* stream) {
    return oa_grf_hc_band(p, seed, stream_id, covsqrt_hc, hc_out, 0, 0, stream);
}

int oa_grf_mix(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ncomp, const void* const* covsqrt_hc, const void* rot_c, const void* rot_s,
               const void* const* hc_in, const void* filt_hcreal, double scale, void* const* hc_out, void* stream) {
    OA_REQUIRE(p && covsqrt_hc && hc_out && ncomp >= 1 && ncomp <= 3, "oa_grf_mix: bad argument (1 <= ncomp <= 3)");
    OA_REQUIRE((rot_c == nullptr) == (rot_s == nullptr), "oa_grf_mix: rotation needs both planes");
    OA_REQUIRE(!rot_c || ncomp == 3, "oa_grf_mix: the rotation acts on components 1, 2 of three");
    for (int i = 0; i < ncomp; ++i) {
        OA_REQUIRE(hc_out[i], "oa_grf_mix: NULL output plane");
        OA_REQUIRE(!hc_in || hc_in[i], "oa_grf_mix: NULL input plane");
    }
    OA_REQUIRE(hc_in || !filt_hcreal, "oa_grf_mix: a filter without input planes");
    return p->dtype == OA_F32 ? grf_mix_launch<float>(p, seed, stream_id0, ncomp, covsqrt_hc, rot_c, rot_s, hc_in, filt_hcreal, scale, hc_out, (hipStream_t)stream)
                              : grf_mix_launch<double>(p, seed, stream_id0, ncomp, covsqrt_hc, rot_c, rot_s, hc_in, filt_hcreal, scale, hc_out, (hipStream_t)stream);
}

int oa_randn(int dtype, uint64_t seed, uint64_t stream_id, void* out, long n, void* stream) {
    OA_REQUIRE(out && n >= 0, "oa_randn: bad argument");
    const int g = flat_grid((n + 3) / 4 > 0 ? (n + 3) / 4 : 1);
    if (dtype == OA_F32)
        hipLaunchKernelGGL(randn_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, seed, stream_id, (float*)out, n);
    else if (dtype == OA_F64)
        hipLaunchKernelGGL(randn_kernel<double>, dim3(g), dim3(256), 0, (hipStream_t)stream, seed, stream_id, (double*)out, n);
    else
        return fail("oa_randn: bad dtype");
    OA_LAUNCH_CHECK();
    return 0;
}

int oa_moments_add(const double* x, int d, int64_t* n, double* S, double* C, void* stream) {
    OA_REQUIRE(x && n && S && C && d >= 1, "oa_moments_add: bad argument");
    const int g = flat_grid((long)d * d, 256, 64);
    hipLaunchKernelGGL(moments_add_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, x, d, n, S, C);
    OA_LAUNCH_CHECK();
    return 0;
}

int oa_moments_add_binned(const double* sums, const int64_t* counts, int d, int64_t* n, double* S, double* C, void* stream) {
    OA_REQUIRE(sums && counts && n && S && C && d >= 1, "oa_moments_add_binned: bad argument");
    const int g = flat_grid((long)d * d, 256, 64);
    hipLaunchKernelGGL(moments_add_binned_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, sums, counts, d, n, S, C);
    OA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
