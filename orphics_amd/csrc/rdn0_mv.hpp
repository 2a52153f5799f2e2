// Tail of oa_mc_run_rdn0_mv (pipeline.hip): the 2 nest kappa_hat planes of ONE realisation of an estimator set -- A_e = QE_e(d; s) + QE_e(s; d)
// at plane e, B_e = QE_e(s; s') + QE_e(s'; s) at plane nest + e -- and the optional MV weights -> per spectrum (a, b) of the list the binned
// Re(A_a conj A_b) and Re(B_a conj B_b) (field nest = the MV combination sum_e w_e Z_e) -> x_i = [p(A_a, A_b) - p(B_a, B_b) / 2 ..., p(B_a, B_b) / 2 ...]
// -> n += 1, S += x_i, C += x_i x_i^T.  THREE launches: per-workgroup partial sums over a fixed group of band rows, a fold that leaves x_i,
// the moment update; kernel boundaries are the only hand-over between workgroups (no ticket, no float atomics).  Every sum is formed in
// float64 in an order fixed by the band, the bins and the spectrum list alone: the result is the same bit for bit on every run and however
// a range of realisations is cut into calls.  Shared by the HIP launchers (elementwise.hip) and the CPU emulator (tests/emul/emul_rdn0_mv.cpp).
#pragma once
#include "cx.hpp"
#include "mc_pol.hpp"

namespace oa {

constexpr int RDN0MV_NT = 64;          // threads of a partial-sum workgroup = columns of a tile step (a thread owns ONE mode of the step)
constexpr int RDN0MV_PARTS = 512;      // most row groups (= partial tables) a band is cut into
constexpr int RDN0MV_SPEC_MAX = 28;    // spectra of the list (oa_bin_power_multi's limit); with nids <= 1024 and nspec * nids <= 4096 the
constexpr int RDN0MV_TABLE_MAX = 4096; // ... tail holds every (nspec, nids >= 3) that entry accepts
constexpr int RDN0MV_IDS_MAX = 1024;
constexpr int RDN0MV_FOLD_NT = 256;    // threads of a fold / moments workgroup
constexpr int RDN0MV_FOLD_Q = 4;       // interleaved sub-sums per (plane set, spectrum, bin) in the fold

OA_HD int rdn0mv_rows_per_group(int nrows) { return (nrows + RDN0MV_PARTS - 1) / RDN0MV_PARTS; }
OA_HD int rdn0mv_groups(int nrows) { const int r = rdn0mv_rows_per_group(nrows); return (nrows + r - 1) / r; }
// dynamic LDS of the partial-sum body: the 2 (nest + 1) field values of a step's modes, their weights norm * m, their bin ids
inline size_t rdn0mv_part_lds() { return (size_t)RDN0MV_NT * (2 * (STACK_MULTI_MAX + 1) * 16 + 8 + 4) + 64; }

struct Rdn0MvSpec {                    // the spectrum list: fields a[s], b[s] in [0, nest] (nest = MV, with weights only)
    int nspec;
    unsigned char a[RDN0MV_SPEC_MAX], b[RDN0MV_SPEC_MAX];
};

/* PARTIAL SUMS.  Grid (row groups), RDN0MV_NT threads.  Workgroup g owns the table part[g][set][s][bin] (set 0: A, 1: B; 2 nspec nids
 * doubles), zeroes it and walks the band rows [g R, (g + 1) R) in row order and every row in tile steps of RDN0MV_NT columns.  In a step
 * thread t owns the mode at column step + t: it loads the nest A and the nest B values, reads the nest weights once, forms
 * A_MV = sum_e w_e A_e and B_MV in double in registers in estimator order, and leaves the 2 (nest + 1) values, the factor pnorm * m
 * (m = the Hermitian multiplicity: 1 at column 0 and at the grid's Nyquist column nxh, 2 between) and the bin id in LDS; a mode with an
 * id outside [0, nids), beyond the band or beyond column nxh carries id -1.  Then the (set, spectrum, bin) items of the bins lo .. hi that
 * occur in the step are dealt to the threads: the owner of an item adds Re(Z_a conj Z_b) * (pnorm * m) of the step's modes of that bin, in
 * column order, to the item's entry of the table.  An entry has one owner per step and steps are separated by barriers: its sum runs over
 * the group's modes in (row, column) order. */
template <typename T>
struct Rdn0MvPartArgs {
    const cx<T>* k;  long kstride;     // 2 nest kappa_hat planes kstride complex elements apart (A_e at e, B_e at nest + e)
    const T* wt;     long wstride;     // nest MV weight planes (real), wstride elements apart; nullptr: no field nest
    long pitch;      int ny;           // row pitch (elements of their own type) and rows of all of them
    const int32_t* ids; long ipitch;   // bin ids on the same grid, row pitch ipitch
    int nest, nids, w, rb, nxh;        // band: columns < w, rows y < rb or y > ny - rb (rb = 0: every row)
    double pnorm;
    Rdn0MvSpec spec;
    double* part;                      // [G][2][nspec][nids]
    int nrows, rows_per_group;         // band rows (2 rb - 1, or ny) and rdn0mv_rows_per_group of them
};
template <typename T, class Ctx>
OA_HD void rdn0mv_part_body(Ctx& ctx, const Rdn0MvPartArgs<T>& a) {
    const int tid = ctx.tid(), nt = ctx.nthreads(), g = ctx.bid_x();
    const int nf = a.nest + (a.wt ? 1 : 0), nspec = a.spec.nspec, nslots = 2 * nspec;
    char* sm = (char*)ctx.smem();
    cx<double>* const z = (cx<double>*)sm;                              // [2][STACK_MULTI_MAX + 1][nt]
    double* const fac = (double*)(z + (size_t)2 * (STACK_MULTI_MAX + 1) * nt);   // [nt]
    int* const sid = (int*)(fac + nt);                                  // [nt]
    double* const tab = a.part + (long)g * nslots * a.nids;
    for (int i = tid; i < nslots * a.nids; i += nt) tab[i] = 0.0;
    ctx.sync();
    const int r0 = g * a.rows_per_group;
    const int r1 = r0 + a.rows_per_group < a.nrows ? r0 + a.rows_per_group : a.nrows;
    for (int r = r0; r < r1; ++r) {
        const long y = band_row_of(r, a.rb, a.ny);
        for (int step = 0; step < a.w; step += nt) {
            const int x = step + tid;
            int id = -1;
            if (x < a.w && x <= a.nxh) {
                id = a.ids[y * a.ipitch + x];
                if (id < 0 || id >= a.nids) id = -1;
            }
            if (id >= 0) {
                const long at = y * a.pitch + x;
#pragma unroll
                for (int set = 0; set < 2; ++set) {
                    double mr = 0.0, mi = 0.0;
#pragma unroll
                    for (int e = 0; e < STACK_MULTI_MAX; ++e) {
                        if (e < a.nest) {
                            const cx<T> v = a.k[at + (long)(set * a.nest + e) * a.kstride];
                            const double vr = (double)v.x, vi = (double)v.y;
                            z[(size_t)(set * (STACK_MULTI_MAX + 1) + e) * nt + tid] = mk<double>(vr, vi);
                            if (a.wt) {
                                const double ww = (double)a.wt[at + e * a.wstride];
                                mr += ww * vr;
                                mi += ww * vi;
                            }
                        }
                    }
                    if (a.wt) z[(size_t)(set * (STACK_MULTI_MAX + 1) + a.nest) * nt + tid] = mk<double>(mr, mi);
                }
                fac[tid] = a.pnorm * (double)((x == 0 || x == a.nxh) ? 1 : 2);
            }
            sid[tid] = id;
            ctx.sync();
            int lo = a.nids, hi = -1;
            for (int t = 0; t < nt; ++t) {
                const int v = sid[t];
                if (v >= 0) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
            }
            const int nitems = hi >= lo ? (hi - lo + 1) * nslots : 0;
            for (int it = tid; it < nitems; it += nt) {
                const int bin = lo + it / nslots, slot = it % nslots;      // slot = set * nspec + s
                const int set = slot / nspec, s = slot - set * nspec;
                const int fa = a.spec.a[s], fb = a.spec.b[s];
                if (fa >= nf || fb >= nf) continue;
                const cx<double>* const za = z + (size_t)(set * (STACK_MULTI_MAX + 1) + fa) * nt;
                const cx<double>* const zb = z + (size_t)(set * (STACK_MULTI_MAX + 1) + fb) * nt;
                double acc = tab[(long)slot * a.nids + bin];
                for (int t = 0; t < nt; ++t)
                    if (sid[t] == bin) acc += (za[t].x * zb[t].x + za[t].y * zb[t].y) * fac[t];
                tab[(long)slot * a.nids + bin] = acc;
            }
            ctx.sync();
        }
    }
}

/* FOLD.  Grid ceil(nspec nids / RDN0MV_FOLD_NT), one thread per (spectrum s, bin): for A and for B the G partials are added as
 * RDN0MV_FOLD_Q interleaved sub-sums (sub-sum q: groups q, q + Q, ... in that order), combined as (s0 + s1) + (s2 + s3); for the interior
 * bins 1 .. nids - 2, with d = nids - 2 and j = bin - 1: pa = sum_A / mcounts[bin], half = 0.5 (sum_B / mcounts[bin]),
 * x[s d + j] = pa - half ("rdn0"), x[(nspec + s) d + j] = half ("mcn0"). */
struct Rdn0MvFoldArgs {
    const double* part;                // [G][2][nspec][nids]
    const int64_t* mcounts;            // [nids]: the data-independent mode counts of the whole plane
    int G, nspec, nids;
    double* x;                         // [2 nspec (nids - 2)]
};
template <class Ctx>
OA_HD void rdn0mv_fold_body(Ctx& ctx, const Rdn0MvFoldArgs& a) {
    const int item = ctx.bid_x() * ctx.nthreads() + ctx.tid();
    if (item >= a.nspec * a.nids) return;
    const int s = item / a.nids, bin = item - s * a.nids;
    if (bin < 1 || bin > a.nids - 2) return;
    const long tsz = 2L * a.nspec * a.nids;
    double tot[2];
    for (int set = 0; set < 2; ++set) {
        const double* src = a.part + ((long)set * a.nspec + s) * a.nids + bin;
        double sub[RDN0MV_FOLD_Q];
        for (int q = 0; q < RDN0MV_FOLD_Q; ++q) {
            double v = 0.0;
            for (int g = q; g < a.G; g += RDN0MV_FOLD_Q) v += src[(long)g * tsz];
            sub[q] = v;
        }
        tot[set] = (sub[0] + sub[1]) + (sub[2] + sub[3]);
    }
    const int d = a.nids - 2, j = bin - 1;
    const double cnt = (double)a.mcounts[bin];
    const double pa = tot[0] / cnt, half = 0.5 * (tot[1] / cnt);
    a.x[(long)s * d + j] = pa - half;
    a.x[((long)a.nspec + s) * d + j] = half;
}

/* MOMENTS.  Any grid of RDN0MV_FOLD_NT-thread workgroups; element e of C (D^2, D = 2 nspec (nids - 2)) belongs to the thread e mod (threads
 * of the grid): C[e] += x[e / D] x[e mod D]; likewise S[e] += x[e] for e < D; the first thread adds 1 to n.  One addition per element:
 * the result does not depend on the grid. */
struct Rdn0MvMomArgs {
    const double* x;
    int D;
    int64_t* n; double* S; double* C;
};
template <class Ctx>
OA_HD void rdn0mv_moments_body(Ctx& ctx, const Rdn0MvMomArgs& a) {
    const long stride = (long)ctx.grid_x() * ctx.nthreads();
    const long gid = (long)ctx.bid_x() * ctx.nthreads() + ctx.tid();
    const long D = a.D, tot = D * D;
    for (long e = gid; e < tot; e += stride) {
        const long j = e / D, l = e - j * D;
        a.C[e] += a.x[j] * a.x[l];
    }
    for (long e = gid; e < D; e += stride) a.S[e] += a.x[e];
    if (gid == 0) a.n[0] += 1;
}

}  // namespace oa
