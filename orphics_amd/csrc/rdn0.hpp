// Tail of oa_mc_run_rdn0 (pipeline.hip): the 2 B kappa_hat planes of a batch of B realisations -- A_i = QE(d, s) + QE(s, d) and
// B_i = QE(s, s') + QE(s', s), planes 2 i and 2 i + 1 -- -> binned |A|^2, |B|^2 -> x_i = [p(A) - p(B) / 2, p(B) / 2] -> n += 1, S += x_i,
// C += x_i x_i^T in realisation order.  TWO launches: per-workgroup partial sums over a fixed group of band rows, then one workgroup
// that folds them; the kernel boundary is the only ordering between workgroups (no ticket, no spin).  Every sum is formed in float64 in
// an order fixed by the geometry (band, bins) alone: the result is the same bit for bit on every run, for every batch size and however
// a range of realisations is cut into calls.  Shared by the HIP launchers (elementwise.hip) and the CPU emulator (tests/emul/emul_rdn0.cpp).
#pragma once
#include "cx.hpp"
#include "mc_pol.hpp"

namespace oa {

constexpr int RDN0_NT = 64;            // threads of a partial-sum workgroup
constexpr int RDN0_SEG = 8;            // consecutive columns per thread and tile step (a tile step covers RDN0_NT * RDN0_SEG columns)
constexpr int RDN0_PARTS = 192;        // most row groups (= partial vectors per realisation) a band is cut into
constexpr int RDN0_FOLD_NT = 256;      // threads of the fold workgroup
constexpr int RDN0_FOLD_Q = 4;         // interleaved sub-sums per (realisation, plane, bin) in the fold
constexpr int RDN0_FOLD_ITEMS = 512;   // (realisation, plane, bin) items folded per pass (LDS: Q doubles each)

// rows per group / groups of a band of nrows rows: a function of the band alone (never of the batch)
OA_HD int rdn0_rows_per_group(int nrows) { return (nrows + RDN0_PARTS - 1) / RDN0_PARTS; }
OA_HD int rdn0_groups(int nrows) { const int r = rdn0_rows_per_group(nrows); return (nrows + r - 1) / r; }
// dynamic LDS of the two bodies
inline size_t rdn0_part_lds(int nids) { return (size_t)RDN0_NT * RDN0_SEG * 20 + (size_t)RDN0_NT * 4 + (size_t)nids * 16 + 64; }
OA_HD int rdn0_fold_pass(int nids, int B) {              // realisations folded per pass
    int nb = RDN0_FOLD_ITEMS / (2 * nids);
    if (nb < 1) nb = 1;
    return nb < B ? nb : B;
}
inline size_t rdn0_fold_lds(int nids, int B) {
    const size_t items = (size_t)rdn0_fold_pass(nids, B) * 2 * nids;
    return items * RDN0_FOLD_Q * 8 + items * 8 + (size_t)B * 2 * (nids - 2) * 8 + 64;
}

/* PARTIAL SUMS.  Grid (row groups, 1, B), RDN0_NT threads.  Workgroup (g, b) walks the band rows [g R, (g + 1) R) of realisation b's two
 * planes in row order and every row in tile steps of RDN0_NT * RDN0_SEG columns.  In a step thread t owns the RDN0_SEG consecutive
 * columns behind column step + t RDN0_SEG: it forms v = (re^2 + im^2) pnorm m in double for both planes (m = the Hermitian
 * multiplicity: 1 at column 0 and at the grid's Nyquist column nxh, 2 between, 0 beyond) and merges them, in column order, into RUNS of
 * equal bin id; modes with an id outside [0, nids) or m = 0 are skipped and do not end a run.  The runs go to LDS; then the owner of bin
 * k (thread k mod RDN0_NT) adds every run of id k to its two accumulators, thread by thread and run by run, i.e. in column order.
 * After the last row the accumulators are the group's partial vector: part[((b G + g) 2 + plane) nids + k]. */
template <typename T>
struct Rdn0PartArgs {
    const cx<T>* k;  long kstride;     // 2 B kappa_hat planes kstride complex elements apart (A_i, B_i at 2 i, 2 i + 1)
    long pitch;      int ny;           // their row pitch (complex elements) and rows
    const int32_t* ids; long ipitch;   // bin ids on the same grid, row pitch ipitch
    int nids, w, rb, nxh;              // band: columns < w, rows y < rb or y > ny - rb (rb = 0: every row)
    double pnorm;
    double* part;                      // [B][G][2][nids]
    int nrows, rows_per_group;         // band rows (2 rb - 1, or ny) and rdn0_rows_per_group of them
};
template <typename T, class Ctx>
OA_HD void rdn0_part_body(Ctx& ctx, const Rdn0PartArgs<T>& a) {
    const int tid = ctx.tid(), nt = ctx.nthreads(), g = ctx.bid_x(), b = ctx.bid_z(), G = ctx.grid_x();
    char* sm = (char*)ctx.smem();
    double* const run_a = (double*)sm;                                  // [nt][SEG]
    double* const run_b = run_a + (size_t)nt * RDN0_SEG;                // [nt][SEG]
    double* const acc = run_b + (size_t)nt * RDN0_SEG;                  // [nids][2]
    int* const run_id = (int*)(acc + 2 * (size_t)a.nids);               // [nt][SEG]
    int* const nruns = run_id + (size_t)nt * RDN0_SEG;                  // [nt]
    for (int k = tid; k < a.nids; k += nt) { acc[2 * k] = 0.0; acc[2 * k + 1] = 0.0; }
    const cx<T>* const kA = a.k + (long)(2 * b) * a.kstride;
    const cx<T>* const kB = kA + a.kstride;
    const int r0 = g * a.rows_per_group;
    const int r1 = r0 + a.rows_per_group < a.nrows ? r0 + a.rows_per_group : a.nrows;
    for (int r = r0; r < r1; ++r) {
        const long y = band_row_of(r, a.rb, a.ny);
        for (int step = 0; step < a.w; step += nt * RDN0_SEG) {
            int nr = 0, cur = -1;
            double sa = 0.0, sb = 0.0;
            const int x0 = step + tid * RDN0_SEG;
            for (int j = 0; j < RDN0_SEG; ++j) {
                const int x = x0 + j;
                if (x >= a.w) break;
                const int id = a.ids[y * a.ipitch + x];
                const int m = (x == 0 || x == a.nxh) ? 1 : (x < a.nxh ? 2 : 0);
                if (id < 0 || id >= a.nids || m == 0) continue;
                const cx<T> va = kA[y * a.pitch + x], vb = kB[y * a.pitch + x];
                const double pa = ((double)va.x * (double)va.x + (double)va.y * (double)va.y) * a.pnorm * (double)m;
                const double pb = ((double)vb.x * (double)vb.x + (double)vb.y * (double)vb.y) * a.pnorm * (double)m;
                if (id != cur) {
                    if (cur >= 0) { run_id[tid * RDN0_SEG + nr] = cur; run_a[tid * RDN0_SEG + nr] = sa; run_b[tid * RDN0_SEG + nr] = sb; ++nr; }
                    cur = id; sa = pa; sb = pb;
                } else { sa += pa; sb += pb; }
            }
            if (cur >= 0) { run_id[tid * RDN0_SEG + nr] = cur; run_a[tid * RDN0_SEG + nr] = sa; run_b[tid * RDN0_SEG + nr] = sb; ++nr; }
            nruns[tid] = nr;
            ctx.sync();
            for (int k = tid; k < a.nids; k += nt) {
                double ta = acc[2 * k], tb = acc[2 * k + 1];
                for (int t = 0; t < nt; ++t) {
                    const int n = nruns[t];
                    for (int j = 0; j < n; ++j)
                        if (run_id[t * RDN0_SEG + j] == k) { ta += run_a[t * RDN0_SEG + j]; tb += run_b[t * RDN0_SEG + j]; }
                }
                acc[2 * k] = ta; acc[2 * k + 1] = tb;
            }
            ctx.sync();
        }
    }
    double* const out = a.part + ((long)b * G + g) * 2 * a.nids;
    for (int k = tid; k < a.nids; k += nt) { out[k] = acc[2 * k]; out[a.nids + k] = acc[2 * k + 1]; }
}

/* FOLD.  ONE workgroup of RDN0_FOLD_NT threads.  Per (realisation, plane, bin) the G partials are added as RDN0_FOLD_Q interleaved
 * sub-sums (sub-sum q: groups q, q + Q, ... in that order), combined as (s0 + s1) + (s2 + s3) -- a fixed tree, the same for every batch;
 * bandpowers p = sum / mcounts[bin] over the interior bins 1 .. nids - 2 (mcounts: the data-independent mode counts of the whole plane);
 * x_i = [p(A) - p(B) / 2, p(B) / 2]; then, element by element with its one owning thread, S[j] += x_i[j] and C[j][l] += x_i[j] x_i[l]
 * for i = 0 .. B - 1 in that order -- Statistics.add of the 2 d-vector --, and n += B. */
struct Rdn0FoldArgs {
    const double* part;                // [B][G][2][nids]
    const int64_t* mcounts;            // [nids]
    int B, G, nids;
    int64_t* n; double* S; double* C;  // 1, 2 d, (2 d)^2 with d = nids - 2
};
template <class Ctx>
OA_HD void rdn0_fold_body(Ctx& ctx, const Rdn0FoldArgs& a) {
    const int tid = ctx.tid(), nt = ctx.nthreads();
    const int d = a.nids - 2, D = 2 * d;
    const int nb = rdn0_fold_pass(a.nids, a.B);
    const int cap = nb * 2 * a.nids;                                    // items of a pass
    double* const sub = (double*)ctx.smem();                            // [Q][cap]
    double* const tot = sub + (size_t)RDN0_FOLD_Q * cap;                // [cap]
    double* const xs = tot + cap;                                       // [B][D]
    for (int b0 = 0; b0 < a.B; b0 += nb) {
        const int bn = b0 + nb < a.B ? nb : a.B - b0;
        const int items = bn * 2 * a.nids;
        for (int w = tid; w < items * RDN0_FOLD_Q; w += nt) {
            const int q = w / items, it = w - q * items;
            const int b = b0 + it / (2 * a.nids), pk = it % (2 * a.nids);           // pk = plane * nids + bin
            const double* src = a.part + (long)b * a.G * 2 * a.nids + pk;
            double s = 0.0;
            for (int g = q; g < a.G; g += RDN0_FOLD_Q) s += src[(long)g * 2 * a.nids];
            sub[(size_t)q * cap + it] = s;
        }
        ctx.sync();
        for (int it = tid; it < items; it += nt)
            tot[it] = (sub[it] + sub[(size_t)cap + it]) + (sub[2 * (size_t)cap + it] + sub[3 * (size_t)cap + it]);
        ctx.sync();
        for (int w = tid; w < bn * d; w += nt) {
            const int bl = w / d, j = w - bl * d;
            const double cnt = (double)a.mcounts[j + 1];
            const double pa = tot[(size_t)bl * 2 * a.nids + j + 1] / cnt;
            const double pb = tot[(size_t)bl * 2 * a.nids + a.nids + j + 1] / cnt;
            const double half = 0.5 * pb;
            xs[(size_t)(b0 + bl) * D + j] = pa - half;
            xs[(size_t)(b0 + bl) * D + d + j] = half;
        }
        ctx.sync();
    }
    for (int j = tid; j < D; j += nt) {
        double s = a.S[j];
        for (int b = 0; b < a.B; ++b) s += xs[(size_t)b * D + j];
        a.S[j] = s;
    }
    for (long e = tid; e < (long)D * D; e += nt) {
        const int j = (int)(e / D), l = (int)(e - (long)j * D);
        double c = a.C[e];
        for (int b = 0; b < a.B; ++b) c += xs[(size_t)b * D + j] * xs[(size_t)b * D + l];
        a.C[e] = c;
    }
    if (tid == 0) a.n[0] += a.B;
}

}  // namespace oa
