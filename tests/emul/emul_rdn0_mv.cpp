// CPU thread emulator, the tail of oa_mc_run_rdn0_mv (TEST INFRASTRUCTURE): the partial-sum, fold and moment bodies of
// orphics_amd/csrc/rdn0_mv.hpp with the grids, workgroup sizes and LDS of their HIP launcher (rdn0mv_tail, orphics_amd/csrc/elementwise.hip).
// Built on the emulator of emul_fft.cpp.
#include "emul_fft.cpp"
#include "../../orphics_amd/csrc/rdn0_mv.hpp"

// k: 2 nest planes of (ny, pitch) complex, kstride apart; wt: nest real planes wstride apart, or nullptr; ids: (ny, pitch) int32;
// part: rdn0mv_groups * 2 * nspec * nids doubles (written whole); x: 2 nspec (nids - 2); n, S, C: 1, D, D^2 with D = 2 nspec (nids - 2)
template <typename T>
static int do_rdn0mv_tail(const cx<T>* k, long kstride, const T* wt, long wstride, int nest, int nspec, const int* ha, const int* hb, int ny,
                          long pitch, int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb, const int64_t* mcounts, double* part,
                          double* x, int64_t* n, double* S, double* C, int mom_blocks) {
    if (nest < 1 || nest > STACK_MULTI_MAX || w < 1 || w > pitch || nxh < 0 || nxh >= pitch || kstride < (long)ny * pitch) return 1;
    if (nspec < 1 || nspec > RDN0MV_SPEC_MAX || nids < 3 || nids > RDN0MV_IDS_MAX || (long)nspec * nids > RDN0MV_TABLE_MAX) return 2;
    for (int s = 0; s < nspec; ++s)
        if (ha[s] < 0 || hb[s] < 0 || ha[s] > nest || hb[s] > nest || (!wt && (ha[s] == nest || hb[s] == nest))) return 3;
    if (!(rb > 0 && 2L * rb - 1 < ny)) rb = 0;
    const int nrows = rb ? 2 * rb - 1 : ny;
    const int R = rdn0mv_rows_per_group(nrows), G = rdn0mv_groups(nrows);
    Rdn0MvSpec spec{};
    spec.nspec = nspec;
    for (int s = 0; s < nspec; ++s) { spec.a[s] = (unsigned char)ha[s]; spec.b[s] = (unsigned char)hb[s]; }
    Rdn0MvPartArgs<T> a{k, kstride, wt, wstride, pitch, ny, ids, pitch, nest, nids, w, rb, nxh, pnorm, spec, part, nrows, R};
    EmuLauncher q;
    q.run(G, 1, RDN0MV_NT, rdn0mv_part_lds(), [&](EmuCtx& c) { rdn0mv_part_body<T>(c, a); });
    Rdn0MvFoldArgs f{part, mcounts, G, nspec, nids, x};
    q.run((nspec * nids + RDN0MV_FOLD_NT - 1) / RDN0MV_FOLD_NT, 1, RDN0MV_FOLD_NT, 0, [&](EmuCtx& c) { rdn0mv_fold_body(c, f); });
    Rdn0MvMomArgs m{x, 2 * nspec * (nids - 2), n, S, C};
    q.run(mom_blocks, 1, RDN0MV_FOLD_NT, 0, [&](EmuCtx& c) { rdn0mv_moments_body(c, m); });
    return 0;
}

extern "C" {
int emu_rdn0mv_groups(int nrows) { return rdn0mv_groups(nrows); }
int emu_rdn0mv_rows_per_group(int nrows) { return rdn0mv_rows_per_group(nrows); }
int emu_rdn0mv_tail_f64(const void* k, long kstride, const void* wt, long wstride, int nest, int nspec, const int* ha, const int* hb, int ny, long pitch,
                        int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb, const int64_t* mcounts, double* part, double* x, int64_t* n,
                        double* S, double* C, int mom_blocks) {
    return do_rdn0mv_tail<double>((const cx<double>*)k, kstride, (const double*)wt, wstride, nest, nspec, ha, hb, ny, pitch, nxh, ids, nids, pnorm, w, rb,
                                  mcounts, part, x, n, S, C, mom_blocks);
}
int emu_rdn0mv_tail_f32(const void* k, long kstride, const void* wt, long wstride, int nest, int nspec, const int* ha, const int* hb, int ny, long pitch,
                        int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb, const int64_t* mcounts, double* part, double* x, int64_t* n,
                        double* S, double* C, int mom_blocks) {
    return do_rdn0mv_tail<float>((const cx<float>*)k, kstride, (const float*)wt, wstride, nest, nspec, ha, hb, ny, pitch, nxh, ids, nids, pnorm, w, rb,
                                 mcounts, part, x, n, S, C, mom_blocks);
}
}
