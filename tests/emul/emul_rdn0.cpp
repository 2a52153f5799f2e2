// CPU thread emulator, the tail of oa_mc_run_rdn0 (TEST INFRASTRUCTURE): the partial-sum and fold bodies of orphics_amd/csrc/rdn0.hpp with
// the grids, workgroup sizes and LDS of their HIP launcher (rdn0_tail, orphics_amd/csrc/elementwise.hip).  Built on the emulator of
// emul_fft.cpp.
#include "emul_fft.cpp"
#include "../../orphics_amd/csrc/rdn0.hpp"

// k: 2 B planes of (ny, pitch) complex, kstride apart; ids: (ny, pitch) int32; part: B * rdn0_groups * 2 * nids doubles (written whole);
// n, S, C: 1, 2 (nids - 2), (2 (nids - 2))^2
template <typename T>
static int do_rdn0_tail(const cx<T>* k, long kstride, int B, int ny, long pitch, int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb,
                        const int64_t* mcounts, double* part, int64_t* n, double* S, double* C) {
    if (B < 1 || nids < 3 || w < 1 || w > pitch || kstride < (long)ny * pitch) return 1;
    if (rdn0_part_lds(nids) > 48 * 1024 || rdn0_fold_lds(nids, B) > 48 * 1024) return 2;
    if (!(rb > 0 && 2L * rb - 1 < ny)) rb = 0;
    const int nrows = rb ? 2 * rb - 1 : ny;
    const int R = rdn0_rows_per_group(nrows), G = rdn0_groups(nrows);
    Rdn0PartArgs<T> a{k, kstride, pitch, ny, ids, pitch, nids, w, rb, nxh, pnorm, part, nrows, R};
    EmuLauncher q;
    q.run(G, 1, RDN0_NT, rdn0_part_lds(nids), [&](EmuCtx& c) { rdn0_part_body<T>(c, a); }, B);
    Rdn0FoldArgs f{part, mcounts, B, G, nids, n, S, C};
    q.run(1, 1, RDN0_FOLD_NT, rdn0_fold_lds(nids, B), [&](EmuCtx& c) { rdn0_fold_body(c, f); });
    return 0;
}

extern "C" {
int emu_rdn0_groups(int nrows) { return rdn0_groups(nrows); }
int emu_rdn0_rows_per_group(int nrows) { return rdn0_rows_per_group(nrows); }
int emu_rdn0_tail_f64(const void* k, long kstride, int B, int ny, long pitch, int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb,
                      const int64_t* mcounts, double* part, int64_t* n, double* S, double* C) {
    return do_rdn0_tail<double>((const cx<double>*)k, kstride, B, ny, pitch, nxh, ids, nids, pnorm, w, rb, mcounts, part, n, S, C);
}
int emu_rdn0_tail_f32(const void* k, long kstride, int B, int ny, long pitch, int nxh, const int32_t* ids, int nids, double pnorm, int w, int rb,
                      const int64_t* mcounts, double* part, int64_t* n, double* S, double* C) {
    return do_rdn0_tail<float>((const cx<float>*)k, kstride, B, ny, pitch, nxh, ids, nids, pnorm, w, rb, mcounts, part, n, S, C);
}
}
