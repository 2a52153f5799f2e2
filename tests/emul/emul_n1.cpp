// CPU thread emulator, oa_n1_tt (TEST INFRASTRUCTURE): the prologue, pair and fold bodies of orphics_amd/csrc/n1.hpp with the grids,
// workgroup sizes, LDS and launch sequence of their HIP launcher (orphics_amd/csrc/n1.hip).  Built on the emulator of emul_fft.cpp.
#include <algorithm>
#include "emul_fft.cpp"
#include "../../orphics_amd/csrc/n1.hpp"

static int signed_index(int i, int n) { return i > n / 2 ? i - n : i; }

extern "C" {
// planes: (ny, kp) doubles; ly, lx: ny, nx doubles; tiles_per_launch > 0 cuts the pair launches finer than n1_tiles_per_launch does
int emu_n1_tt(const double* wg, const double* wh, const double* cr, const double* cpp, const double* ly, const double* lx, int ny, int nx, long kp,
              int leg_cols, int leg_rows, int nL, const int32_t* Lys, const int32_t* Lxs, int tiles_per_launch, double* S_out) {
    if (nL < 1 || 4L * (leg_rows - 1) >= ny || 4L * (leg_cols - 1) >= nx) return 1;
    const N1Box full = n1_box(0, 0, leg_rows, leg_cols);
    std::vector<N1Q> qtab((size_t)full.bh * full.bw);
    std::vector<double> gtab(qtab.size());
    EmuLauncher q;
    for (int i = 0; i < nL; ++i) {
        if (Lys[i] < 0 || Lys[i] >= ny || Lxs[i] < 0 || Lxs[i] >= nx) return 2;
        const int kLy = signed_index(Lys[i], ny), kLx = signed_index(Lxs[i], nx);
        const N1Box b = n1_box(kLy, kLx, leg_rows, leg_cols);
        std::vector<double> part(1, -7.5);
        long np = 0;
        if (b.bh > 0 && b.bw > 0) {
            const long n = (long)b.bh * b.bw;
            N1ProArgs pa{wg, wh, cr, ly, lx, ny, nx, kp, kLy, kLx, b, qtab.data(), gtab.data()};
            q.run((int)((n + N1_NT - 1) / N1_NT), 1, N1_NT, 0, [&](EmuCtx& c) { n1_prologue_body(c, pa); });
            const long ntiles = n1_ntiles(b);
            const int parts = n1_parts(b);
            part.assign((size_t)ntiles * parts, -7.5);
            const long per = tiles_per_launch > 0 ? tiles_per_launch : n1_tiles_per_launch(b);
            for (long t0 = 0; t0 < ntiles; t0 += per) {
                N1PairArgs a{qtab.data(), gtab.data(), cpp, ny, kp, b, t0, parts, part.data()};
                q.run((int)std::min(per, ntiles - t0), parts, N1_NT, n1_pair_lds(), [&](EmuCtx& c) { n1_pair_body(c, a); });
            }
            np = ntiles * parts;
        }
        N1FoldArgs f{part.data(), np, S_out + i};
        q.run(1, 1, N1_NT, N1_NT * sizeof(double), [&](EmuCtx& c) { n1_fold_body(c, f); });
    }
    return 0;
}
int emu_n1_box(int kLy, int kLx, int leg_rows, int leg_cols, int* out4) {
    const N1Box b = n1_box(kLy, kLx, leg_rows, leg_cols);
    out4[0] = b.y0; out4[1] = b.x0; out4[2] = b.bh; out4[3] = b.bw;
    return (b.bh > 0 && b.bw > 0) ? n1_parts(b) : 0;
}
}
