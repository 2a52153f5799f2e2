// CPU thread emulator, source stage of oa_mc_run_mv_windowed (TEST INFRASTRUCTURE): the fused windowed row pass row_fft_body<ROW_WIN>
// (orphics_amd/csrc/fft_kernels.hpp) over nz planes in one launch (grid y = plane, RowArgs::nz, the window shared), and the per-mode
// bodies of orphics_amd/csrc/mc_pol.hpp -- the Q,U -> E,B rotation on the leg band and the mean-field stacks of an estimator set -- with
// the grids of their HIP launchers (elementwise.hip).  Built on the emulator of emul_fft.cpp.
#include "emul_fft.cpp"
#include "../../orphics_amd/csrc/mc_pol.hpp"

// EmuLauncher's row launch with the plane index on grid y, as HipLauncher::row_mode launches it
struct EmuLauncherZ : EmuLauncher {
    template <typename T> void row(int grid, int nt, size_t smem, const RowArgs<T>& a) {
        dispatch_seq(a.logL, [&](auto seq) {
            using S = decltype(seq);
            if (a.mode == ROW_WIN) run(grid, a.nz > 0 ? a.nz : 1, nt, smem, [&](EmuCtx& c) { row_fft_body<T, ROW_WIN, S>(c, a); });
        });
    }
};

// in: nz planes of (ny, kp) complex rows (already inverse-transformed along y), in_zoff apart; window: (ny, nx) reals, shared;
// out: nz planes of (ny, opitch) complex, out_zoff apart, wcols columns written
template <typename T>
static int do_rows_win3(int ny, int nx, int nz, const cx<T>* in, long in_zoff, const T* window, cx<T>* out, long opitch, long out_zoff, double scale,
                        int wcols) {
    if (!is_pow2(ny) || !is_pow2(nx) || nx < 32 || nz < 1 || wcols < 1 || wcols > nx / 2 + 1 || opitch < wcols) return 1;
    Holder<T> h(ny, nx);
    EmuLauncherZ q;
    h.p.rows(q, ROW_WIN, in, h.p.kp, out, opitch, (T)scale, wcols, window, nz, in_zoff, out_zoff);
    return 0;
}

template <typename T>
static int do_band_rot2(const T* c, const T* s, cx<T>* qp, cx<T>* up, int ny, long kp, int w, int rb) {
    if (w <= 0 || w > kp) w = (int)kp;
    if (!(rb > 0 && 2L * rb - 1 < ny)) rb = 0;
    BandRotArgs<T> a{c, s, qp, up, kp, ny, w, rb};
    EmuLauncher q;
    q.run((w + 63) / 64, rb ? 2 * rb - 1 : ny, 64, 0, [&](EmuCtx& ctx) { band_rot2_body<T>(ctx, a); });
    return 0;
}

// acc: nest (+ 1 with has_mv) float64 planes of (ny, kp, 2), contiguous
template <typename T>
static int do_stack_multi(const cx<T>* k, long kstride, const T* wt, long wstride, int nest, double* acc, int has_mv, int ny, long kp, int w, int rb) {
    if (nest < 1 || nest > STACK_MULTI_MAX || (has_mv && !wt)) return 1;
    if (w <= 0 || w > kp) w = (int)kp;
    if (!(rb > 0 && 2L * rb - 1 < ny)) rb = 0;
    StackMultiArgs<T> a{};
    a.k = k; a.kstride = kstride; a.wt = has_mv ? wt : nullptr; a.wstride = wstride;
    for (int e = 0; e < nest; ++e) a.acc[e] = (cx<double>*)acc + (long)e * ny * kp;
    a.acc_mv = has_mv ? (cx<double>*)acc + (long)nest * ny * kp : nullptr;
    a.pitch = kp; a.nest = nest; a.ny = ny; a.w = w; a.rb = rb;
    EmuLauncher q;
    q.run((w + 63) / 64, rb ? 2 * rb - 1 : ny, 64, 0, [&](EmuCtx& ctx) { stack_add_region_multi_body<T>(ctx, a); });
    return 0;
}

extern "C" {
int emu_rows_win3_f64(int ny, int nx, int nz, const void* in, long in_zoff, const double* window, void* out, long opitch, long out_zoff, double scale,
                      int wcols) {
    return do_rows_win3<double>(ny, nx, nz, (const cx<double>*)in, in_zoff, window, (cx<double>*)out, opitch, out_zoff, scale, wcols);
}
int emu_rows_win3_f32(int ny, int nx, int nz, const void* in, long in_zoff, const float* window, void* out, long opitch, long out_zoff, double scale,
                      int wcols) {
    return do_rows_win3<float>(ny, nx, nz, (const cx<float>*)in, in_zoff, window, (cx<float>*)out, opitch, out_zoff, scale, wcols);
}
int emu_band_rot2_f64(const double* c, const double* s, void* q, void* u, int ny, long kp, int w, int rb) {
    return do_band_rot2<double>(c, s, (cx<double>*)q, (cx<double>*)u, ny, kp, w, rb);
}
int emu_band_rot2_f32(const float* c, const float* s, void* q, void* u, int ny, long kp, int w, int rb) {
    return do_band_rot2<float>(c, s, (cx<float>*)q, (cx<float>*)u, ny, kp, w, rb);
}
int emu_stack_multi_f64(const void* k, long kstride, const double* wt, long wstride, int nest, double* acc, int has_mv, int ny, long kp, int w, int rb) {
    return do_stack_multi<double>((const cx<double>*)k, kstride, wt, wstride, nest, acc, has_mv, ny, kp, w, rb);
}
int emu_stack_multi_f32(const void* k, long kstride, const float* wt, long wstride, int nest, double* acc, int has_mv, int ny, long kp, int w, int rb) {
    return do_stack_multi<float>((const cx<float>*)k, kstride, wt, wstride, nest, acc, has_mv, ny, kp, w, rb);
}
}
