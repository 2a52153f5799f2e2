// CPU thread emulator, the Gaussian draw inside inverse column pass 1 (TEST INFRASTRUCTURE): col_grf_body / GrfColLoad / grf_col_fill of
// orphics_amd/csrc/fft_kernels.hpp with the grid, workgroup size and LDS of their HIP launcher (Fft2dPlan::grf_icols), then the in-place
// pass 2.  The lane-pair exchange of grf_col_fill goes through the column tile here (threads have no lanes).  Host logf / sinf / cosf are
// not the device's: this pins counters, edge rules and index mapping, not bits.  Built on the emulator of emul_fft.cpp.
#include <algorithm>
#include "emul_fft.cpp"

// the same pass 1 with the load functor's per-element statement get(n, c) in the place of the pair fill (one counter evaluation per
// element): what grf_col_fill must reproduce bit for bit on the same host
template <typename T, class SEQ, class Ctx>
static void col_grf_plain_body(Ctx& ctx, const GrfColArgs<T>& a) {
    cx<T>* s = reinterpret_cast<cx<T>*>(ctx.smem());
    const int tid = ctx.tid();
    constexpr int CLC = COL_LOGC, logL = seq_total_log<SEQ>();
    constexpr int CNT = ((1 << (logL + CLC)) / EPT) > 0 ? ((1 << (logL + CLC)) / EPT) : 1;
    const int c0 = ctx.bid_x() << CLC;
    const long g = ctx.bid_y();
    const int ncols = std::min(a.width - c0, 1 << CLC);
    cx<T>* twl = s + (1 << (logL + CLC));
    cx<T>* ti = twl + tw_lds_size(logL);
    tw_lds_fill<T>(ctx, twl, a.tw, a.logTw, logL, CNT);
    if (a.twiddle)
        for (int i = tid; i < (1 << logL); i += CNT) ti[i] = a.tw[(unsigned)g * (unsigned)i];
    ctx.sync();
    const int z = ctx.bid_z();
    const GrfColLoad<T> ld{a.seed, a.sid + (uint64_t)z, a.cs, a.pitch, a.ny, a.nxh, a.nxh / 2 + 1, (int)g, (int)a.in_ns, c0, ncols};
    const ColStore<T> st{a.out + (long)z * a.out_zstride + g * a.out_gs * a.pitch + c0, (unsigned)a.pitch, ncols, true, a.twiddle ? ti : nullptr,
                         (unsigned)g, (T)1, 0, 0, 0, 0};
    fft_pipeline<T, false, true, true, SEQ>(ctx, s, tid, CNT, logL, CLC, 0, twl, logL, ld, st);
}

struct GrfEmuLauncher : EmuLauncher {
    int tiles = 1 << 30;        // column tiles run (the others are left untouched)
    bool plain = false;
    template <typename T> void col_grf(int gx, int gy, int nt, size_t smem, const GrfColArgs<T>& a, int nz) {
        dispatch_seq(a.logL, [&](auto seq) {
            using S = decltype(seq);
            if constexpr (seq_total_log<S>() <= 8) {
                if (plain) run(std::min(gx, tiles), gy, nt, smem, [&](EmuCtx& c) { col_grf_plain_body<T, S>(c, a); }, nz);
                else run(std::min(gx, tiles), gy, nt, smem, [&](EmuCtx& c) { col_grf_body<T, S>(c, a); }, nz);
            }
        });
    }
    template <typename T> void col(int gx, int gy, int nt, size_t smem, const ColArgs<T>& a, int nz = 1) {
        EmuLauncher::col<T>(std::min(gx, tiles), gy, nt, smem, a, nz);
    }
};

template <typename T>
static int do_grf_icols(int ny, int nx, uint64_t seed, uint64_t sid, int nreal, const T* cs, cx<T>* out, long zstride, int tiles, int plain) {
    if (ny < 32 || nx < 4 || nreal < 1 || (ny & (ny - 1)) || (nx & (nx - 1))) return 1;
    Holder<T> hd(ny, nx);
    if (zstride < (long)ny * hd.p.kp) return 2;
    GrfEmuLauncher q;
    if (tiles > 0) q.tiles = tiles;
    q.plain = plain != 0;
    hd.p.grf_icols(q, seed, sid, nreal, cs, out, zstride);
    return 0;
}

extern "C" {
long emu_grf_kpitch(int nx) { return kpitch_for(nx); }
int emu_grf_icols_f64(int ny, int nx, uint64_t seed, uint64_t sid, int nreal, const double* cs, void* out, long zstride, int tiles, int plain) {
    return do_grf_icols<double>(ny, nx, seed, sid, nreal, cs, (cx<double>*)out, zstride, tiles, plain);
}
int emu_grf_icols_f32(int ny, int nx, uint64_t seed, uint64_t sid, int nreal, const float* cs, void* out, long zstride, int tiles, int plain) {
    return do_grf_icols<float>(ny, nx, seed, sid, nreal, cs, (cx<float>*)out, zstride, tiles, plain);
}
}
