// CPU thread emulator, the mixed T, Q, U draw inside inverse column pass 1 (TEST INFRASTRUCTURE): col_mix_body / MixColLoad /
// mix_col_normals / mix_col_fill of orphics_amd/csrc/fft_kernels.hpp with the grid, workgroup size and LDS of their HIP launcher
// (Fft2dPlan::grf_mix_icols), then the in-place pass 2.  The lane-pair exchange goes through the column tile here (threads have no lanes).
// Host logf / sinf / cosf are not the device's: this pins counters, edge rules, mixing, rotation and index mapping, not bits.  Built on the
// emulator of emul_fft.cpp.
#include <algorithm>
#include "emul_fft.cpp"

// one plane of a triple as a load functor of the plain pipeline: MixColLoad::get, one evaluation of the three streams per ELEMENT
template <typename T>
struct MixPlaneLoad {
    static constexpr bool reads_lds = false;
    const MixColLoad<T>* ld;
    int plane;
    template <typename U> cx<U> get(int n, int c) const { return ld->template get<U>(n, c, plane); }
};

// the same pass 1 with the per-element statement in the place of the once-per-triple evaluation: what col_mix_body must reproduce bit for
// bit on the same host
template <typename T, class SEQ, class Ctx>
static void col_mix_plain_body(Ctx& ctx, const MixColArgs<T>& a) {
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
    const long t = ctx.bid_z();
    const MixColLoad<T> ld{a.seed, a.sid + 3 * (uint64_t)t, a.cs, a.rc, a.rs, a.pitch, a.ny, a.nxh, a.nxh / 2 + 1, (int)g, (int)a.in_ns, c0, ncols};
    for (int c = 0; c < 3; ++c) {
        const ColStore<T> st{a.out + (3 * t + c) * a.out_zstride + g * a.out_gs * a.pitch + c0, (unsigned)a.pitch, ncols, true,
                             a.twiddle ? ti : nullptr, (unsigned)g, (T)1, 0, 0, 0, 0};
        const MixPlaneLoad<T> pl{&ld, c};
        fft_pipeline<T, false, true, true, SEQ>(ctx, s, tid, CNT, logL, CLC, 0, twl, logL, pl, st);
        ctx.sync();
    }
}

struct MixEmuLauncher : EmuLauncher {
    int tiles = 1 << 30;        // column tiles run (the others are left untouched)
    bool plain = false;
    template <typename T> void col_mix(int gx, int gy, int nt, size_t smem, const MixColArgs<T>& a, int nz) {
        dispatch_seq(a.logL, [&](auto seq) {
            using S = decltype(seq);
            if constexpr (seq_total_log<S>() <= 8) {
                if (plain) run(std::min(gx, tiles), gy, nt, smem, [&](EmuCtx& c) { col_mix_plain_body<T, S>(c, a); }, nz);
                else run(std::min(gx, tiles), gy, nt, smem, [&](EmuCtx& c) { col_mix_body<T, S>(c, a); }, nz);
            }
        });
    }
    template <typename T> void col(int gx, int gy, int nt, size_t smem, const ColArgs<T>& a, int nz = 1) {
        EmuLauncher::col<T>(std::min(gx, tiles), gy, nt, smem, a, nz);
    }
};

template <typename T>
static int do_mix_icols(int ny, int nx, uint64_t seed, uint64_t sid, int ntriples, const T* const* cs, const T* rc, const T* rs, cx<T>* out,
                        long zstride, int tiles, int plain) {
    if (ny < 32 || nx < 4 || ntriples < 1 || (ny & (ny - 1)) || (nx & (nx - 1))) return 1;
    Holder<T> hd(ny, nx);
    if (zstride < (long)ny * hd.p.kp) return 2;
    if ((rc == nullptr) != (rs == nullptr)) return 3;
    MixEmuLauncher q;
    if (tiles > 0) q.tiles = tiles;
    q.plain = plain != 0;
    hd.p.grf_mix_icols(q, seed, sid, ntriples, cs, rc, rs, out, zstride);
    return 0;
}

extern "C" {
long emu_mix_kpitch(int nx) { return kpitch_for(nx); }
// cs: nine (ny, kp) real planes or NULL; rc, rs: the Q, U -> E, B planes or both NULL
int emu_grf_mix_icols_f64(int ny, int nx, uint64_t seed, uint64_t sid, int ntriples, const double* const* cs, const double* rc, const double* rs,
                          void* out, long zstride, int tiles, int plain) {
    return do_mix_icols<double>(ny, nx, seed, sid, ntriples, cs, rc, rs, (cx<double>*)out, zstride, tiles, plain);
}
int emu_grf_mix_icols_f32(int ny, int nx, uint64_t seed, uint64_t sid, int ntriples, const float* const* cs, const float* rc, const float* rs,
                          void* out, long zstride, int tiles, int plain) {
    return do_mix_icols<float>(ny, nx, seed, sid, ntriples, cs, rc, rs, (cx<float>*)out, zstride, tiles, plain);
}
}
