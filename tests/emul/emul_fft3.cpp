// CPU thread emulator, 3 x 2^k column grids of the from-map R-split path (TEST INFRASTRUCTURE): col_fband3_body (fft_fband.hpp),
// the row stage on R-LAYOUT planes of 3 x 2^k rows and col_div3_body (fft_kernels.hpp), driven through the same host plan code
// (Fft2dPlan::legs_fband3 / rows_qe / cols_div3) as the HIP launcher.  Built on the emulator of emul_fft.cpp.
#include "emul_fft.cpp"

struct EmuLauncher3 : EmuLauncher {
    template <typename T> void col_fband3(int gx, int gz, size_t smem, int logMy, const ColFBandArgs<T>& a) {
        constexpr int nt = sizeof(T) == 4 ? 1024 : 512;
        constexpr int lc11 = sizeof(T) == 4 ? 3 : 2, lc10 = lc11 + 1;
        if (logMy == 11) run(gx, 4, nt, smem, [&](EmuCtx& c) { col_fband3_body<T, Seq<16, 16, 8>, lc11>(c, a); }, gz);
        else if (logMy == 10) run(gx, 4, nt, smem, [&](EmuCtx& c) { col_fband3_body<T, Seq<16, 8, 8>, lc10>(c, a); }, gz);
    }
    template <typename T> void col_fband3_pack(int gx, int logMy, const ColFBandArgs<T>& a, cx<T>* out) {
        constexpr int nt = sizeof(T) == 4 ? 1024 : 512;
        constexpr int lc11 = sizeof(T) == 4 ? 3 : 2, lc10 = lc11 + 1;
        if (logMy == 11) run(gx, 4, nt, 0, [&](EmuCtx& c) { col_fband3_pack_body<T, Seq<16, 16, 8>, lc11>(c, a, out); });
        else if (logMy == 10) run(gx, 4, nt, 0, [&](EmuCtx& c) { col_fband3_pack_body<T, Seq<16, 8, 8>, lc10>(c, a, out); });
    }
    template <typename T> void col_div3(int gx, size_t smem, int rows, const ColDivArgs<T>& a, int gz = 1) {
        constexpr int lc = sizeof(T) == 4 ? 3 : 2;
        if (rows == 1536) run(gx, 1, a.NT, smem, [&](EmuCtx& c) { col_div3_body<T, 8, lc>(c, a); }, gz);
        else if (rows == 768) run(gx, 1, a.NT, smem, [&](EmuCtx& c) { col_div3_body<T, 7, lc + 1>(c, a); }, gz);
    }
};

// view of a (ny_full, nx) map on a column grid of `rows` rows (any length: tw_y = W_rows)
template <typename T>
struct GridHolder {
    std::vector<cx<T>> twx, twy, rq8t[RQ8_NGRIDS];
    Fft2dPlan<T> p;
    GridHolder(int ny_full, int rows, int nx) {
        twx = make_twiddles<T>(nx);
        twy = make_twiddles<T>(rows);
        p.ny = rows; p.nx = nx; p.logNy = is_pow2(rows) ? ilog2(rows) : -1; p.logNx = ilog2(nx);
        p.kp = kpitch_for(nx); p.tw_x = twx.data(); p.tw_y = twy.data(); p.ny_full = ny_full;
        for (int i = 0; i < RQ8_NGRIDS; ++i) if (512 * RQ8_WAVES[i] <= nx) { rq8t[i] = rq8_make_consts<T>(RQ8_WAVES[i]); p.rq8c[i] = rq8t[i].data(); }
    }
};

template <typename T>
static int do_fband3(int ny, int nx, const cx<T>* Y, long pitch, const T* FG, const T* FH, const T* lxd, const T* lyd, cx<T>* gx, cx<T>* gy, cx<T>* h,
                     long opitch, int width, int rband, int nmaps, long in_moff, long out_moff, int packed) {
    const int myf = ny / 4, my3 = myf / 4 * 3;
    Holder<T> hd(ny, nx);
    GridHolder<T> cv(ny, my3, nx);
    if (!Fft2dPlan<T>::has_rsplit3(hd.p.logNy, hd.p.logNx, my3, hd.p.clampw(width))) return 1;
    auto twf = make_twiddles<T>(myf);
    EmuLauncher3 q;
    if (packed) {
        std::vector<cx<T>> tab((size_t)hd.p.fband3_table_entries(cv.p, width));
        hd.p.legs_fband3(q, cv.p, twf.data(), (const cx<T>*)nullptr, 0, 0, FG, FH, lxd, lyd, (cx<T>*)nullptr, (cx<T>*)nullptr, (cx<T>*)nullptr, width, rband, 0, 1,
                         0, 0, (const cx<T>*)nullptr, tab.data());
        hd.p.legs_fband3(q, cv.p, twf.data(), Y, (long)myf * pitch, pitch, (const T*)nullptr, (const T*)nullptr, lxd, lyd, gx, gy, h, width, rband, opitch, nmaps,
                         in_moff, out_moff, tab.data());
        return 0;
    }
    hd.p.legs_fband3(q, cv.p, twf.data(), Y, (long)myf * pitch, pitch, FG, FH, lxd, lyd, gx, gy, h, width, rband, opitch, nmaps, in_moff, out_moff);
    return 0;
}

template <typename T>
static int do_cols_div3(int ny_full, int my3, int nx, const cx<T>* pa, const cx<T>* pb, const T* Fn, const T* lxd, const T* lyd, cx<T>* out, int width,
                        int rband, long pin, int nmaps, long in_moff, long out_moff) {
    if (my3 != 1536 && my3 != 768) return 1;
    GridHolder<T> cv(ny_full, my3, nx);
    EmuLauncher3 q;
    cv.p.cols_div3(q, pa, pb, Fn, lxd, lyd, out, 0, width, rband, pin, nmaps, in_moff, out_moff, 0);
    return 0;
}

// the from-map chain behind the row R2C on the column grid `my` (3 x 2^k or the power of two 4/3 of it): Y -> leg planes (R-LAYOUT) ->
// row stage -> divergence into the full-resolution plane `out` (pitch kp)
template <typename T>
static int do_chain(int ny, int nx, int my, const cx<T>* Y, long pitch, const T* FG, const T* FH, const T* Fn, const T* lxd, const T* lyd, cx<T>* out,
                    int wl, int wk, int rl, int rk, int mrow) {
    const int myf = ny / 4;
    Holder<T> hd(ny, nx);
    GridHolder<T> cv(ny, my, nx);
    const long kp = hd.p.kp;
    std::vector<cx<T>> c0((size_t)my * kp), c1((size_t)my * kp), c2((size_t)my * kp), g0((size_t)my * kp), g1((size_t)my * kp);
    EmuLauncher3 q;
    const int wi = hd.p.clampw(wl), wo = hd.p.clampw(wk);
    if (!cv.p.rows_qe_is_pair(wi, wo, mrow)) return 2;
    const double s = 1.0 / ((double)ny * nx), sy = (double)ny / my;
    if (is_m3(my)) {
        if (!Fft2dPlan<T>::has_rsplit3(hd.p.logNy, hd.p.logNx, my, wi)) return 1;
        auto twf = make_twiddles<T>(myf);
        hd.p.legs_fband3(q, cv.p, twf.data(), Y, (long)myf * pitch, pitch, FG, FH, lxd, lyd, c0.data(), c1.data(), c2.data(), wl, rl, kp);
    } else {
        if (my != myf) return 1;
        hd.p.legs_fband(q, cv.p, Y, (long)myf * pitch, pitch, FG, FH, lxd, lyd, c0.data(), c1.data(), c2.data(), wl, rl, kp);
    }
    cv.p.rows_qe(q, c0.data(), c1.data(), c2.data(), g0.data(), g1.data(), (T)(s * s * sy), 0, wi, wo, mrow, 0, 0, 1, 0, 0, -1, nullptr, 2);
    if (is_m3(my)) cv.p.cols_div3(q, g0.data(), g1.data(), Fn, lxd, lyd, out, 0, wk, rk);
    else {
        std::vector<cx<T>> tA((size_t)my * kp), tB((size_t)my * kp);
        cv.p.cols_div(q, g0.data(), g1.data(), Fn, lxd, lyd, out, tA.data(), tB.data(), 0, wk, rk);
    }
    return 0;
}

extern "C" {
#define EMU3(SUF, T)                                                                                                                                  \
    int emu3_fband_##SUF(int ny, int nx, const void* Y, long pitch, const void* FG, const void* FH, const void* lxd, const void* lyd, void* gx, void* gy, \
                         void* h, long opitch, int width, int rband, int nmaps, long in_moff, long out_moff, int packed) {                            \
        return do_fband3<T>(ny, nx, (const cx<T>*)Y, pitch, (const T*)FG, (const T*)FH, (const T*)lxd, (const T*)lyd, (cx<T>*)gx, (cx<T>*)gy, (cx<T>*)h,   \
                            opitch, width, rband, nmaps, in_moff, out_moff, packed);                                                                  \
    }                                                                                                                                                 \
    int emu3_cols_div_##SUF(int ny_full, int my3, int nx, const void* pa, const void* pb, const void* Fn, const void* lxd, const void* lyd, void* out,    \
                            int width, int rband, long pin, int nmaps, long in_moff, long out_moff) {                                                 \
        return do_cols_div3<T>(ny_full, my3, nx, (const cx<T>*)pa, (const cx<T>*)pb, (const T*)Fn, (const T*)lxd, (const T*)lyd, (cx<T>*)out, width,     \
                               rband, pin, nmaps, in_moff, out_moff);                                                                                 \
    }                                                                                                                                                 \
    int emu3_chain_##SUF(int ny, int nx, int my, const void* Y, long pitch, const void* FG, const void* FH, const void* Fn, const void* lxd,             \
                         const void* lyd, void* out, int wl, int wk, int rl, int rk, int mrow) {                                                      \
        return do_chain<T>(ny, nx, my, (const cx<T>*)Y, pitch, (const T*)FG, (const T*)FH, (const T*)Fn, (const T*)lxd, (const T*)lyd, (cx<T>*)out, wl,  \
                           wk, rl, rk, mrow);                                                                                                         \
    }
EMU3(f64, double)
EMU3(f32, float)
#undef EMU3
}
