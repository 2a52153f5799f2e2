// CPU thread emulator, windowed front end of oa_mc_run_windowed on map sides 2^a 3^b 5^c (TEST INFRASTRUCTURE): band_rows_win_body
// (orphics_amd/csrc/fft_band.hpp) with the grid and LDS of the HIP launcher (band_win_r2c, band.hip), alone and behind the inverse column
// transform (mr_col_body) and in front of the pruned column DFT (band_cols_body + band_cols_fold_body); and the unfused flow's row pass
// (mr_row_body, MR_C2R with MrRowArgs::mul).  Built on the emulators of emul_band.cpp / emul_fft.cpp.
#include "emul_band.cpp"

// in: B planes of (ny, kp) complex, already inverse-transformed along y; win: (ny, nx) reals; out: B row planes of (ny, wl) complex
template <typename T>
static int do_band_rows_win(int ny, int nx, int B, const cx<T>* in, long kp, const T* win, double scale, int wl, cx<T>* out) {
    const int N = nx / 2;
    if ((nx & 1) || !mixed_ok(N) || !band_rows_win_fits(N) || B < 1 || B > BAND_MAPS_MAX || wl < 1 || wl > N || kp < N + 1) return 1;
    const auto twx = band_twiddles<T>(nx, 1), twxh = band_twiddles<T>(N, 0);
    BandRowsWinArgs<T> a{};
    a.in = in; a.in_pitch = kp; a.in_bstride = (long)ny * kp; a.win = win; a.out = out; a.out_bstride = (long)ny * wl; a.w = wl; a.N = N;
    a.scale = (T)scale; a.f = mixed_factor(N); a.tw = twxh.data(); a.tw2 = twx.data();
    EmuLauncher q;
    q.run(ny, B, BRW_NT, band_rows_lds<T>(N), [&](EmuCtx& c) { band_rows_win_body<T>(c, a); });
    return 0;
}

template <typename T>
static void cols_inverse(int ny, const cx<T>* in, cx<T>* out, long kp, int width, const cx<T>* twy) {
    MrColArgs<T> a{};
    a.in = in; a.out = out; a.in_pitch = kp; a.out_pitch = kp; a.N = ny; a.width = width; a.logC = mr_col_logc<T>(ny); a.f = mixed_factor(ny);
    a.tw = twy; a.scale = (T)1; a.inverse = 1;
    const int C = 1 << a.logC;
    EmuLauncher q;
    q.run((width + C - 1) / C, 1, 256, mr_col_lds<T>(ny, a.logC), [&](EmuCtx& c) { mr_col_body<T>(c, a); });
}

// hc: one (ny, kp) spectrum plane (overwritten by its inverse column transform, in place as the sequencer runs it) -> the leg band of
// rfft2(irfft2(hc) * win) (irfft2 with its 1 / Npix) in the inner plane out (my, okp)
template <typename T>
static int do_win_front(int ny, int nx, cx<T>* hc, long kp, const T* win, int wl, int rl, cx<T>* out, long okp, int my) {
    const int N = nx / 2;
    if ((nx & 1) || !mixed_ok(N) || !mixed_ok(ny) || wl < 1 || wl > N || rl < 1 || 2 * rl - 1 > (ny < my ? ny : my) || wl > okp) return 1;
    const auto twy = band_twiddles<T>(ny, 0);
    cols_inverse<T>(ny, hc, hc, kp, N + 1, twy.data());
    std::vector<cx<T>> rows((size_t)ny * wl);
    if (int rc = do_band_rows_win<T>(ny, nx, 1, hc, kp, win, 1.0 / ((double)ny * nx), wl, rows.data())) return rc;
    BandColsArgs<T> ca{};
    ca.rows = rows.data(); ca.rows_mstride = (long)ny * wl; ca.ny = ny; ca.w = wl; ca.rl = rl;
    ca.nseg = band_cols_segments(ny, wl, rl, &ca.yseg);
    ca.tw = twy.data();
    const int nk = 2 * rl - 1;
    std::vector<cx<double>> part((size_t)ca.nseg * nk * wl);
    ca.part = part.data();
    EmuLauncher q;
    q.run((wl + BC_TX - 1) / BC_TX, (nk + BC_TK - 1) / BC_TK, 256, band_cols_lds<1>(), [&](EmuCtx& c) { band_cols_body<T, 1>(c, ca); }, ca.nseg);
    BandFoldArgs<T> fa{};
    fa.part = part.data(); fa.nmaps = 1; fa.nseg = ca.nseg; fa.w = wl; fa.rl = rl; fa.ny = ny;
    fa.out = out; fa.out_mstride = (long)my * okp; fa.okp = okp; fa.my = my;
    q.run((wl + 255) / 256, nk, 256, 0, [&](EmuCtx& c) { band_cols_fold_body<T>(c, fa); });
    return 0;
}

// the unfused flow's C2R: hc (ny, kp) -> inverse columns -> MR_C2R rows x scale x win at the store -> out (ny, nx) reals
template <typename T>
static int do_c2r_win(int ny, int nx, const cx<T>* hc, long kp, const T* win, double scale, T* out) {
    const int N = nx / 2;
    if ((nx & 1) || !mixed_ok(N) || !mixed_ok(ny) || kp < N + 1) return 1;
    const auto twx = band_twiddles<T>(nx, 1), twxh = band_twiddles<T>(N, 0), twy = band_twiddles<T>(ny, 0);
    std::vector<cx<T>> tmp((size_t)ny * kp);
    cols_inverse<T>(ny, hc, tmp.data(), kp, N + 1, twy.data());
    MrRowArgs<T> a{};
    a.in = tmp.data(); a.out = out; a.in_pitch = kp; a.out_pitch = nx; a.N = N; a.f = mixed_factor(N); a.tw = twxh.data(); a.tw2 = twx.data();
    a.scale = (T)scale; a.mode = MR_C2R; a.mul = win;
    EmuLauncher q;
    q.run(ny, 1, 256, mr_row_lds<T>(N), [&](EmuCtx& c) { mr_row_body<T>(c, a); });
    return 0;
}

extern "C" {
int emu_band_rows_win_f64(int ny, int nx, int B, const void* in, long kp, const double* win, double scale, int wl, void* out) {
    return do_band_rows_win<double>(ny, nx, B, (const cx<double>*)in, kp, win, scale, wl, (cx<double>*)out);
}
int emu_band_rows_win_f32(int ny, int nx, int B, const void* in, long kp, const float* win, double scale, int wl, void* out) {
    return do_band_rows_win<float>(ny, nx, B, (const cx<float>*)in, kp, win, scale, wl, (cx<float>*)out);
}
int emu_band_win_front_f64(int ny, int nx, void* hc, long kp, const double* win, int wl, int rl, void* out, long okp, int my) {
    return do_win_front<double>(ny, nx, (cx<double>*)hc, kp, win, wl, rl, (cx<double>*)out, okp, my);
}
int emu_band_win_front_f32(int ny, int nx, void* hc, long kp, const float* win, int wl, int rl, void* out, long okp, int my) {
    return do_win_front<float>(ny, nx, (cx<float>*)hc, kp, win, wl, rl, (cx<float>*)out, okp, my);
}
int emu_c2r_win_f64(int ny, int nx, const void* hc, long kp, const double* win, double scale, double* out) {
    return do_c2r_win<double>(ny, nx, (const cx<double>*)hc, kp, win, scale, out);
}
int emu_c2r_win_f32(int ny, int nx, const void* hc, long kp, const float* win, double scale, float* out) {
    return do_c2r_win<float>(ny, nx, (const cx<float>*)hc, kp, win, scale, out);
}
}
