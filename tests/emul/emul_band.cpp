// CPU thread emulator, batched band input stage of oa_qe_mv_maps (TEST INFRASTRUCTURE): band_rows_body, band_cols_body and
// band_cols_fold_body (orphics_amd/csrc/fft_band.hpp) with the grids, the segment rule and the scratch layout of the HIP launcher
// (band_maps_r2c, band.hip).  Built on the emulator of emul_fft.cpp.
#include "emul_fft.cpp"
#include "../../orphics_amd/csrc/fft_band.hpp"

template <typename T>
static std::vector<cx<T>> band_twiddles(int N, int extra) {
    std::vector<cx<T>> t((size_t)N + extra);
    const long double tau = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < N + extra; ++k) { const long double x = tau * k / (long double)N; t[(size_t)k] = mk<T>((T)cosl(x), (T)(-sinl(x))); }
    return t;
}

// maps: nmaps planes of ny x nx reals, back to back; rot_c / rot_s: nullptr or (ny, rot_pitch) planes; out: nmaps inner planes of
// (my, okp) complex, ostride elements apart (only the band is written)
template <typename T>
static int do_band_maps(int ny, int nx, int nmaps, const T* maps, const T* rot_c, const T* rot_s, long rot_pitch, int wl, int rl, cx<T>* out,
                        long ostride, long okp, int my) {
    const int N = nx / 2;
    if ((nx & 1) || !mixed_ok(N) || nmaps < 1 || nmaps > BAND_MAPS_MAX || wl < 1 || wl > N || rl < 1 || 2 * rl - 1 > (ny < my ? ny : my) || wl > okp ||
        (long)my * okp > ostride)
        return 1;
    if ((rot_c != nullptr) != (rot_s != nullptr) || (rot_c && nmaps != 3 && nmaps != 6)) return 2;
    const auto twx = band_twiddles<T>(nx, 1), twxh = band_twiddles<T>(N, 0), twy = band_twiddles<T>(ny, 0);
    std::vector<cx<T>> rows((size_t)nmaps * ny * wl);
    EmuLauncher q;
    BandRowsArgs<T> ra{};
    for (int m = 0; m < BAND_MAPS_MAX; ++m) ra.maps.m[m] = maps + (size_t)(m < nmaps ? m : 0) * ny * nx;
    ra.out = rows.data(); ra.in_pitch = nx; ra.out_mstride = (long)ny * wl; ra.w = wl; ra.N = N; ra.f = mixed_factor(N);
    ra.tw = twxh.data(); ra.tw2 = twx.data();
    q.run(ny, nmaps, 256, band_rows_lds<T>(N), [&](EmuCtx& c) { band_rows_body<T>(c, ra); });
    BandColsArgs<T> ca{};
    ca.rows = rows.data(); ca.rows_mstride = ra.out_mstride; ca.ny = ny; ca.w = wl; ca.rl = rl;
    ca.nseg = band_cols_segments(ny, wl, rl, &ca.yseg);
    ca.tw = twy.data();
    const int nk = 2 * rl - 1;
    std::vector<cx<double>> part((size_t)nmaps * ca.nseg * nk * wl);
    ca.part = part.data();
    const int gx = (wl + BC_TX - 1) / BC_TX, gy = (nk + BC_TK - 1) / BC_TK;
    switch (nmaps) {
        case 1: q.run(gx, gy, 256, band_cols_lds<1>(), [&](EmuCtx& c) { band_cols_body<T, 1>(c, ca); }, ca.nseg); break;
        case 2: q.run(gx, gy, 256, band_cols_lds<2>(), [&](EmuCtx& c) { band_cols_body<T, 2>(c, ca); }, ca.nseg); break;
        case 3: q.run(gx, gy, 256, band_cols_lds<3>(), [&](EmuCtx& c) { band_cols_body<T, 3>(c, ca); }, ca.nseg); break;
        case 4: q.run(gx, gy, 256, band_cols_lds<4>(), [&](EmuCtx& c) { band_cols_body<T, 4>(c, ca); }, ca.nseg); break;
        case 5: q.run(gx, gy, 256, band_cols_lds<5>(), [&](EmuCtx& c) { band_cols_body<T, 5>(c, ca); }, ca.nseg); break;
        default: q.run(gx, gy, 256, band_cols_lds<6>(), [&](EmuCtx& c) { band_cols_body<T, 6>(c, ca); }, ca.nseg); break;
    }
    BandFoldArgs<T> fa{};
    fa.part = part.data(); fa.nmaps = nmaps; fa.nseg = ca.nseg; fa.w = wl; fa.rl = rl;
    fa.rot_c = rot_c; fa.rot_s = rot_s; fa.rot_pitch = rot_pitch; fa.ny = ny;
    fa.out = out; fa.out_mstride = ostride; fa.okp = okp; fa.my = my;
    q.run((wl + 255) / 256, nk, 256, 0, [&](EmuCtx& c) { band_cols_fold_body<T>(c, fa); });
    return 0;
}

extern "C" {
int emu_band_maps_f64(int ny, int nx, int nmaps, const double* maps, const double* rot_c, const double* rot_s, long rot_pitch, int wl, int rl,
                      void* out, long ostride, long okp, int my) {
    return do_band_maps<double>(ny, nx, nmaps, maps, rot_c, rot_s, rot_pitch, wl, rl, (cx<double>*)out, ostride, okp, my);
}
int emu_band_maps_f32(int ny, int nx, int nmaps, const float* maps, const float* rot_c, const float* rot_s, long rot_pitch, int wl, int rl,
                      void* out, long ostride, long okp, int my) {
    return do_band_maps<float>(ny, nx, nmaps, maps, rot_c, rot_s, rot_pitch, wl, rl, (cx<float>*)out, ostride, okp, my);
}
int emu_band_segments(int ny, int wl, int rl) { int ys = 0; return band_cols_segments(ny, wl, rl, &ys); }
}
