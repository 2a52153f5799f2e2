// CPU thread emulator, the pieces of oa_mc_run_mv_windowed on map sides 2^a 3^b 5^c (TEST INFRASTRUCTURE): the mean-field stacks from the
// inner planes of a band grid (band_stack_add_multi_body, orphics_amd/csrc/mc_pol.hpp), the mixed-radix column transform of several planes
// in one launch (mr_col_body with the plane on grid y, orphics_amd/csrc/fft_mixed.hpp) and the pruned column DFT of three row planes with
// the Q, U -> E, B rotation in the fold (band_cols_body<T, 3> + band_cols_fold_body, orphics_amd/csrc/fft_band.hpp), each with the grid
// and LDS of its HIP launcher.  Built on the emulators of emul_band.cpp / emul_fft.cpp.
#include "emul_band.cpp"
#include "../../orphics_amd/csrc/mc_pol.hpp"

// k: nest inner planes (iny, ipitch) complex, kstride apart; wt: nest inner real planes, wstride apart; acc: nest (+ 1 with has_mv)
// float64 N-grid planes of (any, apitch, 2), contiguous
template <typename T>
static int do_band_stack_multi(const cx<T>* k, long kstride, const T* wt, long wstride, int nest, double* acc, int has_mv, int iny, long ipitch,
                               int any, long apitch, int w, int r) {
    if (nest < 1 || nest > STACK_MULTI_MAX || (has_mv && !wt)) return 1;
    if (w < 1 || r < 1 || 2L * r - 1 > (iny < any ? iny : any) || w > ipitch || w > apitch) return 2;
    BandStackMultiArgs<T> a{};
    a.k = k; a.kstride = kstride; a.wt = has_mv ? wt : nullptr; a.wstride = wstride;
    for (int e = 0; e < nest; ++e) a.acc[e] = (cx<double>*)acc + (long)e * any * apitch;
    a.acc_mv = has_mv ? (cx<double>*)acc + (long)nest * any * apitch : nullptr;
    a.ipitch = ipitch; a.iny = iny; a.apitch = apitch; a.any = any; a.nest = nest; a.w = w; a.r = r;
    EmuLauncher q;
    q.run((w + 63) / 64, 2 * r - 1, 64, 0, [&](EmuCtx& ctx) { band_stack_add_multi_body<T>(ctx, a); });
    return 0;
}

// nplanes planes of (ny, pitch) complex, pstride apart, transformed along y over `width` columns in ONE launch (grid y = plane);
// out == in: in place.  ip: the in-place stages (one LDS buffer per workgroup)
template <typename T>
static int do_cols_batch(int ny, int nplanes, const cx<T>* in, cx<T>* out, long pitch, int width, int inverse, long pstride, int ip) {
    if (!mixed_ok(ny) || nplanes < 1 || width < 1 || width > pitch || (nplanes > 1 && pstride < (long)ny * pitch)) return 1;
    const auto twy = band_twiddles<T>(ny, 0);
    MrColArgs<T> a{};
    a.in = in; a.out = out; a.in_pitch = pitch; a.out_pitch = pitch; a.N = ny; a.width = width; a.logC = mr_col_logc<T>(ny); a.f = mixed_factor(ny);
    a.tw = twy.data(); a.scale = (T)1; a.inverse = inverse ? 1 : 0;
    a.in_pstride = nplanes > 1 ? pstride : 0; a.out_pstride = a.in_pstride;
    const int C = 1 << a.logC;
    EmuLauncher q;
    if (!ip) { q.run((width + C - 1) / C, nplanes, 256, mr_col_lds<T>(ny, a.logC), [&](EmuCtx& c) { mr_col_body<T>(c, a); }); return 0; }
    const int nt = ip_threads(a.f, ny, a.logC);
    if (!nt) return 2;
    q.run((width + C - 1) / C, nplanes, nt, ((size_t)ny << a.logC) * sizeof(cx<T>), [&](EmuCtx& c) { mr_col_body<T, true>(c, a); });
    return 0;
}

// rows: three row planes of (ny, wl) complex, back to back (T, Q, U); rot_c / rot_s: nullptr or (ny, rot_pitch) planes; out: three inner
// planes of (my, okp) complex, ostride apart (only the band is written)
template <typename T>
static int do_band_cols3(int ny, const cx<T>* rows, int wl, int rl, const T* rot_c, const T* rot_s, long rot_pitch, cx<T>* out, long ostride,
                         long okp, int my) {
    if (wl < 1 || rl < 1 || 2 * rl - 1 > (ny < my ? ny : my) || wl > okp || (long)my * okp > ostride) return 1;
    if ((rot_c != nullptr) != (rot_s != nullptr) || (rot_c && wl > rot_pitch)) return 2;
    const auto twy = band_twiddles<T>(ny, 0);
    BandColsArgs<T> ca{};
    ca.rows = rows; ca.rows_mstride = (long)ny * wl; ca.ny = ny; ca.w = wl; ca.rl = rl;
    ca.nseg = band_cols_segments(ny, wl, rl, &ca.yseg);
    ca.tw = twy.data();
    const int nk = 2 * rl - 1;
    std::vector<cx<double>> part((size_t)3 * ca.nseg * nk * wl);
    ca.part = part.data();
    EmuLauncher q;
    q.run((wl + BC_TX - 1) / BC_TX, (nk + BC_TK - 1) / BC_TK, 256, band_cols_lds<3>(), [&](EmuCtx& c) { band_cols_body<T, 3>(c, ca); }, ca.nseg);
    BandFoldArgs<T> fa{};
    fa.part = part.data(); fa.nmaps = 3; fa.nseg = ca.nseg; fa.w = wl; fa.rl = rl;
    fa.rot_c = rot_c; fa.rot_s = rot_s; fa.rot_pitch = rot_pitch; fa.ny = ny;
    fa.out = out; fa.out_mstride = ostride; fa.okp = okp; fa.my = my;
    q.run((wl + 255) / 256, nk, 256, 0, [&](EmuCtx& c) { band_cols_fold_body<T>(c, fa); });
    return 0;
}

extern "C" {
int emu_band_stack_multi_f64(const void* k, long kstride, const double* wt, long wstride, int nest, double* acc, int has_mv, int iny, long ipitch,
                             int any, long apitch, int w, int r) {
    return do_band_stack_multi<double>((const cx<double>*)k, kstride, wt, wstride, nest, acc, has_mv, iny, ipitch, any, apitch, w, r);
}
int emu_band_stack_multi_f32(const void* k, long kstride, const float* wt, long wstride, int nest, double* acc, int has_mv, int iny, long ipitch,
                             int any, long apitch, int w, int r) {
    return do_band_stack_multi<float>((const cx<float>*)k, kstride, wt, wstride, nest, acc, has_mv, iny, ipitch, any, apitch, w, r);
}
int emu_cols_batch_f64(int ny, int nplanes, const void* in, void* out, long pitch, int width, int inverse, long pstride, int ip) {
    return do_cols_batch<double>(ny, nplanes, (const cx<double>*)in, (cx<double>*)out, pitch, width, inverse, pstride, ip);
}
int emu_cols_batch_f32(int ny, int nplanes, const void* in, void* out, long pitch, int width, int inverse, long pstride, int ip) {
    return do_cols_batch<float>(ny, nplanes, (const cx<float>*)in, (cx<float>*)out, pitch, width, inverse, pstride, ip);
}
int emu_band_cols3_f64(int ny, const void* rows, int wl, int rl, const double* rot_c, const double* rot_s, long rot_pitch, void* out, long ostride,
                       long okp, int my) {
    return do_band_cols3<double>(ny, (const cx<double>*)rows, wl, rl, rot_c, rot_s, rot_pitch, (cx<double>*)out, ostride, okp, my);
}
int emu_band_cols3_f32(int ny, const void* rows, int wl, int rl, const float* rot_c, const float* rot_s, long rot_pitch, void* out, long ostride,
                       long okp, int my) {
    return do_band_cols3<float>(ny, (const cx<float>*)rows, wl, rl, rot_c, rot_s, rot_pitch, (cx<float>*)out, ostride, okp, my);
}
}
