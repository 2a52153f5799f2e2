/*
 * orphics_amd C-ABI -- MI355X (gfx950) kernels for the flat-sky CMB lensing
 * quadratic-estimator hot path of msyriac/orphics.
 *
 * The reference has NO native/FFI layer: the hot path is Python
 * calling NumPy / pixell.  Each entry point below therefore replaces a NumPy /
 * pixell expression inside a reference function; the reference file:line is
 * cited per function.  The Python classes in orphics_amd/{maps,stats,lensing}.py
 * mirror the reference signatures and bind these symbols with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on error; oa_last_error()
 *    returns the message of the calling thread's last failure; nothing throws;
 *  - all data pointers are DEVICE pointers unless the name says `host_`;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *    work is stream-ordered, no call synchronises unless documented;
 *  - dtype: OA_F32 (float / complex64 planes) or OA_F64 (double / complex128);
 *  - real planes are (ny, nx) row-major; "hc" (half-complex) planes are
 *    (ny, kpitch) complex row-major with kpitch = oa_plan_kpitch(plan)
 *    = nx/2 + 16; columns [0, nx/2] are valid (numpy rfft2 layout), the pad
 *    columns are never read as data and are left untouched;
 *    "full" complex planes are (ny, nx) row-major (numpy fft2 layout);
 *  - a plan is bound to the device current at creation, owns its twiddle tables
 *    and scratch planes, and is not thread-safe (one plan per stream user).
 */
#ifndef ORPHICS_AMD_H
#define ORPHICS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OA_F32 0
#define OA_F64 1

typedef struct oa_plan oa_plan;

/* ---- library ----------------------------------------------------------- */
const char* oa_last_error(void);
/* ABI version = 100 x the build round that last changed a signature in this header; bindings must refuse a library
 * that reports less than the version they were written against (OA_ABI_VERSION) */
#define OA_ABI_VERSION 416
int oa_version(void);
/* number of HIP devices visible; <0 on error (no compute) */
int oa_device_count(void);

/* ---- plan --------------------------------------------------------------
 * Replaces the per-geometry precomputation of FourierCalc.__init__
 * (maps.py:1600-1607).  ny, nx >= 32.  Powers of two run the LDS-staged FFT kernels and every fused
 * estimator kernel.  Other EVEN sides (<= 8192): sides whose only prime factors are 2, 3 and 5 (the reference notebooks
 * use 600, 750, 1200, 2400) run mixed-radix Stockham transforms (mixed.hip), any other side a chirp-z (Bluestein)
 * evaluation on an inner power-of-two plan -- both exact: oa_fft_r2c / oa_fft_c2r / oa_fft_c2c, oa_lens_maps(_hc) and all
 * per-mode / binning / RNG kernels work, `width` / `rband` hints are ignored, and the fused oa_qe_rows /
 * oa_qe_*_cols / oa_fft_cols / oa_fft_pass calls return an error (use the modular oa_qe_legs .. oa_qe_div chain,
 * as orphics_amd/lensing.py:_reconstruct_hc_modular does).  The one-call entries oa_qe_tt, oa_qe_tt_moments(2), oa_mc_run, oa_qe_pol
 * and oa_qe_mv also take 2^a 3^b 5^c sides, on a BAND GRID (see oa_plan_band_grid, oa_qe_band_bind); chirp-z sides have no one-call path. */
int oa_plan_create(int ny, int nx, int dtype, oa_plan** out);
int oa_plan_destroy(oa_plan* p);
long oa_plan_kpitch(const oa_plan* p);
/* bytes of device scratch currently held by the plan */
long oa_plan_scratch_bytes(const oa_plan* p);
/* Upload the signed multipole axes ly[ny], lx[nx] (host float64; pixell
 * enmap.laxes as used by maps.py:1607,1938).  Needed by the oa_qe_* calls. */
int oa_plan_set_laxes(oa_plan* p, const double* host_ly, const double* host_lx);

/* ---- 2-D FFTs ------------------------------------------------------------
 * oa_fft_r2c : real (ny,nx) -> hc, out = scale * sum x e^{-i l.x}
 *              (enmap.fft(normalize=False), maps.py:1613,1636, restricted to
 *              the non-redundant half plane of a real map)
 * oa_fft_c2r : hc -> real, out = scale * sum_k X e^{+i l.x} (input preserved)
 *              (pixell fft.ifft(...,normalize=True) + np.real, maps.py:1633,1923,
 *              with scale = 1/(ny*nx))
 * oa_fft_c2c : full -> full, forward (inverse=0) or inverse (inverse=1),
 *              out != in (MapGen non-Hermitian draws maps.py:1578-1587, pol legs). */
/* ACTIVE COLUMNS (`width`, `win`, `wout` arguments below): band-limited filters (the k-space masks of
 * lensing.Estimator built with maps.mask_kspace, maps.py:1936-1948: the tellmax / kellmax of
 * tutorials/tt_verification.ipynb) leave every hc plane on the estimator path exactly zero beyond some
 * column kx >= width.  A transform told so neither reads nor produces those columns -- same arithmetic on
 * the remaining ones, so results are unchanged; HBM traffic and column-pass work scale with width/(nx/2+1).
 * width <= 0 (or > nx/2+1) means all columns.  r2c: only columns < width of hc_out are written;
 * c2r / inverse cols: columns >= width of the input are taken as zero and never read.
 * ACTIVE ROWS (`rband`): the same masks also confine the planes to the row band |ky index| < rband, i.e. rows
 * y < rband or y > ny - rband.  rband > 0 on oa_fft_r2c: only the band rows hold the transform (the others are left
 * undefined); on oa_qe_cols_div: rows outside the band are not written;
 * on oa_qe_legs_cols: input rows outside the band are not read (the filters vanish there).  0 = all rows. */
int oa_fft_r2c(oa_plan* p, const void* real_in, void* hc_out, double scale, int width, int rband, void* stream);
int oa_fft_c2r(oa_plan* p, const void* hc_in, void* real_out, double scale, int width, void* stream);
/* oa_fft_c2r with a real-space window multiplied into the result at the last pass's store: real_out = window_real *
 * scale * IDFT(hc_in) (window_real: ny x nx reals of the plan's dtype; power-of-two sides and sides 2^a 3^b 5^c, where the window
 * rides on the store of the mixed-radix C2R row pass; chirp-z sides are refused).  The apodisation step of the
 * reference's analysis flow (maps.py:1350-1361 binned_power(imap * mask)) without another pass over the map. */
int oa_fft_c2r_windowed(oa_plan* p, const void* hc_in, void* real_out, double scale, const void* window_real, void* stream);
int oa_fft_c2c(oa_plan* p, const void* full_in, void* full_out, int inverse, double scale, void* stream);
/* One constituent pass of the transforms above, for per-kernel timing (bench.py roofline):
 * pass_id 0 = R2C row pass (real in -> hc out), 1 = column pass 1 (hc -> hc, out != in),
 * 2 = column pass 2 (in place on `out`; `in` ignored), 3 = C2R row pass (hc -> real). */
int oa_fft_pass(oa_plan* p, int pass_id, const void* in, void* out, int width, void* stream);

/* Column half of the transforms above on an hc plane (all ny-point column DFTs of the nx/2+1
 * valid columns), out != in.  With oa_qe_rows it forms the fused estimator pipeline. */
int oa_fft_cols(oa_plan* p, const void* hc_in, void* hc_out, int inverse, double scale, int width, void* stream);
/* Fused QE row stage: inputs are the three leg planes AFTER their inverse column transforms
 * (oa_fft_cols(..., inverse=1)); per row h = C2R(H), P_x = R2C(C2R(Gx) * h), P_y = R2C(C2R(Gy) * h),
 * product scaled by `scale` (pass (1/(ny*nx))^2 for normalised inverses).  Outputs are row-transformed
 * planes awaiting oa_fft_cols(..., inverse=0).  Replaces 3 x oa_fft_c2r rows + 2 x oa_mul_real +
 * 2 x oa_fft_r2c rows: the real-space planes never touch HBM.  accumulate != 0 adds the result to
 * the existing px, py (estimators whose weight is a sum of separable terms: cos/sin spin-2 pieces;
 * `scale` carries the sign).
 * ROW GRID (`mrow`): legs that vanish beyond column `win` have real-space products band-limited to 2 (win - 1), so
 * the row transforms may run on any grid of mrow >= 2 win + wout points (a power of two <= nx, or 1536 = 3 x 512 when
 * win <= 512 and nx >= 2048): no aliased product frequency reaches the kept columns k < wout, which therefore equal the
 * full-length result (the grid-size factor is folded into the scale; rounding differs at the 1e-7 level in f32).  The
 * real-space planes live in LDS only.
 * mrow = 0: full length nx;  mrow < 0: the smallest alias-free grid of 1024, 1536, 2048, 4096, 8192, ... points;  otherwise
 * checked against the bound. */
int oa_qe_rows(oa_plan* p, const void* gx, const void* gy, const void* h, void* px, void* py, double scale,
               int accumulate, int win, int wout, int mrow, void* stream);

/* Fused estimator column stages (the fast path of lensing.Estimator.reconstruct_*):
 *  oa_qe_legs_cols : oa_qe_legs + oa_fft_cols(inverse) of the three leg planes in one go -- kX, kY and the
 *                    filters are read once per column tile, the filtered legs never exist in HBM
 *                    (outputs feed oa_qe_rows);
 *  oa_qe_cols_div  : oa_fft_cols(forward) of the two oa_qe_rows outputs + oa_qe_div in one go:
 *                    out (+)= Fnorm * (i lx FFT[Px] + i ly FFT[Py]). */
int oa_qe_legs_cols(oa_plan* p, const void* kX, const void* kY, const void* FG, const void* FH, void* gx, void* gy, void* h,
                    int width, int rband, void* stream);
/* oa_qe_map_legs_cols: oa_fft_r2c + oa_qe_legs_cols for the common case that BOTH legs come from one real map
 * (kappa_from_map("TT", T), lensing.py:973): the forward column pass 2, the leg filters and the inverse column
 * pass 1 run in one kernel -- the map's transform kT never exists in HBM.  Same outputs as
 * oa_qe_legs_cols(plan, kT, kT, ...). */
int oa_qe_map_legs_cols(oa_plan* p, const void* real_map, const void* FG, const void* FH, void* gx, void* gy, void* h,
                        int width, int rband, void* stream);
int oa_qe_cols_div(oa_plan* p, const void* px_rows, const void* py_rows, const void* Fnorm, void* out, int accumulate,
                   int width, int rband, void* stream);

/* ---- one-call entries (SURVEY.md section 8b export list) ---------------------------------------------------
 * A plan that has been told its TT filters and its radial bins runs whole reconstructions per call; work planes are
 * owned by the plan (allocated once by oa_plan_set_filters, never inside a stream-ordered call afterwards).
 *  oa_plan_set_filters : FG, FH, Fnorm = the estimator's real hc-layout planes (gradient-leg weight C^g/(B C^tot),
 *                        inverse-variance weight 1/(B C^tot), -L(L+1)/2 A_L mask_K; device memory owned by the
 *                        caller, which keeps it alive), their active columns / rows (0 = all) and the row grid
 *                        (mrow as in oa_qe_rows).  Replaces the filter set-up of lensing.qest(...).
 *  oa_plan_set_bins    : radial-bin ids of the hc grid (oa_modl_digitize(..., pitch = kpitch, width = nx/2+1)) and
 *                        the power normalisation area / Npix^2; takes the data-independent mode counts once.
 *                        Replaces stats.bin2D.__init__ (stats.py:783-788).
 *  oa_qe_tt            : qest.kappa_from_map("TT", ...) (lensing.py:973-976) in ONE call: pass a real map (both
 *                        legs from it) XOR Fourier-space leg(s) kX [, kY]; kappa_hat's DFT goes to out_kappa_hc or,
 *                        if NULL, to the plan-owned plane oa_plan_kappa(plan).  The pruned kernels write only
 *                        kappa's active region (kappa_cols x row band); zero_outside != 0 zero-fills the rest of a
 *                        caller-supplied plane first (pass 0 only if it is known to be zero there already, e.g. the
 *                        previous call with the same filters wrote it).
 *  oa_qe_pol           : the general separable estimator (TE, EE, EB, TB; lensing.Estimator.reconstruct_hc): the
 *                        npieces (sign, FG, FH, swap-legs) terms are summed in the row stage, one divergence.
 *                        host_* arrays live on the host; the planes they point to on the device.
 *  oa_filter_map       : maps.filter_map (maps.py:1922-1923): real_out = Re IFFT(FFT(real_in) * filter).
 *  oa_qe_tt_moments    : map -> kappa_hat -> binned auto-power -> n += 1, S += b, C += b b^T (Statistics.add of the
 *                        bandpower vector, stats.py:1068-1090): one Monte-Carlo step per call.
 *  oa_mc_run           : the Gaussian N0 / mean-field Monte-Carlo shard [sim_lo, sim_hi) of
 *                        tutorials/tt_verification.ipynb cell 4: Philox GRF (key = (base_seed, sim)) with per-mode
 *                        amplitude covsqrt_hc -> TT estimator -> bandpower moments (+ mean-field stack of kappa_hat,
 *                        interleaved re/im doubles, if meanfield_acc != NULL).  No host synchronisation.
 *  oa_rdn0_set_data,
 *  oa_mc_run_rdn0      : the realisation-dependent N0 shard of ONE data map: the data's three leg planes are cached by the
 *                        set-up entry, then per realisation two draws s, s' -> A = QE(d, s) + QE(s, d), B = QE(s, s') + QE(s', s)
 *                        -> x = [p(A) - p(B) / 2, p(B) / 2] -> moments of the 2 d-vector (at their declarations below).
 *  oa_mc_run_rdn0_windowed : the same with s, s' multiplied by a real-space window (the simulations of an apodised data map).
 *  oa_rdn0_set_data_mv,
 *  oa_mc_run_rdn0_mv   : the same for an estimator SET (TT, TE, EE, EB, TB ...), its cross-spectra and its MV combination on
 *                        power-of-two plans, and on the band grid of 2^a 3^b 5^c plans behind oa_qe_band_bind + oa_mc_mv_band_bind: the
 *                        data triple's distinct leg planes are cached, then per realisation two T, E, B draws -> the 2 nest planes
 *                        A_e, B_e -> one tail over all spectra (at their declarations below).
 *  BINDING: the plan keeps the POINTERS handed to oa_plan_set_filters / oa_plan_set_bins and may keep derived copies of what they
 *  point to (tile-major Fnorm / ids of the fused divergence launch; the (FG, FH) values of the R-split column stage in thread order).  Every call of either entry invalidates those copies -- also
 *  when the addresses are the ones bound before -- so a caller that changes the contents of a bound plane calls the entry again. */
int oa_plan_set_filters(oa_plan* p, const void* FG, const void* FH, const void* Fnorm, int leg_cols, int kappa_cols,
                        int leg_rows, int kappa_rows, int mrow);
/* COLUMN GRID of the one-call TT path (the y-axis counterpart of the ROW GRID above).  Legs confined to the rows
 * |ky index| < leg_rows have real-space products confined to |ky index| <= 2 (leg_rows - 1); evaluated on
 * mcol >= max(2 leg_rows + kappa_rows, 2 kappa_rows) rows (a power of two < ny) no aliased product frequency reaches
 * the kept rows |ky index| < kappa_rows, which therefore equal the full-resolution result (the grid-size factor is
 * folded into the scale).  The input transform is still taken at full resolution (every map pixel is read); the
 * inverse column transforms of the legs, the row stage and the forward column transforms of the products run on
 * mcol instead of ny rows.  Filters, ly axis, kX / kY and the kappa output stay on the full-resolution grid (the
 * kernels address row y + (y >= mcol/2 ? ny - mcol : 0)).  oa_plan_set_filters selects -1 (auto: the smallest such
 * power of two, or none if that is >= ny or the filters have no row band) unless mrow == 0, which selects 0 (the map's
 * own rows, as for the row grid).  oa_plan_set_col_grid overrides: -1 auto, 0 off, > 0 explicit (checked against the
 * bound); oa_plan_col_grid returns the grid resolved for the TT filters (0 = ny).  oa_qe_pol follows the same policy
 * with the row bands of each call (mrow == 0 switches it off there too).
 * FROM-MAP GRID.  The bound does not ask for a power of two.  Where the from-map entries (oa_qe_tt from a real map, oa_qe_tt_moments,
 * oa_qe_tt_moments2, oa_qe_tt_stage) run the R = 4 R-SPLIT path (oa_plan_rsplit) and three quarters of the column grid still satisfy
 * the bound, their coarse side -- the inverse column transforms of the legs, the row stage, the forward column transforms of the
 * products -- runs on 3 mcol / 4 rows: 8192-row maps on 1536 = 3 x 512 rows (the reference's TT band limits need 2 x 380 + 664 = 1424),
 * 4096-row maps on 768.  The row pass and the forward side of the column stage are unchanged (mcol-point transforms of the R planes);
 * only the kept bins are re-indexed.  A plan then carries two grids: `mcol` for every other entry (Fourier-space legs, oa_qe_pol,
 * oa_qe_mv, oa_qe_tt_splits, oa_mc_run*), unchanged bit for bit, and the from-map grid, which is what oa_plan_col_grid, oa_plan_rsplit
 * and oa_plan_div_fused report.  Chosen with mcol = -1; an explicit power of two keeps every entry on that grid; an explicit 3 x 2^k
 * asks for it (the other entries then run on 4/3 of it) and is refused below the bound or where the geometry has no such path. */
int oa_plan_set_col_grid(oa_plan* p, int mcol);
int oa_plan_col_grid(const oa_plan* p);
/* BAND GRID: the one-call TT entries on map sides 2^a 3^b 5^c that are not powers of two (oa_qe_tt from a map or from kX [, kY],
 * oa_qe_tt_moments, oa_qe_tt_moments2, oa_mc_run incl. OA_OPT_MC_BATCH and the mean-field stack).  The estimator is band-limited
 * (legs: columns < leg_cols, rows |ky| < leg_rows; kappa: columns < kappa_cols, rows |ky| < kappa_rows), so on ANY My x Mx grid with
 *     My >= max(2 leg_rows + kappa_rows, 2 kappa_rows),   Mx >= max(2 leg_cols + kappa_cols, 2 kappa_cols)
 * (Mx >= 2 kappa_cols: kappa's columns fit the inner plane's Mx / 2 + 1) and the same ell lattice (a mode of signed index ky at row ky mod My) it returns the same kappa modes, up to the factor
 * (ny nx) / (My Mx) that the plan folds into its copy of Fnorm.  oa_plan_set_filters on such a plan resolves (My, Mx): Mx from
 * mrow, My from the column-grid policy (oa_plan_set_col_grid): -1 = the smallest power of two >= the bound and >= 128; an explicit
 * power of two is checked against the bound; 0 (the map's own grid), unbounded filters (0 = all) and a grid not smaller than the map
 * side are refused with a message naming the reason (the modular chain serves those).  The plan then owns an inner power-of-two plan
 * of My x Mx points with inner-layout copies of FG, FH, Fnorm and of the bin ids (made by oa_plan_set_filters / oa_plan_set_bins,
 * which synchronise the device; oa_plan_set_bins keeps the WHOLE N-plane mode counts, also where the N-grid row pitch nx / 2 + 16
 * is odd, as at nx = 750), and every call runs the fused power-of-two
 * pipeline there: only the input transform (one mixed-radix row R2C that stores the leg columns, then an ny-point DFT evaluated at the
 * leg rows), the Monte-Carlo draw (the leg band of oa_grf_hc's N-grid draw, same Philox counters) and the scatter of kappa's band
 * into the N-grid output / mean-field stack see the map's grid.  oa_qe_tt_splits runs there too, and oa_qe_tt_split_power is the
 * split-based estimator evaluated on the inner grid (both below, at their declarations); oa_mc_run_windowed runs there behind a
 * full-plane N-grid front end (at its declaration); oa_mc_run_mv_windowed runs there behind oa_qe_band_bind + oa_mc_mv_band_bind (at its declaration); oa_qe_tt_stage stays power-of-two only.  oa_plan_band_grid reports (My, Mx), or (0, 0) when no band grid is bound.
 * oa_qe_pol / oa_qe_mv ON A BAND GRID.  The band-limit argument does not depend on the estimator (every separable piece is a product of
 * fields confined to the leg band; the cos / sin 2 phi_ell factors live on the same ell lattice, so a copy of their band is exact), but
 * these two entries take their planes per call, and a stream-ordered call may neither allocate nor synchronise.  oa_qe_band_bind is
 * their set-up entry on such a plan: host_filters = the nfilters DISTINCT leg-filter planes the calls will pass, host_Fnorm = the
 * nnorms normalisation planes in the order the calls will pass them, the band, the row grid `mrow` and the column-grid policy `mcol`
 * (both: -1 auto, a power of two explicit), max_leg_planes = the most leg planes (2 per distinct (source, FG), 1 per distinct
 * (source, FH)) one oa_qe_mv call will need (0: 3 nfilters).  It resolves (My, Mx) by the rule above (same bounds, same refusals), makes
 * or reuses a private inner plan -- the TT binding of oa_plan_set_filters is not touched, the bands may differ --, copies every plane
 * into the inner layout (ONE inner plane per distinct N-grid plane, so oa_qe_mv's sharing of leg transforms by (source, filter) address
 * survives: 17 fields for TT+TE+EE+EB+TB; the normalisation planes stacked in one evenly spaced allocation, scaled by
 * (My Mx) / (ny nx), so the divergence of all estimators stays one launch) and takes the inner plan's pools.  It synchronises the device
 * and may allocate; it copies CONTENTS, so a caller that refills a bound plane in place calls it again.  On a power-of-two plan it
 * returns 0 and does nothing.  oa_qe_pol / oa_qe_mv on a 2^a 3^b 5^c plan then embed the leg band of their distinct source transforms
 * (at most 6: T, E, B and the Y-leg sources of a split call) into inner planes in one launch, run on the inner plan and scatter kappa's
 * band back: `accumulate` adds into the band of `out` only, `zero_outside` zero-fills the complement element by element in the scatter
 * launch.  They refuse -- naming oa_qe_band_bind -- a filter or normalisation pointer that is not bound, band numbers or an mrow that
 * differ from the bound ones, and an oa_qe_mv call that needs more leg planes than max_leg_planes.  oa_qe_band_grid reports the (My, Mx)
 * of this binding, (0, 0) when there is none. */
int oa_plan_band_grid(const oa_plan* p, int* my, int* mx);
int oa_qe_band_bind(oa_plan* p, int nfilters, const void* const* host_filters, int nnorms, const void* const* host_Fnorm, int leg_cols,
                    int kappa_cols, int leg_rows, int kappa_rows, int mrow, int mcol, int max_leg_planes);
int oa_qe_band_grid(const oa_plan* p, int* my, int* mx);
/* R of the R-SPLIT from-map path this plan's one-call TT entries run (0 = not this geometry; 4: 8192^2 / 4096^2 maps at the reference's
 * band limits, 8: 16384^2 float64, 2: 8192^2 with up to 1280 leg columns -- the T filter to ell = 6000): the row R2C carries the first
 * radix-R butterfly of the column transform (R = ny / column grid) and ONE single-pass column kernel goes from its output to
 * the three leg planes -- instead of forward pass 1, [forward pass 2 + filters + inverse pass 1] and inverse pass 2.
 * Same arithmetic up to the order of the column butterflies; results agree with the multi-pass path to rounding. */
int oa_plan_rsplit(const oa_plan* p);
/* 1 when this plan's one-call moment entries (oa_qe_tt_moments, oa_qe_tt_moments2, oa_mc_run) bin |kappa_hat|^2 and update
 * n, S, C in the tail of the single-pass divergence launch (coarse grids of 1024 / 2048 / 4096 rows and from-map grids of 768 / 1536, bins bound) instead of two more
 * launches over the kappa plane; 0: the separate histogram launches.  Same per-mode arithmetic either way; the order of the
 * float64 sums differs (bandpowers agree to ~1e-15).  The divergence workgroups store their bin partials and end; one single-workgroup
 * launch (divbin_fold_kernel) behind it INSIDE THE SAME CALL, on the same stream, adds them in a fixed order and updates n, S, C per map
 * in map order: n, S, C are complete, in stream order, when the call's work is, and calls issued back to back on one stream need no
 * synchronisation between them (the partials buffer is the plan's; the next call's divergence launch is ordered behind this fold).
 * When fused, these entries do not write the plan-owned kappa plane
 * (oa_plan_kappa) unless the mean-field stack of oa_mc_run needs it; oa_qe_tt always does.  oa_plan_set_option(p, OA_OPT_DIV_BIN, 0)
 * switches it off. */
int oa_plan_div_fused(const oa_plan* p);
/* Which of several EQUIVALENT launch sequences the one-call entries of this plan run.  Every value is a supported configuration
 * (the non-default ones are what geometries without the batched kernels run anyway) and the GPU tests compare them against each
 * other; the library never reads the environment for this.
 *   OA_OPT_MC_BATCH    realisations per launch in oa_mc_run: 1 .. 6 (0 = default, 6); moments and stack do not depend on it
 *   OA_OPT_MV_BATCH    oa_qe_mv / oa_qe_tt_splits: all leg planes in one launch and all divergences in one launch (default 1);
 *                      0: one launch per distinct filtered field / per estimator
 *   OA_OPT_MV_ROWBATCH oa_qe_mv: the row stage of several pieces per launch (default 1); 0: one launch per piece
 *   OA_OPT_MV_CHAIN    oa_qe_mv: estimator chains -- an estimator's pieces summed in real space inside one row-stage launch
 *                      (default 1); 0: the k-th piece of every estimator per launch, accumulated in Fourier space
 *   OA_OPT_DIV_BIN     moment entries: radial binning + moment update in the tail of the single-pass divergence launch
 *                      (default 1, where the geometry has that kernel: oa_plan_div_fused); 0: the separate histogram launches
 *   OA_OPT_WIN_FUSED   oa_mc_run_windowed, oa_mc_run_mv_windowed: inverse columns, then C2R x window -> R2C of every row in ONE kernel (default 1: the
 *                      real map exists in LDS only); 0: C2R with the window at its store, real map in HBM, from-map estimator path
 *                      (sides 2^a 3^b 5^c: the band input transform; until the option is set, or after a value < 0, such a plan takes
 *                      what measured faster: the unfused flow for rows of up to 1200 points, the fused pass for longer ones up to
 *                      the 8192 points its kernel holds)
 *   OA_OPT_DRAW_FUSED  oa_mc_run_rdn0_windowed on power-of-two plans (with OA_OPT_WIN_FUSED = 1): 1 = the draws of up to three
 *                      realisations are evaluated inside ONE inverse column pass-1 launch (oa_grf_hc_icols: the drawn planes never
 *                      exist); 0 = ONE BY ONE: per draw oa_grf_hc, the column transform and the row pass (24 launches per six draws
 *                      against 3); unset or < 0 = what measured faster: 1.  The kernel alone saves 5 - 14 us per drawn plane at 2048^2
 *                      and 4096^2, beyond the spreads; a realisation is 9 - 25 % faster, most of that from the batched launches
 *                      (profiles/rdn0_windowed.jsonl).  The moments are bit-equal between 0 and 1.
 *                      oa_mc_run_rdn0_mv_windowed on power-of-two plans (with OA_OPT_WIN_FUSED = 1): 1 = both triples of a realisation are
 *                      drawn inside ONE inverse column pass-1 launch (oa_grf_mix_icols) and the six planes share every later launch;
 *                      0 = oa_mc_run_mv_windowed's source stage per triple; unset or < 0 = that entry's own default: 0 until the fused kernel
 *                      has been timed against the per-triple draw.
 *                      The moments are bit-equal between 0 and 1. */
enum { OA_OPT_MC_BATCH = 1, OA_OPT_MV_BATCH = 2, OA_OPT_MV_ROWBATCH = 3, OA_OPT_MV_CHAIN = 4, OA_OPT_DIV_BIN = 5, OA_OPT_WIN_FUSED = 6, OA_OPT_DRAW_FUSED = 7 };
int oa_plan_set_option(oa_plan* p, int option, int value);
int oa_plan_set_bins(oa_plan* p, const int32_t* ids_hc, int nids, double norm, void* stream);
void* oa_plan_kappa(oa_plan* p);
const int64_t* oa_plan_bin_counts(oa_plan* p);
int oa_qe_tt(oa_plan* p, const void* real_map, const void* kX, const void* kY, void* out_kappa_hc, int zero_outside,
             void* stream);
int oa_qe_pol(oa_plan* p, int npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH,
              const int* host_swap, const void* kX, const void* kY, const void* Fnorm, void* out, int accumulate,
              int leg_cols, int kappa_cols, int leg_rows, int kappa_rows, int mrow, int zero_outside, void* stream);
/* oa_qe_pol for several estimators accumulated into ONE kappa plane (the minimum-variance combination: Fnorm[e] carries
 * weight x normalisation of estimator e), pieces flattened in estimator order (host_npieces[e] each; host_kX/kY/Fnorm per
 * estimator).  Every distinct filtered field -- identified by its (source plane, filter plane) POINTERS -- is transformed
 * once, all in one inverse pass-2 launch: 17 leg planes instead of 30 for TT+TE+EE+EB+TB when the caller shares its filter
 * plane objects.  Same arithmetic per piece as oa_qe_pol, same results.  When the Fnorm planes are evenly spaced in memory
 * (one stacked allocation) the divergence of all estimators is one launch, each into a plan-owned plane, and one pass sums
 * them in estimator order.  oa_qe_mv and oa_qe_tt_splits keep their leg / product planes in a plan-owned pool that is
 * allocated on first use and grown on demand: THAT call synchronises the device once; later calls are stream-ordered. */
int oa_qe_mv(oa_plan* p, int nest, const int* host_npieces, const double* host_signs, const void* const* host_FG,
             const void* const* host_FH, const int* host_swap, const void* const* host_kX, const void* const* host_kY,
             const void* const* host_Fnorm, void* out, int accumulate, int leg_cols, int kappa_cols, int leg_rows, int kappa_rows,
             int mrow, int zero_outside, void* stream);
/* oa_qe_mv FROM REAL MAPS on a 2^a 3^b 5^c plan (band grid, oa_qe_band_bind): host_maps = nmaps device real planes (1 <= nmaps <= 6, each
 * ny x nx of the plan's dtype); source i is the unnormalised transform of map i (what oa_fft_r2c returns with scale = 1) and
 * host_xsrc[e] / host_ysrc[e] name the sources of estimator e's X and Y leg by index.  rot_c / rot_s: both NULL, or both (ny, kpitch) real
 * planes in the half layout holding cos / sin 2 phi_ell; then nmaps is 3 or 6 and the sources (1, 2) and (4, 5) are replaced per mode by
 * oa_rot2's combination E = Q c - U s, B = Q s + U c.  Only the leg band of the rotation planes is read, straight from the caller's planes
 * (rows |ky| < leg_rows, columns < leg_cols): nothing is copied or bound for them.  Every other argument is oa_qe_mv's; nest = 1 is one
 * estimator.  The filter and normalisation planes are looked up in the oa_qe_band_bind binding exactly as oa_qe_mv does (same checks, same
 * messages naming the set-up entry, same leg-plane budget).  Only the source stage differs: a batched band input transform -- one
 * mixed-radix row R2C per map row that stores the leg columns, a pruned-output column DFT of all maps at the leg rows (double accumulation
 * in both precisions, fixed summation order: deterministic), the rotation in double before the single rounding -- writes the leg band of
 * all sources straight into the binding's inner source planes in three launches.  No N-grid transform plane exists, nothing is embedded,
 * and no pointer table is uploaded: the map pointers travel in the kernel arguments.  The map-side scratch (per map: ny x leg_cols complex
 * + the column pass's partial sums) belongs to the binding, like the inner planes of oa_qe_tt_splits on a band grid: it is taken on the
 * first from-maps call and regrown when a call brings more maps or a wider band than any before -- that call synchronises the device once;
 * later calls neither allocate nor synchronise --, oa_plan_release_pools frees it, and oa_qe_band_bind drops it when it remakes the inner
 * plan.  Refused before anything is launched: a power-of-two plan (oa_fft_r2c, oa_rot2 and oa_qe_mv are the same steps there), a chirp-z
 * plan, no binding or other band numbers / mrow than the bound ones, an unbound filter or normalisation plane, too many leg planes, nmaps
 * outside 1..6, a NULL map, only one of rot_c / rot_s, rotation planes with nmaps not 3 or 6, a source index outside [0, nmaps). */
int oa_qe_mv_maps(oa_plan* p, int nmaps, const void* const* host_maps, const void* rot_c, const void* rot_s, int nest,
                  const int* host_npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH,
                  const int* host_swap, const int* host_xsrc, const int* host_ysrc, const void* const* host_Fnorm, void* out,
                  int accumulate, int leg_cols, int kappa_cols, int leg_rows, int kappa_rows, int mrow, int zero_outside, void* stream);
int oa_filter_map(oa_plan* p, const void* real_in, const void* filt_hcreal, void* real_out, void* stream);
int oa_qe_tt_moments(oa_plan* p, const void* real_map, int64_t* n, double* S, double* C, void* stream);
/* Two Monte-Carlo steps per call (two independent maps): identical results to two oa_qe_tt_moments calls; on the
 * column-grid path every launch behind the two row transforms is shared by both maps. */
int oa_qe_tt_moments2(oa_plan* p, const void* real_map0, const void* real_map1, int64_t* n, double* S, double* C, void* stream);
/* SplitLensing.cross_estimator (lensing.py:980-1003) needs the TT reconstruction of every ordered pair of
 * splits (X / gradient leg from split i, Y leg from split j).  One call: the three filtered leg planes of each split are
 * transformed ONCE (nsplits leg stages instead of nsplits^2), then the row stage + divergence run per pair.
 * host_kmaps: nsplits device hc planes (the splits' transforms); host_out: nsplits^2 device hc planes, [i*nsplits + j];
 * zero_outside as in oa_qe_tt.  Needs oa_plan_set_filters.
 * oa_split_cross_power: the estimator's combination of those planes per mode, in f64 (the QE is bilinear, so the
 * reference's reconstructions involving the split mean are means of the pairwise ones):
 *   out = (n^4 P(kc) - 4 n^2 sum_i P(kic) + 4 sum_{i<j} P(kij)) / (n (n-1)(n-2)(n-3)),  P(x) = |x|^2 norm,
 * written over columns < active_cols and the band rows of the real half-plane `out_hcreal` only (4 <= nsplits <= 8).
 * ON A BAND GRID (sides 2^a 3^b 5^c, TT filters bound) oa_qe_tt_splits embeds the leg band of the nsplits transforms into inner planes in
 * one launch (device table of sources, re-uploaded only when the pointers change), runs itself on the inner plan into a plan-owned,
 * evenly spaced (n, n, My, kp_inner) block -- its divergence stays one batched launch -- and scatters kappa's band of all nsplits^2 planes
 * to host_out in ONE launch (plane on grid z; zero_outside: the complement of every plane is zero-filled in that launch, else nothing is
 * written outside the band).  The inner source planes and the block belong to the plan: the first call, and a call with more splits
 * than any before, allocates and synchronises the device once; later calls do neither; oa_plan_release_pools frees them.
 * oa_qe_tt_split_power is the whole estimate in one call on such a plan: the same embed and inner call, then ONE launch that combines
 * the nsplits^2 INNER planes per mode (the arithmetic of oa_split_cross_power, f64) and stores the real result to the N-grid half-plane
 * out_hcreal (kappa's band; zero_outside: zero elsewhere, same launch) -- the K_ij never exist on the map's grid.  norm = area / Npix^2
 * of the map (FourierCalc.normfact); 4 <= nsplits <= 8 (checked before anything is launched).  A power-of-two plan has no inner grid and
 * refuses, naming oa_qe_tt_splits + oa_split_cross_power, which are the same two steps there. */
int oa_qe_tt_splits(oa_plan* p, int nsplits, const void* const* host_kmaps, void* const* host_out, int zero_outside, void* stream);
int oa_qe_tt_split_power(oa_plan* p, int nsplits, const void* const* host_kmaps, void* out_hcreal, double norm, int zero_outside,
                         void* stream);
int oa_split_cross_power(int dtype, int nsplits, const void* const* host_kappa, void* out_hcreal, double norm, int ny, long kpitch,
                         int active_cols, int active_rows, void* stream);
/* oa_mc_run: realisations sim_lo .. sim_hi-1 (Philox stream = realisation index): GRF draw -> TT estimator -> bandpowers ->
 * moments [-> mean-field stack], no host work per realisation.  Up to 6 realisations (oa_plan_set_option OA_OPT_MC_BATCH,
 * 1 = one by one) share every launch (grid z / y: draw, leg planes, inverse pass 2, row stage, divergence, binned power, moment tail, stack): at
 * 4096^2 a realisation is launch latency, not bytes.  Same kernels on the same operands in the same order per realisation:
 * the moments and the stack do not depend on the batch size.  The first call allocates the batch's planes (one device
 * synchronisation). */
int oa_mc_run(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, int64_t* n, double* S,
              double* C, double* meanfield_acc, void* stream);
/* REALISATION-DEPENDENT N0 (RDN0) of the TT estimator: the Monte Carlo that debiases the kappa_hat auto-spectrum of ONE given map d by
 * pairing it with simulations through the two legs of the estimator.  With QE(X, Y) = oa_qe_tt(kX = X, kY = Y) of the bound filters and,
 * for realisation i, s = the draw of Philox stream 2 i and s' = the draw of stream 2 i + 1 (key base_seed, amplitude covsqrt_hc: the very
 * draws oa_mc_run makes for its realisations 2 i and 2 i + 1 -- the leg band of oa_grf_hc's plane, same counters):
 *     A = QE(d, s) + QE(s, d),      B = QE(s, s') + QE(s', s),
 *     p(Z)_b = binned |Z|^2 * norm over the mode counts of bin b (weights, ids and counts of oa_plan_set_bins, as oa_mc_run's bandpowers),
 *     x_i = [ p(A) - p(B) / 2 ,  p(B) / 2 ]          (2 d numbers, d = nids - 2: "rdn0", then "mcn0"),
 *     n += 1,  S += x_i,  C += x_i x_i^T             (Statistics.add of the 2 d-vector, float64, realisation order).
 * |A|^2 is the four data-simulation terms of the usual six-term RDN0; p(B) / 2 has the expectation of its two simulation-simulation
 * terms and a smaller variance.  The second half alone is the N0 of independent pairs (no data, no signal trispectrum); the debiased
 * spectrum of the map is p(QE(d, d)) - mean(rdn0).  No window here: oa_mc_run_rdn0_windowed (below) is the entry for an apodised map.
 *  oa_rdn0_set_data : set-up entry (needs oa_plan_set_filters; may allocate and synchronise).  kD_hc = the data map's transform; its three
 *                     filtered leg planes are made on the plan's coarse grid, exactly as the leg stage of oa_qe_tt(kX = d) leaves them,
 *                     and kept in a plan-owned buffer (on a band grid: the leg band of kD_hc is embedded into an inner plane first and
 *                     the legs live on the inner plan).  Every later oa_plan_set_filters / oa_plan_set_bins / oa_plan_set_col_grid
 *                     makes them stale (the binding generation is their key): call it after those.  oa_plan_release_pools frees them.
 *  oa_mc_run_rdn0   : the shard [sim_lo, sim_hi); S holds 2 d doubles, C (2 d)^2.  Stream-ordered, no host work on data; it allocates
 *                     nothing after the first call (nothing at all when oa_rdn0_set_data ran with the bins bound).  Refused by name
 *                     before anything is launched: chirp-z sides, no filters, no bins, a binding without a band grid, no data set,
 *                     stale data legs, more bins than the tail's fold workgroup holds.  Realisations are batched as in oa_mc_run
 *                     (OA_OPT_MC_BATCH; a batch of B realisations holds 2 B draws); per batch: 1 draw launch, 2 leg launches (the
 *                     data's legs are cached: only the simulations' 6 B fields are transformed) [+ 1 inverse pass 2], 1 chain row-stage
 *                     launch (A_b, B_b: 2 B estimators of two pieces each, summed in real space), 1 divergence launch, and the 2
 *                     launches of the combine -> bin -> moments tail (partial sums per group of band rows, then one fold workgroup:
 *                     no ticket).  Where the row stage takes one map per launch the realisations run one by one.  Every sum has a
 *                     fixed order: the moments are bit-reproducible and do not depend on the batch size nor on how a range is cut
 *                     into calls. */
int oa_rdn0_set_data(oa_plan* p, const void* kD_hc, void* stream);
int oa_mc_run_rdn0(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, int64_t* n, double* S, double* C,
                   void* stream);
/* oa_mc_run_rdn0_windowed: oa_mc_run_rdn0's definition with ONE change -- s and s' are the WINDOWED draws
 *     s = R2C(window_real . C2R(oa_grf_hc(base_seed, 2 i)) / Npix),      s' = the same from stream 2 i + 1,
 * the full-plane draws oa_mc_run_windowed makes for its realisations 2 i and 2 i + 1 (window_real: ny x nx reals of the plan's dtype).
 * The data legs are those cached by the unchanged oa_rdn0_set_data: its kD_hc is the transform of the map AS ANALYSED, i.e. already
 * apodised by the caller.  A, B, x_i, the tail, its fixed summation order and its bit-reproducibility are oa_mc_run_rdn0's.  There is NO
 * mean-field argument: s, s' and d are independent and zero-mean, so A and B carry no mean field (the mean field of the data's own
 * reconstruction QE(d, d) is the caller's to subtract; mc.RDN0MonteCarlo.data_bandpowers(mean_field=...)).
 * Power-of-two plans, per batch of B realisations: the full-plane part of its 2 B draws in groups of up to six -- OA_OPT_DRAW_FUSED = 1:
 * one pass-1 launch with the draw at its load + pass 2 (oa_grf_hc_icols), one fused row launch C2R x window -> R2C; 0: oa_grf_hc,
 * inverse columns and the row pass per draw -- onto compact row planes, then the forward column transform onto the leg band of the
 * entry's draw planes (six planes per launch), then oa_mc_run_rdn0's launches.  OA_OPT_WIN_FUSED = 0: one by one, per draw oa_grf_hc ->
 * oa_fft_c2r_windowed -> oa_fft_r2c.  Band grid (sides 2^a 3^b 5^c): oa_mc_run_windowed's front end there, the 2 B draws through its six
 * N-grid planes in two halves, the pruned column DFT onto the inner plan's draw planes; the fused / unfused rule by row length is that entry's.
 * Refused by name before anything is launched: a NULL window and everything oa_mc_run_rdn0 refuses.  Nothing is allocated after the
 * first call; oa_plan_release_pools frees what the entry took.
 * A batch is started only where the chain row stage serves the geometry; elsewhere the realisations run one at a time from the start.
 * Measured per realisation against the host loop of existing entries (profiles/rdn0_windowed.jsonl): 0.11 against 0.40 ms at 2048^2 f32,
 * 0.52 against 1.28 ms at 4096^2 f64; band grid (one at a time) 0.31 against 0.40 ms at 1200^2 f32, 0.51 against 0.69 ms at 2400^2 f32. */
/* Which path the LAST oa_mc_run_rdn0 / oa_mc_run_rdn0_windowed call on this plan took: 1 when it ran realisations in batches (a batch
 * reached the tail), 0 when it ran them one at a time (the row stage takes one map per launch, or OA_OPT_WIN_FUSED = 0 / the unfused
 * rule of a band grid), was refused, or was never made. */
int oa_plan_rdn0_batched(const oa_plan* p);
int oa_mc_run_rdn0_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, const void* window_real, int64_t* n,
                            double* S, double* C, void* stream);
/* The same shard with a real-space window applied to every realisation before its transform (the reference's analysis
 * flow: maps.py:1873-1878 get_taper, maps.py:1350-1361): full-plane draw (same Philox counters as oa_mc_run) -> C2R / Npix
 * -> x window_real (ny x nx reals of the plan's dtype) -> TT estimator -> bandpower moments (+ mean-field stack).  With
 * window == 1 the moments equal oa_mc_run's up to rounding; with a taper the stack holds the window's mean field.
 * ON A BAND GRID (sides 2^a 3^b 5^c with filters that bound one; chirp-z sides and a binding without a band grid are refused by name):
 * per realisation the full-plane draw on the N grid and its mixed-radix inverse column transform in place; per batch of up to 6 ONE
 * fused row launch (C2R -> x window / Npix -> R2C per row, the real map in LDS only, the leg columns stored) and the pruned column
 * DFT onto the inner plan's source planes, then oa_mc_run's batched launches there and the N-grid stack update.  OA_OPT_WIN_FUSED = 0:
 * one by one, oa_fft_c2r_windowed -> real map in HBM -> the band input transform.  The first windowed call on such a plan takes the
 * draw and row planes (one device synchronisation); oa_plan_release_pools frees them. */
int oa_mc_run_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* covsqrt_hc, const void* window_real,
                       int64_t* n, double* S, double* C, double* meanfield_acc, void* stream);
/* oa_mc_run_mv: the Gaussian N0 Monte-Carlo shard [sim_lo, sim_hi) of an estimator SET (TT, TE, EE, EB, TB ... and their MV combination),
 * on power-of-two plans and, behind two set-up calls, on the band grid of 2^a 3^b 5^c plans (below).  The estimator arguments are oa_qe_mv's (nest <= 6, pieces flattened in estimator order) except that the sources
 * are named by index -- host_xsrc[e] / host_ysrc[e]: 0 T, 1 E, 2 B, oa_qe_mv_maps' convention -- and that host_Fnorm holds the PURE
 * normalisations (no MV weight).  host_covsqrt: oa_grf_mix's nine hc-real blocks for the fields T, E, B (NULL = zero block), amplitude
 * scaling included.  Per realisation i, stream-ordered, nothing leaving the device and no host work on the data:
 *   1. oa_grf_mix_band(seed = base_seed, stream_id0 = 3 i, ncomp = 3, width = leg_cols, rband = leg_rows) into three hc planes owned by
 *      the entry (the plan's work planes are where step 2 puts the per-estimator kappa_hat);
 *   2. oa_qe_mv's launch sequence without its final sum: estimator e's normalised kappa_hat ends in plane e of an evenly spaced block --
 *      the plan-owned planes of the one-launch divergence when that is engaged (2 <= nest, evenly spaced host_Fnorm, OA_OPT_MV_BATCH = 1),
 *      else the estimators run one at a time into a block the entry owns;
 *   3. oa_bin_power_multi over the block: fields 0 .. nest-1 are the estimators, field nest (only with mv_weights: nest hc-real planes
 *      mv_wstride elements apart) is the MV combination sum_e w_e kappa_hat_e, formed in registers; spectrum s = (host_a[s], host_b[s]),
 *      kappa's band (kappa_cols, kappa_rows) as the active region, ids_hc / nids / norm as for oa_bin_power;
 *   4. one launch: x[s * d + j] = sums[s][j + 1] / counts[j + 1], d = nids - 2 (counts: device int64[nids], the data-independent mode
 *      counts of a full-plane oa_bin_power call), then n += 1, S += x, C += x x^T with D = nspec * d  (S: D doubles, C: D x D).
 * Realisation i's contribution does not depend on how a range is cut into calls.  On a power-of-two plan the first call (and a call that
 * needs more than any before) allocates the entry's planes and synchronises the device once; oa_plan_release_pools frees them.
 * ON A BAND GRID (2^a 3^b 5^c plans).  The filter and normalisation planes are bound by oa_qe_band_bind (the pure normalisations, in the
 * order of host_Fnorm); then oa_mc_mv_band_bind(plan, mv_weights, mv_wstride, nest, ids_hc, nids, nspec_max) -- a set-up call like that
 * one: it may allocate and synchronises the device -- copies kappa's band of the nest weight planes (nothing when mv_weights is NULL)
 * and of the N-grid bin ids into the inner layout (-1 outside the band), takes everything a shard would otherwise allocate on first use
 * (the three inner draw planes, zero-filled once; nest inner kappa planes; oa_bin_power_multi's scratch and sums for
 * nspec_max x nids) and remembers the caller's pointers, the stride, nest and nids.  A later oa_qe_band_bind drops it; on a
 * power-of-two plan it returns 0 and does nothing.  A shard then neither allocates nor synchronises: step 1 is
 * oa_grf_mix_band_inner -- the same draw, written into the inner layout --, steps 2 and 3 run on the inner plan with the inner copies
 * (kappa_hat per mode is the same on both grids; the inner Nyquist column lies outside kappa's band, so column 0 is the only visited
 * one of multiplicity 1, as on the N grid), step 4 divides by the caller's counts, those of the whole N plane.
 * Refused before anything is launched, n, S, C untouched: a chirp-z plan; a 2^a 3^b 5^c plan without an oa_qe_band_bind binding or
 * without an oa_mc_mv_band_bind binding on it, or whose bands, mrow, weights pointer and stride, ids pointer, nids or nest differ from
 * the bound ones, or with nspec > nspec_max (these messages name both set-up entries and the host loop of the existing entries that
 * mc.GaussianN0MonteCarloPol runs with one_call=False); a filter or normalisation plane that is not bound; more leg planes than
 * oa_qe_band_bind's max_leg_planes; nest outside 1..6, a source index outside [0, 3), and every refusal of oa_bin_power_multi (with
 * nfields = nest). */
int oa_mc_mv_band_bind(oa_plan* p, const void* mv_weights, long mv_wstride, int nest, const int32_t* ids_hc, int nids, int nspec_max);
int oa_mc_run_mv(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest, const int* host_npieces,
                 const double* host_signs, const void* const* host_FG, const void* const* host_FH, const int* host_swap, const int* host_xsrc,
                 const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights, long mv_wstride, int nspec, const int* host_a,
                 const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts, double norm, int leg_cols, int kappa_cols,
                 int leg_rows, int kappa_rows, int mrow, int64_t* n, double* S, double* C, void* stream);
/* REALISATION-DEPENDENT N0 of an estimator SET and its MV combination (power-of-two plans; 2^a 3^b 5^c plans on a band grid, below): the RDN0 above for the estimators, crosses and MV
 * field of oa_mc_run_mv.  The estimator set is oa_mc_run_mv's (nest <= 6, pieces flattened in estimator order: sign, FG, FH, swap; sources by
 * index 0 T, 1 E, 2 B; pure normalisations host_Fnorm; optional MV weights) and so are the spectrum list (field nest = MV), the bins, the
 * counts and the bands.  For field triples X = (X_T, X_E, X_B) and Y, QE_e(X; Y) is estimator e with kX = X[xsrc_e], kY = Y[ysrc_e].  With
 * d the data triple and, for realisation i, s = the T, E, B draw of oa_grf_mix_band(seed = base_seed, stream_id0 = 6 i) and s' the draw of
 * stream_id0 = 6 i + 3 (oa_mc_run_mv's draws of its realisations 2 i and 2 i + 1):
 *     A_e = QE_e(d; s) + QE_e(s; d),    B_e = QE_e(s; s') + QE_e(s'; s),    A_MV = sum_e w_e A_e,    B_MV = sum_e w_e B_e,
 *     p(Z_a, Z_b)_j = sum over the modes of bin j + 1 of m Re(Z_a conj Z_b) norm / counts[j + 1]   (m = Hermitian multiplicity),
 *     x_i = [ p(A_a, A_b) - p(B_a, B_b) / 2 for every spectrum (a, b) in list order ] ("rdn0") ++ [ p(B_a, B_b) / 2 likewise ] ("mcn0"),
 *     n += 1,  S += x_i,  C += x_i x_i^T          (D = 2 nspec d, d = nids - 2; S: D doubles, C: D x D).
 * The debiased spectrum of the data is p(QE_a(d; d), QE_b(d; d)) - mean(rdn0_ab).  No window here: oa_mc_run_rdn0_mv_windowed (below) is
 * the entry for an apodised triple.
 *  oa_rdn0_set_data_mv : set-up entry (may allocate and synchronise).  host_kD: the three hc transforms of the data (a plane no estimator
 *                        reads may be NULL).  The data's DISTINCT leg planes -- one gradient pair per distinct (source, FG), one H plane
 *                        per distinct (source, FH): oa_qe_mv's sharing rule -- are transformed once (one batched leg launch where that
 *                        applies) on the column grid of the bands and kept in a plan-owned buffer; oa_plan_release_pools frees it.
 *  oa_mc_run_rdn0_mv   : the shard [sim_lo, sim_hi), one realisation at a time.  Stream-ordered, no host work on data, no allocation after
 *                        the first call (oa_plan_release_pools frees everything both entries took).  Per realisation: 2 band draws into entry-owned planes; the leg planes of s and of s' (one batched
 *                        leg launch per triple [+ 1 inverse pass 2 over both]); the row stage of the 2 nest chains A_e, B_e (2 npieces_e
 *                        pieces each over the leg planes of d, s, s': ONE chain launch where the row-stage table holds them, else two;
 *                        where the chain kernel does not serve the geometry, or with OA_OPT_MV_CHAIN = 0, one launch per piece, the second
 *                        and later pieces accumulating); the divergence of the nest A planes and of the nest B planes (one batched launch
 *                        each where oa_qe_mv's one-launch divergence is engaged, else one per plane) into the entry's 2 nest kappa planes;
 *                        and the 3 launches of the tail (partial sums per fixed group of band rows with A_MV, B_MV formed in registers, the
 *                        fold to x_i, the moment update).  Every sum has an order fixed by the band, the bins and the spectrum list: the
 *                        moments are the same bit for bit on every run and however a range is cut into calls.
 * ON A BAND GRID (2^a 3^b 5^c plans).  Three set-up calls come first, in this order: oa_qe_band_bind with the set's distinct filter planes,
 * its pure normalisations (in the order of host_Fnorm), the call's bands, mrow and column grid; oa_mc_mv_band_bind with the weights, the bin
 * ids, nids and nspec_max >= nspec; then oa_rdn0_set_data_mv.  On such a plan oa_rdn0_set_data_mv looks the call's filter planes up in the
 * oa_qe_band_bind binding, embeds the leg band of the data transforms into inner source planes, makes the data's distinct leg planes on the
 * INNER plan with the inner filter copies and keeps them there; it also takes every plane a shard would otherwise allocate (the inner plan's
 * leg pool for s, s' and the 2 nest chains, the six inner draw planes, the 2 nest inner kappa planes, the tail's scratch for the Monte-Carlo
 * binding's nspec_max x nids, the device tables).  A shard then neither allocates nor synchronises.  Per realisation: ONE launch draws T, E, B
 * of s and of s' into the inner layout (oa_grf_mix_band_inner_triples, ntriples = 2: the N grid's Philox counters, edge rules and covsqrt
 * planes), then the launches above run on the inner plan with the inner copies of the filters, normalisations (they carry My Mx / (ny nx):
 * kappa_hat per mode is the same on both grids), weights and bin ids, the binding's row grid and the inner column grid; the tail divides by
 * the caller's counts, those of the whole N plane.  Since Mx >= 2 kappa_cols the inner Nyquist column is never visited: column 0 is the only
 * visited one of Hermitian multiplicity 1, as on the N grid.  The moments are bit-reproducible and do not depend on how a range is cut into
 * calls.  The data legs belong to the oa_qe_band_bind binding they were made on: EVERY later oa_qe_band_bind call (it rewrites the inner
 * filter copies and may remake the inner plan) makes them stale, also one with the same planes.
 * Refused there by name before anything is launched, n, S, C untouched, every message naming mc.RDN0MonteCarloPol and one_call=False: no
 * oa_qe_band_bind binding (both entries: "bound first (oa_qe_band_bind, then oa_mc_mv_band_bind)"); bands or mrow other than the bound ones
 * (both entries); a filter plane that is not bound (both entries), a normalisation plane that is not bound; no oa_mc_mv_band_bind binding on
 * the current oa_qe_band_bind binding, or weights, stride, ids, nids or nest other than its, or nspec > its nspec_max; no data set; stale
 * data legs (an oa_qe_band_bind call since oa_rdn0_set_data_mv, another filter-plane list, other bands, mrow or inner column grid).
 * oa_mc_run_rdn0_mv_windowed is NOT on the band grid.
 * Refused by name before anything is launched, n, S, C untouched: a chirp-z plan (the message names mc.RDN0MonteCarloPol and
 * one_call=False); no data set; stale data legs (another filter-plane list, other bands or mrow, a column grid changed by
 * oa_plan_set_col_grid since oa_rdn0_set_data_mv); nest outside 1..6; a source index outside [0, 3); NULL planes; a (nspec, nids) beyond the
 * tail's tables: it holds nspec <= 28, 3 <= nids <= 1024, nspec nids <= 4096 -- every (nspec, nids >= 3) oa_bin_power_multi accepts. */
int oa_rdn0_set_data_mv(oa_plan* p, const void* const* host_kD, int nest, const int* host_npieces, const void* const* host_FG,
                        const void* const* host_FH, const int* host_swap, const int* host_xsrc, const int* host_ysrc, int leg_cols, int kappa_cols,
                        int leg_rows, int kappa_rows, int mrow, void* stream);
int oa_mc_run_rdn0_mv(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest, const int* host_npieces,
                      const double* host_signs, const void* const* host_FG, const void* const* host_FH, const int* host_swap, const int* host_xsrc,
                      const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights, long mv_wstride, int nspec, const int* host_a,
                      const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts, double norm, int leg_cols, int kappa_cols,
                      int leg_rows, int kappa_rows, int mrow, int64_t* n, double* S, double* C, void* stream);
/* oa_mc_run_rdn0_mv_windowed: oa_mc_run_rdn0_mv's definition with ONE change -- s and s' are the WINDOWED triples: for z = 0, 1 the T, E, B
 * that oa_mc_run_mv_windowed's source stage makes from the full-plane draw of streams 6 i + 3 z .. 6 i + 3 z + 2 (the very draws that entry
 * makes for its realisations 2 i + z): T, E, B rotated to T, Q, U in the draw, C2R / Npix, x window_real, R2C, Q, U -> E, B on the leg
 * band.  The arguments are oa_mc_run_rdn0_mv's plus window_real, rot_c, rot_s, which mean what they mean in oa_mc_run_mv_windowed: the
 * window multiplies T, Q, U, not E, B, and rot_c / rot_s are the Q, U -> E, B planes.  The data legs are those of the unchanged
 * oa_rdn0_set_data_mv: the data is the triple AS ANALYSED, already apodised by the caller.  A, B, the spectrum list, the tail, its fixed
 * summation order and its bit-reproducibility are oa_mc_run_rdn0_mv's.  There is NO mean-field argument: s, s' and d are independent and
 * zero-mean, so A and B carry no mean field (that of the data's own reconstructions is the caller's to subtract:
 * mc.RDN0MonteCarloPol.data_bandpowers(mean_field=...)).
 * Source stage per realisation (power-of-two plans), onto the leg band of the entry's six draw planes:
 *   OA_OPT_WIN_FUSED = 1, OA_OPT_DRAW_FUSED = 1: FIVE launches for the six planes -- one inverse column pass-1 launch with both triples'
 *     draws at its load (oa_grf_mix_icols, ntriples = 2: each Philox counter evaluated once per triple), one in-place pass 2, one fused
 *     row launch over six planes (C2R / Npix -> x window -> R2C, the real maps in LDS only, compact row planes), one forward column launch
 *     over six -- and the Q, U -> E, B rotation on the band, one launch per pair;
 *   OA_OPT_DRAW_FUSED = 0: oa_mc_run_mv_windowed's fused sequence per triple (the T, Q, U draw into full planes, its batched inverse
 *     columns + fused row launch, its forward column launch, the rotation);
 *   OA_OPT_WIN_FUSED = 0: that entry's unfused flow per triple (oa_fft_c2r_windowed -> real map in HBM -> oa_fft_r2c on the band).
 * The stage's planes (six full hc planes + six compact row planes) are entry-owned, shared with oa_mc_run_mv_windowed: nothing is allocated
 * after the first call and oa_plan_release_pools frees them.
 * Refused by name before anything is launched, n, S, C untouched: a NULL window (the message names oa_mc_run_rdn0_mv, the entry without
 * one), a window without both rotation planes, and everything oa_mc_run_rdn0_mv refuses (a plan that is not power-of-two, no data, stale
 * legs, nest, sources, tail tables); the messages name this entry, mc.RDN0MonteCarloPol and one_call=False. */
int oa_mc_run_rdn0_mv_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest,
                               const int* host_npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH,
                               const int* host_swap, const int* host_xsrc, const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights,
                               long mv_wstride, int nspec, const int* host_a, const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts,
                               double norm, int leg_cols, int kappa_cols, int leg_rows, int kappa_rows, int mrow, const void* window_real,
                               const void* rot_c, const void* rot_s, int64_t* n, double* S, double* C, void* stream);
/* oa_mc_run_mv_windowed: oa_mc_run_mv with a real-space window on the T, Q, U maps of every realisation and with the mean-field stacks of the
 * estimator set.  The arguments are oa_mc_run_mv's, plus
 *   window_real     ny x nx reals of the plan's dtype (the apodisation every map is multiplied by before its transform), or NULL;
 *   rot_c, rot_s    (ny, kpitch) hc-real planes cos / sin 2 phi_l, as oa_qe_mv_maps takes them (needed with a window);
 *   host_meanfield  NULL, or a host array of nest (+ 1 when mv_weights is given) device float64 planes (ny, kpitch, 2): the sums of the
 *                   per-estimator kappa_hat in estimator order, then of the MV combination sum_e w_e kappa_hat_e.
 * POWER-OF-TWO PLANS, AND 2^a 3^b 5^c PLANS ON THEIR BAND GRID (below).  A chirp-z plan is refused before anything is launched (n, S, C and
 * the stacks untouched), naming this entry and the host loop mc.GaussianN0MonteCarloPol runs with one_call=False.
 * The window multiplies Q and U, not E and B: a taper leaks E into B.  Per realisation i, stream-ordered, nothing leaving the device:
 * without a window, step 1 is oa_mc_run_mv's band draw (the moments are then oa_mc_run_mv's bit for bit); with one it is
 *   a. the full-plane oa_grf_mix draw of T, E, B (streams 3 i .. 3 i + 2: the counters of the band draw, so window == 1 reproduces the
 *      unwindowed run to rounding) rotated to T, Q, U in the same pass by the inverse of oa_rot2's combination, Q = E c + B s,
 *      U = -E s + B c, into three hc planes the entry owns;
 *   b. one batched inverse column launch over the three planes, then ONE fused row launch over them (C2R / Npix -> x window -> R2C per row,
 *      the real rows in LDS only, the window shared by the planes): leg_cols columns stored at the compact pitch;
 *   c. one batched forward column launch onto the leg band of the three source planes of oa_mc_run_mv's loop;
 *   d. Q, U -> E, B (oa_rot2's combination) on the leg band only -- rows |ky| < leg_rows, columns < leg_cols --, c and s read from the
 *      caller's planes, arithmetic in double before the one rounding.
 * The real maps never exist in HBM.  oa_plan_set_option(p, OA_OPT_WIN_FUSED, 0): per plane oa_fft_c2r_windowed -> real map in HBM ->
 * oa_fft_r2c(width = leg_cols, rband = leg_rows), then d. (the A/B path, as for oa_mc_run_windowed).  Steps 2-4 are oa_mc_run_mv's.  With
 * host_meanfield one more launch per realisation: a thread owns one mode of kappa's band (kappa_cols, kappa_rows), loads the nest kappa_hat
 * values once, adds each into its stack and the weighted sum, formed in registers, into the MV stack (no atomics: deterministic).
 * Realisation i's contribution to n, S, C and the stacks does not depend on how a range is cut into calls.  The entry's planes (three draw
 * planes, one column temporary per plane, the compact row planes) are taken by the first windowed call, which synchronises the device
 * once; oa_plan_release_pools frees them.  Refused before anything is launched: a window without rot_c / rot_s, a NULL stack plane, and
 * every refusal of oa_mc_run_mv.
 * ON A BAND GRID (2^a 3^b 5^c plans): the two bindings of oa_mc_run_mv (oa_qe_band_bind, then oa_mc_mv_band_bind) and its lookups and
 * refusals, every message naming this entry, mc.GaussianN0MonteCarloPol and one_call=False.  Steps 2-4 run on the inner plan.  The source
 * stage of a windowed realisation runs on the N grid: a. as above (three N-grid hc planes the entry owns); then ONE inverse mixed-radix
 * column launch over the three planes in place (grid y = plane), ONE fused row launch over them (C2R / Npix -> x window -> R2C, leg_cols
 * columns stored), and the pruned column DFT of the three row planes with the fold that rotates Q, U -> E, B in double before the one
 * rounding -- straight onto the three inner source planes.  OA_OPT_WIN_FUSED = 0: oa_fft_c2r_windowed per plane onto a real map in an
 * entry-owned plane, then the batched band input transform of oa_qe_mv_maps over the three maps with the rotation.  Until the option is
 * set (or after a value < 0) the plan takes oa_mc_run_windowed's rule: unfused for rows of up to 1200 points, fused for longer ones; rows
 * of more than 8192 points are always unfused.  Without a window step 1 is oa_grf_mix_band_inner: oa_mc_run_mv's moments bit for bit.  The
 * stacks stay N-grid planes: one launch per realisation reads the nest kappa_hat values of a mode of kappa's band from the inner planes
 * (and the inner copies of the weights) and adds them at the N grid's row and pitch; one owner per mode, no atomics.  The first windowed
 * call takes the N-grid planes (three draws, three real maps, the band input transform's scratch for three maps) with one device
 * synchronisation; they are regrown when the band widens, dropped when the binding's inner plan is remade, and freed by
 * oa_plan_release_pools.  After that the entry neither allocates nor synchronises. */
int oa_mc_run_mv_windowed(oa_plan* p, uint64_t base_seed, long sim_lo, long sim_hi, const void* const* host_covsqrt, int nest,
                          const int* host_npieces, const double* host_signs, const void* const* host_FG, const void* const* host_FH,
                          const int* host_swap, const int* host_xsrc, const int* host_ysrc, const void* const* host_Fnorm, const void* mv_weights,
                          long mv_wstride, int nspec, const int* host_a, const int* host_b, const int32_t* ids_hc, int nids, const int64_t* counts,
                          double norm, int leg_cols, int kappa_cols, int leg_rows, int kappa_rows, int mrow, const void* window_real,
                          const void* rot_c, const void* rot_s, int64_t* n, double* S, double* C, double* const* host_meanfield, void* stream);
/* One stage of oa_qe_tt_moments on the plan's own work planes, for per-kernel timing (bench.py roofline; the
 * one-call path keeps its intermediates on COMPACT planes -- pitch = active columns rounded up to a 32-column tile
 * -- so its kernels are not the same launches as the fine-grained calls on caller planes of pitch kpitch):
 * 0 = row R2C, 1 = forward column pass 1, 2 = fused leg kernel + 3-plane inverse pass 2, 3 = fused row stage,
 * 4 = 2-plane forward pass 1 + divergence kernel, 5 = binned power + moment accumulation (plan-owned dummies). */
int oa_qe_tt_stage(oa_plan* p, int stage, const void* real_map, void* stream);

/* ---- device memory helpers for hosts without a GPU array library (the reference passes NumPy arrays) --------- */
int oa_malloc(void** out, size_t bytes);
int oa_free(void* dptr);
int oa_memcpy(void* dst, const void* src, size_t bytes, int kind, void* stream); /* 1 h2d, 2 d2h, 3 d2d */
int oa_memset(void* dptr, int value, size_t bytes, void* stream);
int oa_stream_synchronize(void* stream);

/* ---- ensemble reduce over GPUs (Statistics.allreduce, stats.py:1209-1230) without torch.distributed ----------
 * RCCL communicator over the ranks of one job (librccl.so is dlopen'ed on first use).  One rank calls
 * oa_comm_unique_id and distributes the 128 bytes (MPI_Bcast in an mpi4py host), every rank then calls
 * oa_comm_init with its rank; oa_allreduce sums a device buffer in place over the ranks, stream-ordered.
 * dtype_code: 0 = float64, 1 = int64, 2 = float32. */
int oa_comm_unique_id(void* id128);
int oa_comm_init(int nranks, int rank, const void* id128, void** comm_out);
int oa_comm_destroy(void* comm);
int oa_allreduce(void* comm, void* device_buf, long count, int dtype_code, void* stream);

/* ---- layout helpers ------------------------------------------------------ */
/* hc -> full by Hermitian symmetry X(-l) = conj X(l) (what the reference's C2C of
 * a real map holds, maps.py:1613) */
int oa_hc_to_full(oa_plan* p, const void* hc_in, void* full_out, void* stream);
/* full -> hc (drops the redundant half) */
int oa_full_to_hc(oa_plan* p, const void* full_in, void* hc_out, void* stream);
/* real-valued hc-layout plane (ny,kpitch) <-> full real (ny,nx), even symmetry */
int oa_hcreal_to_full(oa_plan* p, const void* hcreal_in, void* fullreal_out, void* stream);
int oa_fullreal_to_hc(oa_plan* p, const void* fullreal_in, void* hcreal_out, void* stream);

/* ---- flat elementwise kernels (n = number of elements) --------------------
 * oa_f2power    : out = Re(conj(k1)*k2)*norm        (FourierCalc.f2power, maps.py:1620-1624)
 * oa_cmul_real  : out = k * f (complex * real)      (filter_map's `* kfilter`, maps.py:1923;
 *                                                   MapGen covsqrt*rand scalar case, maps.py:1579)
 * oa_cmul       : out = k * f (complex * complex)   (filter_map with a complex kfilter, maps.py:1923)
 * oa_mul_real   : out = a * b (real)                (QE real-space product)
 * oa_axpby_real : out = alpha*a + beta*b (real)     (observed = beamed + noise, lensing.py:516)
 * norm, alpha and beta are rounded to the planes' precision first.  n = 0 launches nothing that writes; elements at and beyond n are
 * never touched.  ALIGNMENT: oa_f2power, oa_cmul_real, oa_mul_real and oa_axpby_real move 16 bytes per access, so each of their three
 * pointers must be 16-byte aligned (any whole device allocation is; a view that starts at an odd element is not): a misaligned pointer
 * is refused before anything is launched, oa_last_error set.  oa_cmul and oa_rot2 need only the natural alignment of an element.
 * ALIASING: out may be one of the inputs (every element is read before it is written, by the same lane); partial overlaps are not
 * supported. */
int oa_f2power(int dtype, const void* k1, const void* k2, void* out_real, double norm, long n, void* stream);
int oa_cmul_real(int dtype, const void* k_in, const void* filt_real, void* k_out, long n, void* stream);
int oa_cmul(int dtype, const void* k_in, const void* filt_complex, void* k_out, long n, void* stream);
int oa_mul_real(int dtype, const void* a, const void* b, void* out, long n, void* stream);
int oa_axpby_real(int dtype, const void* a, const void* b, void* out, double alpha, double beta, long n, void* stream);
/* per-mode 2x2 rotation of two complex planes: [o1;o2] = [[c,-s],[s,c]] [i1;i2]
 * with c,s real planes (QU<->EB, enmap.map_mul(self.rot, ...), maps.py:1614-1615) */
int oa_rot2(int dtype, const void* c, const void* s, const void* i1, const void* i2, void* o1, void* o2, long n, void* stream);

/* ---- quadratic-estimator legs (hc layout) ---------------------------------
 * The reference class (lensing.Estimator/qest) is absent from the snapshot
 * (SURVEY.md F2); the contract is qest.kappa_from_map (lensing.py:973-976).
 * Real-space Hu-DeDeo-Vale form, spin = 0 (TT) or spin-2 phase variants:
 *  oa_qe_legs : from kX (gradient leg) and kY: Gx = i lx FG kX P, Gy = i ly FG kX P,
 *               H = FH kY Q, where FG, FH are real hc-layout filter planes and the
 *               optional spin-2 phase factors P,Q = exp(+-2 i phi_l) are selected by
 *               `phase_g`/`phase_h` (0: none, +1: e^{2i phi}, -1: e^{-2i phi}), and
 *               `h_times_i` multiplies H by i (B-mode leg).
 *  oa_qe_div  : out = Fnorm * (i lx Px + i ly Py)  (divergence * normalisation) */
int oa_qe_legs(oa_plan* p, const void* kX, const void* kY, const void* FG, const void* FH,
               void* Gx, void* Gy, void* H, int phase_g, int phase_h, int h_times_i, void* stream);
int oa_qe_div(oa_plan* p, const void* Px, const void* Py, const void* Fnorm, void* out, int accumulate, void* stream);

/* ---- flat-sky lensing of simulated maps (lensing.flat_taylens, lensing.py:395-440) ------------------
 * oa_lens_split  : shift[i] = rint(alpha[i]/step), delta[i] = alpha[i] - shift[i]*step (nearest pixel +
 *                  sub-pixel remainder of a displacement component; lensing.py:420-424)
 * oa_lens_gather : out[y,x] (+)= coef * src[(y+sy) mod ny, (x+sx) mod nx] * dx^pow_x * dy^pow_y
 *                  (integer-pixel remap and one Taylor term, lensing.py:428-438)
 * step is rounded to the planes' precision first; rint rounds ties to even.  VALID RANGE: oa_lens_split needs finite alpha with
 * |alpha / step| < 2^31 (the shift is stored as int32; beyond that, and for NaN, it is undefined); oa_lens_gather / oa_lens_taylor /
 * oa_lens_maps accept any shift with |shift| + max(ny, nx) < 2^31 (the index y + shift_y is formed in int32 before the wrap), of
 * either sign and any number of wraps of the map.  0 <= pow_x, pow_y, pow_x + pow_y <= 16; src != out. */
int oa_lens_split(int dtype, const void* alpha, double step, int32_t* shift, void* delta, long n, void* stream);
int oa_lens_gather(oa_plan* p, const void* src, const int32_t* shift_x, const int32_t* shift_y, const void* dx, const void* dy,
                   int pow_x, int pow_y, double coef, void* out, int accumulate, void* stream);
/* The same Taylor series with every term of every order in two launches instead of one derivative kernel, one C2R and
 * one gather per term (lensing.py:395-440; order 5 = 14 terms per map):
 *  oa_hc_derivs   : hc_out_planes[idx(a, b)] = (i lx)^a (i ly)^b hc_in for 1 <= a + b < order, idx(a, b) = n (n + 1) / 2 - 1 + b,
 *                   n = a + b, planes plane_stride complex elements apart (order (order + 1) / 2 - 1 of them).
 *  oa_lens_taylor : out = sum_{a + b < order} dx^a dy^b / (a! b!) D_ab[(y + shift_y) % ny, (x + shift_x) % nx] with D_00 = src
 *                   and D_ab the REAL planes (the C2R of the planes above, normalised) in the same order, plane_stride
 *                   real elements apart.  shift / dx / dy as produced by oa_lens_split. */
int oa_hc_derivs(oa_plan* p, const void* hc_in, int order, void* hc_out_planes, long plane_stride, void* stream);
int oa_lens_taylor(oa_plan* p, const void* src, const void* deriv_planes, long plane_stride, int order, const int32_t* shift_x,
                   const int32_t* shift_y, const void* dx, const void* dy, void* out, void* stream);
/* flat_taylens (lensing.py:395-440) of nmaps real maps (in_stride / out_stride elements apart) by ONE deflection field, given as
 * its nearest-pixel shifts and sub-pixel remainders (oa_lens_split; shared by all maps: T, Q, U of a realisation): nmaps R2Cs, then
 * the inverse transforms of all nmaps * nd derivative fields (nd = order (order + 1) / 2 - 1), SEPARABLY: per map and y-derivative
 * order b one column transform of (i ly)^b k (passes 1 and 2 on ONE plan-owned hc plane, which stays in the infinity cache) and one
 * row launch that takes every x-derivative (i lx)^a at its load (the derivative spectra never exist in HBM) -- and one
 * gather pass per map (oa_lens_taylor).  Same results as oa_hc_derivs + C2R per term + oa_lens_taylor.  The planes live in a
 * plan-owned pool allocated / grown on first use (that call synchronises the device once): nmaps * (1 + nd) planes + one hc plane,
 * e.g. 6.2 GB for T, Q, U at 4096^2 float64 and order 5; oa_plan_release_pools frees it (and the pools of oa_qe_mv /
 * oa_qe_tt_splits / oa_mc_run), the next call reallocates. */
int oa_lens_maps(oa_plan* p, int nmaps, const void* real_in, long in_stride, int order, const int32_t* shift_x, const int32_t* shift_y,
                 const void* dx, const void* dy, void* real_out, long out_stride, void* stream);
/* The same from the maps' hc transforms (a simulation that DREW its fields in harmonic space has them already: MapGen.get_map's
 * transform, lensing.py:499-512): `hc_in` holds nmaps planes hc_stride complex elements apart, map = scale * C2R(hc_in)
 * (scale = 1 / sqrt(Ny Nx) for MapGen's unitary draws).  No forward transform is taken and the undisplaced map itself -- the
 * (a, b) = (0, 0) term -- leaves the same batched row launch as the x-derivatives of the b = 0 column transform: nmaps fewer
 * R2Cs and nmaps fewer separate C2Rs than oa_lens_maps on the inverse-transformed maps, same results to rounding. */
int oa_lens_maps_hc(oa_plan* p, int nmaps, const void* hc_in, long hc_stride, double scale, int order, const int32_t* shift_x,
                    const int32_t* shift_y, const void* dx, const void* dy, void* real_out, long out_stride, void* stream);
int oa_plan_release_pools(oa_plan* p);

/* ---- analytic N1 bias of the TT estimator: direct mode-pair sums (csrc/n1.hpp) ----
 * For each of nL reconstructed modes L (full-plane indices host_Ly[i], host_Lx[i]; host arrays), with l2 = L - l1, l2' = L - l1',
 *     g_L(l1, l2) = (L.l1) wg(l1) wh(l2),      f(a, b) = C_a (m.a) + C_b (m.b),   m = a + b,
 *     S(L) = sum_{l1} sum_{l1'} g_L(l1, l2) g_L(l1', l2') [ Cpp(l1 - l1') f(l1, -l1') f(l2, -l2') + Cpp(l1 - l2') f(l1, -l2') f(l2, -l1') ]
 * goes to S_out[i] (device, nL doubles);  N1_phi(L) = A_L^2 S(L) / Area^2,  N1_kappa(L) = [L (L + 1) / 2]^2 N1_phi(L).
 * wg_hc, wh_hc (the DECONVOLVED leg weights), cr_hc (the response spectrum C) and cpp_hc (C^phiphi on the map's grid) are real hc-layout
 * planes of a FLOAT64 plan; a mode with negative kx is read through its Hermitian partner (-ky mod ny, -kx).  The sums run over the modes
 * |ky index| < leg_rows, |kx index| < leg_cols (the weights' band) in plain index arithmetic, float64 throughout; l vectors come from
 * the plan's axes (oa_plan_set_laxes).  Any plan kind (power-of-two, 2^a 3^b 5^c, chirp-z): only the axes and the row pitch are used.
 * Per L: a prologue launch (box-ordered mode table), pair launches bounded in their pair count (tiles of l1 in registers x chunks of l1'
 * with their Cpp vector in LDS), one fold workgroup; per-workgroup partials in a plan-owned pool (taken on the first call, grown on
 * demand -- that call may synchronise --, freed by oa_plan_release_pools), no atomics: S_out is the same bit for bit on every run and
 * however a list of L is cut into calls.  Stream-ordered.
 * Refused by name before anything is launched: a float32 plan; axes not set; legs not band-limited enough for all four modes of a
 * pair to be un-aliased (needs 4 (leg_rows - 1) < ny and 4 (leg_cols - 1) < nx); nL < 1; an L index outside the plane. */
int oa_n1_tt(oa_plan* p, const void* wg_hc, const void* wh_hc, const void* cr_hc, const void* cpp_hc, int leg_cols, int leg_rows, int nL,
             const int32_t* host_Ly, const int32_t* host_Lx, double* S_out, void* stream);

/* ---- radial binning (stats.bin2D, stats.py:782-811) ------------------------
 * oa_digitize : ids[i] = np.digitize(x[i], edges, right=True) (stats.py:786):
 *               e[id-1] < x <= e[id]; 0 = underflow, nedges = overflow. x, edges
 *               are float64 (bit-exact comparisons); ids are int32.
 * oa_modl_digitize : same, with x = sqrt(ly[y]^2 + lx[x]^2) computed on device in
 *               float64 with IEEE round-to-nearest mul/add/sqrt and no FMA
 *               contraction (NumPy op order of enmap.modlmap).  `pitch`/`width`
 *               select the plane layout: full plane pitch=width=nx; hc plane
 *               pitch=kpitch,width=nx/2+1 (pad columns get id -1 = ignored).
 * oa_bin      : sums[id] += v, counts[id] += m over all i with 0 <= ids[i] < nids
 *               (any other id, negative or >= nids, drops the element) where
 *                 v = data[i] (mode 0) | (data[i]-aux[id])^2 (mode 1; no weights), times
 *                 weights[i] if weights != NULL, times the Hermitian multiplicity m,
 *                 m = 1 (herm_nxh < 0) or {1 for col 0 and col nxh, 2 for 0<col<nxh,
 *                 0 = dropped for col > nxh: the row padding} with col = i % herm_pitch
 *                 (herm_pitch a positive multiple of 4, n a multiple of it);
 *               counts[] are exact int64 (unweighted) ; wsums[] = sum of weights*m (f64).
 *               skip_nan != 0 drops NaN data, with their weights (mask_nan=True, stats.py:793).
 *               Output arrays have nids = nedges+1 entries and are OVERWRITTEN.
 *               Deterministic: per-workgroup partials reduced in fixed order.
 *               `scratch` must hold oa_bin_scratch_bytes(nids) bytes. */
int oa_digitize(const double* x, long n, const double* edges, int nedges, int32_t* ids, void* stream);
int oa_modl_digitize(const double* ly, const double* lx, int ny, int nx, long pitch, int width,
                     const double* edges, int nedges, int32_t* ids, double* modl_out, void* stream);
long oa_bin_scratch_bytes(int nids);
int oa_bin(int dtype, const void* data, const int32_t* ids, const void* weights, const double* aux, long n,
           int nids, int mode, int skip_nan, long herm_pitch, int herm_nxh, double* sums, int64_t* counts,
           double* wsums, void* scratch, void* stream);

/* oa_bin_power: FourierCalc.f2power (maps.py:1620-1624) fused into oa_bin: the binned value is
 * Re(conj(k1[i]) k2[i]) * norm for complex planes k1, k2 (k1 == k2 for auto spectra); the 2-D power
 * plane is never written.  Same ids / multiplicity / determinism contract as oa_bin (mode 0).
 * With weights != NULL the binned value is multiplied by weights[i] and wsums replaces counts, as in oa_bin.
 * active_cols > 0 (Hermitian mode only): only columns < active_cols of each row are binned, exactly -- whatever
 * the planes hold at columns >= active_cols never reaches sums or counts (for planes that vanish beyond them the
 * sums are unchanged); COUNTS then cover the visited columns only -- take the
 * data-independent counts from one full oa_bin_power / oa_bin call at plan time.  active_rows > 0 (with
 * active_cols): additionally only the rows of the band y < active_rows or y > ny - active_rows.  active_cols >=
 * herm_pitch is no limit at all: whole planes are binned and active_rows is ignored. */
int oa_bin_power(int dtype, const void* k1, const void* k2, double norm, const int32_t* ids, const void* weights, long n,
                 int nids, long herm_pitch, int herm_nxh, double* sums, int64_t* counts, double* wsums, void* scratch, int active_cols, int active_rows,
                 void* stream);
/* oa_bin_power_multi: nspec binned (cross-)spectra of a few hc planes in ONE pass and one launch pair.  Field f (0 <= f < nfields <= 6) is
 * the hc plane at k0 + f * fstride (complex elements, row pitch kpitch, ny rows); with w0 != NULL, w0 + f * wstride are hc-real weight
 * planes and field index nfields names the per-mode weighted sum sum_f w_f k_f, formed in registers and never stored.  Spectrum s is
 * Re(conj(F_a[s]) F_b[s]) * norm times oa_bin_power's Hermitian multiplicity (1 for column 0 and column nxh, 2 between); the stored
 * values are converted to double first, products and sums are formed in double in both precisions.  sums[s * nids + id] is overwritten
 * (device, nspec * nids doubles); scratch: oa_bin_power_multi_scratch_bytes(nspec, nids) device bytes (-1 for a refused pair).  A mode's
 * nfields values are loaded once and feed all nspec products.  active_cols / active_rows: oa_bin_power's contract (planes that vanish
 * outside the region give the sums of a full visit; rows only together with columns).  Deterministic: per-workgroup partial sums folded
 * in a fixed order, no floating-point atomics -- two runs give bit-identical sums.  Refused before any launch: nspec outside 1..28 (seven
 * fields have 28 distinct pairs), nids outside 1..1024, nspec * nids > 4096 (the workgroup keeps one table of partial sums per wave in
 * LDS: 4 waves x 4096 x 8 B = 128 KiB of the 160 KiB a gfx950 workgroup can take), nfields outside 1..6, a field index outside
 * [0, nfields], index nfields without w0, NULL pointers, a bad dtype. */
long oa_bin_power_multi_scratch_bytes(int nspec, int nids);
int oa_bin_power_multi(int dtype, int nfields, const void* k0, long fstride, const void* w0, long wstride, int nspec, const int* host_a,
                       const int* host_b, double norm, const int32_t* ids_hc, int nids, int ny, long kpitch, int nxh, int active_cols,
                       int active_rows, double* sums, void* scratch, void* stream);

/* ---- Gaussian random fields (MapGen.get_map, maps.py:1576-1587) --------------
 * Fills an hc plane with Hermitian-consistent complex white noise of unit
 * variance per full-plane mode, scaled per mode by the real hc-layout plane
 * `covsqrt` (may be NULL): the C2R of the result with the unitary scale
 * 1/sqrt(ny*nx) is statistically identical to
 * enmap.ifft(covsqrt*rand_gauss_harm).real.  Counter-based Philox4x32-10,
 * key = (seed, stream_id), so realisations are independent of launch geometry. */
int oa_grf_hc(oa_plan* p, uint64_t seed, uint64_t stream_id, const void* covsqrt_hc, void* hc_out, void* stream);
/* The draw INSIDE the inverse column transform: plane z (z < nreal, zstride complex elements apart) of hc_out is bit for bit
 * oa_fft_cols(inverse = 1, scale = 1, width = nx/2 + 1) of oa_grf_hc(seed, stream_id + z, covsqrt_hc) -- the load of column pass 1
 * evaluates the modes (same Philox counters, same self-conjugate rules at columns 0 and nx/2, same product with the amplitude), so the
 * drawn planes are never stored; pass 2 is the in-place launch.  A lane pair shares each counter (columns 2 p, 2 p + 1): as many Philox
 * evaluations as oa_grf_hc.  Power-of-two plans only (ny >= 32); other plans are refused by name. */
int oa_grf_hc_icols(oa_plan* p, uint64_t seed, uint64_t stream_id, int nreal, const void* covsqrt_hc, void* hc_out, long zstride, void* stream);
/* The same draw restricted to the ACTIVE region (columns < width, rows y < rband or y > ny - rband; 0 = all): a
 * bit-identical subset of oa_grf_hc's plane (every mode keeps its Philox counter), the rest of hc_out is not written.
 * A Monte-Carlo loop whose estimator reads only its leg band (oa_mc_run does this itself) draws ~1 % of the modes. */
int oa_grf_hc_band(oa_plan* p, uint64_t seed, uint64_t stream_id, const void* covsqrt_hc, void* hc_out, int width, int rband,
                   void* stream);
/* MapGen.get_map's draw in ONE pass (maps.py:1579-1587: covsqrt * rand_gauss_harm, then harm2map's rotation): ncomp (1..3) white
 * fields of streams (seed, stream_id0 + j) -- bit-identical to oa_grf_hc's -- mixed by the covariance square root,
 *     v_i = sum_j covsqrt_hc[i * ncomp + j] * w_j        (hc-real planes; a NULL entry is a zero block),
 * then, with rotation planes (ncomp == 3: components 1, 2 <- (x1 c - x2 s, x1 s + x2 c), oa_rot2's convention),
 *     hc_in == NULL : hc_out[i] = scale * rot(v)_i                       (unlensed T, Q, U transforms; kappa)
 *     hc_in != NULL : hc_out[i] = rot(hc_in * filt_hcreal)_i + scale * v_i   (beam x lensed Q, U -> E, B, + noise: the observed
 *                                                                          transforms of lensing.py:513-516 in one pass)
 * filt_hcreal may be NULL (= 1); hc_out[i] may alias hc_in[i]. */
int oa_grf_mix(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ncomp, const void* const* covsqrt_hc, const void* rot_c, const void* rot_s,
               const void* const* hc_in, const void* filt_hcreal, double scale, void* const* hc_out, void* stream);
/* The leg band of oa_grf_mix(p, seed, stream_id0, ncomp, covsqrt_hc, NULL, NULL, NULL, NULL, scale, hc_out, stream): columns < width and
 * rows y < rband or y > ny - rband (0 = all), a bit-identical subset of the full draw -- every mode keeps its Philox counter and the
 * self-conjugate edge rules --; the rest of each output plane is not written.  Any plan kind (element-wise on the N-grid hc layout),
 * ncomp 1..3, NULL blocks are zero.  What oa_grf_hc_band is to oa_grf_hc. */
int oa_grf_mix_band(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ncomp, const void* const* covsqrt_hc, double scale,
                    void* const* hc_out, int width, int rband, void* stream);
/* The mixed T, Q, U draw INSIDE the inverse column transform: plane 3 t + c (t < ntriples, c = 0 T, 1 Q, 2 U; planes zstride complex elements
 * apart) of hc_out is bit for bit oa_fft_cols(inverse = 1, scale = 1, width = nx/2 + 1) of component c of
 *     oa_grf_mix(p, seed, stream_id0 + 3 t, ncomp = 3, covsqrt_hc, rot_c = c, rot_s = -s, NULL, NULL, 1, ...)
 * where rot_c = c, rot_s = s are the caller's Q, U -> E, B planes as oa_mc_run_mv_windowed takes them (the sine enters negated: E, B -> Q, U);
 * both NULL = no rotation, the planes are T, E, B.  Same Philox counters ys * npair + x / 2 of streams stream_id0 + 3 t + k, same
 * self-conjugate rules at columns 0 and nx/2, same 1 / sqrt 2, mixing order and rotation expressions as oa_grf_mix.  A workgroup of column
 * pass 1 owns one column tile of one TRIPLE: it evaluates the three streams' normals ONCE (a lane pair shares each counter, as in
 * oa_grf_hc_icols), keeps them in registers and takes the three planes through the pipeline one after the other; pass 2 is the in-place
 * launch over all planes.  Columns beyond nx/2 are not written.  Power-of-two plans with ny >= 32, nx >= 4 only; other plans are refused
 * by name, as are ntriples outside 1 <= 3 ntriples <= 65535, a zstride below one plane, one rotation plane without the other, and float64
 * plans of 32768 rows and more (512-thread pass-1 workgroups: a triple's normals do not fit their registers without spilling; the entry
 * oa_mc_run_rdn0_mv_windowed runs its per-triple sequence there). */
int oa_grf_mix_icols(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ntriples, const void* const* covsqrt_hc, const void* rot_c,
                     const void* rot_s, void* hc_out, long zstride, void* stream);
/* The band of oa_grf_mix_band written into the hc layout of an INNER grid of `my` rows and row pitch `out_pitch` (complex elements): Philox
 * counters, self-conjugate edge rules and the covsqrt planes are those of the plan's N grid at row y, the value goes to row y of the
 * output planes for y < rband and to row y - ny + my above (ky mod my: the band grid's layout), same column.  Bit-identical to
 * oa_grf_mix_band's values at the same mode; nothing outside the band of the output planes is written.  Refused before any launch:
 * ncomp outside 1..3, a band that is not positive, 2 rband - 1 > min(ny, my), width > nx/2 + 1, 2 ceil(width / 2) > out_pitch, a NULL
 * output plane. */
int oa_grf_mix_band_inner(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ncomp, const void* const* covsqrt_hc, double scale,
                          void* const* hc_out, int my, long out_pitch, int width, int rband, void* stream);
/* ntriples (1 or 2) T, E, B triples of oa_grf_mix_band_inner in ONE launch: hc_out holds 3 ntriples planes, and planes 3 z .. 3 z + 2 are
 * bit for bit those of oa_grf_mix_band_inner(p, seed, stream_id0 + 3 z, ncomp = 3, covsqrt_hc, scale, hc_out + 3 z, my, out_pitch, width,
 * rband, stream).  The triple is the grid's z index: a thread evaluates each Philox counter once for its triple; nothing outside the band of
 * the output planes is written.  On an inner grid of 128^2 .. 512^2 points a draw launch is latency-bound, and a realisation of
 * oa_mc_run_rdn0_mv needs s (streams 6 i ..) and s' (6 i + 3 ..): this is its source stage on a band grid.  Refused before any launch:
 * ntriples outside 1..2, and what oa_grf_mix_band_inner refuses (a band that is not positive, 2 rband - 1 > min(ny, my),
 * width > nx/2 + 1, 2 ceil(width / 2) > out_pitch, a NULL output plane). */
int oa_grf_mix_band_inner_triples(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ntriples, const void* const* covsqrt_hc, double scale,
                                  void* const* hc_out, int my, long out_pitch, int width, int rband, void* stream);
/* real white noise N(0,1) plane of n elements (enmap.rand_gauss) */
int oa_randn(int dtype, uint64_t seed, uint64_t stream_id, void* out, long n, void* stream);

/* ---- one-pass moment accumulation (Statistics.add, stats.py:1068-1090) ---------
 * n += 1 ; S += x ; C += x x^T  for a device vector x of length d (float64). */
int oa_moments_add(const double* x, int d, int64_t* n, double* S, double* C, void* stream);
/* Same with x_a = sums[a] / counts[a] (the bin means of stats.bin2D.bin, stats.py:790-811) formed in the
 * kernel: feeds the interior slots of oa_bin / oa_bin_power output directly (pass sums+1, counts+1, d=nbins). */
int oa_moments_add_binned(const double* sums, const int64_t* counts, int d, int64_t* n, double* S, double* C, void* stream);
/* stack accumulation (Statistics.add_stack, stats.py:1124-1150): acc(f64) += x (dtype) */
int oa_stack_add(int dtype, const void* x, double* acc, long n, void* stream);

/* ---- measurement helpers -------------------------------------------------------
 * Streaming device copy / read of `bytes` (a multiple of 16) with 16-byte accesses: the bandwidth ceiling bench.py
 * measures in the same run as the kernels it prices against it.  `sink`: >= 8 MiB of device scratch (one word per
 * thread of the read probe). */
int oa_probe_copy(void* dst, const void* src, size_t bytes, void* stream);
int oa_probe_read(const void* src, size_t bytes, void* sink, void* stream);
/* The attainable float64 vector rate, measured in the same run as the N1 pair kernel it prices (tools/n1_bench.py): `blocks` workgroups
 * (<= 65536) of 256 threads, each thread `iters` (<= 2^24) steps of 8 independent x = fma(x, a, b) chains and nothing else;
 * blocks x 256 x iters x 8 fused multiply-adds in all.  out: blocks 256 doubles (written once, so that the loop is kept). */
int oa_probe_fma64(int blocks, long iters, double a, double b, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORPHICS_AMD_H */
