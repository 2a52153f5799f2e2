// Per-mode arithmetic of the split-based 4-point combination (SplitLensing.cross_estimator, lensing.py:980-1003), shared by
// split_cross_power_kernel (elementwise.hip: K planes on the caller's grid) and band_split_power_kernel (band.hip: K planes on the
// inner grid of a band-grid plan) -- ONE definition, so the two return the same bits for the same K values.
// K[i*N+j] = QE(X leg from split i, Y leg from split j).  The QE is bilinear, so with s = mean of the splits
//   QE(s,s) = mean_ij K_ij,   (QE(m_i,s) + QE(s,m_i))/2 = sum_j (K_ij + K_ji) / (2N),
// and every term of the estimator is a linear combination of the K's: one pass, arithmetic in f64.
#pragma once
#include "cx.hpp"

namespace oa {

// ld(k): this mode's value of plane k = i * N + j, a cx<float> or cx<double>
template <int N, typename Load>
OA_D double split_cross_mode(const Load& ld, double norm) {
    double rcr[N], rci[N], dr[N], di[N];           // rc_i = sum_j (K_ij + K_ji), d_i = K_ii
#pragma unroll
    for (int i = 0; i < N; ++i) rcr[i] = rci[i] = 0.0;
    double tr = 0.0, ti = 0.0, pij = 0.0;         // sum of all K, sum_{i<j} |K_ij + K_ji|^2
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const auto d = ld(i * N + i);
        dr[i] = (double)d.x; di[i] = (double)d.y;
        rcr[i] += 2.0 * dr[i]; rci[i] += 2.0 * di[i];
        tr += dr[i]; ti += di[i];
#pragma unroll
        for (int j = i + 1; j < N; ++j) {
            const auto a = ld(i * N + j), b = ld(j * N + i);
            const double sr = (double)a.x + (double)b.x, si = (double)a.y + (double)b.y;
            rcr[i] += sr; rci[i] += si; rcr[j] += sr; rci[j] += si;
            tr += sr; ti += si;
            pij += sr * sr + si * si;
        }
    }
    const double n = (double)N, n2 = n * n;
    double sdr = 0.0, sdi = 0.0, pic = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        sdr += dr[i]; sdi += di[i];
        const double cr = rcr[i] / (2.0 * n) - dr[i] / n, ci = rci[i] / (2.0 * n) - di[i] / n;    // k_i - k_ii / N
        pic += cr * cr + ci * ci;
    }
    const double kcr = (tr - sdr) / n2, kci = (ti - sdi) / n2;                                   // QE(s,s) - sum_i k_ii / N^2
    return (n2 * n2 * (kcr * kcr + kci * kci) - 4.0 * n2 * pic + pij) * norm / (n * (n - 1.0) * (n - 2.0) * (n - 3.0));
}

}  // namespace oa
