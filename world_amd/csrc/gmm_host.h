// gmm_host.h -- the joint-density Gaussian mixture's host arithmetic (include/world_hip.h: world_hip_gmm_prepare /
// _gmm_model_parts / _gmm_update state the rule).  No GPU, no HIP type, no other header of the library.  Everything is
// computed in long double and rounded once to double.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace world_hip {

constexpr int kGmmMaxMix = 256, kGmmMaxDim = 128;

// The prepared model: what the device multiplies by, padded to the matrix unit's 16-wide tiles with zeros.
//   c [M] | mux [M][Kp] | muy [M][Ep] | v [M][Ep] | UT [M][Kp][Kp] (U transposed: UT[k][j] = U[j][k]) | AT [M][Kp][Ep]
//   (AT[k][i] = A[i][k]);  Kp = Dx rounded up to 16, Ep = Dy rounded up to 16 (0 for Dy = 0).
struct GmmLayout {
  int M, Dx, Dy, Kp, Ep;
  size_t c, mux, muy, v, ut, at, doubles;
};
inline GmmLayout gmm_layout(int M, int Dx, int Dy) {
  GmmLayout g;
  g.M = M; g.Dx = Dx; g.Dy = Dy;
  g.Kp = (Dx + 15) / 16 * 16;
  g.Ep = (Dy + 15) / 16 * 16;
  const size_t m = (size_t)M, kp = (size_t)g.Kp, ep = (size_t)g.Ep;
  g.c = 0;
  g.mux = g.c + m;
  g.muy = g.mux + m * kp;
  g.v = g.muy + m * ep;
  g.ut = g.v + m * ep;
  g.at = g.ut + m * kp * kp;
  g.doubles = g.at + m * kp * ep;
  return g;
}
// nullptr, or why the shape is refused
inline const char *gmm_shape(int M, int Dx, int Dy) {
  if (M < 1 || M > kGmmMaxMix) return "the number of mixtures must lie in [1, 256]";
  if (Dx < 1 || Dx > kGmmMaxDim) return "the source dimension must lie in [1, 128]";
  if (Dy < 0 || Dy > kGmmMaxDim) return "the target dimension must lie in [0, 128]";
  return nullptr;
}

// the rule's prepare; "" or the refusal
inline std::string gmm_prepare_host(int M, int Dx, int Dy, const double *w, const double *mu, const double *cov, double *model) {
  typedef long double ld;
  const GmmLayout g = gmm_layout(M, Dx, Dy);
  const int P = Dx + Dy;
  const ld ln2pi = logl(2.0L * acosl(-1.0L));
  std::vector<double> out(g.doubles, 0.0);
  std::vector<ld> L((size_t)Dx * Dx), U((size_t)Dx * Dx), W((size_t)Dy * Dx);
  char why[160];
  for (int m = 0; m < M; ++m) {
    if (!std::isfinite(w[m]) || !(w[m] > 0)) {
      snprintf(why, sizeof why, "mixture %d: its weight is not finite and positive", m);
      return why;
    }
    const double *S = cov + (size_t)m * P * P;
    ld ln_det = 0;
    for (int i = 0; i < Dx; ++i)                            // Cholesky, row by row, the lower triangle of Sxx alone
      for (int j = 0; j <= i; ++j) {
        ld s = S[(size_t)i * P + j];
        for (int k = 0; k < j; ++k) s -= L[(size_t)i * Dx + k] * L[(size_t)j * Dx + k];
        if (i == j) {
          if (!std::isfinite((double)s) || !(s > 0)) {
            snprintf(why, sizeof why, "mixture %d: pivot %d of the source covariance is not finite and positive", m, i);
            return why;
          }
          L[(size_t)i * Dx + i] = sqrtl(s);
          ln_det += logl(L[(size_t)i * Dx + i]);
        } else {
          L[(size_t)i * Dx + j] = s / L[(size_t)j * Dx + j];
        }
      }
    for (int j = 0; j < Dx; ++j)                            // U = L^-1, column by column
      for (int i = 0; i < Dx; ++i) {
        if (i < j) { U[(size_t)i * Dx + j] = 0; continue; }
        ld s = i == j ? 1.0L : 0.0L;
        for (int k = j; k < i; ++k) s -= L[(size_t)i * Dx + k] * U[(size_t)k * Dx + j];
        U[(size_t)i * Dx + j] = s / L[(size_t)i * Dx + i];
      }
    out[g.c + m] = (double)(logl((ld)w[m]) - 0.5L * Dx * ln2pi - ln_det);
    for (int k = 0; k < Dx; ++k) out[g.mux + (size_t)m * g.Kp + k] = mu[(size_t)m * P + k];
    for (int i = 0; i < Dy; ++i) out[g.muy + (size_t)m * g.Ep + i] = mu[(size_t)m * P + Dx + i];
    double *ut = out.data() + g.ut + (size_t)m * g.Kp * g.Kp;
    for (int j = 0; j < Dx; ++j)
      for (int k = 0; k <= j; ++k) ut[(size_t)k * g.Kp + j] = (double)U[(size_t)j * Dx + k];
    // W = Syx U' ([Dy][Dx]); A = W U; v = diag(Syy) - the rows of W squared (= diag(Syy - A Sxy))
    double *at = out.data() + g.at + (size_t)m * g.Kp * g.Ep;
    for (int i = 0; i < Dy; ++i) {
      const double *syx = S + (size_t)(Dx + i) * P;
      ld q = 0;
      for (int k = 0; k < Dx; ++k) {
        ld s = 0;
        for (int j = 0; j <= k; ++j) s += (ld)syx[j] * U[(size_t)k * Dx + j];
        W[(size_t)i * Dx + k] = s;
        q += s * s;
      }
      for (int j = 0; j < Dx; ++j) {
        ld s = 0;
        for (int k = j; k < Dx; ++k) s += W[(size_t)i * Dx + k] * U[(size_t)k * Dx + j];
        at[(size_t)j * g.Ep + i] = (double)s;
      }
      const ld v = (ld)syx[Dx + i] - q;
      if (!(v > 0) || !std::isfinite((double)v)) {
        snprintf(why, sizeof why, "mixture %d: the conditional variance of target dimension %d is not positive", m, i);
        return why;
      }
      out[g.v + (size_t)m * g.Ep + i] = (double)v;
    }
  }
  for (size_t i = 0; i < g.doubles; ++i) model[i] = out[i];
  return "";
}

// the M-step's finish; "" or the refusal (nothing is written then)
inline std::string gmm_update_host(int M, int P, const double *N, const double *S1, const double *G, const double *shift,
                                   double total_rows, double reg, double *w, double *mu, double *cov) {
  typedef long double ld;
  char why[160];
  for (int m = 0; m < M; ++m)
    if (!(N[m] >= (double)(P + 1))) {
      snprintf(why, sizeof why, "mixture %d is starved: it holds %.6g rows' worth of weight, below the %d a full covariance needs",
               m, N[m], P + 1);
      return why;
    }
  for (int m = 0; m < M; ++m) {
    const ld n = N[m];
    w[m] = (double)(n / (ld)total_rows);
    for (int i = 0; i < P; ++i) mu[(size_t)m * P + i] = (double)((ld)shift[(size_t)m * P + i] + (ld)S1[(size_t)m * P + i] / n);
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j) {
        const ld di = (ld)S1[(size_t)m * P + i] / n, dj = (ld)S1[(size_t)m * P + j] / n;
        cov[((size_t)m * P + i) * P + j] = (double)((ld)G[((size_t)m * P + i) * P + j] / n - di * dj + (i == j ? (ld)reg : 0.0L));
      }
  }
  return "";
}

}  // namespace world_hip
