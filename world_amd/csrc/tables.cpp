// tables.cpp -- host construction of the twiddle and RNG jump-ahead tables, and the resampler's and the mel-cepstrum's
// host arithmetic.
#include "tables.h"
#include "mcep_host.h"
#include "resample_host.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

namespace world_hip {

void build_twiddles(double2 *out) {
  const long double two_pi = 6.283185307179586476925286766559L;
  for (int k = 0; k < kTwN; ++k) {
    long double a = two_pi * k / kTwN;
    out[k] = make_double2((double)cosl(a), (double)sinl(a));
  }
  // exact values on the axes
  out[0] = make_double2(1.0, 0.0);
  out[kTwN / 4] = make_double2(0.0, 1.0);
  out[kTwN / 2] = make_double2(-1.0, 0.0);
  out[3 * kTwN / 4] = make_double2(0.0, -1.0);
  // dense quarter-wave tables, one per transform size, copied from the entries above (bitwise the same values)
  double *q = reinterpret_cast<double *>(out + kTwN);
  for (int lg = 2; lg <= kTwLog2; ++lg)
    for (int r = 0; r <= (1 << (lg - 2)); ++r) q[quarter_table_offset(lg) + r] = out[(size_t)r << (kTwLog2 - lg)].x;
  if (kQuarterDoubles & 1) q[kQuarterDoubles] = 0.0;
}

namespace {
struct V128 { uint32_t w[4]; };                 // state bits: x = w[0] ... w = w[3]
struct M128 { V128 col[128]; };                 // column c = image of basis vector e_c

// one xorshift128 step (reference src/matlabfunctions.cpp:246-251)
V128 step(V128 s) {
  uint32_t t = s.w[0] ^ (s.w[0] << 11);
  V128 r;
  r.w[0] = s.w[1]; r.w[1] = s.w[2]; r.w[2] = s.w[3];
  r.w[3] = (s.w[3] ^ (s.w[3] >> 19)) ^ (t ^ (t >> 8));
  return r;
}
V128 apply(const M128 &m, const V128 &v) {
  V128 r = {{0, 0, 0, 0}};
  for (int c = 0; c < 128; ++c)
    if ((v.w[c >> 5] >> (c & 31)) & 1u)
      for (int k = 0; k < 4; ++k) r.w[k] ^= m.col[c].w[k];
  return r;
}
M128 mul(const M128 &a, const M128 &b) {        // a * b  (apply b first)
  M128 r;
  for (int c = 0; c < 128; ++c) r.col[c] = apply(a, b.col[c]);
  return r;
}
}  // namespace

void build_jump_tables(uint4 *out) {
  M128 t;
  for (int c = 0; c < 128; ++c) {
    V128 e = {{0, 0, 0, 0}};
    e.w[c >> 5] = 1u << (c & 31);
    t.col[c] = step(e);                          // the step is linear over GF(2)
  }
  M128 m = t;
  for (int i = 1; i < 12; ++i) m = mul(t, m);    // T^12 : one randn() call
  for (int level = 0; level < kJumpLevels; ++level) {
    uint4 *tab = out + (size_t)level * kJumpStride;
    for (int nib = 0; nib < 32; ++nib)
      for (int v = 0; v < 16; ++v) {
        V128 acc = {{0, 0, 0, 0}};
        for (int b = 0; b < 4; ++b)
          if ((v >> b) & 1)
            for (int k = 0; k < 4; ++k) acc.w[k] ^= m.col[4 * nib + b].w[k];
        tab[nib * 16 + v] = make_uint4(acc.w[0], acc.w[1], acc.w[2], acc.w[3]);
      }
    m = mul(m, m);                               // -> 2^(level+1) calls
  }
}

// ---- the resampler (include/world_hip.h: world_hip_resample_batch) -------------------------------------------------------
namespace {
long long gcd_ll(long long a, long long b) {
  while (b) { const long long t = a % b; a = b; b = t; }
  return a;
}
// I0 by its power series sum ((x / 2)^k / k!)^2: every term positive, so the sum loses nothing to cancellation
long double bessel_i0(long double x) {
  const long double h = 0.25L * x * x;
  long double term = 1.0L, sum = 1.0L;
  for (int k = 1; k < 1000; ++k) {
    term *= h / ((long double)k * k);
    sum += term;
    if (term < 1e-22L * sum) break;
  }
  return sum;
}
}  // namespace

int resample_length(long long n_in, long long fs_in, long long fs_out) {
  if (n_in < 1 || fs_in < 1 || fs_out < 1 || n_in > INT_MAX || fs_in > INT_MAX || fs_out > INT_MAX) return -1;
  const long long g = gcd_ll(fs_in, fs_out), L = fs_out / g, M = fs_in / g;
  const long long n = (n_in * L + M - 1) / M;               // < 2^62
  return n > INT_MAX ? -1 : (int)n;
}

const char *resample_shape(long long fs_in, long long fs_out, const ResampleDesign &d, ResampleShape *shape) {
  static thread_local char why[200];
  if (fs_in < 1 || fs_out < 1 || fs_in > INT_MAX || fs_out > INT_MAX) {
    snprintf(why, sizeof why, "sampling rates %lld -> %lld: each must be at least 1", fs_in, fs_out);
    return why;
  }
  if (d.zeros < 1 || d.zeros > 256) { snprintf(why, sizeof why, "zeros %d outside [1, 256]", d.zeros); return why; }
  if (!(d.rolloff > 0.0 && d.rolloff <= 1.0)) { snprintf(why, sizeof why, "rolloff %g outside (0, 1]", d.rolloff); return why; }
  if (!(d.beta >= 0.0 && d.beta <= 40.0)) { snprintf(why, sizeof why, "kaiser_beta %g outside [0, 40]", d.beta); return why; }
  const long long g = gcd_ll(fs_in, fs_out), L = fs_out / g, M = fs_in / g, B = L > M ? L : M;
  const long long W = (d.zeros * B + L - 1) / L;
  if (2 * W > kResampleMaxTaps) {
    snprintf(why, sizeof why, "%lld -> %lld Hz with %d zero crossings needs %lld taps per output, above %d", fs_in, fs_out,
             d.zeros, 2 * W, kResampleMaxTaps);
    return why;
  }
  if (L * 2 * W > kResampleMaxCoefs) {
    snprintf(why, sizeof why, "%lld -> %lld Hz has L = %lld phases of %lld taps: %lld coefficients, above %lld (the rates "
             "share too small a divisor)", fs_in, fs_out, L, 2 * W, L * 2 * W, kResampleMaxCoefs);
    return why;
  }
  shape->L = L; shape->M = M; shape->W = W;
  return nullptr;
}

void build_resample_taps(const ResampleShape &s, const ResampleDesign &d, double *table) {
  const long double pi = 3.14159265358979323846264338327950288L;
  const long long L = s.L, M = s.M, W = s.W, B = L > M ? L : M, zb = d.zeros * B;
  const long double scale = (long double)d.rolloff * (L < M ? L : M) / M, i0_beta = bessel_i0(d.beta);
  for (long long p = 0; p < L; ++p)
    for (long long i = 0; i < 2 * W; ++i) {
      const long long q = p + (W - 1 - i) * L;
      double h = 0.0;
      if (q < zb && -q < zb) {
        const long double u = (long double)q / zb, x = pi * ((long double)d.rolloff * q / B);
        const long double sinc = q == 0 ? 1.0L : sinl(x) / x;
        h = (double)(scale * sinc * bessel_i0(d.beta * sqrtl((1.0L - u) * (1.0L + u))) / i0_beta);
      }
      table[p * 2 * W + i] = h;
    }
}

// ---- the mel-cepstrum (include/world_hip.h: world_hip_sp2mc) -------------------------------------------------------------
namespace {
const long double kPiL = 3.14159265358979323846264338327950288L;
// the all-pass phase of omega, alpha in long double
long double mcep_warp(long double omega, long double alpha) {
  return omega + 2.0L * atan2l(alpha * sinl(omega), 1.0L - alpha * cosl(omega));
}
// in-place radix-2 complex FFT of n = re.size() = 2^lg points in long double; (tw_re, tw_im)[j] = exp(-2 pi i j / n), j < n / 2
void fft_ld(std::vector<long double> &re, std::vector<long double> &im, const std::vector<long double> &tw_re,
            const std::vector<long double> &tw_im) {
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; ++i) {                                 // bit reversal
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const size_t step = n / len;
    for (size_t i = 0; i < n; i += len)
      for (size_t j = 0; j < len / 2; ++j) {
        const long double wr = tw_re[j * step], wi = tw_im[j * step];
        const size_t lo = i + j, hi = lo + len / 2;
        const long double tr = re[hi] * wr - im[hi] * wi, ti = re[hi] * wi + im[hi] * wr;
        re[hi] = re[lo] - tr; im[hi] = im[lo] - ti;
        re[lo] += tr; im[lo] += ti;
      }
  }
}
}  // namespace

double mcep_alpha(int fs) {
  if (fs < 1) return NAN;
  constexpr int kPoints = 1000;
  std::vector<long double> mel(kPoints), omega(kPoints), sn(kPoints), cs(kPoints);
  const long double mel_last = logl(1.0L + ((long double)fs / 2000.0L) * (kPoints - 1) / kPoints);
  for (int j = 0; j < kPoints; ++j) {
    mel[j] = logl(1.0L + ((long double)fs / 2000.0L) * j / kPoints) / mel_last;
    omega[j] = kPiL * j / kPoints;
    sn[j] = sinl(omega[j]);
    cs[j] = cosl(omega[j]);
  }
  auto warp = [&](int j, long double alpha) { return omega[j] + 2.0L * atan2l(alpha * sn[j], 1.0L - alpha * cs[j]); };
  int best = 0;
  long double best_sum = 0.0L;
  for (int i = 0; i < kPoints; ++i) {
    const long double alpha = (long double)i / kPoints, last = warp(kPoints - 1, alpha);
    long double sum = 0.0L;
    for (int j = 0; j < kPoints; ++j) {
      const long double d = warp(j, alpha) / last - mel[j];
      sum += d * d;
    }
    if (i == 0 || sum < best_sum) { best = i; best_sum = sum; }
  }
  return (double)best / 1000.0;
}

const char *mcep_shape(int fft_size, int order, double alpha) {
  static thread_local char why[200];
  if (fft_size < 128 || fft_size > 8192 || (fft_size & (fft_size - 1))) {
    snprintf(why, sizeof why, "fft_size %d is not a power of two in [128, 8192]", fft_size);
    return why;
  }
  const int limit = fft_size / 2 < kMcepMaxOrder ? fft_size / 2 : kMcepMaxOrder;
  if (order < 0 || order > limit) { snprintf(why, sizeof why, "order %d outside [0, %d]", order, limit); return why; }
  if (!std::isfinite(alpha) || !(fabs(alpha) <= kMcepMaxAlpha)) {
    snprintf(why, sizeof why, "alpha %g is not finite or beyond +-%g", alpha, kMcepMaxAlpha);
    return why;
  }
  return nullptr;
}

void build_mcep_encode(int fft_size, int order, double alpha_, double *M) {
  const int N = fft_size, H = N / 2, K = H + 1, P = order + 1, half = H / 2;
  const long double alpha = alpha_;
  // cos(pi j / H), j = 0 .. 2 H - 1, from first-quadrant arguments; exactly 0 at the odd multiples of pi / 2
  std::vector<long double> cosT(2 * (size_t)H);
  for (int j = 0; j < 2 * H; ++j) {
    const int r = j > H ? 2 * H - j : j;
    cosT[j] = r == half ? 0.0L : r < half ? cosl(kPiL * r / H) : -cosl(kPiL * (H - r) / H);
  }
  // A [P][K]: freqt of unit vectors, one column after the other (column n needs column n - 1 and its own rows above)
  std::vector<long double> A((size_t)P * K, 0.0L);
  A[0] = 1.0L;
  for (int n = 1; n < K; ++n) {
    A[n] = alpha * A[n - 1];
    if (P > 1) A[(size_t)K + n] = (1.0L - alpha * alpha) * A[n - 1] + alpha * A[(size_t)K + n - 1];
    for (int m = 2; m < P; ++m)
      A[(size_t)m * K + n] = A[(size_t)(m - 1) * K + n - 1] + alpha * (A[(size_t)m * K + n - 1] - A[(size_t)(m - 1) * K + n]);
  }
  // M = A F, F[n][k] = (2 / N) w_n w_k cos(pi n k / H): row m of M is a cosine transform of row m of A.  Laid out evenly
  // around 0 over N points -- z_j = z_(N - j) = A[m][j] -- its DFT is real, Z_k = 2 sum_n w_n A[m][n] cos(pi n k / H), so
  // M[m][k] = w_k Z_k / N; two rows ride one complex transform as its real and imaginary parts.  O(P N log N) long-double
  // operations (milliseconds at 8192 / 255, where the plain product takes ten seconds) and log N roundings per entry.
  std::vector<long double> tw_re(H), tw_im(H), re(N), im(N);
  for (int j = 0; j < H; ++j) {                                           // exp(-2 pi i j / N); sin x = cos(x - pi / 2)
    tw_re[j] = cosT[j];
    tw_im[j] = -cosT[j >= half ? j - half : half - j];
  }
  for (int m = 0; m < P; m += 2) {
    const long double *a0 = &A[(size_t)m * K], *a1 = m + 1 < P ? &A[(size_t)(m + 1) * K] : nullptr;
    for (int j = 0; j <= H; ++j) {
      re[j] = a0[j];
      im[j] = a1 ? a1[j] : 0.0L;
      if (j > 0 && j < H) { re[N - j] = re[j]; im[N - j] = im[j]; }
    }
    fft_ld(re, im, tw_re, tw_im);
    for (int k = 0; k <= H; ++k) {
      const long double wk = k == 0 || k == H ? 0.5L : 1.0L;
      M[(size_t)m * K + k] = (double)(wk * re[k] / N);
      if (a1) M[(size_t)(m + 1) * K + k] = (double)(wk * im[k] / N);
    }
  }
}

void build_mcep_decode(int fft_size, int order, double alpha, double *D) {
  const int H = fft_size / 2, K = H + 1, P = order + 1;
  for (int k = 0; k < K; ++k) {
    const long double warped = mcep_warp(kPiL * k / H, alpha);
    for (int m = 0; m < P; ++m) D[(size_t)k * P + m] = (double)(2.0L * cosl(m * warped));
  }
}

}  // namespace world_hip
