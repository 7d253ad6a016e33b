// tables.cpp -- host construction of the twiddle and RNG jump-ahead tables, and the resampler's host arithmetic.
#include "tables.h"
#include "resample_host.h"

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

}  // namespace world_hip
