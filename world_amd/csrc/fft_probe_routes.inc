// fft_probe_routes.inc -- every composition of fft.h's entry points that a stage kernel runs, each in a kernel of its own:
// one workgroup per transform, HBM in and HBM out, the SAME templates with the SAME template arguments as the caller named
// beside each kernel (tests/test_gpu_fft_routes.py holds the table and checks it against the call sites).  Included by
// fft_probe.hip (the shipped slot swizzle) and by fft_probe_swz1.hip (d4c.hip's).  Every kernel carries the swizzle map as
// its first template argument: the two units' kernels are different functions for the linker and different labels in a profile.
//   real rows [batch][N], spectra [batch][N/2+1][2], plain complex rows [batch][N][2]
#include "common.h"
#include "fft_probe.h"

namespace world_hip {

__device__ __forceinline__ void fp_load_real(cplx *Z, const double *x, int N) {     // two samples per 16-byte slot
  for (int i = threadIdx.x; i < N / 2; i += blockDim.x) { cplx v; v.re = x[2 * i]; v.im = x[2 * i + 1]; Z[swz(i)] = v; }
}
__device__ __forceinline__ void fp_store_real(const cplx *Z, double *y, int N) {
  for (int i = threadIdx.x; i < N / 2; i += blockDim.x) { const cplx v = Z[swz(i)]; y[2 * i] = v.re; y[2 * i + 1] = v.im; }
}
__device__ __forceinline__ cplx fp_cplx(double2 v) { cplx c; c.re = v.x; c.im = v.y; return c; }

// r2c: X[k] = sum x[n] e^{-2 pi i k n / N}.  tw_lg = lgn - 1: the inner transform's table, the merge takes the fine twiddle
// (ct_frame, hv_band_spectra, d4c_lovetrain); tw_lg = lgn: the table the coders stage (codec_code_sp, ct_frame_coded)
template <int SWZ, int MAXLR, int LGN = 0>
__global__ void fft_route_rfft(const double *in, double2 *out, int lgn, int tw_lg, const double2 *tw_global) {
  DYN_LDS(lds);
  const int N = 1 << lgn;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(lds) + N, tw_lg, tw_global);
  double2 *X = out + (size_t)blockIdx.x * (N / 2 + 1);
  fp_load_real(Z, in + (size_t)blockIdx.x * N, N);
  block_rfft<MAXLR, LGN>(Z, lgn, tw, [&](int k, double re, double im) { X[k] = make_double2(re, im); });
}

// c2r, unscaled (N * irfft, imaginary parts of DC / Nyquist ignored)
template <int SWZ, int MAXLR, int LGN = 0>
__global__ void fft_route_irfft(const double2 *spec, double *out, int lgn, const double2 *tw_global) {
  DYN_LDS(lds);
  const int N = 1 << lgn;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(lds) + N, lgn - 1, tw_global);
  const double2 *X = spec + (size_t)blockIdx.x * (N / 2 + 1);
  block_irfft<MAXLR, LGN>(Z, lgn, tw, [&](int k) { return fp_cplx(X[k]); });
  fp_store_real(Z, out + (size_t)blockIdx.x * N, N);
}

// r2c with the first stage fed by a functor (minimum_phase and the noise spectrum of synthesis.hip, ct_frame's lifter)
template <int SWZ, int MAXLR, int LGN = 0>
__global__ void fft_route_rfft_from(const double *in, double2 *out, int lgn, const double2 *tw_global) {
  DYN_LDS(lds);
  const int N = 1 << lgn;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(lds) + N, lgn - 1, tw_global);
  const double *x = in + (size_t)blockIdx.x * N;
  double2 *X = out + (size_t)blockIdx.x * (N / 2 + 1);
  block_rfft_from<MAXLR, LGN>(Z, lgn, tw, [&](int n) { cplx v; v.re = x[2 * n]; v.im = x[2 * n + 1]; return v; },
                              [&](int k, double re, double im) { X[k] = make_double2(re, im); });
}

// plain complex forward transform, default plan, the table at the transform's own resolution (decode_sp_row)
template <int SWZ>
__global__ void fft_route_cfft(const double2 *in, double2 *out, int lgn, const double2 *tw_global) {
  DYN_LDS(lds);
  const int N = 1 << lgn;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(lds) + 2 * N, lgn, tw_global);
  const double2 *x = in + (size_t)blockIdx.x * N;
  double2 *X = out + (size_t)blockIdx.x * N;
  for (int i = threadIdx.x; i < N; i += blockDim.x) Z[swz(i)] = fp_cplx(x[i]);
  const FftPlan plan = make_plan(lgn);
  block_cfft_dif(Z, plan, tw);
  for (int k = threadIdx.x; k < N; k += blockDim.x) { const cplx v = Z[fft_slot(plan, k)]; X[k] = make_double2(v.re, v.im); }
}

// N-point complex transform of a row that is zero beyond element N/2, the first stage fed by a functor, the table one level
// coarser than the transform (minimum_phase: the cepstrum's causal half)
template <int SWZ>
__global__ void fft_route_cfft_from(const double2 *in, double2 *out, int lgn, const double2 *tw_global) {
  DYN_LDS(lds);
  const int N = 1 << lgn, H = N / 2;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(lds) + 2 * N, lgn - 1, tw_global);
  const double2 *x = in + (size_t)blockIdx.x * N;
  double2 *X = out + (size_t)blockIdx.x * N;
  const FftPlan plan = make_plan_max(lgn, 3);
  block_cfft_dif_from<3>(Z, plan, tw, [&](int j) { cplx z; z.re = 0.0; z.im = 0.0; return j <= H ? fp_cplx(x[j]) : z; });
  for (int k = threadIdx.x; k < N; k += blockDim.x) { const cplx v = Z[fft_slot(plan, k)]; X[k] = make_double2(v.re, v.im); }
}

// dft8 / dft8_head2 (d4c_frame's pruned first stage) on rows of 8 complex values; head2 reads the first two
template <int SWZ, bool HEAD2>
__global__ void fft_route_dft8(const double2 *in, double2 *out, int rows) {
  const int row = flat_thread_x();
  if (row >= rows) return;
  cplx a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = fp_cplx(in[(size_t)row * 8 + j]);
  if (HEAD2) dft8_head2<true>(a[0], a[1], a); else dft8<true>(a);
#pragma unroll
  for (int j = 0; j < 8; ++j) out[(size_t)row * 8 + j] = make_double2(a[j].re, a[j].im);
}

#ifndef WORLD_EMU
// ---- compositions whose workgroup size is a template constant (T threads exactly) --------------------------------------
// the static complex transform, then the merge over natural-order items, the table at lgn - 1.
//   ROT = false: rfft_merge_items, twiddles from the table (hv_block_spectra)
//   ROT = true : rfft_merge_items_w<.., TWICE = true> with the twiddles wbase W16^m (d4c_lovetrain's 4096-point shape): 2 X[k]
template <int SWZ, int LGN, int T, bool ROT>
__global__ void __launch_bounds__(T) fft_route_rfft_items(const double *in, double2 *out, const double2 *tw_global) {
  DYN_LDS(lds);
  constexpr int N = 1 << LGN, h = N / 2, kItems = (N / 4 + 1 + T - 1) / T;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(lds) + N, LGN - 1, tw_global);
  double2 *X = out + (size_t)blockIdx.x * (h + 1);
  fp_load_real(Z, in + (size_t)blockIdx.x * N, N);
  constexpr FftPlan plan = make_plan_max(LGN - 1, 3);
  block_cfft_dif_static<LGN - 1, 3, T>(Z, tw);
  auto emit = [&](int, int k, double ar, double ai, bool paired, double br, double bi) {
    X[k] = make_double2(ar, ai);
    if (paired) X[h - k] = make_double2(br, bi);
  };
  if constexpr (ROT) {
    const cplx wb = twiddle(tw, wg_thread<T>(), LGN, -1);
    rfft_merge_items_w<kItems, T, true>(Z, LGN, plan, [&](int m, int) { return mul_w16_fwd(wb, m); }, emit);
  } else {
    rfft_merge_items<kItems, T>(Z, LGN, plan, tw, emit);
  }
}

// the pre-twiddle over natural-order items, then the static inverse transform (hv_band_events_fft).
//   ROT = true : irfft_pretwiddle_items_w with the twiddles conj(wbase W16^m)
//   ROT = false: irfft_pretwiddle_items, twiddles from the table (fft.h promises irfft_pretwiddle's values)
template <int SWZ, int LGN, int T, bool ROT>
__global__ void __launch_bounds__(T) fft_route_irfft_items(const double2 *spec, double *out, const double2 *tw_global) {
  DYN_LDS(lds);
  constexpr int N = 1 << LGN, hh = N / 2, kItems = (N / 4 + 1 + T - 1) / T;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(lds) + N, LGN - 1, tw_global);
  const double2 *X = spec + (size_t)blockIdx.x * (hh + 1);
  constexpr FftPlan plan = make_plan_max(LGN - 1, 3);
  if constexpr (ROT) {
    const cplx wbf = twiddle(tw, wg_thread<T>(), LGN, -1);
    irfft_pretwiddle_items_w<kItems, T>(Z, LGN, plan, [&](int m, int k, cplx &x, cplx &y, cplx &wk) {
      x = fp_cplx(X[k]); y = fp_cplx(X[hh - k]);
      wk = cconj(mul_w16_fwd(wbf, m));
    });
  } else {
    irfft_pretwiddle_items<kItems, T>(Z, LGN, plan, tw, [&](int k) { return fp_cplx(X[k]); });
  }
  block_cfft_dit_static<LGN - 1, 3, T>(Z, tw);
  fp_store_real(Z, out + (size_t)blockIdx.x * N, N);
}

// d4c_frame's staging -- the quarter-wave table two levels coarser than the merge asks for, direct tables for the two inner
// radix-8 stages on top of it -- and its transform: static stages on T = N / 16 threads, merge twiddles by rotation.
// LDS (doubles): Z (N) | quarter-wave table (2^(lgn-4) + 2) | direct twiddles (2^(lgn-7) + 2^(lgn-10) complex)
constexpr int kFpD4cTwLevel = 2;                               // d4c.hip: D4C_TW_LEVEL
__host__ __device__ __forceinline__ size_t fp_d4c_direct_offset(int lgn) {
  return sizeof(double) * (((size_t)1 << lgn) + twiddle_lds_doubles(lgn - kFpD4cTwLevel));
}
__host__ __device__ __forceinline__ size_t fp_d4c_lds_bytes(int lgn) {
  return fp_d4c_direct_offset(lgn) + sizeof(cplx) * (((size_t)1 << (lgn - 7)) + ((size_t)1 << (lgn - 10)));
}
template <int NMAX, int T>
__device__ __forceinline__ TwLds fp_d4c_stage(char *lds, const double2 *tw_global, TwLds *plain) {
  constexpr int lgn = const_log2(NMAX);
  const TwLds coarse = stage_twiddles<T>(reinterpret_cast<double *>(lds) + NMAX, lgn - kFpD4cTwLevel, tw_global);
  if (plain) *plain = coarse;
  return stage_direct_twiddles<T>(coarse, reinterpret_cast<cplx *>(lds + fp_d4c_direct_offset(lgn)),
                                  lgn - 1 - 3, 1 << (lgn - 1 - 6), lgn - 1 - 6, 1 << (lgn - 1 - 9));
}
// KIND 0: rfft_merge_items_rot<kItems, T>; 1: <kItems, T, true> (2 X[k]); 2: KIND 0 behind the run-time plan's stages
template <int SWZ, int NMAX, int T, int KIND>
__global__ void __launch_bounds__(T) fft_route_d4c_rfft(const double *in, double2 *out, const double2 *tw_global) {
  DYN_LDS(lds);
  constexpr int lgn = const_log2(NMAX), N = NMAX, H = N / 2, kItems = (N / 4 + 1 + T - 1) / T;
  cplx *Z = reinterpret_cast<cplx *>(lds);
  const TwLds tw = fp_d4c_stage<NMAX, T>(lds, tw_global, nullptr);
  double2 *X = out + (size_t)blockIdx.x * (H + 1);
  fp_load_real(Z, in + (size_t)blockIdx.x * N, N);
  constexpr FftPlan plan = make_plan_max(lgn - 1, 3);
  if constexpr (KIND == 2) block_cfft_dif<3>(Z, plan, tw);
  else block_cfft_dif_static<lgn - 1, 3, T>(Z, tw);
  const cplx wb = twiddle(tw, wg_thread<T>(), lgn, -1);
  auto emit = [&](int, int k, double ar, double ai, bool paired, double br, double bi) {
    X[k] = make_double2(ar, ai);
    if (paired) X[H - k] = make_double2(br, bi);
  };
  if constexpr (KIND == 1) rfft_merge_items_rot<kItems, T, true>(Z, lgn, plan, tw, wb, emit);
  else rfft_merge_items_rot<kItems, T>(Z, lgn, plan, tw, wb, emit);
}
// the twiddles that staging serves, as one complex row of N values e^{-2 pi i k / 2^level}:
//   [0, N/128)            level lgn - 4 from the direct table      [N/4, N/4 + N/128)         the same by twiddle() on the plain table
//   [N/128, N/128+N/1024) level lgn - 7 from the direct table      [N/4 + N/128, .. + N/1024) the same by twiddle()
//   [3N/8, 3N/8 + N/16)   level lgn - 1 (one level finer than the table: the first stage's)
//   [N/2, N)              level lgn     (two levels finer: the merge's), k < N/2;          everything else 0
template <int SWZ, int NMAX, int T>
__global__ void __launch_bounds__(T) fft_route_d4c_twiddles(double2 *out, const double2 *tw_global) {
  DYN_LDS(lds);
  constexpr int lgn = const_log2(NMAX), N = NMAX, n_a = N >> 7, n_b = N >> 10;
  TwLds plain;
  const TwLds tw = fp_d4c_stage<NMAX, T>(lds, tw_global, &plain);
  __syncthreads();                                             // publishes the direct tables
  double2 *X = out + (size_t)blockIdx.x * N;
  for (int i = wg_thread<T>(); i < N; i += T) {
    cplx v; v.re = 0.0; v.im = 0.0;
    if (i < n_a) v = twiddle(tw, i, lgn - 4, -1);
    else if (i < n_a + n_b) v = twiddle(tw, i - n_a, lgn - 7, -1);
    else if (i >= N / 4 && i < N / 4 + n_a) v = twiddle(plain, i - N / 4, lgn - 4, -1);
    else if (i >= N / 4 + n_a && i < N / 4 + n_a + n_b) v = twiddle(plain, i - N / 4 - n_a, lgn - 7, -1);
    else if (i >= 3 * N / 8 && i < 3 * N / 8 + N / 16) v = twiddle(tw, i - 3 * N / 8, lgn - 1, -1);
    else if (i >= N / 2) v = twiddle(tw, i - N / 2, lgn, -1);
    X[i] = make_double2(v.re, v.im);
  }
}
#endif  // !WORLD_EMU

// ---- the launcher of this unit's share of the table ---------------------------------------------------------------------
#define FP_BLOCKS(kernel, ...) WH_BLOCKS(kernel, __VA_ARGS__)       // (expands WH_SWZ inside the label)
#define FP_THREADS(kernel, ...) WH_THREADS(kernel, __VA_ARGS__)
#define FP_NAME2(n) launch_fft_routes_swz##n
#define FP_NAME(n) FP_NAME2(n)

// false: the unit has no such composition (the caller names what is supported)
bool FP_NAME(WH_SWZ)(int mode, int lgn, int max_lr, int threads, long batch, const void *d_in, void *d_out, const Tables &tab,
                     hipStream_t stream) {
  // what the units' stage kernels run: d4c.hip the LoveTrain transforms, d4c_frame's route and its pruned radix-8 butterfly;
  // everybody else the rest (dft8 itself is every radix-8 plan's)
#if WH_SWZ == 1
  if (mode < kFpRfftRotTwice && !(mode == kFpRfft && max_lr == 3) && !(mode == kFpRfftStatic && lgn == 11)) return false;
#else
  if (mode >= kFpRfftRotTwice && mode <= kFpD4cTwiddles) return false;
#endif
  if (lgn < 3 || lgn > kTwLog2) return false;
  const dim3 grid((unsigned)batch);
  const size_t N = (size_t)1 << lgn;
  const size_t lds_real = sizeof(double) * (N + twiddle_lds_doubles(lgn - 1));
  const double *rin = static_cast<const double *>(d_in);
  double *rout = static_cast<double *>(d_out);
  const double2 *cin = static_cast<const double2 *>(d_in);
  double2 *cout = static_cast<double2 *>(d_out);
  const bool run_time_size = threads >= 64 && threads <= 1024 && threads % 64 == 0;
  switch (mode) {
    case kFpRfft:
      if (!run_time_size || lgn < 6 || lgn > kTwLog2) return false;
      if (max_lr == 3) FP_BLOCKS((fft_route_rfft<WH_SWZ, 3>), grid, threads, lds_real, stream, rin, cout, lgn, lgn - 1, tab.tw);
      else if (max_lr == 4) FP_BLOCKS((fft_route_rfft<WH_SWZ, 4>), grid, threads, lds_real, stream, rin, cout, lgn, lgn - 1, tab.tw);
      else return false;
      return true;
    case kFpRfftFullTable:
      if (!run_time_size || lgn < 6 || lgn > kTwLog2 - 1 || max_lr != 4) return false;
      FP_BLOCKS((fft_route_rfft<WH_SWZ, 4>), grid, threads, sizeof(double) * (N + twiddle_lds_doubles(lgn)), stream, rin, cout, lgn, lgn, tab.tw);
      return true;
    case kFpIrfft:
      if (!run_time_size || lgn < 6 || lgn > kTwLog2) return false;
      if (max_lr == 3) FP_BLOCKS((fft_route_irfft<WH_SWZ, 3>), grid, threads, lds_real, stream, cin, rout, lgn, tab.tw);
      else if (max_lr == 4) FP_BLOCKS((fft_route_irfft<WH_SWZ, 4>), grid, threads, lds_real, stream, cin, rout, lgn, tab.tw);
      else return false;
      return true;
    case kFpRfftFrom:
      if (!run_time_size || lgn < 6 || lgn > kTwLog2 || max_lr != 3) return false;
      FP_BLOCKS((fft_route_rfft_from<WH_SWZ, 3>), grid, threads, lds_real, stream, rin, cout, lgn, tab.tw);
      return true;
    case kFpCfft:
      if (!run_time_size || lgn < 6 || lgn > kTwLog2 - 1 || max_lr != 4) return false;
      FP_BLOCKS((fft_route_cfft<WH_SWZ>), grid, threads, sizeof(double) * (2 * N + twiddle_lds_doubles(lgn)), stream, cin, cout, lgn, tab.tw);
      return true;
    case kFpCfftFrom:
      if (!run_time_size || lgn < 6 || lgn > kTwLog2 - 1 || max_lr != 3) return false;
      FP_BLOCKS((fft_route_cfft_from<WH_SWZ>), grid, threads, sizeof(double) * (2 * N + twiddle_lds_doubles(lgn - 1)), stream, cin, cout, lgn, tab.tw);
      return true;
    case kFpDft8:
    case kFpDft8Head2:
      if (lgn != 3) return false;
      if (mode == kFpDft8) FP_THREADS((fft_route_dft8<WH_SWZ, false>), batch, 1, 1, stream, cin, cout, (int)batch);
      else FP_THREADS((fft_route_dft8<WH_SWZ, true>), batch, 1, 1, stream, cin, cout, (int)batch);
      return true;
    default: break;
  }
#ifndef WORLD_EMU
  if (max_lr != 3) return false;
  // the length a compile-time constant, the workgroup size still the launch's (ct_frame 1024 .. 4096; d4c_lovetrain 2048)
  if (run_time_size && (mode == kFpRfftStatic || mode == kFpIrfftStatic || mode == kFpRfftFromStatic)) {
#define FP_STATIC(LG) \
    if (lgn == LG && mode == kFpRfftStatic) { FP_BLOCKS((fft_route_rfft<WH_SWZ, 3, LG>), grid, threads, lds_real, stream, rin, cout, lgn, lgn - 1, tab.tw); return true; } \
    if (lgn == LG && mode == kFpIrfftStatic) { FP_BLOCKS((fft_route_irfft<WH_SWZ, 3, LG>), grid, threads, lds_real, stream, cin, rout, lgn, tab.tw); return true; } \
    if (lgn == LG && mode == kFpRfftFromStatic) { FP_BLOCKS((fft_route_rfft_from<WH_SWZ, 3, LG>), grid, threads, lds_real, stream, rin, cout, lgn, tab.tw); return true; }
    FP_STATIC(10) FP_STATIC(11) FP_STATIC(12)
#undef FP_STATIC
    return false;
  }
  // 4096 points on 256 threads: Harvest's filter bank and the LoveTrain pass
  if (lgn == 12 && threads == 256) {
    if (mode == kFpRfftItems) { FP_BLOCKS((fft_route_rfft_items<WH_SWZ, 12, 256, false>), grid, 256, lds_real, stream, rin, cout, tab.tw); return true; }
    if (mode == kFpRfftRotTwice) { FP_BLOCKS((fft_route_rfft_items<WH_SWZ, 12, 256, true>), grid, 256, lds_real, stream, rin, cout, tab.tw); return true; }
    if (mode == kFpIrfftItems) { FP_BLOCKS((fft_route_irfft_items<WH_SWZ, 12, 256, false>), grid, 256, lds_real, stream, cin, rout, tab.tw); return true; }
    if (mode == kFpIrfftItemsRot) { FP_BLOCKS((fft_route_irfft_items<WH_SWZ, 12, 256, true>), grid, 256, lds_real, stream, cin, rout, tab.tw); return true; }
  }
  // d4c_frame's four shapes: N / 16 threads
  if (lgn >= 11 && lgn <= 14 && threads == (1 << (lgn - 4))) {
    const size_t lds = fp_d4c_lds_bytes(lgn);
#define FP_D4C(NMAX, T) \
    if (N == NMAX && mode == kFpD4cRfft) { FP_BLOCKS((fft_route_d4c_rfft<WH_SWZ, NMAX, T, 0>), grid, threads, lds, stream, rin, cout, tab.tw); return true; } \
    if (N == NMAX && mode == kFpD4cRfftTwice) { FP_BLOCKS((fft_route_d4c_rfft<WH_SWZ, NMAX, T, 1>), grid, threads, lds, stream, rin, cout, tab.tw); return true; } \
    if (N == NMAX && mode == kFpD4cRfftRunTime) { FP_BLOCKS((fft_route_d4c_rfft<WH_SWZ, NMAX, T, 2>), grid, threads, lds, stream, rin, cout, tab.tw); return true; } \
    if (N == NMAX && mode == kFpD4cTwiddles) { FP_BLOCKS((fft_route_d4c_twiddles<WH_SWZ, NMAX, T>), grid, threads, lds, stream, cout, tab.tw); return true; }
    FP_D4C(2048, 128) FP_D4C(4096, 256) FP_D4C(8192, 512) FP_D4C(16384, 1024)
#undef FP_D4C
  }
#endif
  return false;
}

}  // namespace world_hip
