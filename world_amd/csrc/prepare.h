// prepare.h -- where each frame's noise sits in the reference's one randn() stream: exclusive prefix sums
// of the per-frame draw counts, one workgroup per utterance.  CheapTrick's scan and D4C's first (the LoveTrain windows)
// follow from F0 alone, so one launch serves both stages of a job (spectral_prepare, d4c.hip); D4C's second pass depends on
// the LoveTrain result: d4c_lovetrain leaves each frame's draw count, and a d4c_frame workgroup sums those of the frames
// before its own (d4c.hip).
#pragma once
#include "stage_params.h"

namespace world_hip {

// cheaptrick.cpp:218.  An F0 above fs/2 (no estimator produces one; a caller-made track can) is analysed as fs/2: the frame
// kernel's smoothing segment is laid out for widths up to 2/3 of that (ct_seg_cap) and a wider one would run over the
// next LDS region -- the one place this path does not follow the reference, which has no such bound.
// A NaN F0 (undefined behaviour in the reference: it becomes a window length through a double -> int conversion,
// cheaptrick.cpp:95) is analysed like an unvoiced frame -- `!(f0 > floor)` instead of `f0 <= floor`.
__device__ __forceinline__ double ct_effective_f0(double f0, double floor_f0, int fs) {
  const double nyq = 0.5 * fs;
  return !(f0 > floor_f0) ? kDefaultF0 : (f0 > nyq ? nyq : f0);
}
// D4C's view of a caller-made F0: NaN counts as 0 (an unvoiced frame: the row is 1 - 1e-12), values above fs/2 as fs/2.
// The reference indexes its spectra with 2 + int(f0 fft_size / fs) (common.cpp:60-62: beyond the arrays from about fs/2
// on) and turns NaN into a window length (d4c.cpp:55-56): both are undefined there; here every window length, stream
// offset and LDS index stays inside what the launch allocated.  Negative and -Inf values take the reference's own
// route (its floors of 40 and 47 Hz apply: d4c.cpp:263, :300).
__device__ __forceinline__ double d4c_sane_f0(double f0, int fs) {
  const double nyq = 0.5 * fs;
  return f0 != f0 ? 0.0 : (f0 > nyq ? nyq : f0);
}

// ---- the frames' uniform constants (stage_params.h: CtFrameRec, D4cFrameRec) ------------------------------------------
// Every expression is written here once, as a function of (F0, position, fs, N): the scans' launches evaluate it once per
// frame (ct_records_utt, d4c_records_utt), a frame kernel of the in-kernel route (REC = false) evaluates it in every thread -- the same IEEE operations on
// the same operands either way.  `nt`: the threads of the consuming kernel's workgroup (a thread's samples are nt apart).

// LinearSmoothing's geometry for one CheapTrick frame (common.cpp:27-50): boundary bins and segment length
struct CtSmooth { double width; int bnd, seg_len; };
__device__ __forceinline__ CtSmooth ct_smooth_shape(double cf0, int N, int fs) {
  CtSmooth s;
  s.width = cf0 * 2.0 / 3.0;
  s.bnd = static_cast<int>(s.width * N / fs) + 1;
  s.seg_len = N / 2 + 2 * s.bnd + 1;
  return s;
}
__device__ __forceinline__ int ct_win_half(int fs, double cf0) { return mround(1.5 * fs / cf0); }     // cheaptrick.cpp:95
__device__ __forceinline__ CtFrameRec ct_frame_consts(double cf0, double pos, int fs, int N, int nt) {
  CtFrameRec r;
  r.cf0 = cf0;
  r.hw = ct_win_half(fs, cf0);
  r.origin = mround(pos * fs + 0.001);
  r.win_scale = 1.0 / 1.5 / fs * cf0;                       // position * f0 = (i - hw) / 1.5 / fs * f0
  sincospi(r.win_scale * nt, &r.step_s, &r.step_c);
  r.upper = 2 + static_cast<int>(cf0 * N / fs);             // DCCorrection, common.cpp:60
  const CtSmooth sm = ct_smooth_shape(cf0, N, fs);
  r.width = sm.width;
  r.bnd = sm.bnd;
  r.origin_axis = -(sm.bnd - 0.5) * fs / N;
  r.f0_over_fs = cf0 / fs;
  return r;
}

// GetWindowedWaveform's geometry in D4C (d4c.cpp:52-60): half length, centre sample and angle per sample of a window of
// `ratio` periods of f0 at time pos
__device__ __forceinline__ int d4c_win_half(double ratio, int fs, double f0) { return mround(ratio * fs / f0 / 2.0); }
__device__ __forceinline__ int d4c_win_origin(double pos, int fs) { return mround(pos * fs + 0.001); }
__device__ __forceinline__ double d4c_win_scale(double ratio, int fs, double f0) { return 2.0 / ratio / fs * f0; }
// LinearSmoothing (common.cpp:27-111) in d4c_frame: interp1Q of the prefix sums at k fs / N -+ width / 2 is, on the
// segment's axis, position k + c_lo and k + c_hi with c_lo = bnd - 0.5 - r / 2, c_hi = c_lo + r (r = width N / fs) -- the
// fractions are the same for EVERY bin and the knot indices are k plus a constant
__device__ __forceinline__ D4cSmoothConsts d4c_smooth_consts(double width, int N, int fs) {
  D4cSmoothConsts s;
  s.bnd = static_cast<int>(width * N / fs) + 1;
  const double origin_axis = -(s.bnd - 0.5) * fs / N;
  const double inv_step = static_cast<double>(N) / fs;
  s.inv_width = 1.0 / width;
  const double c_lo = (0.0 - width / 2.0 - origin_axis) * inv_step, c_hi = (width / 2.0 - origin_axis) * inv_step;
  s.i_lo = static_cast<int>(c_lo); s.i_hi = static_cast<int>(c_hi);
  s.f_lo = c_lo - s.i_lo; s.f_hi = c_hi - s.i_hi;
  s.pad_ = 0;
  return s;
}
// d4c_lovetrain's part: f0 is d4c_sane_f0's value of a voiced frame, M-independent
__device__ __forceinline__ void d4c_love_consts(D4cFrameRec &r, double f0, double pos, int fs, int nt) {
  const double cf0 = f0 > 40.0 ? f0 : 40.0;                           // d4c.cpp:263,279
  r.love_hw = d4c_win_half(3.0, fs, cf0);
  r.love_origin = d4c_win_origin(pos, fs);
  r.love_scale = d4c_win_scale(3.0, fs, cf0);
  sincospi(r.love_scale * nt, &r.love_step_s, &r.love_step_c);
}
// d4c_frame's part (N = fft_size_d4c)
__device__ __forceinline__ void d4c_body_consts(D4cFrameRec &r, double f0, double pos, int fs, int N, int nt) {
  const double cf0 = kFloorF0D4C > f0 ? kFloorF0D4C : f0;
  r.hw = d4c_win_half(4.0, fs, cf0);                                  // d4c.cpp:97,101,155: one length, one angle per sample
  r.scale = d4c_win_scale(4.0, fs, cf0);
  sincospi(r.scale * nt, &r.step_s, &r.step_c);
  r.origin[0] = d4c_win_origin(pos - 0.25 / cf0, fs);
  r.origin[1] = d4c_win_origin(pos + 0.25 / cf0, fs);
  r.origin[2] = d4c_win_origin(pos, fs);
  // DCCorrection (common.cpp:56-75): interp1Q at k fs / N on the axis cf0 - j fs / N is position cf0 N / fs - k
  r.upper = 2 + static_cast<int>(cf0 * N / fs);
  const double pos0 = (0.0 - cf0) * (-static_cast<double>(N) / fs);
  r.b0 = static_cast<int>(pos0);
  r.fr0 = pos0 - r.b0;
  r.sm[0] = d4c_smooth_consts(cf0, N, fs);
  r.sm[1] = d4c_smooth_consts(cf0 / 2.0, N, fs);
}

// The records of frames [chunk kRecSpan, (chunk + 1) kRecSpan) of utterance u, one frame per thread.  Workgroups of their
// own beside the scans' (the grids' tails: ct_prepare, d4c_prepare1, spectral_prepare): inside the scan loops, which one
// workgroup per utterance walks, the records' divisions and sincospi pairs tripled the launch's duration (7.5 -> 20.6 us
// for a 10 s utterance) -- more than the frame kernels of a lone job gained.
constexpr int kRecSpan = 256;
__device__ __forceinline__ void ct_records_utt(const CtParams &p, int u, int chunk) {
  const int nf = p.b.n_frames[u], hi = imin(nf, (chunk + 1) * kRecSpan);
  for (int f = chunk * kRecSpan + threadIdx.x; f < hi; f += blockDim.x) {
    const size_t fi = (size_t)u * p.b.f_stride + f;
    p.frec[fi] = ct_frame_consts(ct_effective_f0(p.f0[fi], p.f0_floor, p.b.fs), p.tpos[fi], p.b.fs, 1 << p.lg_fft, p.frame_threads);
  }
}
__device__ __forceinline__ void d4c_records_utt(const D4cParams &p, int u, int chunk) {
  const int nf = p.b.n_frames[u], hi = imin(nf, (chunk + 1) * kRecSpan);
  for (int f = chunk * kRecSpan + threadIdx.x; f < hi; f += blockDim.x) {
    const size_t fi = (size_t)u * p.b.f_stride + f;
    const double f0f = d4c_sane_f0(p.f0[fi], p.b.fs);
    if (f0f == 0.0) continue;                 // an unvoiced frame has no record: d4c_lovetrain and d4c_frame leave before they would read it
    const double pos = p.tpos[fi];
    D4cFrameRec r;
    d4c_love_consts(r, f0f, pos, p.b.fs, p.love_threads);
    d4c_body_consts(r, f0f, pos, p.b.fs, 1 << p.lg_d4c, p.frame_threads);
    p.frec[fi] = r;
  }
}
__host__ __device__ __forceinline__ int rec_chunks(int max_frames) { return (max_frames + kRecSpan - 1) / kRecSpan; }

// CheapTrick: window draws, then one per bin (cheaptrick.cpp:27-43, :147-149)
__device__ __forceinline__ void ct_offsets_utt(const CtParams &p, int u, double *scratch) {
  const int nf = p.b.n_frames[u];
  const int N = 1 << p.lg_fft, nb = N / 2 + 1;
  const double *f0 = p.f0 + (size_t)u * p.b.f_stride;
  unsigned *off_out = p.offsets + (size_t)u * p.b.f_stride;
  unsigned running = 0;
  for (int base = 0; base < nf; base += blockDim.x) {
    int f = base + threadIdx.x;
    int cnt = 0;
    if (f < nf) {
      double cf0 = ct_effective_f0(f0[f], p.f0_floor, p.b.fs);
      cnt = 2 * ct_win_half(p.b.fs, cf0) + 1 + nb;
    }
    int total, off = block_excl_scan_int(cnt, &total, scratch);
    if (f < nf) off_out[f] = running + (unsigned)off;
    running += (unsigned)total;
  }
}

// D4C pass 1: the LoveTrain window of every voiced frame (d4c.cpp:263-279)
__device__ __forceinline__ void d4c_offsets1_utt(const D4cParams &p, int u, double *scratch) {
  const int nf = p.b.n_frames[u];
  const double *f0 = p.f0 + (size_t)u * p.b.f_stride;
  unsigned *off_out = p.offsets1 + (size_t)u * p.b.f_stride;
  unsigned running = 0;
  for (int base = 0; base < nf; base += blockDim.x) {
    int f = base + threadIdx.x, cnt = 0;
    const double f0f = f < nf ? d4c_sane_f0(f0[f], p.b.fs) : 0.0;
    if (f < nf && f0f != 0.0) {
      double cf0 = f0f > 40.0 ? f0f : 40.0;                          // d4c.cpp:263,279
      cnt = 2 * d4c_win_half(3.0, p.b.fs, cf0) + 1;
    }
    int total, off = block_excl_scan_int(cnt, &total, scratch);
    if (f < nf) off_out[f] = running + (unsigned)off;
    running += (unsigned)total;
  }
  if (threadIdx.x == 0) p.draws1[u] = running;
}

}  // namespace world_hip
