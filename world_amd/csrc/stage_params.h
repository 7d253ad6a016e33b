// stage_params.h -- parameter blocks of the per-frame spectral stages
// (cheaptrick.hip, d4c.hip) and their host launchers.
#pragma once
#include "common.h"

namespace world_hip {

// ---------------------------------------------------------------------------
// Per-frame constants.  gfx950's scalar unit has no FP64: a value that depends on the frame's F0, its position, fs and the
// transform length alone is the same in all threads of the frame's workgroup and still cost a vector instruction in each of
// its wavefronts -- FP64 divisions (15-18 instructions apiece), sincospi pairs.  The launches of the offset scans
// (prepare.h: workgroups of their own behind the scans', one thread per frame) evaluate them ONCE per frame into these
// records; the frame kernels read them at a workgroup-uniform address (scalar loads).  Each expression is written once (prepare.h: ct_frame_consts,
// d4c_frame_consts); a kernel instantiated with REC = false calls the same function itself (the route
// WORLD_HIP_INKERNEL_CONSTS selects: tests/test_gpu_frame_consts.py holds the two to the same bits).
// Only what is uniform and known before the kernel starts: quotients of block sums and per-thread values stay in the kernels.
// A scalar (int, double) of such a record: something an EARLIER kernel wrote and nothing writes while this one runs, read at
// an address that is the same in every thread of the wavefront -- one scalar load, the value in SGPRs.  By itself the
// compiler selects scalar loads only as long as it can prove that nothing has stored to the location since the kernel
// began -- in practice up to the kernel's first LDS traffic; behind that a uniform load becomes a vector load with all 64
// lanes on one address and the value in a VGPR.  Through the constant address space the load is scalar wherever it stands,
// and the compiler still schedules it, merges neighbours and waits for it like any other.
template <class T> __device__ __forceinline__ T uniform_const_load(const T *p) {
#if !defined(WORLD_EMU) && !defined(WORLD_SIMT)
  static_assert(std::is_arithmetic<T>::value, "scalars only");
  return *(const __attribute__((address_space(4))) T *)p;
#else
  return *p;
#endif
}
struct CtFrameRec {
  double cf0;            // ct_effective_f0
  double win_scale;      // 1 / 1.5 / fs * cf0: the window's angle per sample (in units of pi)
  double step_s, step_c; // sincospi(win_scale * threads): the rotation from one of a thread's samples to its next
  double width;          // LinearSmoothing's width, 2/3 cf0 (ct_smooth_shape)
  double origin_axis;    // the smoothing segment's first abscissa
  double f0_over_fs;     // the lifters' argument per quefrency bin
  int hw, origin;        // half window length, the window's centre sample
  int upper, bnd;        // DCCorrection's upper bin; the smoothing segment's boundary bins
};
struct D4cSmoothConsts {   // one LinearSmoothing width of d4c_frame: the two edges' knot offsets and fractions
  double f_lo, f_hi, inv_width;
  int bnd, i_lo, i_hi, pad_;
};
struct D4cFrameRec {
  // d4c_lovetrain: the Blackman window of ratio 3 at max(f0, 40)
  double love_scale, love_step_s, love_step_c;
  int love_hw, love_origin;
  // d4c_frame: the three windows of ratio 4 at cf0 = max(f0, 47) (one length, one angle per sample), DCCorrection's
  // interpolation (the same fraction for every bin) and the smoothings of width cf0 [0] and cf0 / 2 [1]
  double scale, step_s, step_c, fr0;
  int hw, origin[3];     // centres at pos - 0.25 / cf0, pos + 0.25 / cf0, pos
  int upper, b0;
  D4cSmoothConsts sm[2];
};

struct CtParams {
  BatchView b;
  const double *tpos;    // [n_utt][f_stride]
  const double *f0;      // [n_utt][f_stride]
  double *spectrogram;   // [n_utt][f_stride][fft/2+1], or the base of packed records (out_row / out_stride / out_col_bytes)
  const int *out_row;    // nullptr: row of frame (u, f) = u f_stride + f; else out_row[u] + f (records back to back)
  size_t out_stride;     // doubles between consecutive rows (fft/2+1 for the dense layout)
  size_t out_col_bytes;  // bytes from a row's start to this stage's first value (0 for the dense layout)
  int out_f32;           // 1: the row's values are stored as float (the narrow wire format of the multi-GPU exchange)
  unsigned *offsets;     // [n_utt][f_stride] stream position of each frame's first draw
  CtFrameRec *frec;      // [n_utt][f_stride] the frame's constants, written by the offsets' launch (ct_records_utt)
  int frame_consts;      // 1: ct_frame reads frec; 0: it evaluates them itself (WORLD_HIP_INKERNEL_CONSTS)
  int frame_threads;     // threads of a ct_frame workgroup (ct_frame_threads): the window rotation's step
  double lift0;          // the k = 0 lifter, (1 - 2 q1) + 2 q1
  const uint32_t *noise; // randn_value(noise[k]) = k-th randn() of the stream (context-wide table)
  Tables tab;
  double q1;
  double f0_floor;       // GetF0FloorForCheapTrick()
  int lg_fft;            // log2(fft_size)
  // Frame range of the frame kernels: rows of frames [frame_lo, frame_hi) only (the stream positions are those of the
  // whole utterance: ct_prepare always covers every frame).  0 / INT_MAX = all.
  int frame_lo, frame_hi;
  int skip_prepare;      // 1: the offsets of an earlier call with the same shape are still in the workspace
  // Coded records (world_hip_analyze_coded; SURVEY.md 8f.1: the coders "fuse onto K6/K8 outputs"): code_ndim > 0 = the frame
  // kernel writes CodeSpectralEnvelope's first code_ndim coefficients (codec.cpp:268-297) of ITS row instead of the row --
  // the values codec_code_sp would compute from the dense row, bit for bit -- at the row's place in the record.  The tables
  // are the stand-alone coder's (api.hip: codec_tables).
  int code_ndim;
  const int *code_knot;
  const double *code_frac, *code_w_re, *code_w_im;
};

struct D4cParams {
  BatchView b;
  const double *tpos;     // [n_utt][f_stride]
  const double *f0;       // [n_utt][f_stride]
  double *aperiodicity;   // [n_utt][f_stride][fft_out/2+1], or the base of packed records (out_row / out_stride / out_col_bytes)
  const int *out_row;     // as CtParams
  size_t out_stride;
  size_t out_col_bytes;
  int out_f32;
  double *rec;            // packed records' base (column 0 = tpos, 1 = f0), written by d4c_finish; nullptr: dense output
  double *ap0;            // [n_utt][f_stride]  LoveTrain result
  double *coarse;         // [n_utt][f_stride][16] coarse aperiodicity (dB) per band, slot 1 + band
  unsigned *offsets1;     // [n_utt][f_stride]  position of the LoveTrain window within pass 1
  unsigned *draws2;       // [n_utt][f_stride]  draws of the frame's 3 body windows in pass 2 (0: LoveTrain kept the frame out)
  unsigned *draws1;       // [n_utt] total draws of pass 1 (pass 2 continues the stream there)
  D4cFrameRec *frec;      // [n_utt][f_stride] the voiced frames' constants, written by offsets1's launch (d4c_records_utt)
  int frame_consts;       // 1: d4c_lovetrain / d4c_frame read frec and the host's constants below; 0: they evaluate them
  int love_threads, frame_threads;   // threads of a d4c_lovetrain / d4c_frame workgroup: the window rotations' steps
  int love_b[3];          // ceil(100 / 4000 / 7900 Hz * fft_love / fs): LoveTrain's band edges (d4c.cpp:241-249)
  int band_bnd;           // mround(fft_size_d4c * 8 / wl): the bins GetCoarseAperiodicity excludes (d4c.cpp:197)
  const uint32_t *noise;  // randn_value(noise[k]) = k-th randn() of the stream (context-wide table)
  const double *nuttall;  // [wl] NuttallWindow(wl), built on the host
  double *park_ws;        // the 16384-point shape only (96 kHz < fs <= 192 kHz): park_slots slots of N/2 + 2 doubles, one per
  int park_slots;         //   workgroup of a d4c_frame launch (the static group delay does not fit LDS beside that transform)
  Tables tab;
  double threshold;
  int fft_out;            // caller's fft_size (rows have fft_out/2+1 bins)
  int lg_love;            // log2 of the LoveTrain FFT
  int lg_d4c;             // log2 of fft_size_d4c
  int nap;                // number_of_aperiodicities
  int wl;                 // Nuttall window length
  const double *ap_frac;  // [fft_out/2+1] d4c_finish's interpolation onto the caller's bins: the weight s and the upper knot k of
  const int *ap_knot;     //   every bin (GetAperiodicity's interp1 over [0, 3 kHz .., fs/2], d4c.cpp:330-338, :373-375) depend on
                          //   (fs, fft_out) only -- host-built with the kernel's own expressions, cached in the context
  int code_nap;           // > 0: d4c_finish writes CodeAperiodicity's band values (codec.cpp:217-236) of its row instead of the row
  int band_center[8];     // static_cast<int>(3000 (band + 1) fft_size_d4c / fs), d4c.cpp:207-208: the centre bin of band b's slice
                          // (host arithmetic, the reference's expression: in the kernel it was a 20-instruction FP64 division per band)
  // Frame range of d4c_frame / d4c_finish (LoveTrain and the first offset scan always cover every frame: the second
  // pass's stream positions depend on every earlier frame's LoveTrain result).  0 / INT_MAX = all.
  int frame_lo, frame_hi;
  int skip_prepare;       // bits: kD4cSkipScan = offsets1 are in place (an earlier call, or the launch shared with CheapTrick);
                          // kD4cSkipLoveTrain = the LoveTrain pass (ap0, draws2) of an earlier call is still in the workspace
};
constexpr int kD4cSkipScan = 1, kD4cSkipLoveTrain = 2;

void launch_cheaptrick(const CtParams &p, int max_frames, hipStream_t stream);
void launch_d4c(const D4cParams &p, int max_frames, hipStream_t stream);
void launch_spectral_prepare(const CtParams &cp, const D4cParams &dp, int max_frames, hipStream_t stream);   // both stages' F0-only scans
size_t ct_max_draws_per_frame(int fft_size);
size_t d4c_max_draws_per_frame(int fs);
size_t d4c_park_slot_doubles(int lg_d4c);
int ct_frame_threads(int lg_fft);
int d4c_love_threads(int lg_love);
int d4c_frame_threads(int lg_d4c);

}  // namespace world_hip
