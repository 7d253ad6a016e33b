// synthesis.h -- parameter block of the waveform synthesiser (synthesis.hip).
// Reference: Synthesis(), src/synthesis.cpp:339-399.
#pragma once
#include "common.h"

namespace world_hip {

constexpr int kSyThreads = 256;                  // (round 6: one spelling -- tests/emu runs this unit's real workgroups, simt_host.h)
constexpr int kSyPer = 8;                       // consecutive samples per thread in the time-base kernels
constexpr int kSyTile = kSyThreads * kSyPer;    // samples per workgroup

struct SynthParams {
  int n_utt, fs, fft_size, lg_fft;
  double frame_period;      // seconds (the reference divides by 1000 on entry, synthesis.cpp:360,366)
  double lowest_f0;         // fs / fft_size + 1.0 with the reference's integer division (synthesis.cpp:361)
  // Frame j of utterance u is row first_row[u] + j: its rows are sp / ap + row * row_stride (fft_size/2+1 doubles used), its
  // F0 is f0[row * f0_stride].  Dense arrays [n_utt][f_stride](...): first_row[u] = u * f_stride, row_stride = fft_size/2+1,
  // f0_stride = 1.  f64 records read in place (world_hip_synthesis_records, wire 0): the utterance's first record, both
  // strides the record's columns, the three pointers at the record's f0 / sp / ap columns.
  const double *f0;
  const double *sp, *ap;
  const long long *first_row;   // [n_utt] (device)
  size_t row_stride, f0_stride;
  const int *n_frames;      // [n_utt] (device)
  const int *y_len;         // [n_utt] (device)
  double *y;                // [n_utt][y_stride]
  int y_stride;
  // ---- workspace ----
  double *inc;              // [n_utt][y_stride] phase increments, then (in place) the running phase
  unsigned char *flags;     // [n_utt][y_stride] bit0 = interpolated vuv, bit1 = a pulse sits at this sample
  int *blk_cnt;             // [n_utt][nblk] pulses of each tile
  int nblk;
  int *pidx;                // [n_utt][pulse_cap] pulse_locations_index
  double *pshift;           // [n_utt][pulse_cap] pulse_locations_time_shift
  int *np;                  // [n_utt] number_of_pulses (clamped to pulse_cap)
  int pulse_cap;
  int *need;                // context-wide: largest pulse count that did NOT fit pulse_cap (0 = none dropped so far)
  double *resp;             // [n_utt][pulse_cap][resp_stride] impulse response of every pulse (fft_size values)
  int resp_stride;          // fft_size; fft_size + 2 for the 8192-point shape, whose pulse keeps its spectrum there (sy_pulse)
  const double *dc_remover; // [fft_size] GetDCRemover(), host-built
  const uint32_t *noise;    // randn_value(noise[k]) = k-th randn() after reseed
  Tables tab;
};

void launch_synthesis(const SynthParams &p, int max_y, hipStream_t stream);
size_t synth_pulse_lds_bytes(int lg_fft);
int synth_tile_samples();                        // samples one workgroup of the time-base kernels covers (the unit's own constant:
                                                 // callers size their per-tile arrays by asking, not by including it)

// ---- Real-time synthesis (reference src/synthesisrealtime.cpp; the host scheduler is realtime.inc) ----
// One entry per pulse, written by the host when it schedules the pulse: where its two frame rows lie in the stream's frame
// store, how it interpolates between them, and its place in the stream's randn() sequence.
struct RtPulseJob {
  const double *sp0, *sp1, *ap0, *ap1;  // rows of frames floor(t / fp) and floor(t / fp) + 1 (sp1 / ap1 unread when same)
  double wgt;                           // t / fp - floor(t / fp)
  double vuv;                           // the chunk's interpolated V/UV at the pulse (GetCurrentVUV, :230-241)
  uint32_t rng[4];                      // xorshift state at the pulse's first draw (x, y, z, w)
  int noise_size;                       // draws of the pulse, 1 .. fft_size
  int same;                             // floor == ceil: the envelope is the front row alone
  int loc;                              // pulse_locations_index
  int first;                            // first output sample it may touch: the start of the buffer it is rendered into
};
// One stream's part of an overlap-add launch.  Samples [lo, hi): those below final_end are finished and go to out[n - lo],
// the rest stay partial sums in tail_out[n - final_end]; tail_in[n - lo] holds the partial sums of [lo, tail_end).
struct RtOlaStream {
  int p0, np;                           // this stream's pulses in the launch's job list, in pulse order
  int lo, hi, tail_end, final_end;
  const double *tail_in;
  double *tail_out, *out;
};
struct RtParams {
  int fft_size, lg_fft;
  int n_pulses;
  const RtPulseJob *jobs;
  double *resp;                         // [n_pulses][resp_stride]: response, spectrum scratch, noise words
  int resp_stride;                      // rt_resp_stride(fft_size)
  const double *dc_remover;             // [fft_size / 2] GetDCRemover(fft_size / 2) (synthesisrealtime.cpp:428-440)
  const RtOlaStream *ola;
  int n_streams;
  Tables tab;
};
// doubles per pulse: fft_size response values (the 8192-point pulse keeps its spectrum there first: fft_size + 2), then
// fft_size 32-bit noise words
inline int rt_resp_stride(int fft_size) { return fft_size + 2 + fft_size / 2; }
void launch_rt_pulse(const RtParams &p, hipStream_t stream);
void launch_rt_overlap_add(const RtParams &p, int max_span, hipStream_t stream);
// rows [0, n) of src (row_stride doubles apart, nb used) -> frame store rows (first + r) % cap of dst ([cap][nb])
void launch_rt_store_rows(double *dst, int cap, int nb, long long first, const double *src, int row_stride, int n,
                          hipStream_t stream);

}  // namespace world_hip
