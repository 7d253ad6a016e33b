/*
 * world_hip.h -- C ABI of libworld_hip.so, the MI355X (gfx950) implementation of
 * the WORLD analysis path.
 *
 * Part 1 is the drop-in boundary: the 13 `extern "C"` analysis entry points and 4
 * option structs of mmorise/World with identical names, layouts and argument
 * meaning (host pointers, caller-owned buffers, `double **` row pointers for the
 * spectrogram / aperiodicity).  Each declaration cites the reference header it
 * replaces.  A program written against libworld.a links against libworld_hip.so
 * unchanged for these symbols.
 *
 * Part 2 is the batched, device-resident API the drop-in calls are built on:
 * many utterances per call, inputs and outputs in HBM (plain device pointers, no
 * framework types), one HIP stream, no host synchronisation inside a call.
 */
#ifndef WORLD_HIP_H_
#define WORLD_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define WORLD_HIP_API __attribute__((visibility("default")))
#else
#define WORLD_HIP_API
#endif

/* ------------------------------------------------------------------------- */
/* Part 1: drop-in replacements for the reference's analysis API              */
/* ------------------------------------------------------------------------- */

/* reference src/world/dio.h:16-23 */
typedef struct {
  double f0_floor;
  double f0_ceil;
  double channels_in_octave;
  double frame_period; /* msec */
  int speed;           /* 1, 2, ..., 12 */
  double allowed_range;
} DioOption;

/* reference src/world/harvest.h:16-20 */
typedef struct {
  double f0_floor;
  double f0_ceil;
  double frame_period;
} HarvestOption;

/* reference src/world/cheaptrick.h:16-20 */
typedef struct {
  double q1;
  double f0_floor;
  int fft_size;
} CheapTrickOption;

/* reference src/world/d4c.h:16-18 */
typedef struct {
  double threshold;
} D4COption;

/* reference src/world/dio.h:38,48,61 (src/dio.cpp:639-666) */
WORLD_HIP_API void Dio(const double *x, int x_length, int fs, const DioOption *option,
                       double *temporal_positions, double *f0);
WORLD_HIP_API void InitializeDioOption(DioOption *option);
WORLD_HIP_API int GetSamplesForDIO(int fs, int x_length, double frame_period);

/* reference src/world/harvest.h:35,45,59 (src/harvest.cpp:1219-1262) */
WORLD_HIP_API void Harvest(const double *x, int x_length, int fs, const HarvestOption *option,
                           double *temporal_positions, double *f0);
WORLD_HIP_API void InitializeHarvestOption(HarvestOption *option);
WORLD_HIP_API int GetSamplesForHarvest(int fs, int x_length, double frame_period);

/* reference src/world/stonemask.h:27 (src/stonemask.cpp:212-218) */
WORLD_HIP_API void StoneMask(const double *x, int x_length, int fs, const double *temporal_positions,
                             const double *f0, int f0_length, double *refined_f0);

/* reference src/world/cheaptrick.h:38,52,65,80 (src/cheaptrick.cpp:191-240) */
WORLD_HIP_API void CheapTrick(const double *x, int x_length, int fs, const double *temporal_positions,
                              const double *f0, int f0_length, const CheapTrickOption *option,
                              double **spectrogram);
WORLD_HIP_API void InitializeCheapTrickOption(int fs, CheapTrickOption *option);
WORLD_HIP_API int GetFFTSizeForCheapTrick(int fs, const CheapTrickOption *option);
WORLD_HIP_API double GetF0FloorForCheapTrick(int fs, int fft_size);

/* reference src/world/d4c.h:35,46 (src/d4c.cpp:342-407) */
WORLD_HIP_API void D4C(const double *x, int x_length, int fs, const double *temporal_positions,
                       const double *f0, int f0_length, int fft_size, const D4COption *option,
                       double **aperiodicity);
WORLD_HIP_API void InitializeD4COption(D4COption *option);

/* reference src/world/codec.h:23,38,53,69,86 (src/codec.cpp:212-324) -- SURVEY.md 8f.1.
 * All five public symbols of codec.o are defined so that the object is never pulled from
 * a reference archive linked behind this library. */
WORLD_HIP_API int GetNumberOfAperiodicities(int fs);
WORLD_HIP_API void CodeAperiodicity(const double *const *aperiodicity, int f0_length, int fs, int fft_size,
                                    double **coded_aperiodicity);
WORLD_HIP_API void DecodeAperiodicity(const double *const *coded_aperiodicity, int f0_length, int fs,
                                      int fft_size, double **aperiodicity);
WORLD_HIP_API void CodeSpectralEnvelope(const double *const *spectrogram, int f0_length, int fs, int fft_size,
                                        int number_of_dimensions, double **coded_spectral_envelope);
WORLD_HIP_API void DecodeSpectralEnvelope(const double *const *coded_spectral_envelope, int f0_length, int fs,
                                          int fft_size, int number_of_dimensions, double **spectrogram);

/* reference src/world/synthesis.h:30 (src/synthesis.cpp:339-399) -- SURVEY.md 8f.3.  The only public
 * symbol of synthesis.o; the real-time synthesiser of synthesisrealtime.o follows below. */
WORLD_HIP_API void Synthesis(const double *f0, int f0_length, const double *const *spectrogram,
                             const double *const *aperiodicity, int fft_size, double frame_period, int fs,
                             int y_length, double *y);

/* ---- real-time synthesis: reference src/world/synthesisrealtime.h (src/synthesisrealtime.cpp) -----------------------
 * The synthesiser struct and the types it embeds, with the reference's sizes, field offsets and public field names, so
 * that a caller's `WorldSynthesizer s = {0};` and its reads of s.buffer, s.head_pointer, ... work unchanged.  The types
 * below are those of the reference's world/fft.h, world/common.h and world/matlabfunctions.h; this library fills none of
 * the FFT members (the transforms run on the GPU), and they are declared only so that the struct has its size. */
typedef double fft_complex[2];
typedef struct {                 /* world/fft.h: a plan of the reference's FFT (unused here) */
  int n;
  int sign;
  unsigned int flags;
  fft_complex *c_in;
  double *in;
  fft_complex *c_out;
  double *out;
  double *input;
  int *ip;
  double *w;
} fft_plan;
typedef struct {                 /* world/common.h */
  int fft_size;
  double *waveform;
  fft_complex *spectrum;
  fft_plan forward_fft;
} ForwardRealFFT;
typedef struct {                 /* world/common.h */
  int fft_size;
  double *waveform;
  fft_complex *spectrum;
  fft_plan inverse_fft;
} InverseRealFFT;
typedef struct {                 /* world/common.h */
  int fft_size;
  double *log_spectrum;
  fft_complex *minimum_phase_spectrum;
  fft_complex *cepstrum;
  fft_plan inverse_fft;
  fft_plan forward_fft;
} MinimumPhaseAnalysis;
typedef struct {                 /* world/matlabfunctions.h: xorshift128 state of randn() */
  unsigned int g_randn_x;
  unsigned int g_randn_y;
  unsigned int g_randn_z;
  unsigned int g_randn_w;
} RandnState;
/* What this library keeps in each field.  The contract covers every scalar field, f0_length[], f0_origin[],
 * number_of_pulses[] and pulse_locations_index[] (host arrays mirrored after every call), randn_state (the generator
 * after the pulses Synthesis2 has gone past), dc_remover[0, fft_size / 2) and buffer[0, buffer_size): the output of the
 * last successful Synthesis2.  Deviations from the reference:
 *   - the spectrogram / aperiodicity rows are read when AddParameters is called (copied to the GPU), not when they are
 *     synthesised: a caller that rewrites rows after adding them gets the values they had when added;
 *   - buffer[buffer_size, 2 buffer_size + fft_size) is the library's own (the reference keeps its partial sums there);
 *   - `spectrogram` holds the library's state (an opaque handle; do not touch), `aperiodicity`, interpolated_vuv,
 *     pulse_locations, impulse_response and the three FFT members are NULL / zero.
 * fft_size must be a power of two from 128 to 8192 (checked before any GPU work).  Failures report through
 * world_hip_set_error_handler (below); AddParameters, Synthesis2 and IsLocked then return 0. */
typedef struct {
  int fs;
  double frame_period;           /* seconds */
  int buffer_size;
  int number_of_pointers;
  int fft_size;
  double *buffer;                /* [2 buffer_size + fft_size]; [0, buffer_size) = the last Synthesis2 output */
  int current_pointer;
  int i;
  double *dc_remover;            /* [fft_size / 2] */
  int *f0_length;                /* [number_of_pointers] */
  int *f0_origin;                /* [number_of_pointers] */
  double ***spectrogram;         /* this library: its state */
  double ***aperiodicity;
  int current_pointer2;
  int head_pointer;
  int synthesized_sample;
  int handoff;
  double handoff_phase;
  double handoff_f0;
  int last_location;
  int cumulative_frame;
  int current_frame;
  double **interpolated_vuv;
  double **pulse_locations;
  int **pulse_locations_index;   /* [number_of_pointers] -> number_of_pulses[k] sample indices */
  int *number_of_pulses;         /* [number_of_pointers] */
  double *impulse_response;
  RandnState randn_state;
  MinimumPhaseAnalysis minimum_phase;
  InverseRealFFT inverse_real_fft;
  ForwardRealFFT forward_real_fft;
} WorldSynthesizer;
/* reference src/world/synthesisrealtime.h:93,112,118,123,139,151 (src/synthesisrealtime.cpp:444-603) */
WORLD_HIP_API void InitializeSynthesizer(int fs, double frame_period, int fft_size, int buffer_size,
                                         int number_of_pointers, WorldSynthesizer *synth);
WORLD_HIP_API int AddParameters(double *f0, int f0_length, double **spectrogram, double **aperiodicity,
                                WorldSynthesizer *synth);
WORLD_HIP_API void RefreshSynthesizer(WorldSynthesizer *synth);
WORLD_HIP_API void DestroySynthesizer(WorldSynthesizer *synth);
WORLD_HIP_API int IsLocked(WorldSynthesizer *synth);
WORLD_HIP_API int Synthesis2(WorldSynthesizer *synth);

/* ---- audio and parameter files: the reference's tools/ library ------------
 * Same names, arguments and on-disk bytes as tools/audioio.h:25-47 and tools/parameterio.h:24-114,
 * so examples/parameter_io/{f0,sp,ap}analysis.cpp, readandsynthesis.cpp and test/test.cpp link
 * against this library ALONE.  Headers are parsed and written on the host; the per-sample
 * PCM <-> double conversion of wavread()/wavwrite() runs on the GPU (bit-identical results).
 * Failures print the reference's messages to stdout; there is no other error channel. */
/* tools/audioio.h:25 (tools/audioio.cpp:84-130): 16-bit mono, q = int16(clamp(int(x*32767))); nbit is ignored */
WORLD_HIP_API void wavwrite(const double *x, int x_length, int fs, int nbit, const char *filename);
/* tools/audioio.h:35 (tools/audioio.cpp:132-173): samples in the file; 0 = cannot open, -1 = not accepted */
WORLD_HIP_API int GetAudioLength(const char *filename);
/* tools/audioio.h:47 (tools/audioio.cpp:175-252): mono PCM of 8..32 bits, x = q / 2^(nbit-1) */
WORLD_HIP_API void wavread(const char *filename, int *fs, int *nbit, double *x);
/* tools/parameterio.h:24 (tools/parameterio.cpp:58-88): "F0  " NOF FP + f64 values, or "%.5f %.5f\r\n" text */
WORLD_HIP_API void WriteF0(const char *filename, int f0_length, double frame_period,
                           const double *temporal_positions, const double *f0, int text_flag);
/* tools/parameterio.h:39 (tools/parameterio.cpp:90-117): returns 1 on success; positions = i / 1000 * FP */
WORLD_HIP_API int ReadF0(const char *filename, double *temporal_positions, double *f0);
/* tools/parameterio.h:56 (tools/parameterio.cpp:119-143): "NOF ", "FP  ", "FFT ", "NOD ", "FS  "; 0 if absent */
WORLD_HIP_API double GetHeaderInformation(const char *filename, const char *parameter);
/* tools/parameterio.h:70,85 (tools/parameterio.cpp:145-191): "SPEC" NOF FP FFT NOD FS + rows of f64 */
WORLD_HIP_API void WriteSpectralEnvelope(const char *filename, int fs, int f0_length, double frame_period,
                                         int fft_size, int number_of_dimensions, const double *const *spectrogram);
WORLD_HIP_API int ReadSpectralEnvelope(const char *filename, double **spectrogram);
/* tools/parameterio.h:99,114 (tools/parameterio.cpp:193-243): "AP  ", same layout */
WORLD_HIP_API void WriteAperiodicity(const char *filename, int fs, int f0_length, double frame_period,
                                     int fft_size, int number_of_dimensions, const double *const *aperiodicity);
WORLD_HIP_API int ReadAperiodicity(const char *filename, double **aperiodicity);


/* ---- behaviour of the drop-in symbols that the reference does not have to state -----------------
 * Re-entrancy: like the reference (all state on the stack: src/cheaptrick.cpp:205-206, src/d4c.cpp:345-346) the
 * symbols above may be called from several host threads at once.  Each call runs on one SLOT of a small pool (a
 * library context on its own stream + its device / pinned buffers); WORLD_HIP_DROPIN_SLOTS (default 4) calls run side
 * by side on device WORLD_HIP_DEVICE (default 0), further callers wait for a slot.
 * Resident input: a slot keeps the last signal `x` it uploaded; StoneMask / CheapTrick / D4C (and a repeated Harvest /
 * Dio) on the same pointer, length AND content (a 64-bit hash of every sample) skip the upload.
 * WORLD_HIP_DROPIN_CACHE_X=0 turns that off.  Matrices move through pinned staging in chunks, copied to / from the
 * caller's rows by the calling thread and WORLD_HIP_DROPIN_COPY_THREADS (default 3) helper threads.
 * Errors: the reference API has no error channel and never fails; this library can (no GPU, out of device memory, a
 * shape beyond world_hip_check_shape()).  There is NO CPU fallback.  A failing drop-in call reports through the handler
 * installed here: `function` is the symbol's name, `message` the reason (also world_hip_last_error()).  If the handler
 * returns, the drop-in call returns to its caller; it may also longjmp or throw.  The caller's output buffers are untouched
 * when the call was refused up front (a shape limit, a missing GPU) and UNSPECIFIED after a failure in mid-transfer (the
 * matrices are downloaded chunk by chunk into the caller's rows: a device error between two chunks leaves earlier rows written).
 * With no handler (the default, handler = NULL) the reason is printed to stderr and the process aborts.
 * Hostile values (tests/test_hostile.py): samples may be NaN, +-Inf, 1e308 or denormal -- every call returns, the results
 * are as meaningless as the reference's, temporal_positions never depend on the samples, and the next call is unaffected.
 * Caller-made F0 tracks: the reference turns F0 into window lengths and array indices unchecked (src/cheaptrick.cpp:95,
 * src/d4c.cpp:55-56, src/stonemask.cpp:129, src/common.cpp:60-62) -- NaN and values from about fs/2 up are undefined
 * behaviour there.  Here, and ONLY for such values, the analysis differs from it by rule:
 *   F0 is NaN   CheapTrick: the frame is analysed as unvoiced (the default 500 Hz); D4C: unvoiced (the row is 1 - 1e-12);
 *               StoneMask: the refined value is 0
 *   F0 > fs/2   CheapTrick and D4C analyse the frame as F0 = fs/2 (+Inf included).  The frame then draws fewer randn()
 *               values than the reference would, so LATER frames of that utterance meet other noise samples than the
 *               reference's (differences at the 1e-12 safeguard level); utterances without such a frame are unaffected
 *   F0 <= floor, negative, -Inf: the reference's own floors apply (src/cheaptrick.cpp:218, src/d4c.cpp:263,300), as there. */
typedef void (*WorldHipErrorHandler)(const char *function, const char *message, void *user);
WORLD_HIP_API void world_hip_set_error_handler(WorldHipErrorHandler handler, void *user);
/* Releases what the drop-in layer holds: its helper threads are joined and every slot's context, streams, events, device
 * and pinned buffers are freed.  For host processes that want the GPU path gone without exiting; the next drop-in call
 * starts over (a cold call).  Returns 0, or -1 -- nothing released -- while a drop-in call is running.
 * Environment of the drop-in layer, read once: WORLD_HIP_DROPIN_SLOTS (4), WORLD_HIP_DROPIN_COPY_THREADS (3; 0 = the calling
 * thread copies alone), WORLD_HIP_DROPIN_SPIN_US (0: an idle copy helper sleeps; N > 0: it first polls N microseconds for the next chunk of a
 * running transfer -- worth under 1 %), WORLD_HIP_DROPIN_WIRE (f32: the spectrogram / aperiodicity rows cross
 * PCIe as float -- rounded once on the device, 6e-8 relative -- and are widened into the caller's double rows on the host:
 * half the bytes of the path's PCIe-bound stages; default: double, bit-identical to the device-resident analysis). */
WORLD_HIP_API int world_hip_shutdown(void);
/* diagnostic counters of the drop-in layer: slots created, calls that found their signal resident / had to upload it */
WORLD_HIP_API void world_hip_dropin_stats(unsigned long long *slots, unsigned long long *x_hits,
                                          unsigned long long *x_misses);

/* ------------------------------------------------------------------------- */
/* Part 2: batched device-resident API                                        */
/* ------------------------------------------------------------------------- */
/*
 * Layout.  A batch is n_utt utterances with one sampling rate.  Every array is
 * dense and padded to a per-batch stride:
 *   x            [n_utt][x_stride]            samples            (device)
 *   x_length     [n_utt]                      valid samples      (HOST)
 *   tpos, f0     [n_utt][f_stride]            per-frame scalars  (device)
 *   n_frames     [n_utt]                      valid frames       (HOST)
 *   sp, ap       [n_utt][f_stride][fft/2+1]   dense rows         (device)
 * Frame counts follow GetSamplesForHarvest/GetSamplesForDIO.  Rows/frames beyond
 * an utterance's own count are left untouched.  All functions enqueue work on the
 * context's stream and return without synchronising; 0 = success, non-zero =
 * failure with the reason available from world_hip_last_error().
 */
typedef struct WorldHipContext WorldHipContext;

/* stream = a hipStream_t to enqueue on (NULL = the device's default stream) */
WORLD_HIP_API WorldHipContext *world_hip_create(int device, void *stream);
WORLD_HIP_API void world_hip_destroy(WorldHipContext *ctx);
WORLD_HIP_API const char *world_hip_last_error(void);
/* Version of the batched C ABI below (the reference's own 13 symbols never change).  Bumped whenever a prototype in this
 * header changes incompatibly; a binding built against another major value must refuse to bind (world_amd/api.py does).
 *   5  round 5: world_hip_spectral_packed_range / _cheaptrick_batch_range / _d4c_batch_range take `reuse_offsets`
 *   6  round 6: + world_hip_abi_version itself; no prototype changed.  Later additions keep 6: they add entry points and
 *      change no prototype (the world_hip_realtime_* calls, world_hip_modify_batch and its kin, world_hip_synthesis_records
 *      and world_hip_realtime_add_coded); bindings look for them by name.
 * Libraries older than 6 lack the symbol. */
#define WORLD_HIP_ABI_VERSION 6
/* Launch-geometry hints of a context (bits; default 0).  Results never depend on them.
 *   WORLD_HIP_HINT_SHARED_DEVICE  other jobs run on this device at the same time (several contexts on their own streams, as in
 *       bench.py's headline mode): single-utterance calls then keep the narrow launch shapes that fit beside other jobs'
 *       frame kernels.  Without it a single-utterance call assumes the device to itself and gives Harvest's one-workgroup-
 *       per-utterance contour kernels (FixStep1-2 + sections, MergeF0) 1024 threads instead of 256: 0.089 -> 0.047 ms of a
 *       lone 10 s job, at the price of sixteen wavefronts waiting for one CU when the device is busy. */
#define WORLD_HIP_HINT_SHARED_DEVICE 1
WORLD_HIP_API int world_hip_set_hint(WorldHipContext *ctx, int hint);
WORLD_HIP_API int world_hip_abi_version(void);
WORLD_HIP_API int world_hip_sync(WorldHipContext *ctx);
/* bytes of device workspace currently held by the context (its arena, the resampler's coefficient tables and the mel-cepstrum's tables) */
WORLD_HIP_API unsigned long long world_hip_workspace_bytes(WorldHipContext *ctx);
/* The reference's randn() stream (src/matlabfunctions.cpp:237-264) is a constant of the algorithm: one
 * table per device, shared by every context of the process, checked in full against a sequential host
 * statement of the generator whenever it is (re)built.  bytes() = what it holds (live + superseded
 * generations); verify() reduces the live table again and compares (0 = intact; synchronises). */
WORLD_HIP_API unsigned long long world_hip_noise_table_bytes(WorldHipContext *ctx);
WORLD_HIP_API int world_hip_verify_tables(WorldHipContext *ctx);
/* cold-start accounting: host wall-clock milliseconds this process has spent building + verifying the device's tables
 * (all generations), and how many generations were built.  The host statement is stepped by up to
 * WORLD_HIP_TABLE_THREADS (default min(16, cores)) threads, each range's jump-table seed confirmed sequentially. */
WORLD_HIP_API double world_hip_noise_table_build_ms(WorldHipContext *ctx, int *builds);

/* Per-kernel timing with HIP events on the launch stream (process-wide switch).
 * collect() waits for the recorded kernels and returns "kernel_name ms\n" lines. */
WORLD_HIP_API void world_hip_profile_enable(int on);
WORLD_HIP_API int world_hip_profile_collect(char *buf, int cap);

WORLD_HIP_API int world_hip_harvest_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x,
                                          int x_stride, const int *x_length, const HarvestOption *option,
                                          int f_stride, double *d_tpos, double *d_f0);
WORLD_HIP_API int world_hip_dio_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x,
                                      int x_stride, const int *x_length, const DioOption *option,
                                      int f_stride, double *d_tpos, double *d_f0);
WORLD_HIP_API int world_hip_stonemask_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x,
                                            int x_stride, const int *x_length, const int *n_frames,
                                            int f_stride, const double *d_tpos, const double *d_f0,
                                            double *d_refined_f0);
WORLD_HIP_API int world_hip_cheaptrick_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x,
                                             int x_stride, const int *x_length, const int *n_frames,
                                             int f_stride, const double *d_tpos, const double *d_f0,
                                             const CheapTrickOption *option, double *d_spectrogram);
WORLD_HIP_API int world_hip_d4c_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x,
                                      int x_stride, const int *x_length, const int *n_frames,
                                      int f_stride, const double *d_tpos, const double *d_f0,
                                      int fft_size, const D4COption *option, double *d_aperiodicity);

/* Waveform synthesis from analysis parameters (reference src/synthesis.cpp:339-399):
 *   f0 [n_utt][f_stride], spectrogram / aperiodicity [n_utt][f_stride][fft_size/2+1] (device),
 *   n_frames, y_length [n_utt] (HOST), y [n_utt][y_stride] (device).  frame_period in ms.
 * The pulse count is data dependent and only known on the device: the workspace holds a mean pulse rate of
 * 1200 Hz over the longest utterance unless world_hip_set_synthesis_pulse_capacity() said otherwise (pulses
 * per utterance; 0 = automatic).  A call that needs more does NOT fail silently: the device records the count,
 * world_hip_sync() then fails with it in world_hip_last_error(), world_hip_synthesis_pulses_dropped() returns it
 * (0 = every pulse was rendered; synchronises; clears the record) -- set the capacity and repeat the call.
 * The drop-in Synthesis() does exactly that by itself. */
WORLD_HIP_API int world_hip_synthesis_batch(WorldHipContext *ctx, int n_utt, int fs, double frame_period,
                                            int fft_size, const int *n_frames, int f_stride, const double *d_f0,
                                            const double *d_spectrogram, const double *d_aperiodicity,
                                            const int *y_length, int y_stride, double *d_y);

/* Synthesis straight from the records the analysis writes (world_hip_analyze_packed, world_hip_analyze_coded; also what the
 * multi-GPU exchange moves and what a vocoder service is handed): no dense arrays, no unpack or decode call, no buffer of the
 * caller's.  Layout: utterance u's n_frames[u] valid frames occupy rows first_row + sum_{v<u} n_frames[v] ... of d_block
 * ([rows][cols] doubles, device); a record's tpos is not read.
 *   wire 0  f64 records, cols = world_hip_record_columns(fft_size, 0).  Read in place by the pulse kernels: nothing is staged.
 *   wire 1  f32 records, cols = world_hip_record_columns(fft_size, 1).  Widened to f64.
 *   wire 2  coded records [tpos, f0, mel-cepstrum[number_of_dimensions], band aperiodicity], cols =
 *           world_hip_coded_columns(fs, number_of_dimensions).  Decoded with the arithmetic of
 *           world_hip_decode_spectral_envelope / world_hip_decode_aperiodicity (an aperiodic frame -- mean band value above
 *           -0.5 dB -- gets the 1 - 1e-12 row), both rows in one launch.
 * number_of_dimensions is ignored for wires 0 and 1.  Wires 1 and 2 stage each frame's rows once as dense f64 in the
 * context's workspace (8 + 16 (fft_size/2+1) bytes per frame; world_hip_workspace_bytes counts them).  The waveform is, bit
 * for bit, that of world_hip_unpack_results (wire 1: of the widened records) or the two decode calls followed by
 * world_hip_synthesis_batch.  Refused before any GPU work, with a message: cols that do not match the wire, a null block,
 * first_row < 0, n_frames[u] < 2, y_length[u] outside [1, y_stride], a pair (fs, fft_size) world_hip_check_shape refuses,
 * and for wire 2 what the decoders refuse (number_of_dimensions outside [1, fft_size/4+1], fs without an aperiodicity
 * band).  The (fs, fft_size) rule is world_hip_check_shape's whole rule -- the analysis stages' limits too, since records
 * are what the analysis writes -- and so stricter than world_hip_synthesis_batch's own: a pair that only the synthesiser
 * accepts (e.g. fs below what D4C takes) is refused here; unpack or decode such rows and use world_hip_synthesis_batch.
 * Pulse capacity: exactly world_hip_synthesis_batch's (world_hip_set_synthesis_pulse_capacity,
 * world_hip_synthesis_pulses_dropped, world_hip_sync).  Stream order as the other batched calls; after one eager call of
 * the shape a call neither allocates nor copies from the host and can be captured (the row offsets are small per-call
 * arrays like n_frames); a replay reads whatever the block holds then. */
WORLD_HIP_API int world_hip_synthesis_records(WorldHipContext *ctx, int n_utt, int fs, double frame_period, int fft_size,
                                              const int *n_frames, long long first_row, const double *d_block, int cols,
                                              int wire, int number_of_dimensions, const int *y_length, int y_stride,
                                              double *d_y);

/* What box is this?  ~50 ms of microbenchmarks on the context's device (synchronous; allocates and frees 2 GB):
 * values[0] shader clock held under a chip-wide FP64 load (MHz), [1] that load's FMA rate over the whole launch (TFLOP/s; HIP events), [2] / [3] / [4]
 * dependent-load latency of one lane chasing pointers through 2 GB / 64 MB every CU has just read / 1 MB it has just walked (ns per hop), [5] / [6] a dependent LDS read on
 * an idle / a loaded CU (shader cycles), [7] compute units.  n_values >= 8.  bench.py records them in the line's
 * `environment` object: identical binaries ran a lone job 10-90 % slower on some boxes (profiles/r04/README.txt). */
WORLD_HIP_API int world_hip_probe_machine(WorldHipContext *ctx, double *values, int n_values);
/* The per-frame real FFT of the path in isolation (the reference's fft_plan_dft_r2c_1d / _c2r_1d +
 * fft_execute, src/world/fft.h:22-44, as re-implemented in csrc/fft.h): `batch` transforms of 2^lg_n
 * points (64 .. 16384), one workgroup each, straight from and to HBM -- the test and microbenchmark hook.
 *   rfft : d_in [batch][N] -> d_spectrum [batch][N/2+1][2] (re, im), X[k] = sum x[n] e^{-2 pi i k n / N}
 *   irfft: d_spectrum -> d_out [batch][N] = N * irfft (unscaled like the reference's c2r; Im of DC / Nyquist ignored)
 * max_lr = 3 (radix-8 plan) or 4 (radix-16 plan); threads = workgroup size, 0 = one butterfly per thread;
 * static_plan != 0 selects the instantiation whose length is a compile-time constant (what the frame kernels
 * run: radix-8 plan, 1024 / 2048 / 4096 points), 0 the one that takes it at run time. */
WORLD_HIP_API int world_hip_probe_rfft(WorldHipContext *ctx, int lg_n, int max_lr, int threads, int static_plan,
                                       long long batch, const double *d_in, double *d_spectrum);
WORLD_HIP_API int world_hip_probe_irfft(WorldHipContext *ctx, int lg_n, int max_lr, int threads, int static_plan,
                                        long long batch, const double *d_spectrum, double *d_out);
/* Every composition of csrc/fft.h's entry points that a stage kernel runs, in isolation: `batch` transforms of 2^lg_n points,
 * one workgroup of `threads` threads each, with the template arguments of the kernels named below.  swizzle = the LDS slot
 * map the probe is compiled with: 0 the shipped one, 1 d4c.hip's.  Real rows are [batch][N], spectra [batch][N/2+1][2]
 * (re, im), plain complex rows [batch][N][2].  threads = 64 .. 1024 in steps of 64 unless the mode fixes it.  Anything that
 * is not listed fails with a message naming what is; the one-lane host emulation has modes 1 .. 6, 18 and 19 only.
 * Swizzle 0 has modes 1 .. 12, 18 and 19; swizzle 1 has what d4c.hip runs: 1 (max_lr 3), 7 (2^11), 13 .. 19.
 *    1  r2c, block_rfft<max_lr>, the twiddle table of the inner N/2-point transform   2^6 .. 2^14, max_lr 3 | 4
 *       (ct_frame, hv_band_spectra, d4c_lovetrain)
 *    2  c2r unscaled, block_irfft<max_lr> (ct_frame, sy_pulse, rt_pulse)               2^6 .. 2^14, max_lr 3 | 4
 *    3  r2c, block_rfft_from<3>: the first stage reads a functor (sy_pulse, ct_frame)  2^6 .. 2^14, max_lr 3
 *    4  r2c, block_rfft<4>, the table staged at N itself (codec_code_sp, ct_frame_coded) 2^6 .. 2^13, max_lr 4
 *    5  complex forward, block_cfft_dif, default plan (decode_sp_row)                  2^6 .. 2^13, max_lr 4
 *    6  complex forward of a row that is zero beyond element N/2, block_cfft_dif_from<3>, the table one level coarser than
 *       the transform (minimum_phase of synthesis.hip)                                  2^6 .. 2^13, max_lr 3
 *    7, 8, 9  modes 1, 2, 3 with the length a compile-time constant (ct_frame, d4c_lovetrain) 2^10 .. 2^12, max_lr 3
 *   10  r2c, block_cfft_dif_static<11, 3, 256> + rfft_merge_items<5, 256> (hv_block_spectra)      2^12, 256 threads
 *   11  c2r unscaled, irfft_pretwiddle_items_w<5, 256> with twiddles by rotation + block_cfft_dit_static<11, 3, 256>
 *       (hv_band_events_fft)                                                                      2^12, 256 threads
 *   12  c2r unscaled, irfft_pretwiddle_items<5, 256> + the same inverse (no caller: fft.h promises mode 2's values)
 *   13  r2c TIMES TWO, block_cfft_dif_static<11, 3, 256> + rfft_merge_items_w<5, 256, true> with twiddles by rotation
 *       (d4c_lovetrain's 4096-point shape)                                                        2^12, 256 threads
 *   14  r2c by d4c_frame's route: quarter-wave table two levels coarser than the merge's, direct tables for the two inner
 *       radix-8 stages, block_cfft_dif_static<lg-1, 3, N/16> + rfft_merge_items_rot<K, N/16>   2^11 .. 2^14, N/16 threads
 *   15  the same TIMES TWO: rfft_merge_items_rot<K, N/16, true>
 *   16  mode 14 with the run-time plan's stages (block_cfft_dif<3>) for the static ones (no caller: static == run-time)
 *   17  no input read: one complex row of the twiddles e^{-2 pi i k / 2^level} d4c_frame's staging serves -- [0, N/128) level
 *       lg-4 and [N/128, N/128 + N/1024) level lg-7 from the direct tables, the same from the plain table at N/4,
 *       [3N/8, 3N/8 + N/16) level lg-1, [N/2, N) level lg (k < N/2), zero elsewhere
 *   18, 19  dft8<true> / dft8_head2<true> (the latter on the first two values) on `batch` rows of 8 complex values; lg_n = 3 */
WORLD_HIP_API int world_hip_probe_fft(WorldHipContext *ctx, int mode, int lg_n, int max_lr, int threads, int swizzle,
                                      long long batch, const void *d_in, void *d_out);
/* D4C's band selection in isolation (csrc/d4c.hip: the radix select that stands for the reference's std::sort in
 * GetCoarseAperiodicity, src/d4c.cpp:194-225): `rows` workgroups of `threads` threads (128, 256, 512 or 1024: d4c_frame's), each
 * over one row of d_keys [rows][threads][10] -- thread t's ten slots as d4c_frame hands them over: finite doubles with the
 * sign bit clear; slots 0 .. 7 owned, slot 8 non-zero on thread 0 only, slot 9 zero (the probe loads what it is given).
 *   mode 0  block_excluding_largest<threads>(key, K, ..) as the band loop calls it
 *   mode 1  the general routine block_smallest_sum<threads>(key, 10, 10 threads, 10 threads - K, ..) directly
 * d_out [rows][3]: the sum of all slots but the K largest, the sum of all slots (both formed as d4c_frame's tail forms them:
 * the wavefronts' shares added in wavefront order), and the route taken -- 0 one pass, 1 two passes, 2 the general routine
 * (always 2 in mode 1).  1 <= K <= 10 threads (K = 10 threads, no key left: the probe itself writes the 0).  A refusal names the argument and writes nothing. */
WORLD_HIP_API int world_hip_probe_select(WorldHipContext *ctx, int mode, int threads, int K, long long rows,
                                         const double *d_keys, double *d_out);
/* Harvest's back half in isolation (csrc/harvest.hip: hv_prune -- RemoveUnreliableCandidates and SearchF0Base, src/harvest.cpp:
 * 652-705 -- then csrc/harvest_contour.hip: FixStep1 .. 4, SmoothF0Contour and the hop subsampling, :710-1113, :1246-1251) on
 * refined candidates the caller made up, where Harvest proper takes them from hv_refine: the same kernels, launch shapes
 * (the one-utterance shapes and WORLD_HIP_HINT_SHARED_DEVICE included), HarvestParams fields and workspace carve as a Harvest
 * call of n_utt utterances whose longest has max nfb 1 ms frames.
 *   nfb, nc (host, [n_utt])  1 ms frames per utterance (>= 1) and candidates per frame: utterance u uses slots 0 .. 7 nc[u] - 1
 *   maxc                     slots per frame, a multiple of 7 in 7 .. 252 (Harvest's own is 105 at the default F0 range)
 *   fb_stride, sec_cap       the batch's row lengths, given so that both sides state them: (max nfb + 7) & ~7 and max nfb / 2 + 4
 *   d_cand, d_score          [n_utt][fb_stride][maxc] refined candidates (0 = none) and their scores
 * Out, rows 0 .. nfb[u] - 1 of utterance u only (what lies past them is not touched):
 *   d_pruned_cand, d_pruned_score [n_utt][fb_stride][maxc]  after RemoveUnreliableCandidates; slots 7 nc[u] .. maxc - 1 hold
 *                            workspace bytes, and nothing is written for an utterance with nc[u] = 0
 *   d_step2, d_step3, d_step4, d_basic_f0 [n_utt][fb_stride]  the contour after FixStep2, FixStep3, FixStep4 and the smoother
 *   d_sec_n [n_utt][2], d_sec [n_utt][6][sec_cap]  the section table as the last launch leaves it: sec_n[0] voiced sections of
 *                            the step-4 contour, their first and last frames in rows 0 and 1 (rows 2 .. 5 and sec_n[1] are
 *                            scratch of the passes before)
 *   d_tpos, d_f0 [n_utt][f_stride]  frames at frame_period ms: (int)((nfb[u] - 1) / frame_period) + 1 of them
 * Overwritten before the last launch ends and therefore not reported: the base pick (SearchF0Base's contour: FixStep4 writes
 * its own over it -- it shows through step 2 wherever FixStep1 and 2 pass a frame), the number of sections ExtendSub kept
 * (sec_n[1], cleared by the section pass of step 4), the sections of steps 2 and 3 and their extended slices (the smoother's
 * scratch).  Extend's nearest candidate: two candidates whose distances from the previous pick are equal after clearing the
 * low 8 mantissa bits count as equally near, and the later slot wins (the reference: the nearer, the later of exact equals).
 * A refusal names the argument and writes nothing. */
WORLD_HIP_API int world_hip_probe_harvest_contour(WorldHipContext *ctx, int n_utt, const int *nfb, const int *nc, int maxc,
                                                  int fb_stride, const double *d_cand, const double *d_score, double frame_period,
                                                  int f_stride, double *d_pruned_cand, double *d_pruned_score, double *d_step2,
                                                  double *d_step3, double *d_step4, int sec_cap, int *d_sec_n, int *d_sec,
                                                  double *d_basic_f0, double *d_tpos, double *d_f0);
/* Harvest's middle in isolation (csrc/harvest.hip: hv_compact_events, hv_raw_candidates -- GetF0CandidateContour, src/harvest.cpp:
 * 240-293, on the intervals of ZeroCrossingEngine's fine edges, :188-190 -- and hv_detect, DetectOfficialF0Candidates, :348-412)
 * on zero-crossing lists the caller made up, where Harvest proper takes them from the filter bank: the same kernels, grids and
 * LDS sizes, and the lists of ONE group of ev_group utterances in the workspace at a time, as a Harvest call walks them.
 *   nfb (host, [n_utt])      1 ms frames per utterance (>= 1); frame f sits at f / 1000 s
 *   afs, f0_floor, f0_ceil   analysis rate (events are in samples of it) and the gate's limits
 *   nch, band_f0 (host, [nch])  12 .. 365 bands and their positive boundary F0s; maxc = round(nch / 10) * 7, Harvest's own
 *   fb_stride                (max nfb + 7) & ~7, given so that both sides state it
 *   nseg, seg_cap, ev_cap    segment lists per (utterance, band, family), the capacity of one, the capacity of a final list.
 *                            nseg = 1: the segment lists ARE the final lists (seg_cap = ev_cap) and no compaction runs
 *   ev_group                 utterances whose lists are in the workspace at once (Harvest's own: WORLD_HIP_EVENT_GROUP, 40)
 *   stages                   1 compaction, 2 raw candidates (behind the compaction where nseg > 1), 4 detection
 *   d_seg_events [n_utt][nch * 4][nseg][seg_cap], d_seg_count [n_utt][nch * 4][nseg]  ascending fine edges per family (falling,
 *                            rising, peaks, dips) and their numbers, 0 .. seg_cap (read back and checked: a refusal otherwise)
 * Out (device); what is not named is not touched:
 *   d_events [n_utt][nch * 4][ev_cap], d_ev_count [n_utt][nch * 4]  stage 1 with nseg > 1: the first ev_count events of every list
 *   d_raw [n_utt][nch][fb_stride]  stage 2: frames 0 .. nfb[u] - 1 of every band.  Without stage 2 it is detection's INPUT
 *   d_cand [n_utt][fb_stride][maxc]  stage 4: slots 0 .. min(maxc, (nch + 10) / 11 + 1) - 1 of frames 0 .. nfb[u] - 1
 *   d_nc [n_utt]             stage 4: the most candidates a frame of the utterance has (cleared by the probe; in a Harvest call
 *                            hv_remove_mean clears it)
 * Buffers of stages that do not run may be null.  A refusal names the argument and writes nothing. */
WORLD_HIP_API int world_hip_probe_harvest_candidates(WorldHipContext *ctx, int n_utt, const int *nfb, double afs, double f0_floor,
                                                     double f0_ceil, int nch, const double *band_f0, int maxc, int fb_stride,
                                                     int nseg, int seg_cap, int ev_cap, int ev_group, int stages,
                                                     const double *d_seg_events, const int *d_seg_count, double *d_events,
                                                     int *d_ev_count, double *d_raw, double *d_cand, int *d_nc);
/* Harvest's refinement in isolation (csrc/harvest.hip: hv_refine / hv_refine_frames -- OverlapF0Candidates and
 * RefineF0Candidates, src/harvest.cpp:417-631) on a decimated signal and a candidate map the caller made up, where Harvest proper
 * takes them from the decimation and from detection: the same kernels, grid, LDS size and tables (launch_harvest_refine).
 *   y_len, nfb, nc (host, [n_utt])  samples (>= 1), 1 ms frames (>= 1; frame f sits at f / 1000 s) and candidates per frame
 *                            (>= 0, 7 nc <= maxc) of every utterance
 *   afs, f0_floor, f0_ceil   analysis rate (1000 .. 48000 Hz, not necessarily whole), the refinement gate's limits.  f0_floor also
 *                            sizes the tables; its longest window must fit the LDS and a 2^14-point transform
 *   maxc                     slots per frame: a multiple of 7, 7 .. 252
 *   fb_stride, y_stride      (max nfb + 7) & ~7 and the samples per utterance slot (>= max y_len), given so that both sides state them
 *   route                    0 what a Harvest call would run for this afs and environment (WORLD_HIP_REFINE_FRAMES,
 *                            WORLD_HIP_REFINE_ROTATE); 1 hv_refine; 2 hv_refine_frames on the window table; 3 hv_refine_frames with
 *                            windows built by rotation.  1 and 2 are refused where fmod(afs, 1000) != 0: there is no table
 *   d_y [n_utt][y_stride]    the signal; samples at and beyond y_len[u] are not read (indices are clamped into 0 .. y_len - 1)
 *   d_cand [n_utt][fb_stride][maxc]  slots 0 .. nc[u] - 1 of frames 0 .. nfb[u] - 1: 0 (none) or a finite value in
 *                            [f0_floor, min(f0_ceil, afs / 2)] -- read back and checked, a refusal otherwise; nothing else is read
 * Out (device): d_refined, d_score [n_utt][fb_stride][maxc].  Slot j + nc[u] m of frame f takes candidate j of frame f - m
 * (m = 0 .. 3) or f + m - 3 (m = 4 .. 6), refined, or (0, 0) where that frame lies outside the utterance, holds no candidate or
 * the refined value fails the gate.  Slots 0 .. 7 nc[u] - 1 of frames 0 .. nfb[u] - 1 are overwritten, nothing else is touched.
 * The candidate domain and the kernels' margin: a candidate f0 is refined in a window of half length hw(f0) = (int)(1.5 afs / f0
 * + 1).  The kernels' LDS holds cap = 2 hw(f0_floor) + 4 samples around a frame and the window tables reach hw(f0_floor) + 2, so
 * a candidate below f0_floor would still be inside both while hw(f0) <= hw(f0_floor) + 1, i.e. f0 > 1.5 afs / (hw(f0_floor) + 1)
 * (39.74 Hz for a floor of 40 Hz at 8 kHz: hw = 301, 12000 / 302); detection never produces one and the probe refuses them all.  Above afs / 2 a
 * candidate has no harmonic (a division by zero in the reference as well).
 * A refusal names the argument and writes nothing. */
WORLD_HIP_API int world_hip_probe_harvest_refine(WorldHipContext *ctx, int n_utt, const int *y_len, const int *nfb, const int *nc,
                                                 double afs, double f0_floor, double f0_ceil, int maxc, int fb_stride, int y_stride,
                                                 int route, const double *d_y, const double *d_cand, double *d_refined,
                                                 double *d_score);

/* Multi-GPU exchange (the reference has no counterpart).  Utterances are sharded over GPUs
 * and analysed independently; a GPU's results are then packed into ONE contiguous block of records
 *     row = [ tpos, f0, spectrogram[0 .. bins), aperiodicity[0 .. bins) ]      (2 + 2 bins doubles)
 * holding the utterances' valid frames back to back, utterance u starting at record first_row + sum of
 * n_frames[0 .. u).  pack / unpack convert between the batched arrays above and such a block (device side,
 * on the context's stream, no synchronisation).
 * world_hip_allgather_blocks is the exchange for ONE process that drives n_dev contexts (one per GPU, one
 * stream each): afterwards d_dst[d] (on context d's device, room for sum(rows) records of `cols` doubles)
 * holds d_src[0], d_src[1], ... back to back.  Every destination pulls its remote blocks with peer copies
 * on its own stream, so all xGMI links of the mesh are busy at once; nothing waits on the host (the
 * destination is valid, and the sources reusable, in the respective context's stream order).
 * With one process PER GPU (torch.distributed / RCCL) the same blocks go through one all-gather:
 * world_amd/distributed.py. */
/* Harvest -> CheapTrick + D4C of one batch in ONE call, into the dense arrays of the *_batch calls (tpos, f0:
 * [n_utt][f_stride]; spectrogram, aperiodicity: [n_utt][f_stride][fft_size/2+1], fft_size = cheaptrick_option->fft_size).
 * Same results, bit for bit, as the three calls in sequence at a third of their host cost (one lock, one set of
 * small-array look-ups). */
WORLD_HIP_API int world_hip_analyze_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x, int x_stride,
                                          const int *x_length, const HarvestOption *harvest_option,
                                          const CheapTrickOption *cheaptrick_option, const D4COption *d4c_option,
                                          int f_stride, double *d_tpos, double *d_f0, double *d_spectrogram,
                                          double *d_aperiodicity);
/* Harvest + CheapTrick + D4C of one batch written STRAIGHT into packed records: utterance u's frames occupy rows
 * first_row + sum_{v<u} n_frames[v] ... of d_block ([rows][cols] doubles); n_frames[u] = GetSamplesForHarvest(fs,
 * x_length[u], frame_period).  `cols` names the record format (world_hip_record_columns):
 *   wire 0, cols = 2 + 2 nb : [tpos, f0, sp f64[nb], ap f64[nb]]                       nb = fft_size/2 + 1
 *   wire 1, cols = 2 + nb   : [tpos, f0, sp f32[nb], ap f32[nb]]  -- half the bytes for the multi-GPU exchange and the
 *                             D2H copy; the values are the f64 results rounded once to float (6e-8 relative, the
 *                             contract is 1e-4); tpos and f0 stay f64.
 * The stage kernels store their rows at the records' stride, so no pack pass runs (world_hip_pack_results is for results
 * that already exist in the dense layout).  Same stream semantics as the *_batch calls. */
WORLD_HIP_API int world_hip_record_columns(int fft_size, int wire);
WORLD_HIP_API int world_hip_analyze_packed(WorldHipContext *ctx, int n_utt, int fs, const double *d_x, int x_stride,
                                           const int *x_length, const HarvestOption *harvest_option,
                                           const CheapTrickOption *cheaptrick_option, const D4COption *d4c_option,
                                           long long first_row, double *d_block, int cols);
/* The CODED wire format (the coders exist to "shrink the all-gather and D2H by 10-17x"): the same analysis,
 * its records coded before anything leaves the device --
 *   [tpos, f0, mel-cepstrum[number_of_dimensions], band aperiodicity[GetNumberOfAperiodicities(fs)]]   (doubles)
 * = CodeSpectralEnvelope() / CodeAperiodicity() (reference src/codec.cpp:268-297, :217-236) of exactly the spectrogram and
 * aperiodicity a dense call returns: 67 doubles = 536 bytes per frame at 48 kHz with 60 coefficients against 16 416
 * (31 x fewer bytes on the xGMI links and in the D2H copy).  cols = world_hip_coded_columns(fs, number_of_dimensions).  The
 * full records of the batch live in a staging block the context owns (device memory only) and are read once by the coders.
 * Lossy by design -- what the reference's own coder loses -- and therefore opt-in (world_amd.distributed: wire="coded"). */
WORLD_HIP_API int world_hip_coded_columns(int fs, int number_of_dimensions);
WORLD_HIP_API int world_hip_analyze_coded(WorldHipContext *ctx, int n_utt, int fs, const double *d_x, int x_stride,
                                          const int *x_length, const HarvestOption *harvest_option,
                                          const CheapTrickOption *cheaptrick_option, const D4COption *d4c_option,
                                          int number_of_dimensions, long long first_row, double *d_block, int cols);
/* Frame ranges (frame-level sharding of ONE long utterance -- CheapTrick / D4C only, F0 broadcast; the
 * reference's frames are independent given F0: src/cheaptrick.cpp:207-216, src/d4c.cpp:378-400).  The stages' rows of
 * frames [frame_lo, frame_hi) of every utterance of the batch; the positions in the reference's randn() stream are those of
 * a whole-utterance call (the offset scans, and D4C's LoveTrain pass on which its second scan depends, always cover every
 * frame), so a range's rows are BIT-IDENTICAL to the same rows of the full call.
 *   _spectral_packed_range: CheapTrick + D4C given tpos / f0 ([n_utt][f_stride], device) straight into packed records (same
 *       formats as world_hip_analyze_packed): utterance u's range starts at row first_row + sum over v < u of v's frames in range;
 *   _cheaptrick_batch_range / _d4c_batch_range: one stage into the dense arrays of the *_batch calls (rows outside the range
 *       untouched).
 * reuse_offsets != 0 (all three): an earlier call of the stage on this context had the same shape, buffers and options and
 * only the range differs -- its offsets / LoveTrain results are still in the workspace and are not recomputed (LoveTrain
 * over all frames is a seventh of a whole analysis: a rank that walks its frames in S sub-ranges would repeat it S times).
 * CheapTrick's and D4C's prepared arrays occupy disjoint parts of the workspace, so ranges of the two stages may
 * alternate.  The context remembers what the arrays were prepared FOR (shape, the x / tpos / f0 pointers, lengths, options,
 * the workspace's identity); a call that asks for reuse without matching -- another stage (Harvest, DIO, StoneMask, a coder,
 * Synthesis) ran in between, a different shape, a regrown workspace -- fails with a message instead of reading whatever
 * lies there (the CONTENT of the caller's f0 / x buffers is the caller's promise: the library compares pointers). */
WORLD_HIP_API int world_hip_spectral_packed_range(WorldHipContext *ctx, int n_utt, int fs, const double *d_x, int x_stride,
                                                  const int *x_length, const int *n_frames, int f_stride,
                                                  const double *d_tpos, const double *d_f0,
                                                  const CheapTrickOption *cheaptrick_option, const D4COption *d4c_option,
                                                  int frame_lo, int frame_hi, int reuse_offsets, long long first_row,
                                                  double *d_block, int cols);
WORLD_HIP_API int world_hip_cheaptrick_batch_range(WorldHipContext *ctx, int n_utt, int fs, const double *d_x, int x_stride,
                                                   const int *x_length, const int *n_frames, int f_stride,
                                                   const double *d_tpos, const double *d_f0, const CheapTrickOption *option,
                                                   int frame_lo, int frame_hi, int reuse_offsets, double *d_spectrogram);
WORLD_HIP_API int world_hip_d4c_batch_range(WorldHipContext *ctx, int n_utt, int fs, const double *d_x, int x_stride,
                                            const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                                            const double *d_f0, int fft_size, const D4COption *option, int frame_lo,
                                            int frame_hi, int reuse_offsets, double *d_aperiodicity);
WORLD_HIP_API int world_hip_pack_results(WorldHipContext *ctx, int n_utt, const int *n_frames, int f_stride,
                                         int bins, const double *d_tpos, const double *d_f0,
                                         const double *d_spectrogram, const double *d_aperiodicity,
                                         long long first_row, double *d_block);
WORLD_HIP_API int world_hip_unpack_results(WorldHipContext *ctx, int n_utt, const int *n_frames, int f_stride,
                                           int bins, const double *d_block, long long first_row, double *d_tpos,
                                           double *d_f0, double *d_spectrogram, double *d_aperiodicity);
WORLD_HIP_API int world_hip_allgather_blocks(int n_dev, WorldHipContext *const *ctxs, const double *const *d_src,
                                             const long long *rows, int cols, double *const *d_dst);

/* ONE process driving n_dev GPUs (one context each; host side in C/C++, no torch, no RCCL): Harvest + CheapTrick + D4C of
 * a whole job of utterances in HOST memory, sharded longest-first over the devices.  One host thread per device uploads
 * its share in sub-batches of `sub_batch` utterances and analyses each straight into packed records; every other device
 * pulls a finished sub-batch's rows over xGMI (peer copies on its own exchange stream) while the next one is analysed.
 * d_blocks[d]: device d's buffer of rows_capacity x cols doubles, cols = 2 + 2 (fft_size/2 + 1); on return every device
 * holds ALL records at the same rows, where[3 i .. 3 i + 2] = {device index that analysed utterance i, its first row,
 * its frame count}.  Blocking (the inputs are host memory); 0 on success, else world_hip_last_error(). */
WORLD_HIP_API int world_hip_analyze_sharded(int n_dev, WorldHipContext *const *ctxs, int n_utt, int fs,
                                            const double *const *x, const int *x_length,
                                            const HarvestOption *harvest_option, const CheapTrickOption *cheaptrick_option,
                                            const D4COption *d4c_option, int sub_batch, double *const *d_blocks,
                                            long long rows_capacity, int cols, long long *where);

/* Shape limits of the GPU path (the reference has none): 0 = StoneMask, CheapTrick(cheaptrick_fft_size) and D4C all run at
 * this fs; 1 = one of them does not, `why` names the stage and the limit (fs <= 192 kHz for D4C, CheapTrick fft_size <=
 * 8192 -- its default up to fs = 192 kHz --, fs >= 15.8 kHz for D4C, fs <= 240 kHz for StoneMask).  Pure host
 * arithmetic.  The drop-in symbols make the same check before any GPU work and report through the error handler
 * (world_hip_set_error_handler; by default: message + abort -- the reference API has no error channel). */
WORLD_HIP_API int world_hip_check_shape(int fs, int cheaptrick_fft_size, char *why, int why_capacity);

/* HIP graphs: the batched calls enqueued on ctx between _begin and _end are captured into ONE executable graph (bound to
 * the device buffers they were given) instead of being run; _launch replays it on the context's stream at the cost of one
 * host launch (a Harvest + CheapTrick + D4C job is ~45 kernel launches otherwise).  Every call shape must have run once
 * before capture (a captured call may not allocate, copy from the host or wait); an error inside a capture invalidates it.
 * A graph holds raw pointers into memory the CONTEXT owns (workspace arena, small per-call arrays, cached tables).  If a
 * later eager call on the same context has to reallocate any of it (a larger batch, another option set or sampling
 * rate), the graph is stale: world_hip_graph_launch then FAILS (world_hip_last_error: "stale graph") instead of
 * replaying -- capture the job again.  Smaller or equal shapes never invalidate a graph. */
WORLD_HIP_API int world_hip_graph_begin(WorldHipContext *ctx);
WORLD_HIP_API int world_hip_graph_end(WorldHipContext *ctx, void **graph);
WORLD_HIP_API int world_hip_graph_launch(WorldHipContext *ctx, void *graph);
WORLD_HIP_API int world_hip_graph_destroy(void *graph);

WORLD_HIP_API int world_hip_set_synthesis_pulse_capacity(WorldHipContext *ctx, int pulses_per_utterance);
WORLD_HIP_API int world_hip_synthesis_pulses_dropped(WorldHipContext *ctx, int *needed);

/* 16-bit PCM (as stored in a WAV file) -> the doubles the reference's wavread() produces,
 * x = q / 32768 (tools/audioio.cpp:236-249), on the device: upload int16, not FP64. */
WORLD_HIP_API int world_hip_pcm16_to_double(WorldHipContext *ctx, long long n, const short *d_pcm, double *d_x);

/* The general form of the above for a WAV file's data bytes (nbit/8 = 1..4 bytes per sample, little
 * endian, decoded exactly as wavread() does), its inverse for 16-bit output as wavwrite() quantises,
 * and the host-side header parse a batch tool needs to find those bytes:
 *   world_hip_wav_layout() returns 1 and fills fs / nbit / x_length / data_offset (bytes from the
 *   start of the file), 0 if the file cannot be opened, -1 if wavread() would reject it. */
WORLD_HIP_API int world_hip_pcm_to_double(WorldHipContext *ctx, long long n, int nbit, const void *d_pcm, double *d_x);
WORLD_HIP_API int world_hip_double_to_pcm16(WorldHipContext *ctx, long long n, const double *d_x, short *d_pcm);
WORLD_HIP_API int world_hip_wav_layout(const char *filename, int *fs, int *nbit, int *x_length,
                                       long long *data_offset);
/* Host-side writer for samples already quantised (e.g. by world_hip_double_to_pcm16 and one D2H of
 * int16): wavwrite()'s 44-byte header + the samples.  Returns 1 on success, 0 if the file cannot be written. */
WORLD_HIP_API int world_hip_wav_write_pcm16(const char *filename, int fs, long long n, const short *pcm);

/* Sampling-rate conversion on the device: [n_utt][x_stride] doubles at fs_in -> [n_utt][y_stride] doubles
 * at fs_out, by a polyphase Kaiser-windowed sinc.  The reference has no resampler (its decimate() is Harvest's integer-ratio
 * IIR, its interp1() is linear); THIS COMMENT IS THE RULE, and the kernel is held to it bit for bit.
 * g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g, B = max(L, M); all index arithmetic in 64-bit integers.
 *   length.  world_hip_resample_length(n_in, fs_in, fs_out) = ceil(n_in * L / M); -1 for a count or a rate below 1 or a
 *            result above INT_MAX.  Utterance u gets n_out[u] = that of x_length[u]; y_stride must hold it.
 *   grid.    Output sample m lies at the input time m * M / L: k0 = (m * M) div L, p = (m * M) mod L.
 *   option.  zeros = zero crossings of the sinc on each side (in units of the lower rate's samples), rolloff = the cut-off as
 *            a fraction of the lower Nyquist rate, kaiser_beta = the window's shape.  world_hip_resample_option fills a preset
 *            (any other quality value: BEST); a NULL option in any call means BEST.
 *              WORLD_HIP_RESAMPLE_BEST  {64, 0.9475937167399596, 14.769656459379492}
 *              WORLD_HIP_RESAMPLE_FAST  {16, 0.85, 8.555504641634386}
 *   taps.    W = ceil(zeros * B / L) taps on each side, 2 W in all.  Tap i = 0 .. 2 W - 1 reads input sample
 *            k = k0 - W + 1 + i with the coefficient c[p][i] = h(q), q = p + (W - 1 - i) * L: the distance between the output
 *            time and sample k in units of 1 / L sample, an integer.  h(q) is exactly 0.0 where |q| >= zeros * B; otherwise
 *              h(q) = s * sinc(rolloff * q / B) * I0(kaiser_beta * sqrt(1 - u * u)) / I0(kaiser_beta),
 *              u = q / (zeros * B),  s = rolloff * min(L, M) / M,  sinc(x) = sin(pi x) / (pi x),  sinc(0) = 1.
 *            The phases are not renormalised.  The table is made on the host (evaluated in long double, every entry rounded
 *            once to double); world_hip_resample_taps returns it as [L][2 W] (row p), the very doubles the device uses.
 *   sum.     y[m] = x[k] * c[p][i] summed over i = 0 .. 2 W - 1 in ascending i, starting from +0.0, the multiplication and
 *            the addition each rounded on its own (no fused multiply-add).  A sample outside [0, x_length[u]) counts as +0.0.
 *            So the result depends on nothing but the row: not on the batch, the launch shape or a graph replay; a NaN or
 *            an Inf sample spreads to the outputs whose 2 W taps reach it (times-zero coefficients included) and no further.
 *   equal rates.  fs_in == fs_out copies every row's x_length[u] samples bit for bit; no filter is involved.
 * Samples at or beyond n_out[u] are never written.  Refused, before any GPU work and with nothing written: n_utt < 1, a NULL
 * pointer, a length below 1 or above x_stride, y_stride below an n_out[u], a rate below 1, zeros outside [1, 256], rolloff
 * outside (0, 1], kaiser_beta not finite or outside [0, 40], 2 W > 4096, L * 2 W > 2^21 coefficients (rates without a large
 * common divisor, such as 44100 -> 48001: the message names L), an output range that overlaps the input range.
 * world_hip_resample_option / _length / _shape / _taps are host arithmetic and need no GPU; _shape and _taps return 0, or 1
 * with the reason in world_hip_last_error.  world_hip_resample_batch: stream order and errors as the other batched calls;
 * x_length goes through the context's small-array store and the coefficient table stays with the context's device tables
 * (a few (fs_in, fs_out, option) keys are kept; world_hip_workspace_bytes counts them), so after one eager call of a shape
 * the call neither allocates nor copies from the host nor waits, and can be captured. */
#define WORLD_HIP_RESAMPLE_BEST 0
#define WORLD_HIP_RESAMPLE_FAST 1
typedef struct { int zeros; double rolloff; double kaiser_beta; } WorldHipResampleOption;
WORLD_HIP_API void world_hip_resample_option(int quality, WorldHipResampleOption *opt);
WORLD_HIP_API int world_hip_resample_length(int n_in, int fs_in, int fs_out);
WORLD_HIP_API int world_hip_resample_shape(int fs_in, int fs_out, const WorldHipResampleOption *opt, int *L, int *M, int *W);
WORLD_HIP_API int world_hip_resample_taps(int fs_in, int fs_out, const WorldHipResampleOption *opt, double *table /* host, [L][2W] */);
WORLD_HIP_API int world_hip_resample_batch(WorldHipContext *ctx, int n_utt, int fs_in, int fs_out,
                                           const WorldHipResampleOption *opt, const double *d_x, int x_stride,
                                           const int *x_length /* host */, double *d_y, int y_stride);

/* Mel-cepstra by all-pass frequency warping on the device: SPTK's freqt with a constant alpha, what users of a WORLD
 * binding call sp2mc / mc2sp.  (The coders below are the reference's own: a DCT of the log envelope on a mel axis, a
 * different transform with different numbers.)  The reference has no such function; THIS COMMENT IS THE RULE.
 * N = fft_size, H = N / 2, K = H + 1 bins, P = order + 1 coefficients; w_0 = w_H = 1/2 and w = 1 otherwise.
 *   encode (sp2mc).  mc_m = sum over k of M[m][k] ln sp_k, M = A F.
 *            F[n][k] = (2 / N) w_n w_k cos(pi n k / H): c = F ln sp is the one-sided cepstrum, ln sp_k = 2 sum_n c_n
 *            cos(pi n k / H) exactly.  A[m][n] is freqt applied to unit vectors:
 *              A[0][0] = 1, A[m][0] = 0 for m > 0;  A[0][n] = alpha A[0][n-1];
 *              A[1][n] = (1 - alpha^2) A[0][n-1] + alpha A[1][n-1];
 *              A[m][n] = A[m-1][n-1] + alpha (A[m][n-1] - A[m-1][n]) for m >= 2.
 *   decode (mc2sp).  sp_k = exp(sum over m of D[k][m] mc_m), D[k][m] = 2 cos(m w~_k),
 *            w~_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k), w_k = pi k / H: H(z) = exp sum mc_m z~^-m, sp = |H|^2
 *            (SPTK's convention).  With alpha = 0 encode is plain cepstral truncation.
 *   tables.  Both are made on the host in long double and rounded once to double; world_hip_mcep_tables returns them,
 *            M as [P][K] and D as [K][P] (either may be NULL), the very doubles the device multiplies by.  (The rows of M
 *            are cosine transforms of the rows of A and are made by a long-double FFT: milliseconds at any shape.)
 *   alpha.   world_hip_mcep_alpha(fs) = i / 1000 for the first i in [0, 999] that minimises the RMS, over w_j = pi j / 1000,
 *            j = 0 .. 999, of the difference between ln(1 + (fs / 2000) j / 1000) and w_j + 2 atan2(alpha sin w_j,
 *            1 - alpha cos w_j), each divided by its value at j = 999: 0.41 at 16 kHz, 0.554 at 48 kHz.  NaN for fs < 1.
 *   sums.    Each output is a sum over ascending k (m) on the FP64 matrix unit; a row's result depends on nothing but the
 *            row: not on the batch, the row's position, the launch shape or a graph replay.
 * Strides are counted in doubles: d_block + 2 with world_hip_record_columns(fft_size, 0) reads the envelopes of packed f64
 * records where they lie, and a stride above P writes the coefficients into records of the caller's.  Doubles of an output
 * row beyond P (K for mc2sp) and rows beyond `rows` are never written.  Refused, before any GPU work and with nothing written:
 * rows < 1, a NULL pointer, fft_size not a power of two in [128, 8192], order outside [0, min(H, 255)], alpha not finite or
 * |alpha| > 0.9, a stride shorter than the row, an output range that overlaps the input range.  A row with a non-finite or
 * non-positive envelope bin yields an unspecified row (it may be NaN); no other row changes.
 * world_hip_mcep_alpha / _tables are host arithmetic and need no GPU; _tables returns 0, or 1 with the reason in
 * world_hip_last_error.  world_hip_sp2mc / _mc2sp: stream order and errors as the other batched calls; a direction's table
 * stays with the context's device tables (a few (fft_size, order, alpha) keys are kept; world_hip_workspace_bytes counts
 * them), so after one eager call of a shape the call neither allocates nor copies from the host nor waits, and can be
 * captured. */
WORLD_HIP_API double world_hip_mcep_alpha(int fs);
WORLD_HIP_API int world_hip_mcep_tables(int fft_size, int order, double alpha, double *M /* host, [P][K] */,
                                        double *D /* host, [K][P] */);
WORLD_HIP_API int world_hip_sp2mc(WorldHipContext *ctx, int rows, int fft_size, int order, double alpha, const double *d_sp,
                                  long long sp_row_stride, double *d_mc, long long mc_row_stride);
WORLD_HIP_API int world_hip_mc2sp(WorldHipContext *ctx, int rows, int fft_size, int order, double alpha, const double *d_mc,
                                  long long mc_row_stride, double *d_sp, long long sp_row_stride);

/* Dynamic features (delta, delta-delta) and maximum-likelihood parameter generation (MLPG) on the device: what a TTS or
 * voice-conversion stack puts between the statics and an acoustic model, and between the model and the synthesiser.  The
 * reference has no such function; THIS COMMENT IS THE RULE.
 * An utterance u has T = n_frames[u] frames (host array), a stream `dim` = D static dimensions.  There are n_win windows,
 * 1 <= n_win <= 4, all of half-width L = half_width in {0, 1, 2}, given as host doubles win[n_win][2 L + 1] (zeros at the
 * ends are allowed).  Window 0 must be the identity, 1 at tau = 0 and 0 elsewhere: the system below is then positive
 * definite whenever every static variance is positive.  The usual set is [0 1 0], [-0.5 0 0.5], [1 -2 1].  d_mask[u][t]
 * (bytes, mask_utt_stride bytes between utterances; non-zero = present; NULL: every frame is present) marks the frames
 * that exist: the unvoiced frames of an .lf0 stream are the masked ones.
 *   coupling.  A term (t, tau) COUNTS when every frame from t to t + tau inclusive lies inside the utterance and is
 *            present.  Every maximal run of present frames is therefore handled exactly as an utterance of its own, its
 *            windows truncated at its ends (the band-matrix convention of Merlin / nnmnkwii).
 *   deltas (world_hip_delta_batch).  For a present frame t,
 *              o[t][w D + d] = sum over tau = -L .. L, (t, tau) counts, of win[w][tau] c[t + tau][d],
 *            in ascending tau from +0.0, every product and every sum rounded (no FMA).  For a masked frame all n_win D
 *            outputs are `fill`.  Masked rows of d_c are never read.
 *   generation (world_hip_mlpg_batch).  For each (u, d) independently, c[.][d] over the present frames minimises
 *              sum over present t, over w, of p[t][w D + d] (mu[t][w D + d] - sum over tau, (t, tau) counts, of
 *                                                            win[w][tau] c[t + tau][d])^2,
 *            p = 1 / variance, or the given value itself where `precision` is non-zero: the system R c = r, R = W' P W,
 *            r = W' P mu, R symmetric positive definite with half-bandwidth 2 L.  It is solved by a banded L D L' without
 *            pivoting or square roots in double precision.  Masked frames of the output get `fill`; masked rows of d_mean
 *            and d_var are never read.
 *   layouts.  Strides are counted in doubles.  d_mean[u][t][n_win D]: utterance stride and row stride >= n_win D; d_var
 *            the same, where a row stride of 0 means one row per utterance and an utterance stride of 0 as well one global
 *            row (the common case).  d_c[u][t][D], d_out[u][t][D] (generation) or [u][t][n_win D] (deltas) have strides of
 *            their own.  Doubles beyond a row's extent and rows at or beyond n_frames[u] are never written.
 *   data.     A variance (precision) in a present frame that is not finite and positive makes that (u, d) column
 *            unspecified (it may be NaN); no other column changes, the call returns and the next call is unaffected.
 *   determinism.  A column's result depends on nothing but that column's data, T, the mask and the windows: not on the
 *            batch, the column's position, the strides, the launch shape or a graph replay.
 * Refused, before any GPU work and with nothing written (1 is returned, the reason is in world_hip_last_error): n_utt < 1,
 * dim < 1, any n_frames[u] < 1, a NULL win / n_frames / d_c / d_mean / d_var / d_out, n_win outside [1, 4], half_width
 * outside [0, 2], a window coefficient that is not finite, window 0 not the identity, a row stride shorter than the row (a 0
 * stride of d_var excepted), a negative utterance stride, utterances of the output (or of the mask) that run into each
 * other, an output range that overlaps an input range, n_win dim above INT_MAX or more than 2^38 elements (frames x dim)
 * in one utterance.
 * Stream order and errors as the other batched calls.  The generation keeps the factor and the scaled right-hand side,
 * [max T][2 L + 1][n_utt D] doubles, in the context's workspace (world_hip_workspace_bytes counts it; none for L = 0 or
 * for the deltas); once the workspace has the size a call neither allocates nor waits and can be captured, and a capture
 * goes stale when the workspace grows, as for the other batched calls. */
WORLD_HIP_API int world_hip_delta_batch(WorldHipContext *ctx, int n_utt, int dim, int n_win, int half_width,
                                        const double *win /* host, [n_win][2 half_width + 1] */, const int *n_frames /* host */,
                                        const unsigned char *d_mask, long long mask_utt_stride, const double *d_c,
                                        long long c_utt_stride, long long c_row_stride, double fill, double *d_out,
                                        long long out_utt_stride, long long out_row_stride);
WORLD_HIP_API int world_hip_mlpg_batch(WorldHipContext *ctx, int n_utt, int dim, int n_win, int half_width,
                                       const double *win /* host, [n_win][2 half_width + 1] */, const int *n_frames /* host */,
                                       const unsigned char *d_mask, long long mask_utt_stride, const double *d_mean,
                                       long long mean_utt_stride, long long mean_row_stride, const double *d_var,
                                       long long var_utt_stride, long long var_row_stride, int precision, double fill,
                                       double *d_out, long long out_utt_stride, long long out_row_stride);

/* Joint-density Gaussian mixture on the device: the acoustic model of classic voice conversion (Stylianou 1998; Kain 1998;
 * Toda, Black, Tokuda 2007), fitted on aligned joint rows [x, y] and used to turn source rows x into the per-frame means
 * and variances of y that world_hip_mlpg_batch consumes.  The reference has no such function; THIS COMMENT IS THE RULE.
 * A model has M mixtures, 1 <= M <= 256, a source part of Dx dimensions, 1 <= Dx <= 128, a target part of Dy dimensions,
 * 0 <= Dy <= 128, P = Dx + Dy, and the host parameters w[M], mu[M][P], cov[M][P][P]; cov is symmetric and only its lower
 * triangle is read.
 *   prepare (host, no GPU).  world_hip_gmm_prepare computes per mixture, in long double, each value rounded once to double:
 *            the Cholesky factor Sxx = L L'; U = L^-1 (lower triangular); c = ln w - Dx / 2 ln 2 pi - sum ln L_ii;
 *            A = Syx Sxx^-1 [Dy][Dx]; v = diag(Syy - A Sxy) [Dy]; mu_x and mu_y as they are.  It returns 1, the reason
 *            naming the mixture, when a weight is not finite and positive, a pivot is not finite and positive, or an entry of
 *            v is not positive.  `model` takes world_hip_gmm_model_doubles(M, Dx, Dy) doubles (-1 for a refused shape), which
 *            the caller copies to the device; the layout is the library's (every matrix padded with zeros to the matrix
 *            unit's 16-wide tiles, so that no padded operand is ever anything but a zero).  world_hip_gmm_model_parts hands
 *            back the very doubles the device multiplies by: c[M], mux[M][Dx], muy[M][Dy], U[M][Dx][Dx], A[M][Dy][Dx],
 *            v[M][Dy]; any pointer may be NULL.
 *   convert (world_hip_gmm_convert).  Per row t of d_x [rows][Dx] and mixture m:
 *              d = x_t - mu_x (rounded);  z = U d;  q_tm = c_m - 1/2 sum z^2;  e_tm = mu_y + A d;
 *              q_max = the largest q_tm, m^ the lowest m that attains it;  s = sum over ascending m of exp(q_tm - q_max);
 *              loglik_t = q_max + ln s;  gamma_tm = exp(q_tm - q_max) / s  (= exp(q_tm - loglik_t), and a distribution
 *              however far the row lies from every mixture: the largest term of s is 1).
 *            mode 0 (the mixture, moment-matched): mean = sum over ascending m of gamma e, var = sum of gamma (v + e^2)
 *            - mean^2.  mode 1 (the single most likely component, Toda's sub-optimum sequence): mean = e of m^, var = v of
 *            m^.  Each matrix product is a sum over the ascending inner index on the FP64 matrix unit; sum z^2 adds, for
 *            each j mod 16, the squares in ascending j and then the sixteen partial sums in ascending order.
 *            d_mean and d_var are [rows][Dy], d_post [rows][M], d_loglik [rows]; each of the four may be NULL.  With
 *            Dy = 0 d_mean and d_var must be NULL and the call is the E-step of a Dx-dimensional mixture.  With x carrying
 *            static + delta (+ delta-delta) features d_mean / d_var are world_hip_mlpg_batch's with precision = 0.
 *            A row's outputs depend on nothing but the row and the model: not on `rows`, the row's position, the strides,
 *            the launch shape or a graph replay.  A row with an entry that is not finite yields an unspecified row and no
 *            other row changes.  Doubles beyond a row's extent and rows at or beyond `rows` are never written.
 *   statistics (world_hip_gmm_accumulate).  With gamma = d_post [rows][M], z = d_z [rows][P] and the shift s = d_shift [M][P]:
 *              N_m = sum_t gamma_tm;  S1_m = sum_t gamma_tm (z_t - s_m);  G_m = sum_t (gamma_tm (z_t - s_m)) (z_t - s_m)',
 *            z - s and gamma (z - s) each rounded, every sum one accumulator on the matrix unit that runs over t ascending
 *            from the first row to the last, whatever the launch shape; G is written full and bit-symmetric.  The shift is
 *            the mixture's current mean: it keeps the later G / N - delta delta' free of cancellation.  The statistics of
 *            two shards (under the same shift) add.
 *   update (host).  world_hip_gmm_update, in long double rounded once: w = N / total_rows, delta = S1 / N, mu = s + delta,
 *            cov = G / N - delta delta' + reg I.  It returns 1, naming the mixture, when some N_m is below P + 1 (a starved
 *            component); nothing is written then.
 *   fit (world_hip_gmm_fit).  n_iter times: prepare (Dx = P, Dy = 0), the model copied up, convert for gamma and loglik,
 *            accumulate under the shift mu, the statistics copied down, update.  loglik[i] is the mean log-likelihood BEFORE
 *            update i: the sum of loglik_t over ascending t in long double, divided by rows, rounded once.  It waits for
 *            the device every iteration and cannot be captured.  On a refusal from prepare or update it returns 1 and leaves
 *            w, mu, cov as after the last completed iteration.
 *   init (world_hip_gmm_init).  w = 1 / M; mu_m = row floor((2 m + 1) rows / (2 M)); cov_m = the diagonal of the data's
 *            global variance: one accumulate with M = 1, gamma = 1 and the shift equal to row 0, then update with reg = 0.
 * Strides are counted in doubles.  Refused, before any GPU work and with nothing written (1 is returned, the reason is in
 * world_hip_last_error): a NULL where a pointer is required, M, Dx, Dy, P or rows out of range, a stride shorter than its row,
 * mode outside {0, 1}, d_mean or d_var given with Dy = 0, an output range that overlaps an input, the model or another
 * output, reg negative or not finite, n_iter < 1.
 * _model_doubles / _prepare / _model_parts / _update are host arithmetic and need no GPU.  convert and accumulate: stream
 * order and errors as the other batched calls.  convert keeps q and gamma, [rows][M] doubles, and m^, [rows] ints, in the
 * context's workspace (world_hip_workspace_bytes counts it); once the workspace has the size the call neither allocates nor
 * copies from the host nor waits, and can be captured.  accumulate needs no workspace.
 * Time (one MI355X; tools/gmm_bench.py; 10^5 rows, Dx = Dy = 50, M = 64): convert 6.6 ms in either mode; on the joint rows
 * (P = 100) the E-step 6.8 ms, accumulate 15.1 ms, one iteration of fit 77 ms by the wall clock, most of it the host's
 * long-double prepare and update and the copies. */
WORLD_HIP_API long long world_hip_gmm_model_doubles(int M, int Dx, int Dy);
WORLD_HIP_API int world_hip_gmm_prepare(int M, int Dx, int Dy, const double *w, const double *mu, const double *cov,
                                        double *model /* host */);
WORLD_HIP_API int world_hip_gmm_model_parts(int M, int Dx, int Dy, const double *model /* host */, double *c, double *mux,
                                            double *muy, double *U, double *A, double *v);
WORLD_HIP_API int world_hip_gmm_convert(WorldHipContext *ctx, int M, int Dx, int Dy, const double *d_model, int rows,
                                        const double *d_x, long long x_row_stride, int mode, double *d_mean,
                                        long long mean_row_stride, double *d_var, long long var_row_stride, double *d_post,
                                        long long post_row_stride, double *d_loglik);
WORLD_HIP_API int world_hip_gmm_accumulate(WorldHipContext *ctx, int M, int P, int rows, const double *d_z,
                                           long long z_row_stride, const double *d_post, long long post_row_stride,
                                           const double *d_shift /* [M][P] */, double *d_N /* [M] */, double *d_S1 /* [M][P] */,
                                           double *d_G /* [M][P][P] */);
WORLD_HIP_API int world_hip_gmm_update(int M, int P, const double *N, const double *S1, const double *G, const double *shift,
                                       double total_rows, double reg, double *w, double *mu, double *cov);
WORLD_HIP_API int world_hip_gmm_fit(WorldHipContext *ctx, int M, int P, int rows, const double *d_z, long long z_row_stride,
                                    int n_iter, double reg, double *w, double *mu, double *cov /* host, in-out */,
                                    double *loglik /* host, [n_iter] or NULL */);
WORLD_HIP_API int world_hip_gmm_init(WorldHipContext *ctx, int M, int P, int rows, const double *d_z, long long z_row_stride,
                                     double *w, double *mu, double *cov /* host, out */);

/* Training rows of a voice-conversion corpus on the device: the step between world_hip_align_batch and world_hip_gmm_fit.
 * A power gate drops the silent frames of every utterance, an ordered compaction turns the decisions into frame numbers, a
 * gather makes the kept frames adjacent rows (so that all pairs of a corpus go into ONE world_hip_align_batch call), and a
 * second gather builds the joint rows [x, y] along the paths.  The reference has no such function; THIS COMMENT IS THE RULE.
 *   power (world_hip_frame_power_batch).  Utterance u has n_frames[u] envelope rows of K = fft_size / 2 + 1 doubles at
 *            d_sp + u sp_utt_stride + t sp_row_stride.  With N = fft_size,
 *              P_t = ((sp[0] + sp[N/2]) + 2 S) / N,   S = the sum of sp[1 .. N/2 - 1]   (the mean of the N-point spectrum),
 *              mean_u = (sum over t of P_t) / n_frames[u].
 *            Both sums have one order: 64 partial sums, partial j adding from +0.0 the terms whose index (the bin k, the
 *            frame t) is congruent to j modulo 64, in ascending index; then, for s = 32, 16, 8, 4, 2, 1 in turn, partial j
 *            takes partial j + s for every j < s; partial 0 is the sum.  Every addition is rounded on its own, 2 S is exact.
 *            d_power [u][t] (power_utt_stride doubles apart) and d_mean [u]; either may be NULL.
 *   selection (world_hip_select_frames_batch).  Frame t of utterance u is KEPT if
 *              (d_mask == NULL or mask[u][t] != 0) and v_t >= threshold * scale_u,
 *            v_t the double at d_value + u value_utt_stride + t value_stride (a vector with value_stride = 1, or a column of a
 *            record where it lies), scale_u = d_scale[u], or 1 when d_scale is NULL; the product is rounded once.  A NaN on
 *            either side of the comparison keeps nothing.  Outputs, each may be NULL: d_index [u][i] (ints, index_utt_stride
 *            apart) the kept frames' numbers in ascending order; d_count [u]; d_keep [u][t] (bytes, keep_utt_stride apart)
 *            0 / 1, the mask format world_hip_delta_batch and world_hip_mlpg_batch read.  An utterance may have any number
 *            of frames.
 *   gather (world_hip_gather_rows_batch).  out[u][i][0 .. dim) = in[u][index[u][i]][0 .. dim) for i < n_out[u]; n_src[u]
 *            (the rows utterance u of d_in has) and n_out are HOST arrays, the indices live on the device.
 *   joint rows (world_hip_joint_rows_batch).  For pair u and step k < path_len[u] (HOST array; d_path [u][p_stride][2] as
 *            world_hip_align_batch writes it): (i, j) = d_path[u][k]; i' = d_sel_a ? sel_a[u][i] : i, j' likewise from
 *            d_sel_b (selections are ints, sel_*_stride apart, n_sel_*[u] of them: HOST arrays, required with a selection).
 *            Row z_row[u] + k of d_z is the dim_a doubles of A's row a_row[u] + i' followed by the dim_b doubles of B's row
 *            b_row[u] + j'.  a_row, b_row, z_row are HOST arrays with the meaning of world_hip_align_batch's; z_row is the
 *            caller's prefix sum of the path lengths (any rows that keep the pairs apart will do).  dim_b = 0 is allowed
 *            (d_b, b_row, n_b are then not looked at).
 *   copies.   Both gathers copy bits (a NaN keeps its payload).  Strides are counted in doubles and are arbitrary beyond
 *            the row: a source may sit at column 2 or 3 of a record, so pointers are 8-byte aligned and need not be 16-byte
 *            aligned.
 *   never written.  Index entries at or beyond count[u], index and keep entries at or beyond n_frames[u], power entries at or
 *            beyond n_frames[u], doubles beyond a row's extent and rows at or beyond n_out[u] / path_len[u].
 *   data.     Index values cannot be refused before the launch.  A gather index outside [0, n_src[u]) writes that row as
 *            `fill`; in the joint rows an i or j outside the selection's length (or the side's frame count without one) or
 *            an i' or j' outside [0, n_a[u]) / [0, n_b[u]) writes `fill` into that half of the row.  Nothing out of range is
 *            read and no other row changes.  A NaN envelope bin makes that frame's power (and the mean) NaN and nothing else.
 *   determinism.  An utterance's or pair's outputs depend on nothing but its own data and counts: not on the batch, its
 *            position in it, the strides, the launch shape or a graph replay.  The selection's outputs are integers.
 * Refused, before any GPU work and with nothing written (1 is returned, the reason is in world_hip_last_error): a count of
 * utterances or pairs below 1; any n_frames[u], n_src[u], n_out[u], n_a[u], n_b[u], n_sel[u] or path_len[u] below 1; a NULL
 * n_frames / d_sp, n_frames / d_value, n_src / n_out / d_in / d_index / d_out, or a / b (with dim_b > 0) / their row and count
 * arrays / path_len / d_path / z_row / d_z, a selection without its lengths; fft_size not a power of two in [128, 8192]; dim,
 * dim_a below 1 or dim_b below 0; dim_a + dim_b above INT_MAX / 8; a row stride shorter than its row; value_stride below 1; a
 * negative utterance stride or first row; path_len[u] above p_stride; utterances of an output (power, index, keep, the
 * gathered rows; a selection likewise) that run into each other, pairs of d_z that do; an output range that overlaps an input
 * range or another output.
 * Stream order and errors as the other batched calls.  After one eager call of a shape (the count arrays are found by content)
 * a call neither allocates nor copies from the host nor waits, and can be captured.  Workspace: only a mean without d_power,
 * [n_utt][max n_frames] doubles (world_hip_workspace_bytes counts it).
 * Time (one MI355X, 2026-10-20; tools/corpus_bench.py; 200 pairs of 540 to 600 frames a side, D = 50 statics, joint rows of
 * 200 doubles): all joint rows of the corpus through one align call and one joint_rows call 4.9 ms, against 210.8 ms for a
 * loop of one align call a pair with torch indexing (the same bits); by the launch, HIP events after a warm-up: frame_power
 * with its mean on 114 k rows of 513 bins 0.115 ms, select_frames 0.007 ms, gather_rows of the kept statics 0.018 ms,
 * joint_rows 0.072 ms (torch.index_select twice and torch.cat on the same tensors: 0.164 ms).  DESIGN.md 3.18. */
WORLD_HIP_API int world_hip_frame_power_batch(WorldHipContext *ctx, int n_utt, int fft_size, const int *n_frames /* host */,
                                              const double *d_sp, long long sp_utt_stride, long long sp_row_stride,
                                              double *d_power, long long power_utt_stride, double *d_mean);
WORLD_HIP_API int world_hip_select_frames_batch(WorldHipContext *ctx, int n_utt, const int *n_frames /* host */,
                                                const double *d_value, long long value_utt_stride, long long value_stride,
                                                double threshold, const double *d_scale, const unsigned char *d_mask,
                                                long long mask_utt_stride, int *d_index, long long index_utt_stride,
                                                int *d_count, unsigned char *d_keep, long long keep_utt_stride);
WORLD_HIP_API int world_hip_gather_rows_batch(WorldHipContext *ctx, int n_utt, int dim, const int *n_src /* host */,
                                              const double *d_in, long long in_utt_stride, long long in_row_stride,
                                              const int *n_out /* host */, const int *d_index, long long index_utt_stride,
                                              double fill, double *d_out, long long out_utt_stride, long long out_row_stride);
WORLD_HIP_API int world_hip_joint_rows_batch(WorldHipContext *ctx, int n_pairs, int dim_a, int dim_b, const double *d_a,
                                             const long long *a_row /* host */, const int *n_a /* host */, long long a_row_stride,
                                             const double *d_b, const long long *b_row /* host */, const int *n_b /* host */,
                                             long long b_row_stride, const int *path_len /* host */, const int *d_path,
                                             int p_stride, const int *d_sel_a, const int *n_sel_a /* host */,
                                             long long sel_a_stride, const int *d_sel_b, const int *n_sel_b /* host */,
                                             long long sel_b_stride, double fill, double *d_z, const long long *z_row /* host */,
                                             long long z_row_stride);

/* Coders on dense device rows (reference src/codec.cpp:217-324).  Rows are independent:
 *   spectrogram / aperiodicity  [rows][fft_size/2+1]
 *   coded spectral envelope     [rows][number_of_dimensions]
 *   coded aperiodicity          [rows][GetNumberOfAperiodicities(fs)]
 * A batch's [n_utt][f_stride][...] output of the calls above is one such array with
 * rows = n_utt * f_stride (padding rows must then hold finite positive values). */
WORLD_HIP_API int world_hip_code_spectral_envelope(WorldHipContext *ctx, int rows, int fs, int fft_size,
                                                   int number_of_dimensions, const double *d_spectrogram,
                                                   double *d_coded);
WORLD_HIP_API int world_hip_decode_spectral_envelope(WorldHipContext *ctx, int rows, int fs, int fft_size,
                                                     int number_of_dimensions, const double *d_coded,
                                                     double *d_spectrogram);
WORLD_HIP_API int world_hip_code_aperiodicity(WorldHipContext *ctx, int rows, int fs, int fft_size,
                                              const double *d_aperiodicity, double *d_coded);
WORLD_HIP_API int world_hip_decode_aperiodicity(WorldHipContext *ctx, int rows, int fs, int fft_size,
                                                const double *d_coded, double *d_aperiodicity);

/* Parameter modification between analysis and synthesis (reference test/test.cpp:221-258, ParameterModification), per
 * utterance, on the dense arrays of the *_batch calls (f0 [n_utt][f_stride], spectrogram [n_utt][f_stride][fft_size/2+1]):
 *   f0_scale        test.cpp's argv[3]: f0 *= f0_scale (the same multiply, bit for bit); 1 = unchanged; finite, >= 0
 *   formant_shift   test.cpp's argv[4]: every spectrogram row is stretched along frequency -- log, interp1 from the axis
 *                   ratio * i / fft_size * fs onto i / fft_size * fs, exp -- and, for ratio < 1, bins from
 *                   int(fft_size / 2.0 * ratio) up take the value of the bin below; 1 = the row untouched, bit for bit;
 *                   finite, > 0, fft_size / 2 * ratio >= 1
 *   convert_log_f0  1: before the scaling, voiced frames (finite and > 0) become
 *                   exp(log_f0_mean + (ln f0 - mu_s) * (sigma_s > 0 ? log_f0_std / sigma_s : 0)), where mu_s / sigma_s are the
 *                   mean and population standard deviation of ln f0 over the utterance's voiced frames (natural log);
 *                   log_f0_mean finite, log_f0_std finite and >= 0.  0 (off) ignores both.
 * Unvoiced frames (0) stay 0; NaN / Inf frames pass through the conversion unchanged.  Only the spectral envelope is warped:
 * the aperiodicity is left as it is. */
typedef struct {
  double f0_scale;
  double formant_shift;
  int convert_log_f0;
  double log_f0_mean, log_f0_std;
} WorldHipModification;
/* Per-utterance log-F0 statistics: d_stats [n_utt][3] (device) = {voiced frames, mu_s, sigma_s} as defined above; an
 * utterance without a voiced frame gets {0, 0, 0}.  The summation order is fixed per utterance: values never depend on the
 * rest of the batch. */
WORLD_HIP_API int world_hip_f0_statistics(WorldHipContext *ctx, int n_utt, const int *n_frames, int f_stride,
                                          const double *d_f0, double *d_stats);
/* The modification of each utterance u by mods[u] (HOST array of n_utt; NULL = identity for all), for the frames below
 * n_frames[u] (HOST); frames and rows beyond are neither read nor written.  Works after either F0 route (Harvest, or DIO +
 * StoneMask).  f0 (d_f0_in, d_f0_out) and the spectrogram (d_sp_in, d_sp_out) are independent: pass both pointers of a
 * pair or neither (NULL: that part is not touched).  In place (in == out) and out of place give the same bits.  fs and
 * fft_size describe the rows (fft_size a power of two, 128..8192; ignored without a spectrogram).  Every parameter is
 * checked before any GPU work: a refused call (non-zero, world_hip_last_error) has touched no output.  The rows returned
 * feed world_hip_synthesis_batch and world_hip_realtime_add as they are. */
WORLD_HIP_API int world_hip_modify_batch(WorldHipContext *ctx, int n_utt, int fs, int fft_size, const int *n_frames,
                                         int f_stride, const WorldHipModification *mods, const double *d_f0_in,
                                         double *d_f0_out, const double *d_sp_in, double *d_sp_out);
/* Output samples of a resynthesis (test.cpp: int((n_frames - 1) * frame_period / 1000 * fs) + 1, the frame period scaled
 * by time_scale).  Pure host arithmetic; 0 for invalid arguments. */
WORLD_HIP_API int world_hip_resynthesis_length(int fs, int n_frames, double frame_period, double time_scale);
/* Harvest -> CheapTrick + D4C -> world_hip_modify_batch(mods) -> Synthesis of one batch in ONE call: the reference's
 * test.cpp chain (analysis, ParameterModification, Synthesis) without the parameters ever leaving the device.  Synthesis
 * runs at frame_period * time_scale (harvest_option->frame_period; time_scale finite, > 0: 2 = twice as long, the standard
 * WORLD speed change).  x, x_length as world_hip_analyze_batch; y [n_utt][y_stride] (device), y_length [n_utt] (HOST; see
 * world_hip_resynthesis_length).  Every utterance needs at least 2 frames.  Bit for bit what analyze_batch, modify_batch and
 * synthesis_batch produce in sequence on the same context.  The analysis lives in the context's workspace
 * (world_hip_workspace_bytes counts it; a capture of the call goes stale like any other when the workspace grows).  The
 * pulse capacity is that of world_hip_synthesis_batch: a raised F0 raises the pulse count, world_hip_sync /
 * world_hip_synthesis_pulses_dropped report a shortfall.  Invalid parameters are refused before any GPU work. */
WORLD_HIP_API int world_hip_resynthesize_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x, int x_stride,
                                               const int *x_length, const HarvestOption *harvest_option,
                                               const CheapTrickOption *cheaptrick_option, const D4COption *d4c_option,
                                               const WorldHipModification *mods, double time_scale, const int *y_length,
                                               int y_stride, double *d_y);

/* Frame-wise modification behind a time map: what world_hip_modify_batch does with one value per utterance, with one
 * value per OUTPUT frame, and output frames placed anywhere between the source frames.  Each curve is a DEVICE array
 * [n_utt][o_stride] of doubles, or NULL ("not given"); curves == NULL gives none.  Utterance u has n_frames[u] source
 * frames (arrays [n_utt][f_stride]...) and n_out[u] >= 1 output frames (arrays [n_utt][o_stride]...; both counts HOST).
 * Output frame j:
 *   1. source position s = d_time_map[u][j] in source frames, clamped to [0, n_frames[u] - 1] (a value that is not > 0,
 *      NaN included, reads frame 0); without a map s = j and n_out[u] must equal n_frames[u].  k = floor(s), w = s - k,
 *      k1 = min(k + 1, n_frames[u] - 1).
 *   2. spectrogram and aperiodicity rows: w == 0 or k1 == k takes row k bit for bit; otherwise
 *      (1.0 - w) * row[k][i] + w * row[k1][i], the reference synthesiser's blend between two frames.
 *   3. F0 (voiced = finite and > 0): w == 0 or k1 == k takes f0[k] bit for bit (NaN / Inf pass through); both neighbours
 *      voiced: the same blend; exactly one voiced: that frame's F0 if its weight (1 - w for k, w for k1) is above 0.5,
 *      else 0 (the reference's interpolated_vuv > 0.5); none voiced: 0.
 *   4. mods[u].convert_log_f0 acts on the SOURCE track before step 3, with the source utterance's statistics.
 *   5. d_f0_target: a frame that is voiced after step 3 takes d_f0_target[u][j] where that is finite and > 0.
 *   6. F0 *= d_f0_scale[u][j] if given, else mods[u].f0_scale.
 *   7. the row of step 2 is warped by d_formant_shift[u][j] if given, else mods[u].formant_shift: the arithmetic of
 *      world_hip_modify_batch bit for bit; a ratio of 1 leaves the row out of log / exp.
 *   8. d_ap_gain: ap = min(max(ap * g, 0.001), 1 - 1e-12) (GetSafeAperiodicity's bounds); without it the row of step 2.
 * Curve values cannot be checked before the launch: a scale, ratio or gain that world_hip_modify_batch would refuse in
 * mods (not finite, a negative scale or gain, a ratio <= 0 or with fft_size / 2 * ratio < 1) counts as 1 for that frame
 * and touches no other frame.  Everything on the host is checked before any GPU work (mods, shapes, n_out[u] in
 * [1, o_stride]); a refused call has written nothing.  Each in / out pair is optional as in world_hip_modify_batch.
 * With a time map no output may be its input (refused); without one, in place (o_stride == f_stride) and out of place
 * give the same bits.  Output frames and rows at or beyond n_out[u] are never written.  A log-F0 conversion takes
 * n_utt * f_stride doubles of the workspace; in steady state nothing is copied from the host and the call can be
 * captured. */
typedef struct {
  const double *d_time_map, *d_f0_target, *d_f0_scale, *d_formant_shift, *d_ap_gain;
} WorldHipFrameCurves;
WORLD_HIP_API int world_hip_modify_frames_batch(WorldHipContext *ctx, int n_utt, int fs, int fft_size, const int *n_frames,
                                                int f_stride, const int *n_out, int o_stride,
                                                const WorldHipModification *mods, const WorldHipFrameCurves *curves,
                                                const double *d_f0_in, double *d_f0_out, const double *d_sp_in,
                                                double *d_sp_out, const double *d_ap_in, double *d_ap_out);
/* Harvest -> CheapTrick + D4C -> world_hip_modify_frames_batch -> Synthesis in one call, at the analysis frame period
 * (the time map carries every change of duration).  Utterance u gives n_out[u] >= 2 output frames (curves
 * [n_utt][o_stride]) and y_length[u] == world_hip_resynthesis_length(fs, n_out[u], frame_period, 1.0) samples.  The
 * analysis and the modified frames live in the context's workspace.  Bit for bit what analyze_batch, modify_frames_batch
 * and synthesis_batch produce in sequence; pulse capacity and refusals as world_hip_resynthesize_batch. */
WORLD_HIP_API int world_hip_resynthesize_frames_batch(WorldHipContext *ctx, int n_utt, int fs, const double *d_x,
                                                      int x_stride, const int *x_length,
                                                      const HarvestOption *harvest_option,
                                                      const CheapTrickOption *cheaptrick_option,
                                                      const D4COption *d4c_option, const WorldHipModification *mods,
                                                      const WorldHipFrameCurves *curves, const int *n_out, int o_stride,
                                                      const int *y_length, int y_stride, double *d_y);

/* Alignment of two utterances by dynamic time warping: which frame of A belongs to which frame of B, from the coded frames
 * world_hip_analyze_coded / world_hip_code_spectral_envelope write, as the time map world_hip_modify_frames_batch reads.
 * Pair u has n_a[u] >= 1 frames of A and n_b[u] >= 1 frames of B (HOST arrays).  Frame i of A is the n_dims doubles at
 * d_a + (a_row[u] + i) * a_row_stride, B likewise; a_row / b_row are HOST arrays of each pair's first row.  One rule, three
 * layouts: dense coded arrays (a_row[u] = u * f_stride); blocks of coded records (a_row[u] = the prefix sum of the frame
 * counts, d_a pointing at column 2, or column 3 to leave out c0, the usual choice); two utterances of one block (d_a and
 * d_b may alias: the call only reads them).  1 <= n_dims <= the row strides, n_dims <= 256.
 *   local cost  c(i, j) = sqrt(s), s = the sum over k = 0 .. n_dims - 1, in ascending order, of (a_k - b_k) * (a_k - b_k):
 *               subtraction, multiplication and addition each rounded on its own (no fused multiply-add), the square
 *               root IEEE-rounded.
 *   recurrence  D(0, 0) = c(0, 0); D(i, j) = c(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)) over the predecessors that
 *               exist; the predecessor taken is the first of (diagonal, i - 1, j - 1) that attains the minimum (a later
 *               candidate replaces an earlier one only if strictly smaller).  The path is the backtrack from
 *               (n_a - 1, n_b - 1) to (0, 0); K is its length.
 * Outputs (DEVICE arrays, each may be NULL):
 *   d_path [n_pairs][p_stride][2]   the cells (i, j) in ascending order;   d_path_len [n_pairs]   K
 *   d_summary [n_pairs][3]          {D(n_a-1, n_b-1), K, mcd_db}, mcd_db = (10 / ln 10) * sqrt(2) * D / K: the mel-cepstral
 *                                   distortion in dB when the rows are WORLD mel-cepstra without c0
 *   d_map_b [n_pairs][map_stride]   for frame j of B: 0.5 * (i_lo + i_hi) over the path cells of column j (exact).  This
 *                                   is world_hip_modify_frames_batch's d_time_map with A as the source and n_out = n_b.
 *   d_map_a [n_pairs][map_stride]   the mirror image, one value per frame of A
 * Entries beyond a pair's own counts (path rows beyond K, map entries beyond n_b / n_a) are never written.
 * Refused before any GPU work, with nothing written: n_pairs < 1, a NULL input, a count below 1, n_dims outside [1, 256],
 * a row stride below n_dims, a negative row, p_stride < n_a[u] + n_b[u] - 1 when d_path is given, map_stride below the
 * frame count a given map needs, n_a[u] * n_b[u] above world_hip_align_workspace_cells() = 2^26 cells (8192 x 8192; about
 * 40 s against 40 s at a 5 ms hop).  Feature values cannot be checked before the launch: a pair with NaN or Inf features
 * still gets a monotone path from (0, 0) to its last cell, of whatever cost, with every index in bounds, and no other pair
 * is affected.  Workspace: 9 bytes per cell (cost and predecessor; the backward walk reuses the pair's cost bytes) and 8 per
 * pair, for at most 2^26 cells at a time -- larger batches are walked in groups of pairs -- so never more than 0.61 GB;
 * world_hip_workspace_bytes counts it.  Time: the cost is parallel, but a pair's n_a + n_b - 1 anti-diagonals are serial
 * steps in one workgroup -- 0.96 us each as measured on one MI355X: 4 ms at 2001 x 2001, 16 ms at
 * 8192 x 8192.  The cell limit bounds memory, not that: a degenerate pair such as 1 x 2^26 is admitted and would hold one
 * compute unit for about a minute -- keep n_a + n_b to what the use needs (an utterance of 40 s has 8192 frames).  Stream
 * order and errors as the other batched calls; after one eager call of a shape the call neither allocates nor waits and can
 * be captured. */
WORLD_HIP_API int world_hip_align_batch(WorldHipContext *ctx, int n_pairs, int n_dims, const double *d_a,
                                        const long long *a_row, const int *n_a, int a_row_stride, const double *d_b,
                                        const long long *b_row, const int *n_b, int b_row_stride, int p_stride, int *d_path,
                                        int *d_path_len, double *d_summary, int map_stride, double *d_map_b,
                                        double *d_map_a);
WORLD_HIP_API int world_hip_align_workspace_cells(void);   /* the per-pair cell limit; host arithmetic */

/* Morph of two aligned utterances: the frames that lie between A and B -- a time axis part-way along the warping path,
 * F0 and spectral envelope interpolated geometrically between the aligned frames, aperiodicity blended, each with a rate
 * of its own that may change from frame to frame.  Rate 0 is A, rate 1 is B.  Pair u has n_a[u] >= 1 frames of A (arrays
 * [n_pairs][a_stride]..., as world_hip_analyze_batch writes them), n_b[u] >= 1 frames of B ([n_pairs][b_stride]...) and
 * the path world_hip_align_batch wrote for it (d_path [n_pairs][p_stride][2], d_path_len [n_pairs]; DEVICE).  n_a, n_b and
 * morphs are HOST arrays of n_pairs.  The output arrays are [n_pairs][o_stride]...; pair u gets
 * n_out[u] = world_hip_morph_length(n_a[u], n_b[u], morphs[u].time_rate) frames, and o_stride must hold them.
 *   1. time axis.  Path cell k = (i_k, j_k), k = 0 .. K - 1, lies at t_k = (1.0 - r) * i_k + r * j_k, r = time_rate: each
 *      operation rounded on its own (no fused multiply-add), so t is non-decreasing in k for every r.
 *      world_hip_morph_length = floor((1.0 - r) * (n_a - 1) + r * (n_b - 1)) + 1, the same expression at the last cell
 *      (-1 for a count below 1 or an r outside [0, 1]; host arithmetic).  For n_a == n_b that is n_a, or n_a - 1 at a
 *      rate where the rounded sum falls short of n_a - 1.
 *   2. positions.  Output frame m (as a double): lo = the first k with t_k >= m.  If t_lo == m: hi = the last k with
 *      t_k == m, sA = 0.5 * (i_lo + i_hi), sB = 0.5 * (j_lo + j_hi).  Otherwise w = (m - t_{lo-1}) / (t_lo - t_{lo-1}),
 *      sA = i_{lo-1} + w * (i_lo - i_{lo-1}), sB likewise.  So r = 0 gives sA = m and sB = world_hip_align_batch's
 *      d_map_a[m] bit for bit, r = 1 gives sB = m and sA = d_map_b[m].  d_path == NULL: the pair is aligned frame for
 *      frame, n_a[u] must equal n_b[u], sA = sB = m.  sA and sB are clamped to [0, n_a - 1] and [0, n_b - 1] as
 *      world_hip_modify_frames_batch clamps a time map (never needed on a path world_hip_align_batch wrote).
 *   3. rows at a position: row a = world_hip_modify_frames_batch's step 2 at s = sA on A's rows (k = floor(s), w = s - k;
 *      row k bit for bit when w == 0 or k is the last frame, else (1.0 - w) * row[k][i] + w * row[k + 1][i]); row b the
 *      same at sB on B's rows.  fA and fB: its step 3 (the F0 between two frames) at sA and sB.
 *   4. rates.  rho = the curve's value at frame m where that curve is given (DEVICE [n_pairs][o_stride]; a value that is
 *      not finite counts as 0, any other is clamped to [0, 1]), else the pair's value in morphs.
 *   5. spectral envelope: rho == 0 gives row a bit for bit, rho == 1 row b; otherwise
 *      exp((1.0 - rho) * log(a_i) + rho * log(b_i)).  A bin that is not positive gives what IEEE gives, in that bin alone.
 *   6. aperiodicity: the same end cases; otherwise (1.0 - rho) * a_i + rho * b_i -- a convex combination, so it stays
 *      within GetSafeAperiodicity's bounds whenever the inputs do.
 *   7. F0 (voiced = finite and > 0): rho == 0 gives fA, rho == 1 fB, bit for bit; both voiced:
 *      exp((1.0 - rho) * log(fA) + rho * log(fB)); exactly one voiced: that F0 if its weight (1 - rho for A, rho for B) is
 *      above 0.5, else 0 (the reference's interpolated_vuv > 0.5); neither: 0.
 * Each triple (d_f0_a, d_f0_b, d_f0_out), (d_sp_...), (d_ap_...) is optional as a whole: all three pointers or none.
 * d_pos_a / d_pos_b (DEVICE [n_pairs][o_stride], each may be NULL) receive sA / sB; where one is NULL the positions live
 * in n_pairs * o_stride doubles of the workspace (world_hip_workspace_bytes counts them).  Frames and rows at or beyond
 * n_out[u] are never written.  Refused before any GPU work, with nothing written: n_pairs outside [1, 65535], NULL n_a,
 * n_b or morphs, a count below 1 or above its stride, a rate in morphs outside [0, 1] or not finite, o_stride below an
 * n_out[u], a path without d_path_len or with p_stride < n_a[u] + n_b[u] - 1, no path and n_a[u] != n_b[u], a triple given
 * in part, fs < 1 or fft_size not a power of two in [128, 8192] when rows are given, an output that overlaps an input or
 * another output.  A path read from the device cannot be checked before the launch: K is clamped into [1, p_stride] and
 * every index into its utterance (should no k have t_k >= m, lo = K - 1; should lo be 0 with t_0 > m, the position is cell
 * 0), so a path world_hip_align_batch did not write gives positions that mean nothing but stay in bounds, and no other
 * pair is affected.  Stream order and errors as the other batched calls; the per-pair arrays go through the context's
 * small-array store, so after one eager call of a shape the call copies nothing from the host and can be captured. */
typedef struct { double time_rate, f0_rate, sp_rate, ap_rate; } WorldHipMorph;
typedef struct { const double *d_f0_rate, *d_sp_rate, *d_ap_rate; } WorldHipMorphCurves;
WORLD_HIP_API int world_hip_morph_length(int n_a, int n_b, double time_rate);
WORLD_HIP_API int world_hip_morph_batch(WorldHipContext *ctx, int n_pairs, int fs, int fft_size, const int *n_a, int a_stride,
                                        const double *d_f0_a, const double *d_sp_a, const double *d_ap_a, const int *n_b,
                                        int b_stride, const double *d_f0_b, const double *d_sp_b, const double *d_ap_b,
                                        int p_stride, const int *d_path, const int *d_path_len, const WorldHipMorph *morphs,
                                        const WorldHipMorphCurves *curves, int o_stride, double *d_f0_out, double *d_sp_out,
                                        double *d_ap_out, double *d_pos_a, double *d_pos_b);

/* Real-time synthesis, batched (reference src/synthesisrealtime.cpp; the drop-in WorldSynthesizer above is built on it).
 * One object serves n_streams independent streams with one fs, frame_period (ms), fft_size, buffer_size and ring size
 * number_of_pointers; every stream behaves exactly as one reference synthesiser: same pulses, same return values, its own
 * randn() sequence from the seed.  Pulse schedules and ring bookkeeping run on the host; pulse responses and the
 * overlap-add on the GPU, on the context's stream (the object uses the context; destroy the object first).
 *   _add: AddParameters of one chunk of n_frames frames: f0 is HOST memory, the spectrogram / aperiodicity rows are DEVICE
 *       rows row_stride doubles apart (fft_size / 2 + 1 used), e.g. records of world_hip_analyze_packed.  They are copied
 *       into the stream's frame store on the stream before the call returns, so the caller may reuse its buffers for
 *       later work on the same stream.  Returns 1 (added), 0 (the stream's ring is full), -1 (error: world_hip_last_error).
 *   _add_coded: _add of one chunk whose rows are CODED: d_coded_sp (number_of_dimensions mel-cepstrum coefficients per row)
 *       and d_coded_ap (GetNumberOfAperiodicities(fs) band values per row) are DEVICE rows row_stride doubles apart, so both
 *       may point into the same coded records (columns 2 and 2 + number_of_dimensions of world_hip_analyze_coded's).  The
 *       rows are decoded straight into the stream's frame store -- the decoders' arithmetic, no dense chunk in between --
 *       so every later call behaves, bit for bit, as after _add of the rows the two decode calls return.  Refuses what the
 *       decoders refuse; return values as _add.
 *   _synthesize: Synthesis2 for every stream at once: produced[s] (host) = its return value; d_out [n_streams][buffer_size]
 *       (device) gets each producing stream's buffer, zeros for the others.  When some streams need samples not yet
 *       rendered, their pulses that have a successor are rendered in batches of two kernels and one wait for the download:
 *       first what each stream's next buffer needs, then ahead, up to 256 MB of responses per batch.  One batch whatever
 *       n_streams while that holds (about 10 900 pulses at fft 2048, 2 700 at fft 8192); more batches only when it
 *       does not.  Calls that find their samples rendered only copy.  0 / -1; after -1 no stream
 *       has advanced (produced and d_out untouched).
 *   _is_locked: IsLocked (1 / 0; -1 = error).  _refresh: RefreshSynthesizer of one stream (0 / -1).
 *   _create: 0 = success, non-zero = failure (world_hip_last_error), as the calls above; *out = NULL then. */
typedef struct WorldHipRealtime WorldHipRealtime;
WORLD_HIP_API int world_hip_realtime_create(WorldHipContext *ctx, int n_streams, int fs, double frame_period_ms,
                                            int fft_size, int buffer_size, int number_of_pointers,
                                            WorldHipRealtime **out);
WORLD_HIP_API void world_hip_realtime_destroy(WorldHipRealtime *rt);
WORLD_HIP_API int world_hip_realtime_add(WorldHipRealtime *rt, int stream, const double *f0, int n_frames,
                                         const double *d_sp, const double *d_ap, int row_stride);
WORLD_HIP_API int world_hip_realtime_add_coded(WorldHipRealtime *rt, int stream, const double *f0, int n_frames,
                                               const double *d_coded_sp, int number_of_dimensions,
                                               const double *d_coded_ap, int row_stride);
WORLD_HIP_API int world_hip_realtime_synthesize(WorldHipRealtime *rt, double *d_out, int *produced);
WORLD_HIP_API int world_hip_realtime_is_locked(WorldHipRealtime *rt, int stream);
WORLD_HIP_API int world_hip_realtime_refresh(WorldHipRealtime *rt, int stream);
/* test hook: the randn() generator state `draws` calls after `state` ({x, y, z, w}), as the scheduler computes it */
WORLD_HIP_API void world_hip_realtime_rng_jump(const unsigned int *state, unsigned long long draws, unsigned int *out);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_HIP_H_ */
