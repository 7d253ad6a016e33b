/*
 * world_oracle.h -- CPU ORACLE (test infrastructure, NOT product code).
 *
 * Plain-C restatement of the analysis path of mmorise/World
 * (Dio / Harvest / StoneMask / CheapTrick / D4C).  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this
 * library; the shipped HIP path (world_amd/csrc) never links or calls it.
 *
 * Parity pinning: the reference ships no golden vectors, so this
 * restatement is pinned against the reference itself: oracle/_ref/libworld_ref.so
 * (unmodified reference sources compiled in place by oracle/Makefile) and the
 * fixtures under tests/golden/ generated from it (tests/golden/make_golden.py).
 *
 * All 2-D outputs are dense row-major [frames][fft_size/2+1].
 */
#ifndef WORLD_ORACLE_H_
#define WORLD_ORACLE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- primitives (exposed so unit tests can pin them one by one) ---- */
void   wo_randn_seed(uint32_t s[4]);                 /* matlabfunctions.cpp:237-242 */
double wo_randn(uint32_t s[4]);                      /* matlabfunctions.cpp:244-264 */
int    wo_round(double v);                           /* matlabfunctions.cpp:206-208 */
int    wo_pow2_above(int n);                         /* common.cpp:51-54  */
void   wo_rfft(int n, const double *in, double *re, double *im);      /* fft.cpp:49-60  */
void   wo_cfft(int n, double *re, double *im, int sign);                /* fft.cpp:143-212: c2c, in place, unscaled */
void   wo_irfft_unscaled(int n, const double *re, const double *im,
                         double *out);                                 /* fft.cpp:26-35  */
void   wo_nuttall(int len, double *w);               /* common.cpp:113-121 */
void   wo_interp1(const double *x, const double *y, int n,
                  const double *xi, int ni, double *yi);               /* matlabfunctions.cpp:136-176 */
void   wo_interp1q(double x0, double dx, const double *y, int n,
                   const double *xi, int ni, double *yi);              /* matlabfunctions.cpp:214-235 */
void   wo_decimate(const double *x, int n, int r, double *y);         /* matlabfunctions.cpp:27-204 */
void   wo_dc_correction(const double *in, double f0, int fs, int fft_size,
                        double *out);                                  /* common.cpp:56-75 */
void   wo_linear_smoothing(const double *in, double width, int fs,
                           int fft_size, double *out);                 /* common.cpp:27-111 */

/* ---- the analysis path ---- */
int  wo_frame_count(int fs, int x_length, double frame_period);       /* harvest.cpp:1219, dio.cpp:639 */
void wo_harvest(const double *x, int x_length, int fs, double f0_floor,
                double f0_ceil, double frame_period, double *tpos, double *f0);
/* Harvest from the refined candidates on (harvest.cpp:652-1113, 1246-1251): cand, score [nf][nslot] at 1 ms -> the pruned
 * candidates and scores, the contour after FixStep2, 3, 4 and the smoother [nf], and the frames at frame_period (returns
 * their number, (int)((nf - 1) / frame_period) + 1) */
int  wo_harvest_contour(const double *cand, const double *score, int nf, int nslot, double frame_period,
                        double *pruned_cand, double *pruned_score, double *step2, double *step3, double *step4,
                        double *smooth, double *tpos, double *f0, int *counters);
void wo_harvest_smooth(const double *f0, int nf, double *out);         /* harvest.cpp:1079-1113 (value arithmetic in wo_real) */
/* wo_harvest_contour's counters (NULL: none): branches of FixStep3 and FixStep4 taken on this map */
enum { WO_HC_SECTIONS,            /* voiced sections entering step 3 */
       WO_HC_REJECTED, WO_HC_KEPT, WO_HC_COMPACTED,   /* ExtendSub: dropped, kept, kept behind a dropped one (moved down) */
       WO_HC_MERGE_DISJOINT, WO_HC_MERGE_CONTAINED, WO_HC_MERGE_S1_GT, WO_HC_MERGE_S1_EQ, WO_HC_MERGE_S1_LT,
       WO_HC_MERGE_OUT_OF_ORDER,  /* channel 0 met again at its sorted position */
       WO_HC_BRIDGED,             /* FixStep4: gaps filled */
       WO_HC_EXTEND_STOPPED, WO_HC_EXTEND_FULL_REACH,  /* ExtendF0: ended by four misses / by its reach */
       WO_HC_EXTEND_TIE,          /* another value exactly as near as the one picked */
       WO_HC_EXTEND_AT_RANGE,     /* picked exactly at the allowed range */
       WO_HC_EXTEND_HIT_AFTER_3,  /* a hit after three misses */
       WO_HC_COUNTERS };
/* Harvest's candidate stage on made-up zero-crossing lists (harvest.cpp:188-190, 240-293, 348-412): edges [nch][4][ev_cap]
 * ascending fine edges per band and family (falling, rising, peaks, dips), counts [nch][4] -> raw [nch][nf] at the 1 ms frames
 * and cand [nf][maxc]; returns the most candidates a frame has.  edges == NULL: raw is given, detection alone.  A frame can
 * hold (nch - 1) / 11 candidates: maxc must not be less. */
int  wo_harvest_candidates(const double *edges, const int *counts, int ev_cap, double afs, const double *band_f0, int nch,
                           int nf, double f0_floor, double f0_ceil, double *raw, double *cand, int maxc);
/* Harvest's refinement stage on a made-up candidate map (harvest.cpp:417-631): y the decimated signal, cand [nf][nc] candidates
 * per 1 ms frame (0: none) -> refined, score [nf][7 nc], slot j + nc m of frame f from candidate j of frame f - m (m <= 3) or
 * f + m - 3.  The discrete path is the reference's double expressions; every value is wo_real (long double in the wide build:
 * the yardstick of the refinement kernels; in the double build a third statement beside the reference and wo_harvest's own
 * refinement, which is untouched).  raw [nf][7 nc][2] (NULL: none): refined F0 and score BEFORE the gate; report
 * [nf][7 nc][WO_HR_REPORT] (NULL: none): what the slot's candidate fixed and which gate closed. */
void wo_harvest_refine(const double *y, int y_len, double afs, const double *cand, int nf, int nc, double f0_floor,
                       double f0_ceil, double *refined, double *score, double *raw, int *report);
enum { WO_HR_HW, WO_HR_FIRST, WO_HR_LGN, WO_HR_NH,  /* window half length, first base index, log2 fft_size, harmonics */
       WO_HR_IDX,                  /* .. WO_HR_IDX + 5: the harmonics' bins (0 beyond nh) */
       WO_HR_GATE = WO_HR_IDX + 6, /* one of the five below */
       WO_HR_ZERO_POWER,           /* harmonics whose bin has power exactly 0 */
       WO_HR_REPORT };
enum { WO_HR_PASSED, WO_HR_FLOOR, WO_HR_CEIL, WO_HR_SCORE, WO_HR_EMPTY };
void wo_dio(const double *x, int x_length, int fs, double f0_floor,
            double f0_ceil, double channels_in_octave, double frame_period,
            int speed, double allowed_range, double *tpos, double *f0);
void wo_stonemask(const double *x, int x_length, int fs, const double *tpos,
                  const double *f0, int nf, double *refined);
int  wo_cheaptrick_fft_size(int fs, double f0_floor);                 /* cheaptrick.cpp:191-194 */
void wo_cheaptrick(const double *x, int x_length, int fs, const double *tpos,
                   const double *f0, int nf, double q1, int fft_size,
                   double *spectrogram);
void wo_d4c(const double *x, int x_length, int fs, const double *tpos,
            const double *f0, int nf, int fft_size, double threshold,
            double *aperiodicity);


/* codec: contiguous row-major [nf][*] arrays in and out */
int  wo_number_of_aperiodicities(int fs);                              /* codec.cpp:212-215 */
void wo_code_aperiodicity(const double *ap, int nf, int fs, int fft_size,
                          double *coded);                              /* codec.cpp:217-236 */
void wo_decode_aperiodicity(const double *coded, int nf, int fs, int fft_size,
                            double *ap);                               /* codec.cpp:238-266 */
void wo_code_spectral_envelope(const double *sp, int nf, int fs, int fft_size,
                               int ndim, double *coded);               /* codec.cpp:268-297 */
void wo_decode_spectral_envelope(const double *coded, int nf, int fs, int fft_size,
                                 int ndim, double *sp);                /* codec.cpp:299-324 */

/* synthesis: dense [nf][fft_size/2+1] spectrogram / aperiodicity */
void wo_synthesis(const double *f0, int nf, const double *sp, const double *ap, int fft_size,
                  double frame_period, int fs, int y_length, double *y);   /* synthesis.cpp:339-399 */

#ifdef __cplusplus
}
#endif
#endif  /* WORLD_ORACLE_H_ */
