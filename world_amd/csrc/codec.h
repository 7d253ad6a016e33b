// codec.h -- parameter block of the envelope / aperiodicity coders (codec.hip).
// Reference: src/codec.cpp (CodeSpectralEnvelope, DecodeSpectralEnvelope,
// CodeAperiodicity, DecodeAperiodicity).  Rows are dense and independent, so a
// "batch" is simply a row count; every table below depends on (fs, fft_size) only.
#pragma once
#include "common.h"

namespace world_hip {

struct CodecParams {
  const double *in;       // [rows][in_cols]
  double *out;            // [rows][out_cols]
  size_t in_stride, out_stride;   // doubles between consecutive rows; 0 = dense (in_cols / out_cols).  Rows that live inside
                          // packed records (world_hip_analyze_coded: the coded wire format of the multi-GPU exchange) have the
                          // records' strides
  int rows;
  int fs, fft_size;
  int lg_md;              // log2(fft_size / 2): the DCT length ("max_dimension")
  int ndim;               // number_of_dimensions (envelope) / number_of_aperiodicities
  const int *knot;        // interp1 bin of every query (1-based upper knot), host-built
  const double *frac;     // interp1 weight of every query, host-built
  const double *w_re, *w_im;   // DCT / IDCT weights (codec.cpp:170-175, 193-197)
  Tables tab;
};

void launch_code_spectral_envelope(const CodecParams &p, hipStream_t stream);
void launch_decode_spectral_envelope(const CodecParams &p, hipStream_t stream);
void launch_code_aperiodicity(const CodecParams &p, hipStream_t stream);
void launch_decode_aperiodicity(const CodecParams &p, hipStream_t stream);

// Records -> the dense f64 rows the synthesiser reads (world_hip_synthesis_records; sy_stage_records).  One workgroup per
// (frame, utterance) reads one record and writes that frame's F0, spectrogram row and aperiodicity row:
//   wire 2: coded records [tpos, f0, mel-cepstrum[ndim], band aperiodicity[nap]] -- codec_decode_sp's and codec_decode_ap's
//           arithmetic (the same device functions), both rows in the one launch;
//   wire 1: [tpos, f0, sp f32[nb], ap f32[nb]] -- widened.
// Utterance u's records start at row src_row[u] of `block` (`cols` doubles apart), its staged frames at row dst_row[u].
struct StageRecordsParams {
  int n_utt, wire;
  int fft_size, lg_md;           // lg_md = log2(fft_size / 2)
  int ndim, nap;                 // wire 2: coefficients and aperiodicity bands per record
  const int *n_frames;           // [n_utt] (device)
  const int *src_row, *dst_row;  // [n_utt] (device)
  const double *block;
  int cols;
  double *f0;                    // [rows]
  double *sp, *ap;               // [rows][fft_size/2+1]
  // wire 2: the decoders' tables of (fs, fft_size) (api.hip: codec_tables)
  const int *knot_sp, *knot_ap;
  const double *frac_sp, *frac_ap, *w_re, *w_im;
  Tables tab;
};
void launch_stage_records(const StageRecordsParams &p, int max_frames, hipStream_t stream);

// The same decode into a real-time stream's frame store (world_hip_realtime_add_coded; rt_store_coded_rows): coded row r
// of a chunk of n (coded_sp / coded_ap: device rows row_stride doubles apart) -> store row (first + r) % cap of dst_sp and
// dst_ap ([cap][fft_size/2+1]).  rt_store_rows with the decode fused in: no dense chunk exists.
struct RtCodedRowsParams {
  double *dst_sp, *dst_ap;
  int cap, n;
  long long first;
  const double *coded_sp, *coded_ap;
  int row_stride;
  int fft_size, lg_md, ndim, nap;
  const int *knot_sp, *knot_ap;
  const double *frac_sp, *frac_ap, *w_re, *w_im;
  Tables tab;
};
void launch_rt_store_coded_rows(const RtCodedRowsParams &p, hipStream_t stream);

// Parameter modification between analysis and synthesis (the reference's test/test.cpp: ParameterModification): F0
// scaling with an optional log-F0 statistics conversion, and the spectral envelope stretched along frequency.  Every
// per-utterance value is a device array of the context's small-array slabs ([n_utt] unless noted).
struct ModifyParams {
  int n_utt, f_stride;
  int fs, fft_size;              // warp: the rows have fft_size/2+1 bins
  const int *n_frames;           // frames of each utterance; rows / frames beyond are never read or written
  // spectral warp (modify_warp_sp): sp_in may equal sp_out
  const double *ratio;           // formant shift; 1 = the row is left as it is (copied when out-of-place)
  const double *sp_in;
  double *sp_out;
  // F0 map (modify_f0): f0_in may equal f0_out; f0_out == nullptr = statistics only
  const double *f0_scale;
  const int *convert;            // 1 = voiced log-F0 mapped onto target[2u] (mean), target[2u + 1] (std)
  const double *target;          // [n_utt][2]
  const double *f0_in;
  double *f0_out;
  double *stats;                 // [n_utt][3] {voiced frames, mean log F0, std log F0}, or nullptr
};

// LDS of one warp workgroup: the row's log and the knots, 2 (fft_size/2+1) doubles (65.6 KB at fft_size 8192)
size_t modify_warp_lds_bytes(int fft_size);
void launch_modify_warp_sp(const ModifyParams &p, int max_frames, hipStream_t stream);
void launch_modify_f0(const ModifyParams &p, hipStream_t stream);

// Frame-wise modification with a time map (world_hip_modify_frames_batch): output frame j of utterance u is made from the
// source frames floor(s) and floor(s) + 1 around its source position s, then modified by that frame's own values.  A curve
// is a device array [n_utt][o_stride] or nullptr ("not given": the per-utterance value of `m` holds, or no time map / target
// / gain at all).  m.n_frames / m.f_stride describe the source, n_out / o_stride the output; m.sp_in, m.f0_in are source
// arrays, m.sp_out, m.f0_out output arrays.  Curve values that the per-utterance checks would refuse count as 1.
struct ModifyFramesParams {
  ModifyParams m;
  int o_stride;
  const int *n_out;              // output frames of each utterance; rows / frames beyond are never written
  const double *time_map;        // source position in frames, clamped to [0, n_frames - 1]; nullptr: s = j
  const double *f0_target;       // replaces the F0 of voiced output frames where finite and > 0
  const double *f0_scale;        // replaces m.f0_scale[u]
  const double *formant_shift;   // replaces m.ratio[u]
  const double *ap_gain;         // ap = min(max(ap * g, 0.001), 1 - 1e-12); nullptr: the rows as they are
  const double *ap_in;
  double *ap_out;
  const double *f0_src;          // the source track modify_frames_f0 reads: m.f0_in, or its log-F0 conversion (a temporary)
};
void launch_modify_frames_sp(const ModifyFramesParams &p, int max_out, hipStream_t stream);
void launch_modify_frames_ap(const ModifyFramesParams &p, int max_out, hipStream_t stream);
void launch_modify_frames_f0(const ModifyFramesParams &p, int max_out, hipStream_t stream);

// Alignment of two rows of frames by dynamic time warping (world_hip_align_batch; align.inc).  Pair u: n_a[u] frames of A
// from row a_row[u] of `a` (a_stride doubles apart, n_dims of them used), B likewise.  The launches of one GROUP of pairs
// [first_pair, first_pair + pairs) share the workspace: pair u's cells live at cell0[u] of `cost` / `code`, one anti-diagonal
// after the other (cell (i, j) of diagonal d = i + j at the diagonal's start + i - max(0, d - (n_b - 1))), so that the DP
// kernel reads and writes consecutive addresses.  The backward walk ([n_a + n_b - 1][2] ints, far corner first) is written
// over the pair's own costs once the DP has consumed them: 8 bytes per step, and n_a + n_b - 1 <= n_a n_b.
struct AlignParams {
  int n_dims, first_pair;
  const double *a, *b;
  int a_stride, b_stride;
  const long long *a_row, *b_row;   // [n_pairs] (device, as every array below)
  const int *n_a, *n_b;             // [n_pairs]
  const long long *cell0;           // [n_pairs]
  double *cost;                     // local costs c(i, j); after align_dp, the pair's walk
  unsigned char *code;              // predecessor of every cell: 0 diagonal, 1 (i - 1, j), 2 (i, j - 1), 3 none (the origin)
  double *dist;                     // [n_pairs] D(n_a - 1, n_b - 1)
  int cap;                          // slots of each of align_dp's two diagonal buffers in LDS: > min(n_a, n_b) of every pair
  double mcd_scale;                 // (10 / ln 10) sqrt(2)
  // outputs, each optional
  int *path;                        // [n_pairs][p_stride][2]
  int p_stride;
  int *path_len;                    // [n_pairs]
  double *summary;                  // [n_pairs][3]
  int map_stride;
  double *map_b, *map_a;            // [n_pairs][map_stride]
};
size_t align_cost_lds_bytes(int n_dims);
void launch_align_cost(const AlignParams &p, int pairs, int max_tiles, hipStream_t stream);
void launch_align_dp(const AlignParams &p, int pairs, hipStream_t stream);
void launch_align_path(const AlignParams &p, int pairs, hipStream_t stream);
int align_cost_tiles(int n_a, int n_b);

// Morph of two aligned utterances (world_hip_morph_batch; morph.inc).  Pair u: n_a[u] frames of A ([n_pairs][a_stride]...),
// n_b[u] of B, n_out[u] output frames ([n_pairs][o_stride]...).  morph_positions turns the pair's warping path into the
// two source positions of every output frame (pos_a / pos_b: the caller's arrays or workspace); the three row kernels
// read them as modify_frames reads a time map.  Rates: rate[4 u + {0, 1, 2, 3}] = the pair's time, f0, sp and ap rate
// (all within [0, 1]: the host refuses anything else); a curve ([n_pairs][o_stride] or nullptr) replaces its rate per frame.
struct MorphParams {
  int n_pairs, fft_size;
  int a_stride, b_stride, o_stride, p_stride;
  const int *n_a, *n_b, *n_out;     // [n_pairs] (device, as every array below)
  const int *path;                  // [n_pairs][p_stride][2] as align_path wrote it, or nullptr: frame m of A belongs to frame m of B
  const int *path_len;              // [n_pairs]
  const double *rate;               // [n_pairs][4]
  const double *f0_curve, *sp_curve, *ap_curve;
  const double *f0_a, *sp_a, *ap_a, *f0_b, *sp_b, *ap_b;
  double *f0_out, *sp_out, *ap_out;
  double *pos_a, *pos_b;            // [n_pairs][o_stride]
};
void launch_morph_positions(const MorphParams &p, int max_out, hipStream_t stream);
void launch_morph_frames_sp(const MorphParams &p, int max_out, hipStream_t stream);
void launch_morph_frames_ap(const MorphParams &p, int max_out, hipStream_t stream);
void launch_morph_frames_f0(const MorphParams &p, int max_out, hipStream_t stream);

// All-pass mel-cepstra (world_hip_sp2mc / world_hip_mc2sp; mcep.inc): out [rows][k_out] = f(in [rows][k_in]) x table, with
// ln applied to the input (encode: k_in bins -> k_out coefficients) or exp to the output (decode).  `table` is the
// direction's host table transposed to [k_in][k_out] and padded with zeros to [k_pad][n_pad] (mcep_table_shape).
struct McepParams {
  const double *in;
  double *out;
  const double *table;
  long long in_stride, out_stride;  // doubles between rows
  int rows, k_in, k_out, k_pad, n_pad;
};
void mcep_table_shape(bool decode, int fft_size, int order, int *k_pad, int *n_pad);
void launch_mcep(const McepParams &p, bool decode, hipStream_t stream);

// Dynamic features and parameter generation (world_hip_delta_batch / world_hip_mlpg_batch; mlpg.inc).  One block for both:
// the stencil reads `mean` as the statics [u][t][dim] and writes out [u][t][n_win dim]; the generation reads mean and var
// [u][t][n_win dim] and writes out [u][t][dim].  Strides are counted in doubles (mask_us in bytes); var_rs and var_us may
// be 0.  `win` holds the windows centred: win[w][2 + tau], zeros beyond the half-width.
struct MlpgParams {
  const double *mean, *var;
  double *out;
  const unsigned char *mask;      // [u][t], non-zero = present; nullptr: every frame is
  double *ws;                     // the sweeps' workspace [t][B + 1][n_sys] (mlpg_workspace_doubles)
  const int *n_frames;            // device, [n_utt]
  long long mean_us, mean_rs, var_us, var_rs, out_us, out_rs, mask_us;
  long long n_sys;                // systems of the whole call: n_utt * dim
  int u0;                         // first utterance of this launch
  int dim, n_win, precision;
  double fill;
  double win[4][5];
};
size_t mlpg_workspace_doubles(int n_utt, int dim, int max_frames, int half_width);
void launch_delta(const MlpgParams &p, int half_width, int n_utt, int max_frames, hipStream_t stream);
void launch_mlpg(const MlpgParams &p, int half_width, int n_utt, int max_frames, hipStream_t stream);

// Joint-density Gaussian mixture (world_hip_gmm_convert / world_hip_gmm_accumulate; gmm.inc).  `model` is the prepared
// model on the device (gmm_host.h: GmmLayout; the offsets below are its), Kp and Ep the source and target dimensions padded
// to 16.  gmm_q writes q [rows][M], gmm_posterior turns it into gamma in place and finds the most likely mixture, gmm_regress
// reads both.  Strides are counted in doubles.
constexpr int kGmmMaxPad = 128;     // the largest padded dimension
struct GmmParams {
  const double *x;
  const double *model;
  long long x_rs, mean_rs, var_rs, post_rs;
  size_t off_c, off_mux, off_muy, off_v, off_ut, off_at;
  double *q;                      // workspace [rows][M]: q, then gamma
  int *best;                      // workspace [rows]: the lowest mixture that attains the largest q
  double *mean, *var, *post, *loglik;   // outputs, any may be nullptr
  int rows, M, Dx, Dy, Kp, Ep, mode;
};
void launch_gmm_q(const GmmParams &p, hipStream_t stream);
void launch_gmm_posterior(const GmmParams &p, hipStream_t stream);
void launch_gmm_regress(const GmmParams &p, hipStream_t stream);
// N [M], S1 [M][P], G [M][P][P] of rows [0, rows): gamma = post [t][m], the shift [M][P]
struct GmmAccParams {
  const double *z, *post, *shift;
  long long z_rs, post_rs;
  double *N, *S1, *G;
  int rows, M, P;
};
void launch_gmm_accumulate(const GmmAccParams &p, hipStream_t stream);
void launch_gmm_fill(double *d, size_t n, double value, hipStream_t stream);

// Training rows of a corpus (world_hip_frame_power_batch / _select_frames_batch / _gather_rows_batch / _joint_rows_batch;
// corpus.h).  Strides are counted in doubles, in ints for the index arrays and in bytes for the masks; the count arrays are
// device copies of the host's.
struct CorpusPowerParams {
  const double *sp;
  double *power, *mean;           // power [u][t] (the caller's or the workspace), mean [u] or nullptr
  const int *n_frames;
  long long sp_us, sp_rs, power_us;
  int fft_size, n_utt, u0;
};
void launch_frame_power(const CorpusPowerParams &p, int n_utt, int max_frames, hipStream_t stream);
void launch_frame_power_mean(const CorpusPowerParams &p, int n_utt, hipStream_t stream);
struct CorpusSelectParams {
  const double *value, *scale;    // scale [u] or nullptr
  const unsigned char *mask;
  int *index, *count;
  unsigned char *keep;
  const int *n_frames;
  long long value_us, value_s, mask_us, index_us, keep_us;
  double threshold;
  int u0;
};
void launch_select_frames(const CorpusSelectParams &p, int n_utt, hipStream_t stream);
// joint_rows: row k < n_rows[u] of pair u is A's row (through sel_a) then B's (through sel_b) at the path's cell k, or at
// (k, k) without a path; *_off are each pair's first element, `group` the lanes that share a row (corpus_group)
struct CorpusRowsParams {
  const double *a, *b;
  double *z;
  const long long *a_off, *b_off, *z_off;
  const int *n_a, *n_b, *n_sel_a, *n_sel_b, *n_rows;
  const int *path, *sel_a, *sel_b;
  long long a_rs, b_rs, z_rs, path_us, sel_a_us, sel_b_us;
  unsigned long long fill;
  int dim_a, dim_b, group, u0;
};
int corpus_group(int dim_a, int dim_b);
void launch_joint_rows(const CorpusRowsParams &p, int n_pairs, int max_rows, hipStream_t stream);

}  // namespace world_hip
