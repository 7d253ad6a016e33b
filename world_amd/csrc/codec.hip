// codec.hip -- low-dimensional coding of the analysis outputs (reference src/codec.cpp).
//
//   code_sp   : log envelope -> interp1 onto the mel axis -> DCT-II through one real FFT
//               of fft_size/2 points -> first `ndim` coefficients      (codec.cpp:73-87,120-130,268-297)
//   decode_sp : coefficients -> IDCT through one complex FFT -> interp1 back to the linear
//               axis -> exp                                            (codec.cpp:93-115,138-156,299-324)
//   code_ap   : 20 log10(ap) sampled at 3 kHz multiples (interp1Q)     (codec.cpp:217-236)
//   decode_ap : band values -> interp1 over [0, 3k.., fs/2] -> 10^(x/20), aperiodic
//               frames (mean band value > -0.5 dB) left at 1 - 1e-12   (codec.cpp:21-56,238-266)
//
//   sy_stage_records / rt_store_coded_rows : records -> the dense rows the synthesisers read, the two decoders fused in
//               (world_hip_synthesis_records, world_hip_realtime_add_coded)
//
// Both interp1 calls have fixed knots and fixed queries, so their bin search and weights
// are tables built once on the host (api.hip: codec_tables).  One 256-thread workgroup
// per frame for the envelope kernels, one thread per output value for the band kernels.
//
// Beside them, the parameter modification of the reference's test/test.cpp (ParameterModification, :221-258):
//   modify_warp_sp : log row -> interp1 from the axis ratio*i/fft*fs onto i/fft*fs -> exp, bins from
//                    int(fft/2*ratio) up filled with the bin below when ratio < 1   (one workgroup per row)
//   modify_f0      : optional log-F0 statistics conversion, then f0 *= scale     (one workgroup per utterance)
// and their frame-wise form behind a time map, with per-frame values (world_hip_modify_frames_batch):
//   modify_frames_sp / _ap / _f0 : output frame j = the blend of the two source frames around its source position,
//                    then the warp / gain / target and scale of that frame
// The warp's knots depend on each utterance's ratio, so its histc search runs in the kernel instead of a host table.
// And what turns two rows of coded frames into such a time map (world_hip_align_batch): align.inc, included at the end;
// behind it morph.inc, the frames between two utterances aligned that way (world_hip_morph_batch); and mcep.inc, the
// all-pass mel-cepstrum of an envelope and back (world_hip_sp2mc / world_hip_mc2sp) on the FP64 matrix unit; mlpg.inc,
// dynamic features and the maximum-likelihood trajectory behind them (world_hip_delta_batch / world_hip_mlpg_batch);
// gmm.inc, the joint-density Gaussian mixture between the two (world_hip_gmm_convert / world_hip_gmm_accumulate); last
// corpus.h, the rows that mixture is trained on (world_hip_frame_power_batch .. world_hip_joint_rows_batch; a header for the
// reason its head comment gives).
#include "codec.h"
#include "fft.h"

namespace world_hip {

static size_t code_sp_lds_bytes(int lg_md) {
  const size_t md = (size_t)1 << lg_md;
  return sizeof(double) * (md + 2 + md + 16 + twiddle_lds_doubles(lg_md));
}
static size_t decode_sp_lds_bytes(int lg_md) {
  const size_t md = (size_t)1 << lg_md;
  return sizeof(double) * (2 * md + 16 + md + 2 + twiddle_lds_doubles(lg_md));
}

__global__ void __launch_bounds__(256) codec_code_sp(CodecParams p) {
  DYN_LDS(lds);
  const int row = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int md = 1 << p.lg_md, nb = md + 1;
  double *lg = reinterpret_cast<double *>(lds);                       // log envelope, nb bins
  cplx *Z = reinterpret_cast<cplx *>(lg + md + 2);                    // real FFT input, md reals
  const TwLds tw = stage_twiddles(reinterpret_cast<double *>(Z) + md + 16, p.lg_md, p.tab.tw);
  const double *in = p.in + (size_t)row * (p.in_stride ? p.in_stride : (size_t)nb);
  for (int i = tid; i < nb; i += nt) lg[i] = log(in[i]);
  __syncthreads();
  // interp1 onto the mel axis, written straight into DCTForCodec's even/odd reordering
  for (int i = tid; i < md; i += nt) {
    const int k = p.knot[i];
    const double v = lg[k - 1] + p.frac[i] * (lg[k] - lg[k - 1]);
    const int dest = (i & 1) ? md / 2 + (md - 1 - i) / 2 : i / 2;
    rfft_in(Z, dest) = v;
  }
  lds_dead(lg, md + 2);                                               // the log row has gone into Z: the transform reads Z alone
  const double norm = sqrt(static_cast<double>(md));
  double *out = p.out + (size_t)row * (p.out_stride ? p.out_stride : (size_t)p.ndim);
  block_rfft(Z, p.lg_md, tw, [&](int k, double re, double im) {
    if (k < p.ndim) out[k] = (re * p.w_re[k] - im * p.w_im[k]) / norm;
  });
}

// DecodeSpectralEnvelope of ONE row by the whole workgroup: `in` = its p.ndim coefficients, `out` = where its
// fft_size/2+1 bins go, `lds` = decode_sp_lds_bytes(p.lg_md) bytes.  One spelling, three callers (codec_decode_sp,
// sy_stage_records, rt_store_coded_rows): the rows are the same bits wherever they are written.
struct DecodeTables {
  int lg_md, ndim;
  const int *knot;
  const double *frac, *w_re, *w_im;
  Tables tab;
};
__device__ __forceinline__ void decode_sp_row(const DecodeTables p, const double *in, double *out, char *lds, int tid, int nt) {
  const int md = 1 << p.lg_md, nb = md + 1;
  cplx *Z = reinterpret_cast<cplx *>(lds);                            // md complex points
  double *mel = reinterpret_cast<double *>(lds) + 2 * md + 16;        // md + 2 values
  const TwLds tw = stage_twiddles(mel + md + 2, p.lg_md, p.tab.tw);
  const double norm = sqrt(static_cast<double>(md));
  for (int i = tid; i < md; i += nt) {
    cplx v; v.re = 0.0; v.im = 0.0;
    if (i < p.ndim) { const double c = in[i]; v.re = c * p.w_re[i] * norm; v.im = -c * p.w_im[i] * norm; }
    Z[swz(i)] = v;
  }
  // The reference's backward c2c plan returns conj(sum_j in[j] e^{-2 pi i jk/n}) (fft.cpp:36-45);
  // only the real part is read, so a forward transform is what is needed.
  const FftPlan plan = make_plan(p.lg_md);
  block_cfft_dif(Z, plan, tw);
  for (int i = tid; i < md / 2; i += nt) {
    mel[1 + 2 * i] = Z[fft_slot(plan, i)].re;
    mel[2 + 2 * i] = Z[fft_slot(plan, md - 1 - i)].re;
  }
  __syncthreads();
  lds_dead(Z, 2 * md);                                                // the transform has gone into mel: the interpolation reads mel alone
  if (tid == 0) { mel[0] = mel[1]; mel[md + 1] = mel[md]; }
  __syncthreads();
  for (int j = tid; j < nb; j += nt) {
    const int k = p.knot[j];
    const double v = mel[k - 1] + p.frac[j] * (mel[k] - mel[k - 1]);
    out[j] = exp(v / md);
  }
}

__global__ void __launch_bounds__(256) codec_decode_sp(CodecParams p) {
  DYN_LDS(lds);
  const int row = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int md = 1 << p.lg_md, nb = md + 1;
  const double *in = p.in + (size_t)row * (p.in_stride ? p.in_stride : (size_t)p.ndim);
  decode_sp_row(DecodeTables{p.lg_md, p.ndim, p.knot, p.frac, p.w_re, p.w_im, p.tab}, in,
                p.out + (size_t)row * (p.out_stride ? p.out_stride : (size_t)nb), lds, tid, nt);
}

__global__ void codec_code_ap(CodecParams p) {
  const int item = flat_thread_x();
  if (item >= p.rows * p.ndim) return;
  const int row = item / p.ndim, band = item - row * p.ndim;
  const int nb = p.fft_size / 2 + 1;
  const double *in = p.in + (size_t)row * (p.in_stride ? p.in_stride : (size_t)nb);
  // interp1Q(0, fs/fft_size, 20 log10(ap), nb, 3000 (band+1)) -- matlabfunctions.cpp:214-235
  const double pos = (3000.0 * (band + 1.0) - 0) / (static_cast<double>(p.fs) / p.fft_size);
  const int b = static_cast<int>(pos);
  const double fr = pos - b;
  const double y0 = 20 * log10(in[b]);
  const double dy = b < nb - 1 ? 20 * log10(in[b + 1]) - y0 : 0.0;
  p.out[(size_t)row * (p.out_stride ? p.out_stride : (size_t)p.ndim) + band] = y0 + dy * fr;
}

// DecodeAperiodicity of ONE row of `ndim` band values `in`: CheckVUV's mean, once per row, then bin j from it.  The
// callers of decode_sp_row share both.
__device__ __forceinline__ double decode_ap_mean(const double *in, int ndim) {
  double mean = 0.0;                                  // CheckVUV, codec.cpp:31-41
  for (int i = 0; i < ndim; ++i) mean += in[i];
  return mean / ndim;
}
__device__ __forceinline__ double decode_ap_bin(const double *in, int ndim, double mean, const int *knot, const double *frac, int j) {
  double v = 1.0 - kTiny;                             // InitializeAperiodicity, codec.cpp:21-26
  if (!(mean > -0.5)) {
    // coarse = [-60, bands..., -1e-12] over knots [0, 3000.., fs/2]
    const int k = knot[j];
    const double lo = k - 1 == 0 ? -60.0 : in[k - 2];
    const double hi = k == ndim + 1 ? -kTiny : in[k - 1];
    v = pow(10.0, (lo + frac[j] * (hi - lo)) / 20.0);
  }
  return v;
}

__global__ void codec_decode_ap(CodecParams p) {
  const int nb = p.fft_size / 2 + 1;
  const long item = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= (long)p.rows * nb) return;
  const int row = (int)(item / nb), j = (int)(item - (long)row * nb);
  const double *in = p.in + (size_t)row * (p.in_stride ? p.in_stride : (size_t)p.ndim);
  const double v = decode_ap_bin(in, p.ndim, decode_ap_mean(in, p.ndim), p.knot, p.frac, j);
  p.out[(size_t)row * (p.out_stride ? p.out_stride : (size_t)nb) + j] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// Synthesis from records (world_hip_synthesis_records, world_hip_realtime_add_coded): a record becomes the dense f64 rows
// the pulse kernels read, ONCE per frame.  (Decoding inside the pulse instead would run the transform about five times per
// frame -- a pulse reads two frames, an unvoiced stretch has 2.5 pulses per 5 ms frame -- in a kernel that is already bound
// by vector-ALU issue: DESIGN.md 3.9.)  LDS: decode_sp_lds_bytes, the envelope's transform; the aperiodicity row needs none.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sy_stage_records(StageRecordsParams p) {
  DYN_LDS(lds);
  const int f = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  if (f >= p.n_frames[u]) return;
  const int nb = p.fft_size / 2 + 1;
  const double *rec = p.block + ((size_t)p.src_row[u] + f) * p.cols;
  const size_t at = (size_t)p.dst_row[u] + f;
  double *sp = p.sp + at * nb, *ap = p.ap + at * nb;
  if (tid == 0) p.f0[at] = rec[1];
  if (p.wire == 1) {                                  // [tpos, f0, sp f32[nb], ap f32[nb]]
    const float *rows = reinterpret_cast<const float *>(rec + 2);
    for (int j = tid; j < nb; j += nt) { sp[j] = rows[j]; ap[j] = rows[nb + j]; }
    return;
  }
  const DecodeTables ts{p.lg_md, p.ndim, p.knot_sp, p.frac_sp, p.w_re, p.w_im, p.tab};
  decode_sp_row(ts, rec + 2, sp, lds, tid, nt);
  const double *bands = rec + 2 + p.ndim;
  const double mean = decode_ap_mean(bands, p.nap);
  for (int j = tid; j < nb; j += nt) ap[j] = decode_ap_bin(bands, p.nap, mean, p.knot_ap, p.frac_ap, j);
}

__global__ void __launch_bounds__(256) rt_store_coded_rows(RtCodedRowsParams p) {
  DYN_LDS(lds);
  const int r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (r >= p.n) return;
  const int nb = p.fft_size / 2 + 1;
  const size_t row = (size_t)((p.first + r) % p.cap) * nb;
  const DecodeTables ts{p.lg_md, p.ndim, p.knot_sp, p.frac_sp, p.w_re, p.w_im, p.tab};
  decode_sp_row(ts, p.coded_sp + (size_t)r * p.row_stride, p.dst_sp + row, lds, tid, nt);
  const double *bands = p.coded_ap + (size_t)r * p.row_stride;
  const double mean = decode_ap_mean(bands, p.nap);
  for (int j = tid; j < nb; j += nt) p.dst_ap[row + j] = decode_ap_bin(bands, p.nap, mean, p.knot_ap, p.frac_ap, j);
}

// ---------------------------------------------------------------------------------------------------------------------
// Spectral warp.  interp1(x, log row, nb, xi, nb) with x[i] = ratio*i/fft*fs and xi[j] = j/fft*fs (matlabfunctions.cpp:
// 157-176): histc gives the query j the largest k in [1, nb-1] with x[k-1] <= xi[j] (queries at or beyond x[nb-1] get
// nb-1 and are extrapolated from the last interval).  The knots are evaluated once per workgroup, exactly as the reference
// evaluates them, into LDS beside the log row; x[c] <= xi is about c <= j/ratio, and the guess floor(j/ratio) is corrected
// against those knots, so k and the weights are the reference's bit for bit.  Per output bin: two FP64 divisions (xi and
// the interpolation weight), one exp; per input bin: one log, one division for its knot.
// ---------------------------------------------------------------------------------------------------------------------
// One row through the warp, by the whole workgroup: `load(j)` is bin j of the row to warp (read once), `lds` holds 2 nb doubles.
template <class Load>
__device__ __forceinline__ void warp_sp_row(Load load, double *out, double ratio, int fft_size, int fs, char *lds) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nb = fft_size / 2 + 1;
  double *lg = reinterpret_cast<double *>(lds);       // log row, nb doubles
  double *kx = lg + nb;                               // knots, nb doubles
  for (int j = tid; j < nb; j += nt) {
    lg[j] = log(load(j));
    kx[j] = ratio * j / fft_size * fs;                // test.cpp:237, in this order
  }
  __syncthreads();                                    // (in place: every read of the row is done before the first write)
  // ratio < 1: bins m .. nb-1 take bin m-1's warped value (test.cpp:250-254)
  const int m = ratio < 1.0 ? static_cast<int>(fft_size / 2.0 * ratio) : nb;
  const double inv_ratio = 1.0 / ratio;               // (the guess only: the knots decide)
  for (int j = tid; j < nb; j += nt) {
    const int q = j < m ? j : m - 1;
    const double xi = static_cast<double>(q) / fft_size * fs;
    const double g = q * inv_ratio;
    int c = g >= nb - 1 ? nb - 1 : static_cast<int>(g);   // the last knot <= xi: a guess ...
    while (c < nb - 1 && kx[c + 1] <= xi) ++c;
    while (c > 0 && kx[c] > xi) --c;                      // ... corrected (x[0] = 0 <= xi always)
    const int k = c + 1 < nb - 1 ? c + 1 : nb - 1;
    const double s = (xi - kx[k - 1]) / (kx[k] - kx[k - 1]);
    out[j] = exp(lg[k - 1] + s * (lg[k] - lg[k - 1]));
  }
}

__global__ void __launch_bounds__(256) modify_warp_sp(ModifyParams p) {
  DYN_LDS(lds);
  const int f = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  if (f >= p.n_frames[u]) return;
  const int nb = p.fft_size / 2 + 1;
  const size_t row = ((size_t)u * p.f_stride + f) * nb;
  const double *in = p.sp_in + row;
  double *out = p.sp_out + row;
  const double ratio = p.ratio[u];
  if (ratio == 1.0) {                                 // test.cpp without argv[4]: the row as it is
    if (out != in)
      for (int j = tid; j < nb; j += nt) out[j] = in[j];
    return;
  }
  warp_sp_row([&](int j) { return in[j]; }, out, ratio, p.fft_size, p.fs, lds);
}

// ---------------------------------------------------------------------------------------------------------------------
// Frame-wise modification (world_hip_modify_frames_batch).  Output frame j of utterance u sits at the source position
// s = time_map[u][j] (j without a map), clamped to [0, n_frames - 1] (not > 0, NaN included: 0): k = floor(s), w = s - k,
// k1 = min(k + 1, n_frames - 1).  w == 0 or k1 == k: row k as it is; else (1 - w) row[k] + w row[k1], the expression
// of the reference's synthesiser between two frames (synthesis.cpp:141-180).
//   modify_frames_sp : one workgroup per output row; the blend happens as the bins are loaded, so the warp sees one row
//                      and its LDS stays the log row and the knots.  Two source rows read, one written.
//   modify_frames_ap : the same blend, then the optional gain within GetSafeAperiodicity's bounds.  A kernel of its own:
//                      it streams (no LDS, no search), so it runs at full occupancy and leaves modify_frames_sp with
//                      modify_warp_sp's registers and LDS.
//   modify_frames_f0 : one thread per output frame.
// A curve value the per-utterance checks would refuse (api.hip: check_modifications) counts as 1.
// ---------------------------------------------------------------------------------------------------------------------
struct SourcePosition { int k, k1; double w; bool blend; };
__device__ __forceinline__ SourcePosition source_position(const double *time_map, size_t at, int j, int n_src) {
  double s = time_map ? time_map[at] : static_cast<double>(j);
  if (!(s > 0.0)) s = 0.0;
  if (s > n_src - 1) s = n_src - 1;
  SourcePosition sp;
  sp.k = static_cast<int>(s);                         // (s >= 0: the floor)
  sp.w = s - sp.k;
  sp.k1 = sp.k + 1 < n_src - 1 ? sp.k + 1 : n_src - 1;
  sp.blend = sp.w != 0.0 && sp.k1 != sp.k;
  return sp;
}
__device__ __forceinline__ double valid_scale(double v) { return __builtin_isfinite(v) && v >= 0.0 ? v : 1.0; }
__device__ __forceinline__ double valid_ratio(double r, int fft_size) {
  return __builtin_isfinite(r) && r > 0.0 && fft_size / 2.0 * r >= 1.0 ? r : 1.0;
}

__global__ void __launch_bounds__(256) modify_frames_sp(ModifyFramesParams p) {
  DYN_LDS(lds);
  const int j = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int nb = p.m.fft_size / 2 + 1;
  // j < gridDim.x <= o_stride: the frame's curve values exist whether or not the frame does, so they are fetched beside
  // n_out[u] instead of behind it (one round trip to memory less at the head of every workgroup)
  const size_t at = (size_t)u * p.o_stride + j;
  const SourcePosition s = source_position(p.time_map, at, j, p.m.n_frames[u]);
  const double ratio = p.formant_shift ? valid_ratio(p.formant_shift[at], p.m.fft_size) : p.m.ratio[u];
  if (j >= p.n_out[u]) return;
  const double *a = p.m.sp_in + ((size_t)u * p.m.f_stride + s.k) * nb;
  const double *b = p.m.sp_in + ((size_t)u * p.m.f_stride + s.k1) * nb;
  double *out = p.m.sp_out + at * nb;
  const double w = s.w;
  if (ratio == 1.0) {                                 // no log / exp round trip
    if (s.blend)
      for (int i = tid; i < nb; i += nt) out[i] = (1.0 - w) * a[i] + w * b[i];
    else if (out != a)
      for (int i = tid; i < nb; i += nt) out[i] = a[i];
    return;
  }
  if (s.blend)
    warp_sp_row([&](int i) { return (1.0 - w) * a[i] + w * b[i]; }, out, ratio, p.m.fft_size, p.m.fs, lds);
  else
    warp_sp_row([&](int i) { return a[i]; }, out, ratio, p.m.fft_size, p.m.fs, lds);
}

__global__ void __launch_bounds__(256) modify_frames_ap(ModifyFramesParams p) {
  const int j = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int nb = p.m.fft_size / 2 + 1;
  const size_t at = (size_t)u * p.o_stride + j;                                   // (in bounds: see modify_frames_sp)
  const SourcePosition s = source_position(p.time_map, at, j, p.m.n_frames[u]);
  const double g = p.ap_gain ? valid_scale(p.ap_gain[at]) : 1.0;
  if (j >= p.n_out[u]) return;
  const double *a = p.ap_in + ((size_t)u * p.m.f_stride + s.k) * nb;
  const double *b = p.ap_in + ((size_t)u * p.m.f_stride + s.k1) * nb;
  double *out = p.ap_out + at * nb;
  const double w = s.w;
  if (!p.ap_gain && !s.blend && out == a) return;
  for (int i = tid; i < nb; i += nt) {
    double v = s.blend ? (1.0 - w) * a[i] + w * b[i] : a[i];
    if (p.ap_gain) {                                  // GetSafeAperiodicity's bounds (common.cpp); NaN: the lower one
      v *= g;
      v = v > 0.001 ? v : 0.001;
      v = v < 1.0 - kTiny ? v : 1.0 - kTiny;
    }
    out[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// F0 map, one workgroup per utterance.  Voiced = finite and > 0.  Statistics (when converting or asked for): mean of
// ln f0 over the voiced frames (corrected once by the mean of the residuals), then the population standard deviation
// about it -- the passes re-read the utterance's F0, a few KB from L2; each thread sums a fixed
// stride of frames and the workgroup reduction has a fixed shape, so the values depend on the utterance alone.
// Zero voiced frames give {0, 0, 0}.  Then voiced frames (converted) and every other frame are multiplied by the scale:
// the reference's own multiply (test.cpp:225-227).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool voiced_f0(double v) { return v > 0.0 && __builtin_isfinite(v); }

__global__ void __launch_bounds__(256) modify_f0(ModifyParams p) {
  DYN_LDS(lds);
  double *scratch = reinterpret_cast<double *>(lds);  // 96 doubles: three disjoint areas of the block reductions
  const int u = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = p.n_frames[u];
  const double *in = p.f0_in + (size_t)u * p.f_stride;
  const bool convert = p.convert[u] != 0;
  double mu = 0.0, sigma = 0.0;
  if (convert || p.stats) {
    double sum = 0.0, count = 0.0;
    for (int i = tid; i < n; i += nt) {
      const double v = in[i];
      if (voiced_f0(v)) { sum += log(v); count += 1.0; }
    }
    block_sum2(sum, count, scratch);
    lds_dead(scratch, 64);                            // (count is the workgroup's: the branch below is uniform)
    if (count > 0.0) {
      mu = sum / count;
      // one correction of the mean by its residuals: a constant track then has mu exactly its ln f0, hence sigma_s = 0
      double res = 0.0;
      for (int i = tid; i < n; i += nt) {
        const double v = in[i];
        if (voiced_f0(v)) res += log(v) - mu;
      }
      mu += block_sum(res, scratch + 64) / count;
      lds_dead(scratch + 64, 16);
      double ss = 0.0;
      for (int i = tid; i < n; i += nt) {
        const double v = in[i];
        if (voiced_f0(v)) { const double d = log(v) - mu; ss += d * d; }
      }
      ss = block_sum(ss, scratch + 80);
      sigma = sqrt(ss / count);
    }
    if (p.stats && tid == 0) {
      p.stats[3 * u] = count; p.stats[3 * u + 1] = mu; p.stats[3 * u + 2] = sigma;
    }
  }
  if (!p.f0_out) return;
  double *out = p.f0_out + (size_t)u * p.f_stride;
  const double scale = p.f0_scale[u];
  const double mu_t = p.target[2 * u], gain = convert && sigma > 0.0 ? p.target[2 * u + 1] / sigma : 0.0;
  for (int i = tid; i < n; i += nt) {
    double v = in[i];
    if (convert && voiced_f0(v)) v = exp(mu_t + (log(v) - mu) * gain);
    out[i] = v * scale;
  }
}

// The F0 of the output frames, from the source track p.f0_src (already through the log-F0 conversion where one is asked
// for).  Between two frames: both voiced, the blend; one voiced, that frame's F0 while its weight is above 0.5, else 0 --
// the reference's interpolated_vuv > 0.5 (synthesis.cpp:301-308); none, 0.  Then the target, then the scale.
__global__ void modify_frames_f0(ModifyFramesParams p) {
  const int j = flat_thread_x(), u = blockIdx.y;
  if (j >= p.n_out[u]) return;
  const size_t at = (size_t)u * p.o_stride + j;
  const SourcePosition s = source_position(p.time_map, at, j, p.m.n_frames[u]);
  const double *src = p.f0_src + (size_t)u * p.m.f_stride;
  double v = src[s.k];
  if (s.blend) {
    const double v1 = src[s.k1], w = s.w;
    const bool a = voiced_f0(v), b = voiced_f0(v1);
    if (a && b) v = (1.0 - w) * v + w * v1;
    else if (a) v = 1.0 - w > 0.5 ? v : 0.0;
    else if (b) v = w > 0.5 ? v1 : 0.0;
    else v = 0.0;
  }
  if (p.f0_target && voiced_f0(v)) {
    const double t = p.f0_target[at];
    if (voiced_f0(t)) v = t;
  }
  p.m.f0_out[at] = v * (p.f0_scale ? valid_scale(p.f0_scale[at]) : p.m.f0_scale[u]);
}

size_t modify_warp_lds_bytes(int fft_size) { return 2 * sizeof(double) * (fft_size / 2 + 1); }

void launch_modify_warp_sp(const ModifyParams &p, int max_frames, hipStream_t stream) {
  WH_BLOCKS(modify_warp_sp, dim3(max_frames, p.n_utt), 256, modify_warp_lds_bytes(p.fft_size), stream, p);
}
void launch_modify_f0(const ModifyParams &p, hipStream_t stream) {
  WH_BLOCKS(modify_f0, dim3(p.n_utt), 256, sizeof(double) * 128, stream, p);
}
void launch_modify_frames_sp(const ModifyFramesParams &p, int max_out, hipStream_t stream) {
  WH_BLOCKS(modify_frames_sp, dim3(max_out, p.m.n_utt), 256, modify_warp_lds_bytes(p.m.fft_size), stream, p);
}
void launch_modify_frames_ap(const ModifyFramesParams &p, int max_out, hipStream_t stream) {
  WH_BLOCKS(modify_frames_ap, dim3(max_out, p.m.n_utt), 256, 0, stream, p);
}
void launch_modify_frames_f0(const ModifyFramesParams &p, int max_out, hipStream_t stream) {
  WH_THREADS(modify_frames_f0, max_out, p.m.n_utt, 1, stream, p);
}

void launch_code_spectral_envelope(const CodecParams &p, hipStream_t stream) {
  WH_BLOCKS(codec_code_sp, dim3(p.rows), 256, code_sp_lds_bytes(p.lg_md), stream, p);
}
void launch_decode_spectral_envelope(const CodecParams &p, hipStream_t stream) {
  WH_BLOCKS(codec_decode_sp, dim3(p.rows), 256, decode_sp_lds_bytes(p.lg_md), stream, p);
}
void launch_code_aperiodicity(const CodecParams &p, hipStream_t stream) {
  WH_THREADS(codec_code_ap, (long)p.rows * p.ndim, 1, 1, stream, p);
}
void launch_decode_aperiodicity(const CodecParams &p, hipStream_t stream) {
  WH_THREADS(codec_decode_ap, (long)p.rows * (p.fft_size / 2 + 1), 1, 1, stream, p);
}
void launch_stage_records(const StageRecordsParams &p, int max_frames, hipStream_t stream) {
  if (max_frames <= 0) return;
  WH_BLOCKS(sy_stage_records, dim3(max_frames, p.n_utt), 256, p.wire == 2 ? decode_sp_lds_bytes(p.lg_md) : 0, stream, p);
}
void launch_rt_store_coded_rows(const RtCodedRowsParams &p, hipStream_t stream) {
  if (p.n <= 0) return;
  WH_BLOCKS(rt_store_coded_rows, dim3(p.n), 256, decode_sp_lds_bytes(p.lg_md), stream, p);
}

#include "align.inc"
#include "morph.inc"
#include "mcep.inc"
#include "mlpg.inc"
#include "gmm.inc"
#include "corpus.h"

}  // namespace world_hip
