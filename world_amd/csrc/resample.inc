// resample.inc -- sampling-rate conversion by a polyphase Kaiser-windowed sinc (world_hip_resample_batch; the rule is in
// include/world_hip.h), included by pcm.hip inside namespace world_hip.  DESIGN.md 3.14.
//   resample_poly  : grid (ceil(max n_out / tile), n_utt), kResampleThreads threads, one output per thread, `tile` outputs per
//                    workgroup (tile = kResampleThreads unless the input span of that many outputs would not fit the LDS
//                    budget: steep decimations).  Workgroups beyond their utterance's n_out return at once.  The workgroup's
//                    input span -- samples k0(first output) - W + 1 .. k0(last output) + W, at most `span` of them -- is
//                    staged in LDS once, +0.0 where the utterance has no sample; every thread then walks its 2 W taps in
//                    ascending order: acc = acc + x * c, both operations rounded (no FMA).
//   coefficients   : lanes have consecutive m and so scattered phases p = m M mod L; r = m mod L <-> p is a bijection
//                    (gcd(L, M) = 1), and the device table is stored [i][r]: the lanes of a wavefront read consecutive
//                    doubles, wrapping at L.  kdiv[r] = (r M) div L rides along, so that k0 = (m div L) M + kdiv[r] costs one
//                    32-bit division per thread and no 64-bit one.
//   resample_decim : L == 1 (integer decimation): the coefficient of tap i is the same for every lane, and the lanes read
//                    LDS M doubles apart: gcd(M, 32)-way bank conflicts for ds_read_b64 (a 32-lane half over 32 8-byte
//                    banks; the ds_read2_b64 the compiler merges neighbouring taps into conflicts alike over its 16-lane
//                    groups), so 4-way at M = 12 and 8-way at M = 8.  PAD stores sample j at j + (j >> 5), one double of
//                    padding per bank row: 2-way for every even M (tools/lds_bank_model.py resample; the 32 lanes of a half
//                    then span more than 32 rows' worth of slots, so one wrap-around collision remains).  It is used where
//                    it gains, M a multiple of 4; odd M is conflict-free unpadded and M = 2, 6, 10 are 2-way either way.
//   resample_copy  : equal rates -- x_length[u] samples of every row, bit for bit.

constexpr int kResampleThreads = 256;

template <bool PAD> __device__ __forceinline__ int resample_slot(int j) { return PAD ? j + (j >> 5) : j; }

template <bool DECIM, bool PAD> __device__ __forceinline__ void resample_tile(const ResampleParams &p) {
#pragma clang fp contract(off)
  DYN_LDS(lds_raw);
  double *xs = reinterpret_cast<double *>(lds_raw);
  const int u = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int n_out = p.n_out[u], n_in = p.x_len[u];
  const long long m0 = (long long)blockIdx.x * p.tile;
  if (m0 >= n_out) return;
  const unsigned L = (unsigned)p.L;
  // the first sample any output of this workgroup reads
  long long k_first;
  if (DECIM) k_first = m0 * p.M - p.W + 1;
  else k_first = (long long)((unsigned)m0 / L) * p.M + p.kdiv[(unsigned)m0 % L] - p.W + 1;
  const double *x = p.x + (size_t)u * p.x_stride;
  for (int j = tid; j < p.span; j += nt) {
    const long long k = k_first + j;
    xs[resample_slot<PAD>(j)] = k >= 0 && k < n_in ? x[k] : 0.0;
  }
  __syncthreads();
  const int taps = 2 * p.W;
  for (int t = tid; t < p.tile; t += nt) {
    const long long m = m0 + t;
    if (m >= n_out) break;
    int base;                                            // of tap 0 in the staged span: k0 - W + 1 - k_first
    const double *c = p.coef;
    if (DECIM) {
      base = t * p.M;
    } else {
      const unsigned a = (unsigned)m / L, r = (unsigned)m % L;
      base = (int)((long long)a * p.M + p.kdiv[r] - p.W + 1 - k_first);
      c += r;
    }
    double acc = 0.0;
    for (int i = 0; i < taps; ++i) acc = acc + xs[resample_slot<PAD>(base + i)] * c[(size_t)i * L];
    p.y[(size_t)u * p.y_stride + m] = acc;
  }
}

__global__ void __launch_bounds__(kResampleThreads) resample_poly(ResampleParams p) { resample_tile<false, false>(p); }
__global__ void __launch_bounds__(kResampleThreads) resample_decim(ResampleParams p) { resample_tile<true, false>(p); }
__global__ void __launch_bounds__(kResampleThreads) resample_decim_pad(ResampleParams p) { resample_tile<true, true>(p); }

__global__ void resample_copy(ResampleParams p) {
  const int k = flat_thread_x(), u = blockIdx.y;
  if (k < p.x_len[u]) p.y[(size_t)u * p.y_stride + k] = p.x[(size_t)u * p.x_stride + k];
}

// Outputs per workgroup and doubles of LDS for a ratio: kResampleThreads outputs unless their input span exceeds the
// budget of 8192 doubles.  64 KiB (66 KiB padded) is the largest span of which two workgroups still fit a CU's 160 KiB, so
// that one stages while the other walks its taps; it is reached by steep decimations only.  The usual ratios stage 3 KB
// (44.1 -> 48 kHz) to 28 KB (192 -> 16 kHz), where the eight workgroups of 256 threads a CU can hold are not limited by LDS
// up to 20 KB and five fit at 28 KB.
ResamplePlan resample_plan(long long L, long long M, long long W) {
  constexpr long long kBudget = 8192;                    // doubles: 64 KiB
  ResamplePlan pl;
  auto span_of = [&](long long tile) { return ((tile - 1) * M + (L - 1)) / L + 2 * W; };
  long long tile = kResampleThreads;
  if (span_of(tile) > kBudget) tile = std::max<long long>(1, ((kBudget - 2 * W) * L - (L - 1)) / M + 1);
  while (tile > 1 && span_of(tile) > kBudget) --tile;    // (the closed form is exact; this guards its rounding)
  pl.tile = (int)tile;
  pl.span = (int)span_of(tile);
  pl.decim = L == 1;
  pl.pad = L == 1 && M % 4 == 0;
  pl.lds_doubles = pl.pad ? pl.span + (pl.span >> 5) + 1 : pl.span;
  return pl;
}

void launch_resample(const ResampleParams &p, const ResamplePlan &pl, int max_out, int n_utt, hipStream_t stream) {
  const dim3 grid((unsigned)(((long long)max_out + pl.tile - 1) / pl.tile), (unsigned)n_utt);   // (max_out may be INT_MAX)
  const size_t lds = sizeof(double) * (size_t)pl.lds_doubles;
  if (!pl.decim) WH_BLOCKS(resample_poly, grid, kResampleThreads, lds, stream, p);
  else if (pl.pad) WH_BLOCKS(resample_decim_pad, grid, kResampleThreads, lds, stream, p);
  else WH_BLOCKS(resample_decim, grid, kResampleThreads, lds, stream, p);
}
void launch_resample_copy(const ResampleParams &p, int max_len, int n_utt, hipStream_t stream) {
  WH_THREADS(resample_copy, max_len, n_utt, 1, stream, p);
}
