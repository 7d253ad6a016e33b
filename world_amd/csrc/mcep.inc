// mcep.inc -- all-pass mel-cepstra (world_hip_sp2mc / world_hip_mc2sp; the rule is in include/world_hip.h), included by
// codec.hip inside namespace world_hip.  DESIGN.md 3.15.
// Both directions are one product: out [rows][k_out] = f(in [rows][k_in]) x table [k_in][k_out], ln on the way in (encode)
// or exp on the way out (decode).  One kernel template, mcep_product<MT, NT, LN, EXP>:
//   grid      (ceil(rows / BM), n_pad / BN), 256 threads = 4 wavefronts.  BM = 64 MT rows, BN = 16 NT columns; wavefront w
//             owns rows 16 MT w .. 16 MT (w + 1) - 1 of the block and all BN columns: MT x NT accumulators of 16 x 16, each
//             four doubles per lane.  Encode launches with BN >= k_out (NT = 4, 8 or 16 for up to 64, 128, 256
//             coefficients), so grid.y = 1: an envelope element is read once and goes through ln once.  Decode walks the
//             bins in grid.y chunks of 64; what it re-reads per chunk is the short cepstrum rows.
//   k loop    chunks of 32: the input tile [BM][32] (ln applied as it is staged; +0.0 where the row or the column does not
//             exist) and the table tile [32][BN] go to LDS -- from registers that were loaded while the previous chunk was
//             being multiplied -- then every wavefront runs 8 k-steps of
//             v_mfma_f64_16x16x4_f64 per accumulator, k ascending.  The table on the device is padded with zeros to
//             [k_pad][n_pad] (k_pad a multiple of 32, n_pad of BN), so a padded k-step multiplies a staged zero by a table
//             zero, a padded column a finite input by a table zero; nothing past a row or in unwritten LDS is ever an
//             operand.  A row's sum is the same sequence of operations wherever the row sits: row position only chooses
//             the lane.
//   operands  lane l gives A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15], one double each; the results are
//             C[row (l >> 4) + 4 i][column l & 15] in register i = 0 .. 3 (the f64 map: NOT the f32 16x16x4 one).
//   LDS       input rows 34 doubles apart: the 32 lanes of a half read rows 0 .. 15 at k and k + 1, banks 2 r + {0, 1}, all
//             different.  Table rows BN + 16 doubles apart (16 mod 32): lanes 16 .. 31 read the next table row in the other
//             sixteen banks.  55 KB (NT = 4), 54 KB (8), 87 KB (16): two workgroups per CU, or one.
// The host emulation (-DWORLD_EMU: one lane per wavefront, one wavefront per workgroup) spells the accumulator as a plain
// 16 x 16 array and the instruction as three loops; a workgroup is then one wavefront's rows.

#ifdef WORLD_EMU
constexpr int kMcepWaves = 1;
struct McepAcc { double c[16][16]; };
struct McepFrag { const double *p; int ld; };
__device__ __forceinline__ void mcep_zero(McepAcc &a) { memset(&a, 0, sizeof a); }
__device__ __forceinline__ McepFrag mcep_frag_a(const double *tile, int ld) { return McepFrag{tile, ld}; }
__device__ __forceinline__ McepFrag mcep_frag_b(const double *tile, int ld) { return McepFrag{tile, ld}; }
__device__ __forceinline__ void mcep_mma(McepAcc &acc, const McepFrag &a, const McepFrag &b) {
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c)
      for (int k = 0; k < 4; ++k) acc.c[r][c] = acc.c[r][c] + a.p[r * a.ld + k] * b.p[k * b.ld + c];
}
template <class F> __device__ __forceinline__ void mcep_each(const McepAcc &acc, F f) {
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) f(r, c, acc.c[r][c]);
}
#else
constexpr int kMcepWaves = 4;
typedef double mcep_v4 __attribute__((ext_vector_type(4)));
struct McepAcc { mcep_v4 c; };
typedef double McepFrag;
__device__ __forceinline__ void mcep_zero(McepAcc &a) { a.c = mcep_v4{0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ McepFrag mcep_frag_a(const double *tile, int ld) {
  const int l = lane_id();
  return tile[(l & 15) * ld + (l >> 4)];
}
__device__ __forceinline__ McepFrag mcep_frag_b(const double *tile, int ld) {
  const int l = lane_id();
  return tile[(l >> 4) * ld + (l & 15)];
}
__device__ __forceinline__ void mcep_mma(McepAcc &acc, const McepFrag &a, const McepFrag &b) {
  acc.c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc.c, 0, 0, 0);
}
template <class F> __device__ __forceinline__ void mcep_each(const McepAcc &acc, F f) {
  const int l = lane_id();
  for (int i = 0; i < 4; ++i) f((l >> 4) + 4 * i, l & 15, acc.c[i]);
}
#endif

constexpr int kMcepThreads = 256, kMcepChunk = 32, kMcepLda = kMcepChunk + 2;
constexpr int kMcepLanes = kMcepWaves * WAVE;           // the threads a workgroup really has: 256, or 1 in the host emulation

template <int MT, int NT, bool LN, bool EXP> __device__ __forceinline__ void mcep_product(const McepParams &p) {
  constexpr int BM = 16 * MT * kMcepWaves, BN = 16 * NT, LDB = BN + 16;
  DYN_LDS(lds_raw);
  double *as = reinterpret_cast<double *>(lds_raw), *bs = as + BM * kMcepLda;
  const int tid = threadIdx.x, wave = wave_in_block();
  const long long row0 = (long long)blockIdx.x * BM;
  const int n0 = (int)blockIdx.y * BN;
  McepAcc acc[MT][NT];
  for (int i = 0; i < MT; ++i)
    for (int j = 0; j < NT; ++j) mcep_zero(acc[i][j]);
  // the chunk's elements of this thread: fetched into registers one chunk ahead, so that the loads of chunk c + 1 are in
  // flight while the matrix unit works on chunk c; ln is applied when they go to LDS
  constexpr int A_IT = BM * kMcepChunk / kMcepLanes, B_IT = kMcepChunk * BN / kMcepLanes;
  double va[A_IT], vb[B_IT];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int e = tid + it * kMcepLanes, r = e / kMcepChunk, kk = e % kMcepChunk;
      const long long row = row0 + r;
      va[it] = row < p.rows && k0 + kk < p.k_in ? p.in[(size_t)row * p.in_stride + k0 + kk] : 1.0;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int e = tid + it * kMcepLanes, kk = e / BN, c = e % BN;
      vb[it] = p.table[(size_t)(k0 + kk) * p.n_pad + n0 + c];
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < p.k_pad; k0 += kMcepChunk) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int e = tid + it * kMcepLanes, r = e / kMcepChunk, kk = e % kMcepChunk;
      const bool there = row0 + r < p.rows && k0 + kk < p.k_in;
      as[r * kMcepLda + kk] = there ? (LN ? log(va[it]) : va[it]) : 0.0;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int e = tid + it * kMcepLanes, kk = e / BN, c = e % BN;
      bs[kk * LDB + c] = vb[it];
    }
    __syncthreads();
    if (k0 + kMcepChunk < p.k_pad) fetch(k0 + kMcepChunk);
    const double *aw = as + wave * (16 * MT) * kMcepLda;
#pragma unroll
    for (int ks = 0; ks < kMcepChunk; ks += 4) {
      McepFrag a[MT], b[NT];
      for (int i = 0; i < MT; ++i) a[i] = mcep_frag_a(aw + i * 16 * kMcepLda + ks, kMcepLda);
      for (int j = 0; j < NT; ++j) b[j] = mcep_frag_b(bs + ks * LDB + j * 16, LDB);
      for (int i = 0; i < MT; ++i)
        for (int j = 0; j < NT; ++j) mcep_mma(acc[i][j], a[i], b[j]);
    }
    __syncthreads();
  }
  for (int i = 0; i < MT; ++i)
    for (int j = 0; j < NT; ++j)
      mcep_each(acc[i][j], [&](int r, int c, double v) {
        const long long row = row0 + wave * (16 * MT) + i * 16 + r;
        const int col = n0 + j * 16 + c;
        if (row < p.rows && col < p.k_out) p.out[(size_t)row * p.out_stride + col] = EXP ? exp(v) : v;
      });
}

// (two workgroups per CU is what the LDS of the NT = 4 and 8 shapes allows: the registers are held to that as well)
#ifdef WORLD_EMU
#define MCEP_TWO_PER_SIMD
#else
#define MCEP_TWO_PER_SIMD __attribute__((amdgpu_waves_per_eu(2)))
#endif
__global__ void __launch_bounds__(kMcepThreads) MCEP_TWO_PER_SIMD mcep_encode_64(McepParams p) { mcep_product<2, 4, true, false>(p); }
__global__ void __launch_bounds__(kMcepThreads) MCEP_TWO_PER_SIMD mcep_encode_128(McepParams p) { mcep_product<1, 8, true, false>(p); }
__global__ void __launch_bounds__(kMcepThreads) mcep_encode_256(McepParams p) { mcep_product<1, 16, true, false>(p); }
__global__ void __launch_bounds__(kMcepThreads) MCEP_TWO_PER_SIMD mcep_decode(McepParams p) { mcep_product<2, 4, false, true>(p); }

// the padded shape of the device table: encode [k_pad >= K][n_pad = 64 | 128 | 256 >= P], decode [k_pad >= P][n_pad >= K]
void mcep_table_shape(bool decode, int fft_size, int order, int *k_pad, int *n_pad) {
  const int K = fft_size / 2 + 1, P = order + 1;
  const int k_in = decode ? P : K;
  *k_pad = (k_in + kMcepChunk - 1) / kMcepChunk * kMcepChunk;
  *n_pad = decode ? (K + 63) / 64 * 64 : P <= 64 ? 64 : P <= 128 ? 128 : 256;
}

void launch_mcep(const McepParams &p, bool decode, hipStream_t stream) {
  const int nt = decode || p.n_pad == 64 ? 4 : p.n_pad / 16, mt = nt == 4 ? 2 : 1;   // the instantiations above
  const int bm = 16 * mt * kMcepWaves, bn = 16 * nt;
  const dim3 grid((unsigned)(((long long)p.rows + bm - 1) / bm), (unsigned)(p.n_pad / bn));
  const size_t lds = sizeof(double) * ((size_t)bm * kMcepLda + (size_t)kMcepChunk * (bn + 16));
  if (decode) WH_BLOCKS(mcep_decode, grid, kMcepThreads, lds, stream, p);
  else if (nt == 4) WH_BLOCKS(mcep_encode_64, grid, kMcepThreads, lds, stream, p);
  else if (nt == 8) WH_BLOCKS(mcep_encode_128, grid, kMcepThreads, lds, stream, p);
  else WH_BLOCKS(mcep_encode_256, grid, kMcepThreads, lds, stream, p);
}
