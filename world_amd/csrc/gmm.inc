// gmm.inc -- joint-density Gaussian mixture (world_hip_gmm_convert / world_hip_gmm_accumulate; the rule is in
// include/world_hip.h), included by codec.hip inside namespace world_hip behind mcep.inc, whose accumulator, fragment and
// instruction helpers it uses.  DESIGN.md 3.17.
// Conversion is two passes over the mixtures with the posterior between them (the alternative, one pass with running sums
// rescaled whenever a larger q turns up, would make a row's sums depend on the order in which the maxima arrive and multiply
// every term by one more rounded factor; two passes keep each output the plain ascending sum the rule states, and the
// E-step of a fit needs the first pass alone):
//   gmm_q          grid ceil(rows / BM), 256 threads = 4 wavefronts, wavefront w owns rows 16 w .. 16 w + 15 of the block's
//                  BM = 64.  The x tile [BM][Kp] is staged once (+0.0 where the row or the column does not exist).  For each
//                  mixture the block walks k in chunks of 16: the chunk of U' [16][Kp] and of mu_x go to LDS -- from
//                  registers that were loaded while the previous chunk was being multiplied -- and each wavefront runs four
//                  k-steps of v_mfma_f64_16x16x4_f64 per column tile, the A operand formed as x - mu_x on the way out of
//                  LDS.  U is lower triangular: column tile j needs k < 16 (j + 1) only, so chunk c is neither fetched nor
//                  multiplied for the tiles j < c.  After the last chunk each lane squares its results and adds them, column
//                  tiles ascending, into red [row][column mod 16] in LDS; one thread per row adds the sixteen ascending and
//                  writes q = c_m - sum / 2 to the workspace.
//   gmm_posterior  one thread per row: the largest q and the lowest mixture that attains it, the sum of exp(q - q_max) over
//                  ascending m, loglik, gamma = exp(q - q_max) / sum written over q (and to d_post).
//   gmm_regress    the same product with A' [16][Ep] in place of U' (no triangle).  After a mixture's last chunk
//                  e = mu_y + accumulator; mode 0 adds gamma e and gamma (v + e e) to two running accumulators of the
//                  accumulator's own shape, mode 1 keeps e and v of the row's best mixture.
//   LDS            x rows Kp + 2 doubles apart, table rows N + 16 apart (mcep.inc's reasoning); at Kp = Ep = 128:
//                  66.6 + 18.4 + 8.8 KB, one workgroup per CU; at 64: 33.8 + 10.2 + 8.8 KB, three.
//   registers      eight accumulators of four doubles (and twice that again in gmm_regress): 64 (192) of the 512 a wavefront
//                  has when the workgroup is alone on its SIMDs.
//   gmm_accumulate grid (tiles of the (P + 1) x (P + 1) statistics, mixtures); a tile is 64 x 64 (16 x 64 per wavefront) and
//                  only those that meet the lower triangle work.  Dimension P is the column of ones: row P of the product is
//                  S1 and N.  The block runs down t in chunks of 64: gamma (z - s) [64][64] transposed into LDS as the A
//                  operand, (z - s) [64][64] as B (75 KB), sixteen k-steps per column tile, t ascending throughout: one accumulator per
//                  element from the first row to the last, whatever the launch.  Elements on or below the diagonal are
//                  written, and their mirror.
// The host emulation (-DWORLD_EMU: one lane per wavefront, one wavefront per workgroup) runs this text with BM = 16.

#ifdef WORLD_EMU
struct GmmFragA { double v[16][4]; };
__device__ __forceinline__ void gmm_frag_a(GmmFragA &f, const double *tile, int ld, const double *mu) {
  for (int r = 0; r < 16; ++r)
    for (int k = 0; k < 4; ++k) f.v[r][k] = tile[r * ld + k] - mu[k];
}
__device__ __forceinline__ void gmm_mma(McepAcc &acc, const GmmFragA &a, const McepFrag &b) {
  mcep_mma(acc, McepFrag{&a.v[0][0], 4}, b);
}
// f(row, column, a's element, b's element, c's element) with a and b writable
template <class F> __device__ __forceinline__ void gmm_each(McepAcc &a, McepAcc &b, const McepAcc &c, F f) {
  for (int r = 0; r < 16; ++r)
    for (int k = 0; k < 16; ++k) f(r, k, a.c[r][k], b.c[r][k], c.c[r][k]);
}
#else
typedef double GmmFragA;
__device__ __forceinline__ void gmm_frag_a(GmmFragA &f, const double *tile, int ld, const double *mu) {
  const int l = lane_id();
  f = tile[(l & 15) * ld + (l >> 4)] - mu[l >> 4];
}
__device__ __forceinline__ void gmm_mma(McepAcc &acc, const GmmFragA &a, const McepFrag &b) { mcep_mma(acc, a, b); }
template <class F> __device__ __forceinline__ void gmm_each(McepAcc &a, McepAcc &b, const McepAcc &c, F f) {
  const int l = lane_id();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double x = a.c[i], y = b.c[i];
    f((l >> 4) + 4 * i, l & 15, x, y, c.c[i]);
    a.c[i] = x;
    b.c[i] = y;
  }
}
#endif

constexpr int kGmmChunk = 16, kGmmTiles = kGmmMaxPad / 16, kGmmRed = 17;
constexpr int kGmmBM = 16 * kMcepWaves;

__host__ __device__ inline size_t gmm_product_lds_doubles(int Kp, int N) {
  return (size_t)kGmmBM * (Kp + 2) + (size_t)kGmmChunk * (N + 16) + kGmmChunk + (size_t)kGmmBM * kGmmRed;
}

template <bool REGRESS> __device__ __forceinline__ void gmm_product(const GmmParams &p) {
  constexpr int BM = kGmmBM;
  const int Kp = p.Kp, N = REGRESS ? p.Ep : p.Kp, nt = N / 16, lda = Kp + 2, ldb = N + 16;
  DYN_LDS(lds_raw);
  double *xs = reinterpret_cast<double *>(lds_raw), *bs = xs + BM * lda, *mus = bs + kGmmChunk * ldb, *red = mus + kGmmChunk;
  const int tid = threadIdx.x, wave = wave_in_block();
  const long long row0 = (long long)blockIdx.x * BM;
  const double *table = p.model + (REGRESS ? p.off_at : p.off_ut), *mux = p.model + p.off_mux;
  for (int e = tid; e < BM * Kp; e += kMcepLanes) {
    const int r = e / Kp, k = e % Kp;
    const long long row = row0 + r;
    xs[r * lda + k] = row < p.rows && k < p.Dx ? p.x[(size_t)row * p.x_rs + k] : 0.0;
  }
  McepAcc acc[kGmmTiles], sum1[REGRESS ? kGmmTiles : 1], sum2[REGRESS ? kGmmTiles : 1];
  if constexpr (REGRESS)
    for (int j = 0; j < kGmmTiles; ++j) { mcep_zero(sum1[j]); mcep_zero(sum2[j]); }
  // a chunk's elements of this thread, [16][128] at the most: fetched one chunk ahead
  constexpr int B_IT = kGmmChunk * kGmmMaxPad / kMcepLanes;
  double vb[B_IT];
  auto fetch = [&](int m, int k0) {
    const double *src = table + ((size_t)m * Kp + k0) * N;
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int e = tid + it * kMcepLanes, kk = e / kGmmMaxPad, c = e % kGmmMaxPad;
      if (c < N && (REGRESS || c >= k0)) vb[it] = src[(size_t)kk * N + c];
    }
  };
  fetch(0, 0);
  int m = 0, k0 = 0, fm = 0, fk = 0;
  for (;;) {
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int e = tid + it * kMcepLanes, kk = e / kGmmMaxPad, c = e % kGmmMaxPad;
      if (c < N && (REGRESS || c >= k0)) bs[kk * ldb + c] = vb[it];
    }
    for (int e = tid; e < kGmmChunk; e += kMcepLanes) mus[e] = mux[(size_t)m * Kp + k0 + e];
    if constexpr (REGRESS) {                                // the rows' weights of this mixture
      if (k0 == 0)
        for (int r = tid; r < BM; r += kMcepLanes) {
          const long long row = row0 + r;
          red[r] = row >= p.rows ? 0.0 : p.mode == 0 ? p.q[(size_t)row * p.M + m] : p.best[row] == m ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    fk += kGmmChunk;
    if (fk >= Kp) { fk = 0; ++fm; }
    if (fm < p.M) fetch(fm, fk);
    if (k0 == 0)
      for (int j = 0; j < kGmmTiles; ++j) mcep_zero(acc[j]);
    const double *xw = xs + wave * 16 * lda + k0;
#pragma unroll
    for (int ks = 0; ks < kGmmChunk; ks += 4) {
      GmmFragA a;
      gmm_frag_a(a, xw + ks, lda, mus + ks);
#pragma unroll
      for (int j = 0; j < kGmmTiles; ++j)
        if (j < nt && (REGRESS || 16 * j >= k0)) gmm_mma(acc[j], a, mcep_frag_b(bs + ks * ldb + 16 * j, ldb));
    }
    if (k0 + kGmmChunk >= Kp) {                             // the mixture's last chunk
      if constexpr (REGRESS) {
        const double *muy = p.model + p.off_muy + (size_t)m * p.Ep, *v = p.model + p.off_v + (size_t)m * p.Ep;
        const int mode = p.mode;
#pragma unroll
        for (int j = 0; j < kGmmTiles; ++j)
          if (j < nt)
            gmm_each(sum1[j], sum2[j], acc[j], [&](int r, int c, double &s1, double &s2, double prod) {
              const double g = red[wave * 16 + r], e = muy[16 * j + c] + prod, vv = v[16 * j + c];
              if (mode == 0) {
                s1 = s1 + g * e;
                s2 = s2 + g * (vv + e * e);
              } else if (g != 0.0) {
                s1 = e;
                s2 = vv;
              }
            });
      } else {
#pragma unroll
        for (int j = 0; j < kGmmTiles; ++j)
          if (j < nt)
            mcep_each(acc[j], [&](int r, int c, double z) {
              double *s = red + (wave * 16 + r) * kGmmRed + c;
              *s = (j == 0 ? 0.0 : *s) + z * z;
            });
        __syncthreads();
        const double cm = p.model[p.off_c + m];
        for (int r = tid; r < BM; r += kMcepLanes) {
          const long long row = row0 + r;
          if (row < p.rows) {
            double s = 0.0;
            for (int c = 0; c < 16; ++c) s = s + red[r * kGmmRed + c];
            p.q[(size_t)row * p.M + m] = cm - 0.5 * s;
          }
        }
      }
      lds_dead(red, BM * kGmmRed);                          // the next mixture's weights / squares start afresh
    }
    lds_dead(bs, kGmmChunk * ldb + kGmmChunk);              // the chunk and its mu_x: the next one is read only where it is written
    __syncthreads();
    k0 += kGmmChunk;
    if (k0 >= Kp) {
      k0 = 0;
      if (++m >= p.M) break;
    }
  }
  if constexpr (REGRESS) {
#pragma unroll
    for (int j = 0; j < kGmmTiles; ++j)
      if (j < nt)
        gmm_each(sum1[j], sum2[j], acc[j], [&](int r, int c, double &s1, double &s2, double) {
          const long long row = row0 + wave * 16 + r;
          const int col = 16 * j + c;
          if (row < p.rows && col < p.Dy) {
            if (p.mean) p.mean[(size_t)row * p.mean_rs + col] = s1;
            if (p.var) p.var[(size_t)row * p.var_rs + col] = p.mode == 0 ? s2 - s1 * s1 : s2;
          }
        });
  }
}
__global__ void __launch_bounds__(kMcepThreads) gmm_q(GmmParams p) { gmm_product<false>(p); }
__global__ void __launch_bounds__(kMcepThreads) gmm_regress(GmmParams p) { gmm_product<true>(p); }

__global__ void gmm_posterior(GmmParams p) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= p.rows) return;
  double *q = p.q + (size_t)row * p.M;
  double q_max = q[0];
  int best = 0;
  for (int m = 1; m < p.M; ++m)
    if (q[m] > q_max) { q_max = q[m]; best = m; }
  double s = 0.0;
  for (int m = 0; m < p.M; ++m) s = s + exp(q[m] - q_max);
  if (p.loglik) p.loglik[row] = q_max + log(s);
  for (int m = 0; m < p.M; ++m) {
    const double g = exp(q[m] - q_max) / s;
    q[m] = g;
    if (p.post) p.post[(size_t)row * p.post_rs + m] = g;
  }
  p.best[row] = best;
}

void launch_gmm_q(const GmmParams &p, hipStream_t stream) {
  const dim3 grid((unsigned)(((long long)p.rows + kGmmBM - 1) / kGmmBM));
  WH_BLOCKS(gmm_q, grid, kMcepThreads, sizeof(double) * gmm_product_lds_doubles(p.Kp, p.Kp), stream, p);
}
void launch_gmm_posterior(const GmmParams &p, hipStream_t stream) { WH_THREADS(gmm_posterior, (long)p.rows, 1, 1, stream, p); }
void launch_gmm_regress(const GmmParams &p, hipStream_t stream) {
  const dim3 grid((unsigned)(((long long)p.rows + kGmmBM - 1) / kGmmBM));
  WH_BLOCKS(gmm_regress, grid, kMcepThreads, sizeof(double) * gmm_product_lds_doubles(p.Kp, p.Ep), stream, p);
}

// ---- the sufficient statistics
constexpr int kGmmAccBN = 64, kGmmAccChunk = 64, kGmmAccLda = kGmmAccChunk + 2, kGmmAccLdb = kGmmAccBN + 16;

__global__ void __launch_bounds__(kMcepThreads) gmm_accumulate(GmmAccParams p) {
  constexpr int BM = kGmmBM, BN = kGmmAccBN, NT = BN / 16;
  const int P = p.P, Pa = P + 1, tiles_j = (Pa + BN - 1) / BN;
  const int i0 = (int)(blockIdx.x / tiles_j) * BM, j0 = (int)(blockIdx.x % tiles_j) * BN, m = (int)blockIdx.y;
  if (i0 + BM - 1 < j0) return;                             // wholly above the diagonal: its mirror's block writes it
  DYN_LDS(lds_raw);
  double *as = reinterpret_cast<double *>(lds_raw), *bs = as + BM * kGmmAccLda;
  const int tid = threadIdx.x, wave = wave_in_block();
  const double *shift = p.shift + (size_t)m * P;
  McepAcc acc[NT];
  for (int j = 0; j < NT; ++j) mcep_zero(acc[j]);
  constexpr int A_IT = BM * kGmmAccChunk / kMcepLanes, B_IT = kGmmAccChunk * BN / kMcepLanes;
  double va[A_IT], vb[B_IT];
  // d[t][i] = z[t][i] - s[i], 1 in the column of ones, +0.0 where the row or the column does not exist
  // (the loads are unconditional, from the nearest element that exists, and the choice comes after them: loads under a
  // branch each wait for their own data, and a chunk then costs thirty-two memory latencies in a row)
  auto centred = [&](long long t, int i) {
    const long long tc = t < p.rows ? t : p.rows - 1;
    const int ic = i < P ? i : P - 1;
    const double d = p.z[(size_t)tc * p.z_rs + ic] - shift[ic];
    return t >= p.rows || i > P ? 0.0 : i == P ? 1.0 : d;
  };
  auto fetch = [&](long long t0) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int e = tid + it * kMcepLanes, tt = e / BM, r = e % BM;
      const long long t = t0 + tt, tc = t < p.rows ? t : p.rows - 1;
      const double g = p.post[(size_t)tc * p.post_rs + m], d = centred(t, i0 + r);
      va[it] = t < p.rows && i0 + r <= P ? d * g : 0.0;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int e = tid + it * kMcepLanes, tt = e / BN, c = e % BN;
      vb[it] = centred(t0 + tt, j0 + c);
    }
  };
  fetch(0);
  for (long long t0 = 0; t0 < p.rows; t0 += kGmmAccChunk) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int e = tid + it * kMcepLanes, tt = e / BM, r = e % BM;
      as[r * kGmmAccLda + tt] = va[it];
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int e = tid + it * kMcepLanes, tt = e / BN, c = e % BN;
      bs[tt * kGmmAccLdb + c] = vb[it];
    }
    __syncthreads();
    if (t0 + kGmmAccChunk < p.rows) fetch(t0 + kGmmAccChunk);
    const double *aw = as + wave * 16 * kGmmAccLda;
#pragma unroll
    for (int ks = 0; ks < kGmmAccChunk; ks += 4) {
      const McepFrag a = mcep_frag_a(aw + ks, kGmmAccLda);
#pragma unroll
      for (int j = 0; j < NT; ++j) mcep_mma(acc[j], a, mcep_frag_b(bs + ks * kGmmAccLdb + 16 * j, kGmmAccLdb));
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NT; ++j)
    mcep_each(acc[j], [&](int r, int c, double v) {
      const int i = i0 + wave * 16 + r, jj = j0 + 16 * j + c;
      if (i > P || jj > i) return;
      if (i < P) {
        p.G[((size_t)m * P + i) * P + jj] = v;
        p.G[((size_t)m * P + jj) * P + i] = v;
      } else if (jj < P) {
        p.S1[(size_t)m * P + jj] = v;
      } else {
        p.N[m] = v;
      }
    });
}

void launch_gmm_accumulate(const GmmAccParams &p, hipStream_t stream) {
  const int Pa = p.P + 1;
  const dim3 grid((unsigned)(((Pa + kGmmBM - 1) / kGmmBM) * ((Pa + kGmmAccBN - 1) / kGmmAccBN)), (unsigned)p.M);
  const size_t lds = sizeof(double) * ((size_t)kGmmBM * kGmmAccLda + (size_t)kGmmAccChunk * kGmmAccLdb);
  WH_BLOCKS(gmm_accumulate, grid, kMcepThreads, lds, stream, p);
}

__global__ void gmm_fill(double *d, size_t n, double value) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = value;
}
void launch_gmm_fill(double *d, size_t n, double value, hipStream_t stream) { WH_THREADS(gmm_fill, (long)n, 1, 1, stream, d, n, value); }
