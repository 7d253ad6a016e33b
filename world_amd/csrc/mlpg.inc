// mlpg.inc -- dynamic features and maximum-likelihood parameter generation (world_hip_delta_batch / world_hip_mlpg_batch;
// the rule is in include/world_hip.h), included by codec.hip inside namespace world_hip.  DESIGN.md 3.16.
//   delta_rows     : one thread per (utterance, frame, static dimension), consecutive threads consecutive dimensions.  The
//                    frame's run is followed up to L frames either way, the 2 L + 1 (or fewer) statics are read once and
//                    every window's sum runs in ascending tau, product and sum each rounded (no FMA: the rule's arithmetic).
//   mlpg_static    : B = 0 (every window one tap): R and r are one number each per element, c = r / R.  Same grid.
//   mlpg_sweeps<B> : B = 2 or 4.  One lane per (utterance, dimension) system, the 64 lanes of a wavefront 64 consecutive
//                    dimensions of one utterance: every read of mean / var [t][w D + d], every access of the workspace
//                    [t][B + 1][system] and every write of out [t][d] is one coalesced row.  No cross-lane operation.
//     forward       banded L D L^T without square roots, right-looking.  A window of B + 2 rows of R (B + 1 band entries and
//                   the right-hand side each) lives in registers.  Step i first adds observation o = i + L + 1 -- its
//                   precisions, means and truncated window coefficients -- to rows o - L .. o + L = i + 1 .. i + B + 1, then
//                   eliminates row i: inv = 1 / d_i, l_m = R[i][i + m] inv, y_i = r_i inv, rows i + 1 .. i + B updated by
//                   fma(-l_m, .., ..).  So row i + 1 has every observation before row i touches it, and the serial chain
//                   per frame is the reciprocal, one product and one FMA.  Observations are read PD = B + 2 frames ahead
//                   into a register ring (the mask bytes 2 PD ahead: a masked row is never read), so no global-load latency
//                   is on the chain.  The loop is unrolled B + 2 times, which turns both rings' indices into constants.
//                   The sweep starts at i = -(L + 1): frames outside the utterance are masked frames.  Addresses are running
//                   offsets and the windows go through 160 bytes of LDS into vector registers: per-slot base addresses and
//                   twenty uniform doubles beside the strides would not fit the scalar register file.
//     mask          a term (t, tau) that does not count has coefficient 0, a masked frame precision 0 and pivot 1: its
//                   couplings and its right-hand side come out as zeros, the updates it sends on are fma(-0, .., x) = x, and a
//                   run of present frames goes through exactly the operations of an utterance of its own.
//     backward      c_i = y_i - sum_m l[i][m] c_{i + m}, the c_{i + 1} term last: one FMA on the chain.  The rows of the
//                   workspace are read four frames ahead, the last B results live in a ring of four.
// The host emulation (-DWORLD_EMU: one lane per wavefront) runs this very text; fma() is the fused operation in both.

constexpr int kMlpgLanes = WAVE;                         // threads of a workgroup of the sweeps: one wavefront

__device__ __forceinline__ bool mlpg_present(const unsigned char *mask, int t, int T) {
  return t >= 0 && t < T && (!mask || mask[t] != 0);
}

// (u, t, d) of a thread of the flat kernels; false: nothing to do
__device__ __forceinline__ bool mlpg_element(const MlpgParams &p, int *u, int *t, int *d, int *T) {
  *u = p.u0 + (int)blockIdx.y;
  *T = p.n_frames[*u];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)*T * p.dim) return false;
  *t = (int)(e / p.dim);
  *d = (int)(e % p.dim);
  return true;
}

template <int L> __device__ __forceinline__ void delta_rows_impl(const MlpgParams &p) {
#pragma clang fp contract(off)
  int u, t, d, T;
  if (!mlpg_element(p, &u, &t, &d, &T)) return;
  const unsigned char *mask = p.mask ? p.mask + (size_t)u * p.mask_us : nullptr;
  double *out = p.out + (size_t)u * p.out_us + (size_t)t * p.out_rs + d;
  if (!mlpg_present(mask, t, T)) {
    for (int w = 0; w < p.n_win; ++w) out[(size_t)w * p.dim] = p.fill;
    return;
  }
  int lo = 0, hi = 0;                                    // how far the run reaches either way, L at the most
  while (lo < L && mlpg_present(mask, t - lo - 1, T)) ++lo;
  while (hi < L && mlpg_present(mask, t + hi + 1, T)) ++hi;
  const double *in = p.mean + (size_t)u * p.mean_us + d;
  double c[2 * L + 1];
#pragma unroll
  for (int k = 0; k <= 2 * L; ++k) c[k] = k - L >= -lo && k - L <= hi ? in[(size_t)(t + k - L) * p.mean_rs] : 0.0;
  for (int w = 0; w < p.n_win; ++w) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k <= 2 * L; ++k)
      if (k - L >= -lo && k - L <= hi) acc = acc + p.win[w][k - L + 2] * c[k];
    out[(size_t)w * p.dim] = acc;
  }
}
__global__ void delta_rows_0(MlpgParams p) { delta_rows_impl<0>(p); }
__global__ void delta_rows_1(MlpgParams p) { delta_rows_impl<1>(p); }
__global__ void delta_rows_2(MlpgParams p) { delta_rows_impl<2>(p); }

__device__ __forceinline__ double mlpg_precision(const MlpgParams &p, double v) { return p.precision ? v : 1.0 / v; }

__global__ void mlpg_static(MlpgParams p) {
  int u, t, d, T;
  if (!mlpg_element(p, &u, &t, &d, &T)) return;
  const unsigned char *mask = p.mask ? p.mask + (size_t)u * p.mask_us : nullptr;
  double *out = p.out + (size_t)u * p.out_us + (size_t)t * p.out_rs + d;
  if (!mlpg_present(mask, t, T)) {
    *out = p.fill;
    return;
  }
  const double *mean = p.mean + (size_t)u * p.mean_us + (size_t)t * p.mean_rs + d;
  const double *var = p.var + (size_t)u * p.var_us + (size_t)t * p.var_rs + d;
  double R = 0.0, r = 0.0;
  for (int w = 0; w < p.n_win; ++w) {
    const double q = mlpg_precision(p, var[(size_t)w * p.dim]) * p.win[w][2];
    R = fma(q, p.win[w][2], R);
    r = fma(q, mean[(size_t)w * p.dim], r);
  }
  *out = r / R;
}

template <int B> __device__ __forceinline__ void mlpg_sweeps_impl(const MlpgParams &p) {
  constexpr int L = B / 2, NR = B + 2, PD = NR, NB = 4;
  DYN_LDS(lds_raw);
  double *wl = reinterpret_cast<double *>(lds_raw);
  for (int k = (int)threadIdx.x; k < 20; k += (int)blockDim.x) wl[k] = p.win[k / 5][k % 5];
  __syncthreads();
  const int u = p.u0 + (int)blockIdx.y;
  const int d = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (d >= p.dim) return;
  const int T = p.n_frames[u], nw = p.n_win;
  const size_t D = (size_t)p.dim;
  const unsigned char *mask = p.mask ? p.mask + (size_t)u * p.mask_us : nullptr;
  const double *mean = p.mean + (size_t)u * p.mean_us + d;
  const double *var = p.var + (size_t)u * p.var_us + d;
  double *out = p.out + (size_t)u * p.out_us + d;
  double *ws = p.ws + ((size_t)u * D + d);               // [t][B + 1][system]
  const size_t ws_k = (size_t)p.n_sys, ws_t = (size_t)(B + 1) * ws_k;

  // ---- forward
  double A[NR][B + 1], Rh[NR];                           // rows i .. i + B + 1 of R's upper band and of r, row j in slot j mod NR
  double rv[PD][4], rm[PD][4];                           // observations o .. o + PD - 1 in flight
  unsigned char mk[PD];                                  // mask bytes of frames o + PD .. o + 2 PD - 1 in flight
  unsigned pbits = 0;                                    // bit j: frame o + PD - 1 - j is present
  size_t om = 0, ov = 0, ow = 0;                         // where the next frame to fetch (to store) lies in mean, var (ws)
#pragma unroll
  for (int s = 0; s < NR; ++s) {
    Rh[s] = 0.0;
    for (int k = 0; k <= B; ++k) A[s][k] = 0.0;
    for (int w = 0; w < 4; ++w) rv[s][w] = rm[s][w] = 0.0;
    mk[s] = 0;
  }
#pragma unroll
  for (int s = 0; s < PD; ++s) {
    const bool pf = mlpg_present(mask, s, T);
    pbits = (pbits << 1) | (pf ? 1u : 0u);
    if (pf) {
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (w < nw) {
          rm[s][w] = mean[om + w * D];
          rv[s][w] = var[ov + w * D];
        }
    }
    om += (size_t)p.mean_rs;
    ov += (size_t)p.var_rs;
    if (mask && s + PD < T) mk[s] = mask[s + PD];
  }
  for (int o0 = 0; o0 - (L + 1) < T; o0 += NR) {
#pragma unroll
    for (int s = 0; s < NR; ++s) {
      const int o = o0 + s, i = o - (L + 1);
      if (i < T) {
        auto pres = [&](int k) { return ((pbits >> (PD - 1 - k)) & 1u) != 0; };   // is frame o + k present
        // the observation o: which of its terms count, then its share of rows o - L .. o + L
        if (pres(0)) {
          bool cnt[2 * L + 1];
          cnt[L] = true;
#pragma unroll
          for (int k = 1; k <= L; ++k) {
            cnt[L + k] = cnt[L + k - 1] && pres(k);
            cnt[L - k] = cnt[L - k + 1] && pres(-k);
          }
#pragma unroll
          for (int w = 0; w < 4; ++w)
            if (w < nw) {
              const double pw = mlpg_precision(p, rv[s][w]), mu = rm[s][w];
              double cf[2 * L + 1];
#pragma unroll
              for (int a = 0; a <= 2 * L; ++a) cf[a] = cnt[a] ? wl[w * 5 + a - L + 2] : 0.0;
#pragma unroll
              for (int a = 0; a <= 2 * L; ++a) {
                const double q = pw * cf[a];
                const int row = (s + 1 + a) % NR;        // row o - L + a = i + 1 + a
                Rh[row] = fma(q, mu, Rh[row]);
#pragma unroll
                for (int b = a; b <= 2 * L; ++b) A[row][b - a] = fma(q, cf[b], A[row][b - a]);
              }
            }
        }
        // row i
        const double inv = 1.0 / (pres(-(L + 1)) ? A[s][0] : 1.0);
        double l[B + 1];
        l[0] = Rh[s] * inv;
#pragma unroll
        for (int m = 1; m <= B; ++m) l[m] = A[s][m] * inv;
        if (i >= 0) {
#pragma unroll
          for (int k = 0; k <= B; ++k) ws[ow + k * ws_k] = l[k];
          ow += ws_t;
        }
#pragma unroll
        for (int m = 1; m <= B; ++m) {
          const int row = (s + m) % NR;
          Rh[row] = fma(-l[m], Rh[s], Rh[row]);
#pragma unroll
          for (int k = 0; k + m <= B; ++k) A[row][k] = fma(-l[m], A[s][m + k], A[row][k]);
        }
        Rh[s] = 0.0;
#pragma unroll
        for (int k = 0; k <= B; ++k) A[s][k] = 0.0;
        // frame o + PD takes the observation's place in the ring, the mask byte of frame o + 2 PD that frame's
        const int f = o + PD;
        const bool pf = f < T && (!mask || mk[s] != 0);
        pbits = (pbits << 1) | (pf ? 1u : 0u);
        if (pf) {
#pragma unroll
          for (int w = 0; w < 4; ++w)
            if (w < nw) {
              rm[s][w] = mean[om + w * D];
              rv[s][w] = var[ov + w * D];
            }
        }
        om += (size_t)p.mean_rs;
        ov += (size_t)p.var_rs;
        if (mask && f + PD < T) mk[s] = mask[f + PD];
      }
    }
  }

  // ---- backward: step j is frame i = T - 1 - j, its row and its result in slot j mod NB
  double bw[NB][B + 1], cr[NB];
  bool bp[NB];
  size_t oo = (size_t)(T - 1) * p.out_rs;                // where the frame to write (ow: to fetch) lies in out (ws)
  ow = (size_t)(T - 1) * ws_t;
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    cr[s] = 0.0;
    bp[s] = false;
    for (int k = 0; k <= B; ++k) bw[s][k] = 0.0;
    const int i = T - 1 - s;
    if (i >= 0) {
      bp[s] = !mask || mask[i] != 0;
#pragma unroll
      for (int k = 0; k <= B; ++k) bw[s][k] = ws[ow + k * ws_k];
      ow -= ws_t;
    }
  }
  for (int j0 = 0; j0 < T; j0 += NB) {
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      const int i = T - 1 - (j0 + s);
      if (i >= 0) {
        double acc = bw[s][0];
#pragma unroll
        for (int m = B; m >= 1; --m) acc = fma(-bw[s][m], cr[(s + NB - m) % NB], acc);   // c_{i + m}: m steps ago
        cr[s] = acc;
        out[oo] = bp[s] ? acc : p.fill;
        oo -= (size_t)p.out_rs;
        const int f = i - NB;
        if (f >= 0) {
          bp[s] = !mask || mask[f] != 0;
#pragma unroll
          for (int k = 0; k <= B; ++k) bw[s][k] = ws[ow + k * ws_k];
          ow -= ws_t;
        }
      }
    }
  }
}
__global__ void __launch_bounds__(64) mlpg_sweeps_2(MlpgParams p) { mlpg_sweeps_impl<2>(p); }
__global__ void __launch_bounds__(64) mlpg_sweeps_4(MlpgParams p) { mlpg_sweeps_impl<4>(p); }

// doubles of workspace the sweeps of a call keep: the factor's B sub-diagonals and the scaled right-hand side per frame
size_t mlpg_workspace_doubles(int n_utt, int dim, int max_frames, int half_width) {
  return half_width == 0 ? 0 : (size_t)max_frames * (2 * half_width + 1) * ((size_t)n_utt * dim);
}

// the flat kernels: utterances [p.u0, p.u0 + n_utt) of at most max_frames frames
void launch_delta(const MlpgParams &p, int half_width, int n_utt, int max_frames, hipStream_t stream) {
  const long items = (long)max_frames * p.dim;
  if (half_width == 0) WH_THREADS(delta_rows_0, items, (unsigned)n_utt, 1, stream, p);
  else if (half_width == 1) WH_THREADS(delta_rows_1, items, (unsigned)n_utt, 1, stream, p);
  else WH_THREADS(delta_rows_2, items, (unsigned)n_utt, 1, stream, p);
}
void launch_mlpg(const MlpgParams &p, int half_width, int n_utt, int max_frames, hipStream_t stream) {
  if (half_width == 0) {
    WH_THREADS(mlpg_static, (long)max_frames * p.dim, (unsigned)n_utt, 1, stream, p);
    return;
  }
  const dim3 grid((unsigned)((p.dim + kMlpgLanes - 1) / kMlpgLanes), (unsigned)n_utt);
  if (half_width == 1) WH_BLOCKS(mlpg_sweeps_2, grid, kMlpgLanes, sizeof(p.win), stream, p);
  else WH_BLOCKS(mlpg_sweeps_4, grid, kMlpgLanes, sizeof(p.win), stream, p);
}
