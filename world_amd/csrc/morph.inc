// morph.inc -- the frames between two aligned utterances (world_hip_morph_batch), included by codec.hip inside namespace
// world_hip.  Four launches (DESIGN.md: morph):
//   morph_positions : one thread per (pair, output frame).  Path cell k = (i_k, j_k) lies at the time
//                     t_k = (1.0 - r) * i_k + r * j_k, non-decreasing in k; frame m finds lo = the first k with t_k >= m by
//                     binary search and, where t_lo == m, hi = the last such k by a second one: about 2 log2(K) dependent
//                     8-byte loads, which is why the positions are computed once here and not at the head of every
//                     workgroup of the three row kernels.  Writes sA and sB, clamped into their utterances.
//   morph_frames_sp : one workgroup per output row, as modify_frames_sp, without its LDS: every thread loads its bins of up
//                     to four rows (A's k, k + 1, B's k, k + 1), blends each side as modify_frames does, then
//                     exp((1.0 - rho) * log(a) + rho * log(b)).  rho == 0, rho == 1 and w == 0 are uniform per workgroup
//                     and skip the transcendentals and the loads of the rows they do not need.
//   morph_frames_ap : the same with (1.0 - rho) * a + rho * b.  A kernel of its own: it streams, no transcendental, and runs
//                     at full occupancy whatever morph_frames_sp's registers are.
//   morph_frames_f0 : one thread per output frame.
// Every index read from the path is clamped into its utterance and K into [1, p_stride]: a path that align did not write
// gives positions that mean nothing but stay in bounds, for that pair alone.

struct MorphCell { int i, j; };
__device__ __forceinline__ MorphCell morph_cell(const int *path, int k, int na, int nb) {
  MorphCell c;
  c.i = path[2 * (size_t)k]; c.j = path[2 * (size_t)k + 1];
  c.i = c.i < 0 ? 0 : (c.i > na - 1 ? na - 1 : c.i);
  c.j = c.j < 0 ? 0 : (c.j > nb - 1 ? nb - 1 : c.j);
  return c;
}
__device__ __forceinline__ double morph_time(MorphCell c, double r) {
#pragma clang fp contract(off)
  return (1.0 - r) * c.i + r * c.j;
}
__device__ __forceinline__ double morph_clamp(double s, int n) {
  if (!(s > 0.0)) s = 0.0;
  if (s > n - 1) s = n - 1;
  return s;
}
// the rate of frame `at`: the curve's value (not finite: 0; else clamped to [0, 1]) or the pair's own
__device__ __forceinline__ double morph_rate(const double *curve, size_t at, const double *rate, int u, int which) {
  if (!curve) return rate[4 * (size_t)u + which];
  const double v = curve[at];
  if (!__builtin_isfinite(v)) return 0.0;
  return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

__global__ void morph_positions(MorphParams p) {
#pragma clang fp contract(off)
  const int m = flat_thread_x(), u = blockIdx.y;
  if (m >= p.n_out[u]) return;
  const size_t at = (size_t)u * p.o_stride + m;
  const int na = p.n_a[u], nb = p.n_b[u];
  double sa = m, sb = m;
  if (p.path) {
    const int *path = p.path + 2 * (size_t)u * p.p_stride;
    int K = p.path_len[u];
    K = K < 1 ? 1 : (K > p.p_stride ? p.p_stride : K);
    const double r = p.rate[4 * (size_t)u], x = m;
    int lo = 0;
    for (int n = K; n > 0;) {                         // the first k with t_k >= m
      const int half = n >> 1;
      if (morph_time(morph_cell(path, lo + half, na, nb), r) < x) { lo += half + 1; n -= half + 1; }
      else n = half;
    }
    if (lo > K - 1) lo = K - 1;                       // (never on a path align wrote: its last t is >= n_out - 1)
    const MorphCell cl = morph_cell(path, lo, na, nb);
    const double tl = morph_time(cl, r);
    if (tl == x) {
      int hi = lo + 1;                                // the first k behind lo with t_k > m; the cell before it is the last at m
      for (int n = K - hi; n > 0;) {
        const int half = n >> 1;
        if (!(morph_time(morph_cell(path, hi + half, na, nb), r) > x)) { hi += half + 1; n -= half + 1; }
        else n = half;
      }
      const MorphCell ch = morph_cell(path, hi - 1, na, nb);
      sa = 0.5 * (cl.i + ch.i);
      sb = 0.5 * (cl.j + ch.j);
    } else if (lo == 0) {                             // (never on a path align wrote: t_0 == 0)
      sa = cl.i; sb = cl.j;
    } else {
      const MorphCell cp = morph_cell(path, lo - 1, na, nb);
      const double tp = morph_time(cp, r);
      const double w = (x - tp) / (tl - tp);
      sa = cp.i + w * (cl.i - cp.i);
      sb = cp.j + w * (cl.j - cp.j);
    }
  }
  p.pos_a[at] = morph_clamp(sa, na);
  p.pos_b[at] = morph_clamp(sb, nb);
}

// out = the geometric (GEO) or arithmetic mix of the two sides' rows; BA / BB: that side blends two source rows
template <bool GEO, bool BA, bool BB>
__device__ __forceinline__ void morph_mix_rows(const double *a0, const double *a1, double wa, const double *b0,
                                               const double *b1, double wb, double rho, double *out, int nb, int tid, int nt) {
#pragma clang fp contract(off)
  for (int i = tid; i < nb; i += nt) {
    const double x = BA ? (1.0 - wa) * a0[i] + wa * a1[i] : a0[i];
    const double y = BB ? (1.0 - wb) * b0[i] + wb * b1[i] : b0[i];
    out[i] = GEO ? exp((1.0 - rho) * log(x) + rho * log(y)) : (1.0 - rho) * x + rho * y;
  }
}
// one side alone (rho == 0 or 1): modify_frames' row at that position
__device__ __forceinline__ void morph_one_row(const double *r0, const double *r1, double w, bool blend, double *out, int nb,
                                              int tid, int nt) {
#pragma clang fp contract(off)
  if (blend)
    for (int i = tid; i < nb; i += nt) out[i] = (1.0 - w) * r0[i] + w * r1[i];
  else
    for (int i = tid; i < nb; i += nt) out[i] = r0[i];
}
template <bool GEO>
__device__ __forceinline__ void morph_row(const MorphParams &p, const double *rows_a, const double *rows_b, double *rows_out,
                                          const double *curve, int which) {
  const int m = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int nb = p.fft_size / 2 + 1;
  // m < gridDim.x <= o_stride: the frame's positions and rate lie inside their arrays whether or not the frame exists, so
  // they are fetched beside n_out[u] instead of behind it (as modify_frames_sp does)
  const size_t at = (size_t)u * p.o_stride + m;
  const SourcePosition sa = source_position(p.pos_a, at, m, p.n_a[u]);
  const SourcePosition sb = source_position(p.pos_b, at, m, p.n_b[u]);
  const double rho = morph_rate(curve, at, p.rate, u, which);
  if (m >= p.n_out[u]) return;
  const double *a0 = rows_a + ((size_t)u * p.a_stride + sa.k) * nb, *a1 = rows_a + ((size_t)u * p.a_stride + sa.k1) * nb;
  const double *b0 = rows_b + ((size_t)u * p.b_stride + sb.k) * nb, *b1 = rows_b + ((size_t)u * p.b_stride + sb.k1) * nb;
  double *out = rows_out + at * nb;
  if (rho == 0.0) { morph_one_row(a0, a1, sa.w, sa.blend, out, nb, tid, nt); return; }
  if (rho == 1.0) { morph_one_row(b0, b1, sb.w, sb.blend, out, nb, tid, nt); return; }
  if (sa.blend) {
    if (sb.blend) morph_mix_rows<GEO, true, true>(a0, a1, sa.w, b0, b1, sb.w, rho, out, nb, tid, nt);
    else morph_mix_rows<GEO, true, false>(a0, a1, sa.w, b0, b1, sb.w, rho, out, nb, tid, nt);
  } else {
    if (sb.blend) morph_mix_rows<GEO, false, true>(a0, a1, sa.w, b0, b1, sb.w, rho, out, nb, tid, nt);
    else morph_mix_rows<GEO, false, false>(a0, a1, sa.w, b0, b1, sb.w, rho, out, nb, tid, nt);
  }
}

__global__ void __launch_bounds__(256) morph_frames_sp(MorphParams p) {
  morph_row<true>(p, p.sp_a, p.sp_b, p.sp_out, p.sp_curve, 2);
}
__global__ void __launch_bounds__(256) morph_frames_ap(MorphParams p) {
  morph_row<false>(p, p.ap_a, p.ap_b, p.ap_out, p.ap_curve, 3);
}

// modify_frames' F0 at a source position (its step 3): the frame as it is at a whole position; between two frames the
// blend where both are voiced, the voiced one while its weight is above 0.5, else 0
__device__ __forceinline__ double morph_f0_at(const double *src, const SourcePosition &s) {
#pragma clang fp contract(off)
  double v = src[s.k];
  if (s.blend) {
    const double v1 = src[s.k1], w = s.w;
    const bool a = voiced_f0(v), b = voiced_f0(v1);
    if (a && b) v = (1.0 - w) * v + w * v1;
    else if (a) v = 1.0 - w > 0.5 ? v : 0.0;
    else if (b) v = w > 0.5 ? v1 : 0.0;
    else v = 0.0;
  }
  return v;
}
__global__ void morph_frames_f0(MorphParams p) {
#pragma clang fp contract(off)
  const int m = flat_thread_x(), u = blockIdx.y;
  if (m >= p.n_out[u]) return;
  const size_t at = (size_t)u * p.o_stride + m;
  const double fa = morph_f0_at(p.f0_a + (size_t)u * p.a_stride, source_position(p.pos_a, at, m, p.n_a[u]));
  const double fb = morph_f0_at(p.f0_b + (size_t)u * p.b_stride, source_position(p.pos_b, at, m, p.n_b[u]));
  const double rho = morph_rate(p.f0_curve, at, p.rate, u, 1);
  double v;
  if (rho == 0.0) v = fa;
  else if (rho == 1.0) v = fb;
  else {
    const bool a = voiced_f0(fa), b = voiced_f0(fb);
    if (a && b) v = exp((1.0 - rho) * log(fa) + rho * log(fb));
    else if (a) v = 1.0 - rho > 0.5 ? fa : 0.0;
    else if (b) v = rho > 0.5 ? fb : 0.0;
    else v = 0.0;
  }
  p.f0_out[at] = v;
}

void launch_morph_positions(const MorphParams &p, int max_out, hipStream_t stream) {
  WH_THREADS(morph_positions, max_out, p.n_pairs, 1, stream, p);
}
void launch_morph_frames_sp(const MorphParams &p, int max_out, hipStream_t stream) {
  WH_BLOCKS(morph_frames_sp, dim3(max_out, p.n_pairs), 256, 0, stream, p);
}
void launch_morph_frames_ap(const MorphParams &p, int max_out, hipStream_t stream) {
  WH_BLOCKS(morph_frames_ap, dim3(max_out, p.n_pairs), 256, 0, stream, p);
}
void launch_morph_frames_f0(const MorphParams &p, int max_out, hipStream_t stream) {
  WH_THREADS(morph_frames_f0, max_out, p.n_pairs, 1, stream, p);
}
