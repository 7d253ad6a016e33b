// align.inc -- dynamic time warping of two rows of coded frames (world_hip_align_batch), included by codec.hip inside
// namespace world_hip.  Three launches per group of pairs (DESIGN.md: alignment):
//   align_cost : c(i, j) = sqrt(sum_k (a_k - b_k)^2), k ascending, every operation rounded on its own.  One workgroup per
//                16 x 32 tile of (i, j); the tile's A and B rows sit in LDS at an odd row stride.  Fully parallel, written
//                in the diagonal-major layout of AlignParams so that the serial kernel below never waits for a strided read.
//   align_dp   : D(i, j) = c(i, j) + min over the predecessors that exist; one workgroup per pair walks the n_a + n_b - 1
//                anti-diagonals with ONE barrier each.  Two diagonal buffers in LDS, not three: diagonal d keeps cell i in
//                slot (i - d / 2) mod cap of the buffer of d's parity, which is exactly the slot of cell (i - 1, j - 1) of
//                diagonal d - 2 -- the one value of that diagonal cell i needs -- so every thread overwrites what only it
//                has read, and 2 (min(n_a, n_b) + 1) doubles hold any pair the cell limit admits (131 KB at 8192 x 8192).
//                The coming diagonal's costs are fetched one step ahead into registers.  That does not make a step wait
//                for LDS and the barrier alone: __syncthreads() is a workgroup-scope release, the step's predecessor bytes
//                are stores in flight, and the compiler puts s_waitcnt vmcnt(0) in front of every barrier -- a step waits
//                for its store acknowledgements and for the fetch (0.96 us per step measured on one MI355X, DESIGN.md 3.12).
//   align_path : one lane walks the predecessor codes back from the far corner (every code names a predecessor that
//                exists, so the walk ends at (0, 0) after at most n_a + n_b - 2 steps whatever the costs were), writing
//                the cells over the pair's costs, which nobody reads any more (8 B per step, n_a + n_b - 1 <= n_a n_b); then the
//                workgroup writes the path in ascending order and the two maps from the runs of equal j / equal i.
// Ties: the first of (diagonal, i - 1, j - 1) wins; a later candidate replaces an earlier one only if strictly smaller, so
// a NaN that got in first stays (any monotone path is as good as another then).

constexpr int kAlignTileI = 16, kAlignTileJ = 32;       // align_cost's tile: 512 cells, two per thread
constexpr int kAlignDpThreads = 512, kAlignAhead = 4;   // align_dp: diagonals up to 2048 cells are fetched ahead whole

__device__ __forceinline__ int align_diag_lo(int d, int nb) { return d > nb - 1 ? d - (nb - 1) : 0; }
// cells of the diagonals before d
__device__ __forceinline__ long long align_diag_start(int d, int na, int nb) {
  const int m = na < nb ? na : nb, M = na < nb ? nb : na;
  if (d <= m) return (long long)d * (d + 1) / 2;
  if (d <= M) return (long long)m * (m + 1) / 2 + (long long)(d - m) * m;
  const long long r = (long long)na + nb - 1 - d;
  return (long long)na * nb - r * (r + 1) / 2;
}
__device__ __forceinline__ long long align_cell(int i, int j, int na, int nb) {
  return align_diag_start(i + j, na, nb) + (i - align_diag_lo(i + j, nb));
}

__global__ void __launch_bounds__(256) align_cost(AlignParams p) {
  DYN_LDS(lds);
  const int u = p.first_pair + blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int na = p.n_a[u], nb = p.n_b[u];
  const int tiles_j = (nb + kAlignTileJ - 1) / kAlignTileJ, tiles_i = (na + kAlignTileI - 1) / kAlignTileI;
  if ((int)blockIdx.x >= tiles_i * tiles_j) return;
  const int i0 = (int)blockIdx.x / tiles_j * kAlignTileI, j0 = (int)blockIdx.x % tiles_j * kAlignTileJ;
  const int nd = p.n_dims, ld = nd | 1;               // odd stride: the 16 / 32 rows a wavefront reads fall into different banks
  double *as = reinterpret_cast<double *>(lds), *bs = as + kAlignTileI * ld;
  const double *a = p.a + (size_t)(p.a_row[u] + i0) * p.a_stride, *b = p.b + (size_t)(p.b_row[u] + j0) * p.b_stride;
  for (int e = tid; e < kAlignTileI * nd; e += nt) {
    const int r = e / nd, k = e - r * nd;
    if (i0 + r < na) as[r * ld + k] = a[(size_t)r * p.a_stride + k];
  }
  for (int e = tid; e < kAlignTileJ * nd; e += nt) {
    const int r = e / nd, k = e - r * nd;
    if (j0 + r < nb) bs[r * ld + k] = b[(size_t)r * p.b_stride + k];
  }
  __syncthreads();
  double *cost = p.cost + p.cell0[u];
  for (int c = tid; c < kAlignTileI * kAlignTileJ; c += nt) {
    // 16 consecutive threads: 16 rows i of one anti-diagonal of the tile (or of two, 32 apart) -- consecutive addresses
    const int ti = c & (kAlignTileI - 1), tj = ((c >> 4) - ti) & (kAlignTileJ - 1);
    const int i = i0 + ti, j = j0 + tj;
    if (i >= na || j >= nb) continue;
    const double *x = as + ti * ld, *y = bs + tj * ld;
    double s = 0.0;
    {
#pragma clang fp contract(off)
      for (int k = 0; k < nd; ++k) {
        const double d = x[k] - y[k];
        s = s + d * d;
      }
    }
    cost[align_cell(i, j, na, nb)] = sqrt(s);
  }
}

__global__ void __launch_bounds__(kAlignDpThreads) align_dp(AlignParams p) {
  DYN_LDS(lds);
  const int u = p.first_pair + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int na = p.n_a[u], nb = p.n_b[u], cap = p.cap;
  double *buf = reinterpret_cast<double *>(lds);      // [2][cap]
  const double *cost = p.cost + p.cell0[u];
  unsigned char *code = p.code + p.cell0[u];
  const int n_diag = na + nb - 1;
  double ahead[kAlignAhead];
#pragma unroll
  for (int q = 0; q < kAlignAhead; ++q) ahead[q] = tid + q * nt < 1 ? cost[tid + q * nt] : 0.0;
  long long off = 0;                                  // align_diag_start(d)
  int lo_prev = 0, base = 0, base_prev = 0;           // base = (lo - d / 2) mod cap: the slot of the diagonal's first cell
  for (int d = 0; d < n_diag; ++d) {
    const int lo = align_diag_lo(d, nb), len = (d < na - 1 ? d : na - 1) - lo + 1;
    const int lo_next = align_diag_lo(d + 1, nb);
    const int len_next = d + 1 < n_diag ? (d + 1 < na - 1 ? d + 1 : na - 1) - lo_next + 1 : 0;
    const long long off_next = off + len;
    double next[kAlignAhead];
#pragma unroll
    for (int q = 0; q < kAlignAhead; ++q) next[q] = tid + q * nt < len_next ? cost[off_next + tid + q * nt] : 0.0;
    double *cur = buf + (d & 1) * cap;
    const double *prev = buf + ((d & 1) ^ 1) * cap;
    const int shift = lo - lo_prev;                   // cell i of this diagonal is element i - lo + shift of the previous one
    auto cell = [&](int t, double c) {
      const int i = lo + t, j = d - i;
      int s = base + t;
      if (s >= cap) s -= cap;
      double best = 0.0;
      int from = 3;
      if (i > 0 && j > 0) { best = cur[s]; from = 0; }                    // (i - 1, j - 1): this cell's own slot
      if (i > 0) {
        int q = base_prev + t + shift - 1;
        if (q >= cap) q -= cap;
        const double v = prev[q];
        if (from == 3 || v < best) { best = v; from = 1; }
      }
      if (j > 0) {
        int q = base_prev + t + shift;
        if (q >= cap) q -= cap;
        const double v = prev[q];
        if (from == 3 || v < best) { best = v; from = 2; }
      }
      const double total = from == 3 ? c : c + best;
      cur[s] = total;
      code[off + t] = (unsigned char)from;
      if (d == n_diag - 1) p.dist[u] = total;
    };
#pragma unroll
    for (int q = 0; q < kAlignAhead; ++q)
      if (tid + q * nt < len) cell(tid + q * nt, ahead[q]);
    for (int t = tid + kAlignAhead * nt; t < len; t += nt) cell(t, cost[off + t]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kAlignAhead; ++q) ahead[q] = next[q];
    base_prev = base;
    base += (lo_next - lo) - (((d + 1) >> 1) - (d >> 1));
    if (base < 0) base += cap;
    if (base >= cap) base -= cap;
    lo_prev = lo;
    off = off_next;
  }
}

__global__ void __launch_bounds__(256) align_path(AlignParams p) {
  DYN_LDS(lds);
  int *steps = reinterpret_cast<int *>(lds);          // [1]
  const int u = p.first_pair + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int na = p.n_a[u], nb = p.n_b[u];
  const unsigned char *code = p.code + p.cell0[u];
  int *walk = reinterpret_cast<int *>(p.cost + p.cell0[u]);   // the costs are dead behind align_dp; 8 B per step <= 8 B per cell
  if (tid == 0) {
    int i = na - 1, j = nb - 1, k = 0;
    for (;;) {
      walk[2 * k] = i; walk[2 * k + 1] = j;
      ++k;
      if (i == 0 && j == 0) break;
      int from = code[align_cell(i, j, na, nb)];
      if (i == 0) from = 2;                           // (what align_dp wrote there anyway: the walk cannot leave the matrix)
      else if (j == 0) from = 1;
      else if (from > 2) from = 0;
      if (from != 2) --i;
      if (from != 1) --j;
    }
    steps[0] = k;
  }
  __syncthreads();
  const int K = steps[0];
  if (tid == 0) {
    if (p.path_len) p.path_len[u] = K;
    if (p.summary) {
      const double D = p.dist[u];
      double *s = p.summary + 3 * (size_t)u;
      s[0] = D; s[1] = K; s[2] = p.mcd_scale * D / K;
    }
  }
  // path entry q is walk entry K - 1 - q
  for (int q = tid; q < K; q += nt) {
    const int *w = walk + 2 * (size_t)(K - 1 - q);
    const int i = w[0], j = w[1];
    if (p.path) {
      int *out = p.path + 2 * ((size_t)u * p.p_stride + q);
      out[0] = i; out[1] = j;
    }
    // the first cell of a column (row) of the path counts the cells that stay in it: they follow it, one row (column) up each
    if (p.map_b && (q == 0 || w[3] != j)) {
      int run = 0;
      while (q + run + 1 < K && w[-2 * (run + 1) + 1] == j) ++run;
      p.map_b[(size_t)u * p.map_stride + j] = 0.5 * (i + (i + run));
    }
    if (p.map_a && (q == 0 || w[2] != i)) {
      int run = 0;
      while (q + run + 1 < K && w[-2 * (run + 1)] == i) ++run;
      p.map_a[(size_t)u * p.map_stride + i] = 0.5 * (j + (j + run));
    }
  }
}

size_t align_cost_lds_bytes(int n_dims) { return sizeof(double) * (kAlignTileI + kAlignTileJ) * (size_t)(n_dims | 1); }
int align_cost_tiles(int n_a, int n_b) {
  return ((n_a + kAlignTileI - 1) / kAlignTileI) * ((n_b + kAlignTileJ - 1) / kAlignTileJ);
}
void launch_align_cost(const AlignParams &p, int pairs, int max_tiles, hipStream_t stream) {
  WH_BLOCKS(align_cost, dim3(max_tiles, pairs), 256, align_cost_lds_bytes(p.n_dims), stream, p);
}
void launch_align_dp(const AlignParams &p, int pairs, hipStream_t stream) {
  WH_BLOCKS(align_dp, dim3(pairs), kAlignDpThreads, 2 * sizeof(double) * (size_t)p.cap, stream, p);
}
void launch_align_path(const AlignParams &p, int pairs, hipStream_t stream) {
  WH_BLOCKS(align_path, dim3(pairs), 256, 16, stream, p);
}
