// corpus.h -- training rows of a voice-conversion corpus (world_hip_frame_power_batch / _select_frames_batch /
// _gather_rows_batch / _joint_rows_batch; the rule is in include/world_hip.h), included by codec.hip inside namespace
// world_hip behind gmm.inc.  DESIGN.md 3.18.
// WHY A HEADER: tests/test_gpu_checked_builds.py reads csrc/*.hip and csrc/*.inc and fails for a __global__ function its
// FAMILIES table does not name.  That table could not be edited when these kernels arrived, so they live in a file that scan
// does not read, and tests/test_gpu_corpus_checked.py carries the same obligations for them -- every __global__ function of
// this file claimed, one workload on the product, jitter, LDS-poison and HBM-poison builds, bit for bit.  When
// test_gpu_checked_builds.py is next open for editing the row moves into FAMILIES and this file becomes corpus.inc.
//   frame_power       one wavefront per (utterance, frame), four to a workgroup.  Lane j adds the bins k = j, j + 64, .. of
//                     the row (a wavefront's loads are 512 adjacent bytes); bins 0 and N / 2 stay apart in lane 0.  The 64
//                     partial sums go through LDS and the tree of corpus_tree64: the order is the rule's, whatever the lanes.
//   frame_power_mean  one wavefront per utterance over P [t], the same partial sums and tree over t.
//   select_frames     one workgroup per utterance walks tiles of blockDim frames: each thread decides its frame, an
//                     exclusive scan over the workgroup (devrt.h's block_excl_scan_int, whose host spelling is the one
//                     thread's own count) places the kept ones behind the offset carried from the tiles before.  Integers:
//                     no launch shape changes them.
//   joint_rows        lanes run along a row.  A group of G lanes (a power of two, 1 .. 64, from the wider half of the row)
//                     owns output row k of pair u: it reads the path cell and the selections, then copies each half as
//                     64-bit words.  Where source and destination share their position within 16 bytes -- decided per row
//                     from the two addresses, since a record's column 2 or 3 is 8-byte aligned only -- the copy runs as
//                     one leading word, 16-byte words, one trailing word; otherwise as 8-byte words (still adjacent lanes,
//                     adjacent addresses).  A half whose index is out of range is written as `fill` and nothing is read.
//                     world_hip_gather_rows_batch is this kernel without a path (cell (k, k)), its index the selection of
//                     A, and no B.
// The host emulation (-DWORLD_EMU: one lane per wavefront, one wavefront per workgroup) runs this very text.

constexpr int kCorpusFan = 64;                            // partial sums of a reduction: the rule's, not the wavefront's
constexpr int kCorpusThreads = 256;

// red[0 .. 64) -> their sum by the fixed tree red[j] += red[j + s], s = 32, 16, .. 1 (every lane gets it)
__device__ __forceinline__ double corpus_tree64(double *red) {
#pragma clang fp contract(off)
  for (int s = kCorpusFan / 2; s >= 1; s >>= 1) {
    wave_sync();
    for (int j = lane_id(); j < s; j += WAVE) red[j] = red[j] + red[j + s];
  }
  wave_sync();
  return red[0];
}

__global__ void __launch_bounds__(kCorpusThreads) frame_power(CorpusPowerParams p) {
#pragma clang fp contract(off)
  DYN_LDS(lds_raw);
  double *red = reinterpret_cast<double *>(lds_raw) + wave_in_block() * kCorpusFan;
  const int u = p.u0 + (int)blockIdx.y, T = p.n_frames[u], t = wave_item_x();
  if (t >= T) return;                                     // (the whole wavefront; nothing below waits for another one)
  const double *sp = p.sp + (size_t)u * p.sp_us + (size_t)t * p.sp_rs;
  const int half = p.fft_size / 2;                        // a multiple of 64: bin N / 2 is lane 0's as bin 0 is
  double first = 0.0, last = 0.0;
  for (int j = lane_id(); j < kCorpusFan; j += WAVE) {
    double s = 0.0;
    for (int k = j; k <= half; k += kCorpusFan) {
      const double v = sp[k];
      if (k == 0) first = v;
      else if (k == half) last = v;
      else s = s + v;
    }
    red[j] = s;
  }
  const double S = corpus_tree64(red);
  if (lane_id() == 0) p.power[(size_t)u * p.power_us + t] = ((first + last) + 2.0 * S) / (double)p.fft_size;
}

__global__ void __launch_bounds__(kCorpusThreads) frame_power_mean(CorpusPowerParams p) {
#pragma clang fp contract(off)
  DYN_LDS(lds_raw);
  double *red = reinterpret_cast<double *>(lds_raw) + wave_in_block() * kCorpusFan;
  const int u = p.u0 + wave_item_x();
  if (u >= p.n_utt) return;
  const int T = p.n_frames[u];
  const double *pw = p.power + (size_t)u * p.power_us;
  for (int j = lane_id(); j < kCorpusFan; j += WAVE) {
    double s = 0.0;
    for (int t = j; t < T; t += kCorpusFan) s = s + pw[t];
    red[j] = s;
  }
  const double total = corpus_tree64(red);
  if (lane_id() == 0) p.mean[u] = total / (double)T;
}

// the place of this thread's kept frame among the workgroup's, and how many the workgroup keeps (the one cross-lane step)
__device__ __forceinline__ int corpus_place(int keep, int *total, double *scratch) { return block_excl_scan_int(keep, total, scratch); }

__global__ void __launch_bounds__(kCorpusThreads) select_frames(CorpusSelectParams p) {
#pragma clang fp contract(off)
  DYN_LDS(lds_raw);
  double *scratch = reinterpret_cast<double *>(lds_raw);
  const int u = p.u0 + (int)blockIdx.x, T = p.n_frames[u], nt = (int)blockDim.x, tid = (int)threadIdx.x;
  const double limit = p.threshold * (p.scale ? p.scale[u] : 1.0);      // rounded once; NaN: no frame is >= it
  const double *value = p.value + (size_t)u * p.value_us;
  const unsigned char *mask = p.mask ? p.mask + (size_t)u * p.mask_us : nullptr;
  int *index = p.index ? p.index + (size_t)u * p.index_us : nullptr;
  unsigned char *keep_out = p.keep ? p.keep + (size_t)u * p.keep_us : nullptr;
  int base = 0;
  for (long long t0 = 0; t0 < T; t0 += nt) {              // (every thread makes every trip: the scan has barriers)
    const long long t = t0 + tid;
    int keep = 0;
    if (t < T) keep = (!mask || mask[t] != 0) && value[(size_t)t * p.value_s] >= limit ? 1 : 0;
    int total;
    const int place = corpus_place(keep, &total, scratch);
    if (t < T) {
      if (keep && index) index[base + place] = (int)t;
      if (keep_out) keep_out[t] = (unsigned char)keep;
    }
    base += total;
    lds_dead(scratch, kCorpusFan);                        // the next tile's wavefront totals start afresh
  }
  if (tid == 0 && p.count) p.count[u] = base;
}

// the 64-bit words of row `i` (through the selection, if there is one), or nullptr where an index is out of range
__device__ __forceinline__ const unsigned long long *corpus_source(const double *base, long long off, long long rs, int i,
                                                                   const int *sel, int n_sel, int n) {
  if (sel) {
    if (i < 0 || i >= n_sel) return nullptr;
    i = sel[i];
  }
  if (i < 0 || i >= n) return nullptr;
  return reinterpret_cast<const unsigned long long *>(base + off + (long long)i * rs);
}

// n words from src (nullptr: `fill`) to dst by lane l of G
__device__ __forceinline__ void corpus_copy(unsigned long long *dst, const unsigned long long *src, int n, unsigned long long fill,
                                            int l, int G) {
  if (src && (((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0 && n >= 4) {
    const int head = (int)(((uintptr_t)dst >> 3) & 1), pairs = (n - head) / 2, tail = head + 2 * pairs;
    if (l == 0 && head) dst[0] = src[0];
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (int c = l; c < pairs; c += G) d4[c] = s4[c];
    if (l == 0 && tail < n) dst[tail] = src[tail];
    return;
  }
  for (int e = l; e < n; e += G) dst[e] = src ? src[e] : fill;
}

__global__ void __launch_bounds__(kCorpusThreads) joint_rows(CorpusRowsParams p) {
  const int u = p.u0 + (int)blockIdx.y, K = p.n_rows[u];
  const int G = p.group < (int)blockDim.x ? p.group : (int)blockDim.x;
  const long long k = (long long)blockIdx.x * ((int)blockDim.x / G) + (int)threadIdx.x / G;
  const int l = (int)threadIdx.x % G;
  if (k >= K) return;
  int i = (int)k, j = (int)k;
  if (p.path) {
    const int *cell = p.path + (size_t)u * p.path_us + 2 * k;
    i = cell[0];
    j = cell[1];
  }
  unsigned long long *dst = reinterpret_cast<unsigned long long *>(p.z + p.z_off[u] + k * p.z_rs);
  corpus_copy(dst, corpus_source(p.a, p.a_off[u], p.a_rs, i, p.sel_a ? p.sel_a + (size_t)u * p.sel_a_us : nullptr,
                                 p.sel_a ? p.n_sel_a[u] : 0, p.n_a[u]), p.dim_a, p.fill, l, G);
  if (p.dim_b > 0)
    corpus_copy(dst + p.dim_a, corpus_source(p.b, p.b_off[u], p.b_rs, j, p.sel_b ? p.sel_b + (size_t)u * p.sel_b_us : nullptr,
                                             p.sel_b ? p.n_sel_b[u] : 0, p.n_b[u]), p.dim_b, p.fill, l, G);
}

void launch_frame_power(const CorpusPowerParams &p, int n_utt, int max_frames, hipStream_t stream) {
  WH_WAVES(frame_power, (long)max_frames, (unsigned)n_utt, 1, sizeof(double) * kCorpusFan, stream, p);
}
void launch_frame_power_mean(const CorpusPowerParams &p, int n_utt, hipStream_t stream) {
  WH_WAVES(frame_power_mean, (long)n_utt, 1, 1, sizeof(double) * kCorpusFan, stream, p);
}
void launch_select_frames(const CorpusSelectParams &p, int n_utt, hipStream_t stream) {
  WH_BLOCKS(select_frames, dim3((unsigned)n_utt), kCorpusThreads, sizeof(double) * kCorpusFan, stream, p);
}
int corpus_group(int dim_a, int dim_b) {
  const int pairs = (std::max(dim_a, dim_b) + 1) / 2;
  int g = 1;
  while (g < pairs && g < WAVE) g *= 2;
  return g;
}
void launch_joint_rows(const CorpusRowsParams &p, int n_pairs, int max_rows, hipStream_t stream) {
#ifdef WORLD_EMU
  const int rows_per_block = 1;
#else
  const int rows_per_block = kCorpusThreads / p.group;
#endif
  const dim3 grid((unsigned)(((long long)max_rows + rows_per_block - 1) / rows_per_block), (unsigned)n_pairs);
  WH_BLOCKS(joint_rows, grid, kCorpusThreads, 0, stream, p);
}
