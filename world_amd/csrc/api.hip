// api.hip -- host planner + the C ABI of libworld_hip.so (include/world_hip.h).
//
// The planner mirrors the scalar set-up code at the top of the reference's entry
// points (Harvest()/HarvestGeneralBody src/harvest.cpp:1145-1165,1223-1244,
// CheapTrick() src/cheaptrick.cpp:191-214, D4C() src/d4c.cpp:350-379), carves a
// per-call workspace out of one grow-only HBM arena and enqueues the stage
// kernels on the context's stream.  Nothing here waits for the GPU except the
// drop-in host-pointer entry points, which must hand results back in caller memory.
#include "../../include/world_hip.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstdarg>
#include <deque>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"
#include "bandfilter.h"
#include "codec.h"
#include "decimate.h"
#include "dio.h"
#include "exchange.h"
#include "fft_probe.h"
#include "d4c_select_probe.h"
#include "gmm_host.h"
#include "machine_probe.h"
#include "mcep_host.h"
#include "resample.h"
#include "harvest.h"
#include "stage_params.h"
#include "synthesis.h"

namespace world_hip {

static thread_local std::string g_last_error;

[[noreturn]] static void fail(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw std::runtime_error(buf);
}

// ---------------------------------------------------------------------------
// A stage's workspace is written down once, as a carve: the function that takes its arrays from an Arena in order.  Run
// against a counting arena (no base, no limit) the carve measures the workspace; the context's arena is grown to that
// and the same carve then runs for real.
struct Arena {
  char *base = nullptr;
  size_t cap = 0, used = 0;
  // bytes at the bottom that outlive the stages of one call (world_hip_resynthesize_batch keeps its analysis there): the
  // stages carve above them.  0 outside such a call.
  size_t floor = 0;
  void reset() { used = floor; }
  template <class T> T *take(size_t count) {
    size_t bytes = (count * sizeof(T) + 255) & ~size_t(255);
    if (used + bytes > cap) fail("workspace arena overflow (%zu + %zu > %zu)", used, bytes, cap);
    T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
    used += bytes;
    return p;
  }
};
template <class Carve> static size_t measure(Carve carve) {
  Arena count;
  count.cap = SIZE_MAX;
  carve(count);
  return count.used;
}

struct HarvestBands {            // cached per (fs, f0_floor, f0_ceil)
  int fs = 0;
  double f0_floor = 0, f0_ceil = 0;
  int nch = 0, max_half = 0;
  double *d_band_f0 = nullptr, *d_taps = nullptr;
  int *d_half = nullptr, *d_off = nullptr;
  double *d_win_tab = nullptr;   // refinement-window angle steps per half length (hv_refine)
  int win_tab_len = 0;
  size_t win_full_entries = 0;   // (w, dw) pairs of every whole-sample-centred window behind the two tables above (0: none)
  double win_afs = 0, win_floor = 0;   // the (analysis rate, f0_floor) those three were built for (prepare_refine_windows)
  double2 *d_spec = nullptr;     // [nch][kBandFftBins] spectra of the taps / kBandFft (FFT path of the filter bank)
  int fft_seg = 0;               // outputs per block of that path (0: filters too long, direct FIR)
  std::vector<double> band_f0;
};

struct DioBands {                // cached per (fs, f0_floor, f0_ceil, channels, ratio)
  int fs = 0, ratio = 0;
  double f0_floor = 0, f0_ceil = 0, cpo = 0;
  int nb = 0, cut = 0, max_ntap = 0;
  double band_f0_first = 0;      // boundary_f0_list[0]
  double *d_band_f0 = nullptr, *d_taps = nullptr, *d_lowcut = nullptr;
  int *d_hal = nullptr, *d_off = nullptr;
};

struct CodecTables {             // the coders' tables of one (fs, fft_size) (reference src/codec.cpp)
  int fs = 0, fft_size = 0;
  int *d_knot_code = nullptr, *d_knot_dec = nullptr, *d_knot_ap = nullptr;
  double *d_frac_code = nullptr, *d_frac_dec = nullptr, *d_frac_ap = nullptr;
  double *d_wc_re = nullptr, *d_wc_im = nullptr, *d_wd_re = nullptr, *d_wd_im = nullptr;
};

// The two kinds of entry of cached_table (below): a few of each are kept, least recently used out.  `used` is the
// context's table_clock at the call that last used the entry, Host the host arrays put() uploads.
struct ResampleTable {           // the resampler's device tables of one (L, M, design)
  long long L = 0, M = 0, W = 0;
  ResampleDesign design{0, 0.0, 0.0};
  double *d_coef = nullptr;      // [2 W][L], column r = m mod L (resample.h)
  int *d_kdiv = nullptr;         // [L]
  unsigned long long used = 0;
  struct Host { std::vector<double> coef; std::vector<int> kdiv; };
  void put(WorldHipContext *c, const Host &h);
  void drop(WorldHipContext *c);
  unsigned long long bytes() const { return (2ull * W * sizeof(double) + sizeof(int)) * L; }
};

struct McepTable {               // one direction's device table of one (fft_size, order, alpha)
  int fft_size = 0, order = 0;
  unsigned long long alpha_bits = 0;
  bool decode = false;
  int k_pad = 0, n_pad = 0;
  double *d_table = nullptr;     // [k_pad][n_pad], zero beyond the table (codec.h: McepParams)
  unsigned long long used = 0;
  using Host = std::vector<double>;
  void put(WorldHipContext *c, const Host &h);
  void drop(WorldHipContext *c);
  unsigned long long bytes() const { return sizeof(double) * (unsigned long long)k_pad * n_pad; }
};

}  // namespace world_hip

// The small per-call host arrays (lengths, frame counts, row offsets: a few ints per utterance) depend only on the
// call's shape, and a service sees the same shapes again and again: every distinct array is uploaded ONCE into a
// persistent slab and found again by content.  A call in steady state therefore does no host-to-device copy, touches no
// staging buffer and waits for no event -- which is also what makes the batched calls capturable into a HIP graph
// (round 2 staged them through a ring of pinned buffers guarded by events; hipErrorStreamCaptureInvalidated).
// Slabs are CHAINED, never replaced under a call: a stage uploads several arrays before it launches, and a pointer it
// already holds must stay valid whatever the later uploads do (a full 4 MB slab used to be freed and
// reallocated between two uploads of one call).  The whole set is dropped only at the START of a stage (open_uploads), with
// the stream drained, once it holds more than kSmallBudget bytes -- a service fed ever-new length vectors then pays one
// synchronisation per ~16 k distinct arrays instead of growing without bound.  Lookup is a hash of the content.
struct SmallArrays {
  struct Entry { std::vector<char> bytes; char *dev; };
  struct Slab { char *base; size_t cap, used; };
  std::vector<Slab> slabs;
  std::unordered_multimap<uint64_t, Entry> entries;
  size_t held = 0;               // bytes of all slabs
  static uint64_t hash(const void *data, size_t bytes) {          // FNV-1a over the content and its length
    uint64_t h = 1469598103934665603ull ^ bytes;
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
  }
};
static size_t small_slab() {                                      // WORLD_HIP_SMALL_SLAB: test hook (bytes per chained slab)
  static const size_t v = [] { const char *e = getenv("WORLD_HIP_SMALL_SLAB"); return e ? std::max<size_t>(256, (size_t)atoll(e)) : (size_t(4) << 20); }();
  return v;
}
static size_t small_budget() {                                    // WORLD_HIP_SMALL_BUDGET: test hook (bytes)
  static const size_t v = [] { const char *e = getenv("WORLD_HIP_SMALL_BUDGET"); return e ? (size_t)atoll(e) : (size_t(64) << 20); }();
  return v;
}

struct WorldHipContext {
  int device = 0;
  hipStream_t stream = nullptr;
  world_hip::Tables tab{nullptr, nullptr};
  world_hip::Arena arena;
  world_hip::HarvestBands bands;
  double *d_nuttall = nullptr;   // D4C band window
  int nuttall_len = 0;
  double *d_ap_frac = nullptr;   // d4c_finish's per-bin interpolation weight and knot (D4cParams::ap_frac / ap_knot), for
  int *d_ap_knot = nullptr;      //   (ap_grid_fs, ap_grid_fft)
  int ap_grid_fs = 0, ap_grid_fft = 0;
  world_hip::DioBands dio_bands;
  double *d_dc_remover = nullptr; // GetDCRemover(fft_size) of the synthesiser
  int dc_remover_len = 0;
  int *d_synth_need = nullptr;   // largest pulse count a synthesis call could not hold (0 = nothing was dropped)
  int synth_pulse_cap = 0;       // caller's capacity per utterance (0 = automatic)
  std::vector<world_hip::CodecTables> codec_tables;
  std::vector<world_hip::ResampleTable> resample_tables;
  std::vector<world_hip::McepTable> mcep_tables;
  unsigned long long table_clock = 0;   // look-ups of the two caches above (cached_table)
  // the device arrays of tab and of the cached tables (bands, d_nuttall .. codec_tables, d_pk): allocated and freed by
  // put_table / drop_table only, released together when the context goes
  std::vector<void *> tables;
  SmallArrays small;             // the per-call host arrays, uploaded once per distinct content
  void *xchg_ready = nullptr, *xchg_done = nullptr;   // events of world_hip_allgather_blocks
  double *d_pk = nullptr;        // dense (tpos, f0) of world_hip_analyze_packed: [2][n_utt][f_stride], grow-only
  size_t pk_cap = 0;
  int hint = 0;                  // WORLD_HIP_HINT_* bits (world_hip_set_hint)
  // world_hip_analyze_sharded: this device's exchange stream, input staging (two pinned halves) and device input, grow-only
  hipStream_t xstream = nullptr;
  double *h_xin = nullptr, *d_xin = nullptr;
  size_t xin_cap = 0;            // doubles per half
  // Bumped whenever memory a captured graph may have baked in is freed or replaced (arena, small-array slabs, d_pk, the
  // cached filter / window / codec tables): world_hip_graph_launch refuses a graph of an older generation.
  unsigned long long generation = 0;
  // What the offset scans (and D4C's LoveTrain pass) still lying in the workspace were computed FOR: a later call may
  // ask to reuse them (`reuse_offsets`, the frame-range entries) and gets them only if its own inputs say the same thing
  // and nothing has touched that part of the arena since (the flag used to be trusted blindly).
  struct PrepToken {
    bool valid = false;
    int n_utt = 0, fs = 0, f_stride = 0, x_stride = 0, fft = 0;
    const void *x = nullptr, *f0 = nullptr, *tpos = nullptr, *arena_base = nullptr;
    double opt = 0.0;              // CheapTrick: its F0 floor; D4C: the threshold
    uint64_t lengths_hash = 0;     // x_length and n_frames
    size_t lo = 0, hi = 0;         // the arena bytes the prepared arrays occupy
    unsigned long long generation = 0;
    bool same_inputs(const PrepToken &o) const {
      return n_utt == o.n_utt && fs == o.fs && f_stride == o.f_stride && x_stride == o.x_stride && fft == o.fft && x == o.x &&
             f0 == o.f0 && tpos == o.tpos && arena_base == o.arena_base && opt == o.opt && lengths_hash == o.lengths_hash &&
             lo == o.lo && hi == o.hi && generation == o.generation;
    }
  };
  PrepToken prep_ct, prep_d4c;
  std::mutex lock;               // one call at a time per context
};

namespace world_hip {

// Thrown by ensure_arena while a floor is held: the arena cannot move under the arrays kept there, so the call that holds
// the floor grows it to `bytes` (floor included) with the floor released and starts over.  Invariant: a floor is set only
// by hold_at_floor, whose attempt loop catches this.  It is not a std::exception, so that
// no stage's own error handling can swallow it; should it ever escape a call, guarded() turns it into an internal error
// instead of letting it cross the C boundary.
struct ArenaRegrow { size_t bytes; };

static void ensure_arena(WorldHipContext *c, size_t bytes) {
  if (c->arena.floor + bytes <= c->arena.cap) return;
  if (c->arena.floor) throw ArenaRegrow{c->arena.floor + bytes};
  devrt::sync(c->stream);
  if (c->arena.base) { devrt::dfree(c->arena.base); ++c->generation; }
  size_t cap = bytes + bytes / 8 + (1u << 20);
  c->arena.base = static_cast<char *>(devrt::dmalloc(cap));
  c->arena.cap = cap;
}

// A cached device table of the context.  Freeing one frees memory a captured graph may point into: the generation moves.
// The callers drain the stream around a group of replacements (a kernel may still read the old copy).
template <class T> static void drop_table(WorldHipContext *c, T *&slot) {
  if (!slot) return;
  c->tables.erase(std::find(c->tables.begin(), c->tables.end(), static_cast<void *>(slot)));
  devrt::dfree(slot);
  slot = nullptr;
  ++c->generation;
}
// `slot` := a fresh device array of n T, filled from `host` on the stream unless that is null
template <class T> static void put_table(WorldHipContext *c, T *&slot, size_t n, const T *host = nullptr) {
  drop_table(c, slot);
  slot = static_cast<T *>(devrt::dmalloc(sizeof(T) * std::max<size_t>(n, 1)));
  c->tables.push_back(slot);
  if (host && n) devrt::h2d(slot, host, sizeof(T) * n, c->stream);
}
template <class T> static void put_table(WorldHipContext *c, T *&slot, const std::vector<T> &host) {
  put_table(c, slot, host.size(), host.data());
}

// A small keyed cache of device tables, at most `keep` of them, least recently used out (resample_table, mcep_table).
// `same` is the kind's key comparison and `refusal` its words for a miss under capture; on a miss `build` fills the new
// entry's key and shape and returns the host arrays that the entry's put() uploads.
template <class Table, class Same, class Build>
static const Table &cached_table(WorldHipContext *c, std::vector<Table> &kept, size_t keep, const char *refusal, Same same,
                                 Build build) {
  ++c->table_clock;
  for (Table &t : kept)
    if (same(t)) {
      t.used = c->table_clock;
      return t;
    }
  // a miss allocates and uploads: neither is possible while the stream is being captured into a graph
  if (devrt::is_capturing(c->stream)) fail("%s", refusal);
  Table t;
  const typename Table::Host host = build(t);
  devrt::sync(c->stream);                        // (a kernel may still read the table that goes)
  if (kept.size() >= keep) {
    auto oldest = std::min_element(kept.begin(), kept.end(), [](const Table &a, const Table &b) { return a.used < b.used; });
    oldest->drop(c);
    kept.erase(oldest);
  }
  t.used = c->table_clock;
  t.put(c, host);
  devrt::sync(c->stream);                        // (the host copies go out of scope)
  kept.push_back(t);
  return kept.back();
}

// The randn() stream is a constant of the algorithm: its first `draws` values live in the device's
// shared, fully verified table (rng.h / rng_fill.hip), generated once per process and extended on demand.
static const uint32_t *ensure_noise(WorldHipContext *c, size_t draws) {
  return noise_table_acquire(c->device, draws, c->tab.jump, c->stream);
}

// A small host array on the device: found by content in the context's slabs, or appended to them (one H2D copy from a
// host copy that lives as long as the entry).  Nothing a call already holds a pointer to is ever freed by an upload.
static void drop_small_arrays(WorldHipContext *c) {
  SmallArrays &sa = c->small;
  for (SmallArrays::Slab &sl : sa.slabs) devrt::dfree(sl.base);
  sa.slabs.clear();
  sa.entries.clear();
  sa.held = 0;
}
// The start of a stage's upload section: the ONLY place the small arrays may be dropped -- no params struct of this
// stage holds a pointer yet, and the kernels of earlier stages are waited for first.
static void open_uploads(WorldHipContext *c) {
  if (c->small.held > small_budget() && !devrt::is_capturing(c->stream)) {
    devrt::sync(c->stream);
    drop_small_arrays(c);
    ++c->generation;
  }
}

static char *small_array(WorldHipContext *c, const void *data, size_t bytes) {
  SmallArrays &sa = c->small;
  const uint64_t h = SmallArrays::hash(data, bytes);
  auto range = sa.entries.equal_range(h);
  for (auto it = range.first; it != range.second; ++it)
    if (it->second.bytes.size() == bytes && memcmp(it->second.bytes.data(), data, bytes) == 0) return it->second.dev;
  // a miss uploads (and may allocate): neither is possible while the stream is being captured into a graph
  if (devrt::is_capturing(c->stream)) fail("a call shape that was never run before cannot be captured: run it once first");
  const size_t padded = (bytes + 255) & ~size_t(255);
  if (sa.slabs.empty() || sa.slabs.back().used + padded > sa.slabs.back().cap) {
    SmallArrays::Slab sl;                                          // chain a fresh slab; the old ones stay valid
    sl.cap = std::max(small_slab(), padded);
    sl.base = static_cast<char *>(devrt::dmalloc(sl.cap));
    sl.used = 0;
    sa.slabs.push_back(sl);
    sa.held += sl.cap;
  }
  SmallArrays::Slab &sl = sa.slabs.back();
  SmallArrays::Entry e;
  e.bytes.assign(static_cast<const char *>(data), static_cast<const char *>(data) + bytes);
  e.dev = sl.base + sl.used;
  sl.used += padded;
  auto kept = sa.entries.emplace(h, std::move(e));
  devrt::h2d(kept->second.dev, kept->second.bytes.data(), bytes, c->stream);   // the source outlives the copy (node-based map)
  return kept->second.dev;
}

template <class T> static T *upload(WorldHipContext *c, const T *host, size_t n) {
  if (n == 0) return reinterpret_cast<T *>(small_array(c, "", 1));
  return reinterpret_cast<T *>(small_array(c, host, sizeof(T) * n));
}
template <class T> static T *upload(WorldHipContext *c, const std::vector<T> &v) { return upload(c, v.data(), v.size()); }

// An output may not overlap an input or another output: the byte ranges of what a call touches.  Null pointers are skipped.
struct Span { const void *p; size_t bytes; const char *name; };
static void refuse_overlap(const char *call, std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
  auto meet = [](const Span &a, const Span &b) {
    const char *a_lo = static_cast<const char *>(a.p), *b_lo = static_cast<const char *>(b.p);
    return a.p && b.p && a_lo < b_lo + b.bytes && b_lo < a_lo + a.bytes;
  };
  for (const Span *o = outs.begin(); o != outs.end(); ++o) {
    for (const Span &i : ins)
      if (meet(*o, i)) fail("%s: %s overlaps %s; no output may alias an input", call, o->name, i.name);
    for (const Span *o2 = o + 1; o2 != outs.end(); ++o2)
      if (meet(*o, *o2)) fail("%s: %s overlaps %s", call, o->name, o2->name);
  }
}

static int ilog2_exact(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  if ((1 << l) != n) fail("fft size %d is not a power of two", n);
  return l;
}
constexpr int kGridY = 65535;                                         // a grid's y extent: a launch takes that many utterances or pairs

static int frame_count(int fs, int x_length, double frame_period) {   // harvest.cpp:1219, dio.cpp:639
  return static_cast<int>(1000.0 * x_length / fs / frame_period) + 1;
}

static void check_batch(int n_utt, int fs, const void *d_x, int x_stride, const int *x_length) {
  if (n_utt <= 0) fail("n_utt must be positive");
  if (fs <= 0) fail("fs must be positive");
  if (!d_x || !x_length) fail("null input");
  for (int u = 0; u < n_utt; ++u)
    if (x_length[u] <= 0 || x_length[u] > x_stride) fail("x_length[%d]=%d outside (0, x_stride=%d]", u, x_length[u], x_stride);
}
// the largest of n_frames[0 .. n_utt), every one checked against [0, f_stride]
static int max_frame_count(const int *n_frames, int n_utt, int f_stride) {
  int max_frames = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (n_frames[u] < 0 || n_frames[u] > f_stride) fail("n_frames[%d] outside [0, f_stride]", u);
    max_frames = std::max(max_frames, n_frames[u]);
  }
  return max_frames;
}
// the first record of every utterance: utterance u's n_frames[u] records follow those of u - 1, from first_row on
static std::vector<int> record_rows(const int *n_frames, int n_utt, long long first_row) {
  std::vector<int> rows(n_utt);
  long long row = first_row;
  for (int u = 0; u < n_utt; ++u) {
    if (row + n_frames[u] > 0x7FFFFFFFll) fail("block exceeds 2^31 records");
    rows[u] = static_cast<int>(row);
    row += n_frames[u];
  }
  return rows;
}
static BatchView batch_view(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                            const int *n_frames, int f_stride) {
  BatchView b;
  b.n_utt = n_utt; b.fs = fs; b.x_stride = x_stride; b.f_stride = f_stride; b.x = d_x;
  b.x_len = upload(c, std::vector<int>(x_length, x_length + n_utt));
  b.n_frames = upload(c, std::vector<int>(n_frames, n_frames + n_utt));
  return b;
}

// Where a per-frame stage writes its rows: the dense [n_utt][f_stride][bins] array of the batched API (rows == nullptr),
// or rows of packed records -- frame f of utterance u at row rows[u] + f, `stride` doubles apart (exchange.hip's layout,
// written by the stage kernels themselves instead of a pack pass over 2 x 16 KB per frame).
struct RowLayout {
  const int *rows = nullptr;     // host, [n_utt]
  size_t stride = 0;             // 0: bins
  size_t col_bytes = 0;          // bytes from a record's start to this stage's row (the stage's output pointer = records' base)
  int f32 = 0;                   // 1: rows stored as float (narrow wire format)
  double *rec = nullptr;         // D4C only: records' base for the (tpos, f0) head of every record
  // coded records (run_analyze_coded): > 0 = the stage writes its CODED row -- CheapTrick the first code_dims mel-cepstrum
  // coefficients (with the coder's tables), D4C the band aperiodicities -- instead of the row itself
  int code_dims = 0;
  const int *code_knot = nullptr;
  const double *code_frac = nullptr, *code_w_re = nullptr, *code_w_im = nullptr;
  // frames [frame_lo, frame_hi) of every utterance only (stream positions as in a whole-utterance call); skip_prepare:
  // the offsets (and D4C's LoveTrain pass) of the previous call with the same shape are still in the workspace
  int frame_lo = 0, frame_hi = 0x7FFFFFFF;
  bool skip_prepare = false;
};
// Doubles per packed record.  wire 0: [tpos, f0, sp f64[nb], ap f64[nb]]; wire 1: [tpos, f0, sp f32[nb], ap f32[nb]] -- half
// the bytes on the xGMI links and in the D2H copy, 6e-8 relative (the contract is 1e-4): 16 + 8 nb bytes = 2 + nb doubles.
static int record_cols(int fft_size, int wire) {
  const int nb = fft_size / 2 + 1;
  return wire == 1 ? 2 + nb : 2 + 2 * nb;
}

// (d4c.cpp:350-351) fft_size_d4c, the transform of the frame kernel
static int d4c_internal_fft(int fs) { return static_cast<int>(pow(2.0, 1.0 + static_cast<int>(log(4.0 * fs / kFloorF0D4C + 1) / kLog2))); }
// workgroups per d4c_frame launch of the 16384-point shape (each parks its group delay in a slot of global memory,
// stage_params.h): eight rounds of a 256-CU chip that runs one such workgroup per CU -- 134 MB
static int d4c_park_slots(int n_utt, int f_stride) {
  return static_cast<int>(std::min<size_t>((size_t)n_utt * f_stride, (size_t)std::max(n_utt, 2048)));
}

static void arena_reset(WorldHipContext *c) {
  c->arena.reset();
  c->prep_ct.valid = c->prep_d4c.valid = false;
}
// The start of every stage but CheapTrick and D4C: the arena grown to what `carve` measures and carved for real, the
// prepared offsets voided (whatever they were computed for is overwritten), the upload section opened.
template <class Carve> static void begin_stage(WorldHipContext *c, Carve carve) {
  ensure_arena(c, measure(carve));
  arena_reset(c);
  devrt::dpoison(c->arena.base + c->arena.floor, c->arena.cap - c->arena.floor, c->stream);   // (what a call holds at the floor stays)
  carve(c->arena);
  open_uploads(c);
}
// Arrays that outlive the stages of one call: `carve` takes them at the bottom of the arena, where they are held
// (Arena::floor) while `body` runs stages that carve above them.  A stage that needs a larger arena than the one held
// cannot grow it under those arrays (ArenaRegrow): the arena is grown with the floor released and carve and body start over
// (the first call of a shape only; the stages then fit).  `what` names the call in the message.
template <class Carve, class Body> static void hold_at_floor(WorldHipContext *c, const char *what, Carve carve, Body body) {
  struct Release {                                          // the floor never outlives the call, whatever happens in it
    WorldHipContext *c;
    ~Release() { c->arena.floor = 0; c->prep_ct.valid = c->prep_d4c.valid = false; }
  } release{c};
  size_t want = 0;
  for (int attempt = 0;; ++attempt) {
    c->arena.floor = 0;
    ensure_arena(c, std::max(measure(carve), want));
    arena_reset(c);
    devrt::dpoison(c->arena.base, c->arena.cap, c->stream);
    carve(c->arena);
    c->arena.floor = c->arena.used;
    try {
      body();
      return;
    } catch (const ArenaRegrow &r) {
      // growing frees the arena: not possible while the stream is being captured into a graph
      if (devrt::is_capturing(c->stream)) fail("a call shape that was never run before cannot be captured: run it once first");
      if (attempt >= 4) fail("%s: the workspace did not settle", what);
      want = std::max(want, r.bytes);
    }
  }
}

// ---------------------------------------------------------------------------
// The spectral stages' workspace.  CheapTrick's arrays sit at the bottom of the arena, D4C's behind them (a D4C call by
// itself skips CheapTrick's part for its own shape): the two never overlap, so the offset scans of both -- and D4C's
// LoveTrain pass -- survive the other stage's calls, one prepare kernel can serve both (run_spectral_stages), and frame
// ranges of the two stages can alternate while reusing them.  Any other stage's arena_reset() voids them.
// ---------------------------------------------------------------------------
static uint64_t lengths_hash(const int *x_length, const int *n_frames, int n_utt) {
  const uint64_t a = SmallArrays::hash(x_length, sizeof(int) * n_utt), b = SmallArrays::hash(n_frames, sizeof(int) * n_utt);
  return a * 0x9E3779B97F4A7C15ull ^ b;
}
// Claims [lo, hi) of the arena for `mine`; with `reuse` the claim must equal what is there (else: a clear error instead
// of kernels reading garbage offsets).  The other stage's prepared arrays are void if the claim runs into them.
static void claim_prepared(WorldHipContext *c, WorldHipContext::PrepToken &mine, WorldHipContext::PrepToken &other,
                           WorldHipContext::PrepToken want, bool reuse, const char *stage) {
  want.arena_base = c->arena.base; want.generation = c->generation;
  if (reuse) {
    if (!mine.valid)
      fail("%s: reuse_offsets, but this context holds no prepared offsets (another stage, another shape or a regrown "
           "workspace since the call that prepared them)", stage);
    if (!mine.same_inputs(want))
      fail("%s: reuse_offsets, but the prepared offsets belong to other inputs (shape, buffers or options differ from the "
           "call that prepared them)", stage);
    return;
  }
  if (other.valid && want.lo < other.hi && other.lo < want.hi) other.valid = false;
  mine = want;
  mine.valid = true;
}
static void carve_cheaptrick(Arena &a, CtParams &p) {
  // the frame kernel keeps everything between x and the spectrogram in LDS: no per-frame scratch
  p.offsets = a.take<unsigned>((size_t)p.b.n_utt * p.b.f_stride);
  p.frec = a.take<CtFrameRec>((size_t)p.b.n_utt * p.b.f_stride);       // written by the offsets' launch
}
static void carve_d4c(Arena &a, D4cParams &p) {
  CtParams below;
  below.b = p.b;
  carve_cheaptrick(a, below);                                          // behind CheapTrick's part for this shape
  const size_t fr = (size_t)p.b.n_utt * p.b.f_stride;
  p.ap0 = a.take<double>(fr);
  p.offsets1 = a.take<unsigned>(fr);
  p.draws2 = a.take<unsigned>(fr);
  p.draws1 = a.take<unsigned>(p.b.n_utt);
  p.frec = a.take<D4cFrameRec>(fr);                                    // written by offsets1's launch
  p.coarse = a.take<double>(fr * 16);
  const size_t slot = d4c_park_slot_doubles(p.lg_d4c);
  p.park_ws = slot ? a.take<double>(slot * p.park_slots) : nullptr;
}
// A call of CheapTrick and / or D4C: the arena grown to what the carves measure (D4C's includes CheapTrick's part), each
// stage's arrays carved, and its claim on them made -- or, with skip_prepare, checked
static void spectral_workspace(WorldHipContext *c, CtParams *ct, D4cParams *d4c, const int *x_length, const int *n_frames) {
  ensure_arena(c, d4c ? measure([&](Arena &a) { carve_d4c(a, *d4c); }) : measure([&](Arena &a) { carve_cheaptrick(a, *ct); }));
  const BatchView &b = ct ? ct->b : d4c->b;
  WorldHipContext::PrepToken t;
  t.n_utt = b.n_utt; t.fs = b.fs; t.f_stride = b.f_stride; t.x_stride = b.x_stride; t.x = b.x;
  t.lengths_hash = lengths_hash(x_length, n_frames, b.n_utt);
  if (ct) {
    c->arena.reset();
    carve_cheaptrick(c->arena, *ct);
    t.fft = 1 << ct->lg_fft; t.f0 = ct->f0; t.tpos = ct->tpos; t.opt = ct->f0_floor;
    t.lo = 0; t.hi = c->arena.used;
    claim_prepared(c, c->prep_ct, c->prep_d4c, t, ct->skip_prepare != 0, "CheapTrick");
    // (the claim starts at 0 whatever a call holds at the floor, the carve above it: only the carve is this stage's to lose.
    // With skip_prepare everything CheapTrick carves is what the earlier call prepared.)
    if (!ct->skip_prepare) devrt::dpoison(c->arena.base + c->arena.floor, c->arena.used - c->arena.floor, c->stream);
  }
  if (d4c) {
    c->arena.reset();
    carve_d4c(c->arena, *d4c);
    t.fft = d4c->fft_out; t.f0 = d4c->f0; t.tpos = d4c->tpos; t.opt = d4c->threshold;
    t.lo = reinterpret_cast<char *>(d4c->ap0) - c->arena.base; t.hi = c->arena.used;      // (ap0: D4C's first array)
    claim_prepared(c, c->prep_d4c, c->prep_ct, t, d4c->skip_prepare != 0, "D4C");
    // from ap0: CheapTrick's part below it survives a D4C call, as the layout intends.  With skip_prepare ap0 .. frec are
    // what the earlier call prepared; coarse and park_ws behind them are scratch that every call writes before it reads.
    char *lo = reinterpret_cast<char *>(d4c->skip_prepare ? d4c->coarse : d4c->ap0);
    devrt::dpoison(lo, c->arena.base + c->arena.used - lo, c->stream);
  }
}

// ---------------------------------------------------------------------------
// CheapTrick
// ---------------------------------------------------------------------------
static std::string shape_limit(int what, int fs, int fft_size);       // below: "Shape limits of the GPU path"
static void refuse_shape_limit(int what, int fs, int fft_size) {      // a call's first check: before any upload or launch
  const std::string lim = shape_limit(what, fs, fft_size);
  if (!lim.empty()) fail("%s", lim.c_str());
}
// WORLD_HIP_INKERNEL_CONSTS: the frame kernels and Harvest's filter bank evaluate their workgroup-uniform constants
// themselves instead of reading them from the records their producers leave (stage_params.h: CtFrameRec, D4cFrameRec;
// harvest.h: quirk) -- the comparison route of tests/test_gpu_frame_consts.py, read per call like WORLD_HIP_REFINE_FRAMES
static bool inkernel_consts() { return getenv("WORLD_HIP_INKERNEL_CONSTS") != nullptr; }
static CtParams setup_cheaptrick(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                                 const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                                 const double *d_f0, const CheapTrickOption *opt, double *d_sp, const RowLayout &lay,
                                 int *max_frames_out) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  const int lg = ilog2_exact(opt->fft_size);
  const std::string lim = shape_limit(2, fs, opt->fft_size);            // before any upload or launch
  if (!lim.empty()) fail("%s", lim.c_str());
  const int max_frames = *max_frames_out = max_frame_count(n_frames, n_utt, f_stride);
  CtParams p;
  p.b = batch_view(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride);
  p.tpos = d_tpos; p.f0 = d_f0; p.spectrogram = d_sp;
  p.out_row = lay.rows ? upload(c, std::vector<int>(lay.rows, lay.rows + n_utt)) : nullptr;
  p.out_stride = lay.stride ? lay.stride : (size_t)(opt->fft_size / 2 + 1);
  p.out_col_bytes = lay.col_bytes; p.out_f32 = lay.f32;
  p.code_ndim = lay.code_dims; p.code_knot = lay.code_knot; p.code_frac = lay.code_frac;
  p.code_w_re = lay.code_w_re; p.code_w_im = lay.code_w_im;
  if (p.code_ndim > 0 && (lay.f32 || !lay.code_knot || p.code_ndim > opt->fft_size / 4 + 1)) fail("CheapTrick: bad coded-row layout");
  p.f0_floor = 3.0 * fs / (opt->fft_size - 3.0);                       // cheaptrick.cpp:196-198
  p.noise = ensure_noise(c, (size_t)max_frames * ct_max_draws_per_frame(opt->fft_size));
  p.tab = c->tab;
  p.q1 = opt->q1;
  p.lg_fft = lg;
  p.frec = nullptr;                                                    // (carve_cheaptrick)
  p.frame_consts = inkernel_consts() ? 0 : 1;
  p.frame_threads = ct_frame_threads(lg);
  p.lift0 = (1.0 - 2.0 * opt->q1) + 2.0 * opt->q1;                     // ct_frame's k = 0 lifter: the kernel's own expression
  if (lay.frame_lo < 0 || lay.frame_hi < lay.frame_lo) fail("bad frame range [%d, %d)", lay.frame_lo, lay.frame_hi);
  p.frame_lo = lay.frame_lo; p.frame_hi = lay.frame_hi; p.skip_prepare = lay.skip_prepare ? 1 : 0;
  return p;
}
static void run_cheaptrick(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                           const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                           const double *d_f0, const CheapTrickOption *opt, double *d_sp,
                           const RowLayout &lay = RowLayout()) {
  open_uploads(c);
  int max_frames = 0;
  CtParams p = setup_cheaptrick(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, opt, d_sp, lay,
                                &max_frames);
  spectral_workspace(c, &p, nullptr, x_length, n_frames);
  launch_cheaptrick(p, max_frames, c->stream);
}

// ---------------------------------------------------------------------------
// D4C
// ---------------------------------------------------------------------------
static D4cParams setup_d4c(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                           const int *n_frames, int f_stride, const double *d_tpos, const double *d_f0, int fft_size,
                           const D4COption *opt, double *d_ap, const RowLayout &lay, int *max_frames_out) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  ilog2_exact(fft_size);
  const int max_frames = *max_frames_out = max_frame_count(n_frames, n_utt, f_stride);
  // d4c.cpp:350-363 and :264-265
  const int fft_d4c = d4c_internal_fft(fs);
  const int fft_love = static_cast<int>(pow(2.0, 1.0 + static_cast<int>(log(3.0 * fs / 40.0 + 1) / kLog2)));
  if (fft_d4c > 16384 || fft_love > 16384)
    fail("D4C: fs=%d needs an internal FFT of %d > 16384 points (LDS budget); fs <= 192 kHz supported", fs, std::max(fft_d4c, fft_love));
  if (fs < 15800) fail("D4C: fs=%d is below the 15.8 kHz the reference's LoveTrain band edges require", fs);
  const int nap = static_cast<int>(std::min(15000.0, fs / 2.0 - 3000.0) / 3000.0);
  const int wl = static_cast<int>(3000.0 * fft_d4c / fs) * 2 + 1;
  if (nap < 1 || nap > 6) fail("D4C: unsupported number of aperiodicity bands %d", nap);
  if (c->nuttall_len != wl) {                                         // NuttallWindow, common.cpp:113-121
    std::vector<double> w(wl);
    for (int i = 0; i < wl; ++i) {
      double t = i / (wl - 1.0);
      w[i] = 0.355768 - 0.487396 * cos(2.0 * kPi * t) + 0.144232 * cos(4.0 * kPi * t) - 0.012604 * cos(6.0 * kPi * t);
    }
    devrt::sync(c->stream);
    put_table(c, c->d_nuttall, w);
    devrt::sync(c->stream);
    c->nuttall_len = wl;
  }
  if (c->ap_grid_fs != fs || c->ap_grid_fft != fft_size) {
    // GetAperiodicity's interp1 (d4c.cpp:330-338) of the nap + 2 coarse values at knots [0, 3000, .., 3000 nap, fs/2] onto the
    // caller's bins i fs / fft_size: knot (histc) and weight of every bin, with the expressions d4c_finish evaluated per
    // bin and frame until round 6 (same operands, same order: the same bits)
    const int nb_out = fft_size / 2 + 1, nk = nap + 2;
    std::vector<double> frac(nb_out);
    std::vector<int> knot(nb_out);
    for (int i = 0; i < nb_out; ++i) {
      const double xi = static_cast<double>(i) * fs / fft_size;
      int cnt = 0;
      for (int k = 0; k < nk; ++k) {
        const double kn = k <= nap ? k * 3000.0 : fs / 2.0;
        if (kn <= xi) cnt++;
      }
      const int k = cnt < 1 ? 1 : (cnt > nk - 1 ? nk - 1 : cnt);
      const double x0 = (k - 1) <= nap ? (k - 1) * 3000.0 : fs / 2.0;
      const double x1 = k <= nap ? k * 3000.0 : fs / 2.0;
      knot[i] = k;
      frac[i] = (xi - x0) / (x1 - x0);
    }
    devrt::sync(c->stream);
    put_table(c, c->d_ap_frac, frac);
    put_table(c, c->d_ap_knot, knot);
    devrt::sync(c->stream);
    c->ap_grid_fs = fs; c->ap_grid_fft = fft_size;
  }
  D4cParams p;
  p.b = batch_view(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride);
  p.tpos = d_tpos; p.f0 = d_f0; p.aperiodicity = d_ap;
  p.out_row = lay.rows ? upload(c, std::vector<int>(lay.rows, lay.rows + n_utt)) : nullptr;
  p.out_stride = lay.stride ? lay.stride : (size_t)(fft_size / 2 + 1);
  p.out_col_bytes = lay.col_bytes; p.out_f32 = lay.f32;
  p.code_nap = lay.code_dims;
  if (p.code_nap > 0 && lay.f32) fail("D4C: bad coded-row layout");
  p.rec = lay.rec;
  p.park_slots = d4c_park_slots(n_utt, f_stride);
  p.noise = ensure_noise(c, (size_t)max_frames * d4c_max_draws_per_frame(fs));
  p.nuttall = c->d_nuttall;
  p.ap_frac = c->d_ap_frac; p.ap_knot = c->d_ap_knot;
  p.tab = c->tab;
  p.threshold = opt->threshold;
  p.fft_out = fft_size;
  p.lg_love = ilog2_exact(fft_love);
  p.lg_d4c = ilog2_exact(fft_d4c);
  p.nap = nap;
  p.wl = wl;
  // d4c_frame's band transforms rely on the slice being at most 512 packed elements (3000 N / fs < 511.1 for every fs >= 15.8 kHz)
  if (wl / 2 + 1 > 512) fail("D4C: band window of %d samples at fs=%d exceeds the 1023 the frame kernel is built for", wl, fs);
  for (int b = 0; b < 8; ++b) p.band_center[b] = static_cast<int>(3000.0 * (b + 1) * fft_d4c / fs);      // d4c.cpp:207-208
  // the launch's other constants, with the kernels' own expressions (d4c_love_frame, d4c_frame: their REC = false route)
  p.frec = nullptr;                                                    // (carve_d4c)
  p.frame_consts = inkernel_consts() ? 0 : 1;
  p.love_threads = d4c_love_threads(p.lg_love);
  p.frame_threads = d4c_frame_threads(p.lg_d4c);
  p.love_b[0] = static_cast<int>(ceil(100.0 * fft_love / fs));
  p.love_b[1] = static_cast<int>(ceil(4000.0 * fft_love / fs));
  p.love_b[2] = static_cast<int>(ceil(7900.0 * fft_love / fs));
  p.band_bnd = mround(fft_d4c * 8.0 / wl);
  if (lay.frame_lo < 0 || lay.frame_hi < lay.frame_lo) fail("bad frame range [%d, %d)", lay.frame_lo, lay.frame_hi);
  p.frame_lo = lay.frame_lo; p.frame_hi = lay.frame_hi;
  p.skip_prepare = lay.skip_prepare ? kD4cSkipScan | kD4cSkipLoveTrain : 0;
  return p;
}
static void run_d4c(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                    const int *n_frames, int f_stride, const double *d_tpos, const double *d_f0, int fft_size,
                    const D4COption *opt, double *d_ap, const RowLayout &lay = RowLayout()) {
  open_uploads(c);
  int max_frames = 0;
  D4cParams p = setup_d4c(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, fft_size, opt, d_ap,
                          lay, &max_frames);
  spectral_workspace(c, nullptr, &p, x_length, n_frames);
  launch_d4c(p, max_frames, c->stream);
}

// ---------------------------------------------------------------------------
// Harvest
// ---------------------------------------------------------------------------
static void prepare_bands(WorldHipContext *c, int fs, double f0_floor, double f0_ceil, int ratio) {
  HarvestBands &hb = c->bands;
  if (hb.fs == fs && hb.f0_floor == f0_floor && hb.f0_ceil == f0_ceil && hb.nch > 0) return;
  // harvest.cpp:1149-1157
  const double lo = f0_floor * 0.9, hi = f0_ceil * 1.1, cpo = 40;
  const int nch = 1 + static_cast<int>(log(hi / lo) / kLog2 * cpo);
  const double afs = static_cast<double>(fs) / ratio;
  std::vector<double> fb(nch), taps;
  std::vector<int> half(nch), off(nch);
  int max_half = 0;
  for (int i = 0; i < nch; ++i) {
    fb[i] = lo * pow(2.0, (i + 1) / cpo);
    // GetFilteredSignal's time-domain design, harvest.cpp:101-108
    const int L = mround(afs / fb[i] * 2.0);
    half[i] = L;
    off[i] = (int)taps.size();
    max_half = std::max(max_half, L);
    const int len = 2 * L + 1;
    for (int k = -L; k <= L; ++k) {
      double t = (k + L) / (len - 1.0);
      double w = 0.355768 - 0.487396 * cos(2.0 * kPi * t) + 0.144232 * cos(4.0 * kPi * t) - 0.012604 * cos(6.0 * kPi * t);
      taps.push_back(w * cos(2 * kPi * fb[i] * k / afs));
    }
  }
  devrt::sync(c->stream);
  put_table(c, hb.d_band_f0, fb);
  put_table(c, hb.d_taps, taps);
  put_table(c, hb.d_half, half);
  put_table(c, hb.d_off, off);
  devrt::sync(c->stream);
  hb.fs = fs; hb.f0_floor = f0_floor; hb.f0_ceil = f0_ceil; hb.nch = nch; hb.max_half = max_half;
  hb.band_f0 = fb;
  hb.fft_seg = getenv("WORLD_HIP_HARVEST_FIR") ? 0 : hv_fft_segment(max_half);
  if (hb.fft_seg > 0) {
    put_table(c, hb.d_spec, (size_t)nch * kBandFftBins);
    launch_band_spectra(hb.d_taps, hb.d_off, hb.d_half, nch, hb.d_spec, c->tab, c->stream);
    devrt::sync(c->stream);
  } else {
    drop_table(c, hb.d_spec);
  }
}

// The refinement stage's window tables (hv_refine, hv_refine_frames) for one analysis rate and floor, cached beside the bands:
// run_harvest and world_hip_probe_harvest_refine both come here, the probe with an afs of its own.
static void prepare_refine_windows(WorldHipContext *c, double afs, double f0_floor) {
  HarvestBands &hb = c->bands;
  if (hb.win_afs == afs && hb.win_floor == f0_floor && hb.win_tab_len > 0) return;
  devrt::sync(c->stream);
  // GetMainWindow's angles for every window half length hv_refine can meet (harvest.cpp:446-456), d = 2/(2hw+1):
  //   [hw][6]        sin/cos(pi d), sin/cos(pi kWinLanes d), 2 / window length in seconds, pi d
  //   then [hw][kWinLanes] (sin, cos)(pi (lane - hw - 1) d): a lane's FIRST sample of the window when the frame centre falls on
  //                  a whole sample (it does at 8 kHz: the decimated rate of 16 / 32 / 48 / 96 kHz input); the kernel turns
  //                  it by the residual angle for other rates.  One 16-byte load replaces a division and a sincospi per
  //                  window rebuild (70 of its ~190 instructions).
  const int hw_max = static_cast<int>(1.5 * afs / f0_floor + 1.0) + 2;
  const size_t head = (size_t)(hw_max + 1) * 6;
  std::vector<double> wt(head + (size_t)(hw_max + 1) * kWinLanes * 2);
  const long double pi_l = 3.14159265358979323846264338327950288L;
  for (int hw = 0; hw <= hw_max; ++hw) {
    const double wlen_t = (2.0 * hw + 1.0) / afs;
    const double d = (1.0 / afs) * (2.0 / wlen_t);
    wt[6 * hw + 0] = sin(kPi * d); wt[6 * hw + 1] = cos(kPi * d);
    wt[6 * hw + 2] = sin(kPi * (kWinLanes * d)); wt[6 * hw + 3] = cos(kPi * (kWinLanes * d));
    wt[6 * hw + 4] = 2.0 / ((2.0 * hw + 1.0) * (1.0 / afs));           // the kernel's two_over_t, same operations
    wt[6 * hw + 5] = kPi * d;
    const long double dl = 2.0L / (2.0L * hw + 1.0L);
    for (int lane = 0; lane < kWinLanes; ++lane) {
      const long double a = pi_l * (lane - hw - 1) * dl;
      wt[head + ((size_t)hw * kWinLanes + lane) * 2 + 0] = (double)sinl(a);
      wt[head + ((size_t)hw * kWinLanes + lane) * 2 + 1] = (double)cosl(a);
    }
  }
  // Where a millisecond is a whole number of samples (8 kHz: the decimated rate of 16 / 32 / 48 / 96 kHz input) every
  // refinement window is centred ON a sample, and the window of half length hw is the same 2 hw + 1 numbers at every
  // frame: the main window (GetMainWindow, harvest.cpp:446-456) and its central difference (GetDiffWindow, :462-468) as
  // (w, dw) pairs, the window of half length hw at entry hw^2 (sum of 2 h + 1 below it).  A rebuild is then a load and two
  // products per sample instead of ~25 FP64 operations (round 4: window rebuilds were 18 of a wavefront-frame's 65
  // thousand cycles).  Other rates keep the rotation route (wt above).
  hb.win_full_entries = 0;
  if (fmod(afs, 1000.0) == 0.0) {
    hb.win_full_entries = (size_t)(hw_max + 1) * (hw_max + 1);
    const size_t base = wt.size();
    wt.resize(base + 2 * hb.win_full_entries);
    std::vector<long double> w;
    for (int hw = 0; hw <= hw_max; ++hw) {
      const int blen = 2 * hw + 1;
      w.assign(blen, 0.0L);
      const long double dl = 2.0L / (2.0L * hw + 1.0L);
      for (int i = 0; i < blen; ++i) {
        const long double a = pi_l * (i - hw - 1) * dl;
        w[i] = 0.42L + 0.5L * cosl(a) + 0.08L * cosl(2.0L * a);
      }
      double *o = wt.data() + base + 2 * (size_t)hw * hw;
      for (int i = 0; i < blen; ++i) {
        long double dw;
        if (blen == 1) dw = 0.0L;
        else if (i == 0) dw = -w[1] / 2.0L;
        else if (i == blen - 1) dw = w[blen - 2] / 2.0L;
        else dw = -(w[i + 1] - w[i - 1]) / 2.0L;
        o[2 * i] = (double)w[i]; o[2 * i + 1] = (double)dw;
      }
    }
  }
  put_table(c, hb.d_win_tab, wt);
  devrt::sync(c->stream);
  hb.win_tab_len = hw_max + 1;
  hb.win_afs = afs; hb.win_floor = f0_floor;
}
// What the refinement kernels read beside the signal and the candidates (p.afs and p.f0_floor are set): the LDS doubles per
// window, the tables above and the route.  `rotate`: build the windows by rotation where the table exists too
// (WORLD_HIP_REFINE_ROTATE); `frames`: the frame-major kernel on the table (WORLD_HIP_REFINE_FRAMES).
static void plan_harvest_refine(WorldHipContext *c, HarvestParams &p, bool rotate, bool frames) {
  prepare_refine_windows(c, p.afs, p.f0_floor);
  const HarvestBands &hb = c->bands;
  p.refine_cap = 2 * static_cast<int>(1.5 * p.afs / p.f0_floor + 1.0) + 4;
  p.tab = c->tab;
  p.win_tab = hb.d_win_tab; p.win_lane = hb.d_win_tab + (size_t)hb.win_tab_len * 6;
  p.win_full = hb.win_full_entries && !rotate
                   ? reinterpret_cast<const double2 *>(p.win_lane + (size_t)hb.win_tab_len * kWinLanes * 2) : nullptr;
  // the candidate-major hv_refine serves the table route; this runs the frame-major kernel there instead (same bits)
  p.refine_frames = frames;
}

// Harvest's back half -- hv_prune and the contour kernels (launch_harvest_tail) -- as run_harvest and
// world_hip_probe_harvest_contour both set it up: the HarvestParams fields those kernels read beside maxc, nc and nfb, and the
// part of the workspace they work in (the end of run_harvest's carve).
static void plan_harvest_tail(const WorldHipContext *c, HarvestParams &p, int n_utt, int max_fb) {
  p.fb_stride = (max_fb + 7) & ~7;
  p.sec_cap = hv_section_rows(max_fb);
  p.lone_job = n_utt == 1 && !(c->hint & WORLD_HIP_HINT_SHARED_DEVICE);
  p.ext_cap = max_fb + 304 * hv_sliced_sections(max_fb) + 8;
}
static void carve_harvest_tail(Arena &a, HarvestParams &p, size_t B) {
  const size_t cand_elems = B * p.fb_stride * p.maxc;
  p.cand_a = a.take<double>(cand_elems); p.score_a = a.take<double>(cand_elems);
  p.cand_b = a.take<double>(cand_elems); p.score_b = a.take<double>(cand_elems);
  p.nc = a.take<int>(B);
  p.c0 = a.take<double>(B * p.fb_stride);
  p.c2 = a.take<double>(B * p.fb_stride); p.c3 = a.take<double>(B * p.fb_stride);
  p.basic_f0 = a.take<double>(B * p.fb_stride);
  p.sec = a.take<int>(B * 6 * p.sec_cap);
  p.sec_n = a.take<int>(B * 2);
  p.sec_sum = a.take<double>(B * p.sec_cap);
  p.ext = a.take<double>(B * p.ext_cap);
}

static void run_harvest(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                        const int *x_length, const HarvestOption *opt, int f_stride, double *d_tpos,
                        double *d_f0) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  if (!(opt->f0_floor > 0) || !(opt->f0_ceil > opt->f0_floor) || !(opt->frame_period > 0)) fail("bad HarvestOption");
  HarvestParams p;
  // Harvest(): harvest.cpp:1226-1228
  p.ratio = std::max(std::min(mround(fs / 8000.0), 12), 1);
  p.afs = static_cast<double>(fs) / p.ratio;
  prepare_bands(c, fs, opt->f0_floor, opt->f0_ceil, p.ratio);
  const HarvestBands &hb = c->bands;
  p.f0_floor = opt->f0_floor; p.f0_ceil = opt->f0_ceil; p.frame_period = opt->frame_period;
  p.nch = hb.nch;
  p.maxc = mround(hb.nch / 10.0) * 7;                                  // harvest.cpp:1179-1181
  if (p.maxc > 256) fail("Harvest: %d candidate slots per frame exceed the 256 the tracking kernel handles", p.maxc);
  p.lag = static_cast<int>(ceil(140.0 / p.ratio) * p.ratio);           // harvest.cpp:50-51
  std::vector<int> xl(x_length, x_length + n_utt), yl(n_utt), nfb(n_utt), nfr(n_utt), rfft(n_utt);
  int max_x = 0, max_y = 0, max_fb = 0, max_fr = 0;
  for (int u = 0; u < n_utt; ++u) {
    yl[u] = static_cast<int>(ceil(static_cast<double>(xl[u]) / p.ratio));   // harvest.cpp:1161-1162
    // the reference's transform length (harvest.cpp:1164-1165, GetSuitableFFTSize = common.cpp:51-54)
    const int span = yl[u] + 5 + 2 * static_cast<int>(2.0 * p.afs / hb.band_f0[0]);
    rfft[u] = static_cast<int>(pow(2.0, static_cast<int>(log(static_cast<double>(span)) / kLog2) + 1.0));
    nfb[u] = frame_count(fs, xl[u], 1);
    nfr[u] = frame_count(fs, xl[u], opt->frame_period);
    if (nfr[u] > f_stride) fail("f_stride %d too small for %d frames", f_stride, nfr[u]);
    max_x = std::max(max_x, xl[u]); max_y = std::max(max_y, yl[u]);
    max_fb = std::max(max_fb, nfb[u]); max_fr = std::max(max_fr, nfr[u]);
  }
  p.y_stride = (max_y + 7) & ~7;
  plan_harvest_tail(c, p, n_utt, max_fb);
  p.m_stride = (max_x + 2 * p.lag + 2 * kDecPad + 7) & ~7;
  p.ev_cap = max_y / 2 + 2;
  plan_harvest_refine(c, p, getenv("WORLD_HIP_REFINE_ROTATE") != nullptr, getenv("WORLD_HIP_REFINE_FRAMES") != nullptr);
  p.max_half = hb.max_half;
  p.fft_seg = hb.fft_seg;
  p.fft_pre = hb.max_half - 1;
  p.band_spec = hb.d_spec;
  if (p.fft_seg > 0) {
    // FFT path: a workgroup filters `chunk_blocks` consecutive blocks of one (band, utterance) and appends their events to one
    // list.  Batches get one chunk per utterance (the final lists, no compaction pass); a lone utterance is cut into
    // enough chunks to fill the chip (~2048 workgroups).
    p.nblk = (max_y + p.fft_seg - 1) / p.fft_seg;
    const int want = std::max(1, std::min(p.nblk, (2048 + p.nch * n_utt - 1) / (p.nch * n_utt)));
    p.chunk_blocks = (p.nblk + want - 1) / want;
    p.nseg = (p.nblk + p.chunk_blocks - 1) / p.chunk_blocks;
    p.seg_cap = p.nseg == 1 ? p.ev_cap : std::min(p.ev_cap, p.chunk_blocks * p.fft_seg / 2 + 2);
  } else {
    p.nblk = 0; p.chunk_blocks = 0;
    p.nseg = band_segments(max_y);
    p.seg_cap = kSegCap;
  }
  const bool direct_lists = p.fft_seg > 0 && p.nseg == 1;     // the filter bank writes the final event lists itself

  const size_t B = n_utt;
  // utterances whose zero-crossing lists exist at once (harvest.hip: launch_harvest): WORLD_HIP_EVENT_GROUP, default 40 --
  // a 40-utterance launch of the filter bank is 6 080 workgroups, six times what the chip holds at once.  Measured on the
  // configs[3] share (128 utterances, two contexts in flight): groups of 128 / 64 / 32 -> 4.625 / 4.614 / 4.599 M frames/s
  // with 36.0 / 21.9 / 14.9 GB of workspace; configs[2] (256 utterances): 10.68 M with 71.9 GB ungrouped, 10.69 M with
  // 29.9 GB in groups of 64.
  static const int ev_group_env = [] { const char *e = getenv("WORLD_HIP_EVENT_GROUP"); return e ? std::max(1, atoi(e)) : 40; }();
  p.ev_group = std::min(n_utt, ev_group_env);
  p.ev_u0 = 0;
  const size_t E = p.ev_group;
  p.nyq_slices = (max_y + 4095) / 4096;                                // kMeanSlice of harvest.hip
  // launch_harvest's grids: spans of the decimation sweeps (harvest.hip), or the 4096-sample slices at ratio 1
  p.mean_parts = p.ratio == 1 ? p.nyq_slices : (max_x + 2 * p.lag + 2 * kDecPad + kDecSpan - 1) / kDecSpan;
  begin_stage(c, [&](Arena &a) {
    p.nyq = a.take<double>(B * p.nyq_slices * 4);
    p.mean_part = a.take<double>(B * p.mean_parts);
    p.quirk = a.take<double>(B * p.nch * kQuirkDoubles);
    p.fwd = a.take<double>(B * p.m_stride);
    p.y = a.take<double>(B * p.y_stride);
    p.events = a.take<double>(E * p.nch * 4 * p.ev_cap);
    p.ev_count = a.take<int>(E * p.nch * 4);
    if (direct_lists) {
      p.seg_events = p.events; p.seg_count = p.ev_count;
    } else {
      p.seg_events = a.take<double>(E * p.nch * 4 * p.nseg * p.seg_cap);
      p.seg_count = a.take<int>(E * p.nch * 4 * p.nseg);
    }
    p.blk_spec = a.take<double2>(B * p.nblk * kBandFftBins);
    p.raw = a.take<double>(B * p.nch * p.fb_stride);
    carve_harvest_tail(a, p, B);
  });
  p.b = batch_view(c, n_utt, fs, d_x, x_stride, x_length, nfr.data(), f_stride);
  p.y_len = upload(c, yl);
  p.nfb = upload(c, nfb);
  p.ref_fft = upload(c, rfft);
  p.band_f0 = hb.d_band_f0; p.band_half = hb.d_half; p.band_off = hb.d_off; p.band_taps = hb.d_taps;
  p.inkernel_consts = inkernel_consts() ? 1 : 0;
  p.tpos = d_tpos; p.f0 = d_f0;
  launch_harvest(p, max_x, max_y, max_fb, max_fr, c->stream);
#ifdef WORLD_EMU
  // host emulation only (synchronous): intermediate stages for debugging against the oracle's WO_DUMP
  if (const char *dump = getenv("WORLD_EMU_DUMP")) {
    auto put = [&](const char *tag, const void *ptr, size_t bytes) {
      std::string fn = std::string(dump) + "_" + tag + ".bin";
      FILE *f = fopen(fn.c_str(), "wb"); fwrite(ptr, 1, bytes, f); fclose(f);
    };
    int hdr[6] = {p.nch, p.fb_stride, p.maxc, max_fb, p.y_stride, yl[0]};
    put("hdr", hdr, sizeof hdr);
    put("y", p.y, sizeof(double) * p.y_stride);
    put("raw", p.raw, sizeof(double) * p.nch * p.fb_stride);
    put("cand_a", p.cand_a, sizeof(double) * p.fb_stride * p.maxc);
    put("cand_b", p.cand_b, sizeof(double) * p.fb_stride * p.maxc);
    put("score_a", p.score_a, sizeof(double) * p.fb_stride * p.maxc);
    put("score_b", p.score_b, sizeof(double) * p.fb_stride * p.maxc);
    put("basic", p.basic_f0, sizeof(double) * p.fb_stride);
    put("nc", p.nc, sizeof(int));
  }
#endif
}

// ---------------------------------------------------------------------------
// DIO / StoneMask
// ---------------------------------------------------------------------------
static void prepare_dio_bands(WorldHipContext *c, int fs, const DioOption *opt, int ratio) {
  DioBands &db = c->dio_bands;
  if (db.fs == fs && db.ratio == ratio && db.f0_floor == opt->f0_floor && db.f0_ceil == opt->f0_ceil &&
      db.cpo == opt->channels_in_octave && db.nb > 0)
    return;
  const double afs = static_cast<double>(fs) / ratio;
  // dio.cpp:582-586
  const int nb = 1 + static_cast<int>(log(opt->f0_ceil / opt->f0_floor) / kLog2 * opt->channels_in_octave);
  std::vector<double> fb(nb), taps, lowcut;
  std::vector<int> hal(nb), off(nb);
  int max_ntap = 0;
  for (int i = 0; i < nb; ++i) {
    fb[i] = opt->f0_floor * pow(2.0, (i + 1) / opt->channels_in_octave);
    hal[i] = mround(afs / fb[i] / 2.0);                               // dio.cpp:532
    off[i] = (int)taps.size();
    const int len = 4 * hal[i];                                      // NuttallWindow(hal*4), dio.cpp:301
    max_ntap = std::max(max_ntap, len);
    for (int k = 0; k < len; ++k) {
      double t = k / (len - 1.0);
      taps.push_back(0.355768 - 0.487396 * cos(2.0 * kPi * t) + 0.144232 * cos(4.0 * kPi * t) -
                     0.012604 * cos(6.0 * kPi * t));
    }
  }
  // DesignLowCutFilter (dio.cpp:40-53): delta minus a normalised Hanning window, centred
  const int cut = mround(afs / 50.0);
  const int n = 2 * cut + 1;
  lowcut.resize(n);
  for (int i = 1; i <= n; ++i) lowcut[i - 1] = 0.5 - 0.5 * cos(i * 2.0 * kPi / (n + 1));
  double sum = 0.0;
  for (int i = 0; i < n; ++i) sum += lowcut[i];
  for (int i = 0; i < n; ++i) lowcut[i] = -lowcut[i] / sum;
  lowcut[cut] += 1.0;
  devrt::sync(c->stream);
  put_table(c, db.d_band_f0, fb);
  put_table(c, db.d_taps, taps);
  put_table(c, db.d_lowcut, lowcut);
  put_table(c, db.d_hal, hal);
  put_table(c, db.d_off, off);
  devrt::sync(c->stream);
  db.fs = fs; db.ratio = ratio; db.f0_floor = opt->f0_floor; db.f0_ceil = opt->f0_ceil;
  db.cpo = opt->channels_in_octave; db.nb = nb; db.cut = cut; db.max_ntap = max_ntap;
  db.band_f0_first = fb[0];
}

static void run_dio(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                    const DioOption *opt, int f_stride, double *d_tpos, double *d_f0) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  if (!(opt->f0_floor > 0) || !(opt->f0_ceil > opt->f0_floor) || !(opt->frame_period > 0) ||
      !(opt->channels_in_octave > 0))
    fail("bad DioOption");
  DioParams p;
  p.ratio = std::max(std::min(opt->speed, 12), 1);                    // dio.cpp:589
  p.afs = static_cast<double>(fs) / p.ratio;
  prepare_dio_bands(c, fs, opt, p.ratio);
  const DioBands &db = c->dio_bands;
  p.f0_floor = opt->f0_floor; p.f0_ceil = opt->f0_ceil; p.frame_period = opt->frame_period;
  p.allowed_range = opt->allowed_range;
  p.nb = db.nb; p.cut = db.cut; p.max_ntap = db.max_ntap;
  // one tile of the longest channel filter (4 round(fs / ratio / (floor 2^(1/channels)) / 2) taps) with its inputs and outputs is
  // what a workgroup of dio_band_events holds in LDS; the low-cut filter has a route with its taps left in global memory
  if (band_lds_bytes(p.max_ntap) > kLdsPerCu || band_lds_bytes(2 * p.cut + 1) - sizeof(double) * (2 * p.cut + 2) > kLdsPerCu)
    fail("Dio: fs=%d / speed %d with f0_floor %g needs a channel filter of %d taps, more LDS than a CU has "
         "(raise DioOption.speed or f0_floor: <= %d taps)", fs, p.ratio, opt->f0_floor, p.max_ntap, 7400);
  p.vrm = static_cast<int>(0.5 + 1000.0 / opt->frame_period / opt->f0_floor) * 2 + 1;   // dio.cpp:263-264
  std::vector<int> xl(x_length, x_length + n_utt), yl(n_utt), nfr(n_utt), rfft(n_utt);
  int max_x = 0, max_y = 0, max_fr = 0;
  for (int u = 0; u < n_utt; ++u) {
    yl[u] = 1 + xl[u] / p.ratio;                                      // dio.cpp:590
    // the reference's transform length (dio.cpp:592-594, GetSuitableFFTSize = common.cpp:51-54)
    const int span = yl[u] + mround(p.afs / 50.0) * 2 + 1 + 4 * static_cast<int>(1.0 + p.afs / db.band_f0_first / 2.0);
    rfft[u] = static_cast<int>(pow(2.0, static_cast<int>(log(static_cast<double>(span)) / kLog2) + 1.0));
    nfr[u] = frame_count(fs, xl[u], opt->frame_period);
    if (nfr[u] > f_stride) fail("f_stride %d too small for %d frames", f_stride, nfr[u]);
    max_x = std::max(max_x, xl[u]); max_y = std::max(max_y, yl[u]); max_fr = std::max(max_fr, nfr[u]);
  }
  p.y_stride = (max_y + 8) & ~7;
  p.z_stride = (max_y + 2 * p.cut + 8) & ~7;
  p.m_stride = (max_x + 2 * kDecPad + 8) & ~7;
  p.nseg = band_segments(max_y);
  p.ev_cap = max_y / 2 + 2;
  const size_t B = n_utt;
  begin_stage(c, [&](Arena &a) {
    p.nyq = a.take<double>(B * 4);
    p.quirk = a.take<double>(B * p.nb * 4);
    p.fwd = a.take<double>(B * p.m_stride);
    p.y = a.take<double>(B * p.y_stride);
    p.z = a.take<double>(B * p.z_stride);
    p.seg_events = a.take<double>(B * p.nb * 4 * p.nseg * kSegCap);
    p.seg_count = a.take<int>(B * p.nb * 4 * p.nseg);
    p.events = a.take<double>(B * p.nb * 4 * p.ev_cap);
    p.ev_count = a.take<int>(B * p.nb * 4);
    p.cand = a.take<double>(B * p.nb * f_stride);
    p.score = a.take<double>(B * p.nb * f_stride);
    p.t1 = a.take<double>(B * f_stride);
    p.t2 = a.take<double>(B * f_stride);
  });
  p.b = batch_view(c, n_utt, fs, d_x, x_stride, x_length, nfr.data(), f_stride);
  p.y_len = upload(c, yl);
  p.ref_fft = upload(c, rfft);
  p.band_f0 = db.d_band_f0; p.band_hal = db.d_hal; p.band_off = db.d_off; p.band_taps = db.d_taps;
  p.lowcut_taps = db.d_lowcut;
  p.tpos = d_tpos; p.f0 = d_f0;
  launch_dio(p, max_x, max_y, max_fr, c->stream);
}

static void run_stonemask(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                          const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                          const double *d_f0, double *d_refined) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  const int max_frames = max_frame_count(n_frames, n_utt, f_stride);
  StoneMaskParams p;
  p.win_cap = 2 * static_cast<int>(1.5 * fs / 40.0 + 1.0) + 4;       // longest window: f0 just above 40 Hz
  if (stonemask_lds_bytes(p.win_cap) > 160 * 1024)
    fail("StoneMask: fs=%d needs a %d-sample window (%zu bytes of LDS > 160 KiB); fs <= 240 kHz supported", fs, p.win_cap,
         stonemask_lds_bytes(p.win_cap));
  begin_stage(c, [](Arena &) {});
  p.b = batch_view(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride);
  p.tpos = d_tpos; p.f0 = d_f0; p.refined = d_refined;
  p.tab = c->tab;
  launch_stonemask(p, max_frames, c->stream);
}

// ---------------------------------------------------------------------------
// Codec (reference src/codec.cpp): every table depends on (fs, fft_size) only
// ---------------------------------------------------------------------------
// interp1's histc + weights (matlabfunctions.cpp:136-176) for fixed knots x and queries xi
static void interp1_tables(const std::vector<double> &x, const std::vector<double> &xi, std::vector<int> *knot,
                           std::vector<double> *frac) {
  const int n = (int)x.size();
  knot->resize(xi.size()); frac->resize(xi.size());
  for (size_t i = 0; i < xi.size(); ++i) {
    int c = 0;
    while (c < n && x[c] <= xi[i]) ++c;
    const int k = c < 1 ? 1 : (c > n - 1 ? n - 1 : c);
    (*knot)[i] = k;
    (*frac)[i] = (xi[i] - x[k - 1]) / (x[k] - x[k - 1]);
  }
}

// (not a cached_table: this cache is unbounded and does not refuse a miss under capture, and stays so)
static const CodecTables &codec_tables(WorldHipContext *c, int fs, int fft_size) {
  for (const CodecTables &t : c->codec_tables)
    if (t.fs == fs && t.fft_size == fft_size) return t;
  const int md = fft_size / 2, nb = md + 1;
  const double kM0 = 1127.01048, kF0 = 700.0;                          // constantnumbers.h:45-46
  auto mel_of = [&](double f) { return kM0 * log(f / kF0 + 1.0); };    // codec.cpp:59-61
  auto freq_of = [&](double m) { return kF0 * (exp(m / kM0) - 1.0); }; // codec.cpp:66-68
  const double floor_mel = mel_of(40.0), ceil_mel = mel_of(std::min(fs / 2.0, 20000.0));
  std::vector<int> knot;
  std::vector<double> frac;
  CodecTables t;
  t.fs = fs; t.fft_size = fft_size;
  {  // GetParametersForCoding, codec.cpp:162-180
    std::vector<double> mel_axis(md), faxis(nb), wr(md), wi(md);
    for (int i = 0; i < md; ++i) {
      mel_axis[i] = (ceil_mel - floor_mel) * i / md + floor_mel;
      wr[i] = 2.0 * cos(i * kPi / fft_size) / sqrt(static_cast<double>(fft_size));
      wi[i] = 2.0 * sin(i * kPi / fft_size) / sqrt(static_cast<double>(fft_size));
    }
    wr[0] /= sqrt(2.0);
    for (int i = 0; i <= md; ++i) faxis[i] = mel_of(static_cast<double>(i) * fs / fft_size);
    interp1_tables(faxis, mel_axis, &knot, &frac);
    put_table(c, t.d_knot_code, knot); put_table(c, t.d_frac_code, frac);
    put_table(c, t.d_wc_re, wr); put_table(c, t.d_wc_im, wi);
    devrt::sync(c->stream);
  }
  {  // GetParametersForDecoding, codec.cpp:185-207
    std::vector<double> mel_axis(md + 2), faxis(nb), wr(md), wi(md);
    for (int i = 0; i < md; ++i) {
      wr[i] = cos(i * kPi / fft_size) * sqrt(static_cast<double>(fft_size));
      wi[i] = sin(i * kPi / fft_size) * sqrt(static_cast<double>(fft_size));
      mel_axis[i + 1] = freq_of((ceil_mel - floor_mel) * i / md + floor_mel);
    }
    wr[0] /= sqrt(2.0);
    mel_axis[0] = 0;
    mel_axis[md + 1] = fs / 2.0;
    for (int i = 0; i < nb; ++i) faxis[i] = static_cast<double>(i) * fs / fft_size;
    interp1_tables(mel_axis, faxis, &knot, &frac);
    put_table(c, t.d_knot_dec, knot); put_table(c, t.d_frac_dec, frac);
    put_table(c, t.d_wd_re, wr); put_table(c, t.d_wd_im, wi);
    devrt::sync(c->stream);
  }
  {  // DecodeAperiodicity's axes, codec.cpp:242-250
    const int nap = static_cast<int>(std::min(15000.0, fs / 2.0 - 3000.0) / 3000.0);
    std::vector<double> caxis(std::max(nap, 0) + 2), faxis(nb);
    for (int i = 0; i <= nap; ++i) caxis[i] = i * 3000.0;
    caxis[std::max(nap, 0) + 1] = fs / 2.0;
    for (int i = 0; i < nb; ++i) faxis[i] = static_cast<double>(fs) / fft_size * i;
    interp1_tables(caxis, faxis, &knot, &frac);
    put_table(c, t.d_knot_ap, knot); put_table(c, t.d_frac_ap, frac);
    devrt::sync(c->stream);
  }
  c->codec_tables.push_back(t);
  return c->codec_tables.back();
}

static int number_of_aperiodicities(int fs) {                          // codec.cpp:212-215
  return static_cast<int>(std::min(15000.0, fs / 2.0 - 3000.0) / 3000.0);
}

void launch_pcm16_to_double(const short *d_pcm, double *d_x, long n, hipStream_t stream);   // pcm.hip
void launch_pcm_bytes_to_double(const unsigned char *d_pcm, double *d_x, long n, int qb, double zero_line,
                                hipStream_t stream);
void launch_double_to_pcm16(const double *d_x, short *d_pcm, long n, hipStream_t stream);

enum CodecOp { kCodeSp, kDecodeSp, kCodeAp, kDecodeAp };
static void run_codec(WorldHipContext *c, CodecOp op, int rows, int fs, int fft_size, int ndim, const double *d_in,
                      double *d_out, size_t in_stride = 0, size_t out_stride = 0) {
  if (rows < 0) fail("negative row count");
  if (rows == 0) return;
  if (fs <= 0) fail("fs must be positive");
  if (!d_in || !d_out) fail("null buffer");
  const int lg = ilog2_exact(fft_size);
  CodecParams p;
  p.in = d_in; p.out = d_out; p.rows = rows; p.fs = fs; p.fft_size = fft_size; p.lg_md = lg - 1; p.ndim = ndim;
  p.in_stride = in_stride; p.out_stride = out_stride;
  p.tab = c->tab;
  p.knot = nullptr; p.frac = nullptr; p.w_re = nullptr; p.w_im = nullptr;
  if (op == kCodeSp || op == kDecodeSp) {
    if (lg < 7 || lg > 13) fail("codec: fft_size %d unsupported (128..8192)", fft_size);
    // the DCT is one real FFT of fft_size/2 points: it has fft_size/4+1 bins (the reference reads
    // never-written plan memory beyond them, codec.cpp:84-86)
    if (ndim < 1 || ndim > fft_size / 4 + 1) fail("codec: number_of_dimensions %d outside [1, fft_size/4+1]", ndim);
  } else {
    p.ndim = number_of_aperiodicities(fs);
    if (p.ndim < 1) fail("codec: fs=%d has no aperiodicity band (needs fs >= 12 kHz)", fs);
    if (3000.0 * p.ndim > fs / 2.0) fail("codec: band centre beyond fs/2");
  }
  const CodecTables &t = codec_tables(c, fs, fft_size);
  switch (op) {
    case kCodeSp:
      p.knot = t.d_knot_code; p.frac = t.d_frac_code; p.w_re = t.d_wc_re; p.w_im = t.d_wc_im;
      launch_code_spectral_envelope(p, c->stream);
      break;
    case kDecodeSp:
      p.knot = t.d_knot_dec; p.frac = t.d_frac_dec; p.w_re = t.d_wd_re; p.w_im = t.d_wd_im;
      launch_decode_spectral_envelope(p, c->stream);
      break;
    case kCodeAp:
      launch_code_aperiodicity(p, c->stream);
      break;
    case kDecodeAp:
      p.knot = t.d_knot_ap; p.frac = t.d_frac_ap;
      launch_decode_aperiodicity(p, c->stream);
      break;
  }
}

// ---------------------------------------------------------------------------
// Synthesis (reference src/synthesis.cpp:339-399)
// ---------------------------------------------------------------------------
// Where the synthesiser finds its frames (SynthParams' row addressing, synthesis.h): the dense arrays of the batched
// calls, a staging of the same kind, or f64 records read in place.
struct SynthRows {
  const double *f0, *sp, *ap;
  std::vector<long long> first_row;   // [n_utt]
  size_t row_stride, f0_stride;
};
// the synthesis stage itself; every argument has been checked (max_y = the largest y_length)
static void synthesize_rows(WorldHipContext *c, int n_utt, int fs, double frame_period, int fft_size, const int *n_frames,
                            const SynthRows &rows, const int *y_length, int y_stride, int max_y, double *d_y) {
  const int lg = ilog2_exact(fft_size);
  if (c->dc_remover_len != fft_size) {                                 // GetDCRemover, synthesis.cpp:320-335
    std::vector<double> rem(fft_size);
    double dc = 0.0;
    for (int i = 0; i < fft_size / 2; ++i) {
      rem[i] = 0.5 - 0.5 * cos(2.0 * kPi * (i + 1.0) / (1.0 + fft_size));
      rem[fft_size - i - 1] = rem[i];
      dc += rem[i] * 2.0;
    }
    for (int i = 0; i < fft_size / 2; ++i) { rem[i] /= dc; rem[fft_size - i - 1] = rem[i]; }
    devrt::sync(c->stream);
    put_table(c, c->d_dc_remover, rem);
    devrt::sync(c->stream);
    c->dc_remover_len = fft_size;
  }
  SynthParams p;
  p.n_utt = n_utt; p.fs = fs; p.fft_size = fft_size; p.lg_fft = lg;
  p.frame_period = frame_period / 1000.0;
  p.lowest_f0 = fs / fft_size + 1.0;                                   // integer division (synthesis.cpp:361)
  p.f0 = rows.f0; p.sp = rows.sp; p.ap = rows.ap; p.row_stride = rows.row_stride; p.f0_stride = rows.f0_stride;
  p.y = d_y; p.y_stride = y_stride;
  p.nblk = (max_y + synth_tile_samples() - 1) / synth_tile_samples();
  // Room for a mean pulse rate of 1200 Hz over the longest utterance unless the caller said otherwise (voiced
  // pulses come at f0, unvoiced ones at 500 Hz).  The pulse count is only known on the device; a call that
  // needs more records the count (need), world_hip_sync / world_hip_synthesis_pulses_dropped report it, and the
  // drop-in Synthesis() -- which waits for its result anyway -- repeats the call with the exact capacity.
  p.pulse_cap = c->synth_pulse_cap > 0 ? c->synth_pulse_cap : static_cast<int>(static_cast<double>(max_y) * 1200.0 / fs) + 16;
  if (!c->d_synth_need) {
    put_table(c, c->d_synth_need, 1);
    devrt::dzero(c->d_synth_need, sizeof(int), c->stream);
  }
  p.need = c->d_synth_need;
  p.resp_stride = lg > 12 ? fft_size + 2 : fft_size;                   // (sy_pulse: the 8192-point pulse keeps its spectrum in its slot)
  const size_t B = n_utt;
  begin_stage(c, [&](Arena &a) {
    p.inc = a.take<double>(B * y_stride);
    p.flags = a.take<unsigned char>(B * y_stride);
    p.blk_cnt = a.take<int>(B * p.nblk);
    p.pidx = a.take<int>(B * p.pulse_cap);
    p.pshift = a.take<double>(B * p.pulse_cap);
    p.np = a.take<int>(B);
    p.resp = a.take<double>(B * p.pulse_cap * p.resp_stride);
  });
  p.n_frames = upload(c, n_frames, n_utt);
  p.y_len = upload(c, y_length, n_utt);
  p.first_row = upload(c, rows.first_row);
  p.dc_remover = c->d_dc_remover;
  p.noise = ensure_noise(c, (size_t)max_y + 8);
  p.tab = c->tab;
  launch_synthesis(p, max_y, c->stream);
}

static void run_synthesis(WorldHipContext *c, int n_utt, int fs, double frame_period, int fft_size, const int *n_frames,
                          int f_stride, const double *d_f0, const double *d_sp, const double *d_ap,
                          const int *y_length, int y_stride, double *d_y) {
  if (n_utt <= 0) fail("n_utt must be positive");
  if (fs <= 0 || frame_period <= 0) fail("fs and frame_period must be positive");
  if (!d_f0 || !d_sp || !d_ap || !d_y || !n_frames || !y_length) fail("null buffer");
  ilog2_exact(fft_size);
  refuse_shape_limit(8, fs, fft_size);
  int max_y = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (n_frames[u] < 2 || n_frames[u] > f_stride) fail("n_frames[%d]=%d outside [2, f_stride]", u, n_frames[u]);
    if (y_length[u] < 1 || y_length[u] > y_stride) fail("y_length[%d]=%d outside [1, y_stride]", u, y_length[u]);
    max_y = std::max(max_y, y_length[u]);
  }
  SynthRows rows;
  rows.f0 = d_f0; rows.sp = d_sp; rows.ap = d_ap;
  rows.row_stride = fft_size / 2 + 1; rows.f0_stride = 1;
  rows.first_row.resize(n_utt);
  for (int u = 0; u < n_utt; ++u) rows.first_row[u] = (long long)u * f_stride;
  synthesize_rows(c, n_utt, fs, frame_period, fft_size, n_frames, rows, y_length, y_stride, max_y, d_y);
}

// ---------------------------------------------------------------------------
// Result packing for the multi-GPU exchange (exchange.hip)
// ---------------------------------------------------------------------------
static void run_pack(WorldHipContext *c, bool unpack, int n_utt, const int *n_frames, int f_stride, int nb,
                     const double *d_tpos, const double *d_f0, const double *d_sp, const double *d_ap, long long first_row,
                     double *d_block) {
  if (n_utt <= 0) fail("n_utt must be positive");
  if (!n_frames || !d_tpos || !d_f0 || !d_sp || !d_ap || !d_block) fail("null buffer");
  if (nb < 1 || first_row < 0) fail("bad record shape");
  const int max_frames = max_frame_count(n_frames, n_utt, f_stride);
  const std::vector<int> off = record_rows(n_frames, n_utt, first_row);
  if (max_frames == 0) return;
  begin_stage(c, [](Arena &) {});
  PackArgs a;
  a.n_utt = n_utt; a.f_stride = f_stride; a.nb = nb;
  a.n_frames = upload(c, n_frames, n_utt);
  a.row_offset = upload(c, off);
  a.tpos = d_tpos; a.f0 = d_f0; a.sp = d_sp; a.ap = d_ap; a.block = d_block;
  launch_pack_rows(a, max_frames, unpack, c->stream);
}

// ---------------------------------------------------------------------------
// CheapTrick, then D4C, of one batch.  (Measured in round 3: CheapTrick on a second stream of the context beside D4C --
// they are independent given F0 -- gains nothing: d4c_frame fills the chip by itself, a lone job stayed at 1.11 ms, and
// twelve jobs in flight dropped from 3.67 to 3.11 M frames/s with 24 streams contending for the hardware queues.)
// ---------------------------------------------------------------------------
static void run_spectral_stages(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                                const int *n_frames, int f_stride, const double *d_tpos, const double *d_f0,
                                const CheapTrickOption *copt, const D4COption *dopt, double *d_sp, double *d_ap,
                                const RowLayout &lay_sp, const RowLayout &lay_ap) {
  open_uploads(c);                                          // ONE upload section for both stages' small arrays
  int max_ct = 0, max_d4c = 0;
  CtParams cp = setup_cheaptrick(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, copt, d_sp, lay_sp,
                                 &max_ct);
  D4cParams dp = setup_d4c(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, copt->fft_size, dopt, d_ap,
                           lay_ap, &max_d4c);
  spectral_workspace(c, &cp, &dp, x_length, n_frames);
  // both stages' first offset scans depend on F0 alone: one launch serves both (two 1-workgroup kernels per job were two
  // of the narrow launches the twelve-jobs-in-flight mode pays 10-25 us apiece for)
  if (!cp.skip_prepare && !dp.skip_prepare) {
    launch_spectral_prepare(cp, dp, std::max(max_ct, max_d4c), c->stream);
    cp.skip_prepare = 1; dp.skip_prepare |= kD4cSkipScan;
  }
  launch_cheaptrick(cp, max_ct, c->stream);
  launch_d4c(dp, max_d4c, c->stream);
}

// Harvest + CheapTrick + D4C of one batch into the dense arrays of the *_batch calls (world_hip_analyze_batch)
static void run_analyze_dense(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                              const HarvestOption *hopt, const CheapTrickOption *copt, const D4COption *dopt, int f_stride,
                              double *d_tpos, double *d_f0, double *d_sp, double *d_ap) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  std::vector<int> nf(n_utt);
  for (int u = 0; u < n_utt; ++u) {
    nf[u] = frame_count(fs, x_length[u], hopt->frame_period);
    if (nf[u] > f_stride) fail("f_stride %d too small for %d frames", f_stride, nf[u]);
  }
  run_harvest(c, n_utt, fs, d_x, x_stride, x_length, hopt, f_stride, d_tpos, d_f0);
  run_spectral_stages(c, n_utt, fs, d_x, x_stride, x_length, nf.data(), f_stride, d_tpos, d_f0, copt, dopt, d_sp, d_ap,
                      RowLayout(), RowLayout());
}

// ---------------------------------------------------------------------------
// Harvest + CheapTrick + D4C of one batch straight into packed records (include/world_hip.h: world_hip_analyze_packed)
// ---------------------------------------------------------------------------
// code_ndim > 0: CODED records [tpos, f0, mel-cepstrum[code_ndim], band aperiodicity[nap]] (cols = coded_cols): the frame
// kernels code their own rows (cheaptrick.hip: ct_frame's coded epilogue; d4c.hip: d4c_finish) -- no dense row exists anywhere
static void analyze_into_records(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                                 const HarvestOption *hopt, const CheapTrickOption *copt, const D4COption *dopt,
                                 long long first_row, double *d_block, int cols, int code_ndim) {
  const int nb = copt->fft_size / 2 + 1;
  // the record width names the wire format: 2 + 2 nb doubles = f64 spectra, 2 + nb doubles = f32 spectra
  const int wire = code_ndim == 0 && cols == record_cols(copt->fft_size, 1) ? 1 : 0;
  std::vector<int> nf(n_utt);
  int f_stride = 1;
  for (int u = 0; u < n_utt; ++u) {
    nf[u] = frame_count(fs, x_length[u], hopt->frame_period);
    f_stride = std::max(f_stride, nf[u]);
  }
  const std::vector<int> rows = record_rows(nf.data(), n_utt, first_row);
  // the time axis and F0 stay dense ([n_utt][f_stride]: what CheapTrick and D4C read); they outlive the stages' arenas
  const size_t fr = (size_t)n_utt * f_stride;
  if (c->pk_cap < 2 * fr) {
    devrt::sync(c->stream);
    put_table(c, c->d_pk, 2 * fr + fr / 4);
    c->pk_cap = 2 * fr + fr / 4;
  }
  devrt::dpoison(c->d_pk, sizeof(double) * c->pk_cap, c->stream);
  double *d_tpos = c->d_pk, *d_f0 = c->d_pk + fr;
  run_harvest(c, n_utt, fs, d_x, x_stride, x_length, hopt, f_stride, d_tpos, d_f0);
  RowLayout lay_sp, lay_ap;
  lay_sp.rows = lay_ap.rows = rows.data(); lay_sp.stride = lay_ap.stride = (size_t)cols;
  lay_sp.f32 = lay_ap.f32 = wire == 1;
  const size_t elem = wire == 1 ? sizeof(float) : sizeof(double);
  lay_sp.col_bytes = 2 * sizeof(double);
  lay_ap.col_bytes = 2 * sizeof(double) + (code_ndim > 0 ? sizeof(double) * code_ndim : elem * nb);
  lay_ap.rec = d_block;
  if (code_ndim > 0) {
    const CodecTables &t = codec_tables(c, fs, copt->fft_size);
    lay_sp.code_dims = code_ndim;
    lay_sp.code_knot = t.d_knot_code; lay_sp.code_frac = t.d_frac_code; lay_sp.code_w_re = t.d_wc_re; lay_sp.code_w_im = t.d_wc_im;
    lay_ap.code_dims = number_of_aperiodicities(fs);
  }
  run_spectral_stages(c, n_utt, fs, d_x, x_stride, x_length, nf.data(), f_stride, d_tpos, d_f0, copt, dopt, d_block,
                      d_block, lay_sp, lay_ap);
}
static void run_analyze_packed(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                               const HarvestOption *hopt, const CheapTrickOption *copt, const D4COption *dopt,
                               long long first_row, double *d_block, int cols) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  const int wire = cols == record_cols(copt->fft_size, 1) ? 1 : 0;
  if (cols != record_cols(copt->fft_size, wire))
    fail("analyze_packed: %d columns, fft_size %d needs %d (f64 records) or %d (f32 spectra)", cols, copt->fft_size,
         record_cols(copt->fft_size, 0), record_cols(copt->fft_size, 1));
  if (!d_block) fail("analyze_packed: null block");
  if (first_row < 0) fail("analyze_packed: negative first_row");
  analyze_into_records(c, n_utt, fs, d_x, x_stride, x_length, hopt, copt, dopt, first_row, d_block, cols, 0);
}

// ---------------------------------------------------------------------------
// Harvest + CheapTrick + D4C of one batch into CODED records [tpos, f0, mel-cepstrum[ndim], band aperiodicity[nap]]
// (include/world_hip.h: world_hip_analyze_coded; SURVEY.md 8f.1: the coders "fuse onto K6/K8 outputs" and "shrink the
// all-gather and D2H by 10-17x" -- 31 x at 48 kHz with 60 coefficients: 536 instead of 16 416 bytes per frame).
// CodeSpectralEnvelope / CodeAperiodicity (reference src/codec.cpp:217-236, 268-297) of exactly the analysis a dense call
// returns, computed by the kernels that produce the rows: ct_frame turns its log envelope into the mel-cepstrum in the LDS
// it already holds, d4c_finish evaluates the two bins each band value interpolates.  (Round 5 wrote full 16 KB records to a
// staging block and ran the stand-alone coders over it: one extra HBM write + read per frame and two more launches.)
// ---------------------------------------------------------------------------
static int coded_cols(int fs, int ndim) { return 2 + ndim + number_of_aperiodicities(fs); }
static void run_analyze_coded(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                              const HarvestOption *hopt, const CheapTrickOption *copt, const D4COption *dopt, int ndim,
                              long long first_row, double *d_block, int cols) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  if (!d_block) fail("analyze_coded: null block");
  if (first_row < 0) fail("analyze_coded: negative first_row");
  const int nap = number_of_aperiodicities(fs);
  if (nap < 1) fail("analyze_coded: fs=%d has no aperiodicity band", fs);
  if (3000.0 * nap > fs / 2.0) fail("analyze_coded: band centre beyond fs/2");
  if (ndim < 1 || ndim > copt->fft_size / 4 + 1) fail("analyze_coded: number_of_dimensions %d outside [1, fft_size/4+1]", ndim);
  if (cols != coded_cols(fs, ndim)) fail("analyze_coded: %d columns, %d coefficients at fs=%d need %d", cols, ndim, fs, coded_cols(fs, ndim));
  analyze_into_records(c, n_utt, fs, d_x, x_stride, x_length, hopt, copt, dopt, first_row, d_block, cols, ndim);
}

// ---------------------------------------------------------------------------
// Synthesis straight from records (include/world_hip.h: world_hip_synthesis_records): the mirror image of analyze_packed /
// analyze_coded.  wire 0: the f64 records are read in place through SynthParams' row addressing, nothing is staged.
// wire 1 / 2: sy_stage_records (codec.hip) turns every record into dense f64 rows once -- F0 [rows], sp and ap [rows][nb],
// the utterances back to back -- carved at the bottom of the arena and held there while the synthesis stage carves above
// them (hold_at_floor).
// ---------------------------------------------------------------------------
static void run_synthesis_records(WorldHipContext *c, int n_utt, int fs, double frame_period, int fft_size,
                                  const int *n_frames, long long first_row, const double *d_block, int cols, int wire,
                                  int ndim, const int *y_length, int y_stride, double *d_y) {
  if (n_utt <= 0) fail("n_utt must be positive");
  if (fs <= 0 || frame_period <= 0) fail("fs and frame_period must be positive");
  if (!d_block) fail("synthesis_records: null block");
  if (!d_y || !n_frames || !y_length) fail("null buffer");
  if (first_row < 0) fail("synthesis_records: negative first_row");
  if (wire < 0 || wire > 2) fail("synthesis_records: wire %d (0: f64 records, 1: f32 records, 2: coded records)", wire);
  refuse_shape_limit(15, fs, fft_size);                                 // world_hip_check_shape's rule
  const int lg = ilog2_exact(fft_size), nb = fft_size / 2 + 1;
  int nap = 0;
  if (wire == 2) {                                                      // what the decoders refuse (run_codec)
    nap = number_of_aperiodicities(fs);
    if (nap < 1) fail("synthesis_records: fs=%d has no aperiodicity band (needs fs >= 12 kHz)", fs);
    if (3000.0 * nap > fs / 2.0) fail("synthesis_records: band centre beyond fs/2");
    if (ndim < 1 || ndim > fft_size / 4 + 1)
      fail("synthesis_records: number_of_dimensions %d outside [1, fft_size/4+1]", ndim);
    if (cols != coded_cols(fs, ndim))
      fail("synthesis_records: %d columns, %d coefficients at fs=%d need %d", cols, ndim, fs, coded_cols(fs, ndim));
  } else if (cols != record_cols(fft_size, wire)) {
    fail("synthesis_records: %d columns, wire %d at fft_size %d needs %d", cols, wire, fft_size, record_cols(fft_size, wire));
  }
  long long total = 0;
  int max_y = 0, max_frames = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (n_frames[u] < 2) fail("n_frames[%d]=%d: synthesis needs 2 frames", u, n_frames[u]);
    if (y_length[u] < 1 || y_length[u] > y_stride) fail("y_length[%d]=%d outside [1, y_stride]", u, y_length[u]);
    total += n_frames[u];
    max_y = std::max(max_y, y_length[u]);
    max_frames = std::max(max_frames, n_frames[u]);
  }
  const std::vector<int> src = record_rows(n_frames, n_utt, first_row), dst = record_rows(n_frames, n_utt, 0);
  SynthRows rows;
  if (wire == 0) {                                                      // [tpos, f0, sp[nb], ap[nb]] in place
    rows.f0 = d_block + 1; rows.sp = d_block + 2; rows.ap = d_block + 2 + nb;
    rows.first_row.assign(src.begin(), src.end()); rows.row_stride = rows.f0_stride = (size_t)cols;
    synthesize_rows(c, n_utt, fs, frame_period, fft_size, n_frames, rows, y_length, y_stride, max_y, d_y);
    return;
  }
  StageRecordsParams sp;
  sp.n_utt = n_utt; sp.wire = wire; sp.fft_size = fft_size; sp.lg_md = lg - 1; sp.ndim = ndim; sp.nap = nap;
  sp.block = d_block; sp.cols = cols;
  sp.knot_sp = sp.knot_ap = nullptr; sp.frac_sp = sp.frac_ap = sp.w_re = sp.w_im = nullptr;
  auto carve = [&](Arena &a) {
    sp.f0 = a.take<double>((size_t)total);
    sp.sp = a.take<double>((size_t)total * nb); sp.ap = a.take<double>((size_t)total * nb);
  };
  hold_at_floor(c, "synthesis_records", carve, [&] {
    open_uploads(c);
    if (wire == 2) {
      const CodecTables &t = codec_tables(c, fs, fft_size);
      sp.knot_sp = t.d_knot_dec; sp.frac_sp = t.d_frac_dec; sp.w_re = t.d_wd_re; sp.w_im = t.d_wd_im;
      sp.knot_ap = t.d_knot_ap; sp.frac_ap = t.d_frac_ap;
    }
    sp.n_frames = upload(c, n_frames, n_utt);
    sp.src_row = upload(c, src); sp.dst_row = upload(c, dst);
    sp.tab = c->tab;
    launch_stage_records(sp, max_frames, c->stream);
    rows.f0 = sp.f0; rows.sp = sp.sp; rows.ap = sp.ap;
    rows.first_row.assign(dst.begin(), dst.end()); rows.row_stride = (size_t)nb; rows.f0_stride = 1;
    synthesize_rows(c, n_utt, fs, frame_period, fft_size, n_frames, rows, y_length, y_stride, max_y, d_y);
  });
}

// ---------------------------------------------------------------------------
// CheapTrick + D4C of the frames [frame_lo, frame_hi) of every utterance, given F0, straight into packed records
// (include/world_hip.h: world_hip_spectral_packed_range): the unit of frame-level sharding ("CheapTrick /
// D4C only, F0 broadcast") and of the drop-in calls' download that overlaps the kernels.
// ---------------------------------------------------------------------------
static void run_spectral_packed_range(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                                      const int *n_frames, int f_stride, const double *d_tpos, const double *d_f0,
                                      const CheapTrickOption *copt, const D4COption *dopt, int frame_lo, int frame_hi,
                                      long long first_row, double *d_block, int cols, bool reuse_offsets) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  if (!n_frames || !d_tpos || !d_f0 || !d_block) fail("null buffer");
  if (frame_lo < 0 || frame_hi < frame_lo || first_row < 0) fail("bad frame range [%d, %d) or first row", frame_lo, frame_hi);
  const int nb = copt->fft_size / 2 + 1;
  const int wire = cols == record_cols(copt->fft_size, 1) ? 1 : 0;
  if (cols != record_cols(copt->fft_size, wire))
    fail("spectral_packed_range: %d columns, fft_size %d needs %d (f64 records) or %d (f32 spectra)", cols, copt->fft_size,
         record_cols(copt->fft_size, 0), record_cols(copt->fft_size, 1));
  // utterance u's frame f goes to row rows[u] + f: its range's first frame lands where the previous utterance's range ended
  max_frame_count(n_frames, n_utt, f_stride);
  std::vector<int> rows(n_utt);
  long long row = first_row;
  for (int u = 0; u < n_utt; ++u) {
    const int lo = std::min(frame_lo, n_frames[u]), hi = std::min(frame_hi, n_frames[u]);
    if (row - lo < -0x7FFFFFFFll || row + (hi - lo) > 0x7FFFFFFFll) fail("block exceeds 2^31 records");
    rows[u] = static_cast<int>(row - lo);
    row += hi - lo;
  }
  RowLayout lay_sp, lay_ap;
  lay_sp.rows = lay_ap.rows = rows.data(); lay_sp.stride = lay_ap.stride = (size_t)cols;
  lay_sp.f32 = lay_ap.f32 = wire == 1;
  const size_t elem = wire == 1 ? sizeof(float) : sizeof(double);
  lay_sp.col_bytes = 2 * sizeof(double); lay_ap.col_bytes = 2 * sizeof(double) + elem * nb;
  lay_ap.rec = d_block;
  lay_sp.frame_lo = lay_ap.frame_lo = frame_lo; lay_sp.frame_hi = lay_ap.frame_hi = frame_hi;
  lay_sp.skip_prepare = lay_ap.skip_prepare = reuse_offsets;
  run_spectral_stages(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, copt, dopt, d_block, d_block,
                      lay_sp, lay_ap);
}

// ---------------------------------------------------------------------------
// Shape limits of the GPU path (the reference has none: it allocates whatever fs asks for).  One function states them,
// the stages and world_hip_check_shape ask it, and the drop-in entries ask it BEFORE any upload or launch.
// what: bit 0 StoneMask, bit 1 CheapTrick (needs fft_size), bit 2 D4C, bit 3 Synthesis and the real-time synthesiser
// (needs fft_size).  Returns an empty string or the reason.
//
// The pair (fs, fft_size).  The reference sizes its per-frame buffers by fft_size alone and fills them by fs:
//  * CheapTrick analyses every frame at or below its floor 3 fs / (fft_size - 3) -- every unvoiced frame -- at the
//    500 Hz default, with a window of 2 round(1.5 fs / 500) + 1 samples written into the fft_size-long waveform
//    (cheaptrick.cpp:115-137, :218).  A voiced frame above the floor has a window of at most fft_size - 2.
//  * Synthesis places the pulses of unvoiced stretches 500 Hz apart and fills noise_size = the distance to the next pulse
//    samples of the fft_size-long waveform (synthesis.cpp:19-31, :307, :371; synthesisrealtime.cpp likewise).  The phase
//    advances by 2 pi 500 / fs per sample, so two such pulses are floor(fs / 500) or one more samples apart (also where
//    fs / 500 is whole: the accumulated phase reaches 2 pi only to rounding).
// Beyond either the reference writes past its buffers; here the pair is refused.
// ---------------------------------------------------------------------------
static int ct_default_window(int fs) { return 2 * static_cast<int>(1.5 * fs / 500.0 + 0.5) + 1; }   // (matlab_round, positive)
static int synth_default_spacing(int fs) { return fs / 500 + 1; }
static int smallest_fft_for(int need) {
  int n = 128;
  while (n < need && n < (1 << 30)) n *= 2;
  return n;
}

// a stage's fft_size: a power of two in 128..8192 (`why`) that holds the `need` samples the 500 Hz default asks for at fs
// (`needs`: a format with one %d for that count)
static std::string fft_size_limit(const char *stage, const char *why, int fs, int fft_size, int need, const char *needs) {
  char msg[320], count[96];
  int lg = 0;
  while (lg < 30 && (1 << lg) < fft_size) ++lg;
  if (fft_size < 1 || (1 << lg) != fft_size || lg < 7 || lg > 13) {
    snprintf(msg, sizeof msg, "%s: fft_size %d unsupported (a power of two, 128..8192: %s)", stage, fft_size, why);
    return msg;
  }
  if (need > fft_size) {
    snprintf(count, sizeof count, needs, need);
    snprintf(msg, sizeof msg, "%s: fft_size %d is too small for fs=%d: %s (the reference writes past its buffer there); the smallest fft_size for this fs is %d",
             stage, fft_size, fs, count, smallest_fft_for(need));
    return msg;
  }
  return std::string();
}

static std::string shape_limit(int what, int fs, int fft_size) {
  char msg[256];
  if (fs <= 0) return "fs must be positive";
  if (what & 1) {
    const int win_cap = 2 * static_cast<int>(1.5 * fs / 40.0 + 1.0) + 4;
    if (stonemask_lds_bytes(win_cap) > 160 * 1024) {
      snprintf(msg, sizeof msg, "StoneMask: fs=%d needs a %d-sample window, more LDS than a CU has; fs <= 240 kHz supported", fs, win_cap);
      return msg;
    }
  }
  if (what & 2) {
    const std::string r = fft_size_limit("CheapTrick", "one frame must fit LDS; fs <= 192 kHz at the default f0 floor", fs, fft_size,
                                         ct_default_window(fs), "an unvoiced frame's 500 Hz window has %d samples");
    if (!r.empty()) return r;
  }
  if (what & 8) {
    const std::string r = fft_size_limit("Synthesis", "one pulse's transform must fit LDS", fs, fft_size,
                                         synth_default_spacing(fs), "unvoiced pulses lie up to %d samples apart");
    if (!r.empty()) return r;
  }
  if (what & 4) {
    const int fft_d4c = std::max(d4c_internal_fft(fs), static_cast<int>(pow(2.0, 1.0 + static_cast<int>(log(3.0 * fs / 40.0 + 1) / kLog2))));
    if (fft_d4c > 16384) {
      snprintf(msg, sizeof msg, "D4C: fs=%d needs an internal FFT of %d > 16384 points (LDS budget); fs <= 192 kHz supported", fs, fft_d4c);
      return msg;
    }
    if (fs < 15800) {
      snprintf(msg, sizeof msg, "D4C: fs=%d is below the 15.8 kHz the reference's LoveTrain band edges require (the reference reads out of bounds there)", fs);
      return msg;
    }
  }
  return std::string();
}

// ---------------------------------------------------------------------------
// Parameter modification between analysis and synthesis (reference test/test.cpp:221-258, ParameterModification) and the
// whole analyse -> modify -> synthesise chain in one call (include/world_hip.h: world_hip_modify_batch,
// world_hip_resynthesize_batch).  The kernels are codec.hip's modify_warp_sp and modify_f0.
// ---------------------------------------------------------------------------
// every value of every utterance's modification checked before any GPU work; fft_size = 0: the rows are not modified (the
// fill bound does not apply)
static void check_modifications(const WorldHipModification *mods, int n_utt, int fft_size) {
  if (!mods) return;
  for (int u = 0; u < n_utt; ++u) {
    const WorldHipModification &m = mods[u];
    if (!std::isfinite(m.f0_scale) || m.f0_scale < 0.0) fail("modification %d: f0_scale %g must be finite and >= 0", u, m.f0_scale);
    if (!std::isfinite(m.formant_shift) || !(m.formant_shift > 0.0))
      fail("modification %d: formant_shift %g must be finite and > 0", u, m.formant_shift);
    if (fft_size > 0 && !(fft_size / 2.0 * m.formant_shift >= 1.0))
      fail("modification %d: formant_shift %g leaves no bin below fft_size/2 * ratio to fill from (fft_size %d)", u,
           m.formant_shift, fft_size);
    if (m.convert_log_f0 != 0 && m.convert_log_f0 != 1) fail("modification %d: convert_log_f0 must be 0 or 1", u);
    if (m.convert_log_f0 && !std::isfinite(m.log_f0_mean)) fail("modification %d: log_f0_mean %g is not finite", u, m.log_f0_mean);
    if (m.convert_log_f0 && (!std::isfinite(m.log_f0_std) || m.log_f0_std < 0.0))
      fail("modification %d: log_f0_std %g must be finite and >= 0", u, m.log_f0_std);
  }
}

// f0 and sp independently optional (both pointers of a pair, or neither); in == out allowed for each
static void run_modify(WorldHipContext *c, int n_utt, int fs, int fft_size, const int *n_frames, int f_stride,
                       const WorldHipModification *mods, const double *d_f0_in, double *d_f0_out, const double *d_sp_in,
                       double *d_sp_out) {
  if (n_utt <= 0) fail("n_utt must be positive");
  if (!n_frames) fail("null n_frames");
  if (!d_f0_in != !d_f0_out) fail("modify: give both d_f0_in and d_f0_out, or neither");
  if (!d_sp_in != !d_sp_out) fail("modify: give both d_sp_in and d_sp_out, or neither");
  const bool with_sp = d_sp_in != nullptr;
  if (with_sp) {
    if (fs <= 0) fail("fs must be positive");
    const int lg = ilog2_exact(fft_size);
    if (lg < 7 || lg > 13) fail("modify: fft_size %d unsupported (128..8192)", fft_size);
  }
  check_modifications(mods, n_utt, with_sp ? fft_size : 0);
  const int max_frames = max_frame_count(n_frames, n_utt, f_stride);
  std::vector<double> ratio(n_utt, 1.0), scale(n_utt, 1.0), target(2 * (size_t)n_utt, 0.0);
  std::vector<int> convert(n_utt, 0);
  bool warp = with_sp && d_sp_in != d_sp_out, map = d_f0_in && d_f0_in != d_f0_out;   // out-of-place always writes
  for (int u = 0; mods && u < n_utt; ++u) {
    ratio[u] = mods[u].formant_shift; scale[u] = mods[u].f0_scale; convert[u] = mods[u].convert_log_f0;
    target[2 * u] = mods[u].log_f0_mean; target[2 * u + 1] = mods[u].log_f0_std;
    warp |= with_sp && ratio[u] != 1.0;
    map |= d_f0_in && (scale[u] != 1.0 || convert[u] != 0);
  }
  if (max_frames == 0 || (!warp && !map)) return;
  open_uploads(c);                                          // (the stage uses no workspace: prepared offsets stay valid)
  ModifyParams p;
  p.n_utt = n_utt; p.f_stride = f_stride; p.fs = fs; p.fft_size = fft_size;
  p.n_frames = upload(c, n_frames, n_utt);
  p.ratio = upload(c, ratio); p.sp_in = d_sp_in; p.sp_out = d_sp_out;
  p.f0_scale = upload(c, scale); p.convert = upload(c, convert); p.target = upload(c, target);
  p.f0_in = d_f0_in; p.f0_out = d_f0_out; p.stats = nullptr;
  if (warp) launch_modify_warp_sp(p, max_frames, c->stream);
  if (map) launch_modify_f0(p, c->stream);
}

static void run_f0_statistics(WorldHipContext *c, int n_utt, const int *n_frames, int f_stride, const double *d_f0,
                              double *d_stats) {
  if (n_utt <= 0) fail("n_utt must be positive");
  if (!n_frames || !d_f0 || !d_stats) fail("null buffer");
  max_frame_count(n_frames, n_utt, f_stride);
  open_uploads(c);
  ModifyParams p;
  p.n_utt = n_utt; p.f_stride = f_stride; p.fs = 0; p.fft_size = 0;
  p.n_frames = upload(c, n_frames, n_utt);
  p.ratio = nullptr; p.sp_in = nullptr; p.sp_out = nullptr;
  p.convert = upload(c, std::vector<int>(n_utt, 0));
  p.f0_scale = nullptr; p.target = nullptr;
  p.f0_in = d_f0; p.f0_out = nullptr; p.stats = d_stats;
  launch_modify_f0(p, c->stream);
}

static int resynthesis_length(int fs, int n_frames, double frame_period, double time_scale) {   // test.cpp:302-303
  return static_cast<int>((n_frames - 1) * frame_period * time_scale / 1000.0 * fs) + 1;
}

// what the resynthesis calls refuse first: the batch, a null option, a HarvestOption no analysis could run with
static void check_analysis_input(int n_utt, int fs, const void *d_x, int x_stride, const int *x_length, const HarvestOption *hopt,
                                 const CheapTrickOption *copt, const D4COption *dopt) {
  check_batch(n_utt, fs, d_x, x_stride, x_length);
  if (!hopt || !copt || !dopt) fail("null option");
  if (!(hopt->f0_floor > 0) || !(hopt->f0_ceil > hopt->f0_floor) || !(hopt->frame_period > 0) ||
      !std::isfinite(hopt->frame_period) || !std::isfinite(hopt->f0_ceil))
    fail("bad HarvestOption");
}

// Harvest -> CheapTrick + D4C -> modification -> Synthesis at frame_period * time_scale.  tpos, f0, sp and ap are carved at
// the bottom of the arena and held there while the stages carve above them (hold_at_floor).
static void run_resynthesis(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                            const HarvestOption *hopt, const CheapTrickOption *copt, const D4COption *dopt,
                            const WorldHipModification *mods, double time_scale, const int *y_length, int y_stride,
                            double *d_y) {
  check_analysis_input(n_utt, fs, d_x, x_stride, x_length, hopt, copt, dopt);
  if (!std::isfinite(time_scale) || !(time_scale > 0.0)) fail("resynthesize: time_scale %g must be finite and > 0", time_scale);
  if (!y_length || !d_y) fail("null buffer");
  const int fft_size = copt->fft_size;
  refuse_shape_limit(14, fs, fft_size);
  check_modifications(mods, n_utt, fft_size);
  std::vector<int> nf(n_utt);
  int f_stride = 1;
  for (int u = 0; u < n_utt; ++u) {
    nf[u] = frame_count(fs, x_length[u], hopt->frame_period);
    if (nf[u] < 2) fail("resynthesize: utterance %d has %d frame(s); synthesis needs 2", u, nf[u]);
    if (y_length[u] < 1 || y_length[u] > y_stride) fail("y_length[%d]=%d outside [1, y_stride]", u, y_length[u]);
    f_stride = std::max(f_stride, nf[u]);
  }
  const size_t fr = (size_t)n_utt * f_stride, nb = fft_size / 2 + 1;
  double *tpos = nullptr, *f0 = nullptr, *sp = nullptr, *ap = nullptr;
  auto carve = [&](Arena &a) {
    tpos = a.take<double>(fr); f0 = a.take<double>(fr);
    sp = a.take<double>(fr * nb); ap = a.take<double>(fr * nb);
  };
  hold_at_floor(c, "resynthesize", carve, [&] {
    run_analyze_dense(c, n_utt, fs, d_x, x_stride, x_length, hopt, copt, dopt, f_stride, tpos, f0, sp, ap);
    run_modify(c, n_utt, fs, fft_size, nf.data(), f_stride, mods, f0, f0, sp, sp);
    run_synthesis(c, n_utt, fs, hopt->frame_period * time_scale, fft_size, nf.data(), f_stride, f0, sp, ap, y_length, y_stride,
                  d_y);
  });
}

// Frame-wise modification behind a time map (include/world_hip.h: world_hip_modify_frames_batch; codec.hip's
// modify_frames_sp / _ap / _f0).  Everything the host can know is checked before any GPU work; the curves' values live on
// the device and are made harmless in the kernels.  f0, sp and ap independently optional, as in run_modify.
static void run_modify_frames(WorldHipContext *c, int n_utt, int fs, int fft_size, const int *n_frames, int f_stride,
                              const int *n_out, int o_stride, const WorldHipModification *mods,
                              const WorldHipFrameCurves *curves, const double *d_f0_in, double *d_f0_out,
                              const double *d_sp_in, double *d_sp_out, const double *d_ap_in, double *d_ap_out) {
  if (n_utt <= 0) fail("n_utt must be positive");
  if (!n_frames || !n_out) fail("null n_frames / n_out");
  if (!d_f0_in != !d_f0_out) fail("modify_frames: give both d_f0_in and d_f0_out, or neither");
  if (!d_sp_in != !d_sp_out) fail("modify_frames: give both d_sp_in and d_sp_out, or neither");
  if (!d_ap_in != !d_ap_out) fail("modify_frames: give both d_ap_in and d_ap_out, or neither");
  const bool with_sp = d_sp_in != nullptr, with_ap = d_ap_in != nullptr, with_f0 = d_f0_in != nullptr;
  if (with_sp || with_ap) {
    if (fs <= 0) fail("fs must be positive");
    const int lg = ilog2_exact(fft_size);
    if (lg < 7 || lg > 13) fail("modify_frames: fft_size %d unsupported (128..8192)", fft_size);
  }
  check_modifications(mods, n_utt, with_sp ? fft_size : 0);
  max_frame_count(n_frames, n_utt, f_stride);
  const WorldHipFrameCurves none = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const WorldHipFrameCurves &cv = curves ? *curves : none;
  const bool in_place = (with_f0 && d_f0_in == d_f0_out) || (with_sp && d_sp_in == d_sp_out) || (with_ap && d_ap_in == d_ap_out);
  if (cv.d_time_map && in_place) fail("modify_frames: a time map needs output arrays of their own (in == out)");
  if (in_place && o_stride != f_stride) fail("modify_frames: in place needs o_stride == f_stride");
  int max_out = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (n_out[u] < 1 || n_out[u] > o_stride) fail("n_out[%d]=%d outside [1, o_stride=%d]", u, n_out[u], o_stride);
    if (cv.d_time_map && n_frames[u] < 1) fail("modify_frames: utterance %d has no source frame to read", u);
    if (!cv.d_time_map && n_out[u] != n_frames[u])
      fail("modify_frames: utterance %d: without a time map n_out (%d) must equal n_frames (%d)", u, n_out[u], n_frames[u]);
    max_out = std::max(max_out, n_out[u]);
  }
  if (!with_sp && !with_ap && !with_f0) return;
  std::vector<double> ratio(n_utt, 1.0), scale(n_utt, 1.0), one(n_utt, 1.0), target(2 * (size_t)n_utt, 0.0);
  std::vector<int> convert(n_utt, 0);
  bool converts = false;
  for (int u = 0; mods && u < n_utt; ++u) {
    ratio[u] = mods[u].formant_shift; scale[u] = mods[u].f0_scale; convert[u] = mods[u].convert_log_f0;
    target[2 * u] = mods[u].log_f0_mean; target[2 * u + 1] = mods[u].log_f0_std;
    converts |= with_f0 && convert[u] != 0;
  }
  // the log-F0 conversion acts on the SOURCE track, before the frames are blended: modify_f0 as it is (scale 1) into a
  // temporary, which modify_frames_f0 then reads
  double *f0_conv = nullptr;
  if (converts)
    begin_stage(c, [&](Arena &a) { f0_conv = a.take<double>((size_t)n_utt * f_stride); });
  else
    open_uploads(c);                                        // (no workspace: prepared offsets stay valid)
  ModifyFramesParams p;
  p.m.n_utt = n_utt; p.m.f_stride = f_stride; p.m.fs = fs; p.m.fft_size = fft_size;
  p.m.n_frames = upload(c, n_frames, n_utt);
  p.m.ratio = upload(c, ratio); p.m.sp_in = d_sp_in; p.m.sp_out = d_sp_out;
  p.m.f0_scale = upload(c, scale); p.m.convert = upload(c, convert); p.m.target = upload(c, target);
  p.m.f0_in = d_f0_in; p.m.f0_out = d_f0_out; p.m.stats = nullptr;
  p.o_stride = o_stride;
  p.n_out = upload(c, n_out, n_utt);
  p.time_map = cv.d_time_map; p.f0_target = cv.d_f0_target; p.f0_scale = cv.d_f0_scale;
  p.formant_shift = cv.d_formant_shift; p.ap_gain = cv.d_ap_gain;
  p.ap_in = d_ap_in; p.ap_out = d_ap_out;
  p.f0_src = d_f0_in;
  if (converts) {
    ModifyParams conv = p.m;
    conv.f0_scale = upload(c, one); conv.f0_out = f0_conv;
    launch_modify_f0(conv, c->stream);
    p.f0_src = f0_conv;
  }
  if (with_sp) launch_modify_frames_sp(p, max_out, c->stream);
  if (with_ap) launch_modify_frames_ap(p, max_out, c->stream);
  if (with_f0) launch_modify_frames_f0(p, max_out, c->stream);
}

// Harvest -> CheapTrick + D4C -> run_modify_frames -> Synthesis at the analysis frame period.  As run_resynthesis, with
// the n_out modified frames held at the bottom of the arena beside the analysis they are made from.
static void run_resynthesis_frames(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                                   const HarvestOption *hopt, const CheapTrickOption *copt, const D4COption *dopt,
                                   const WorldHipModification *mods, const WorldHipFrameCurves *curves, const int *n_out,
                                   int o_stride, const int *y_length, int y_stride, double *d_y) {
  check_analysis_input(n_utt, fs, d_x, x_stride, x_length, hopt, copt, dopt);
  if (!n_out || !y_length || !d_y) fail("null buffer");
  const int fft_size = copt->fft_size;
  refuse_shape_limit(14, fs, fft_size);
  check_modifications(mods, n_utt, fft_size);
  const bool mapped = curves && curves->d_time_map;
  std::vector<int> nf(n_utt);
  int f_stride = 1;
  for (int u = 0; u < n_utt; ++u) {
    nf[u] = frame_count(fs, x_length[u], hopt->frame_period);
    if (nf[u] < 2) fail("resynthesize_frames: utterance %d has %d frame(s); synthesis needs 2", u, nf[u]);
    if (n_out[u] < 2 || n_out[u] > o_stride) fail("resynthesize_frames: n_out[%d]=%d outside [2, o_stride=%d]", u, n_out[u], o_stride);
    if (!mapped && n_out[u] != nf[u])
      fail("resynthesize_frames: utterance %d: without a time map n_out must equal its %d frames (n_out %d)", u, nf[u], n_out[u]);
    if (y_length[u] != resynthesis_length(fs, n_out[u], hopt->frame_period, 1.0) || y_length[u] > y_stride)
      fail("y_length[%d]=%d is not the length of %d frames within y_stride=%d", u, y_length[u], n_out[u], y_stride);
    f_stride = std::max(f_stride, nf[u]);
  }
  const size_t fr = (size_t)n_utt * f_stride, fo = (size_t)n_utt * o_stride, nb = fft_size / 2 + 1;
  double *tpos = nullptr, *f0 = nullptr, *sp = nullptr, *ap = nullptr, *f0m = nullptr, *spm = nullptr, *apm = nullptr;
  auto carve = [&](Arena &a) {
    tpos = a.take<double>(fr); f0 = a.take<double>(fr);
    sp = a.take<double>(fr * nb); ap = a.take<double>(fr * nb);
    f0m = a.take<double>(fo); spm = a.take<double>(fo * nb); apm = a.take<double>(fo * nb);
  };
  hold_at_floor(c, "resynthesize_frames", carve, [&] {
    run_analyze_dense(c, n_utt, fs, d_x, x_stride, x_length, hopt, copt, dopt, f_stride, tpos, f0, sp, ap);
    run_modify_frames(c, n_utt, fs, fft_size, nf.data(), f_stride, n_out, o_stride, mods, curves, f0, f0m, sp, spm, ap, apm);
    run_synthesis(c, n_utt, fs, hopt->frame_period, fft_size, n_out, o_stride, f0m, spm, apm, y_length, y_stride, d_y);
  });
}

// Alignment of pairs of frame rows by dynamic time warping (include/world_hip.h: world_hip_align_batch; align.inc).
// Everything the host can know is refused before any GPU work.  The pairs are walked in groups of at most kAlignCells
// cells, so the workspace is 9 bytes per cell (the cost and the predecessor code) of the largest group, never more than
// 9 * kAlignCells bytes (+ 8 per pair for D), whatever the batch: the backward walk of a pair, n_a + n_b - 1 <= n_a n_b
// entries of 8 bytes, is written over the pair's own costs, which are dead once align_dp has run.
// Time is another matter: a pair takes n_a + n_b - 1 serial diagonal steps of about 1 us, 16 ms at 8192 x 8192 -- but a
// degenerate 1 x 2^26 pair is within the cell limit too and would keep one CU busy for about a minute (the header says so).
static const long long kAlignCells = 1LL << 26;

static void run_align(WorldHipContext *c, int n_pairs, int n_dims, const double *d_a, const long long *a_row, const int *n_a,
                      int a_row_stride, const double *d_b, const long long *b_row, const int *n_b, int b_row_stride,
                      int p_stride, int *d_path, int *d_path_len, double *d_summary, int map_stride, double *d_map_b,
                      double *d_map_a) {
  if (n_pairs < 1) fail("align: n_pairs must be positive");
  if (!d_a || !d_b || !a_row || !b_row || !n_a || !n_b) fail("align: null input");
  if (n_dims < 1 || n_dims > 256) fail("align: n_dims %d outside [1, 256]", n_dims);
  if (a_row_stride < n_dims || b_row_stride < n_dims)
    fail("align: row strides (%d, %d) below n_dims %d", a_row_stride, b_row_stride, n_dims);
  for (int u = 0; u < n_pairs; ++u) {
    if (n_a[u] < 1 || n_b[u] < 1) fail("align: pair %d has %d x %d frames; each side needs one", u, n_a[u], n_b[u]);
    if (a_row[u] < 0 || b_row[u] < 0) fail("align: pair %d starts at a negative row", u);
    if ((long long)n_a[u] * n_b[u] > kAlignCells)
      fail("align: pair %d has %d x %d cells, more than the %lld of world_hip_align_workspace_cells()", u, n_a[u], n_b[u], kAlignCells);
    if (d_path && (long long)p_stride < (long long)n_a[u] + n_b[u] - 1)
      fail("align: p_stride %d cannot hold pair %d's longest path (%d + %d - 1)", p_stride, u, n_a[u], n_b[u]);
    if (d_map_b && map_stride < n_b[u]) fail("align: map_stride %d below n_b[%d]=%d", map_stride, u, n_b[u]);
    if (d_map_a && map_stride < n_a[u]) fail("align: map_stride %d below n_a[%d]=%d", map_stride, u, n_a[u]);
  }
  if (!d_path && !d_path_len && !d_summary && !d_map_b && !d_map_a) return;
  // groups of consecutive pairs within the cell budget; a pair's place in its group's workspace
  std::vector<long long> cell0(n_pairs);
  std::vector<int> first;                                   // first pair of every group, then n_pairs
  long long cells = 0, max_cells = 0;
  for (int u = 0; u < n_pairs; ++u) {
    const long long own = (long long)n_a[u] * n_b[u];
    if (u == 0 || cells + own > kAlignCells || u - first.back() >= 32768) { first.push_back(u); cells = 0; }
    cell0[u] = cells;
    cells += own;
    max_cells = std::max(max_cells, cells);
  }
  first.push_back(n_pairs);
  AlignParams p;
  begin_stage(c, [&](Arena &a) {
    p.cost = a.take<double>((size_t)max_cells);
    p.code = a.take<unsigned char>((size_t)max_cells);
    p.dist = a.take<double>((size_t)n_pairs);
  });
  p.n_dims = n_dims;
  p.a = d_a; p.b = d_b; p.a_stride = a_row_stride; p.b_stride = b_row_stride;
  p.a_row = upload(c, a_row, n_pairs);
  p.b_row = upload(c, b_row, n_pairs);
  p.n_a = upload(c, n_a, n_pairs);
  p.n_b = upload(c, n_b, n_pairs);
  p.cell0 = upload(c, cell0);
  p.mcd_scale = 10.0 / log(10.0) * sqrt(2.0);
  p.path = d_path; p.p_stride = p_stride; p.path_len = d_path_len; p.summary = d_summary;
  p.map_stride = map_stride; p.map_b = d_map_b; p.map_a = d_map_a;
  for (size_t g = 0; g + 1 < first.size(); ++g) {
    int tiles = 0, shorter = 0;
    for (int u = first[g]; u < first[g + 1]; ++u) {
      tiles = std::max(tiles, align_cost_tiles(n_a[u], n_b[u]));
      shorter = std::max(shorter, std::min(n_a[u], n_b[u]));
    }
    p.first_pair = first[g];
    p.cap = shorter + 1;
    const int pairs = first[g + 1] - first[g];
    launch_align_cost(p, pairs, tiles, c->stream);
    launch_align_dp(p, pairs, c->stream);
    launch_align_path(p, pairs, c->stream);
  }
}

// Morph of two aligned utterances (include/world_hip.h: world_hip_morph_batch; morph.inc).  Everything the host can know
// is refused before any GPU work; the path and the curves live on the device and are made harmless in the kernels.
static int morph_length(int n_a, int n_b, double time_rate) {
#pragma clang fp contract(off)
  if (n_a < 1 || n_b < 1 || !(time_rate >= 0.0 && time_rate <= 1.0)) return -1;
  return static_cast<int>((1.0 - time_rate) * (n_a - 1) + time_rate * (n_b - 1)) + 1;   // (>= 0: the floor)
}

static void run_morph(WorldHipContext *c, int n_pairs, int fs, int fft_size, const int *n_a, int a_stride, const double *d_f0_a,
                      const double *d_sp_a, const double *d_ap_a, const int *n_b, int b_stride, const double *d_f0_b,
                      const double *d_sp_b, const double *d_ap_b, int p_stride, const int *d_path, const int *d_path_len,
                      const WorldHipMorph *morphs, const WorldHipMorphCurves *curves, int o_stride, double *d_f0_out,
                      double *d_sp_out, double *d_ap_out, double *d_pos_a, double *d_pos_b) {
  if (n_pairs < 1 || n_pairs > kGridY) fail("morph: n_pairs %d outside [1, %d]", n_pairs, kGridY);
  if (!n_a || !n_b || !morphs) fail("morph: null n_a / n_b / morphs");
  if ((!d_f0_a != !d_f0_b) || (!d_f0_a != !d_f0_out)) fail("morph: give d_f0_a, d_f0_b and d_f0_out, or none of them");
  if ((!d_sp_a != !d_sp_b) || (!d_sp_a != !d_sp_out)) fail("morph: give d_sp_a, d_sp_b and d_sp_out, or none of them");
  if ((!d_ap_a != !d_ap_b) || (!d_ap_a != !d_ap_out)) fail("morph: give d_ap_a, d_ap_b and d_ap_out, or none of them");
  const bool with_f0 = d_f0_a != nullptr, with_sp = d_sp_a != nullptr, with_ap = d_ap_a != nullptr;
  if (with_sp || with_ap) {
    if (fs <= 0) fail("morph: fs must be positive");
    if (fft_size < 128 || fft_size > 8192 || (fft_size & (fft_size - 1)) != 0)
      fail("morph: fft_size %d is not a power of two in [128, 8192]", fft_size);
  }
  if (d_path && !d_path_len) fail("morph: a path needs d_path_len (null)");
  std::vector<int> n_out(n_pairs);
  std::vector<double> rate(4 * (size_t)n_pairs);
  int max_out = 0;
  for (int u = 0; u < n_pairs; ++u) {
    if (n_a[u] < 1 || n_b[u] < 1) fail("morph: pair %d has %d x %d frames; each side needs one", u, n_a[u], n_b[u]);
    if (n_a[u] > a_stride || n_b[u] > b_stride)
      fail("morph: pair %d has %d x %d frames, beyond the strides (%d, %d)", u, n_a[u], n_b[u], a_stride, b_stride);
    const double r[4] = {morphs[u].time_rate, morphs[u].f0_rate, morphs[u].sp_rate, morphs[u].ap_rate};
    for (int q = 0; q < 4; ++q) {
      if (!(r[q] >= 0.0 && r[q] <= 1.0)) fail("morph: pair %d: rate %g outside [0, 1]", u, r[q]);
      rate[4 * (size_t)u + q] = r[q];
    }
    if (d_path && (long long)p_stride < (long long)n_a[u] + n_b[u] - 1)
      fail("morph: p_stride %d cannot hold pair %d's longest path (%d + %d - 1)", p_stride, u, n_a[u], n_b[u]);
    if (!d_path && n_a[u] != n_b[u])
      fail("morph: pair %d: without a path n_a (%d) must equal n_b (%d)", u, n_a[u], n_b[u]);
    n_out[u] = morph_length(n_a[u], n_b[u], r[0]);
    if (n_out[u] > o_stride) fail("morph: o_stride %d below pair %d's %d output frames", o_stride, u, n_out[u]);
    max_out = std::max(max_out, n_out[u]);
  }
  const WorldHipMorphCurves none = {nullptr, nullptr, nullptr};
  const WorldHipMorphCurves &cv = curves ? *curves : none;
  {
    const size_t f0 = (size_t)n_pairs * sizeof(double), bins = f0 * (fft_size / 2 + 1);   // bytes per frame of all pairs
    refuse_overlap("morph",
                   {{d_f0_out, f0 * o_stride, "d_f0_out"}, {d_sp_out, bins * o_stride, "d_sp_out"}, {d_ap_out, bins * o_stride, "d_ap_out"},
                    {d_pos_a, f0 * o_stride, "d_pos_a"}, {d_pos_b, f0 * o_stride, "d_pos_b"}},
                   {{d_f0_a, f0 * a_stride, "d_f0_a"}, {d_f0_b, f0 * b_stride, "d_f0_b"}, {d_sp_a, bins * a_stride, "d_sp_a"},
                    {d_sp_b, bins * b_stride, "d_sp_b"}, {d_ap_a, bins * a_stride, "d_ap_a"}, {d_ap_b, bins * b_stride, "d_ap_b"},
                    {d_path, (size_t)n_pairs * p_stride * 2 * sizeof(int), "d_path"}, {d_path_len, (size_t)n_pairs * sizeof(int), "d_path_len"},
                    {cv.d_f0_rate, f0 * o_stride, "d_f0_rate"}, {cv.d_sp_rate, f0 * o_stride, "d_sp_rate"},
                    {cv.d_ap_rate, f0 * o_stride, "d_ap_rate"}});
  }
  if (!with_f0 && !with_sp && !with_ap && !d_pos_a && !d_pos_b) return;
  MorphParams p;
  p.pos_a = d_pos_a; p.pos_b = d_pos_b;
  if (!d_pos_a || !d_pos_b)
    begin_stage(c, [&](Arena &a) {
      if (!d_pos_a) p.pos_a = a.take<double>((size_t)n_pairs * o_stride);
      if (!d_pos_b) p.pos_b = a.take<double>((size_t)n_pairs * o_stride);
    });
  else
    open_uploads(c);                                        // (no workspace: prepared offsets stay valid)
  p.n_pairs = n_pairs; p.fft_size = fft_size;
  p.a_stride = a_stride; p.b_stride = b_stride; p.o_stride = o_stride; p.p_stride = p_stride;
  p.n_a = upload(c, n_a, n_pairs);
  p.n_b = upload(c, n_b, n_pairs);
  p.n_out = upload(c, n_out);
  p.rate = upload(c, rate);
  p.path = d_path; p.path_len = d_path_len;
  p.f0_curve = cv.d_f0_rate; p.sp_curve = cv.d_sp_rate; p.ap_curve = cv.d_ap_rate;
  p.f0_a = d_f0_a; p.sp_a = d_sp_a; p.ap_a = d_ap_a; p.f0_b = d_f0_b; p.sp_b = d_sp_b; p.ap_b = d_ap_b;
  p.f0_out = d_f0_out; p.sp_out = d_sp_out; p.ap_out = d_ap_out;
  launch_morph_positions(p, max_out, c->stream);
  if (with_sp) launch_morph_frames_sp(p, max_out, c->stream);
  if (with_ap) launch_morph_frames_ap(p, max_out, c->stream);
  if (with_f0) launch_morph_frames_f0(p, max_out, c->stream);
}

// Sampling-rate conversion (include/world_hip.h: world_hip_resample_batch; resample.inc).  The host arithmetic -- lengths,
// shape, refusals, coefficients -- is tables.cpp's; here the table is put on the device once per (L, M, design) and found again.
static ResampleDesign resample_design(const WorldHipResampleOption *opt) {
  WorldHipResampleOption best;
  if (!opt) { world_hip_resample_option(WORLD_HIP_RESAMPLE_BEST, &best); opt = &best; }   // (the presets are named there alone)
  return ResampleDesign{opt->zeros, opt->rolloff, opt->kaiser_beta};
}
constexpr size_t kResampleTablesKept = 4;        // a mixed-rate tool run alternates between a few ratios
void ResampleTable::put(WorldHipContext *c, const Host &h) { put_table(c, d_coef, h.coef); put_table(c, d_kdiv, h.kdiv); }
void ResampleTable::drop(WorldHipContext *c) { drop_table(c, d_coef); drop_table(c, d_kdiv); }
static const ResampleTable &resample_table(WorldHipContext *c, const ResampleShape &sh, const ResampleDesign &d) {
  return cached_table(
      c, c->resample_tables, kResampleTablesKept, "resample: a ratio that was never run before cannot be captured: run it once first",
      [&](const ResampleTable &t) {
        return t.L == sh.L && t.M == sh.M && t.W == sh.W && t.design.zeros == d.zeros && t.design.rolloff == d.rolloff &&
               t.design.beta == d.beta;
      },
      [&](ResampleTable &t) {
        t.L = sh.L; t.M = sh.M; t.W = sh.W; t.design = d;
        const size_t taps = 2 * (size_t)sh.W, L = (size_t)sh.L;
        std::vector<double> host(L * taps);
        ResampleTable::Host dev{std::vector<double>(L * taps), std::vector<int>(L)};
        build_resample_taps(sh, d, host.data());
        for (size_t r = 0; r < L; ++r) {
          const size_t p = (size_t)(((long long)r * sh.M) % sh.L);
          dev.kdiv[r] = (int)(((long long)r * sh.M) / sh.L);
          for (size_t i = 0; i < taps; ++i) dev.coef[i * L + r] = host[p * taps + i];
        }
        return dev;
      });
}

static void run_resample(WorldHipContext *c, int n_utt, int fs_in, int fs_out, const WorldHipResampleOption *opt,
                         const double *d_x, int x_stride, const int *x_length, double *d_y, int y_stride) {
  if (n_utt < 1) fail("resample: n_utt must be positive");
  if (!d_x || !d_y || !x_length) fail("resample: null d_x / d_y / x_length");
  const ResampleDesign design = resample_design(opt);
  ResampleShape sh;
  if (const char *why = resample_shape(fs_in, fs_out, design, &sh)) fail("resample: %s", why);
  std::vector<int> n_out(n_utt);
  int max_out = 0, max_in = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (x_length[u] < 1 || x_length[u] > x_stride)
      fail("resample: x_length[%d]=%d outside [1, x_stride=%d]", u, x_length[u], x_stride);
    n_out[u] = resample_length(x_length[u], fs_in, fs_out);
    if (n_out[u] < 1) fail("resample: utterance %d: %d samples at %d Hz are more than INT_MAX at %d Hz", u, x_length[u], fs_in, fs_out);
    if (n_out[u] > y_stride) fail("resample: y_stride %d below utterance %d's %d output samples", y_stride, u, n_out[u]);
    max_out = std::max(max_out, n_out[u]);
    max_in = std::max(max_in, x_length[u]);
  }
  refuse_overlap("resample", {{d_y, sizeof(double) * (size_t)n_utt * y_stride, "d_y"}},
                 {{d_x, sizeof(double) * (size_t)n_utt * x_stride, "d_x"}});
  open_uploads(c);                                          // (no workspace: prepared offsets stay valid)
  ResampleParams p;
  p.L = (int)sh.L; p.M = (int)sh.M; p.W = (int)sh.W;
  p.tile = p.span = 0;
  p.x_stride = x_stride; p.y_stride = y_stride;
  p.coef = nullptr; p.kdiv = nullptr;
  const bool copy = fs_in == fs_out;
  ResamplePlan plan{};
  if (!copy) {
    const ResampleTable &t = resample_table(c, sh, design);
    p.coef = t.d_coef; p.kdiv = t.d_kdiv;
    plan = resample_plan(sh.L, sh.M, sh.W);
    p.tile = plan.tile; p.span = plan.span;
  }
  const int *d_len = upload(c, x_length, n_utt), *d_out = upload(c, n_out);
  for (int u0 = 0; u0 < n_utt; u0 += kGridY) {
    const int n = std::min(kGridY, n_utt - u0);
    p.x = d_x + (size_t)u0 * x_stride; p.y = d_y + (size_t)u0 * y_stride;
    p.x_len = d_len + u0; p.n_out = d_out + u0;
    if (copy) launch_resample_copy(p, max_in, n, c->stream);
    else launch_resample(p, plan, max_out, n, c->stream);
  }
}

// All-pass mel-cepstra (include/world_hip.h: world_hip_sp2mc / world_hip_mc2sp; mcep.inc).  The host arithmetic -- the
// refusals of a shape, the tables -- is tables.cpp's; here a direction's table is put on the device once per
// (fft_size, order, alpha) and found again.
constexpr size_t kMcepTablesKept = 4;            // both directions of two shapes
void McepTable::put(WorldHipContext *c, const Host &h) { put_table(c, d_table, h); }
void McepTable::drop(WorldHipContext *c) { drop_table(c, d_table); }
static const McepTable &mcep_table(WorldHipContext *c, bool decode, int fft_size, int order, double alpha) {
  unsigned long long bits;
  memcpy(&bits, &alpha, sizeof bits);
  return cached_table(
      c, c->mcep_tables, kMcepTablesKept, "mcep: a (fft_size, order, alpha) that was never run before cannot be captured: run it once first",
      [&](const McepTable &t) { return t.decode == decode && t.fft_size == fft_size && t.order == order && t.alpha_bits == bits; },
      [&](McepTable &t) {
        t.fft_size = fft_size; t.order = order; t.alpha_bits = bits; t.decode = decode;
        mcep_table_shape(decode, fft_size, order, &t.k_pad, &t.n_pad);
        const size_t K = (size_t)fft_size / 2 + 1, P = (size_t)order + 1;
        std::vector<double> host(K * P), dev((size_t)t.k_pad * t.n_pad, 0.0);
        if (decode) {                            // D [K][P] -> [m][k]
          build_mcep_decode(fft_size, order, alpha, host.data());
          for (size_t k = 0; k < K; ++k)
            for (size_t m = 0; m < P; ++m) dev[m * t.n_pad + k] = host[k * P + m];
        } else {                                 // M [P][K] -> [k][m]
          build_mcep_encode(fft_size, order, alpha, host.data());
          for (size_t m = 0; m < P; ++m)
            for (size_t k = 0; k < K; ++k) dev[k * t.n_pad + m] = host[m * K + k];
        }
        return dev;
      });
}

static void run_mcep(WorldHipContext *c, bool decode, int rows, int fft_size, int order, double alpha, const double *d_in,
                     long long in_stride, double *d_out, long long out_stride) {
  const char *name = decode ? "mc2sp" : "sp2mc";
  if (rows < 1) fail("%s: rows must be positive", name);
  if (!d_in || !d_out) fail("%s: null %s", name, decode ? "d_mc / d_sp" : "d_sp / d_mc");
  if (const char *why = mcep_shape(fft_size, order, alpha)) fail("%s: %s", name, why);
  const long long K = fft_size / 2 + 1, P = order + 1, in_cols = decode ? P : K, out_cols = decode ? K : P;
  if (in_stride < in_cols)
    fail("%s: %s %lld below the row's %lld doubles", name, decode ? "mc_row_stride" : "sp_row_stride", in_stride, in_cols);
  if (out_stride < out_cols)
    fail("%s: %s %lld below the row's %lld doubles", name, decode ? "sp_row_stride" : "mc_row_stride", out_stride, out_cols);
  refuse_overlap(name, {{d_out, sizeof(double) * (size_t)((rows - 1) * out_stride + out_cols), decode ? "d_sp" : "d_mc"}},
                 {{d_in, sizeof(double) * (size_t)((rows - 1) * in_stride + in_cols), decode ? "d_mc" : "d_sp"}});
  const McepTable &t = mcep_table(c, decode, fft_size, order, alpha);
  McepParams p;
  p.in = d_in; p.out = d_out; p.table = t.d_table;
  p.in_stride = in_stride; p.out_stride = out_stride;
  p.rows = rows; p.k_in = (int)in_cols; p.k_out = (int)out_cols; p.k_pad = t.k_pad; p.n_pad = t.n_pad;
  launch_mcep(p, decode, c->stream);
}

// Dynamic features and parameter generation (include/world_hip.h: world_hip_delta_batch / world_hip_mlpg_batch; mlpg.inc).
// Everything the host can know is refused before any GPU work.  The stencil (generate == false) reads the statics
// [u][t][dim] as `d_in` and needs no workspace; the generation reads means and variances [u][t][n_win dim] and keeps the
// factor and the scaled right-hand side of every system, [max T][2 L + 1][n_utt dim] doubles, in the arena.
static void run_mlpg_or_delta(WorldHipContext *c, bool generate, int n_utt, int dim, int n_win, int half_width,
                              const double *win, const int *n_frames, const unsigned char *d_mask, long long mask_us,
                              const double *d_in, long long in_us, long long in_rs, const double *d_var, long long var_us,
                              long long var_rs, int precision, double fill, double *d_out, long long out_us, long long out_rs) {
  const char *name = generate ? "mlpg" : "delta";
  if (n_utt < 1) fail("%s: n_utt must be positive", name);
  if (dim < 1) fail("%s: dim must be positive", name);
  if (!win || !n_frames || !d_in || !d_out || (generate && !d_var))
    fail("%s: null %s", name, generate ? "win / n_frames / d_mean / d_var / d_out" : "win / n_frames / d_c / d_out");
  if (n_win < 1 || n_win > 4) fail("%s: n_win %d outside [1, 4]", name, n_win);
  if (half_width < 0 || half_width > 2) fail("%s: half_width %d outside [0, 2]", name, half_width);
  const int taps = 2 * half_width + 1;
  for (int k = 0; k < n_win * taps; ++k)
    if (!std::isfinite(win[k])) fail("%s: window %d has a coefficient that is not finite", name, k / taps);
  for (int k = 0; k < taps; ++k)
    if (win[k] != (k == half_width ? 1.0 : 0.0)) fail("%s: window 0 must be the identity (1 at tau = 0, 0 elsewhere)", name);
  if ((long long)n_win * dim > INT_MAX) fail("%s: n_win * dim above INT_MAX", name);
  int max_frames = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (n_frames[u] < 1) fail("%s: n_frames[%d]=%d; an utterance needs a frame", name, u, n_frames[u]);
    max_frames = std::max(max_frames, n_frames[u]);
  }
  if ((long long)max_frames * dim > (1LL << 38)) fail("%s: %d frames of %d dimensions are more than 2^38 elements", name, max_frames, dim);
  const long long in_cols = generate ? (long long)n_win * dim : dim, out_cols = generate ? dim : (long long)n_win * dim;
  const char *in_name = generate ? "mean" : "c";
  if (in_rs < in_cols) fail("%s: %s_row_stride %lld below the row's %lld doubles", name, in_name, in_rs, in_cols);
  if (out_rs < out_cols) fail("%s: out_row_stride %lld below the row's %lld doubles", name, out_rs, out_cols);
  if (generate && var_rs != 0 && var_rs < in_cols) fail("%s: var_row_stride %lld is neither 0 nor the row's %lld doubles or more", name, var_rs, in_cols);
  if (in_us < 0 || out_us < 0 || (generate && var_us < 0) || (d_mask && mask_us < 0)) fail("%s: a negative utterance stride", name);
  // the doubles (bytes for the mask) each array spans; utterances of the output may not run into each other
  long long in_span = 0, var_span = 0, out_span = 0, mask_span = 0;
  for (int u = 0; u < n_utt; ++u) {
    const long long rows = n_frames[u] - 1;
    if (u + 1 < n_utt && rows * out_rs + out_cols > out_us)
      fail("%s: out_utt_stride %lld below utterance %d's %lld doubles", name, out_us, u, rows * out_rs + out_cols);
    if (d_mask && u + 1 < n_utt && n_frames[u] > mask_us) fail("%s: mask_utt_stride %lld below n_frames[%d]=%d", name, mask_us, u, n_frames[u]);
    in_span = std::max(in_span, u * in_us + rows * in_rs + in_cols);
    var_span = std::max(var_span, u * var_us + rows * var_rs + in_cols);
    out_span = std::max(out_span, u * out_us + rows * out_rs + out_cols);
    mask_span = std::max(mask_span, u * mask_us + rows + 1);
  }
  refuse_overlap(name, {{d_out, sizeof(double) * (size_t)out_span, "d_out"}},
                 {{d_in, sizeof(double) * (size_t)in_span, generate ? "d_mean" : "d_c"},
                  {d_var, sizeof(double) * (size_t)var_span, "d_var"}, {d_mask, (size_t)mask_span, "d_mask"}});   // (delta: no d_var)
  MlpgParams p;
  p.ws = nullptr;
  if (generate && half_width > 0)
    begin_stage(c, [&](Arena &a) { p.ws = a.take<double>(mlpg_workspace_doubles(n_utt, dim, max_frames, half_width)); });
  else
    open_uploads(c);                                        // (no workspace: prepared offsets stay valid)
  p.mean = d_in; p.var = d_var; p.out = d_out; p.mask = d_mask;
  p.mean_us = in_us; p.mean_rs = in_rs; p.var_us = var_us; p.var_rs = var_rs; p.out_us = out_us; p.out_rs = out_rs;
  p.mask_us = mask_us;
  p.n_sys = (long long)n_utt * dim;
  p.dim = dim; p.n_win = n_win; p.precision = precision != 0; p.fill = fill;
  for (int w = 0; w < 4; ++w)
    for (int k = 0; k < 5; ++k) {
      const int tau = k - 2;
      p.win[w][k] = w < n_win && tau >= -half_width && tau <= half_width ? win[w * taps + tau + half_width] : 0.0;
    }
  p.n_frames = upload(c, n_frames, n_utt);
  for (int u0 = 0; u0 < n_utt; u0 += kGridY) {
    const int n = std::min(kGridY, n_utt - u0);
    p.u0 = u0;
    if (generate) launch_mlpg(p, half_width, n, max_frames, c->stream);
    else launch_delta(p, half_width, n, max_frames, c->stream);
  }
}
static void run_delta(WorldHipContext *c, int n_utt, int dim, int n_win, int half_width, const double *win, const int *n_frames,
                      const unsigned char *d_mask, long long mask_us, const double *d_c, long long c_us, long long c_rs,
                      double fill, double *d_out, long long out_us, long long out_rs) {
  run_mlpg_or_delta(c, false, n_utt, dim, n_win, half_width, win, n_frames, d_mask, mask_us, d_c, c_us, c_rs, nullptr, 0, 0, 0,
                    fill, d_out, out_us, out_rs);
}
static void run_mlpg(WorldHipContext *c, int n_utt, int dim, int n_win, int half_width, const double *win, const int *n_frames,
                     const unsigned char *d_mask, long long mask_us, const double *d_mean, long long mean_us, long long mean_rs,
                     const double *d_var, long long var_us, long long var_rs, int precision, double fill, double *d_out,
                     long long out_us, long long out_rs) {
  run_mlpg_or_delta(c, true, n_utt, dim, n_win, half_width, win, n_frames, d_mask, mask_us, d_mean, mean_us, mean_rs, d_var,
                    var_us, var_rs, precision, fill, d_out, out_us, out_rs);
}

// Joint-density Gaussian mixture (include/world_hip.h: world_hip_gmm_convert / _accumulate / _fit / _init; gmm.inc).  The
// host arithmetic -- the prepared model, the M-step's finish -- is gmm_host.h's.  q and gamma [rows][M] and the best mixture
// [rows] are the conversion's workspace.
static void run_gmm_convert(WorldHipContext *c, int M, int Dx, int Dy, const double *d_model, int rows, const double *d_x,
                            long long x_rs, int mode, double *d_mean, long long mean_rs, double *d_var, long long var_rs,
                            double *d_post, long long post_rs, double *d_loglik) {
  if (const char *why = gmm_shape(M, Dx, Dy)) fail("gmm_convert: %s", why);
  if (rows < 1) fail("gmm_convert: rows must be positive");
  if (!d_model || !d_x) fail("gmm_convert: null d_model / d_x");
  if (mode != 0 && mode != 1) fail("gmm_convert: mode %d is neither 0 (mixture) nor 1 (most likely component)", mode);
  if (Dy == 0 && (d_mean || d_var)) fail("gmm_convert: d_mean / d_var given, but the model has no target part (Dy = 0)");
  if (x_rs < Dx) fail("gmm_convert: x_row_stride %lld below the row's %d doubles", x_rs, Dx);
  if (d_mean && mean_rs < Dy) fail("gmm_convert: mean_row_stride %lld below the row's %d doubles", mean_rs, Dy);
  if (d_var && var_rs < Dy) fail("gmm_convert: var_row_stride %lld below the row's %d doubles", var_rs, Dy);
  if (d_post && post_rs < M) fail("gmm_convert: post_row_stride %lld below the row's %d doubles", post_rs, M);
  const GmmLayout g = gmm_layout(M, Dx, Dy);
  const size_t r1 = (size_t)rows - 1;
  refuse_overlap("gmm_convert",
                 {{d_mean, sizeof(double) * (r1 * mean_rs + Dy), "d_mean"}, {d_var, sizeof(double) * (r1 * var_rs + Dy), "d_var"},
                  {d_post, sizeof(double) * (r1 * post_rs + M), "d_post"}, {d_loglik, sizeof(double) * (size_t)rows, "d_loglik"}},
                 {{d_x, sizeof(double) * (r1 * x_rs + Dx), "d_x"}, {d_model, sizeof(double) * g.doubles, "d_model"}});
  GmmParams p;
  begin_stage(c, [&](Arena &a) {
    p.q = a.take<double>((size_t)rows * M);
    p.best = a.take<int>((size_t)rows);
  });
  p.x = d_x; p.model = d_model;
  p.x_rs = x_rs; p.mean_rs = mean_rs; p.var_rs = var_rs; p.post_rs = post_rs;
  p.off_c = g.c; p.off_mux = g.mux; p.off_muy = g.muy; p.off_v = g.v; p.off_ut = g.ut; p.off_at = g.at;
  p.mean = d_mean; p.var = d_var; p.post = d_post; p.loglik = d_loglik;
  p.rows = rows; p.M = M; p.Dx = Dx; p.Dy = Dy; p.Kp = g.Kp; p.Ep = g.Ep; p.mode = mode;
  launch_gmm_q(p, c->stream);
  launch_gmm_posterior(p, c->stream);
  if (d_mean || d_var) launch_gmm_regress(p, c->stream);
}

static void check_gmm_rows(const char *name, int M, int P, int rows, const double *d_z, long long z_rs) {
  if (M < 1 || M > kGmmMaxMix) fail("%s: the number of mixtures must lie in [1, %d]", name, kGmmMaxMix);
  if (P < 1 || P > kGmmMaxDim) fail("%s: the dimension must lie in [1, %d]", name, kGmmMaxDim);
  if (rows < 1) fail("%s: rows must be positive", name);
  if (!d_z) fail("%s: null d_z", name);
  if (z_rs < P) fail("%s: z_row_stride %lld below the row's %d doubles", name, z_rs, P);
}

static void run_gmm_accumulate(WorldHipContext *c, int M, int P, int rows, const double *d_z, long long z_rs,
                               const double *d_post, long long post_rs, const double *d_shift, double *d_N, double *d_S1,
                               double *d_G) {
  check_gmm_rows("gmm_accumulate", M, P, rows, d_z, z_rs);
  if (!d_post || !d_shift || !d_N || !d_S1 || !d_G) fail("gmm_accumulate: null d_post / d_shift / d_N / d_S1 / d_G");
  if (post_rs < M) fail("gmm_accumulate: post_row_stride %lld below the row's %d doubles", post_rs, M);
  const size_t r1 = (size_t)rows - 1, mp = (size_t)M * P;
  refuse_overlap("gmm_accumulate",
                 {{d_N, sizeof(double) * (size_t)M, "d_N"}, {d_S1, sizeof(double) * mp, "d_S1"}, {d_G, sizeof(double) * mp * P, "d_G"}},
                 {{d_z, sizeof(double) * (r1 * z_rs + P), "d_z"}, {d_post, sizeof(double) * (r1 * post_rs + M), "d_post"},
                  {d_shift, sizeof(double) * mp, "d_shift"}});
  GmmAccParams p;
  p.z = d_z; p.post = d_post; p.shift = d_shift; p.z_rs = z_rs; p.post_rs = post_rs;
  p.N = d_N; p.S1 = d_S1; p.G = d_G; p.rows = rows; p.M = M; p.P = P;
  launch_gmm_accumulate(p, c->stream);
}

static void check_gmm_host(const char *name, const double *w, const double *mu, const double *cov) {
  if (!w || !mu || !cov) fail("%s: null w / mu / cov", name);
}

// The statistics of one set of rows on the host: N [M], S1 [M][P], G [M][P][P] (accumulate, then copied down; waits).
struct GmmStats { std::vector<double> N, S1, G; };
struct GmmDeviceStats { double *N, *S1, *G; };
static void gmm_stats_down(WorldHipContext *c, int M, int P, const GmmDeviceStats &d, GmmStats *h) {
  const size_t mp = (size_t)M * P;
  h->N.resize(M); h->S1.resize(mp); h->G.resize(mp * P);
  devrt::d2h(h->N.data(), d.N, sizeof(double) * M, c->stream);
  devrt::d2h(h->S1.data(), d.S1, sizeof(double) * mp, c->stream);
  devrt::d2h(h->G.data(), d.G, sizeof(double) * mp * P, c->stream);
  devrt::sync(c->stream);
}

static void run_gmm_fit(WorldHipContext *c, int M, int P, int rows, const double *d_z, long long z_rs, int n_iter, double reg,
                        double *w, double *mu, double *cov, double *loglik) {
  check_gmm_rows("gmm_fit", M, P, rows, d_z, z_rs);
  check_gmm_host("gmm_fit", w, mu, cov);
  if (n_iter < 1) fail("gmm_fit: n_iter must be positive");
  if (!std::isfinite(reg) || reg < 0) fail("gmm_fit: reg must be finite and not negative");
  if (devrt::is_capturing(c->stream)) fail("gmm_fit: the fit waits for the device every iteration and cannot be captured");
  const GmmLayout g = gmm_layout(M, P, 0);
  const size_t mp = (size_t)M * P;
  double *d_model = nullptr, *d_post = nullptr, *d_ll = nullptr, *d_shift = nullptr;
  GmmDeviceStats ds{nullptr, nullptr, nullptr};
  std::vector<double> model(g.doubles), ll(rows), w2(M), mu2(mp), cov2(mp * P);
  GmmStats hs;
  hold_at_floor(
      c, "gmm_fit",
      [&](Arena &a) {
        d_model = a.take<double>(g.doubles);
        d_post = a.take<double>((size_t)rows * M);
        d_ll = a.take<double>((size_t)rows);
        d_shift = a.take<double>(mp);
        ds.N = a.take<double>((size_t)M);
        ds.S1 = a.take<double>(mp);
        ds.G = a.take<double>(mp * P);
      },
      [&] {
        for (int it = 0; it < n_iter; ++it) {
          const std::string why = gmm_prepare_host(M, P, 0, w, mu, cov, model.data());
          if (!why.empty()) fail("gmm_fit: iteration %d: %s", it, why.c_str());
          devrt::h2d(d_model, model.data(), sizeof(double) * g.doubles, c->stream);
          devrt::h2d(d_shift, mu, sizeof(double) * mp, c->stream);
          run_gmm_convert(c, M, P, 0, d_model, rows, d_z, z_rs, 0, nullptr, 0, nullptr, 0, d_post, M, d_ll);
          run_gmm_accumulate(c, M, P, rows, d_z, z_rs, d_post, M, d_shift, ds.N, ds.S1, ds.G);
          devrt::d2h(ll.data(), d_ll, sizeof(double) * rows, c->stream);
          gmm_stats_down(c, M, P, ds, &hs);
          long double sum = 0;
          for (int t = 0; t < rows; ++t) sum += ll[t];
          const std::string starved = gmm_update_host(M, P, hs.N.data(), hs.S1.data(), hs.G.data(), mu, (double)rows, reg,
                                                      w2.data(), mu2.data(), cov2.data());
          if (!starved.empty()) fail("gmm_fit: iteration %d: %s", it, starved.c_str());
          if (loglik) loglik[it] = (double)(sum / rows);
          std::copy(w2.begin(), w2.end(), w);
          std::copy(mu2.begin(), mu2.end(), mu);
          std::copy(cov2.begin(), cov2.end(), cov);
        }
      });
}

static void run_gmm_init(WorldHipContext *c, int M, int P, int rows, const double *d_z, long long z_rs, double *w, double *mu,
                         double *cov) {
  check_gmm_rows("gmm_init", M, P, rows, d_z, z_rs);
  check_gmm_host("gmm_init", w, mu, cov);
  if (devrt::is_capturing(c->stream)) fail("gmm_init: the call waits for the device and cannot be captured");
  const size_t p = (size_t)P;
  double *d_ones = nullptr;
  GmmDeviceStats ds{nullptr, nullptr, nullptr};
  begin_stage(c, [&](Arena &a) {
    d_ones = a.take<double>((size_t)rows);
    ds.N = a.take<double>(1);
    ds.S1 = a.take<double>(p);
    ds.G = a.take<double>(p * p);
  });
  launch_gmm_fill(d_ones, (size_t)rows, 1.0, c->stream);
  run_gmm_accumulate(c, 1, P, rows, d_z, z_rs, d_ones, 1, d_z, ds.N, ds.S1, ds.G);   // (the shift: row 0 where it lies)
  GmmStats hs;
  std::vector<double> row0(p), centre((size_t)M * p), w1(1), mu1(p), cov1(p * p);
  devrt::d2h(row0.data(), d_z, sizeof(double) * p, c->stream);
  for (int m = 0; m < M; ++m) {
    const long long t = (2LL * m + 1) * rows / (2LL * M);
    devrt::d2h(centre.data() + (size_t)m * p, d_z + (size_t)t * z_rs, sizeof(double) * p, c->stream);
  }
  gmm_stats_down(c, 1, P, ds, &hs);
  const std::string why = gmm_update_host(1, P, hs.N.data(), hs.S1.data(), hs.G.data(), row0.data(), (double)rows, 0.0, w1.data(),
                                          mu1.data(), cov1.data());
  if (!why.empty()) fail("gmm_init: %d rows are too few for %d dimensions", rows, P);
  for (int m = 0; m < M; ++m) {
    w[m] = 1.0 / M;
    for (size_t i = 0; i < p; ++i) {
      mu[(size_t)m * p + i] = centre[(size_t)m * p + i];
      for (size_t j = 0; j < p; ++j) cov[((size_t)m * p + i) * p + j] = i == j ? cov1[i * p + i] : 0.0;
    }
  }
}

// Training rows of a corpus (include/world_hip.h: world_hip_frame_power_batch / _select_frames_batch / _gather_rows_batch /
// _joint_rows_batch; corpus.h).  Everything the host can know is refused before any GPU work; the indices live on the
// device and are made harmless in the kernel.  Only a mean without d_power takes workspace (P [n_utt][max T]).
static int corpus_counts(const char *name, const char *what, const int *n, int count) {
  int largest = 0;
  for (int u = 0; u < count; ++u) {
    if (n[u] < 1) fail("%s: %s[%d]=%d; each needs one", name, what, u, n[u]);
    largest = std::max(largest, n[u]);
  }
  return largest;
}
static void run_frame_power(WorldHipContext *c, int n_utt, int fft_size, const int *n_frames, const double *d_sp, long long sp_us,
                            long long sp_rs, double *d_power, long long power_us, double *d_mean) {
  const char *name = "frame_power";
  if (n_utt < 1) fail("%s: n_utt must be positive", name);
  if (!n_frames || !d_sp) fail("%s: null n_frames / d_sp", name);
  if (fft_size < 128 || fft_size > 8192 || (fft_size & (fft_size - 1))) fail("%s: fft_size %d is not a power of two in [128, 8192]", name, fft_size);
  const int bins = fft_size / 2 + 1, max_frames = corpus_counts(name, "n_frames", n_frames, n_utt);
  if (sp_rs < bins) fail("%s: sp_row_stride %lld below the row's %d doubles", name, sp_rs, bins);
  if (sp_us < 0 || (d_power && power_us < 0)) fail("%s: a negative utterance stride", name);
  long long sp_span = 0, power_span = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (d_power && u + 1 < n_utt && n_frames[u] > power_us) fail("%s: power_utt_stride %lld below n_frames[%d]=%d", name, power_us, u, n_frames[u]);
    sp_span = std::max(sp_span, u * sp_us + (n_frames[u] - 1) * sp_rs + bins);
    power_span = std::max(power_span, u * power_us + n_frames[u]);
  }
  refuse_overlap(name, {{d_power, sizeof(double) * (size_t)power_span, "d_power"}, {d_mean, sizeof(double) * (size_t)n_utt, "d_mean"}},
                 {{d_sp, sizeof(double) * (size_t)sp_span, "d_sp"}});
  if (!d_power && !d_mean) return;
  CorpusPowerParams p;
  p.power = d_power; p.power_us = power_us;
  if (!d_power) {
    begin_stage(c, [&](Arena &a) { p.power = a.take<double>((size_t)n_utt * max_frames); });
    p.power_us = max_frames;
  } else {
    open_uploads(c);
  }
  p.sp = d_sp; p.sp_us = sp_us; p.sp_rs = sp_rs; p.mean = d_mean; p.fft_size = fft_size; p.n_utt = n_utt;
  p.n_frames = upload(c, n_frames, n_utt);
  for (int u0 = 0; u0 < n_utt; u0 += kGridY) {
    p.u0 = u0;
    launch_frame_power(p, std::min(kGridY, n_utt - u0), max_frames, c->stream);
  }
  p.u0 = 0;
  if (d_mean) launch_frame_power_mean(p, n_utt, c->stream);
}

static void run_select_frames(WorldHipContext *c, int n_utt, const int *n_frames, const double *d_value, long long value_us,
                              long long value_s, double threshold, const double *d_scale, const unsigned char *d_mask,
                              long long mask_us, int *d_index, long long index_us, int *d_count, unsigned char *d_keep,
                              long long keep_us) {
  const char *name = "select_frames";
  if (n_utt < 1) fail("%s: n_utt must be positive", name);
  if (!n_frames || !d_value) fail("%s: null n_frames / d_value", name);
  corpus_counts(name, "n_frames", n_frames, n_utt);
  if (value_s < 1) fail("%s: value_stride %lld below the one double of a value", name, value_s);
  if (value_us < 0 || (d_mask && mask_us < 0) || (d_index && index_us < 0) || (d_keep && keep_us < 0)) fail("%s: a negative utterance stride", name);
  long long value_span = 0, frames_span[3] = {0, 0, 0};     // mask, index, keep
  const long long us[3] = {mask_us, index_us, keep_us};
  for (int u = 0; u < n_utt; ++u) {
    if (d_index && u + 1 < n_utt && n_frames[u] > index_us) fail("%s: index_utt_stride %lld below n_frames[%d]=%d", name, index_us, u, n_frames[u]);
    if (d_keep && u + 1 < n_utt && n_frames[u] > keep_us) fail("%s: keep_utt_stride %lld below n_frames[%d]=%d", name, keep_us, u, n_frames[u]);
    value_span = std::max(value_span, u * value_us + (n_frames[u] - 1) * value_s + 1);
    for (int k = 0; k < 3; ++k) frames_span[k] = std::max(frames_span[k], u * us[k] + n_frames[u]);
  }
  refuse_overlap(name, {{d_index, sizeof(int) * (size_t)frames_span[1], "d_index"}, {d_count, sizeof(int) * (size_t)n_utt, "d_count"},
                        {d_keep, (size_t)frames_span[2], "d_keep"}},
                 {{d_value, sizeof(double) * (size_t)value_span, "d_value"}, {d_scale, sizeof(double) * (size_t)n_utt, "d_scale"},
                  {d_mask, (size_t)frames_span[0], "d_mask"}});
  if (!d_index && !d_count && !d_keep) return;
  open_uploads(c);
  CorpusSelectParams p;
  p.value = d_value; p.scale = d_scale; p.mask = d_mask; p.index = d_index; p.count = d_count; p.keep = d_keep;
  p.value_us = value_us; p.value_s = value_s; p.mask_us = mask_us; p.index_us = index_us; p.keep_us = keep_us;
  p.threshold = threshold;
  p.n_frames = upload(c, n_frames, n_utt);
  for (int u0 = 0; u0 < n_utt; u0 += kGridY) {
    p.u0 = u0;
    launch_select_frames(p, std::min(kGridY, n_utt - u0), c->stream);
  }
}

// both gathers: pair u's output rows z_off[u] + k z_rs, k < n_rows[u]
struct CorpusSide {
  const char *name;
  const double *d;
  const long long *row;           // host, first row of every pair; nullptr: utt_stride apart
  long long utt_stride, rs;
  const int *n;                   // host, rows of every pair
  const int *d_sel, *n_sel;       // the selection (device) and its lengths (host), or nullptr
  long long sel_us;
  int dim;
};
static void run_rows(WorldHipContext *c, const char *name, int n_pairs, CorpusSide A, CorpusSide B, const int *n_rows, const int *d_path,
                     int p_stride, double fill, double *d_z, const long long *z_row, long long z_us, long long z_rs) {
  if (n_pairs < 1) fail("%s: the number of utterances or pairs must be positive", name);
  if (A.dim < 1 || B.dim < 0) fail("%s: a row of %d + %d doubles", name, A.dim, B.dim);
  if ((long long)A.dim + B.dim > INT_MAX / 8) fail("%s: a row of %lld doubles is more than INT_MAX bytes", name, (long long)A.dim + B.dim);
  const int dim = A.dim + B.dim;
  if (!A.d || !A.n || !n_rows || !d_z || (B.dim && (!B.d || !B.n))) fail("%s: null input, count array or output", name);
  if (d_path ? (!A.row || !z_row || (B.dim && !B.row)) : !A.d_sel) fail("%s: null row array or index", name);
  if (z_rs < dim) fail("%s: the output's row stride %lld below the row's %d doubles", name, z_rs, dim);
  if (z_us < 0) fail("%s: a negative utterance stride", name);
  const int max_rows = corpus_counts(name, d_path ? "path_len" : "n_out", n_rows, n_pairs);
  std::vector<long long> z_off(n_pairs);
  std::vector<std::pair<long long, long long>> taken(n_pairs);      // rows [first, last] of every pair's output, in z_rs units
  long long z_lo = LLONG_MAX, z_hi = 0;
  for (int u = 0; u < n_pairs; ++u) {
    if (z_row && z_row[u] < 0) fail("%s: pair %d's output starts at a negative row", name, u);
    if (d_path && n_rows[u] > p_stride) fail("%s: path_len[%d]=%d above p_stride %d", name, u, n_rows[u], p_stride);
    z_off[u] = z_row ? z_row[u] * z_rs : u * z_us;
    const long long end = z_off[u] + (n_rows[u] - 1) * z_rs + dim;
    taken[u] = {z_off[u], end};
    z_lo = std::min(z_lo, z_off[u]);
    z_hi = std::max(z_hi, end);
  }
  std::sort(taken.begin(), taken.end());
  for (int u = 0; u + 1 < n_pairs; ++u)
    if (taken[u].second > taken[u + 1].first) fail("%s: two utterances or pairs of the output run into each other", name);
  Span ins[5] = {};
  int n_ins = 0;
  std::vector<long long> off[2];
  for (CorpusSide *s : {&A, &B}) {
    if (!s->dim) continue;
    if (s->rs < s->dim) fail("%s: %s's row stride %lld below the row's %d doubles", name, s->name, s->rs, s->dim);
    if (s->utt_stride < 0 || (s->d_sel && s->sel_us < 0)) fail("%s: a negative utterance stride", name);
    if (s->d_sel && !s->n_sel) fail("%s: a selection of %s without its lengths", name, s->name);
    corpus_counts(name, s == &A ? "n_a" : "n_b", s->n, n_pairs);
    if (s->d_sel) corpus_counts(name, "n_sel", s->n_sel, n_pairs);
    std::vector<long long> &o = off[s == &B];
    o.resize(n_pairs);
    long long span = 0, sel_span = 0;
    for (int u = 0; u < n_pairs; ++u) {
      if (s->row && s->row[u] < 0) fail("%s: pair %d of %s starts at a negative row", name, u, s->name);
      o[u] = s->row ? s->row[u] * s->rs : u * s->utt_stride;
      span = std::max(span, o[u] + (s->n[u] - 1) * s->rs + s->dim);
      if (s->d_sel) {
        if (u + 1 < n_pairs && s->n_sel[u] > s->sel_us) fail("%s: %s's selection stride %lld below its %d entries of pair %d", name, s->name, s->sel_us, s->n_sel[u], u);
        sel_span = std::max(sel_span, u * s->sel_us + s->n_sel[u]);
      }
    }
    ins[n_ins++] = {s->d, sizeof(double) * (size_t)span, s->name};
    ins[n_ins++] = {s->d_sel, sizeof(int) * (size_t)sel_span, "a selection"};
  }
  long long path_span = 0;
  for (int u = 0; u < n_pairs; ++u) path_span = std::max(path_span, ((long long)u * p_stride + n_rows[u]) * 2);
  ins[n_ins++] = {d_path, sizeof(int) * (size_t)path_span, "d_path"};
  refuse_overlap(name, {{d_z + z_lo, sizeof(double) * (size_t)(z_hi - z_lo), "the output"}}, {ins[0], ins[1], ins[2], ins[3], ins[4]});
  open_uploads(c);
  CorpusRowsParams p;
  p.a = A.d; p.b = B.dim ? B.d : nullptr; p.z = d_z;
  p.a_rs = A.rs; p.b_rs = B.rs; p.z_rs = z_rs;
  p.path = d_path; p.path_us = 2LL * p_stride;
  p.sel_a = A.d_sel; p.sel_a_us = A.sel_us; p.sel_b = B.dim ? B.d_sel : nullptr; p.sel_b_us = B.sel_us;
  p.dim_a = A.dim; p.dim_b = B.dim; p.group = corpus_group(A.dim, B.dim);
  memcpy(&p.fill, &fill, sizeof(fill));
  p.a_off = upload(c, off[0]);
  p.b_off = B.dim ? upload(c, off[1]) : p.a_off;
  p.z_off = upload(c, z_off);
  p.n_a = upload(c, A.n, n_pairs);
  p.n_b = B.dim ? upload(c, B.n, n_pairs) : p.n_a;
  p.n_sel_a = A.d_sel ? upload(c, A.n_sel, n_pairs) : p.n_a;
  p.n_sel_b = p.sel_b ? upload(c, B.n_sel, n_pairs) : p.n_a;
  p.n_rows = upload(c, n_rows, n_pairs);
  for (int u0 = 0; u0 < n_pairs; u0 += kGridY) {
    p.u0 = u0;
    launch_joint_rows(p, std::min(kGridY, n_pairs - u0), max_rows, c->stream);
  }
}
static void run_gather_rows(WorldHipContext *c, int n_utt, int dim, const int *n_src, const double *d_in, long long in_us,
                            long long in_rs, const int *n_out, const int *d_index, long long index_us, double fill, double *d_out,
                            long long out_us, long long out_rs) {
  const CorpusSide in{"d_in", d_in, nullptr, in_us, in_rs, n_src, d_index, n_out, index_us, dim};
  run_rows(c, "gather_rows", n_utt, in, CorpusSide{"", nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, 0}, n_out, nullptr, 0, fill,
           d_out, nullptr, out_us, out_rs);
}
static void run_joint_rows(WorldHipContext *c, int n_pairs, int dim_a, int dim_b, const double *d_a, const long long *a_row,
                           const int *n_a, long long a_rs, const double *d_b, const long long *b_row, const int *n_b, long long b_rs,
                           const int *path_len, const int *d_path, int p_stride, const int *d_sel_a, const int *n_sel_a,
                           long long sel_a_us, const int *d_sel_b, const int *n_sel_b, long long sel_b_us, double fill, double *d_z,
                           const long long *z_row, long long z_rs) {
  if (!d_path) fail("joint_rows: null d_path");
  run_rows(c, "joint_rows", n_pairs, CorpusSide{"d_a", d_a, a_row, 0, a_rs, n_a, d_sel_a, n_sel_a, sel_a_us, dim_a},
           CorpusSide{"d_b", d_b, b_row, 0, b_rs, n_b, d_sel_b, n_sel_b, sel_b_us, dim_b}, path_len, d_path, p_stride, fill, d_z, z_row, 0, z_rs);
}

// ---------------------------------------------------------------------------
// error plumbing for the C ABI
// ---------------------------------------------------------------------------
// A context's allocations and launches belong to ITS device: a thread that drives several GPUs calls in
// with whatever device it last selected, so select the context's for the duration of the call and put the
// caller's back afterwards.
struct DeviceScope {
  int before, wanted;
  explicit DeviceScope(int device) : before(devrt::current_device()), wanted(device) {
    if (before != wanted) devrt::set_device(wanted);
  }
  ~DeviceScope() {
    if (before != wanted) {
      try { devrt::set_device(before); } catch (...) {}
    }
  }
};
template <class F> static int guarded(WorldHipContext *c, F f) {
  if (!c) { g_last_error = "null context"; return 2; }
  std::lock_guard<std::mutex> g(c->lock);
  try {
    DeviceScope on_device(c->device);
    f();
    return 0;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return 1;
  } catch (const ArenaRegrow &) {
    c->arena.floor = 0;
    g_last_error = "internal error: the workspace had to grow under arrays held by the call";
    return 1;
  }
}

}  // namespace world_hip

using namespace world_hip;

// ===========================================================================
// Part 2 of include/world_hip.h
// ===========================================================================
extern "C" {

WorldHipContext *world_hip_create(int device, void *stream) {
  try {
    DeviceScope on_device(device);       // the caller's current device is left as it was
    WorldHipContext *c = new WorldHipContext;
    c->device = device;
    c->stream = static_cast<hipStream_t>(stream);
    std::vector<double2> tw(kTwAlloc);
    build_twiddles(tw.data());
    std::vector<uint4> jump((size_t)kJumpLevels * kJumpStride);
    build_jump_tables(jump.data());
    double2 *d_tw = nullptr;
    uint4 *d_jump = nullptr;
    put_table(c, d_tw, tw);
    put_table(c, d_jump, jump);
    devrt::sync(c->stream);
    c->tab = Tables{d_tw, d_jump};
    noise_table_retain(device);
    return c;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return nullptr;
  }
}

void world_hip_destroy(WorldHipContext *c) {
  if (!c) return;
  // the device's shared randn table is reference counted: give the reference back whatever happens below
  try { DeviceScope on_device(c->device); devrt::sync(c->stream); } catch (...) {}
  try { DeviceScope on_device(c->device); noise_table_release(c->device); } catch (...) {}
  try {
    DeviceScope on_device(c->device);    // the context's allocations belong to ITS device, not to the caller's current one
    devrt::sync(c->stream);
    if (c->arena.base) devrt::dfree(c->arena.base);
    if (c->d_xin) devrt::dfree(c->d_xin);
    if (c->h_xin) devrt::hfree_pinned(c->h_xin);
    if (c->xstream) { devrt::sync(c->xstream); devrt::stream_destroy(c->xstream); }
    for (void *t : c->tables) devrt::dfree(t);
    drop_small_arrays(c);
    if (c->xchg_ready) devrt::event_destroy(c->xchg_ready);
    if (c->xchg_done) devrt::event_destroy(c->xchg_done);
  } catch (...) {
  }
  delete c;
}

int world_hip_set_hint(WorldHipContext *ctx, int hint) {
  if (!ctx) return -1;
  ctx->hint = hint;
  return 0;
}
int world_hip_abi_version(void) { return WORLD_HIP_ABI_VERSION; }
const char *world_hip_last_error(void) { return g_last_error.c_str(); }

// pulses a synthesis call since the last check had no room for (0 = none); synchronises, clears the record
static int synthesis_need(WorldHipContext *c) {
  if (!c->d_synth_need) return 0;
  int need = 0;
  devrt::d2h(&need, c->d_synth_need, sizeof(int), c->stream);
  devrt::sync(c->stream);
  if (need > 0) devrt::dzero(c->d_synth_need, sizeof(int), c->stream);
  return need;
}

int world_hip_sync(WorldHipContext *c) {
  return guarded(c, [&] {
    devrt::sync(c->stream);
    const int need = synthesis_need(c);
    if (need > 0)
      fail("Synthesis dropped pulses: an utterance has %d, more than the capacity in force; call "
           "world_hip_set_synthesis_pulse_capacity(ctx, %d) and repeat the call", need, need);
  });
}

int world_hip_set_synthesis_pulse_capacity(WorldHipContext *c, int pulses_per_utterance) {
  return guarded(c, [&] {
    if (pulses_per_utterance < 0) fail("negative capacity");
    c->synth_pulse_cap = pulses_per_utterance;
  });
}

int world_hip_synthesis_pulses_dropped(WorldHipContext *c, int *needed) {
  return guarded(c, [&] {
    const int need = synthesis_need(c);
    if (needed) *needed = need;
  });
}

unsigned long long world_hip_workspace_bytes(WorldHipContext *c) {
  if (!c) return 0;
  unsigned long long bytes = c->arena.cap;
  for (const ResampleTable &t : c->resample_tables) bytes += t.bytes();
  for (const McepTable &t : c->mcep_tables) bytes += t.bytes();
  return bytes;
}

// the device's shared randn table (live + superseded generations), see rng.h
unsigned long long world_hip_noise_table_bytes(WorldHipContext *c) { return c ? noise_table_bytes(c->device) : 0; }

// wall-clock milliseconds this process has spent building + verifying the device's randn tables (cold-start cost)
double world_hip_noise_table_build_ms(WorldHipContext *c, int *builds) {
  if (!c) { if (builds) *builds = 0; return 0.0; }
  return noise_table_build_ms(c->device, builds);
}

// re-reduce the live randn table on the device and compare it with the host's sums (diagnostic; synchronises)
int world_hip_verify_tables(WorldHipContext *c) {
  return guarded(c, [&] { noise_table_verify(c->device, c->stream); });
}

#ifdef WORLD_EMU
// the host emulation always poisons (devrt.h): its counter, as the -DWH_HBM_POISON build exports it from devrt.cpp
unsigned long long world_hip_debug_poisoned_bytes(void) { return __atomic_load_n(&devrt::g_poisoned_bytes, __ATOMIC_RELAXED); }
#endif

// per-kernel HIP-event timing (used by bench.py for the roofline figure)
void world_hip_profile_enable(int on) {
#ifndef WORLD_EMU
  devrt::prof_enable(on != 0);
#else
  (void)on;
#endif
}
// Waits for the recorded kernels and writes "kernel_name milliseconds\n" lines into buf
// (truncated to cap-1 bytes).  Returns the untruncated length.
int world_hip_profile_collect(char *buf, int cap) {
#ifndef WORLD_EMU
  try {
    std::string s = devrt::prof_collect();
    if (buf && cap > 0) {
      size_t n = std::min((size_t)cap - 1, s.size());
      memcpy(buf, s.data(), n);
      buf[n] = 0;
    }
    return (int)s.size();
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return -1;
  }
#else
  if (buf && cap > 0) buf[0] = 0;
  return 0;
#endif
}

int world_hip_harvest_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                            const int *x_length, const HarvestOption *option, int f_stride, double *d_tpos,
                            double *d_f0) {
  return guarded(c, [&] { run_harvest(c, n_utt, fs, d_x, x_stride, x_length, option, f_stride, d_tpos, d_f0); });
}

int world_hip_dio_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                        const int *x_length, const DioOption *option, int f_stride, double *d_tpos, double *d_f0) {
  return guarded(c, [&] { run_dio(c, n_utt, fs, d_x, x_stride, x_length, option, f_stride, d_tpos, d_f0); });
}

int world_hip_stonemask_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                              const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                              const double *d_f0, double *d_refined) {
  return guarded(c, [&] {
    run_stonemask(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, d_refined);
  });
}

int world_hip_cheaptrick_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                               const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                               const double *d_f0, const CheapTrickOption *option, double *d_sp) {
  return guarded(c, [&] {
    run_cheaptrick(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, option, d_sp);
  });
}

int world_hip_d4c_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                        const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                        const double *d_f0, int fft_size, const D4COption *option, double *d_ap) {
  return guarded(c, [&] {
    run_d4c(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, fft_size, option, d_ap);
  });
}

int world_hip_analyze_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                            const HarvestOption *harvest_option, const CheapTrickOption *cheaptrick_option,
                            const D4COption *d4c_option, int f_stride, double *d_tpos, double *d_f0, double *d_spectrogram,
                            double *d_aperiodicity) {
  return guarded(c, [&] {
    run_analyze_dense(c, n_utt, fs, d_x, x_stride, x_length, harvest_option, cheaptrick_option, d4c_option, f_stride, d_tpos,
                      d_f0, d_spectrogram, d_aperiodicity);
  });
}

int world_hip_record_columns(int fft_size, int wire) {
  if (fft_size < 2 || (wire != 0 && wire != 1)) return -1;
  return record_cols(fft_size, wire);
}

int world_hip_analyze_packed(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                             const HarvestOption *harvest_option, const CheapTrickOption *cheaptrick_option,
                             const D4COption *d4c_option, long long first_row, double *d_block, int cols) {
  return guarded(c, [&] {
    run_analyze_packed(c, n_utt, fs, d_x, x_stride, x_length, harvest_option, cheaptrick_option, d4c_option, first_row,
                       d_block, cols);
  });
}

int world_hip_coded_columns(int fs, int number_of_dimensions) {
  if (fs <= 0 || number_of_dimensions < 1 || world_hip::number_of_aperiodicities(fs) < 1) return -1;
  return coded_cols(fs, number_of_dimensions);
}

int world_hip_analyze_coded(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                            const HarvestOption *harvest_option, const CheapTrickOption *cheaptrick_option,
                            const D4COption *d4c_option, int number_of_dimensions, long long first_row, double *d_block,
                            int cols) {
  return guarded(c, [&] {
    run_analyze_coded(c, n_utt, fs, d_x, x_stride, x_length, harvest_option, cheaptrick_option, d4c_option,
                      number_of_dimensions, first_row, d_block, cols);
  });
}

int world_hip_spectral_packed_range(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                                     const int *n_frames, int f_stride, const double *d_tpos, const double *d_f0,
                                     const CheapTrickOption *cheaptrick_option, const D4COption *d4c_option, int frame_lo,
                                     int frame_hi, int reuse_offsets, long long first_row, double *d_block, int cols) {
  return guarded(c, [&] {
    run_spectral_packed_range(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, cheaptrick_option,
                              d4c_option, frame_lo, frame_hi, first_row, d_block, cols, reuse_offsets != 0);
  });
}

// one stage, one frame range, dense rows (the rows of frames outside the range are not touched)
int world_hip_cheaptrick_batch_range(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                                     const int *x_length, const int *n_frames, int f_stride, const double *d_tpos,
                                     const double *d_f0, const CheapTrickOption *option, int frame_lo, int frame_hi,
                                     int reuse_offsets, double *d_sp) {
  return guarded(c, [&] {
    RowLayout lay;
    lay.frame_lo = frame_lo; lay.frame_hi = frame_hi; lay.skip_prepare = reuse_offsets != 0;
    run_cheaptrick(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, option, d_sp, lay);
  });
}
int world_hip_d4c_batch_range(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                              const int *n_frames, int f_stride, const double *d_tpos, const double *d_f0, int fft_size,
                              const D4COption *option, int frame_lo, int frame_hi, int reuse_offsets, double *d_ap) {
  return guarded(c, [&] {
    RowLayout lay;
    lay.frame_lo = frame_lo; lay.frame_hi = frame_hi; lay.skip_prepare = reuse_offsets != 0;
    run_d4c(c, n_utt, fs, d_x, x_stride, x_length, n_frames, f_stride, d_tpos, d_f0, fft_size, option, d_ap, lay);
  });
}

// HIP graphs: every batched call enqueued on the context between begin and end -- a whole
// Harvest + CheapTrick + D4C job is ~45 launches -- becomes ONE replayable graph bound to the buffers it was captured with.
// The shapes must have run once before (workspace, tables and the small per-call arrays are then resident and a call
// neither allocates nor copies nor waits); a replay costs the host one launch.
// A graph bakes in raw device pointers to memory the context owns (arena, small-array slabs, d_pk, cached tables).  The
// handle remembers the context's generation at capture; a later eager call that had to free or regrow any of that memory
// bumps the generation, and a replay of the stale graph is REFUSED instead of reading freed memory.
struct GraphHandle {
  void *exec;
  WorldHipContext *ctx;
  unsigned long long generation;
};
int world_hip_graph_begin(WorldHipContext *c) {
  return guarded(c, [&] { devrt::graph_begin(c->stream); });
}
int world_hip_graph_end(WorldHipContext *c, void **graph) {
  return guarded(c, [&] {
    if (!graph) fail("null graph handle");
    *graph = nullptr;
    void *exec = devrt::graph_end(c->stream);
    *graph = new GraphHandle{exec, c, c->generation};
  });
}
int world_hip_graph_launch(WorldHipContext *c, void *graph) {
  return guarded(c, [&] {
    if (!graph) fail("null graph");
    const GraphHandle *g = static_cast<const GraphHandle *>(graph);
    if (g->ctx != c) fail("graph_launch: the graph was captured on another context");
    if (g->generation != c->generation)
      fail("graph_launch: stale graph -- the context reallocated memory the graph points into since it was captured "
           "(a larger batch, a new option set or shape ran eagerly); capture it again");
    devrt::graph_launch(g->exec, c->stream);
  });
}
int world_hip_graph_destroy(void *graph) {
  if (!graph) return 0;
  GraphHandle *g = static_cast<GraphHandle *>(graph);
  try { devrt::graph_destroy(g->exec); delete g; return 0; } catch (const std::exception &e) { delete g; g_last_error = e.what(); return 1; }
}

// 0: every stage of the analysis path supports (fs, cheaptrick_fft_size); 1: it does not, and why (<= cap bytes) says which
// stage and limit.  Pure host arithmetic: callers (and the drop-in symbols) ask before any GPU work.
int world_hip_check_shape(int fs, int cheaptrick_fft_size, char *why, int cap) {
  const std::string r = shape_limit(15, fs, cheaptrick_fft_size);
  if (why && cap > 0) { snprintf(why, (size_t)cap, "%s", r.c_str()); }
  return r.empty() ? 0 : 1;
}

int world_hip_synthesis_batch(WorldHipContext *c, int n_utt, int fs, double frame_period, int fft_size,
                              const int *n_frames, int f_stride, const double *d_f0, const double *d_spectrogram,
                              const double *d_aperiodicity, const int *y_length, int y_stride, double *d_y) {
  return guarded(c, [&] {
    run_synthesis(c, n_utt, fs, frame_period, fft_size, n_frames, f_stride, d_f0, d_spectrogram, d_aperiodicity,
                  y_length, y_stride, d_y);
  });
}

int world_hip_synthesis_records(WorldHipContext *c, int n_utt, int fs, double frame_period, int fft_size,
                                const int *n_frames, long long first_row, const double *d_block, int cols, int wire,
                                int number_of_dimensions, const int *y_length, int y_stride, double *d_y) {
  return guarded(c, [&] {
    run_synthesis_records(c, n_utt, fs, frame_period, fft_size, n_frames, first_row, d_block, cols, wire,
                          number_of_dimensions, y_length, y_stride, d_y);
  });
}

// what box is this? (machine_probe.hip; synchronous, ~50 ms, allocates and frees 2 GB)
int world_hip_probe_machine(WorldHipContext *c, double *values, int n_values) {
  return guarded(c, [&] {
    if (!values || n_values < world_hip::kMachineProbeValues) fail("probe_machine: room for %d values needed", world_hip::kMachineProbeValues);
    devrt::sync(c->stream);
    world_hip::run_machine_probe(values, c->stream);
  });
}

// fft.h in isolation (fft_probe.hip): `batch` real transforms of 2^lg_n points, one workgroup each
static void run_fft_probe(WorldHipContext *c, bool inverse, int lg_n, int max_lr, int threads, int static_plan,
                          long long batch, const void *d_in, void *d_out) {
  if (lg_n < 6 || lg_n > kTwLog2) fail("probe: 2^%d points unsupported (64 .. %d)", lg_n, kTwN);   // (16384: 147 KB of LDS)
  if (max_lr != 3 && max_lr != 4) fail("probe: max_lr must be 3 (radix-8 plan) or 4 (radix-16 plan)");
  if (threads == 0) threads = std::max(64, (1 << lg_n) >> (max_lr + 1));      // one butterfly per thread and stage
  if (threads < 64 || threads > 1024 || threads % 64) fail("probe: bad workgroup size %d", threads);
  if (batch < 0 || batch > 0x7FFFFFFFll) fail("probe: bad batch");
  if (batch == 0) return;
  if (!d_in || !d_out) fail("null buffer");
  if (static_plan && !fft_probe_has_static(lg_n, max_lr)) fail("probe: no compile-time plan for 2^%d points, max_lr %d", lg_n, max_lr);
  launch_fft_probe(inverse, lg_n, max_lr, threads, static_plan != 0, (long)batch, d_in, d_out, c->tab, c->stream);
}
int world_hip_probe_rfft(WorldHipContext *c, int lg_n, int max_lr, int threads, int static_plan, long long batch,
                         const double *d_in, double *d_spectrum) {
  return guarded(c, [&] { run_fft_probe(c, false, lg_n, max_lr, threads, static_plan, batch, d_in, d_spectrum); });
}
int world_hip_probe_irfft(WorldHipContext *c, int lg_n, int max_lr, int threads, int static_plan, long long batch,
                          const double *d_spectrum, double *d_out) {
  return guarded(c, [&] { run_fft_probe(c, true, lg_n, max_lr, threads, static_plan, batch, d_spectrum, d_out); });
}

// every composition of fft.h's entry points a stage kernel runs (fft_probe.h: FftProbeMode), under either slot swizzle
int world_hip_probe_fft(WorldHipContext *c, int mode, int lg_n, int max_lr, int threads, int swizzle, long long batch,
                        const void *d_in, void *d_out) {
  return guarded(c, [&] {
    if (swizzle != 0 && swizzle != 1) fail("probe_fft: swizzle map %d unsupported (0: the shipped map, 1: d4c.hip's)", swizzle);
    if (batch < 0 || batch > 0x7FFFFFFFll) fail("probe_fft: bad batch");
    if (batch == 0) return;
    if (!d_in || !d_out) fail("null buffer");
#ifdef WORLD_EMU
    if (swizzle == 1 && !launch_fft_routes_swz1) fail("probe_fft: this host emulation was built without fft_probe_swz1.hip");
#endif
    const bool ok = swizzle == 0 ? launch_fft_routes_swz0(mode, lg_n, max_lr, threads, (long)batch, d_in, d_out, c->tab, c->stream)
                                 : launch_fft_routes_swz1(mode, lg_n, max_lr, threads, (long)batch, d_in, d_out, c->tab, c->stream);
    if (!ok)
      fail("probe_fft: mode %d at 2^%d points, max_lr %d, %d threads, swizzle %d is not a composition the stage kernels run.  Supported "
           "(threads = 64 .. 1024 in steps of 64 unless fixed; include/world_hip.h): modes 1, 2 at 2^6 .. 2^14, max_lr 3 or 4; 3 at "
           "2^6 .. 2^14, max_lr 3; 4, 5 at 2^6 .. 2^13, max_lr 4; 6 at 2^6 .. 2^13, max_lr 3; 7, 8, 9 at 2^10 .. 2^12, max_lr 3; 10 .. 13 "
           "at 2^12, max_lr 3, 256 threads; 14 .. 17 at 2^11 .. 2^14, max_lr 3, N / 16 threads; 18, 19 at lg_n 3 (rows of 8).  Swizzle 0 has modes "
           "1 .. 12, 18 and 19; swizzle 1 modes 1 (max_lr 3), 7 (2^11) and 13 .. 19.  Modes 7 .. 17 do not exist in the one-lane host emulation", mode, lg_n, max_lr, threads, swizzle);
  });
}

// d4c_frame's band selection in isolation (d4c.hip: d4c_select_probe), one workgroup per row of keys
int world_hip_probe_select(WorldHipContext *c, int mode, int threads, int K, long long rows, const double *d_keys, double *d_out) {
  return guarded(c, [&] {
    if (mode != 0 && mode != 1) fail("probe_select: mode %d unsupported (0: block_excluding_largest, 1: block_smallest_sum)", mode);
    if (threads != 128 && threads != 256 && threads != 512 && threads != 1024)
      fail("probe_select: threads = %d is not one of d4c_frame's workgroup sizes (128, 256, 512, 1024)", threads);
    if (K < 1 || K > 10 * threads) fail("probe_select: K = %d outside 1 .. %d (the keys of a row)", K, 10 * threads);
    if (rows < 0 || rows > 0x7FFFFFFFll) fail("probe_select: bad rows");
    if (!d_keys || !d_out) fail("probe_select: null buffer (%s)", !d_keys ? "keys" : "out");
    if (rows == 0) return;
    if (!launch_d4c_select_probe(mode, threads, K, (long)rows, d_keys, d_out, c->stream)) fail("probe_select: threads = %d has no kernel", threads);
  });
}

// Harvest's back half in isolation (harvest.hip: launch_harvest_tail -- hv_prune and the contour kernels, as launch_harvest
// ends), on candidates the caller made up: run_harvest's plan and carve of that half (plan_harvest_tail, carve_harvest_tail),
// the caller's candidates copied where hv_refine leaves its own, the workspace's rows copied out behind the last launch.
int world_hip_probe_harvest_contour(WorldHipContext *c, int n_utt, const int *nfb, const int *nc, int maxc, int fb_stride,
                                    const double *d_cand, const double *d_score, double frame_period, int f_stride,
                                    double *d_pruned_cand, double *d_pruned_score, double *d_step2, double *d_step3,
                                    double *d_step4, int sec_cap, int *d_sec_n, int *d_sec, double *d_basic_f0,
                                    double *d_tpos, double *d_f0) {
  return guarded(c, [&] {
    const char *const me = "probe_harvest_contour";
    if (n_utt <= 0 || n_utt > kGridY) fail("%s: n_utt = %d outside 1 .. %d", me, n_utt, kGridY);
    if (!nfb || !nc) fail("%s: null buffer (%s)", me, !nfb ? "nfb" : "nc");
    if (maxc < 7 || maxc > 256 || maxc % 7) fail("%s: maxc = %d is not a multiple of 7 in 7 .. 252 (256 slots is what the tracking kernel handles)", me, maxc);
    if (!(frame_period > 0)) fail("%s: frame_period must be positive", me);
    const struct { const void *p; const char *name; } bufs[] = {
        {d_cand, "cand"}, {d_score, "score"}, {d_pruned_cand, "pruned_cand"}, {d_pruned_score, "pruned_score"}, {d_step2, "step2"},
        {d_step3, "step3"}, {d_step4, "step4"}, {d_sec_n, "sec_n"}, {d_sec, "sec"}, {d_basic_f0, "basic_f0"}, {d_tpos, "tpos"}, {d_f0, "f0"}};
    for (const auto &b : bufs)
      if (!b.p) fail("%s: null buffer (%s)", me, b.name);
    HarvestParams p{};
    p.maxc = maxc; p.frame_period = frame_period;
    std::vector<int> fb(nfb, nfb + n_utt), cn(nc, nc + n_utt), nfr(n_utt);
    int max_fb = 0, max_fr = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (fb[u] < 1) fail("%s: nfb[%d] = %d: an utterance has at least one frame", me, u, fb[u]);
      if (cn[u] < 0 || cn[u] * 7 > maxc) fail("%s: nc[%d] = %d: 7 nc slots do not fit maxc = %d", me, u, cn[u], maxc);
      // Harvest()'s frame count (harvest.cpp:1219) of a signal that ends on 1 ms frame nfb - 1
      nfr[u] = static_cast<int>((fb[u] - 1) / frame_period) + 1;
      if (nfr[u] > f_stride) fail("%s: f_stride %d too small for %d frames", me, f_stride, nfr[u]);
      max_fb = std::max(max_fb, fb[u]); max_fr = std::max(max_fr, nfr[u]);
    }
    plan_harvest_tail(c, p, n_utt, max_fb);
    if (fb_stride != p.fb_stride) fail("%s: fb_stride = %d, the batch's is %d (max nfb rounded up to 8)", me, fb_stride, p.fb_stride);
    if (sec_cap != p.sec_cap) fail("%s: sec_cap = %d, the batch's is %d (max nfb / 2 + 4)", me, sec_cap, p.sec_cap);
    const size_t B = n_utt, row = p.fb_stride, cand_bytes = sizeof(double) * B * row * maxc;
    refuse_overlap(me,
                   {{d_pruned_cand, cand_bytes, "pruned_cand"}, {d_pruned_score, cand_bytes, "pruned_score"},
                    {d_step2, sizeof(double) * B * row, "step2"}, {d_step3, sizeof(double) * B * row, "step3"},
                    {d_step4, sizeof(double) * B * row, "step4"}, {d_basic_f0, sizeof(double) * B * row, "basic_f0"},
                    {d_sec_n, sizeof(int) * B * 2, "sec_n"}, {d_sec, sizeof(int) * B * 6 * p.sec_cap, "sec"},
                    {d_tpos, sizeof(double) * B * f_stride, "tpos"}, {d_f0, sizeof(double) * B * f_stride, "f0"}},
                   {{d_cand, cand_bytes, "cand"}, {d_score, cand_bytes, "score"}});
    begin_stage(c, [&](Arena &a) { carve_harvest_tail(a, p, B); });
    p.b.n_utt = n_utt; p.b.f_stride = f_stride;
    p.b.n_frames = upload(c, nfr);
    p.nfb = upload(c, fb);
    devrt::d2d(p.nc, upload(c, cn), sizeof(int) * B, c->stream);                  // (hv_detect's output in the product)
    for (size_t u = 0; u < B; ++u) {                                              // rows past nfb[u] stay the workspace's
      const size_t at = u * row * maxc, n = sizeof(double) * fb[u] * maxc;
      devrt::d2d(p.cand_b + at, d_cand + at, n, c->stream);
      devrt::d2d(p.score_b + at, d_score + at, n, c->stream);
    }
    p.tpos = d_tpos; p.f0 = d_f0;
    launch_harvest_tail(p, max_fb, max_fr, c->stream);
    for (size_t u = 0; u < B; ++u) {                                              // the rows of the utterance, no others
      const size_t at = u * row * maxc, n = sizeof(double) * fb[u] * maxc, f = u * row, nf = sizeof(double) * fb[u];
      if (cn[u]) {                                                                // (nc = 0: hv_prune has nothing to write)
        devrt::d2d(d_pruned_cand + at, p.cand_a + at, n, c->stream);
        devrt::d2d(d_pruned_score + at, p.score_a + at, n, c->stream);
      }
      devrt::d2d(d_step2 + f, p.c2 + f, nf, c->stream);
      devrt::d2d(d_step3 + f, p.c3 + f, nf, c->stream);
      devrt::d2d(d_step4 + f, p.c0 + f, nf, c->stream);
      devrt::d2d(d_basic_f0 + f, p.basic_f0 + f, nf, c->stream);
    }
    devrt::d2d(d_sec_n, p.sec_n, sizeof(int) * B * 2, c->stream);
    devrt::d2d(d_sec, p.sec, sizeof(int) * B * 6 * p.sec_cap, c->stream);
  });
}

// Harvest's middle in isolation (harvest.hip: launch_harvest_raw -- hv_compact_events and hv_raw_candidates, the body of
// launch_harvest's group loop behind the filter bank -- and launch_harvest_detect) on zero-crossing lists the caller made up:
// the event lists live in a workspace for ONE group of ev_group utterances, carved as run_harvest carves it, and every group's
// slice of the caller's lists is copied there before its launches (ev_u0 = 0, ev_group, 2 ev_group, ...).  raw, cand and nc are
// the caller's own arrays: the kernels write what they write in the product and nothing else.  nc is cleared here; in the
// product hv_remove_mean does that, launches earlier.
int world_hip_probe_harvest_candidates(WorldHipContext *c, int n_utt, const int *nfb, double afs, double f0_floor, double f0_ceil,
                                       int nch, const double *band_f0, int maxc, int fb_stride, int nseg, int seg_cap, int ev_cap,
                                       int ev_group, int stages, const double *d_seg_events, const int *d_seg_count,
                                       double *d_events, int *d_ev_count, double *d_raw, double *d_cand, int *d_nc) {
  return guarded(c, [&] {
    const char *const me = "probe_harvest_candidates";
    if (n_utt <= 0 || n_utt > kGridY) fail("%s: n_utt = %d outside 1 .. %d", me, n_utt, kGridY);
    if (stages <= 0 || (stages & ~7)) fail("%s: stages = %d: 1 compaction, 2 raw candidates, 4 detection", me, stages);
    if (nch < 12 || nch > 365) fail("%s: nch = %d outside 12 .. 365", me, nch);
    if (!nfb || !band_f0) fail("%s: null buffer (%s)", me, !nfb ? "nfb" : "band_f0");
    for (int j = 0; j < nch; ++j)
      if (!(band_f0[j] > 0)) fail("%s: band_f0[%d] is not positive", me, j);
    if (maxc != mround(nch / 10.0) * 7) fail("%s: maxc = %d, Harvest's is %d (round(nch / 10) * 7)", me, maxc, mround(nch / 10.0) * 7);
    if (!(afs > 0) || !(f0_floor > 0) || !(f0_ceil > f0_floor)) fail("%s: afs, f0_floor, f0_ceil must be positive and ascending", me);
    if (nseg < 1) fail("%s: nseg = %d: at least one segment list", me, nseg);
    if (seg_cap < 1) fail("%s: seg_cap = %d: a segment list holds at least one event", me, seg_cap);
    if (ev_cap < 1) fail("%s: ev_cap = %d: an event list holds at least one event", me, ev_cap);
    if (ev_group < 1) fail("%s: ev_group = %d: a group has at least one utterance", me, ev_group);
    const bool direct_lists = nseg == 1;                       // run_harvest's rule: the segment lists are the final lists
    if (direct_lists && seg_cap != ev_cap) fail("%s: seg_cap = %d, but with nseg = 1 the segment lists are the final lists of ev_cap = %d", me, seg_cap, ev_cap);
    if ((stages & 3) == 2 && !direct_lists) fail("%s: stages = %d: %d segment lists need the compaction (1) in front of the raw candidates (2)", me, stages, nseg);
    const bool reports_lists = (stages & 1) && !direct_lists;
    const struct { const void *p; bool needed; const char *name; } bufs[] = {
        {d_seg_events, (stages & 3) != 0, "seg_events"}, {d_seg_count, (stages & 3) != 0, "seg_count"}, {d_events, reports_lists, "events"},
        {d_ev_count, reports_lists, "ev_count"}, {d_raw, (stages & 6) != 0, "raw"}, {d_cand, (stages & 4) != 0, "cand"}, {d_nc, (stages & 4) != 0, "nc"}};
    for (const auto &b : bufs)
      if (b.needed && !b.p) fail("%s: null buffer (%s)", me, b.name);
    HarvestParams p{};
    p.afs = afs; p.f0_floor = f0_floor; p.f0_ceil = f0_ceil; p.nch = nch; p.maxc = maxc;
    p.nseg = nseg; p.seg_cap = seg_cap; p.ev_cap = ev_cap;
    p.fft_seg = direct_lists ? 1 : 0;                          // (launch_harvest_raw reads only its sign: with one segment list the FFT bank's direct lists)
    std::vector<int> fb(nfb, nfb + n_utt);
    int max_fb = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (fb[u] < 1) fail("%s: nfb[%d] = %d: an utterance has at least one frame", me, u, fb[u]);
      max_fb = std::max(max_fb, fb[u]);
    }
    plan_harvest_tail(c, p, n_utt, max_fb);
    if (fb_stride != p.fb_stride) fail("%s: fb_stride = %d, the batch's is %d (max nfb rounded up to 8)", me, fb_stride, p.fb_stride);
    const size_t B = n_utt, L = static_cast<size_t>(nch) * 4, row = p.fb_stride;
    p.ev_group = std::min(n_utt, ev_group);
    const size_t E = p.ev_group;
    refuse_overlap(me,
                   {{reports_lists ? d_events : nullptr, sizeof(double) * B * L * ev_cap, "events"},
                    {reports_lists ? d_ev_count : nullptr, sizeof(int) * B * L, "ev_count"},
                    {(stages & 2) ? d_raw : nullptr, sizeof(double) * B * nch * row, "raw"},
                    {(stages & 4) ? d_cand : nullptr, sizeof(double) * B * row * maxc, "cand"}, {(stages & 4) ? d_nc : nullptr, sizeof(int) * B, "nc"}},
                   {{(stages & 3) ? d_seg_events : nullptr, sizeof(double) * B * L * nseg * seg_cap, "seg_events"},
                    {(stages & 3) ? d_seg_count : nullptr, sizeof(int) * B * L * nseg, "seg_count"},
                    {(stages & 6) == 4 ? d_raw : nullptr, sizeof(double) * B * nch * row, "raw"}});
    if (stages & 3) {                                          // a count past its list's capacity would send a kernel out of bounds
      std::vector<int> cnt(B * L * nseg);
      devrt::d2h(cnt.data(), d_seg_count, sizeof(int) * cnt.size(), c->stream);
      devrt::sync(c->stream);
      for (size_t i = 0; i < cnt.size(); ++i)
        if (cnt[i] < 0 || cnt[i] > seg_cap) fail("%s: seg_count[%zu] = %d outside 0 .. seg_cap = %d", me, i, cnt[i], seg_cap);
    }
    begin_stage(c, [&](Arena &a) {                             // run_harvest's carve of the lists, for one group
      p.events = a.take<double>(E * L * ev_cap);
      p.ev_count = a.take<int>(E * L);
      if (direct_lists) {
        p.seg_events = p.events; p.seg_count = p.ev_count;
      } else {
        p.seg_events = a.take<double>(E * L * nseg * seg_cap);
        p.seg_count = a.take<int>(E * L * nseg);
      }
    });
    p.b.n_utt = n_utt;
    p.nfb = upload(c, fb);
    p.band_f0 = upload(c, band_f0, static_cast<size_t>(nch));
    p.raw = d_raw; p.cand_a = d_cand; p.nc = d_nc;
    std::vector<int> got;
    if (stages & 3)
      for (int u0 = 0; u0 < n_utt; u0 += p.ev_group) {         // launch_harvest's walk
        HarvestParams g = p;
        g.ev_u0 = u0;
        const int G = std::min(p.ev_group, n_utt - u0);
        devrt::d2d(p.seg_events, d_seg_events + u0 * L * nseg * seg_cap, sizeof(double) * G * L * nseg * seg_cap, c->stream);
        devrt::d2d(p.seg_count, d_seg_count + u0 * L * nseg, sizeof(int) * G * L * nseg, c->stream);
        launch_harvest_raw(g, G, max_fb, stages & 3, c->stream);
        if (reports_lists) {                                   // ev_count[list] events of every list, no more
          got.resize(G * L);
          devrt::d2h(got.data(), p.ev_count, sizeof(int) * got.size(), c->stream);
          devrt::sync(c->stream);
          for (size_t l = 0; l < got.size(); ++l)
            if (got[l] > 0)
              devrt::d2d(d_events + (u0 * L + l) * ev_cap, p.events + l * ev_cap, sizeof(double) * std::min(got[l], ev_cap), c->stream);
          devrt::d2d(d_ev_count + u0 * L, p.ev_count, sizeof(int) * got.size(), c->stream);
        }
      }
    if (stages & 4) {
      devrt::dzero(d_nc, sizeof(int) * B, c->stream);          // (hv_remove_mean's store in the product)
      launch_harvest_detect(p, max_fb, c->stream);
    }
  });
}

// Harvest's refinement in isolation (harvest.hip: launch_harvest_refine -- hv_refine or hv_refine_frames, what launch_harvest
// runs between detection and the tail) on a decimated signal and a candidate map the caller made up.  Tables, LDS size and route
// come from plan_harvest_refine as in run_harvest, the route from the argument instead of the environment.  The kernels read
// the caller's y and cand and write the caller's refined and score: slots below 7 nc[u] of frames below nfb[u], nothing else.
int world_hip_probe_harvest_refine(WorldHipContext *c, int n_utt, const int *y_len, const int *nfb, const int *nc, double afs,
                                   double f0_floor, double f0_ceil, int maxc, int fb_stride, int y_stride, int route,
                                   const double *d_y, const double *d_cand, double *d_refined, double *d_score) {
  return guarded(c, [&] {
    const char *const me = "probe_harvest_refine";
    if (n_utt <= 0 || n_utt > kGridY) fail("%s: n_utt = %d outside 1 .. %d", me, n_utt, kGridY);
    if (!y_len || !nfb || !nc) fail("%s: null buffer (%s)", me, !y_len ? "y_len" : !nfb ? "nfb" : "nc");
    if (!(afs >= 1000.0) || !(afs <= 48000.0)) fail("%s: afs outside 1000 .. 48000 Hz", me);
    if (!(f0_floor > 0) || !(f0_ceil > f0_floor) || !(f0_ceil < 1e300)) fail("%s: f0_floor, f0_ceil must be positive, ascending and finite", me);
    if (!(f0_floor <= afs / 2.0)) fail("%s: f0_floor above afs / 2: no candidate has a harmonic below the Nyquist frequency", me);
    if (route < 0 || route > 3) fail("%s: route = %d: 0 Harvest's own, 1 hv_refine, 2 hv_refine_frames on the table, 3 by rotation", me, route);
    if ((route == 1 || route == 2) && fmod(afs, 1000.0) != 0.0)
      fail("%s: route = %d needs the window table, which exists where a millisecond is a whole number of samples (afs)", me, route);
    if (maxc < 7 || maxc > 256 || maxc % 7) fail("%s: maxc = %d is not a multiple of 7 in 7 .. 252", me, maxc);
    const struct { const void *p; const char *name; } bufs[] = {{d_y, "y"}, {d_cand, "cand"}, {d_refined, "refined"}, {d_score, "score"}};
    for (const auto &b : bufs)
      if (!b.p) fail("%s: null buffer (%s)", me, b.name);
    HarvestParams p{};
    p.afs = afs; p.f0_floor = f0_floor; p.f0_ceil = f0_ceil; p.maxc = maxc; p.y_stride = y_stride;
    std::vector<int> yl(y_len, y_len + n_utt), fb(nfb, nfb + n_utt), cn(nc, nc + n_utt);
    int max_fb = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (fb[u] < 1) fail("%s: nfb[%d] = %d: an utterance has at least one frame", me, u, fb[u]);
      if (cn[u] < 0 || cn[u] * 7 > maxc) fail("%s: nc[%d] = %d: 7 nc slots do not fit maxc = %d", me, u, cn[u], maxc);
      if (yl[u] < 1 || yl[u] > y_stride) fail("%s: y_len[%d] = %d outside 1 .. y_stride = %d", me, u, yl[u], y_stride);
      max_fb = std::max(max_fb, fb[u]);
    }
    if (max_fb > (1 << 24)) fail("%s: nfb above 2^24 frames", me);
    p.fb_stride = (max_fb + 7) & ~7;
    if (fb_stride != p.fb_stride) fail("%s: fb_stride = %d, the batch's is %d (max nfb rounded up to 8)", me, fb_stride, p.fb_stride);
    // the longest window: its transform must have twiddles, and four wavefronts' LDS must fit a CU
    const int hw_floor = static_cast<int>(1.5 * afs / f0_floor + 1.0);
    if (2 + (31 - __builtin_clz(static_cast<unsigned>(2 * hw_floor + 1))) > kTwLog2) fail("%s: f0_floor: a window of %d samples needs a transform above 2^%d", me, 2 * hw_floor + 1, kTwLog2);
    const bool env_rotate = getenv("WORLD_HIP_REFINE_ROTATE") != nullptr, env_frames = getenv("WORLD_HIP_REFINE_FRAMES") != nullptr;
    plan_harvest_refine(c, p, route == 0 ? env_rotate : route == 3, route == 0 ? env_frames : route == 2);
    if (4 * hv_refine_lds_bytes(p) > 160 * 1024) fail("%s: f0_floor: windows of %d samples do not fit the LDS", me, 2 * hw_floor + 1);
    const size_t B = n_utt, row = p.fb_stride, map_elems = B * row * maxc;
    refuse_overlap(me, {{d_refined, sizeof(double) * map_elems, "refined"}, {d_score, sizeof(double) * map_elems, "score"}},
                   {{d_y, sizeof(double) * B * y_stride, "y"}, {d_cand, sizeof(double) * map_elems, "cand"}});
    {                                                          // a candidate outside the domain would send a kernel out of its tables
      std::vector<double> cand(map_elems);
      devrt::d2h(cand.data(), d_cand, sizeof(double) * map_elems, c->stream);
      devrt::sync(c->stream);
      const double top = std::min(f0_ceil, afs / 2.0);
      for (size_t u = 0; u < B; ++u)
        for (int f = 0; f < fb[u]; ++f)
          for (int j = 0; j < cn[u]; ++j) {
            const double v = cand[(u * row + f) * maxc + j];
            if (!(v == 0.0 || (v >= f0_floor && v <= top)))
              fail("%s: cand[%zu][%d][%d] = %g is neither 0 nor in f0_floor .. min(f0_ceil, afs / 2)", me, u, f, j, v);
          }
    }
    begin_stage(c, [](Arena &) {});
    p.b.n_utt = n_utt;
    p.y_len = upload(c, yl);
    p.nfb = upload(c, fb);
    p.nc = const_cast<int *>(upload(c, cn));                   // (hv_detect's output in the product; the refinement reads it)
    p.y = const_cast<double *>(d_y);
    p.cand_a = const_cast<double *>(d_cand);
    p.cand_b = d_refined; p.score_b = d_score;
    launch_harvest_refine(p, max_fb, c->stream);
  });
}

int world_hip_pack_results(WorldHipContext *c, int n_utt, const int *n_frames, int f_stride, int bins,
                           const double *d_tpos, const double *d_f0, const double *d_spectrogram,
                           const double *d_aperiodicity, long long first_row, double *d_block) {
  return guarded(c, [&] {
    run_pack(c, false, n_utt, n_frames, f_stride, bins, d_tpos, d_f0, d_spectrogram, d_aperiodicity, first_row, d_block);
  });
}

int world_hip_unpack_results(WorldHipContext *c, int n_utt, const int *n_frames, int f_stride, int bins,
                             const double *d_block, long long first_row, double *d_tpos, double *d_f0,
                             double *d_spectrogram, double *d_aperiodicity) {
  return guarded(c, [&] {
    run_pack(c, true, n_utt, n_frames, f_stride, bins, d_tpos, d_f0, d_spectrogram, d_aperiodicity, first_row,
             const_cast<double *>(d_block));
  });
}

// One process, n_dev contexts (normally one per GPU): every context's packed block to every context.
// Fully stream-ordered: destination d waits (on its own stream) for source s's block to be complete, pulls it
// with a peer copy, and source s's stream in turn waits until every destination has pulled -- so the caller may
// reuse the source blocks in stream order without ever synchronising the host.
int world_hip_allgather_blocks(int n_dev, WorldHipContext *const *ctxs, const double *const *d_src, const long long *rows,
                               int cols, double *const *d_dst) {
  try {
    if (n_dev <= 0 || !ctxs || !d_src || !rows || !d_dst || cols <= 0) fail("bad arguments");
    std::vector<long long> first(n_dev + 1, 0);
    for (int d = 0; d < n_dev; ++d) {
      if (!ctxs[d] || rows[d] < 0 || (rows[d] > 0 && !d_src[d]) || !d_dst[d]) fail("bad block %d", d);
      for (int e = 0; e < d; ++e)
        if (ctxs[e] == ctxs[d]) fail("context %d listed twice", d);
      first[d + 1] = first[d] + rows[d];
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    {                                                       // a fixed global order keeps concurrent callers deadlock-free
      std::vector<WorldHipContext *> order(ctxs, ctxs + n_dev);
      std::sort(order.begin(), order.end());
      for (WorldHipContext *c : order) locks.emplace_back(c->lock);
    }
    for (int s = 0; s < n_dev; ++s) {
      WorldHipContext *c = ctxs[s];
      DeviceScope on_device(c->device);
      if (!c->xchg_ready) { c->xchg_ready = devrt::event_create(); c->xchg_done = devrt::event_create(); }
      for (int d = 0; d < n_dev; ++d) devrt::enable_peer_access(c->device, ctxs[d]->device);
      devrt::event_record(c->xchg_ready, c->stream);
    }
    for (int d = 0; d < n_dev; ++d) {
      WorldHipContext *c = ctxs[d];
      DeviceScope on_device(c->device);
      // remote blocks first, starting with the neighbour: destinations then pull from different sources at any moment
      for (int k = 1; k <= n_dev; ++k) {
        const int s = (d + k) % n_dev;
        if (s != d) devrt::stream_wait_event(c->stream, ctxs[s]->xchg_ready);
        devrt::peer_copy(d_dst[d] + first[s] * cols, c->device, d_src[s], ctxs[s]->device,
                         sizeof(double) * (size_t)rows[s] * cols, c->stream);
      }
      devrt::event_record(c->xchg_done, c->stream);
    }
    for (int s = 0; s < n_dev; ++s) {
      DeviceScope on_device(ctxs[s]->device);
      for (int d = 0; d < n_dev; ++d)
        if (d != s) devrt::stream_wait_event(ctxs[s]->stream, ctxs[d]->xchg_done);
    }
    return 0;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return 1;
  }
}

// Sub-batch sizes of a device's share of n utterances (world_amd/distributed.py: chunk_sizes states the same schedule):
// full sub-batches of sb, and the LAST one tapered into halves (sb/2, sb/4, sb/4) -- sub-batch k's exchange runs under the
// analysis of k + 1, so only the last exchange is exposed, and tapering shrinks it from 1/4 of a 128-utterance share to
// 1/16.  Tails of fewer than 8 utterances stay whole (smaller batches stop filling the chip).
static std::vector<int> chunk_sizes(int n, int sb) {
  std::vector<int> out;
  sb = std::max(1, sb);
  while (n > sb) { out.push_back(sb); n -= sb; }
  if (n >= 8 && !getenv("WORLD_HIP_NO_TAPER")) {
    const int a = (n + 1) / 2, b = (n - a + 1) / 2, c = n - a - b;
    out.push_back(a);
    if (b > 0) out.push_back(b);
    if (c > 0) out.push_back(c);
  } else if (n > 0) {
    out.push_back(n);
  }
  return out;
}

// One PROCESS, n_dev GPUs ("one host thread + stream per GPU"): the C/C++ counterpart of
// world_amd/distributed.py.  Utterances (host memory) are partitioned longest-first over the contexts' devices; a host
// thread per device uploads its share in sub-batches (pinned double buffer), analyses each straight into packed records
// (world_hip_analyze_packed) at the sub-batch's rows of ITS copy of the job's one record block, and as soon as a
// sub-batch is enqueued every other device pulls those rows over xGMI on its own exchange stream (peer copies by the
// copy engines) -- the exchange of sub-batch k runs under the analysis of sub-batch k + 1.  Every device ends up with
// ALL records at identical offsets.  where[3 i .. 3 i + 2] = {device index, first row, n_frames} of utterance i.
// Returns when every device's block is complete (the streams are synchronised: the inputs are host memory anyway).
int world_hip_analyze_sharded(int n_dev, WorldHipContext *const *ctxs, int n_utt, int fs, const double *const *x,
                              const int *x_length, const HarvestOption *hopt, const CheapTrickOption *copt,
                              const D4COption *dopt, int sub_batch, double *const *d_blocks, long long rows_capacity, int cols,
                              long long *where) {
  try {
    if (n_dev <= 0 || !ctxs || n_utt < 0 || !x_length || !hopt || !copt || !dopt || !d_blocks || !where) fail("bad arguments");
    if (n_utt > 0 && !x) fail("null input");
    if (cols != record_cols(copt->fft_size, 0) && cols != record_cols(copt->fft_size, 1))
      fail("analyze_sharded: %d columns do not fit fft_size %d (%d for f64 records, %d for f32 spectra)", cols, copt->fft_size,
           record_cols(copt->fft_size, 0), record_cols(copt->fft_size, 1));
    for (int d = 0; d < n_dev; ++d) {
      if (!ctxs[d] || !d_blocks[d]) fail("bad device entry %d", d);
      for (int e = 0; e < d; ++e) {
        if (ctxs[e] == ctxs[d]) fail("context %d listed twice", d);
        if (d_blocks[e] == d_blocks[d]) fail("devices %d and %d share a block", e, d);
      }
    }
    const int sb = std::max(1, sub_batch);
    // greedy longest-first partition (world_amd/distributed.py: partition), utterances of a device in index order
    std::vector<int> order(n_utt);
    for (int i = 0; i < n_utt; ++i) {
      if (x_length[i] <= 0 || !x[i]) fail("utterance %d is empty", i);
      order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return x_length[a] > x_length[b]; });
    std::vector<std::vector<int>> part(n_dev);
    std::vector<long long> load(n_dev, 0);
    for (int i : order) {
      int r = 0;
      for (int d = 1; d < n_dev; ++d) if (load[d] < load[r]) r = d;
      part[r].push_back(i);
      load[r] += x_length[i];
    }
    // rows: device after device, sub-batch after sub-batch, utterance after utterance
    struct Chunk { int dev, lo, hi; long long first, rows; int max_len; };
    std::vector<Chunk> chunks;
    long long row = 0;
    for (int r = 0; r < n_dev; ++r) {
      std::sort(part[r].begin(), part[r].end());
      size_t lo = 0;
      for (int take : chunk_sizes((int)part[r].size(), sb)) {
        Chunk c{r, (int)lo, (int)(lo + take), row, 0, 0};
        lo += take;
        for (int j = c.lo; j < c.hi; ++j) {
          const int i = part[r][j], nf = frame_count(fs, x_length[i], hopt->frame_period);
          where[3 * i] = r; where[3 * i + 1] = row; where[3 * i + 2] = nf;
          row += nf;
          c.max_len = std::max(c.max_len, x_length[i]);
        }
        c.rows = row - c.first;
        chunks.push_back(c);
      }
    }
    if (row > rows_capacity) fail("analyze_sharded: the job has %lld records, the blocks hold %lld", row, rows_capacity);
    if (n_utt == 0) return 0;
    std::vector<std::unique_lock<std::mutex>> locks;
    {                                                       // a fixed global order keeps concurrent callers deadlock-free
      std::vector<WorldHipContext *> ord(ctxs, ctxs + n_dev);
      std::sort(ord.begin(), ord.end());
      for (WorldHipContext *c : ord) locks.emplace_back(c->lock);
    }
    // per-device set-up on the calling thread: exchange stream, peer access, one event per sub-batch
    std::vector<void *> done(chunks.size(), nullptr);
    for (int d = 0; d < n_dev; ++d) {
      WorldHipContext *c = ctxs[d];
      DeviceScope on_device(c->device);
      if (!c->xstream) c->xstream = devrt::stream_create();
      for (int e = 0; e < n_dev; ++e) devrt::enable_peer_access(c->device, ctxs[e]->device);
    }
    for (size_t k = 0; k < chunks.size(); ++k) {
      DeviceScope on_device(ctxs[chunks[k].dev]->device);
      done[k] = devrt::event_create();
    }
    std::vector<std::string> errors(n_dev);
    std::mutex xlock;                                       // enqueues on another device's exchange stream, one thread at a time
    auto worker = [&](int r) {
      WorldHipContext *c = ctxs[r];
      try {
        devrt::set_device(c->device);
        size_t need = 0;
        for (const Chunk &ch : chunks) if (ch.dev == r) need = std::max(need, (size_t)(ch.hi - ch.lo) * ch.max_len);
        if (need > c->xin_cap) {
          devrt::sync(c->stream);
          if (c->d_xin) devrt::dfree(c->d_xin);
          if (c->h_xin) devrt::hfree_pinned(c->h_xin);
          c->xin_cap = need + need / 8;
          c->d_xin = static_cast<double *>(devrt::dmalloc(sizeof(double) * 2 * c->xin_cap));
          c->h_xin = static_cast<double *>(devrt::hmalloc_pinned(sizeof(double) * 2 * c->xin_cap));
        }
        void *staged[2] = {devrt::event_create(), devrt::event_create()};   // half h of the staging buffers is free again
        int turn = 0;
        for (size_t k = 0; k < chunks.size(); ++k) {
          const Chunk &ch = chunks[k];
          if (ch.dev != r) continue;
          const int b = ch.hi - ch.lo, half = turn & 1;
          if (turn >= 2) devrt::event_sync(staged[half]);  // the analysis that read this half two sub-batches ago is done
          double *h = c->h_xin + (size_t)half * c->xin_cap, *dx = c->d_xin + (size_t)half * c->xin_cap;
          std::vector<int> xl(b);
          for (int j = 0; j < b; ++j) {
            const int i = part[r][ch.lo + j];
            xl[j] = x_length[i];
            memcpy(h + (size_t)j * ch.max_len, x[i], sizeof(double) * x_length[i]);
            if (x_length[i] < ch.max_len) memset(h + (size_t)j * ch.max_len + x_length[i], 0, sizeof(double) * (ch.max_len - x_length[i]));
          }
          devrt::dpoison(dx, sizeof(double) * c->xin_cap, c->stream);
          devrt::h2d(dx, h, sizeof(double) * (size_t)b * ch.max_len, c->stream);
          run_analyze_packed(c, b, fs, dx, ch.max_len, xl.data(), hopt, copt, dopt, ch.first, d_blocks[r], cols);
          devrt::event_record(staged[half], c->stream);
          devrt::event_record(done[k], c->stream);
          ++turn;
          // every other device pulls this sub-batch's rows on its exchange stream, the neighbour first
          std::lock_guard<std::mutex> g(xlock);
          for (int s = 1; s < n_dev; ++s) {
            const int d = (r + s) % n_dev;
            DeviceScope on_dst(ctxs[d]->device);
            devrt::stream_wait_event(ctxs[d]->xstream, done[k]);
            devrt::peer_copy(d_blocks[d] + ch.first * cols, ctxs[d]->device, d_blocks[r] + ch.first * cols, c->device,
                             sizeof(double) * (size_t)ch.rows * cols, ctxs[d]->xstream);
          }
        }
        devrt::sync(c->stream);
        devrt::event_destroy(staged[0]); devrt::event_destroy(staged[1]);
      } catch (const std::exception &e) {
        errors[r] = e.what();
      }
    };
    std::vector<std::thread> threads;
    for (int r = 1; r < n_dev; ++r) threads.emplace_back(worker, r);
    const int before = devrt::current_device();
    worker(0);                                              // the calling thread drives device 0
    for (std::thread &t : threads) t.join();
    for (int d = 0; d < n_dev; ++d) {
      try { devrt::set_device(ctxs[d]->device); devrt::sync(ctxs[d]->xstream); } catch (const std::exception &e) { if (errors[d].empty()) errors[d] = e.what(); }
    }
    for (size_t k = 0; k < chunks.size(); ++k) {
      try { devrt::set_device(ctxs[chunks[k].dev]->device); devrt::event_destroy(done[k]); } catch (...) {}
    }
    try { devrt::set_device(before); } catch (...) {}
    for (int d = 0; d < n_dev; ++d)
      if (!errors[d].empty()) fail("device %d: %s", d, errors[d].c_str());
    return 0;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return 1;
  }
}

int world_hip_pcm16_to_double(WorldHipContext *c, long long n, const short *d_pcm, double *d_x) {
  return guarded(c, [&] {
    if (n < 0) fail("negative sample count");
    if (n > 0 && (!d_pcm || !d_x)) fail("null buffer");
    if (n > 0) launch_pcm16_to_double(d_pcm, d_x, (long)n, c->stream);
  });
}

int world_hip_f0_statistics(WorldHipContext *c, int n_utt, const int *n_frames, int f_stride, const double *d_f0,
                            double *d_stats) {
  return guarded(c, [&] { run_f0_statistics(c, n_utt, n_frames, f_stride, d_f0, d_stats); });
}
int world_hip_modify_batch(WorldHipContext *c, int n_utt, int fs, int fft_size, const int *n_frames, int f_stride,
                           const WorldHipModification *mods, const double *d_f0_in, double *d_f0_out, const double *d_sp_in,
                           double *d_sp_out) {
  return guarded(c, [&] {
    run_modify(c, n_utt, fs, fft_size, n_frames, f_stride, mods, d_f0_in, d_f0_out, d_sp_in, d_sp_out);
  });
}
int world_hip_modify_frames_batch(WorldHipContext *c, int n_utt, int fs, int fft_size, const int *n_frames, int f_stride,
                                  const int *n_out, int o_stride, const WorldHipModification *mods,
                                  const WorldHipFrameCurves *curves, const double *d_f0_in, double *d_f0_out,
                                  const double *d_sp_in, double *d_sp_out, const double *d_ap_in, double *d_ap_out) {
  return guarded(c, [&] {
    run_modify_frames(c, n_utt, fs, fft_size, n_frames, f_stride, n_out, o_stride, mods, curves, d_f0_in, d_f0_out, d_sp_in,
                      d_sp_out, d_ap_in, d_ap_out);
  });
}
int world_hip_resynthesize_frames_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride,
                                        const int *x_length, const HarvestOption *harvest_option,
                                        const CheapTrickOption *cheaptrick_option, const D4COption *d4c_option,
                                        const WorldHipModification *mods, const WorldHipFrameCurves *curves, const int *n_out,
                                        int o_stride, const int *y_length, int y_stride, double *d_y) {
  return guarded(c, [&] {
    run_resynthesis_frames(c, n_utt, fs, d_x, x_stride, x_length, harvest_option, cheaptrick_option, d4c_option, mods, curves,
                           n_out, o_stride, y_length, y_stride, d_y);
  });
}
int world_hip_align_batch(WorldHipContext *c, int n_pairs, int n_dims, const double *d_a, const long long *a_row,
                          const int *n_a, int a_row_stride, const double *d_b, const long long *b_row, const int *n_b,
                          int b_row_stride, int p_stride, int *d_path, int *d_path_len, double *d_summary, int map_stride,
                          double *d_map_b, double *d_map_a) {
  return guarded(c, [&] {
    run_align(c, n_pairs, n_dims, d_a, a_row, n_a, a_row_stride, d_b, b_row, n_b, b_row_stride, p_stride, d_path, d_path_len,
              d_summary, map_stride, d_map_b, d_map_a);
  });
}
int world_hip_align_workspace_cells(void) { return (int)kAlignCells; }
int world_hip_morph_length(int n_a, int n_b, double time_rate) { return morph_length(n_a, n_b, time_rate); }
int world_hip_morph_batch(WorldHipContext *c, int n_pairs, int fs, int fft_size, const int *n_a, int a_stride,
                          const double *d_f0_a, const double *d_sp_a, const double *d_ap_a, const int *n_b, int b_stride,
                          const double *d_f0_b, const double *d_sp_b, const double *d_ap_b, int p_stride, const int *d_path,
                          const int *d_path_len, const WorldHipMorph *morphs, const WorldHipMorphCurves *curves, int o_stride,
                          double *d_f0_out, double *d_sp_out, double *d_ap_out, double *d_pos_a, double *d_pos_b) {
  return guarded(c, [&] {
    run_morph(c, n_pairs, fs, fft_size, n_a, a_stride, d_f0_a, d_sp_a, d_ap_a, n_b, b_stride, d_f0_b, d_sp_b, d_ap_b, p_stride,
              d_path, d_path_len, morphs, curves, o_stride, d_f0_out, d_sp_out, d_ap_out, d_pos_a, d_pos_b);
  });
}
void world_hip_resample_option(int quality, WorldHipResampleOption *opt) {
  if (!opt) return;
  if (quality == WORLD_HIP_RESAMPLE_FAST) *opt = WorldHipResampleOption{16, 0.85, 8.555504641634386};
  else *opt = WorldHipResampleOption{64, 0.9475937167399596, 14.769656459379492};
}
int world_hip_resample_length(int n_in, int fs_in, int fs_out) { return resample_length(n_in, fs_in, fs_out); }
int world_hip_resample_shape(int fs_in, int fs_out, const WorldHipResampleOption *opt, int *L, int *M, int *W) {
  ResampleShape sh;
  if (const char *why = resample_shape(fs_in, fs_out, resample_design(opt), &sh)) {
    g_last_error = std::string("resample: ") + why;
    return 1;
  }
  if (L) *L = (int)sh.L;
  if (M) *M = (int)sh.M;
  if (W) *W = (int)sh.W;
  return 0;
}
int world_hip_resample_taps(int fs_in, int fs_out, const WorldHipResampleOption *opt, double *table) {
  ResampleShape sh;
  const ResampleDesign design = resample_design(opt);
  if (const char *why = resample_shape(fs_in, fs_out, design, &sh)) {
    g_last_error = std::string("resample: ") + why;
    return 1;
  }
  if (!table) { g_last_error = "resample: null table"; return 1; }
  build_resample_taps(sh, design, table);
  return 0;
}
int world_hip_resample_batch(WorldHipContext *c, int n_utt, int fs_in, int fs_out, const WorldHipResampleOption *opt,
                             const double *d_x, int x_stride, const int *x_length, double *d_y, int y_stride) {
  return guarded(c, [&] { run_resample(c, n_utt, fs_in, fs_out, opt, d_x, x_stride, x_length, d_y, y_stride); });
}
double world_hip_mcep_alpha(int fs) { return mcep_alpha(fs); }
int world_hip_mcep_tables(int fft_size, int order, double alpha, double *M, double *D) {
  if (const char *why = mcep_shape(fft_size, order, alpha)) {
    g_last_error = std::string("mcep: ") + why;
    return 1;
  }
  if (M) build_mcep_encode(fft_size, order, alpha, M);
  if (D) build_mcep_decode(fft_size, order, alpha, D);
  return 0;
}
int world_hip_sp2mc(WorldHipContext *c, int rows, int fft_size, int order, double alpha, const double *d_sp,
                    long long sp_row_stride, double *d_mc, long long mc_row_stride) {
  return guarded(c, [&] { run_mcep(c, false, rows, fft_size, order, alpha, d_sp, sp_row_stride, d_mc, mc_row_stride); });
}
int world_hip_mc2sp(WorldHipContext *c, int rows, int fft_size, int order, double alpha, const double *d_mc,
                    long long mc_row_stride, double *d_sp, long long sp_row_stride) {
  return guarded(c, [&] { run_mcep(c, true, rows, fft_size, order, alpha, d_mc, mc_row_stride, d_sp, sp_row_stride); });
}
int world_hip_delta_batch(WorldHipContext *c, int n_utt, int dim, int n_win, int half_width, const double *win,
                          const int *n_frames, const unsigned char *d_mask, long long mask_utt_stride, const double *d_c,
                          long long c_utt_stride, long long c_row_stride, double fill, double *d_out,
                          long long out_utt_stride, long long out_row_stride) {
  return guarded(c, [&] {
    run_delta(c, n_utt, dim, n_win, half_width, win, n_frames, d_mask, mask_utt_stride, d_c, c_utt_stride, c_row_stride, fill,
              d_out, out_utt_stride, out_row_stride);
  });
}
int world_hip_mlpg_batch(WorldHipContext *c, int n_utt, int dim, int n_win, int half_width, const double *win,
                         const int *n_frames, const unsigned char *d_mask, long long mask_utt_stride, const double *d_mean,
                         long long mean_utt_stride, long long mean_row_stride, const double *d_var, long long var_utt_stride,
                         long long var_row_stride, int precision, double fill, double *d_out, long long out_utt_stride,
                         long long out_row_stride) {
  return guarded(c, [&] {
    run_mlpg(c, n_utt, dim, n_win, half_width, win, n_frames, d_mask, mask_utt_stride, d_mean, mean_utt_stride,
             mean_row_stride, d_var, var_utt_stride, var_row_stride, precision, fill, d_out, out_utt_stride, out_row_stride);
  });
}
// the host calls of the mixture: 0, or 1 with the reason in world_hip_last_error
static int gmm_host_call(const std::string &why) {
  if (why.empty()) return 0;
  g_last_error = why;
  return 1;
}
long long world_hip_gmm_model_doubles(int M, int Dx, int Dy) {
  if (const char *why = gmm_shape(M, Dx, Dy)) { g_last_error = std::string("gmm: ") + why; return -1; }
  return (long long)gmm_layout(M, Dx, Dy).doubles;
}
int world_hip_gmm_prepare(int M, int Dx, int Dy, const double *w, const double *mu, const double *cov, double *model) {
  if (const char *why = gmm_shape(M, Dx, Dy)) return gmm_host_call(std::string("gmm_prepare: ") + why);
  if (!w || !mu || !cov || !model) return gmm_host_call("gmm_prepare: null w / mu / cov / model");
  const std::string why = gmm_prepare_host(M, Dx, Dy, w, mu, cov, model);
  return gmm_host_call(why.empty() ? why : "gmm_prepare: " + why);
}
int world_hip_gmm_model_parts(int M, int Dx, int Dy, const double *model, double *c, double *mux, double *muy, double *U,
                              double *A, double *v) {
  if (const char *why = gmm_shape(M, Dx, Dy)) return gmm_host_call(std::string("gmm_model_parts: ") + why);
  if (!model) return gmm_host_call("gmm_model_parts: null model");
  const GmmLayout g = gmm_layout(M, Dx, Dy);
  for (int m = 0; m < M; ++m) {
    if (c) c[m] = model[g.c + m];
    for (int k = 0; k < Dx; ++k) {
      if (mux) mux[(size_t)m * Dx + k] = model[g.mux + (size_t)m * g.Kp + k];
      for (int j = 0; j < Dx; ++j)
        if (U) U[((size_t)m * Dx + j) * Dx + k] = model[g.ut + ((size_t)m * g.Kp + k) * g.Kp + j];
      for (int i = 0; i < Dy; ++i)
        if (A) A[((size_t)m * Dy + i) * Dx + k] = model[g.at + ((size_t)m * g.Kp + k) * g.Ep + i];
    }
    for (int i = 0; i < Dy; ++i) {
      if (muy) muy[(size_t)m * Dy + i] = model[g.muy + (size_t)m * g.Ep + i];
      if (v) v[(size_t)m * Dy + i] = model[g.v + (size_t)m * g.Ep + i];
    }
  }
  return 0;
}
int world_hip_gmm_update(int M, int P, const double *N, const double *S1, const double *G, const double *shift,
                         double total_rows, double reg, double *w, double *mu, double *cov) {
  if (M < 1 || M > kGmmMaxMix || P < 1 || P > kGmmMaxDim) return gmm_host_call("gmm_update: M or P out of range");
  if (!N || !S1 || !G || !shift || !w || !mu || !cov) return gmm_host_call("gmm_update: null N / S1 / G / shift / w / mu / cov");
  if (!std::isfinite(reg) || reg < 0) return gmm_host_call("gmm_update: reg must be finite and not negative");
  if (!std::isfinite(total_rows) || !(total_rows > 0)) return gmm_host_call("gmm_update: total_rows must be finite and positive");
  const std::string why = gmm_update_host(M, P, N, S1, G, shift, total_rows, reg, w, mu, cov);
  return gmm_host_call(why.empty() ? why : "gmm_update: " + why);
}
int world_hip_gmm_convert(WorldHipContext *c, int M, int Dx, int Dy, const double *d_model, int rows, const double *d_x,
                          long long x_row_stride, int mode, double *d_mean, long long mean_row_stride, double *d_var,
                          long long var_row_stride, double *d_post, long long post_row_stride, double *d_loglik) {
  return guarded(c, [&] {
    run_gmm_convert(c, M, Dx, Dy, d_model, rows, d_x, x_row_stride, mode, d_mean, mean_row_stride, d_var, var_row_stride, d_post,
                    post_row_stride, d_loglik);
  });
}
int world_hip_gmm_accumulate(WorldHipContext *c, int M, int P, int rows, const double *d_z, long long z_row_stride,
                             const double *d_post, long long post_row_stride, const double *d_shift, double *d_N, double *d_S1,
                             double *d_G) {
  return guarded(c, [&] { run_gmm_accumulate(c, M, P, rows, d_z, z_row_stride, d_post, post_row_stride, d_shift, d_N, d_S1, d_G); });
}
int world_hip_gmm_fit(WorldHipContext *c, int M, int P, int rows, const double *d_z, long long z_row_stride, int n_iter,
                      double reg, double *w, double *mu, double *cov, double *loglik) {
  return guarded(c, [&] { run_gmm_fit(c, M, P, rows, d_z, z_row_stride, n_iter, reg, w, mu, cov, loglik); });
}
int world_hip_gmm_init(WorldHipContext *c, int M, int P, int rows, const double *d_z, long long z_row_stride, double *w,
                       double *mu, double *cov) {
  return guarded(c, [&] { run_gmm_init(c, M, P, rows, d_z, z_row_stride, w, mu, cov); });
}
int world_hip_frame_power_batch(WorldHipContext *c, int n_utt, int fft_size, const int *n_frames, const double *d_sp,
                                long long sp_utt_stride, long long sp_row_stride, double *d_power, long long power_utt_stride,
                                double *d_mean) {
  return guarded(c, [&] { run_frame_power(c, n_utt, fft_size, n_frames, d_sp, sp_utt_stride, sp_row_stride, d_power, power_utt_stride, d_mean); });
}
int world_hip_select_frames_batch(WorldHipContext *c, int n_utt, const int *n_frames, const double *d_value,
                                  long long value_utt_stride, long long value_stride, double threshold, const double *d_scale,
                                  const unsigned char *d_mask, long long mask_utt_stride, int *d_index, long long index_utt_stride,
                                  int *d_count, unsigned char *d_keep, long long keep_utt_stride) {
  return guarded(c, [&] {
    run_select_frames(c, n_utt, n_frames, d_value, value_utt_stride, value_stride, threshold, d_scale, d_mask, mask_utt_stride,
                      d_index, index_utt_stride, d_count, d_keep, keep_utt_stride);
  });
}
int world_hip_gather_rows_batch(WorldHipContext *c, int n_utt, int dim, const int *n_src, const double *d_in,
                                long long in_utt_stride, long long in_row_stride, const int *n_out, const int *d_index,
                                long long index_utt_stride, double fill, double *d_out, long long out_utt_stride,
                                long long out_row_stride) {
  return guarded(c, [&] {
    run_gather_rows(c, n_utt, dim, n_src, d_in, in_utt_stride, in_row_stride, n_out, d_index, index_utt_stride, fill, d_out,
                    out_utt_stride, out_row_stride);
  });
}
int world_hip_joint_rows_batch(WorldHipContext *c, int n_pairs, int dim_a, int dim_b, const double *d_a, const long long *a_row,
                               const int *n_a, long long a_row_stride, const double *d_b, const long long *b_row, const int *n_b,
                               long long b_row_stride, const int *path_len, const int *d_path, int p_stride, const int *d_sel_a,
                               const int *n_sel_a, long long sel_a_stride, const int *d_sel_b, const int *n_sel_b,
                               long long sel_b_stride, double fill, double *d_z, const long long *z_row, long long z_row_stride) {
  return guarded(c, [&] {
    run_joint_rows(c, n_pairs, dim_a, dim_b, d_a, a_row, n_a, a_row_stride, d_b, b_row, n_b, b_row_stride, path_len, d_path, p_stride,
                   d_sel_a, n_sel_a, sel_a_stride, d_sel_b, n_sel_b, sel_b_stride, fill, d_z, z_row, z_row_stride);
  });
}
int world_hip_resynthesis_length(int fs, int n_frames, double frame_period, double time_scale) {
  if (fs <= 0 || n_frames < 1 || !std::isfinite(frame_period) || !(frame_period > 0) || !std::isfinite(time_scale) ||
      !(time_scale > 0))
    return 0;
  const double y = (n_frames - 1) * frame_period * time_scale / 1000.0 * fs;
  if (!(y < 2147483646.0)) return 0;
  return resynthesis_length(fs, n_frames, frame_period, time_scale);
}
int world_hip_resynthesize_batch(WorldHipContext *c, int n_utt, int fs, const double *d_x, int x_stride, const int *x_length,
                                 const HarvestOption *harvest_option, const CheapTrickOption *cheaptrick_option,
                                 const D4COption *d4c_option, const WorldHipModification *mods, double time_scale,
                                 const int *y_length, int y_stride, double *d_y) {
  return guarded(c, [&] {
    run_resynthesis(c, n_utt, fs, d_x, x_stride, x_length, harvest_option, cheaptrick_option, d4c_option, mods, time_scale,
                    y_length, y_stride, d_y);
  });
}

int world_hip_code_spectral_envelope(WorldHipContext *c, int rows, int fs, int fft_size, int number_of_dimensions,
                                     const double *d_spectrogram, double *d_coded) {
  return guarded(c, [&] { run_codec(c, kCodeSp, rows, fs, fft_size, number_of_dimensions, d_spectrogram, d_coded); });
}
int world_hip_decode_spectral_envelope(WorldHipContext *c, int rows, int fs, int fft_size, int number_of_dimensions,
                                       const double *d_coded, double *d_spectrogram) {
  return guarded(c, [&] { run_codec(c, kDecodeSp, rows, fs, fft_size, number_of_dimensions, d_coded, d_spectrogram); });
}
int world_hip_code_aperiodicity(WorldHipContext *c, int rows, int fs, int fft_size, const double *d_aperiodicity,
                                double *d_coded) {
  return guarded(c, [&] { run_codec(c, kCodeAp, rows, fs, fft_size, 0, d_aperiodicity, d_coded); });
}
int world_hip_decode_aperiodicity(WorldHipContext *c, int rows, int fs, int fft_size, const double *d_coded,
                                  double *d_aperiodicity) {
  return guarded(c, [&] { run_codec(c, kDecodeAp, rows, fs, fft_size, 0, d_coded, d_aperiodicity); });
}

}  // extern "C"

#include "realtime.inc"
#include "dropin.inc"
#include "fileio.inc"
