// dropin.inc -- Part 1 of include/world_hip.h: the reference's host-pointer C API
// (SURVEY.md 8b) on top of the batched device path.  Caller-owned host buffers in,
// caller-owned host buffers out, so each call uploads x, runs the stage on the
// GPU and downloads the result.  There is no CPU fallback: a call that cannot run
// on the GPU reports through world_hip_set_error_handler()'s handler -- by default
// it prints the reason and aborts (the reference API has no error channel to report
// through), an embedding process may install one that records the failure and lets
// the call return with its outputs untouched.
//
// Re-entrancy (the reference is re-entrant: all state on the stack, src/cheaptrick.cpp:205-206,
// src/d4c.cpp:345-346).  A drop-in call runs on one SLOT of a small pool: a library context on a
// stream of its own, its device and pinned buffers, and the resident copy of the last input signal.
// K host threads therefore run K calls side by side (WORLD_HIP_DROPIN_SLOTS, default 4; round 3
// held one process-wide mutex for the whole of every call).

#include <atomic>
#include <condition_variable>
#include <chrono>
#include <deque>
#include <pthread.h>

namespace world_hip {

// host-side cost of the drop-in layer's own steps (WORLD_HIP_HOST_TRACE=1: printed at exit with devrt's call sites)
struct DropinTimed {
#ifndef WORLD_EMU
  const char *name;
  std::chrono::steady_clock::time_point t0;
  explicit DropinTimed(const char *n) : name(n) { if (devrt::g_host_trace) t0 = std::chrono::steady_clock::now(); }
  ~DropinTimed() {
    if (devrt::g_host_trace) devrt::host_trace_add(name, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
#else
  explicit DropinTimed(const char *) {}
#endif
};

// ---- error policy ------------------------------------------------------------------------
typedef void (*DropinErrorHandler)(const char *function, const char *message, void *user);
static std::mutex g_handler_lock;
static DropinErrorHandler g_handler = nullptr;
static void *g_handler_user = nullptr;
static void report_failure(const char *what, const std::string &msg) {
  DropinErrorHandler h; void *user;
  { std::lock_guard<std::mutex> g(g_handler_lock); h = g_handler; user = g_handler_user; }
  g_last_error = msg;
  if (h) { h(what, msg.c_str(), user); return; }   // may return (the drop-in call then returns, outputs untouched), longjmp or throw
  fprintf(stderr, "libworld_hip: %s failed: %s\n", what, msg.c_str());
  abort();
}

static void must(int rc, const char *what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + world_hip_last_error());
}

// ---- helper threads for host-side copies ---------------------------------------------------
// The 16 MB spectrogram of a 10 s utterance leaves pinned staging as 2001 rows of 8 KB; one core moves that at
// ~10 GB/s (1.6 ms, a third of round 3's whole drop-in sequence).  A few helper threads (WORLD_HIP_DROPIN_COPY_THREADS,
// default 3; 0 = none) share such copies with the calling thread, block by block through one atomic counter.  The
// caller always takes part and finishes the copy alone if no helper shows up (a forked child has none).
struct CopyTask {
  const char *src_base; const char *const *src_rows;   // row i: src_rows ? src_rows[i] : src_base + i * src_stride
  char *dst_base; char *const *dst_rows;               // row i: dst_rows ? dst_rows[i] : dst_base + i * row_bytes
  size_t row_bytes; int rows, grain;
  size_t src_stride = 0;                               // bytes between source rows (0: row_bytes)
  int widen = 0;                                       // > 0: a source row is `widen` floats, the destination row as many doubles
  std::atomic<int> next{0}, done{0}, users{0};
};
static void copy_task_work(CopyTask &t) {
  const size_t sstride = t.src_stride ? t.src_stride : t.row_bytes;
  for (;;) {
    const int r0 = t.next.fetch_add(t.grain, std::memory_order_relaxed);
    if (r0 >= t.rows) return;
    const int r1 = std::min(t.rows, r0 + t.grain);
    for (int i = r0; i < r1; ++i) {
      char *dst = t.dst_rows ? t.dst_rows[i] : t.dst_base + (size_t)i * t.row_bytes;
      const char *src = t.src_rows ? t.src_rows[i] : t.src_base + (size_t)i * sstride;
      if (t.widen > 0) {                                // the narrow download (WORLD_HIP_DROPIN_WIRE=f32): float -> double
        const float *f = reinterpret_cast<const float *>(src);
        double *d = reinterpret_cast<double *>(dst);
        for (int j = 0; j < t.widen; ++j) d[j] = static_cast<double>(f[j]);
      } else {
        memcpy(dst, src, t.row_bytes);
      }
    }
    t.done.fetch_add(r1 - r0, std::memory_order_release);
  }
}
struct CopyPool {
  std::mutex m;
  std::condition_variable cv;
  std::deque<CopyTask *> tasks;
  std::vector<std::thread> threads;               // joined by world_hip_shutdown()
  int started = -1;                               // helper threads running (-1: not yet decided)
  bool stop = false;
  // A matrix arrives as a handful of chunks ~100 us apart: a helper that went to sleep on the condition variable between
  // two of them wakes up 20-50 us late -- as long as its share of the chunk takes.  While a transfer is in progress
  // (sessions > 0) an idle helper MAY therefore poll `open` for spin_us microseconds after it last had work
  // (WORLD_HIP_DROPIN_SPIN_US) before it sleeps like outside transfers.  Default 0 -- it always sleeps: round 4 spun for the
  // whole session (three cores per transfer, its event waits included; ADVICE r04), and measured from the C++ caller the
  // spin buys under 1 % (10 s utterance, one call: 1.823 / 1.836 ms with 150 us of spinning, 1.841 / 1.849 ms with none).
  std::atomic<int> sessions{0}, open{0};
  int spin_us = 0;
  void helper() {
    std::unique_lock<std::mutex> lk(m);
    auto last_work = std::chrono::steady_clock::now();
    for (;;) {
      if (stop) return;
      CopyTask *t = nullptr;
      for (CopyTask *q : tasks) if (q->next.load(std::memory_order_relaxed) < q->rows) { t = q; break; }
      if (!t) {
        if (spin_us > 0 && sessions.load(std::memory_order_relaxed) > 0 &&
            std::chrono::steady_clock::now() - last_work < std::chrono::microseconds(spin_us)) {
          lk.unlock();
          for (int spin = 0; spin < 256 && open.load(std::memory_order_acquire) == 0; ++spin) __builtin_ia32_pause();
          lk.lock();
          continue;
        }
        cv.wait(lk);
        last_work = std::chrono::steady_clock::now();     // (woken for a task, a new session or shutdown: the window restarts)
        continue;
      }
      t->users.fetch_add(1, std::memory_order_relaxed);
      lk.unlock();
      copy_task_work(*t);
      t->users.fetch_sub(1, std::memory_order_release);
      lk.lock();
      last_work = std::chrono::steady_clock::now();
    }
  }
  void run(CopyTask &t) {
    DropinTimed t_("dropin:host_copy");
    const size_t bytes = t.row_bytes * (size_t)t.rows;
    bool shared = false;
    // (copies below 1 MB are the caller's alone; WORLD_HIP_DROPIN_COPY_MIN_BYTES: test hook)
    static const size_t min_bytes = [] { const char *e = getenv("WORLD_HIP_DROPIN_COPY_MIN_BYTES"); return e ? (size_t)atoll(e) : (size_t(1) << 20); }();
    if (bytes >= min_bytes) {
      std::lock_guard<std::mutex> g(m);
      if (started < 0) {
        const char *e = getenv("WORLD_HIP_DROPIN_COPY_THREADS");
        const int want = e ? std::max(0, std::min(16, atoi(e))) : 3;
        const char *su = getenv("WORLD_HIP_DROPIN_SPIN_US");
        if (su) spin_us = std::max(0, atoi(su));
        started = 0;
        for (int i = 0; i < want; ++i) {
          try { threads.emplace_back(&CopyPool::helper, this); ++started; } catch (...) { break; }
        }
      }
      if (started > 0) { tasks.push_back(&t); open.fetch_add(1, std::memory_order_release); shared = true; }
    }
    if (shared) cv.notify_all();
    copy_task_work(t);
    if (!shared) return;
    {                                               // no new helper may pick the task up ...
      std::lock_guard<std::mutex> g(m);
      for (auto it = tasks.begin(); it != tasks.end(); ++it) if (*it == &t) { tasks.erase(it); break; }
      open.fetch_sub(1, std::memory_order_release);
    }
    while (t.users.load(std::memory_order_acquire) != 0 || t.done.load(std::memory_order_acquire) < t.rows)
      std::this_thread::yield();                    // ... and those that did are in their last block
  }
  void shutdown() {                                 // joins the helpers; the next large copy starts new ones
    std::vector<std::thread> th;
    { std::lock_guard<std::mutex> g(m); stop = true; th.swap(threads); }
    cv.notify_all();
    for (std::thread &t : th) if (t.joinable()) t.join();
    std::lock_guard<std::mutex> g(m);
    stop = false; started = -1;
  }
};
struct CopySession {                               // a transfer of several chunks is in progress: helpers stay awake
  CopySession();
  ~CopySession();
};
// The pool is never destroyed (helpers may outlive static destruction).  A fork()ed child gets a FRESH one: the parent's
// helper threads do not exist there, and its mutex / queue may have been copied mid-operation (ADVICE r04: a child forked
// while a helper held the mutex deadlocked in run()).  The same for the slots below: their GPU state means nothing in the child.
static std::atomic<CopyPool *> g_copy_pool{nullptr};
static void dropin_after_fork_in_child();
// registered by whichever pool is created first (ADVICE r05: a process that had made slots but never touched the copy
// pool forked without the handler)
static void register_fork_handler() {
  static std::once_flag once;
  std::call_once(once, [] { pthread_atfork(nullptr, nullptr, dropin_after_fork_in_child); });
}
static CopyPool &copy_pool() {
  CopyPool *p = g_copy_pool.load(std::memory_order_acquire);
  if (!p) {
    static std::mutex once;
    std::lock_guard<std::mutex> g(once);
    p = g_copy_pool.load(std::memory_order_acquire);
    if (!p) {
      p = new CopyPool;
      register_fork_handler();
      g_copy_pool.store(p, std::memory_order_release);
    }
  }
  return *p;
}
CopySession::CopySession() { copy_pool().sessions.fetch_add(1, std::memory_order_relaxed); copy_pool().cv.notify_all(); }
CopySession::~CopySession() { copy_pool().sessions.fetch_sub(1, std::memory_order_relaxed); }
// dense bytes -> dense bytes in blocks of 256 KB
static void parallel_memcpy(void *dst, const void *src, size_t bytes) {
  const size_t blk = size_t(256) << 10;
  const int full = (int)(bytes / blk);
  if (full > 0) {
    CopyTask t;
    t.src_base = static_cast<const char *>(src); t.src_rows = nullptr;
    t.dst_base = static_cast<char *>(dst); t.dst_rows = nullptr;
    t.row_bytes = blk; t.rows = full; t.grain = 1;
    copy_pool().run(t);
  }
  if (bytes > (size_t)full * blk)
    memcpy(static_cast<char *>(dst) + (size_t)full * blk, static_cast<const char *>(src) + (size_t)full * blk, bytes - (size_t)full * blk);
}

// ---- the slots --------------------------------------------------------------------------------
// 64-bit content hash of the input signal (four independent multiply-xor lanes: ~1 word per cycle, a third of the time
// the upload it saves would take).  EVERY word takes part: a caller that edits a few samples in place between
// Harvest() and CheapTrick() gets the edited signal analysed, not the resident copy.
static uint64_t signal_hash(const double *x, int n) {
  DropinTimed t_("dropin:signal_hash");
  uint64_t h0 = 0x9E3779B97F4A7C15ull, h1 = 0xC2B2AE3D27D4EB4Full, h2 = 0x165667B19E3779F9ull, h3 = 0x27D4EB2F165667C5ull;
  const uint64_t K = 0xFF51AFD7ED558CCDull;
  const uint64_t *w = reinterpret_cast<const uint64_t *>(x);
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    uint64_t a, b, c, d;
    memcpy(&a, w + i, 8); memcpy(&b, w + i + 1, 8); memcpy(&c, w + i + 2, 8); memcpy(&d, w + i + 3, 8);
    h0 = (h0 ^ a) * K; h1 = (h1 ^ b) * K; h2 = (h2 ^ c) * K; h3 = (h3 ^ d) * K;
    h0 ^= h0 >> 29; h1 ^= h1 >> 31; h2 ^= h2 >> 30; h3 ^= h3 >> 28;
  }
  for (; i < n; ++i) { uint64_t a; memcpy(&a, w + i, 8); h0 = (h0 ^ a) * K; h0 ^= h0 >> 29; }
  uint64_t h = h0 ^ (h1 * 3) ^ (h2 * 5) ^ (h3 * 7) ^ (uint64_t)n;
  h ^= h >> 33; h *= K; h ^= h >> 33;
  return h;
}

struct DropinSlot {
  static constexpr int kBufs = 8;
  WorldHipContext *ctx = nullptr;
  bool busy = false;
  void *dev[kBufs] = {};                 // grow-only device buffers of the running call, in construction order
  size_t cap[kBufs] = {};
  int next = 0;
  void *pinned[2] = {nullptr, nullptr};  // double-buffered staging of the chunked transfers
  size_t pinned_cap = 0;                 // bytes per half
  void *ev[2] = {nullptr, nullptr};
  hipStream_t copy_stream = nullptr;     // downloads of finished frame ranges run here, beside the kernels of the next range
  std::vector<void *> range_ev;          // range r's rows are complete on the context's stream
  bool half_busy[2] = {false, false};    // an H2D transfer out of this half may still be in flight (its event says when not)
  // the input signal resident on the device: (caller's pointer, length, content hash) name it
  double *d_x = nullptr;
  size_t x_cap = 0;
  const double *x_ptr = nullptr;
  int x_len = 0;
  uint64_t x_hash = 0;
  bool x_valid = false;
  unsigned long long x_hits = 0, x_misses = 0;
  unsigned long long released = 0;       // the pool's clock when the slot was last given back
};
struct DropinPool {
  std::mutex m;
  std::condition_variable cv;
  std::vector<DropinSlot *> slots;
  int limit = 0, device = 0;
  bool shutting_down = false;            // world_hip_shutdown is releasing the slots and joining the copy helpers: callers wait
  unsigned long long clock = 0;
  bool cache_x = true;
};
static std::atomic<DropinPool *> g_dropin_pool{nullptr};
static DropinPool *new_dropin_pool() {
  DropinPool *p = new DropinPool;                // never released: the process owns it until it exits (or world_hip_shutdown empties it)
  const char *e = getenv("WORLD_HIP_DROPIN_SLOTS");
  p->limit = e ? std::max(1, std::min(64, atoi(e))) : 4;
  const char *d = getenv("WORLD_HIP_DEVICE");
  p->device = d ? atoi(d) : 0;
  const char *cx = getenv("WORLD_HIP_DROPIN_CACHE_X");
  p->cache_x = !(cx && atoi(cx) == 0);
  return p;
}
static DropinPool &dropin_pool() {
  DropinPool *p = g_dropin_pool.load(std::memory_order_acquire);
  if (!p) {
    static std::mutex once;
    std::lock_guard<std::mutex> g(once);
    p = g_dropin_pool.load(std::memory_order_acquire);
    if (!p) { p = new_dropin_pool(); register_fork_handler(); g_dropin_pool.store(p, std::memory_order_release); }
  }
  return *p;
}
static void dropin_after_fork_in_child() {
  // (async-signal-safety: only pointer stores and allocations of fresh objects; nothing of the parent's is touched)
  g_copy_pool.store(new CopyPool, std::memory_order_release);
  if (g_dropin_pool.load(std::memory_order_acquire)) g_dropin_pool.store(new_dropin_pool(), std::memory_order_release);
}
static thread_local DropinSlot *tls_slot = nullptr;

// A free slot for a call on signal `x` (nullptr: no signal): the one that already holds x, else the free slot released
// longest ago; a NEW slot (context, tables, workspace: milliseconds) only when every existing one is busy -- i.e. for
// real concurrency, not for a single thread that analyses one buffer after another.  Waits if every slot is busy and
// the pool is at its limit.
static DropinSlot *acquire_slot(const double *x) {
  DropinPool &P = dropin_pool();
  std::unique_lock<std::mutex> lk(P.m);
  for (;;) {
    if (P.shutting_down) { P.cv.wait(lk); continue; }        // (until the copy pool's helpers are joined: ADVICE r05)
    DropinSlot *pick = nullptr;
    for (DropinSlot *s : P.slots) if (!s->busy && x && s->x_valid && s->x_ptr == x) { pick = s; break; }
    if (!pick) for (DropinSlot *s : P.slots) if (!s->busy && (!pick || s->released < pick->released)) pick = s;
    if (!pick && (int)P.slots.size() < P.limit) {
      DropinSlot *s = new DropinSlot;
      s->busy = true;
      P.slots.push_back(s);
      lk.unlock();
      try {
        DeviceScope on_device(P.device);
        hipStream_t st = devrt::stream_create();
        s->ctx = world_hip_create(P.device, st);
        if (!s->ctx) { devrt::stream_destroy(st); throw std::runtime_error(std::string("cannot initialise the GPU path: ") + world_hip_last_error()); }
        s->ev[0] = devrt::event_create(); s->ev[1] = devrt::event_create();
        s->copy_stream = devrt::stream_create();
      } catch (...) {
        lk.lock();
        for (auto it = P.slots.begin(); it != P.slots.end(); ++it) if (*it == s) { P.slots.erase(it); break; }
        delete s;
        P.cv.notify_all();
        throw;
      }
      return s;
    }
    if (pick) { pick->busy = true; return pick; }
    P.cv.wait(lk);
  }
}
static void release_slot(DropinSlot *s) {
  DropinPool &P = dropin_pool();
  { std::lock_guard<std::mutex> g(P.m); s->busy = false; s->next = 0; s->released = ++P.clock; }
  P.cv.notify_one();
}

static WorldHipContext *default_context() {      // the context of the slot the running drop-in call holds
  if (!tls_slot) throw std::runtime_error("drop-in helper used outside a drop-in call");
  return tls_slot->ctx;
}

// a device buffer that lives for one drop-in call (destroyed in reverse order of construction)
struct DevBuf {
  void *p = nullptr;
  explicit DevBuf(size_t bytes) {
    DropinSlot &io = *tls_slot;
    if (io.next >= DropinSlot::kBufs) throw std::runtime_error("drop-in call needs more device buffers than the slot holds");
    const int slot = io.next++;
    if (bytes > io.cap[slot]) {
      if (io.dev[slot]) { devrt::sync(io.ctx->stream); devrt::dfree(io.dev[slot]); }
      io.dev[slot] = nullptr; io.cap[slot] = 0;
      io.dev[slot] = devrt::dmalloc(bytes + bytes / 8);
      io.cap[slot] = bytes + bytes / 8;
    }
    p = io.dev[slot];
    devrt::dpoison(p, io.cap[slot], io.ctx->stream);   // (the last call's data, perhaps a longer call's, lies behind this one's)
  }
  ~DevBuf() { --tls_slot->next; }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  template <class T> T *as() { return static_cast<T *>(p); }
};
// the two halves of the slot's pinned staging, each of at least `bytes`
static void pinned_halves(DropinSlot &io, size_t bytes) {
  if (bytes <= io.pinned_cap) return;
  devrt::sync(io.ctx->stream);
  io.half_busy[0] = io.half_busy[1] = false;
  for (int h = 0; h < 2; ++h) { if (io.pinned[h]) devrt::hfree_pinned(io.pinned[h]); io.pinned[h] = nullptr; }
  io.pinned_cap = 0;
  const size_t cap = bytes + bytes / 8;
  io.pinned[0] = devrt::hmalloc_pinned(cap);
  io.pinned[1] = devrt::hmalloc_pinned(cap);
  io.pinned_cap = cap;
}
constexpr size_t kUpChunk = size_t(1) << 20;      // bytes per pipelined upload chunk
constexpr size_t kDownChunk = size_t(4) << 20;    // bytes per pipelined download chunk (whole rows)
static void claim_half(DropinSlot &io, int h) {   // the host is about to write into staging half h
  if (io.half_busy[h]) { devrt::event_sync(io.ev[h]); io.half_busy[h] = false; }
}

// Host bytes -> device, pipelined: helper threads fill one pinned half while the copy engine drains the other
// (a pageable hipMemcpy stages through the runtime's bounce buffer on one core).  Returns without waiting for the
// last chunks: the transfer is ordered before everything enqueued on the slot's stream after it.
static void upload_bytes(DropinSlot &io, void *d_dst, const void *src, size_t bytes) {
  if (bytes == 0) return;
  hipStream_t st = io.ctx->stream;
  pinned_halves(io, std::max(kUpChunk, kDownChunk));
  CopySession awake;
  const size_t n = (bytes + kUpChunk - 1) / kUpChunk;
  for (size_t k = 0; k < n; ++k) {
    const int h = (int)(k & 1);
    const size_t off = k * kUpChunk, len = std::min(kUpChunk, bytes - off);
    claim_half(io, h);
    parallel_memcpy(io.pinned[h], static_cast<const char *>(src) + off, len);
    devrt::h2d(static_cast<char *>(d_dst) + off, io.pinned[h], len, st);
    devrt::event_record(io.ev[h], st);
    io.half_busy[h] = true;
  }
}

// Run `launch(d_x)` -- the stage's kernels, enqueued on the slot's stream -- on the call's input signal.  When the slot's
// resident copy names the same caller memory (pointer, length) the kernels are launched on it AT ONCE and the content
// hash of the caller's samples is taken while the GPU works (0.16 ms for 10 s of audio: a fifth of a stage if it stood
// in front of the launch); a mismatch -- the caller edited the signal in place -- uploads the signal and launches again
// over the same outputs.  Otherwise: pipelined upload, launch, and the hash again under the kernels.
template <class Launch> static void run_on_signal(DropinSlot &io, const double *x, int x_length, Launch launch) {
  DropinPool &P = dropin_pool();
  const size_t bytes = sizeof(double) * (size_t)x_length;
  if (P.cache_x && io.x_valid && io.x_ptr == x && io.x_len == x_length) {
    launch(static_cast<const double *>(io.d_x));
    if (signal_hash(x, x_length) == io.x_hash) { ++io.x_hits; return; }
  }
  ++io.x_misses;
  io.x_valid = false;
  if (bytes > io.x_cap * sizeof(double)) {
    if (io.d_x) { devrt::sync(io.ctx->stream); devrt::dfree(io.d_x); }
    io.d_x = nullptr; io.x_cap = 0;
    io.d_x = static_cast<double *>(devrt::dmalloc(bytes + bytes / 8));
    io.x_cap = (bytes + bytes / 8) / sizeof(double);
  }
  devrt::dpoison(io.d_x, io.x_cap * sizeof(double), io.ctx->stream);
  upload_bytes(io, io.d_x, x, bytes);
  launch(static_cast<const double *>(io.d_x));
  if (P.cache_x) {
    // the upload read the caller's memory chunk by chunk just now; hashing the same memory afterwards names the same
    // content unless another thread writes to it during the call -- which the reference does not support either
    io.x_hash = signal_hash(x, x_length);
    io.x_ptr = x; io.x_len = x_length; io.x_valid = true;
  }
}

// a shape the GPU path cannot run is refused BEFORE anything touches the GPU (no upload, no launch, no allocation)
static void require_shape(int what, int fs, int fft_size) {
  const std::string r = shape_limit(what, fs, fft_size);
  if (!r.empty()) throw std::runtime_error(r);
}
// Every drop-in call runs on the pool's device whatever device the calling thread had selected (a multi-GPU host
// process); the caller's selection is restored afterwards.  `x`: the call's input signal, for slot affinity.
template <class F> static void dropin_guard(const char *what, const double *x, F f) {
  DropinTimed t_(what);
  std::string failure;
  bool failed = false;
  DropinSlot *outer = tls_slot;                  // (a handler-driven re-entry keeps its own slot)
  DropinSlot *s = nullptr;
  try {
    s = acquire_slot(x);
    tls_slot = s;
    DeviceScope on_device(s->ctx->device);
    f();
  } catch (const std::exception &e) {
    failed = true;
    failure = e.what();
    if (s) {
      s->x_valid = false;                        // whatever was in flight: never trust the resident copy after a failure
      try { DeviceScope on_device(s->ctx->device); devrt::sync(s->ctx->stream); if (s->copy_stream) devrt::sync(s->copy_stream); } catch (...) {}
    }
  }
  tls_slot = outer;
  if (s) release_slot(s);
  if (failed) report_failure(what, failure);
}
template <class F> static void dropin_guard(const char *what, F f) { dropin_guard(what, nullptr, f); }

}  // namespace world_hip

extern "C" {

void world_hip_set_error_handler(void (*handler)(const char *function, const char *message, void *user), void *user) {
  std::lock_guard<std::mutex> g(world_hip::g_handler_lock);
  world_hip::g_handler = handler;
  world_hip::g_handler_user = user;
}

// Gives back everything the drop-in layer holds -- the helper threads are joined, every slot's context, streams, events,
// device and pinned buffers are released -- so that a host process can unload the GPU path (or hand the device to something
// else) without exiting.  The next drop-in call starts over (contexts, tables and workspace are rebuilt: a cold call).
// Returns 0, or -1 if a drop-in call is still running (nothing is released then).
int world_hip_shutdown(void) {
  using namespace world_hip;
  DropinPool &P = dropin_pool();
  std::vector<DropinSlot *> slots;
  {
    std::lock_guard<std::mutex> g(P.m);
    if (P.shutting_down) { g_last_error = "world_hip_shutdown: already shutting down"; return -1; }
    for (DropinSlot *s : P.slots) if (s->busy) { g_last_error = "world_hip_shutdown: a drop-in call is still running"; return -1; }
    slots.swap(P.slots);
    P.shutting_down = true;              // a drop-in call that starts now waits in acquire_slot until everything below is done
  }
  for (DropinSlot *s : slots) {
    try {
      DeviceScope on_device(s->ctx ? s->ctx->device : P.device);
      if (s->ctx) devrt::sync(s->ctx->stream);
      if (s->copy_stream) { devrt::sync(s->copy_stream); devrt::stream_destroy(s->copy_stream); }
      for (int k = 0; k < DropinSlot::kBufs; ++k) if (s->dev[k]) devrt::dfree(s->dev[k]);
      for (int h = 0; h < 2; ++h) { if (s->pinned[h]) devrt::hfree_pinned(s->pinned[h]); if (s->ev[h]) devrt::event_destroy(s->ev[h]); }
      for (void *e : s->range_ev) devrt::event_destroy(e);
      if (s->d_x) devrt::dfree(s->d_x);
      if (s->ctx) { hipStream_t st = s->ctx->stream; world_hip_destroy(s->ctx); devrt::stream_destroy(st); }
    } catch (...) {}
    delete s;
  }
  copy_pool().shutdown();
  { std::lock_guard<std::mutex> g(P.m); P.shutting_down = false; }
  P.cv.notify_all();
  return 0;
}

// counters of the drop-in layer (diagnostic; tests and bench.py read them)
void world_hip_dropin_stats(unsigned long long *slots, unsigned long long *x_hits, unsigned long long *x_misses) {
  world_hip::DropinPool &P = world_hip::dropin_pool();
  std::lock_guard<std::mutex> g(P.m);
  unsigned long long h = 0, m = 0;
  for (world_hip::DropinSlot *s : P.slots) { h += s->x_hits; m += s->x_misses; }
  if (slots) *slots = P.slots.size();
  if (x_hits) *x_hits = h;
  if (x_misses) *x_misses = m;
}

}  // extern "C"

extern "C" {

// ---- option helpers: pure host arithmetic, identical to the reference ----------
void InitializeDioOption(DioOption *option) {            // src/dio.cpp:650-666
  option->channels_in_octave = 2.0;
  option->f0_ceil = 800.0;
  option->f0_floor = 71.0;
  option->frame_period = 5;
  option->speed = 1;
  option->allowed_range = 0.1;
}
int GetSamplesForDIO(int fs, int x_length, double frame_period) {      // src/dio.cpp:639-641
  return static_cast<int>(1000.0 * x_length / fs / frame_period) + 1;
}
void InitializeHarvestOption(HarvestOption *option) {    // src/harvest.cpp:1257-1262
  option->f0_ceil = 800.0;
  option->f0_floor = 71.0;
  option->frame_period = 5;
}
int GetSamplesForHarvest(int fs, int x_length, double frame_period) {  // src/harvest.cpp:1219-1221
  return static_cast<int>(1000.0 * x_length / fs / frame_period) + 1;
}
int GetFFTSizeForCheapTrick(int fs, const CheapTrickOption *option) {  // src/cheaptrick.cpp:191-194
  return static_cast<int>(pow(2.0, 1.0 + static_cast<int>(log(3.0 * fs / option->f0_floor + 1) / world_hip::kLog2)));
}
double GetF0FloorForCheapTrick(int fs, int fft_size) {   // src/cheaptrick.cpp:196-198
  return 3.0 * fs / (fft_size - 3.0);
}
void InitializeCheapTrickOption(int fs, CheapTrickOption *option) {    // src/cheaptrick.cpp:231-240
  option->q1 = -0.15;
  option->f0_floor = 71.0;
  option->fft_size = GetFFTSizeForCheapTrick(fs, option);
}
void InitializeD4COption(D4COption *option) { option->threshold = 0.85; }   // src/d4c.cpp:405-407

// ---- F0 estimators -----------------------------------------------------------------
void Harvest(const double *x, int x_length, int fs, const HarvestOption *option, double *temporal_positions,
             double *f0) {
  using namespace world_hip;
  dropin_guard("Harvest", x, [&] {
    DropinSlot &io = *tls_slot;
    WorldHipContext *c = io.ctx;
    const int nf = GetSamplesForHarvest(fs, x_length, option->frame_period);
    if (x_length <= 0 || nf <= 0) throw std::runtime_error("empty input");
    DevBuf dt(sizeof(double) * nf), df(sizeof(double) * nf);
    run_on_signal(io, x, x_length, [&](const double *dx) {
      must(world_hip_harvest_batch(c, 1, fs, dx, x_length, &x_length, option, nf, dt.as<double>(), df.as<double>()), "Harvest");
    });
    devrt::d2h(temporal_positions, dt.p, sizeof(double) * nf, c->stream);
    devrt::d2h(f0, df.p, sizeof(double) * nf, c->stream);
    devrt::sync(c->stream);
  });
}

void Dio(const double *x, int x_length, int fs, const DioOption *option, double *temporal_positions, double *f0) {
  using namespace world_hip;
  dropin_guard("Dio", x, [&] {
    DropinSlot &io = *tls_slot;
    WorldHipContext *c = io.ctx;
    const int nf = GetSamplesForDIO(fs, x_length, option->frame_period);
    if (x_length <= 0 || nf <= 0) throw std::runtime_error("empty input");
    DevBuf dt(sizeof(double) * nf), df(sizeof(double) * nf);
    run_on_signal(io, x, x_length, [&](const double *dx) {
      // FixF0Contour returns without writing f0 when the utterance has no more frames than
      // voice_range_minimum (dio.cpp:266): the caller's buffer keeps its contents there too
      devrt::h2d(df.p, f0, sizeof(double) * nf, c->stream);
      must(world_hip_dio_batch(c, 1, fs, dx, x_length, &x_length, option, nf, dt.as<double>(), df.as<double>()), "Dio");
    });
    devrt::d2h(temporal_positions, dt.p, sizeof(double) * nf, c->stream);
    devrt::d2h(f0, df.p, sizeof(double) * nf, c->stream);
    devrt::sync(c->stream);
  });
}

void StoneMask(const double *x, int x_length, int fs, const double *temporal_positions, const double *f0,
               int f0_length, double *refined_f0) {
  using namespace world_hip;
  dropin_guard("StoneMask", x, [&] {
    require_shape(1, fs, 0);
    DropinSlot &io = *tls_slot;
    WorldHipContext *c = io.ctx;
    if (x_length <= 0 || f0_length <= 0) throw std::runtime_error("empty input");
    DevBuf dt(sizeof(double) * f0_length), df(sizeof(double) * f0_length), dr(sizeof(double) * f0_length);
    devrt::h2d(dt.p, temporal_positions, sizeof(double) * f0_length, c->stream);
    devrt::h2d(df.p, f0, sizeof(double) * f0_length, c->stream);
    run_on_signal(io, x, x_length, [&](const double *dx) {
      must(world_hip_stonemask_batch(c, 1, fs, dx, x_length, &x_length, &f0_length, f0_length,
                                     dt.as<double>(), df.as<double>(), dr.as<double>()), "StoneMask");
    });
    devrt::d2h(refined_f0, dr.p, sizeof(double) * f0_length, c->stream);
    devrt::sync(c->stream);
  });
}

}  // extern "C"

// ---- spectral stages: rows of the caller's double** are separate allocations -------
// The matrix leaves the device in chunks of whole rows through the slot's two pinned halves: chunk k + 1 is on the
// PCIe link while the calling thread and the helper threads copy chunk k's rows to where the caller wants them
// (round 3: one monolithic copy, then 2001 serial memcpys).  Dense caller memory (numpy, one allocation cut into rows)
// takes the same route: a pageable hipMemcpy is the runtime's single-threaded version of it.
// WORLD_HIP_DROPIN_WIRE=f32: the spectral stages' rows leave the device as float (rounded once by the stage kernels, 6e-8
// relative against the contract's 1e-4) and are widened into the caller's double rows by the host copies: half the bytes
// on PCIe, which is what the drop-in path of a 10 s utterance is bound by (33 MB of f64 rows at ~40 GB/s = 0.8 of 1.8 ms).
// Default off: the rows then equal a device-resident analysis bit for bit.
static bool dropin_f32() {
  static const bool v = [] { const char *e = getenv("WORLD_HIP_DROPIN_WIRE"); return e && strcmp(e, "f32") == 0; }();
  return v;
}
// doubles between two rows of the device matrix: cols, or -- narrow rows -- the floats of a row padded to whole doubles
static size_t dropin_row_doubles(int cols, bool f32) { return f32 ? (size_t)(cols + 1) / 2 : (size_t)cols; }

static void rows_to_host(world_hip::DropinSlot &io, const double *d_dense, int rows, int cols, double **host_rows, bool f32 = false) {
  using namespace world_hip;
  if (rows <= 0 || cols <= 0) return;
  hipStream_t st = io.ctx->stream;
  const size_t row_bytes = sizeof(double) * dropin_row_doubles(cols, f32);     // of a DEVICE row
  pinned_halves(io, std::max(std::max(kUpChunk, kDownChunk), row_bytes));
  const int chunk_rows = std::max<int>(1, (int)(kDownChunk / row_bytes));
  const int n = (rows + chunk_rows - 1) / chunk_rows;
  world_hip::CopySession awake;
  auto issue = [&](int k) {
    const int h = k & 1, r0 = k * chunk_rows, nr = std::min(chunk_rows, rows - r0);
    claim_half(io, h);
    devrt::d2h(io.pinned[h], reinterpret_cast<const char *>(d_dense) + (size_t)r0 * row_bytes, row_bytes * nr, st);
    devrt::event_record(io.ev[h], st);
  };
  issue(0);
  for (int k = 0; k < n; ++k) {
    if (k + 1 < n) issue(k + 1);                    // half (k+1)&1 was emptied by the host copy of chunk k-1
    const int h = k & 1, r0 = k * chunk_rows, nr = std::min(chunk_rows, rows - r0);
    devrt::event_sync(io.ev[h]);
    CopyTask t;
    t.src_base = static_cast<const char *>(io.pinned[h]); t.src_rows = nullptr;
    t.dst_base = nullptr; t.dst_rows = reinterpret_cast<char *const *>(host_rows + r0);
    t.row_bytes = sizeof(double) * (size_t)cols; t.src_stride = row_bytes; t.widen = f32 ? cols : 0;
    t.rows = nr; t.grain = std::max<int>(1, (int)((size_t(128) << 10) / row_bytes));
    copy_pool().run(t);
  }
}

// The spectral stages' matrices are produced frame range by frame range (world_hip_*_batch_range), so a finished
// range can travel while the kernels of the next one run: range r's rows are copied on the slot's second stream as soon
// as the event behind its kernels fires, through the two pinned halves as above (round 3: the whole matrix waited for
// the last kernel, then for one monolithic copy).  kRangeFrames frames per range: 4.2 MB of rows at 1025 bins.
constexpr int kRangeFrames = 512;                       // a multiple of the wavefront (CheapTrick's serial scans)
// WORLD_HIP_DROPIN_RANGES: which stages are produced and downloaded range by range -- 0 none, 1 D4C (default: its
// kernels are 0.35 ms of a 10 s utterance, worth hiding a download behind), 2 CheapTrick as well (0.1 ms of kernels:
// the twelve smaller launches cost what the overlap saves)
static int dropin_ranges() {
  static const int v = [] { const char *e = getenv("WORLD_HIP_DROPIN_RANGES"); return e ? atoi(e) : 1; }();
  return v;
}
static int range_count(int rows) { return (rows + kRangeFrames - 1) / kRangeFrames; }
static void range_events(world_hip::DropinSlot &io, int n) {
  while ((int)io.range_ev.size() < n) io.range_ev.push_back(devrt::event_create());
}
static void ranges_to_host(world_hip::DropinSlot &io, const double *d_dense, int rows, int cols, double **host_rows, bool f32 = false) {
  using namespace world_hip;
  if (rows <= 0 || cols <= 0) return;
  const size_t row_bytes = sizeof(double) * dropin_row_doubles(cols, f32);     // of a DEVICE row
  pinned_halves(io, std::max(std::max(kUpChunk, kDownChunk), row_bytes * kRangeFrames));
  const int n = range_count(rows);
  CopySession awake;
  auto issue = [&](int k) {
    const int h = k & 1, r0 = k * kRangeFrames, nr = std::min(kRangeFrames, rows - r0);
    claim_half(io, h);
    devrt::stream_wait_event(io.copy_stream, io.range_ev[k]);
    devrt::d2h(io.pinned[h], reinterpret_cast<const char *>(d_dense) + (size_t)r0 * row_bytes, row_bytes * nr, io.copy_stream);
    devrt::event_record(io.ev[h], io.copy_stream);
  };
  issue(0);
  for (int k = 0; k < n; ++k) {
    if (k + 1 < n) issue(k + 1);                    // half (k+1)&1 was emptied by the host copy of range k-1
    const int h = k & 1, r0 = k * kRangeFrames, nr = std::min(kRangeFrames, rows - r0);
    devrt::event_sync(io.ev[h]);
    CopyTask t;
    t.src_base = static_cast<const char *>(io.pinned[h]); t.src_rows = nullptr;
    t.dst_base = nullptr; t.dst_rows = reinterpret_cast<char *const *>(host_rows + r0);
    t.row_bytes = sizeof(double) * (size_t)cols; t.src_stride = row_bytes; t.widen = f32 ? cols : 0;
    t.rows = nr; t.grain = std::max<int>(1, (int)((size_t(128) << 10) / row_bytes));
    copy_pool().run(t);
  }
}

// one spectral stage of the slot's utterance into dense device rows -- double, or (f32) float rows padded to whole doubles:
// the stage kernels round once as they store (the RowLayout of the multi-GPU exchange's narrow wire, one row per frame)
static void dropin_stage(WorldHipContext *c, bool d4c, int fs, const double *dx, int x_length, int f0_length, const double *d_tpos,
                         const double *d_f0, const CheapTrickOption *copt, int fft_size, const D4COption *dopt, int frame_lo,
                         int frame_hi, bool reuse, bool f32, double *d_rows) {
  using namespace world_hip;
  const int rc = guarded(c, [&] {
    RowLayout lay;
    lay.frame_lo = frame_lo; lay.frame_hi = frame_hi; lay.skip_prepare = reuse;
    if (f32) { lay.f32 = 1; lay.stride = dropin_row_doubles(fft_size / 2 + 1, true); }
    if (d4c) run_d4c(c, 1, fs, dx, x_length, &x_length, &f0_length, f0_length, d_tpos, d_f0, fft_size, dopt, d_rows, lay);
    else run_cheaptrick(c, 1, fs, dx, x_length, &x_length, &f0_length, f0_length, d_tpos, d_f0, copt, d_rows, lay);
  });
  must(rc, d4c ? "D4C" : "CheapTrick");
}

static void rows_to_device(world_hip::DropinSlot &io, const double *const *host_rows, int rows, int cols, double *d_dense) {
  using namespace world_hip;
  if (rows <= 0 || cols <= 0) return;
  hipStream_t st = io.ctx->stream;
  const size_t row_bytes = sizeof(double) * (size_t)cols;
  pinned_halves(io, std::max(std::max(kUpChunk, kDownChunk), row_bytes));
  const int chunk_rows = std::max<int>(1, (int)(kUpChunk / row_bytes));
  const int n = (rows + chunk_rows - 1) / chunk_rows;
  world_hip::CopySession awake;
  for (int k = 0; k < n; ++k) {
    const int h = k & 1, r0 = k * chunk_rows, nr = std::min(chunk_rows, rows - r0);
    claim_half(io, h);
    CopyTask t;
    t.src_base = nullptr; t.src_rows = reinterpret_cast<const char *const *>(host_rows + r0);
    t.dst_base = static_cast<char *>(io.pinned[h]); t.dst_rows = nullptr;
    t.row_bytes = row_bytes; t.rows = nr; t.grain = std::max<int>(1, (int)((size_t(128) << 10) / row_bytes));
    copy_pool().run(t);
    devrt::h2d(d_dense + (size_t)r0 * cols, io.pinned[h], row_bytes * nr, st);
    devrt::event_record(io.ev[h], st);
    io.half_busy[h] = true;
  }
}

extern "C" {

void CheapTrick(const double *x, int x_length, int fs, const double *temporal_positions, const double *f0,
                int f0_length, const CheapTrickOption *option, double **spectrogram) {
  using namespace world_hip;
  dropin_guard("CheapTrick", x, [&] {
    require_shape(2, fs, option->fft_size);
    DropinSlot &io = *tls_slot;
    WorldHipContext *c = io.ctx;
    if (x_length <= 0 || f0_length <= 0) throw std::runtime_error("empty input");
    const int nb = option->fft_size / 2 + 1;
    const bool f32 = dropin_f32();
    DevBuf dt(sizeof(double) * f0_length), df(sizeof(double) * f0_length), ds(sizeof(double) * (size_t)f0_length * dropin_row_doubles(nb, f32));
    devrt::h2d(dt.p, temporal_positions, sizeof(double) * f0_length, c->stream);
    devrt::h2d(df.p, f0, sizeof(double) * f0_length, c->stream);
    const int n_ranges = dropin_ranges() >= 2 ? range_count(f0_length) : 0;
    if (n_ranges == 0) {
      run_on_signal(io, x, x_length, [&](const double *dx) {
        dropin_stage(c, false, fs, dx, x_length, f0_length, dt.as<double>(), df.as<double>(), option, option->fft_size, nullptr,
                     0, 0x7FFFFFFF, false, f32, ds.as<double>());
      });
      rows_to_host(io, ds.as<double>(), f0_length, nb, spectrogram, f32);
      return;
    }
    range_events(io, n_ranges);
    run_on_signal(io, x, x_length, [&](const double *dx) {
      for (int r = 0; r < n_ranges; ++r) {
        dropin_stage(c, false, fs, dx, x_length, f0_length, dt.as<double>(), df.as<double>(), option, option->fft_size, nullptr,
                     r * kRangeFrames, (r + 1) * kRangeFrames, r > 0, f32, ds.as<double>());
        devrt::event_record(io.range_ev[r], c->stream);
      }
    });
    ranges_to_host(io, ds.as<double>(), f0_length, nb, spectrogram, f32);
  });
}

void D4C(const double *x, int x_length, int fs, const double *temporal_positions, const double *f0, int f0_length,
         int fft_size, const D4COption *option, double **aperiodicity) {
  using namespace world_hip;
  dropin_guard("D4C", x, [&] {
    require_shape(4, fs, fft_size);
    DropinSlot &io = *tls_slot;
    WorldHipContext *c = io.ctx;
    if (x_length <= 0 || f0_length <= 0) throw std::runtime_error("empty input");
    const int nb = fft_size / 2 + 1;
    const bool f32 = dropin_f32();
    DevBuf dt(sizeof(double) * f0_length), df(sizeof(double) * f0_length), da(sizeof(double) * (size_t)f0_length * dropin_row_doubles(nb, f32));
    devrt::h2d(dt.p, temporal_positions, sizeof(double) * f0_length, c->stream);
    devrt::h2d(df.p, f0, sizeof(double) * f0_length, c->stream);
    const int n_ranges = dropin_ranges() >= 1 ? range_count(f0_length) : 0;
    if (n_ranges == 0) {
      run_on_signal(io, x, x_length, [&](const double *dx) {
        dropin_stage(c, true, fs, dx, x_length, f0_length, dt.as<double>(), df.as<double>(), nullptr, fft_size, option,
                     0, 0x7FFFFFFF, false, f32, da.as<double>());
      });
      rows_to_host(io, da.as<double>(), f0_length, nb, aperiodicity, f32);
      return;
    }
    range_events(io, n_ranges);
    run_on_signal(io, x, x_length, [&](const double *dx) {
      for (int r = 0; r < n_ranges; ++r) {          // LoveTrain and the offset scans cover every frame, once (r == 0)
        dropin_stage(c, true, fs, dx, x_length, f0_length, dt.as<double>(), df.as<double>(), nullptr, fft_size, option,
                     r * kRangeFrames, (r + 1) * kRangeFrames, r > 0, f32, da.as<double>());
        devrt::event_record(io.range_ev[r], c->stream);
      }
    });
    ranges_to_host(io, da.as<double>(), f0_length, nb, aperiodicity, f32);
  });
}

// ---- codec (src/world/codec.h): coded parameters for statistical models --------------
int GetNumberOfAperiodicities(int fs) {                   // src/codec.cpp:212-215
  return static_cast<int>(std::min(15000.0, fs / 2.0 - 3000.0) / 3000.0);
}

}  // extern "C"

template <class Run>
static void codec_dropin(const char *what, const double *const *in, int rows, int in_cols, int out_cols, double **out,
                         Run run) {
  using namespace world_hip;
  dropin_guard(what, [&] {
    if (rows <= 0) return;
    DropinSlot &io = *tls_slot;
    WorldHipContext *c = io.ctx;
    DevBuf di(sizeof(double) * (size_t)rows * in_cols), dout(sizeof(double) * (size_t)rows * out_cols);
    rows_to_device(io, in, rows, in_cols, di.as<double>());
    must(run(c, di.as<double>(), dout.as<double>()), what);
    rows_to_host(io, dout.as<double>(), rows, out_cols, out);
  });
}

extern "C" {

void CodeAperiodicity(const double *const *aperiodicity, int f0_length, int fs, int fft_size,
                      double **coded_aperiodicity) {
  codec_dropin("CodeAperiodicity", aperiodicity, f0_length, fft_size / 2 + 1, GetNumberOfAperiodicities(fs),
               coded_aperiodicity, [&](WorldHipContext *c, const double *i, double *o) {
                 return world_hip_code_aperiodicity(c, f0_length, fs, fft_size, i, o);
               });
}

void DecodeAperiodicity(const double *const *coded_aperiodicity, int f0_length, int fs, int fft_size,
                        double **aperiodicity) {
  codec_dropin("DecodeAperiodicity", coded_aperiodicity, f0_length, GetNumberOfAperiodicities(fs), fft_size / 2 + 1,
               aperiodicity, [&](WorldHipContext *c, const double *i, double *o) {
                 return world_hip_decode_aperiodicity(c, f0_length, fs, fft_size, i, o);
               });
}

void CodeSpectralEnvelope(const double *const *spectrogram, int f0_length, int fs, int fft_size,
                          int number_of_dimensions, double **coded_spectral_envelope) {
  codec_dropin("CodeSpectralEnvelope", spectrogram, f0_length, fft_size / 2 + 1, number_of_dimensions,
               coded_spectral_envelope, [&](WorldHipContext *c, const double *i, double *o) {
                 return world_hip_code_spectral_envelope(c, f0_length, fs, fft_size, number_of_dimensions, i, o);
               });
}

void DecodeSpectralEnvelope(const double *const *coded_spectral_envelope, int f0_length, int fs, int fft_size,
                            int number_of_dimensions, double **spectrogram) {
  codec_dropin("DecodeSpectralEnvelope", coded_spectral_envelope, f0_length, number_of_dimensions, fft_size / 2 + 1,
               spectrogram, [&](WorldHipContext *c, const double *i, double *o) {
                 return world_hip_decode_spectral_envelope(c, f0_length, fs, fft_size, number_of_dimensions, i, o);
               });
}

// ---- synthesis (src/world/synthesis.h:30) ----------------------------------------------
void Synthesis(const double *f0, int f0_length, const double *const *spectrogram, const double *const *aperiodicity,
               int fft_size, double frame_period, int fs, int y_length, double *y) {
  using namespace world_hip;
  dropin_guard("Synthesis", [&] {
    require_shape(8, fs, fft_size);
    DropinSlot &io = *tls_slot;
    WorldHipContext *c = io.ctx;
    const int nb = fft_size / 2 + 1;
    DevBuf df(sizeof(double) * f0_length), ds(sizeof(double) * (size_t)f0_length * nb),
        da(sizeof(double) * (size_t)f0_length * nb), dy(sizeof(double) * y_length);
    devrt::h2d(df.p, f0, sizeof(double) * f0_length, c->stream);
    rows_to_device(io, spectrogram, f0_length, nb, ds.as<double>());
    rows_to_device(io, aperiodicity, f0_length, nb, da.as<double>());
    // the reference has no pulse limit: if the automatic workspace was too small the device says how many
    // pulses there are, and the call is repeated with exactly that capacity
    // (the slot's context gets its automatic capacity back whatever happens in between: ADVICE r02)
    struct CapacityGuard {
      WorldHipContext *c;
      ~CapacityGuard() { world_hip_set_synthesis_pulse_capacity(c, 0); }
    } restore{c};
    for (int attempt = 0; attempt < 3; ++attempt) {
      must(world_hip_synthesis_batch(c, 1, fs, frame_period, fft_size, &f0_length, f0_length, df.as<double>(),
                                     ds.as<double>(), da.as<double>(), &y_length, y_length, dy.as<double>()), "Synthesis");
      int need = 0;
      must(world_hip_synthesis_pulses_dropped(c, &need), "Synthesis");
      if (need == 0) break;
      if (attempt == 2) throw std::runtime_error("pulse count keeps exceeding the workspace");
      // a pulse needs at least one output sample: a count beyond y_length is a corrupted contour, not a workspace to allocate
      if (need > y_length) throw std::runtime_error("more pitch pulses than output samples");
      must(world_hip_set_synthesis_pulse_capacity(c, need + 16), "Synthesis");
    }
    devrt::d2h(y, dy.p, sizeof(double) * y_length, c->stream);
    devrt::sync(c->stream);
  });
}

}  // extern "C"

#include "realtime_dropin.inc"
