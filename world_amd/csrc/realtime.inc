// realtime.inc -- real-time synthesis (reference src/synthesisrealtime.cpp): the per-stream scheduler on the host and
// the batched entry points world_hip_realtime_* of include/world_hip.h.  Included by api.hip, so the time base below is
// compiled with the library's -ffp-contract=off.
//
// What stays on the host, and why: AddParameters' return value, Synthesis2's return value, IsLocked and every public
// field of the reference's synthesiser are decided by pulse positions, synchronously, call by call; and a chunk's time
// base is a strictly sequential phase sum of O(chunk samples) scalar adds.  So each stream keeps the reference's control
// state here, field for field, and runs the reference's bookkeeping (ring, pointers, Seek / Clear) in the reference's
// order.  What goes to the GPU is the work per pulse: its two minimum-phase spectra, the noise transform and the
// overlap-add (synthesis.hip: rt_pulse, rt_overlap_add).
//
// Render-ahead.  Adding chunks never inserts a pulse before an existing one, a pulse's noise_size is the distance to the
// next pulse, and the reference renders only pulses before last_location.  So every pulse that has a successor is final
// and can be rendered as soon as it exists.  When a call needs samples not yet finished, every such pulse of the stream
// is rendered in one batch of launches (all needy streams together) and the finished samples go to a host window; later
// calls are served from the window without GPU work.  The control fields still advance call by call exactly as the
// reference's do, and each pulse the reference would render at that point is checked against the one rendered ahead.
//
// Output rounding.  In the reference a pulse rendered while the buffer starts at sample b = synthesized_sample adds its
// response to samples >= b only, in pulse order, onto whatever earlier pulses left there.  b is the multiple of
// buffer_size at or below the pulse (pulses are rendered in the call whose buffer contains them), so each job carries
// `first` = that multiple, and rt_overlap_add continues each stream's partial sums in pulse order.

namespace world_hip {

// ---- the reference's randn() state on the host ------------------------------------------------------------------
struct RtRng { uint32_t x, y, z, w; };
static RtRng rt_seed() { return RtRng{123456789u, 362436069u, 521288629u, 88675123u}; }   // randn_reseed()
static const std::vector<uint4> &rt_host_jump() {
  static const std::vector<uint4> tab = [] {
    std::vector<uint4> t((size_t)kJumpLevels * kJumpStride);
    build_jump_tables(t.data());
    return t;
  }();
  return tab;
}
// the state after `calls` more randn() calls: the jump matrices of rng.h, 2^level calls each (64-bit counts: a stream
// may outlive 2^32 draws)
static RtRng rt_jump(RtRng s, unsigned long long calls) {
  const std::vector<uint4> &tab = rt_host_jump();
  auto level = [&](RtRng v, int lv) {
    const uint4 *t = tab.data() + (size_t)lv * kJumpStride;
    const uint32_t in[4] = {v.x, v.y, v.z, v.w};
    RtRng r{0, 0, 0, 0};
    for (int wd = 0; wd < 4; ++wd)
      for (int n = 0; n < 8; ++n) {
        const uint4 e = t[(wd * 8 + n) * 16 + ((in[wd] >> (4 * n)) & 15u)];
        r.x ^= e.x; r.y ^= e.y; r.z ^= e.z; r.w ^= e.w;
      }
    return r;
  };
  for (int lv = 0; lv < 32; ++lv)
    if ((calls >> lv) & 1ull) s = level(s, lv);
  for (unsigned long long hi = calls >> 32; hi != 0; --hi) s = level(level(s, 31), 31);
  return s;
}

// ---- matlabfunctions.cpp:136-176, 206-208 (histc, interp1, matlab_round), restated ---------------------------------
static void rt_histc(const double *x, int x_length, const double *edges, int edges_length, int *index) {
  int count = 1, i = 0;
  for (; i < edges_length; ++i) {
    index[i] = 1;
    if (edges[i] >= x[0]) break;
  }
  for (; i < edges_length; ++i) {
    if (edges[i] < x[count]) {
      index[i] = count;
    } else {
      index[i--] = count++;
    }
    if (count == x_length) break;
  }
  count--;
  for (i++; i < edges_length; ++i) index[i] = count;
}
static void rt_interp1(const double *x, const double *y, int x_length, const double *xi, int xi_length, double *yi) {
  std::vector<double> h(x_length - 1);
  std::vector<int> k(xi_length, 0);
  for (int i = 0; i < x_length - 1; ++i) h[i] = x[i + 1] - x[i];
  rt_histc(x, x_length, xi, xi_length, k.data());
  for (int i = 0; i < xi_length; ++i) {
    const double s = (xi[i] - x[k[i] - 1]) / h[k[i] - 1];
    yi[i] = y[k[i] - 1] + s * (y[k[i]] - y[k[i] - 1]);
  }
}
static int rt_round(double x) { return x > 0 ? static_cast<int>(x + 0.5) : static_cast<int>(x - 0.5); }

// ---- one stream --------------------------------------------------------------------------------------------------
struct RtPulse {
  int loc;
  double vuv;
};
struct RtStream {
  // the reference's control fields (WorldSynthesizer), same names, same meaning
  int current_pointer = 0, i = 0, current_pointer2 = 0, head_pointer = 0, synthesized_sample = 0;
  int handoff = 0, last_location = 0, cumulative_frame = -1, current_frame = 0;
  double handoff_phase = 0.0, handoff_f0 = 0.0;
  std::vector<int> f0_length, f0_origin, number_of_pulses;
  std::vector<std::vector<int>> pulse_index;      // pulse_locations_index of each ring slot
  RtRng ref_rng = rt_seed();                      // randn_state after the pulses Synthesis2 has gone past
  // every pulse since the last refresh that is still needed: sched[k] is pulse number sched_base + k
  std::deque<RtPulse> sched;
  long long sched_base = 0;
  long long rendered = 0;                         // pulses [0, rendered) have been rendered on the device
  long long ref_next = 0;                         // the next pulse Synthesis2 goes past
  RtRng render_rng = rt_seed();                   // randn_state at pulse `rendered`
  // frame store: frames [store_lo, frames) are resident, frame g in row g % store_cap
  double *d_sp = nullptr, *d_ap = nullptr;
  int store_cap = 0;
  long long store_lo = 0, frames = 0;
  // output: samples [0, final_end) are finished; the host window holds [win_lo, final_end), the device tail the partial
  // sums of [final_end, tail_end)
  int final_end = 0, tail_end = 0, tail_par = 0;
  std::vector<double> window;
  int win_lo = 0;
};

}  // namespace world_hip

struct WorldHipRealtime {
  WorldHipContext *ctx = nullptr;
  bool own_ctx = false;                           // the drop-in's synthesiser owns its context (and the context's stream)
  int n_streams = 0, fs = 0, fft_size = 0, lg_fft = 0, buffer_size = 0, number_of_pointers = 0;
  double frame_period = 0.0;                      // seconds, as the reference keeps it
  std::vector<world_hip::RtStream> streams;
  double *d_dc_remover = nullptr;                 // GetDCRemover(fft_size / 2)
  std::vector<double> dc_remover;
  double *d_tails = nullptr;                      // [n_streams][2][tail_cap]
  int tail_cap = 0;
  // grow-only workspace of a render batch
  world_hip::RtPulseJob *d_jobs = nullptr;
  size_t jobs_cap = 0;
  double *d_resp = nullptr;
  size_t resp_cap = 0;                            // pulses
  world_hip::RtOlaStream *d_ola = nullptr;
  double *d_stage = nullptr, *h_stage = nullptr;
  size_t stage_cap = 0;
  std::vector<world_hip::RtPulseJob> jobs;
  std::vector<world_hip::RtOlaStream> ola;
  // world_hip_realtime_synthesize's output staging: two pinned halves, each reused once its copy has completed
  double *h_out[2] = {nullptr, nullptr};
  void *out_ev[2] = {nullptr, nullptr};
  bool out_busy[2] = {false, false};
  int out_half = 0;
  // the drop-in's row staging (AddParameters' double ** rows): two pinned halves
  double *h_rows[2] = {nullptr, nullptr};
  size_t rows_cap = 0;                            // doubles per half
  void *rows_ev[2] = {nullptr, nullptr};
  bool rows_busy[2] = {false, false};
  int rows_half = 0;
};

namespace world_hip {

// pulses of one render batch, at most (bounds the response buffer)
// (WORLD_HIP_REALTIME_BATCH_PULSES: test hook, a smaller limit; 1 renders one pulse per batch, i.e. no render-ahead)
static size_t rt_batch_pulses(int fft_size) {
  const size_t per = sizeof(double) * (size_t)rt_resp_stride(fft_size);
  const size_t cap = std::max<size_t>(64, (size_t(256) << 20) / per);
  const char *e = getenv("WORLD_HIP_REALTIME_BATCH_PULSES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? std::min(cap, (size_t)v) : cap;
}

static void rt_check_stream(WorldHipRealtime *rt, int s) {
  if (s < 0 || s >= rt->n_streams) fail("stream %d outside [0, %d)", s, rt->n_streams);
}

static void rt_reset(WorldHipRealtime *rt, RtStream &st) {       // RefreshSynthesizer (:521-542)
  const int P = rt->number_of_pointers;
  for (int k = 0; k < P; ++k) { st.number_of_pulses[k] = 0; st.pulse_index[k].clear(); }
  st.handoff_phase = 0; st.handoff_f0 = 0; st.cumulative_frame = -1; st.last_location = 0;
  st.current_pointer = 0; st.current_pointer2 = 0; st.head_pointer = 0; st.handoff = 0;
  st.i = 0; st.current_frame = 0; st.synthesized_sample = 0;
  st.ref_rng = rt_seed();
  st.sched.clear(); st.sched_base = 0; st.rendered = 0; st.ref_next = 0; st.render_rng = rt_seed();
  st.store_lo = 0; st.frames = 0;
  st.final_end = 0; st.tail_end = 0; st.tail_par = 0;
  st.window.clear(); st.win_lo = 0;
}

struct RtUndo;
static void rt_undo_clear(RtUndo *undo, int slot, int pulses, std::vector<int> &index);
static void rt_clear_ring(WorldHipRealtime *rt, RtStream &st, int start, int end, RtUndo *undo = nullptr) {
  for (int k = start; k < end; ++k) {                                                   // ClearRingBuffer (:81-99)
    const int p = k % rt->number_of_pointers;
    if (undo) rt_undo_clear(undo, p, st.number_of_pulses[p], st.pulse_index[p]);
    st.number_of_pulses[p] = 0;
    st.pulse_index[p].clear();
  }
}
static void rt_seek(WorldHipRealtime *rt, RtStream &st, double current_location, RtUndo *undo = nullptr) {   // SeekSynthesizer (:101-117)
  const int frame_number = static_cast<int>(current_location / rt->frame_period);
  int tmp_pointer = st.current_pointer2;
  for (int k = 0; k < st.head_pointer - st.current_pointer2; ++k) {
    const int p = (tmp_pointer + k) % rt->number_of_pointers;
    if (st.f0_origin[p] <= frame_number && frame_number < st.f0_origin[p] + st.f0_length[p]) {
      tmp_pointer += k;
      break;
    }
  }
  rt_clear_ring(rt, st, st.current_pointer2, tmp_pointer, undo);
  st.current_pointer2 = tmp_pointer;
}
static int rt_next_pulse(WorldHipRealtime *rt, RtStream &st) {                          // GetNextPulseLocationIndex (:380-393)
  int p = st.current_pointer % rt->number_of_pointers;
  if (st.i < st.number_of_pulses[p] - 1) return st.pulse_index[p][st.i + 1];
  if (st.current_pointer == st.head_pointer - 1) return 0;
  for (int k = 1; k < rt->number_of_pointers; ++k) {
    p = (k + st.current_pointer) % rt->number_of_pointers;
    if (st.number_of_pulses[p] != 0) return st.pulse_index[p][0];
  }
  return 0;
}
static void rt_update(WorldHipRealtime *rt, RtStream &st) {                             // UpdateSynthesizer (:395-413)
  int p = st.current_pointer % rt->number_of_pointers;
  if (st.i < st.number_of_pulses[p] - 1) { st.i++; return; }
  if (st.current_pointer == st.head_pointer - 1) return;
  for (int k = 1; k < rt->number_of_pointers; ++k) {
    p = (k + st.current_pointer) % rt->number_of_pointers;
    if (st.number_of_pulses[p] != 0) { st.i = 0; st.current_pointer += k; return; }
  }
}
static int rt_can_advance(WorldHipRealtime *rt, RtStream &st) {                          // CheckSynthesizer (:415-426)
  if (st.synthesized_sample + rt->buffer_size >= st.last_location) return 0;
  int p = st.current_pointer % rt->number_of_pointers;
  while (st.number_of_pulses[p] == 0) {
    if (st.current_pointer == st.head_pointer) break;
    st.current_pointer++;
    p = st.current_pointer % rt->number_of_pointers;
  }
  return 1;
}
static int rt_locked(WorldHipRealtime *rt, const RtStream &st) {                         // IsLocked (:566-575)
  int judge = 0;
  if (st.head_pointer - st.current_pointer2 == rt->number_of_pointers) judge++;
  if (st.synthesized_sample + rt->buffer_size >= st.last_location) judge++;
  return judge == 2 ? 1 : 0;
}

// GetTimeBase and what it calls (:283-378) for the chunk just entered in ring slot `pointer`: appends its pulses to the
// slot and to the stream's schedule.  Expression order is the reference's throughout (the unvoiced pulses of 16 / 32 /
// 48 kHz sit within an ulp of the fmod wrap).
static void rt_time_base(WorldHipRealtime *rt, RtStream &st, const double *f0, int f0_length, int start_sample,
                         int number_of_samples, int pointer) {
  const int fs = rt->fs, h = st.handoff, nk = f0_length + h;
  const double fp = rt->frame_period;
  std::vector<double> coarse_time_axis(nk), coarse_f0(nk), coarse_vuv(nk);
  const int cumulative_frame = std::max(0, st.cumulative_frame - f0_length);
  coarse_f0[0] = st.handoff_f0;
  coarse_time_axis[0] = cumulative_frame * fp;
  coarse_vuv[0] = st.handoff_f0 == 0 ? 0.0 : 1.0;
  for (int k = 0; k < f0_length; ++k) {
    coarse_time_axis[k + h] = (k + cumulative_frame + h) * fp;
    coarse_f0[k + h] = f0[k];
    coarse_vuv[k + h] = f0[k] == 0.0 ? 0.0 : 1.0;
  }
  const int n = number_of_samples;
  std::vector<double> interpolated_f0(n), time_axis(n), vuv(n + 1, 0.0);
  for (int k = 0; k < n; ++k) time_axis[k] = (k + start_sample) / static_cast<double>(fs);
  rt_interp1(coarse_time_axis.data(), coarse_f0.data(), nk, time_axis.data(), n, interpolated_f0.data());
  rt_interp1(coarse_time_axis.data(), coarse_vuv.data(), nk, time_axis.data(), n, vuv.data());
  for (int k = 0; k < n; ++k) {
    vuv[k] = vuv[k] > 0.5 ? 1.0 : 0.0;
    interpolated_f0[k] = vuv[k] == 0.0 ? kDefaultF0 : interpolated_f0[k];
  }
  // GetPulseLocationsForTimeBase (:298-339)
  std::vector<double> total_phase(std::max(2, n + h)), wrap_phase(n + h);
  total_phase[0] = h == 1 ? st.handoff_phase : 2.0 * kPi * interpolated_f0[0] / fs;
  total_phase[1] = total_phase[0] + 2.0 * kPi * interpolated_f0[0] / fs;
  for (int k = 1 + h; k < n + h; ++k) total_phase[k] = total_phase[k - 1] + 2.0 * kPi * interpolated_f0[k - h] / fs;
  st.handoff_phase = total_phase[n - 1 + h];
  for (int k = 0; k < n + h; ++k) wrap_phase[k] = fmod(total_phase[k], 2.0 * kPi);
  std::vector<int> &idx = st.pulse_index[pointer];
  idx.clear();
  for (int k = 0; k < n - 1 + h; ++k)
    if (fabs(wrap_phase[k + 1] - wrap_phase[k]) > kPi) {
      const double location = time_axis[k] - static_cast<double>(h) / fs;
      const int index = rt_round(location * fs);
      idx.push_back(index);
      // the V/UV GetCurrentVUV (:230-241) will read for this pulse: the slot's contour at index - start + 1
      const int at = index - start_sample + 1;
      st.sched.push_back(RtPulse{index, at >= 0 && at <= n ? vuv[at] : 0.0});
    }
  st.number_of_pulses[pointer] = (int)idx.size();
  if (!idx.empty()) st.last_location = idx.back();
  st.handoff_f0 = interpolated_f0[n - 1];
}

// Room in the stream's frame store for `n` more frames, keeping every frame a pulse still to be rendered may read.
static void rt_make_room(WorldHipRealtime *rt, RtStream &st, int n) {
  const int nb = rt->fft_size / 2 + 1;
  long long keep = std::max(0LL, st.frames - 2);               // the next chunk's first pulse may sit in the frame before
  if (st.rendered < st.sched_base + (long long)st.sched.size()) {
    const double t = (double)st.sched[st.rendered - st.sched_base].loc / rt->fs;
    keep = std::min(keep, (long long)std::max(0, static_cast<int>(t / rt->frame_period)));
  }
  keep = std::max(keep, st.store_lo);
  const long long need = st.frames + n - keep;
  if (need > st.store_cap) {
    const long long cap = std::max<long long>({need, 2LL * st.store_cap, 64LL});
    if (cap > (1LL << 30) / nb) fail("realtime: %lld frames to keep resident", need);
    double *sp = static_cast<double *>(devrt::dmalloc(sizeof(double) * cap * nb));
    double *ap = static_cast<double *>(devrt::dmalloc(sizeof(double) * cap * nb));
    for (long long g = keep; g < st.frames;) {
      const long long a = g % st.store_cap, b = g % cap;
      const long long len = std::min({st.store_cap - a, cap - b, st.frames - g});
      devrt::d2d(sp + b * nb, st.d_sp + a * nb, sizeof(double) * len * nb, rt->ctx->stream);
      devrt::d2d(ap + b * nb, st.d_ap + a * nb, sizeof(double) * len * nb, rt->ctx->stream);
      g += len;
    }
    devrt::sync(rt->ctx->stream);
    if (st.d_sp) devrt::dfree(st.d_sp);
    if (st.d_ap) devrt::dfree(st.d_ap);
    st.d_sp = sp; st.d_ap = ap; st.store_cap = (int)cap;
  }
  st.store_lo = keep;
}

// AddParameters (:480-519).  The rows are stored by `store(first_frame)`; returns 1, or 0 when the ring is full.
template <class Store>
static int rt_add(WorldHipRealtime *rt, int s, const double *f0, int f0_length, Store store) {
  rt_check_stream(rt, s);
  if (!f0) fail("null f0");
  if (f0_length < 1) fail("f0_length %d: a chunk holds at least one frame", f0_length);
  RtStream &st = rt->streams[s];
  if (st.head_pointer - st.current_pointer2 == rt->number_of_pointers) return 0;
  rt_make_room(rt, st, f0_length);
  store(st.frames);
  st.frames += f0_length;
  const int pointer = st.head_pointer % rt->number_of_pointers;
  st.f0_length[pointer] = f0_length;
  st.f0_origin[pointer] = st.cumulative_frame + 1;
  st.cumulative_frame += f0_length;
  st.pulse_index[pointer].clear();
  if (st.cumulative_frame < 1) {
    st.handoff_f0 = f0[f0_length - 1];
    st.number_of_pulses[pointer] = 0;
    st.head_pointer++;
    st.handoff = 1;
    return 1;
  }
  const int start_sample =
      std::max(0, static_cast<int>(ceil((st.cumulative_frame - f0_length) * rt->frame_period * rt->fs)));
  const int end_sample = static_cast<int>(ceil((st.cumulative_frame) * rt->frame_period * rt->fs));
  const int number_of_samples = end_sample - start_sample;
  if (number_of_samples >= 1) rt_time_base(rt, st, f0, f0_length, start_sample, number_of_samples, pointer);
  else st.number_of_pulses[pointer] = 0;         // (the reference's arrays would be empty: undefined there)
  st.handoff_f0 = f0[f0_length - 1];
  st.head_pointer++;
  st.handoff = 1;
  return 1;
}

static int floor_multiple(int x, int m) { return (x >= 0 ? x / m : -((-x + m - 1) / m)) * m; }

// Render pulses of the streams in `who` (each with a successor), overlap-add, and move the samples that are now finished
// into the streams' windows.  Two launches; one synchronisation for the download.  A batch holds at most
// rt_batch_pulses(): first every stream gets the pulses its next buffer needs (those before need[k]), in order while the
// budget lasts; what is left renders further ahead, stream by stream.  Nothing of a stream changes unless the batch
// completes.  Returns the number of pulses rendered.
static size_t rt_render(WorldHipRealtime *rt, const std::vector<int> &who, const std::vector<int> &need) {
  const int N = rt->fft_size, H = N / 2, bs = rt->buffer_size;
  hipStream_t stream = rt->ctx->stream;
  size_t budget = rt_batch_pulses(N);
  const size_t ns = who.size();
  std::vector<long long> take(ns, 0), avail(ns, 0);
  for (size_t k = 0; k < ns; ++k) {                  // pass 1: what each stream's next buffer needs
    const RtStream &st = rt->streams[who[k]];
    avail[k] = std::max(0LL, st.sched_base + (long long)st.sched.size() - 1 - st.rendered);
    long long m = 0;
    while (m < avail[k] && st.sched[st.rendered + m - st.sched_base].loc < need[k]) ++m;
    take[k] = std::min<long long>(m, (long long)budget);
    budget -= (size_t)take[k];
  }
  for (size_t k = 0; k < ns && budget > 0; ++k) {    // pass 2: render ahead with what is left
    const long long more = std::min<long long>(avail[k] - take[k], (long long)budget);
    take[k] += more;
    budget -= (size_t)more;
  }
  rt->jobs.clear();
  rt->ola.clear();
  std::vector<int> out_at, out_len, sid;
  std::vector<long long> upto;
  std::vector<RtRng> rng_after;
  size_t finals = 0;
  int max_span = 0;
  for (size_t k = 0; k < ns; ++k) {
    if (take[k] <= 0) continue;
    const int s = who[k];
    const RtStream &st = rt->streams[s];
    const long long last = st.rendered + take[k];                        // render [rendered, last)
    RtRng rng = st.render_rng;
    RtOlaStream o;
    o.p0 = (int)rt->jobs.size();
    o.lo = st.final_end;
    o.tail_end = st.tail_end;
    int hi = st.tail_end;
    for (long long q = st.rendered; q < last; ++q) {
      const RtPulse &pu = st.sched[q - st.sched_base];
      const int next = st.sched[q + 1 - st.sched_base].loc;
      RtPulseJob j;
      const double t = static_cast<double>(pu.loc) / rt->fs;
      const int ff = static_cast<int>(t / rt->frame_period), fc = static_cast<int>(ceil(t / rt->frame_period));
      j.wgt = t / rt->frame_period - ff;
      j.same = ff == fc;
      auto row = [&](long long g) { return std::min(std::max(g, st.store_lo), st.frames - 1) % st.store_cap; };
      j.sp0 = st.d_sp + row(ff) * (N / 2 + 1);
      j.ap0 = st.d_ap + row(ff) * (N / 2 + 1);
      j.sp1 = st.d_sp + row((long long)ff + 1) * (N / 2 + 1);
      j.ap1 = st.d_ap + row((long long)ff + 1) * (N / 2 + 1);
      j.vuv = pu.vuv;
      j.rng[0] = rng.x; j.rng[1] = rng.y; j.rng[2] = rng.z; j.rng[3] = rng.w;
      const long long draws = (long long)next - pu.loc;
      // (a noise_size outside 1 .. fft_size overruns the reference's buffers: undefined there, clamped here)
      j.noise_size = (int)std::min<long long>(std::max<long long>(draws, 1), N);
      if (draws > 0) rng = rt_jump(rng, (unsigned long long)draws);
      j.loc = pu.loc;
      j.first = floor_multiple(pu.loc, bs);
      hi = std::max(hi, pu.loc + H + 1);
      rt->jobs.push_back(j);
    }
    o.np = (int)rt->jobs.size() - o.p0;
    const int next_loc = st.sched[last - st.sched_base].loc;             // the first pulse not rendered yet
    const int fin = std::max(st.final_end, floor_multiple(next_loc, bs));
    hi = std::max(hi, fin);
    if (hi - fin > rt->tail_cap) fail("realtime: partial sums beyond the tail (%d > %d)", hi - fin, rt->tail_cap);
    o.hi = hi;
    o.final_end = fin;
    double *tails = rt->d_tails + (size_t)s * 2 * rt->tail_cap;
    o.tail_in = tails + (size_t)st.tail_par * rt->tail_cap;
    o.tail_out = tails + (size_t)(1 - st.tail_par) * rt->tail_cap;
    o.out = nullptr;
    out_at.push_back((int)finals);
    out_len.push_back(fin - o.lo);
    finals += (size_t)(fin - o.lo);
    max_span = std::max(max_span, hi - o.lo);
    rt->ola.push_back(o);
    sid.push_back(s);
    upto.push_back(last);
    rng_after.push_back(rng);
  }
  if (rt->ola.empty()) return 0;
  // workspace (grow-only)
  const size_t np = rt->jobs.size(), stride = (size_t)rt_resp_stride(N);
  if (np > rt->jobs_cap) {
    devrt::sync(stream);
    if (rt->d_jobs) devrt::dfree(rt->d_jobs);
    rt->d_jobs = nullptr; rt->jobs_cap = 0;
    rt->d_jobs = static_cast<RtPulseJob *>(devrt::dmalloc(sizeof(RtPulseJob) * (np + np / 2 + 16)));
    rt->jobs_cap = np + np / 2 + 16;
  }
  if (np > rt->resp_cap) {
    devrt::sync(stream);
    if (rt->d_resp) devrt::dfree(rt->d_resp);
    rt->d_resp = nullptr; rt->resp_cap = 0;
    const size_t cap = std::min(rt_batch_pulses(N), np + np / 2 + 16);
    rt->d_resp = static_cast<double *>(devrt::dmalloc(sizeof(double) * stride * cap));
    rt->resp_cap = cap;
  }
  if (finals > rt->stage_cap) {
    devrt::sync(stream);
    if (rt->d_stage) devrt::dfree(rt->d_stage);
    if (rt->h_stage) devrt::hfree_pinned(rt->h_stage);
    rt->d_stage = nullptr; rt->h_stage = nullptr; rt->stage_cap = 0;
    const size_t cap = finals + finals / 2 + 4096;
    rt->d_stage = static_cast<double *>(devrt::dmalloc(sizeof(double) * cap));
    rt->h_stage = static_cast<double *>(devrt::hmalloc_pinned(sizeof(double) * cap));
    rt->stage_cap = cap;
  }
  for (size_t k = 0; k < rt->ola.size(); ++k) rt->ola[k].out = rt->d_stage + out_at[k];
  devrt::h2d(rt->d_jobs, rt->jobs.data(), sizeof(RtPulseJob) * np, stream);
  devrt::h2d(rt->d_ola, rt->ola.data(), sizeof(RtOlaStream) * rt->ola.size(), stream);
  RtParams p;
  p.fft_size = N; p.lg_fft = rt->lg_fft;
  p.n_pulses = (int)np;
  p.jobs = rt->d_jobs;
  p.resp = rt->d_resp;
  p.resp_stride = (int)stride;
  p.dc_remover = rt->d_dc_remover;
  p.ola = rt->d_ola;
  p.n_streams = (int)rt->ola.size();
  p.tab = rt->ctx->tab;
  launch_rt_pulse(p, stream);
  launch_rt_overlap_add(p, max_span, stream);
  if (finals) devrt::d2h(rt->h_stage, rt->d_stage, sizeof(double) * finals, stream);
  devrt::sync(stream);
  for (size_t k = 0; k < rt->ola.size(); ++k) {      // the batch is complete: commit it
    RtStream &st = rt->streams[sid[k]];
    const RtOlaStream &o = rt->ola[k];
    st.window.insert(st.window.end(), rt->h_stage + out_at[k], rt->h_stage + out_at[k] + out_len[k]);
    st.final_end = o.final_end;
    st.tail_end = o.hi;
    st.tail_par = 1 - st.tail_par;
    st.rendered = upto[k];
    st.render_rng = rng_after[k];
  }
  return np;
}

// What Synthesis2 changes in a stream, for putting it back when a call fails half-way: the scalar fields and the ring
// slots SeekSynthesizer cleared (their contents are moved into the log, not freed).
struct RtUndo {
  int current_pointer, i, current_pointer2, synthesized_sample;
  RtRng ref_rng;
  long long ref_next;
  struct Slot { int slot, pulses; std::vector<int> index; };
  std::vector<Slot> cleared;
};
static void rt_undo_clear(RtUndo *undo, int slot, int pulses, std::vector<int> &index) {
  undo->cleared.push_back(RtUndo::Slot{slot, pulses, std::vector<int>()});
  undo->cleared.back().index.swap(index);
}
static void rt_save(const RtStream &st, RtUndo &u) {
  u.current_pointer = st.current_pointer; u.i = st.i; u.current_pointer2 = st.current_pointer2;
  u.synthesized_sample = st.synthesized_sample; u.ref_rng = st.ref_rng; u.ref_next = st.ref_next;
  u.cleared.clear();
}
static void rt_restore(RtStream &st, RtUndo &u) {
  for (size_t k = u.cleared.size(); k-- > 0;) {
    RtUndo::Slot &c = u.cleared[k];
    st.number_of_pulses[c.slot] = c.pulses;
    st.pulse_index[c.slot].swap(c.index);
  }
  u.cleared.clear();
  st.current_pointer = u.current_pointer; st.i = u.i; st.current_pointer2 = u.current_pointer2;
  st.synthesized_sample = u.synthesized_sample; st.ref_rng = u.ref_rng; st.ref_next = u.ref_next;
}

// Synthesis2 (:577-603) of one stream whose samples [synthesized_sample, + buffer_size) are finished: walks the pulses
// the reference renders in this call, checking each against the one rendered ahead, and copies the buffer out.
static void rt_advance(WorldHipRealtime *rt, RtStream &st, double *out, RtUndo *undo) {
  const int bs = rt->buffer_size, ss = st.synthesized_sample;
  const int pointer = st.current_pointer % rt->number_of_pointers;
  int current_location = st.pulse_index[pointer][st.i];
  while (current_location < ss + bs) {
    const int tmp = rt_next_pulse(rt, st);
    const int noise_size = tmp - current_location;
    // the pulse the reference renders here must be the one rendered ahead
    const long long q = st.ref_next - st.sched_base;
    if (st.ref_next >= st.rendered || q < 0 || st.sched[q].loc != current_location || st.sched[q + 1].loc != tmp)
      fail("realtime: the ring no longer holds pulse %lld where it was scheduled (a frame outside every chunk?)",
           st.ref_next);
    rt_seek(rt, st, static_cast<double>(current_location) / rt->fs, undo);   // GetOneFrameSegment's seek (:253-254)
    if (noise_size > 0) st.ref_rng = rt_jump(st.ref_rng, (unsigned long long)noise_size);
    ++st.ref_next;
    current_location = tmp;
    rt_update(rt, st);
  }
  if (out) memcpy(out, st.window.data() + (ss - st.win_lo), sizeof(double) * bs);
  st.synthesized_sample += bs;
  rt_seek(rt, st, st.synthesized_sample, undo);  // (:601: the sample count goes in where a time in seconds is expected)
}

// drop what no later call reads: output before the playhead, pulses behind both cursors
static void rt_trim(RtStream &st) {
  const int drop = st.synthesized_sample - st.win_lo;
  if (drop > 0 && drop >= (int)st.window.size() / 2) {
    st.window.erase(st.window.begin(), st.window.begin() + std::min<size_t>(drop, st.window.size()));
    st.win_lo += drop;
  }
  while (!st.sched.empty() && st.sched_base + 1 < std::min(st.ref_next, st.rendered)) { st.sched.pop_front(); ++st.sched_base; }
}

// One Synthesis2 call for the streams in `who`: outs[k] gets stream who[k]'s buffer and produced[k] its return value.
// Renders first (as many batches as the pulses need), then advances every stream; if anything fails, every stream's
// control state is as it was before the call.
static void rt_synthesize(WorldHipRealtime *rt, const std::vector<int> &who, double *const *outs, int *produced) {
  const size_t n = who.size();
  const int bs = rt->buffer_size;
  std::vector<RtUndo> undo(n);
  std::vector<int> can(n, 0);
  size_t k = 0;
  try {
    for (k = 0; k < n; ++k) {
      rt_save(rt->streams[who[k]], undo[k]);
      can[k] = rt_can_advance(rt, rt->streams[who[k]]);
    }
    for (;;) {
      std::vector<int> ids, need;
      for (size_t j = 0; j < n; ++j) {
        const RtStream &st = rt->streams[who[j]];
        if (can[j] && st.synthesized_sample + bs > st.final_end) { ids.push_back(who[j]); need.push_back(st.synthesized_sample + bs); }
      }
      if (ids.empty()) break;
      if (rt_render(rt, ids, need) == 0) fail("realtime: stream %d needs samples no scheduled pulse finishes", ids[0]);
    }
    for (size_t j = 0; j < n; ++j)
      if (can[j]) rt_advance(rt, rt->streams[who[j]], outs[j], &undo[j]);
  } catch (...) {
    for (size_t j = std::min(k, n); j-- > 0;) rt_restore(rt->streams[who[j]], undo[j]);
    throw;
  }
  for (size_t j = 0; j < n; ++j) {
    produced[j] = can[j];
    rt_trim(rt->streams[who[j]]);
  }
}

static WorldHipRealtime *rt_create(WorldHipContext *c, int n_streams, int fs, double frame_period_ms, int fft_size,
                                   int buffer_size, int number_of_pointers) {
  if (n_streams < 1) fail("n_streams must be positive");
  if (fs <= 0) fail("fs must be positive");
  if (!(frame_period_ms > 0.0) || !std::isfinite(frame_period_ms)) fail("frame_period must be positive");
  if (buffer_size < 1) fail("buffer_size must be positive");
  if (number_of_pointers < 1) fail("number_of_pointers must be positive");
  const std::string lim = shape_limit(8, fs, fft_size);                 // fft_size and the pair (fs, fft_size), before any allocation
  if (!lim.empty()) fail("realtime synthesis: %s", lim.c_str());
  const int lg = ilog2_exact(fft_size);
  WorldHipRealtime *rt = new WorldHipRealtime;
  try {
    rt->ctx = c;
    rt->n_streams = n_streams; rt->fs = fs; rt->fft_size = fft_size; rt->lg_fft = lg;
    rt->buffer_size = buffer_size; rt->number_of_pointers = number_of_pointers;
    rt->frame_period = frame_period_ms / 1000.0;
    // GetDCRemover(fft_size / 2) (:428-440)
    const int half = fft_size / 2;
    rt->dc_remover.assign(half, 0.0);
    double dc_component = 0.0;
    for (int k = 0; k < half / 2; ++k) {
      rt->dc_remover[k] = 0.5 - 0.5 * cos(2.0 * kPi * (k + 1.0) / (1.0 + half));
      rt->dc_remover[half - k - 1] = rt->dc_remover[k];
      dc_component += rt->dc_remover[k] * 2.0;
    }
    for (int k = 0; k < half / 2; ++k) {
      rt->dc_remover[k] /= dc_component;
      rt->dc_remover[half - k - 1] = rt->dc_remover[k];
    }
    rt->d_dc_remover = static_cast<double *>(devrt::dmalloc(sizeof(double) * half));
    devrt::h2d(rt->d_dc_remover, rt->dc_remover.data(), sizeof(double) * half, c->stream);
    rt->tail_cap = buffer_size + fft_size + 64;
    rt->d_tails = static_cast<double *>(devrt::dmalloc(sizeof(double) * 2 * rt->tail_cap * (size_t)n_streams));
    rt->d_ola = static_cast<RtOlaStream *>(devrt::dmalloc(sizeof(RtOlaStream) * n_streams));
    rt->streams.resize(n_streams);
    for (RtStream &st : rt->streams) {
      st.f0_length.assign(number_of_pointers, 0);
      st.f0_origin.assign(number_of_pointers, 0);
      st.number_of_pulses.assign(number_of_pointers, 0);
      st.pulse_index.assign(number_of_pointers, std::vector<int>());
      rt_reset(rt, st);
    }
    for (int h = 0; h < 2; ++h) { rt->out_ev[h] = devrt::event_create(); rt->rows_ev[h] = devrt::event_create(); }
    rt_host_jump();
    devrt::sync(c->stream);
  } catch (...) {
    delete rt;                                     // (what was allocated stays with the failed call: rare, and small)
    throw;
  }
  return rt;
}

static void rt_free(WorldHipRealtime *rt) {
  if (!rt) return;
  hipStream_t stream = rt->ctx ? rt->ctx->stream : nullptr;
  try {
    devrt::sync(stream);
    for (RtStream &st : rt->streams) { if (st.d_sp) devrt::dfree(st.d_sp); if (st.d_ap) devrt::dfree(st.d_ap); }
    for (void *p : {(void *)rt->d_dc_remover, (void *)rt->d_tails, (void *)rt->d_jobs, (void *)rt->d_resp,
                    (void *)rt->d_ola, (void *)rt->d_stage})
      if (p) devrt::dfree(p);
    for (double *p : {rt->h_stage, rt->h_out[0], rt->h_out[1], rt->h_rows[0], rt->h_rows[1]})
      if (p) devrt::hfree_pinned(p);
    for (int h = 0; h < 2; ++h) {
      if (rt->out_ev[h]) devrt::event_destroy(rt->out_ev[h]);
      if (rt->rows_ev[h]) devrt::event_destroy(rt->rows_ev[h]);
    }
  } catch (...) {
  }
  delete rt;
}

template <class F> static int rt_guarded(WorldHipRealtime *rt, F f) {
  if (!rt) { g_last_error = "null realtime synthesiser"; return -1; }
  int r = -1;
  const int rc = guarded(rt->ctx, [&] { r = f(); });
  return rc == 0 ? r : -1;
}

}  // namespace world_hip

extern "C" {

int world_hip_realtime_create(WorldHipContext *c, int n_streams, int fs, double frame_period_ms, int fft_size,
                              int buffer_size, int number_of_pointers, WorldHipRealtime **out) {
  if (out) *out = nullptr;
  return guarded(c, [&] {
    if (!out) fail("null output pointer");
    *out = rt_create(c, n_streams, fs, frame_period_ms, fft_size, buffer_size, number_of_pointers);
  });
}

void world_hip_realtime_destroy(WorldHipRealtime *rt) {
  if (!rt) return;
  WorldHipContext *c = rt->ctx;
  if (!c) { rt_free(rt); return; }
  std::lock_guard<std::mutex> g(c->lock);
  try { DeviceScope on_device(c->device); rt_free(rt); } catch (...) {}
}

int world_hip_realtime_add(WorldHipRealtime *rt, int stream, const double *f0, int n_frames, const double *d_sp,
                           const double *d_ap, int row_stride) {
  return rt_guarded(rt, [&] {
    const int nb = rt->fft_size / 2 + 1;
    if (!d_sp || !d_ap) fail("null spectrogram / aperiodicity rows");
    if (row_stride < nb) fail("row_stride %d < fft_size / 2 + 1 = %d", row_stride, nb);
    return rt_add(rt, stream, f0, n_frames, [&](long long first) {
      RtStream &st = rt->streams[stream];
      launch_rt_store_rows(st.d_sp, st.store_cap, nb, first, d_sp, row_stride, n_frames, rt->ctx->stream);
      launch_rt_store_rows(st.d_ap, st.store_cap, nb, first, d_ap, row_stride, n_frames, rt->ctx->stream);
    });
  });
}

// AddParameters of a chunk whose rows are coded: rt_store_coded_rows (codec.hip) decodes them straight into the stream's
// frame store -- the decoders' arithmetic, their refusals
int world_hip_realtime_add_coded(WorldHipRealtime *rt, int stream, const double *f0, int n_frames, const double *d_coded_sp,
                                 int number_of_dimensions, const double *d_coded_ap, int row_stride) {
  return rt_guarded(rt, [&] {
    WorldHipContext *c = rt->ctx;
    const int fs = rt->fs, fft_size = rt->fft_size, ndim = number_of_dimensions;
    if (!d_coded_sp || !d_coded_ap) fail("null coded spectral envelope / aperiodicity rows");
    const int nap = world_hip::number_of_aperiodicities(fs);
    if (nap < 1) fail("realtime_add_coded: fs=%d has no aperiodicity band (needs fs >= 12 kHz)", fs);
    if (3000.0 * nap > fs / 2.0) fail("realtime_add_coded: band centre beyond fs/2");
    if (ndim < 1 || ndim > fft_size / 4 + 1)
      fail("realtime_add_coded: number_of_dimensions %d outside [1, fft_size/4+1]", ndim);
    if (row_stride < std::max(ndim, nap)) fail("row_stride %d < the %d values of a coded row", row_stride, std::max(ndim, nap));
    return rt_add(rt, stream, f0, n_frames, [&](long long first) {
      RtStream &st = rt->streams[stream];
      const CodecTables &t = codec_tables(c, fs, fft_size);
      RtCodedRowsParams p;
      p.dst_sp = st.d_sp; p.dst_ap = st.d_ap; p.cap = st.store_cap; p.n = n_frames; p.first = first;
      p.coded_sp = d_coded_sp; p.coded_ap = d_coded_ap; p.row_stride = row_stride;
      p.fft_size = fft_size; p.lg_md = rt->lg_fft - 1; p.ndim = ndim; p.nap = nap;
      p.knot_sp = t.d_knot_dec; p.frac_sp = t.d_frac_dec; p.w_re = t.d_wd_re; p.w_im = t.d_wd_im;
      p.knot_ap = t.d_knot_ap; p.frac_ap = t.d_frac_ap;
      p.tab = c->tab;
      launch_rt_store_coded_rows(p, c->stream);
    });
  });
}

int world_hip_realtime_synthesize(WorldHipRealtime *rt, double *d_out, int *produced) {
  return rt_guarded(rt, [&] {
    if (!d_out || !produced) fail("null output");
    const int n = rt->n_streams, bs = rt->buffer_size;
    const int h = rt->out_half;
    if (!rt->h_out[h]) rt->h_out[h] = static_cast<double *>(devrt::hmalloc_pinned(sizeof(double) * (size_t)n * bs));
    if (rt->out_busy[h]) { devrt::event_sync(rt->out_ev[h]); rt->out_busy[h] = false; }
    double *host = rt->h_out[h];
    std::vector<int> who(n);
    std::vector<double *> outs(n);
    for (int s = 0; s < n; ++s) { who[s] = s; outs[s] = host + (size_t)s * bs; }
    rt_synthesize(rt, who, outs.data(), produced);
    for (int s = 0; s < n; ++s)
      if (!produced[s]) memset(outs[s], 0, sizeof(double) * bs);
    devrt::h2d(d_out, host, sizeof(double) * (size_t)n * bs, rt->ctx->stream);
    devrt::event_record(rt->out_ev[h], rt->ctx->stream);
    rt->out_busy[h] = true;
    rt->out_half = 1 - h;
    return 0;
  });
}

int world_hip_realtime_is_locked(WorldHipRealtime *rt, int stream) {
  return rt_guarded(rt, [&] {
    rt_check_stream(rt, stream);
    return rt_locked(rt, rt->streams[stream]);
  });
}

int world_hip_realtime_refresh(WorldHipRealtime *rt, int stream) {
  return rt_guarded(rt, [&] {
    rt_check_stream(rt, stream);
    rt_reset(rt, rt->streams[stream]);
    return 0;
  });
}

// the randn() state `draws` calls after `state` (x, y, z, w), by the jump matrices the scheduler uses (test hook)
void world_hip_realtime_rng_jump(const unsigned int *state, unsigned long long draws, unsigned int *out) {
  world_hip::RtRng s{state[0], state[1], state[2], state[3]};
  s = world_hip::rt_jump(s, draws);
  out[0] = s.x; out[1] = s.y; out[2] = s.z; out[3] = s.w;
}

}  // extern "C"
