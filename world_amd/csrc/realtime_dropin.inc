// realtime_dropin.inc -- the drop-in WorldSynthesizer symbols of include/world_hip.h (reference
// src/synthesisrealtime.cpp), included by dropin.inc.  Each synthesiser is a one-stream WorldHipRealtime (realtime.inc)
// on a library context and stream of its own, for as long as the caller keeps it: the handle lives in the struct's
// `spectrogram` field.  The public fields are mirrored from the stream after every call.

namespace world_hip {

static WorldHipRealtime *rt_of(WorldSynthesizer *synth) {
  if (!synth) throw std::runtime_error("null synthesizer");
  WorldHipRealtime *rt = reinterpret_cast<WorldHipRealtime *>(synth->spectrogram);
  if (!rt) throw std::runtime_error("synthesizer not initialised (InitializeSynthesizer)");
  return rt;
}

static void rt_mirror(WorldHipRealtime *rt, WorldSynthesizer *synth) {
  const RtStream &st = rt->streams[0];
  synth->current_pointer = st.current_pointer;
  synth->i = st.i;
  synth->current_pointer2 = st.current_pointer2;
  synth->head_pointer = st.head_pointer;
  synth->synthesized_sample = st.synthesized_sample;
  synth->handoff = st.handoff;
  synth->handoff_phase = st.handoff_phase;
  synth->handoff_f0 = st.handoff_f0;
  synth->last_location = st.last_location;
  synth->cumulative_frame = st.cumulative_frame;
  synth->current_frame = st.current_frame;
  for (int k = 0; k < rt->number_of_pointers; ++k) {
    synth->f0_length[k] = st.f0_length[k];
    synth->f0_origin[k] = st.f0_origin[k];
    synth->number_of_pulses[k] = st.number_of_pulses[k];
    synth->pulse_locations_index[k] = st.pulse_index[k].empty() ? nullptr : const_cast<int *>(st.pulse_index[k].data());
  }
  synth->randn_state.g_randn_x = st.ref_rng.x;
  synth->randn_state.g_randn_y = st.ref_rng.y;
  synth->randn_state.g_randn_z = st.ref_rng.z;
  synth->randn_state.g_randn_w = st.ref_rng.w;
}

// a drop-in call on the synthesiser's own context: its lock and device; failures go to the error handler
template <class F> static void rt_dropin(const char *what, WorldSynthesizer *synth, F f) {
  std::string failure;
  try {
    WorldHipRealtime *rt = rt_of(synth);
    std::lock_guard<std::mutex> g(rt->ctx->lock);
    DeviceScope on_device(rt->ctx->device);
    f(rt);
    rt_mirror(rt, synth);
    return;
  } catch (const std::exception &e) {
    failure = e.what();
  }
  report_failure(what, failure);
}

// the caller's rows of frames [first, first + n) -> the stream's frame store, through the synthesiser's pinned staging
static void rt_store_host_rows(WorldHipRealtime *rt, long long first, const double *const *sp, const double *const *ap,
                               int n) {
  RtStream &st = rt->streams[0];
  const int nb = rt->fft_size / 2 + 1;
  const size_t need = (size_t)2 * n * nb;
  hipStream_t stream = rt->ctx->stream;
  if (need > rt->rows_cap) {
    devrt::sync(stream);
    for (int h = 0; h < 2; ++h) {
      if (rt->h_rows[h]) devrt::hfree_pinned(rt->h_rows[h]);
      rt->h_rows[h] = nullptr;
      rt->rows_busy[h] = false;
    }
    rt->rows_cap = 0;
    const size_t cap = need + need / 2 + (size_t)8 * nb;
    for (int h = 0; h < 2; ++h) rt->h_rows[h] = static_cast<double *>(devrt::hmalloc_pinned(sizeof(double) * cap));
    rt->rows_cap = cap;
  }
  const int h = rt->rows_half;
  if (rt->rows_busy[h]) { devrt::event_sync(rt->rows_ev[h]); rt->rows_busy[h] = false; }
  double *hs = rt->h_rows[h], *ha = hs + (size_t)n * nb;
  for (int r = 0; r < n; ++r) {
    memcpy(hs + (size_t)r * nb, sp[r], sizeof(double) * nb);
    memcpy(ha + (size_t)r * nb, ap[r], sizeof(double) * nb);
  }
  for (long long g = first; g < first + n;) {           // at most two pieces: the store is a ring of frames
    const long long at = g % st.store_cap, len = std::min<long long>(st.store_cap - at, first + n - g);
    devrt::h2d(st.d_sp + at * nb, hs + (g - first) * nb, sizeof(double) * len * nb, stream);
    devrt::h2d(st.d_ap + at * nb, ha + (g - first) * nb, sizeof(double) * len * nb, stream);
    g += len;
  }
  devrt::event_record(rt->rows_ev[h], stream);
  rt->rows_busy[h] = true;
  rt->rows_half = 1 - h;
}

static void rt_dropin_release(WorldHipRealtime *rt) {
  WorldHipContext *c = rt->ctx;
  hipStream_t stream = c ? c->stream : nullptr;
  if (c) { DeviceScope on_device(c->device); rt_free(rt); }
  else rt_free(rt);
  if (c) {
    world_hip_destroy(c);
    try { devrt::stream_destroy(stream); } catch (...) {}
  }
}

}  // namespace world_hip

extern "C" {

void InitializeSynthesizer(int fs, double frame_period, int fft_size, int buffer_size, int number_of_pointers,
                           WorldSynthesizer *synth) {
  using namespace world_hip;
  std::string failure;
  try {
    if (!synth) throw std::runtime_error("null synthesizer");
    DropinPool &P = dropin_pool();
    DeviceScope on_device(P.device);
    WorldHipContext *c = nullptr;
    WorldHipRealtime *rt = nullptr;
    // the shape is checked before anything touches the GPU
    if (buffer_size < 1 || number_of_pointers < 1 || fs <= 0 || !(frame_period > 0.0))
      throw std::runtime_error("fs, frame_period, buffer_size and number_of_pointers must be positive");
    const std::string lim = shape_limit(8, fs, fft_size);
    if (!lim.empty()) throw std::runtime_error(lim);
    hipStream_t st = devrt::stream_create();
    c = world_hip_create(P.device, st);
    if (!c) {
      devrt::stream_destroy(st);
      throw std::runtime_error(std::string("cannot initialise the GPU path: ") + world_hip_last_error());
    }
    if (world_hip_realtime_create(c, 1, fs, frame_period, fft_size, buffer_size, number_of_pointers, &rt) != 0) {
      const std::string why = world_hip_last_error();
      world_hip_destroy(c);
      devrt::stream_destroy(st);
      throw std::runtime_error(why);
    }
    rt->own_ctx = true;
    memset(synth, 0, sizeof *synth);
    synth->fs = fs;
    synth->frame_period = frame_period / 1000.0;
    synth->buffer_size = buffer_size;
    synth->number_of_pointers = number_of_pointers;
    synth->fft_size = fft_size;
    synth->buffer = new double[(size_t)buffer_size * 2 + fft_size]();
    synth->dc_remover = new double[fft_size / 2];
    memcpy(synth->dc_remover, rt->dc_remover.data(), sizeof(double) * (fft_size / 2));
    synth->f0_length = new int[number_of_pointers]();
    synth->f0_origin = new int[number_of_pointers]();
    synth->number_of_pulses = new int[number_of_pointers]();
    synth->pulse_locations_index = new int *[number_of_pointers]();
    synth->spectrogram = reinterpret_cast<double ***>(rt);
    rt_mirror(rt, synth);
    return;
  } catch (const std::exception &e) {
    failure = e.what();
  }
  report_failure("InitializeSynthesizer", failure);
}

int AddParameters(double *f0, int f0_length, double **spectrogram, double **aperiodicity, WorldSynthesizer *synth) {
  using namespace world_hip;
  int r = 0;
  rt_dropin("AddParameters", synth, [&](WorldHipRealtime *rt) {
    if (!spectrogram || !aperiodicity) throw std::runtime_error("null spectrogram / aperiodicity");
    for (int k = 0; k < f0_length; ++k)
      if (!spectrogram[k] || !aperiodicity[k]) throw std::runtime_error("null spectrogram / aperiodicity row");
    r = rt_add(rt, 0, f0, f0_length, [&](long long first) {
      rt_store_host_rows(rt, first, spectrogram, aperiodicity, f0_length);
    });
  });
  return r;
}

int Synthesis2(WorldSynthesizer *synth) {
  using namespace world_hip;
  int produced = 0;
  rt_dropin("Synthesis2", synth, [&](WorldHipRealtime *rt) {
    std::vector<int> who(1, 0);
    double *out = synth->buffer;
    rt_synthesize(rt, who, &out, &produced);
  });
  return produced;
}

int IsLocked(WorldSynthesizer *synth) {
  using namespace world_hip;
  int r = 0;
  rt_dropin("IsLocked", synth, [&](WorldHipRealtime *rt) { r = rt_locked(rt, rt->streams[0]); });
  return r;
}

void RefreshSynthesizer(WorldSynthesizer *synth) {
  using namespace world_hip;
  rt_dropin("RefreshSynthesizer", synth, [&](WorldHipRealtime *rt) {
    rt_reset(rt, rt->streams[0]);
    memset(synth->buffer, 0, sizeof(double) * ((size_t)rt->buffer_size * 2 + rt->fft_size));
  });
}

void DestroySynthesizer(WorldSynthesizer *synth) {
  using namespace world_hip;
  std::string failure;
  try {
    WorldHipRealtime *rt = rt_of(synth);
    synth->spectrogram = nullptr;
    rt_dropin_release(rt);
  } catch (const std::exception &e) {
    failure = e.what();
  }
  if (synth) {
    delete[] synth->buffer;
    delete[] synth->dc_remover;
    delete[] synth->f0_length;
    delete[] synth->f0_origin;
    delete[] synth->number_of_pulses;
    delete[] synth->pulse_locations_index;
    synth->buffer = synth->dc_remover = nullptr;
    synth->f0_length = synth->f0_origin = synth->number_of_pulses = nullptr;
    synth->pulse_locations_index = nullptr;
  }
  if (!failure.empty()) report_failure("DestroySynthesizer", failure);
}

}  // extern "C"
