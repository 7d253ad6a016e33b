"""Real-time synthesis (reference src/synthesisrealtime.cpp) without a GPU: the WorldSynthesizer layout, the drop-in
header, and the emulated library (tests/emu: the pulse kernel runs on the SIMT emulator) against the unmodified
reference's recordings in tests/golden/realtime.npz (make_golden_realtime.py)."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from backends import EMU_DIR, ROOT, emu  # noqa: F401 (emu: a fixture)
from util import GOLDEN

REF = "/root/reference"


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_realtime", os.path.join(GOLDEN, "make_golden_realtime.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
FIX = np.load(os.path.join(GOLDEN, "realtime.npz"))
NAMES = [str(n) for n in FIX["names"]]


def plan_of(name):
    return GEN.cases()[name]


def check_against_fixture(rec, name, tol):
    """control exactly (return values, scalar fields, randn_state, pulses, ring arrays), buffers within tol of the peak"""
    want = {k: FIX[f"{name}.{k}"] for k in ("calls", "out", "pulses", "pulse_counts", "rings")}
    assert rec["calls"].shape == want["calls"].shape, (rec["calls"].shape, want["calls"].shape)
    bad = np.argwhere(rec["calls"] != want["calls"])
    assert bad.size == 0, f"{name}: control differs first at call {bad[0][0]} column {bad[0][1]}"
    for k in ("pulses", "pulse_counts", "rings"):
        assert np.array_equal(rec[k], want[k]), f"{name}: {k} differ"
    assert rec["out"].shape == want["out"].shape and want["out"].size > 0
    peak = np.abs(want["out"]).max()
    err = np.abs(rec["out"] - want["out"]).max() / peak
    assert err <= tol, f"{name}: buffer error {err:.3e} of the peak"


def _compile_layout(tmp_path, include_dir, header):
    src = tmp_path / "layout.cpp"
    body = "".join(f'  printf("%zu\\n", offsetof(WorldSynthesizer, {f}));\n' for f in GEN.REALTIME_LAYOUT_FIELDS)
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "' + header + '"\nint main() {\n'
                   '  printf("%zu\\n", sizeof(WorldSynthesizer));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-I", include_dir, "-o", str(exe), str(src)], check=True)
    return np.array([int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()])


def test_synthesizer_layout_matches_the_reference(tmp_path):
    ours = _compile_layout(tmp_path, os.path.join(ROOT, "include"), "world/synthesisrealtime.h")
    assert np.array_equal(ours, FIX["layout"]), (ours, FIX["layout"])
    from world_amd.api import WorldSynthesizer
    assert C.sizeof(WorldSynthesizer) == FIX["layout"][0]
    for f, off in zip(GEN.REALTIME_LAYOUT_FIELDS, FIX["layout"][1:]):
        assert getattr(WorldSynthesizer, f).offset == off, f
    if os.path.isdir(os.path.join(REF, "src")):         # the live reference header, where it exists
        (tmp_path / "ref").mkdir()
        live = _compile_layout(tmp_path / "ref", os.path.join(REF, "src"), "world/synthesisrealtime.h")
        assert np.array_equal(ours, live)


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_realtime_header_compiles_alone(tmp_path, lang):
    src = tmp_path / ("caller.c" if lang == "c" else "caller.cpp")
    src.write_text('#include "world/synthesisrealtime.h"\n'
                   "int run(double *f0, double **sp, double **ap, int n) {\n"
                   "  WorldSynthesizer s = {0};\n"
                   "  InitializeSynthesizer(16000, 5.0, 1024, 64, 4, &s);\n"
                   "  int got = AddParameters(f0, n, sp, ap, &s);\n"
                   "  while (Synthesis2(&s) != 0) got += (int)(s.buffer[0] != 0.0);\n"
                   "  got += IsLocked(&s);\n"
                   "  RefreshSynthesizer(&s);\n"
                   "  DestroySynthesizer(&s);\n"
                   "  return got + s.head_pointer + s.randn_state.g_randn_x;\n"
                   "}\n")
    cc = "gcc" if lang == "c" else "g++"
    subprocess.run([cc, "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "c.o"),
                    str(src)], check=True)


@pytest.mark.parametrize("name", NAMES)
def test_emulated_realtime_reproduces_the_reference(emu, name):
    check_against_fixture(emu.realtime_plan(plan_of(name)), name, 1e-8)


def _batched_run(L, plans, fs, fft, bs, P):
    """world_hip_realtime_* on the emulated library (device memory is host memory there): every stream follows its own
    chunk plan, one synthesize() for all streams per round; returns each stream's concatenated output"""
    from world_amd.api import load_library
    L = load_library(L)
    ctx = L.world_hip_create(0, None)
    assert ctx
    h = C.c_void_p()
    assert L.world_hip_realtime_create(ctx, len(plans), fs, 5.0, fft, bs, P, C.byref(h)) == 0, L.world_hip_last_error()
    outs = [[] for _ in plans]
    pos = [0] * len(plans)
    k = [0] * len(plans)
    buf = np.zeros((len(plans), bs))
    produced = np.zeros(len(plans), dtype=np.int32)
    try:
        for _ in range(10000):
            busy = False
            for s, (f0, sp, ap, chunks) in enumerate(plans):
                if k[s] < len(chunks):
                    n = chunks[k[s]]
                    r = L.world_hip_realtime_add(h, s, f0[pos[s]:].ctypes.data_as(C.POINTER(C.c_double)), n,
                                                 C.c_void_p(sp[pos[s]:].ctypes.data), C.c_void_p(ap[pos[s]:].ctypes.data),
                                                 sp.shape[1])
                    assert r in (0, 1)
                    if r == 1:
                        pos[s] += n
                        k[s] += 1
                    busy = True
            while True:
                assert L.world_hip_realtime_synthesize(h, C.c_void_p(buf.ctypes.data),
                                                       produced.ctypes.data_as(C.POINTER(C.c_int))) == 0
                for s in range(len(plans)):
                    if produced[s]:
                        outs[s].append(buf[s].copy())
                if not produced.any():
                    break
            if not busy:
                break
    finally:
        L.world_hip_realtime_destroy(h)
        L.world_hip_destroy(ctx)
    return [np.concatenate(o) if o else np.zeros(0) for o in outs]


def _stream_plans(n, fs, fft, nf, seed):
    from util import synth_params
    rng = np.random.default_rng(seed)
    plans = []
    for s in range(n):
        f0, sp, ap = synth_params(fs, nf, fft, seed=s)
        chunks, left = [], nf
        while left > 0:
            c = int(min(left, rng.integers(1, 9)))
            chunks.append(c)
            left -= c
        plans.append((f0, np.ascontiguousarray(sp), np.ascontiguousarray(ap), chunks))
    return plans


def _lone_run(host, plan, fs, fft, bs, P):
    f0, sp, ap, chunks = plan
    rec = host.realtime_plan(dict(fs=fs, frame_period=5.0, fft_size=fft, buffer_size=bs, number_of_pointers=P, f0=f0,
                                  sp=sp, ap=ap, chunks=chunks))
    return rec["out"]


def test_emulated_batched_streams_match_lone_synthesizers(emu):
    fs, fft, bs, P = 16000, 1024, 64, 64
    plans = _stream_plans(5, fs, fft, 30, seed=11)
    got = _batched_run(os.path.join(EMU_DIR, "libworld_emu.so"), plans, fs, fft, bs, P)
    for s, plan in enumerate(plans):
        want = _lone_run(emu, plan, fs, fft, bs, P)
        assert want.size > 0 and np.array_equal(got[s], want), f"stream {s}"


def _sequential_states(tmp_path, positions):
    """randn_state after k randn() calls, k in positions, from a generator stepped one call at a time (no jump tables)"""
    src = tmp_path / "seq.c"
    src.write_text(
        "#include <stdio.h>\n#include <stdint.h>\n#include <stdlib.h>\n"
        "int main(int argc, char **argv) {\n"
        "  uint32_t x = 123456789u, y = 362436069u, z = 521288629u, w = 88675123u;\n"
        "  unsigned long long done = 0;\n"
        "  for (int a = 1; a < argc; ++a) {\n"
        "    unsigned long long want = strtoull(argv[a], 0, 10);\n"
        "    for (; done < want; ++done)\n"
        "      for (int k = 0; k < 12; ++k) { uint32_t t = x ^ (x << 11); x = y; y = z; z = w; w = (w ^ (w >> 19)) ^ (t ^ (t >> 8)); }\n"
        "    printf(\"%u %u %u %u\\n\", x, y, z, w);\n"
        "  }\n"
        "  return 0;\n}\n")
    exe = tmp_path / "seq"
    subprocess.run(["gcc", "-O2", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)] + [str(p) for p in positions], capture_output=True, text=True, check=True).stdout
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def test_pulse_noise_states_follow_the_sequential_generator(emu, tmp_path):
    """the scheduler's jump-ahead (one per pulse, by the previous pulse's draw count) lands where stepping lands,
    including positions past 2^24 draws"""
    from world_amd.api import load_library
    L = load_library(os.path.join(EMU_DIR, "libworld_emu.so"))
    rng = np.random.default_rng(3)
    sizes = list(rng.integers(1, 2049, size=40)) + [(1 << 24) - 5000, 12345, 7, (1 << 23) + 3]
    positions = list(np.cumsum(sizes))
    want = _sequential_states(tmp_path, positions)
    state = (C.c_uint32 * 4)(123456789, 362436069, 521288629, 88675123)
    for size, pos, w in zip(sizes, positions, want):
        nxt = (C.c_uint32 * 4)()
        L.world_hip_realtime_rng_jump(state, int(size), nxt)
        assert tuple(nxt) == w, f"after {pos} draws"
        state = nxt
    assert positions[-1] > (1 << 24)


def test_emulated_batches_beyond_the_render_budget(emu, monkeypatch):
    """streams that each add a whole utterance at once need more pulses than one render batch holds: the call renders
    as many batches as it takes, and every stream's output is still its lone synthesiser's"""
    monkeypatch.setenv("WORLD_HIP_REALTIME_BATCH_PULSES", "2")
    fs, fft, bs, P = 16000, 1024, 64, 4
    plans = [(f0, sp, ap, [20, len(f0) - 20]) for f0, sp, ap, _ in _stream_plans(5, fs, fft, 40, seed=4)]
    got = _batched_run(os.path.join(EMU_DIR, "libworld_emu.so"), plans, fs, fft, bs, P)
    monkeypatch.delenv("WORLD_HIP_REALTIME_BATCH_PULSES")
    for s, plan in enumerate(plans):
        want = _lone_run(emu, plan, fs, fft, bs, P)
        assert want.size > 0 and np.array_equal(got[s], want), f"stream {s}"


def test_emulated_one_pulse_at_a_time_equals_render_ahead(emu, monkeypatch):
    """a batch of one pulse renders no further than the next buffer needs: the same control and the same bits as rendering
    every settled pulse at once"""
    ahead = emu.realtime_plan(plan_of("all_at_once"))
    monkeypatch.setenv("WORLD_HIP_REALTIME_BATCH_PULSES", "1")
    single = emu.realtime_plan(plan_of("all_at_once"))
    assert np.array_equal(ahead["calls"], single["calls"]) and np.array_equal(ahead["out"], single["out"])
    check_against_fixture(single, "all_at_once", 1e-8)


def test_emulated_drop_in_synthesizer_across_shutdown_and_fork(emu, tmp_path):
    """world_hip_shutdown() in the middle of a stream leaves the synthesiser working; a child forked after the parent's
    calls builds a fresh synthesiser and gets the same output, and the parent goes on"""
    import sys
    out = str(tmp_path / "lc.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "realtime_lifecycle.py"),
                    os.path.join(EMU_DIR, "libworld_emu.so"), out, "fork"], check=True, timeout=600)
    r = np.load(out)
    assert int(r["shutdown_rc"]) == 0 and r["first"].size > 0
    assert np.array_equal(r["first"], r["second"])
    assert int(r["child"]) == 0, f"the forked child's synthesis: status {int(r['child'])}"
