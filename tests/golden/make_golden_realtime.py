"""Fixtures of the real-time synthesiser (reference src/synthesisrealtime.cpp): tests/golden/realtime.npz.

Run on a CPU machine where oracle/_ref/libworld.a exists (oracle/Makefile builds it from the unmodified reference):

    python tests/golden/make_golden_realtime.py [--asan]

The archive is linked whole into a throwaway shared object (-Wl,-Bsymbolic) and driven through ctypes by
world_amd.api.run_realtime_plan; the reference's sources are read only by the compiler that built the archive.  Inputs
come from tests/util.synth_params.  For every case the file holds the plan (chunk sizes, options) and what the plan
recorded: the return value of every AddParameters / Synthesis2 / IsLocked call with the scalar fields and randn_state
after it, every output buffer [0, buffer_size), the pulse indices of every added chunk and the ring arrays after every
add.  `layout` is sizeof(WorldSynthesizer) and the offsets of its fields (REALTIME_LAYOUT_FIELDS), compiled against the
reference's headers.

Every case is an input on which the reference is defined: pulse spacing at most fft_size (the noise buffer), and each
case was run once with --asan, which repeats the plans in a child process against the reference's real-time sources
built with -fsanitize=address (host code only): no report.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from util import synth_params  # noqa: E402
from world_amd.api import bind_realtime, run_realtime_plan  # noqa: E402

REF = os.environ.get("WORLD_REF", "/root/reference")
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libworld.a")
REALTIME_LAYOUT_FIELDS = ("fs", "frame_period", "buffer_size", "number_of_pointers", "fft_size", "buffer",
                          "current_pointer", "i", "dc_remover", "f0_length", "f0_origin", "spectrogram", "aperiodicity",
                          "current_pointer2", "head_pointer", "synthesized_sample", "handoff", "handoff_phase",
                          "handoff_f0", "last_location", "cumulative_frame", "current_frame", "interpolated_vuv",
                          "pulse_locations", "pulse_locations_index", "number_of_pulses", "impulse_response",
                          "randn_state", "minimum_phase", "inverse_real_fft", "forward_real_fft")


def cases():
    """name -> plan (see world_amd.api.run_realtime_plan)"""
    out = {}
    f0, sp, ap = synth_params(16000, 100, 1024, seed=0)
    base = dict(fs=16000, frame_period=5.0, fft_size=1024, buffer_size=64, f0=f0, sp=sp, ap=ap)
    # 1. test.cpp "Synthesis 2": every frame in one AddParameters, a ring of one
    out["all_at_once"] = dict(base, number_of_pointers=1, chunks=[100])
    # 2. test.cpp "Synthesis 3": one frame per AddParameters, a ring of 100, stop when locked
    out["frame_by_frame"] = dict(base, number_of_pointers=100, chunks=[1] * 100, stop_on_lock=True)
    # 3. 48 kHz, random chunk sizes 1..13, ring 8, drained only every tenth add (the ring fills: refused adds, retries);
    # single-frame chunks without a pulse and unvoiced stretches come with the contour
    f0, sp, ap = synth_params(48000, 90, 2048, seed=1)
    rng = np.random.default_rng(7)
    chunks, left = [], 90
    while left > 0:
        c = int(min(left, rng.integers(1, 14)))
        chunks.append(c)
        left -= c
    out["random_chunks_48k"] = dict(fs=48000, frame_period=5.0, fft_size=2048, buffer_size=256, number_of_pointers=8,
                                    f0=f0, sp=sp, ap=ap, chunks=chunks, drain_every=10)
    # 4. 22.05 kHz, 10 ms hop, a buffer that is not a power of two
    f0, sp, ap = synth_params(22050, 40, 1024, seed=2)
    out["hop10_22k"] = dict(fs=22050, frame_period=10.0, fft_size=1024, buffer_size=100, number_of_pointers=6,
                            f0=f0, sp=sp, ap=ap, chunks=[3, 1, 5, 2, 7, 4, 6, 1, 8, 3])
    # 5. 192 kHz, fft 8192, short
    f0, sp, ap = synth_params(192000, 10, 8192, seed=3)
    out["fs192k_fft8192"] = dict(fs=192000, frame_period=5.0, fft_size=8192, buffer_size=512, number_of_pointers=4,
                                 f0=f0, sp=sp, ap=ap, chunks=[2, 3, 1, 4])
    # 6. RefreshSynthesizer in mid-stream, then a second utterance
    fa, sa, aa = synth_params(16000, 40, 1024, seed=4)
    fb, sb, ab = synth_params(16000, 40, 1024, seed=5)
    out["refresh_midstream"] = dict(fs=16000, frame_period=5.0, fft_size=1024, buffer_size=80, number_of_pointers=5,
                                    f0=np.concatenate([fa[:25], fb]), sp=np.concatenate([sa[:25], sb]),
                                    ap=np.concatenate([aa[:25], ab]), chunks=[5] * 5 + [4] * 10, refresh_before=5)
    # 7., 8. fft_size off the rate's default (tests/test_gpu_offdefault_fft.py).  The real-time reference has no lowest_f0:
    # every non-zero frame is voiced, so the pulse spacing fs / f0 must itself stay within fft_size, and a voiced stretch
    # starts and ends at twice that or more (F0 is interpolated towards 0 at its boundaries).
    f0, sp, ap = (v[12:] for v in synth_params(16000, 32, 4096, seed=6))          # 15 voiced frames, 5 unvoiced
    out["fs16k_fft4096"] = dict(fs=16000, frame_period=5.0, fft_size=4096, buffer_size=96, number_of_pointers=4,
                                f0=f0, sp=sp, ap=ap, chunks=[4, 1, 7, 3, 5])
    # 48 kHz / 512: Synthesis' lowest_f0 would be 48000 / 512 + 1 = 94 Hz; frames at 93.9 and 93.8 Hz lie below it and
    # still space their pulses 512 samples apart (fs / fft_size = 93.75 Hz), frames at 96 Hz and up lie above
    _, sp, ap = synth_params(48000, 20, 512, seed=7)
    f0 = np.array([0.0, 0.0, 220.0, 180.0, 150.0, 110.0, 96.0, 93.9, 93.9, 96.0, 120.0, 93.8, 100.0, 160.0, 220.0, 0.0, 0.0,
                   200.0, 0.0, 0.0])
    ap = np.where((f0 == 0.0)[:, None], 1.0 - 1e-12, np.minimum(ap, 1.0 - 1e-6))
    out["fs48k_fft512"] = dict(fs=48000, frame_period=5.0, fft_size=512, buffer_size=200, number_of_pointers=5,
                               f0=f0, sp=sp, ap=ap, chunks=[2, 5, 1, 6, 3, 3])
    return out


def layout(tmp):
    """sizeof(WorldSynthesizer) and the offsets of its fields, from the reference's header"""
    src = os.path.join(tmp, "layout.cpp")
    with open(src, "w") as f:
        f.write('#include <cstdio>\n#include <cstddef>\n#include "world/synthesisrealtime.h"\nint main() {\n')
        f.write('  printf("%zu\\n", sizeof(WorldSynthesizer));\n')
        for name in REALTIME_LAYOUT_FIELDS:
            f.write(f'  printf("%zu\\n", offsetof(WorldSynthesizer, {name}));\n')
        f.write("  return 0;\n}\n")
    exe = os.path.join(tmp, "layout")
    subprocess.run(["g++", "-I", os.path.join(REF, "src"), "-o", exe, src], check=True)
    return np.array([int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()])


def reference_library(tmp, asan=False):
    so = os.path.join(tmp, "libref_rt_asan.so" if asan else "libref_rt.so")
    if asan:
        srcs = [os.path.join(REF, "src", u + ".cpp") for u in ("synthesisrealtime", "common", "fft", "matlabfunctions")]
        subprocess.run(["g++", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=address", "-I", os.path.join(REF, "src"),
                        "-o", so, *srcs, "-lm"], check=True)
    else:
        subprocess.run(["g++", "-shared", "-o", so, "-Wl,--whole-archive", ARCHIVE, "-Wl,--no-whole-archive",
                        "-Wl,-Bsymbolic", "-lm"], check=True)
    return so


def main():
    with tempfile.TemporaryDirectory() as tmp:
        if "--asan-child" in sys.argv:
            L = bind_realtime(C.CDLL(sys.argv[-1]))
            for name, plan in cases().items():
                run_realtime_plan(L, plan)
                print("asan:", name, "ok")
            return
        if "--asan" in sys.argv:
            so = reference_library(tmp, asan=True)
            libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
            preload = " ".join(v for v in (libasan, os.environ.get("LD_PRELOAD", "")) if v)   # in front of what is preloaded already
            env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--asan-child", so], env=env, check=True)
        L = bind_realtime(C.CDLL(reference_library(tmp)))
        arrays = {"layout": layout(tmp), "names": np.array(sorted(cases()))}
        for name, plan in cases().items():
            rec = run_realtime_plan(L, plan)
            for k in ("fs", "frame_period", "fft_size", "buffer_size", "number_of_pointers"):
                arrays[f"{name}.{k}"] = np.array(plan[k])
            arrays[f"{name}.chunks"] = np.array(plan["chunks"], dtype=np.int64)
            arrays[f"{name}.options"] = np.array([plan.get("drain_every", 1), plan.get("refresh_before", -1),
                                                  int(plan.get("stop_on_lock", False))], dtype=np.int64)
            for k, v in rec.items():
                arrays[f"{name}.{k}"] = v
            print(f"{name}: {len(rec['calls'])} calls, {len(rec['out'])} samples, {len(rec['pulses'])} pulses")
        np.savez_compressed(os.path.join(HERE, "realtime.npz"), **arrays)


if __name__ == "__main__":
    main()
