"""Real-time synthesis timings; prints one JSON line.

    python tools/realtime_bench.py [--seconds S] [--streams 1,16,256]

* test_cpp: the reference's own test program (oracle/_ref/test_ref: reference archive alone; test_hip: libworld_hip.so in
  front of it) on vaiueo2d.wav (rebuilt from tests/golden/vaiueo2d_harvest.npz): the msec it prints for "Synthesis 2"
  (every frame added at once) and "Synthesis 3" (one frame per AddParameters).  Absent when the programs were not built.
* streams: WorldHip.realtime at 48 kHz, fft 2048, one 5 ms frame per add, buffer 256, for each stream count N: every
  round adds one frame to every stream and calls synthesize() until no stream produces; `rtf` = N x seconds of audio
  produced per second of wall time, p50 / p99 = wall milliseconds of one synthesize() call (its result copied back).
"""
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
_sys.path.insert(0, _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "tests"))
import argparse
import json
import os
import re
import subprocess
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp():
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    exes = {"ref": os.path.join(ref_dir, "test_ref"), "hip": os.path.join(ref_dir, "test_hip")}
    if not all(os.path.exists(e) for e in exes.values()):
        return None
    g = np.load(os.path.join(ROOT, "tests", "golden", "vaiueo2d_harvest.npz"))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in.wav")
        with wave.open(src, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(g["fs"]))
            w.writeframes(g["q"].astype("<i2").tobytes())
        for tag, exe in exes.items():
            r = subprocess.run([exe, src, "out.wav"], cwd=tmp, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                res[tag] = {"error": r.returncode}
                continue
            out = {}
            for label, key in (("Synthesis 2", "synthesis2_ms"), ("Synthesis 3", "synthesis3_ms")):
                m = re.search(re.escape(label) + r"[^\n]*\n(?:[^\n]*\n)*?WORLD: (\d+) \[msec\]", r.stdout)
                out[key] = int(m.group(1)) if m else None
            res[tag] = out
    return res


def streams(n, seconds):
    import torch
    from util import synth_params
    from world_amd.api import WorldHip
    fs, fft, bs, fp = 48000, 2048, 256, 5.0
    nf = int(seconds * 1000 / fp) + 1
    f0, sp, ap = synth_params(fs, nf, fft, seed=1)
    wh = WorldHip(device=0)
    d_sp, d_ap = torch.from_numpy(sp).cuda(), torch.from_numpy(ap).cuda()
    rt = wh.realtime(n, fs, fp, fft, bs, 64)
    calls, produced_samples = [], 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(nf):
        for s in range(n):
            assert rt.add(s, f0[i:i + 1], d_sp[i:], d_ap[i:]) == 1
        while True:
            c0 = time.perf_counter()
            out, produced = rt.synthesize()
            torch.cuda.current_stream().synchronize()
            calls.append(time.perf_counter() - c0)
            produced_samples += int(produced.sum()) * bs
            if not produced.any():
                break
    wall = time.perf_counter() - t0
    rt.close()
    wh.close()
    ms = np.array(calls) * 1e3
    return {"n_streams": n, "audio_s_per_stream": produced_samples / n / fs, "wall_s": wall,
            "rtf": produced_samples / fs / wall, "synthesize_p50_ms": float(np.percentile(ms, 50)),
            "synthesize_p99_ms": float(np.percentile(ms, 99)), "calls": len(calls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--streams", default="1,16,256")
    a = ap.parse_args()
    line = {"metric": "realtime_synthesis", "test_cpp": test_cpp(),
            "streams_48k": [streams(int(n), a.seconds) for n in a.streams.split(",")]}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
