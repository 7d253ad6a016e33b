"""Time world_hip_resample_batch on the GPU: 12 utterances of 10 s, (a) 44.1 -> 48 kHz and (b) 48 -> 16 kHz with the BEST
design, (c) the same two with FAST -- beside world_hip_analyze_batch of the resampled batch in the same process, which is
what the conversion stands in front of.

    python tools/resample_bench.py [--utterances 12] [--seconds 10] [--repeats 10] [--warmup 3] [--no-analysis]

Every call is timed with HIP events around it (warm-up first, then `repeats` runs: median, min, max); the kernel separately
with the library's per-kernel events (WorldHip.profile), in runs of their own.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("a_44100_48000_best", 44100, 48000, "best"), ("b_48000_16000_best", 48000, 16000, "best"),
         ("c_44100_48000_fast", 44100, 48000, "fast"), ("c_48000_16000_fast", 48000, 16000, "fast")]


def spread(ms):
    ms = sorted(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), runs=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=12)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-analysis", action="store_true", help="time the conversion alone")
    a = ap.parse_args()
    import torch
    from world_amd import synth
    from world_amd.api import WorldHip, resample_length
    if not torch.cuda.is_available():
        sys.exit("resample_bench: no GPU")
    wh = WorldHip()

    def timed(fn, repeats):
        out = []
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            out.append(t0.elapsed_time(t1))
        return out

    result = dict(utterances=a.utterances, seconds=a.seconds)
    analysed = {}
    for label, fs_in, fs_out, quality in CASES:
        n_in = int(a.seconds * fs_in)
        x = torch.stack([synth.utterance(u, fs_in, a.seconds)[:n_in] for u in range(a.utterances)]).to(wh.device).contiguous()
        n_out = resample_length(n_in, fs_in, fs_out)
        y = torch.zeros((a.utterances, n_out), dtype=torch.float64, device=wh.device)
        call = lambda: wh.resample(x, fs_in, fs_out, quality=quality, out=y)
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        entry = dict(outputs=a.utterances * n_out, call=spread(timed(call, a.repeats)))
        kernels = {}
        for _ in range(a.repeats):
            for name, ms in wh.profile(call).items():
                if name.startswith("resample_"):
                    kernels.setdefault(name, []).append(sum(ms))
        for name, ms in kernels.items():
            entry[name] = spread(ms)
        if not a.no_analysis:
            if fs_out not in analysed:                           # the analysis the conversion feeds, on its own output
                analyze = lambda: wh.analyze(y, fs_out)
                for _ in range(a.warmup):
                    analyze()
                torch.cuda.synchronize()
                analysed[fs_out] = spread(timed(analyze, a.repeats))
            entry["analyze_of_output"] = analysed[fs_out]
            entry["call_over_analysis"] = round(entry["call"]["median_ms"] / analysed[fs_out]["median_ms"], 4)
        result[label] = entry
        del x, y
    result["workspace_mb"] = round(wh.workspace_bytes() / 1e6, 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
