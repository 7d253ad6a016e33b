"""Time world_hip_align_batch on the GPU at the headline utterance's length: 12 pairs of 2001 x 2001 frames with 59
dimensions (60 mel-cepstral coefficients without c0), beside the time analyze_coded takes for the same 24 utterances --
the scale against which a user judges it.

    python tools/align_bench.py [--pairs 12] [--frames 2001] [--dims 59] [--repeats 10] [--no-analysis]

The whole call is timed with HIP events around it (warm-up first, then `repeats` runs: median, min, max); the three
kernels separately with the library's per-kernel events (WorldHip.profile), in runs of their own.  The diagonal step is
the DP kernel's time over its n_a + n_b - 1 diagonals.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    ms = sorted(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), runs=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--frames", type=int, default=2001)
    ap.add_argument("--dims", type=int, default=59)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-analysis", action="store_true")
    a = ap.parse_args()
    import torch
    from world_amd import synth
    from world_amd.api import WorldHip, frame_count
    if not torch.cuda.is_available():
        sys.exit("align_bench: no GPU")
    wh = WorldHip()
    P, F, D = a.pairs, a.frames, a.dims
    # two smooth random walks per pair: neighbouring frames resemble each other, as cepstra do
    g = torch.Generator(device="cpu").manual_seed(5)
    feats = torch.cumsum(0.1 * torch.randn((2, P, F, D), generator=g, dtype=torch.float64), dim=2).to(wh.device)
    n = np.full(P, F, dtype=np.int32)
    call = lambda: wh.align(feats[0], feats[1], n, n)

    def timed(fn, repeats):
        out = []
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            out.append(t0.elapsed_time(t1))
        return out

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    result = dict(pairs=P, frames=F, dims=D, align_call=spread(timed(call, a.repeats)))
    kernels = {}
    for _ in range(a.repeats):
        for name, ms in wh.profile(call).items():
            if name.startswith("align_"):
                kernels.setdefault(name, []).append(sum(ms))
    for name, ms in kernels.items():
        result[name] = spread(ms)
    if "align_dp" in result:
        result["diagonal_step_us"] = round(1e3 * result["align_dp"]["median_ms"] / (2 * F - 1), 4)
    result["workspace_mb"] = round(wh.workspace_bytes() / 1e6, 1)
    if not a.no_analysis:
        fs, seconds, dims = 48000, (F - 1) * 0.005, D + 1
        x = torch.stack([synth.vowel(fs, seconds, seed=40 + u) for u in range(2 * P)]).to(wh.device).contiguous()
        nf = frame_count(fs, x.shape[1], 5.0)
        block = torch.zeros((2 * P * nf, wh.lib.world_hip_coded_columns(fs, dims)), dtype=torch.float64, device=wh.device)
        analysis = lambda: wh.analyze_coded(x, fs, block, number_of_dimensions=dims)
        for _ in range(2):
            analysis()
        torch.cuda.synchronize()
        result["analyze_coded_same_utterances"] = spread(timed(analysis, max(3, a.repeats // 2)))
        result["analysis_frames_per_utterance"] = nf
    print(json.dumps(result))


if __name__ == "__main__":
    main()
