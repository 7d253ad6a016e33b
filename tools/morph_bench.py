"""Time world_hip_morph_batch on the GPU at the headline utterance's length: 12 pairs of 2001 x 2001 frames at 48 kHz
(1025 bins per row), paths from world_hip_align_batch on random walks, every rate 0.5 (both sides blended, every bin
through log / exp: the most work the call can have) -- beside world_hip_modify_frames_batch on the same number of output
rows in the same process (a fractional time map and a formant ratio per frame, so that its rows go through the warp).

    python tools/morph_bench.py [--pairs 12] [--frames 2001] [--fs 48000] [--repeats 10] [--rate 0.5]

The whole call is timed with HIP events around it (warm-up first, then `repeats` runs: median, min, max); the kernels
separately with the library's per-kernel events (WorldHip.profile), in runs of their own.  One JSON line at the end."""
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
    ap.add_argument("--fs", type=int, default=48000)
    ap.add_argument("--rate", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from world_amd.api import WorldHip, cheaptrick_fft_size
    if not torch.cuda.is_available():
        sys.exit("morph_bench: no GPU")
    wh = WorldHip()
    P, F, fs = a.pairs, a.frames, a.fs
    fft = cheaptrick_fft_size(fs, 71.0)
    nb = fft // 2 + 1
    g = torch.Generator(device="cpu").manual_seed(7)
    feats = torch.cumsum(0.1 * torch.randn((2, P, F, 24), generator=g, dtype=torch.float64), dim=2).to(wh.device)
    n = np.full(P, F, dtype=np.int32)
    path, path_len, _, _, _ = wh.align(feats[0], feats[1], n, n)
    del feats
    dg = torch.Generator(device=wh.device).manual_seed(8)
    rows = lambda lo, hi: torch.rand((P, F, nb), generator=dg, dtype=torch.float64, device=wh.device) * (hi - lo) + lo
    sides = []
    for _ in range(2):
        f0 = torch.rand((P, F), generator=dg, dtype=torch.float64, device=wh.device) * 300.0 + 80.0
        f0[:, ::7] = 0.0
        sides.append((f0, rows(1e-6, 1e-2), rows(0.001, 0.999)))
    n_out = wh.morph_length(F, F, a.rate)
    outs = tuple(torch.zeros((P, n_out) + tuple(x.shape[2:]), dtype=torch.float64, device=wh.device) for x in sides[0])
    call = lambda: wh.morph(sides[0], sides[1], n, n, fs, fft, path, path_len, rate=a.rate, out=outs)
    time_map = (torch.arange(n_out, dtype=torch.float64, device=wh.device) * ((F - 1) / max(n_out - 1, 1))).clamp_(0.0, F - 1.0)
    shift = 1.0 + 0.2 * torch.sin(torch.arange(n_out, dtype=torch.float64, device=wh.device) / 50.0)
    modify = lambda: wh.modify_frames(*sides[0], n, fs, fft, n_out=n_out, time_map=time_map, formant_shift=shift, validate=False, out=outs)

    def timed(fn, repeats):
        out = []
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            out.append(t0.elapsed_time(t1))
        return out

    result = dict(pairs=P, frames=F, fs=fs, fft_size=fft, rate=a.rate, output_rows=P * n_out,
                  path_cells=[int(path_len.min()), int(path_len.max())])
    for label, fn, prefix in (("morph_call", call, "morph_"), ("modify_frames_call", modify, "modify_frames_")):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        result[label] = spread(timed(fn, a.repeats))
        kernels = {}
        for _ in range(a.repeats):
            for name, ms in wh.profile(fn).items():
                if name.startswith(prefix):
                    kernels.setdefault(name, []).append(sum(ms))
        for name, ms in kernels.items():
            result[name] = spread(ms)
    for name in ("morph_frames_sp", "morph_frames_ap", "modify_frames_sp", "modify_frames_ap"):
        if name in result:
            result[name + "_ns_per_row"] = round(1e6 * result[name]["median_ms"] / (P * n_out), 3)
    result["workspace_mb"] = round(wh.workspace_bytes() / 1e6, 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
