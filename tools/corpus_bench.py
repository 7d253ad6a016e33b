#!/usr/bin/env python
"""Time the assembly of voice-conversion training rows on the GPU at a corpus shape: 200 pairs of 600-frame utterances,
D = 50 statics, so [static, delta] rows of 100 and joint rows of 200 doubles.
  per_pair_loop   what vc-train did before the corpus stage: per pair two deltas calls, one world_hip_align_batch call,
                  a host read of the path length, torch indexing and torch.cat (restated here)
  batched         tools.vc_joint_rows: one deltas call a speaker, ONE align call, one host read, one joint_rows call
  kernels         each corpus kernel through WorldHip.profile -- frame_power (+ frame_power_mean), select_frames, joint_rows
                  as gather_rows and as joint_rows -- in milliseconds and effective GB/s (bytes read + bytes written)
  index_select    torch.index_select (+ torch.cat for the joint rows) on the same tensors and indices, HIP events

    python tools/corpus_bench.py [--pairs 200] [--frames 600] [--dim 50] [--fft-size 1024] [--repeats 5] [--warmup 2]

The loop and the batched path are timed by the wall clock around a device synchronisation (both read path lengths back).
One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    ms = sorted(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), runs=len(ms))


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--pairs", type=int, default=200)
    ap_.add_argument("--frames", type=int, default=600)
    ap_.add_argument("--dim", type=int, default=50)
    ap_.add_argument("--fft-size", type=int, default=1024)
    ap_.add_argument("--repeats", type=int, default=5)
    ap_.add_argument("--warmup", type=int, default=2)
    a = ap_.parse_args()
    import torch
    from world_amd import tools
    from world_amd.api import WorldHip
    if not torch.cuda.is_available():
        sys.exit("corpus_bench: no GPU")
    wh = WorldHip()
    P, T, D, bins = a.pairs, a.frames, a.dim, a.fft_size // 2 + 1
    rng = np.random.default_rng(1)
    # two "speakers": a random walk and a time-warped, perturbed copy of it, lengths within 10 % of --frames
    src, tgt = [], []
    for u in range(P):
        na, nb = (int(T * f) for f in rng.uniform(0.9, 1.0, 2))
        walk = np.cumsum(rng.standard_normal((T, D)), axis=0) * 0.1
        src.append(torch.from_numpy(walk[np.linspace(0, T - 1, na).astype(int)] + 0.01 * rng.standard_normal((na, D))).to(wh.device))
        tgt.append(torch.from_numpy(1.1 * walk[np.linspace(0, T - 1, nb).astype(int)] + 0.01 * rng.standard_normal((nb, D))).to(wh.device))

    def per_pair_loop():
        rows = []
        for s, t in zip(src, tgt):
            xa, xb = wh.deltas(s, windows=tools.VC_WINDOWS), wh.deltas(t, windows=tools.VC_WINDOWS)
            path, path_len, _, _, _ = wh.align(s[None, :, 1:], t[None, :, 1:], [len(s)], [len(t)])
            steps = path[0, :int(path_len[0])].long()
            rows.append(torch.cat([xa[steps[:, 0]], xb[steps[:, 1]]], dim=1))
        return torch.cat(rows)

    def batched():
        return tools.vc_joint_rows(wh, tools.vc_speaker(wh, src), tools.vc_speaker(wh, tgt))[0]

    def wall(fn, repeats):
        ms = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, ms

    wall(batched, a.warmup)
    z_batched, t_batched = wall(batched, a.repeats)
    wall(per_pair_loop, 1)
    z_loop, t_loop = wall(per_pair_loop, max(2, a.repeats // 2))
    same = z_loop.shape == z_batched.shape and bool((z_loop.view(torch.int64) == z_batched.view(torch.int64)).all())
    result = dict(pairs=P, frames=T, dim=D, joint_width=4 * D, rows=int(z_batched.shape[0]), fft_size=a.fft_size,
                  batched_equals_loop=same, per_pair_loop=spread(t_loop), batched=spread(t_batched))
    result["speedup"] = round(result["per_pair_loop"]["median_ms"] / result["batched"]["median_ms"], 2)

    # the kernels by themselves, and torch's gather on the same tensors
    a_side, b_side = tools.vc_speaker(wh, src), tools.vc_speaker(wh, tgt)
    (sa, xa, na), (sb, xb, nb) = a_side, b_side
    path, path_len, _, _, _ = wh.align(sa[:, :, 1:], sb[:, :, 1:], na, nb)
    K = path_len.cpu().numpy()
    rows = int(K.sum())
    z = torch.empty((rows, 4 * D), dtype=torch.float64, device=wh.device)
    sp = torch.rand((P, T, bins), dtype=torch.float64, device=wh.device) + 1e-3
    power, mean = wh.frame_power(sp, na)
    index, count, keep = wh.select_frames(power, na, 1.0, scale=mean)
    k = count.cpu().numpy()
    kept = torch.empty((P, int(k.max()), D - 1), dtype=torch.float64, device=wh.device)
    F = xa.shape[1]
    steps = torch.cat([path[u, :K[u]].long() + torch.tensor([u * F, u * xb.shape[1]], device=wh.device) for u in range(P)])
    ia, ib = steps[:, 0].contiguous(), steps[:, 1].contiguous()
    flat_a, flat_b = xa.reshape(-1, 2 * D), xb.reshape(-1, 2 * D)
    flat_s = sa.reshape(-1, D)[:, 1:]
    ik = torch.cat([index[u, :k[u]].long() + u * F for u in range(P)])
    calls = {
        "frame_power": (lambda: wh.frame_power(sp, na), int(na.sum()) * bins * 8 + int(na.sum()) * 8, ("frame_power", "frame_power_mean")),
        "select_frames": (lambda: wh.select_frames(power, na, 1.0, scale=mean), int(na.sum()) * (8 + 4 + 1), ("select_frames",)),
        "gather_rows": (lambda: wh.gather_rows(sa[:, :, 1:], index, k, n_src=na, out=kept), int(k.sum()) * (D - 1) * 16 + int(k.sum()) * 4, ("joint_rows",)),
        "joint_rows": (lambda: wh.joint_rows(xa, xb, path, K, n_a=na, n_b=nb, out=z), rows * 4 * D * 16 + rows * 8, ("joint_rows",)),
    }
    for name, (fn, nbytes, labels) in calls.items():
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            prof = wh.profile(fn)
            ms.append(sum(sum(v) for label, v in prof.items() if label in labels))
        result[name] = spread(ms)
        result[name]["GB_per_s"] = round(nbytes / (result[name]["median_ms"] * 1e-3) / 1e9, 1)
    torch_calls = {
        "torch_index_select_gather": (lambda: flat_s.index_select(0, ik), int(k.sum()) * (D - 1) * 16 + int(k.sum()) * 8),
        "torch_index_select_joint": (lambda: torch.cat([flat_a.index_select(0, ia), flat_b.index_select(0, ib)], dim=1), rows * 4 * D * 16 + rows * 16),
    }
    for name, (fn, nbytes) in torch_calls.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        result[name] = spread(ms)
        result[name]["GB_per_s"] = round(nbytes / (result[name]["median_ms"] * 1e-3) / 1e9, 1)
    got = torch.cat([flat_a.index_select(0, ia), flat_b.index_select(0, ib)], dim=1)
    wh.joint_rows(xa, xb, path, K, n_a=na, n_b=nb, out=z)
    result["joint_rows_equals_index_select"] = bool((got.view(torch.int64) == z.view(torch.int64)).all())
    for name in ("per_pair_loop", "batched", *calls, *torch_calls):
        r = result[name]
        rate = f"  {r['GB_per_s']:8.1f} GB/s" if "GB_per_s" in r else ""
        print(f"{name:28s} median {r['median_ms']:10.4f} ms  (min {r['min_ms']:.4f}, max {r['max_ms']:.4f}){rate}")
    print(f"batched / loop: {result['speedup']} x; the same bits: {same}; joint_rows equals index_select: {result['joint_rows_equals_index_select']}")
    print(json.dumps(result))
    wh.close()


if __name__ == "__main__":
    main()
