#!/usr/bin/env python
"""Time world_hip_sp2mc and world_hip_mc2sp on the GPU beside the reference's coder on the same rows: 64 x 1000 envelope
rows at 48 kHz (fft_size 2048, 1025 bins), order 59 -- and world_hip_code_spectral_envelope /
world_hip_decode_spectral_envelope with 60 dimensions, which read and write the same bytes and emit the same 60 columns.

    python tools/mcep_bench.py [--rows 64000] [--fs 48000] [--order 59] [--repeats 15] [--warmup 3]

The four calls are timed interleaved (one of each per round) with HIP events around each, after a warm-up; medians, minima
and maxima are reported, the ratio of each direction to the coder's, the envelope bytes moved per second, and the first
call of each direction (host table build + upload + kernel) in milliseconds.  One JSON line at the end."""
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64000)
    ap.add_argument("--fs", type=int, default=48000)
    ap.add_argument("--order", type=int, default=59)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from world_amd.api import WorldHip, cheaptrick_fft_size
    if not torch.cuda.is_available():
        sys.exit("mcep_bench: no GPU")
    wh = WorldHip()
    fft_size = cheaptrick_fft_size(a.fs, 71.0)
    K, P = fft_size // 2 + 1, a.order + 1
    alpha = wh.mcep_alpha(a.fs)
    g = torch.Generator(device=wh.device).manual_seed(1)
    f = torch.arange(K, dtype=torch.float64, device=wh.device) / (K - 1)
    sp = torch.exp(-8.0 - 6.0 * f + 3.0 * torch.cos(7.0 * f) +
                   0.5 * torch.randn((a.rows, K), dtype=torch.float64, device=wh.device, generator=g)).contiguous()
    mc = torch.empty((a.rows, P), dtype=torch.float64, device=wh.device)
    back = torch.empty((a.rows, K), dtype=torch.float64, device=wh.device)

    def first(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 3)

    ctx, lib = wh._context(), wh.lib
    calls = {
        "sp2mc": lambda: wh._check(lib.world_hip_sp2mc(ctx, a.rows, fft_size, a.order, alpha, sp.data_ptr(), K, mc.data_ptr(), P), "sp2mc"),
        "mc2sp": lambda: wh._check(lib.world_hip_mc2sp(ctx, a.rows, fft_size, a.order, alpha, mc.data_ptr(), P, back.data_ptr(), K), "mc2sp"),
        "code_spectral_envelope": lambda: wh._check(lib.world_hip_code_spectral_envelope(
            ctx, a.rows, a.fs, fft_size, P, sp.data_ptr(), mc.data_ptr()), "code"),
        "decode_spectral_envelope": lambda: wh._check(lib.world_hip_decode_spectral_envelope(
            ctx, a.rows, a.fs, fft_size, P, mc.data_ptr(), back.data_ptr()), "decode"),
    }
    result = dict(rows=a.rows, fs=a.fs, fft_size=fft_size, order=a.order, alpha=alpha,
                  first_call_ms={name: first(calls[name]) for name in ("sp2mc", "mc2sp")})
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(a.repeats):
        # (each call's input is what the previous left in place: mc holds coefficients of one coder or the other, both
        # finite, and the time of a product does not depend on the values)
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
    envelope_bytes = 8.0 * a.rows * K
    for name, ms in times.items():
        result[name] = spread(ms)
        result[name]["envelope_GB_per_s"] = round(envelope_bytes / (result[name]["median_ms"] * 1e-3) / 1e9, 1)
    result["sp2mc_over_code"] = round(result["sp2mc"]["median_ms"] / result["code_spectral_envelope"]["median_ms"], 3)
    result["mc2sp_over_decode"] = round(result["mc2sp"]["median_ms"] / result["decode_spectral_envelope"]["median_ms"], 3)
    result["sp2mc_matrix_TFLOPs"] = round(2.0 * a.rows * K * P / (result["sp2mc"]["median_ms"] * 1e-3) / 1e12, 2)
    result["mc2sp_matrix_TFLOPs"] = round(2.0 * a.rows * K * P / (result["mc2sp"]["median_ms"] * 1e-3) / 1e12, 2)
    for name in ("sp2mc", "mc2sp", "code_spectral_envelope", "decode_spectral_envelope"):
        r = result[name]
        print(f"{name:26s} median {r['median_ms']:8.4f} ms  (min {r['min_ms']:.4f}, max {r['max_ms']:.4f})  "
              f"{r['envelope_GB_per_s']:7.1f} GB/s of envelope")
    print(f"sp2mc / code {result['sp2mc_over_code']}, mc2sp / decode {result['mc2sp_over_decode']}; first calls "
          f"{result['first_call_ms']} ms")
    print(json.dumps(result))
    wh.close()


if __name__ == "__main__":
    main()
