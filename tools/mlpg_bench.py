#!/usr/bin/env python
"""Time world_hip_mlpg_batch on the GPU beside what it feeds and beside the host: 64 utterances x 1000 frames x 60
mel-cepstra with the usual three windows -- per-frame variances and one global row -- the same for one utterance,
world_hip_delta_batch, then world_hip_mc2sp and world_hip_synthesis_batch on the very frames generated (48 kHz, fft_size
2048, 5 ms), and scipy.linalg.solveh_banded over the same systems on the host as the outside yardstick.

    python tools/mlpg_bench.py [--utts 64] [--frames 1000] [--dim 60] [--fs 48000] [--repeats 15] [--warmup 3]

The GPU calls are timed interleaved (one of each per round) with HIP events around each, after a warm-up; medians, minima
and maxima are reported.  One JSON line at the end."""
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


def host_solve(mean, prec, win):
    """the same systems by scipy.linalg.solveh_banded: mean, prec [T][n_win D] of one utterance -> (seconds, [T][D])"""
    from scipy.linalg import solveh_banded
    T, cols = mean.shape
    n_win, L = win.shape[0], win.shape[1] // 2
    D = cols // n_win
    t0 = time.perf_counter()
    ab, r = np.zeros((D, 2 * L + 1, T)), np.zeros((D, T))       # lower form: ab[d][k][i] = R[i + k][i]
    for w in range(n_win):
        p, pm = prec[:, w * D:(w + 1) * D].T, (prec[:, w * D:(w + 1) * D] * mean[:, w * D:(w + 1) * D]).T   # [D][T]
        for a in range(-L, L + 1):
            if win[w, a + L] == 0.0:
                continue
            lo, hi = max(0, -a), min(T, T - a)                   # observations t with 0 <= t + a < T
            r[:, lo + a:hi + a] += win[w, a + L] * pm[:, lo:hi]
            for b in range(a, L + 1):
                lo2, hi2 = max(lo, -b), min(hi, T - b)
                ab[:, b - a, lo2 + a:hi2 + a] += win[w, a + L] * win[w, b + L] * p[:, lo2:hi2]
    out = np.empty((T, D))
    for d in range(D):
        out[:, d] = solveh_banded(ab[d], r[d], lower=True)
    return time.perf_counter() - t0, out


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--utts", type=int, default=64)
    ap_.add_argument("--frames", type=int, default=1000)
    ap_.add_argument("--dim", type=int, default=60)
    ap_.add_argument("--fs", type=int, default=48000)
    ap_.add_argument("--repeats", type=int, default=15)
    ap_.add_argument("--warmup", type=int, default=3)
    a = ap_.parse_args()
    import torch
    from world_amd.api import WorldHip, cheaptrick_fft_size
    if not torch.cuda.is_available():
        sys.exit("mlpg_bench: no GPU")
    wh = WorldHip()
    U, T, D = a.utts, a.frames, a.dim
    win = np.array(WorldHip.DEFAULT_WINDOWS)
    n_win = len(win)
    fft_size = cheaptrick_fft_size(a.fs, 71.0)
    K, alpha, period = fft_size // 2 + 1, wh.mcep_alpha(a.fs), 5.0
    g = torch.Generator(device=wh.device).manual_seed(1)
    # cepstra of a plausible size (c0 about -8, the rest decaying), their dynamic features as the means, variances over a decade
    decay = 1.0 / (1.0 + torch.arange(D, dtype=torch.float64, device=wh.device))
    c = 0.3 * decay * torch.randn((U, T, D), dtype=torch.float64, device=wh.device, generator=g)
    c[:, :, 0] -= 8.0
    mean = wh.deltas(c)
    var_frame = 10.0 ** (torch.rand((U, T, n_win * D), dtype=torch.float64, device=wh.device, generator=g) - 0.5)
    var_global = var_frame[0, 0].clone()
    out = torch.empty((U, T, D), dtype=torch.float64, device=wh.device)
    dyn = torch.empty((U, T, n_win * D), dtype=torch.float64, device=wh.device)
    sp = torch.empty((U, T, K), dtype=torch.float64, device=wh.device)
    apd = torch.full((U, T, K), 0.1, dtype=torch.float64, device=wh.device)
    f0 = torch.full((U, T), 150.0, dtype=torch.float64, device=wh.device)
    nf = np.full(U, T, dtype=np.int32)
    y_length = np.full(U, int(T * period / 1000.0 * a.fs), dtype=np.int32)
    calls = {
        "mlpg_frame_var": lambda: wh.mlpg(mean, var_frame, out=out),
        "mlpg_global_var": lambda: wh.mlpg(mean, var_global, out=out),
        "mlpg_one_utt_frame_var": lambda: wh.mlpg(mean[:1], var_frame[:1], out=out[:1]),
        "mlpg_one_utt_global_var": lambda: wh.mlpg(mean[:1], var_global, out=out[:1]),
        "deltas": lambda: wh.deltas(c, out=dyn),
        "mc2sp": lambda: wh.mc2sp(out.view(U * T, D), alpha, fft_size, out=sp.view(U * T, K)),
        "synthesis": lambda: wh.synthesis(f0, sp, apd, nf, fft_size, period, a.fs, y_length, check_pulses=False),
        "synthesis_one_utt": lambda: wh.synthesis(f0[:1], sp[:1], apd[:1], nf[:1], fft_size, period, a.fs, y_length[:1], check_pulses=False),
    }
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    err = float((out - c).abs().max())
    times = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
    result = dict(utts=U, frames=T, dim=D, windows=win.tolist(), fs=a.fs, fft_size=fft_size, round_trip_max_error=err,
                  workspace_MB=round(wh.workspace_bytes() / 2 ** 20, 1))
    for name, ms in times.items():
        result[name] = spread(ms)
    # the host: utterance 0 solved by scipy (all of its D systems), scaled to the batch
    mean0 = mean[0].cpu().numpy()
    for name, v in (("frame_var", var_frame[0].cpu().numpy()), ("global_var", np.broadcast_to(var_global.cpu().numpy(), (T, n_win * D)))):
        runs = [host_solve(mean0, 1.0 / v, win) for _ in range(3)]
        sec = min(r[0] for r in runs)
        result["scipy_one_utt_" + name] = dict(ms=round(sec * 1e3, 2), batch_ms=round(sec * 1e3 * U, 1),
                                               max_diff_to_gpu=float(np.abs(runs[0][1] - (
                                                   wh.mlpg(mean[:1], var_frame[:1] if name == "frame_var" else var_global)[0].cpu().numpy())).max()))
    result["mlpg_over_synthesis"] = round(result["mlpg_frame_var"]["median_ms"] / result["synthesis"]["median_ms"], 4)
    result["mlpg_over_mc2sp"] = round(result["mlpg_frame_var"]["median_ms"] / result["mc2sp"]["median_ms"], 4)
    result["mlpg_us_per_frame_one_utt"] = round(result["mlpg_one_utt_frame_var"]["median_ms"] * 1e3 / T, 4)
    for name in calls:
        r = result[name]
        print(f"{name:26s} median {r['median_ms']:9.4f} ms  (min {r['min_ms']:.4f}, max {r['max_ms']:.4f})")
    for name in ("frame_var", "global_var"):
        r = result["scipy_one_utt_" + name]
        print(f"scipy solveh_banded, {name:10s}: one utterance {r['ms']} ms, {U} of them {r['batch_ms']} ms (|host - GPU| <= {r['max_diff_to_gpu']:.2e})")
    print(f"mlpg / synthesis {result['mlpg_over_synthesis']}, mlpg / mc2sp {result['mlpg_over_mc2sp']}, "
          f"{result['mlpg_us_per_frame_one_utt']} us per frame of one utterance; round trip error {err:.2e}")
    print(json.dumps(result))
    wh.close()


if __name__ == "__main__":
    main()
