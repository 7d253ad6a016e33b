#!/usr/bin/env python
"""Time the joint-density Gaussian mixture on the GPU at a corpus shape: world_hip_gmm_convert (10^5 rows, Dx = Dy = 50,
M = 64, both modes), the posterior alone, world_hip_gmm_accumulate and one EM iteration of world_hip_gmm_fit on the joint
rows (P = 100), beside world_hip_mc2sp on as many rows and, where sklearn imports, GaussianMixture's E-step and one EM
iteration on the box's CPUs.  The achieved FP64 rate (the useful operations of the rule: the triangle of U and of G counted
once) is set against what the box sustains (world_hip_probe_machine: bench.py's roofline.fp64.peak_measured).

    python tools/gmm_bench.py [--rows 100000] [--dx 50] [--dy 50] [--mix 64] [--repeats 7] [--warmup 2]

The GPU calls are timed with HIP events around each, after a warm-up; the fit by the wall clock (it waits for the device).
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
    ap_.add_argument("--rows", type=int, default=100000)
    ap_.add_argument("--dx", type=int, default=50)
    ap_.add_argument("--dy", type=int, default=50)
    ap_.add_argument("--mix", type=int, default=64)
    ap_.add_argument("--repeats", type=int, default=7)
    ap_.add_argument("--warmup", type=int, default=2)
    a = ap_.parse_args()
    import torch
    from world_amd.api import WorldHip
    if not torch.cuda.is_available():
        sys.exit("gmm_bench: no GPU")
    wh = WorldHip()
    rows, dx, dy, M = a.rows, a.dx, a.dy, a.mix
    P = dx + dy
    rng = np.random.default_rng(1)
    # rows of M well-populated clusters with a random linear relation between the source and the target part
    centres = 3.0 * rng.standard_normal((M, P))
    mixing = rng.standard_normal((P, P)) / np.sqrt(P) + np.eye(P)
    z_host = centres[rng.integers(0, M, rows)] + rng.standard_normal((rows, P)) @ mixing.T
    z = torch.from_numpy(z_host).to(wh.device)
    w0, mu0 = np.full(M, 1.0 / M), centres + 0.1 * rng.standard_normal((M, P))
    cov0 = np.stack([mixing @ mixing.T] * M)
    model = wh.gmm_prepare(w0, mu0, cov0, dx)
    joint = wh.gmm_prepare(w0, mu0, cov0, P)
    x = z[:, :dx]                                                    # (a view: the row stride is P)
    mean, var = (torch.empty((rows, dy), dtype=torch.float64, device=wh.device) for _ in range(2))
    post, _ = wh.gmm_posterior(joint, z)
    shift = torch.from_numpy(mu0).to(wh.device)
    N, S1, G = (torch.empty(s, dtype=torch.float64, device=wh.device) for s in ((M,), (M, P), (M, P, P)))
    fft_size, order = 1024, 49
    alpha = wh.mcep_alpha(16000)
    mc = 0.01 * torch.randn((rows, order + 1), dtype=torch.float64, device=wh.device)
    sp = torch.empty((rows, fft_size // 2 + 1), dtype=torch.float64, device=wh.device)

    def accumulate():
        wh._check(wh.lib.world_hip_gmm_accumulate(wh._context(), M, P, rows, z.data_ptr(), P, post.data_ptr(), M, shift.data_ptr(),
                                                  N.data_ptr(), S1.data_ptr(), G.data_ptr()), "gmm_accumulate")
    calls = {
        "convert_mixture": lambda: wh.gmm_convert(model, x, mode="mixture", out=(mean, var)),
        "convert_hard": lambda: wh.gmm_convert(model, x, mode="hard", out=(mean, var)),
        "posterior_joint": lambda: wh.gmm_posterior(joint, z),
        "accumulate_joint": accumulate,
        "mc2sp": lambda: wh.mc2sp(mc, alpha, fft_size, out=sp),
    }
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(a.repeats):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
    fit = []
    for _ in range(max(3, a.repeats // 2)):
        t0 = time.perf_counter()
        wh.gmm_fit(z, M, n_iter=1, reg=1e-6, init=(w0, mu0, cov0))
        fit.append((time.perf_counter() - t0) * 1e3)
    probe = wh.probe_machine() or {}
    peak = probe.get("fp64_fma_tflops")
    result = dict(rows=rows, dx=dx, dy=dy, mixtures=M, workspace_MB=round(wh.workspace_bytes() / 2 ** 20, 1), fp64_peak_measured_tflops=peak)
    flop = {"convert_mixture": rows * M * (dx * (dx + 1) + 2 * dx * dy), "convert_hard": rows * M * (dx * (dx + 1) + 2 * dx * dy),
            "posterior_joint": rows * M * P * (P + 1), "accumulate_joint": rows * M * (P + 1) * (P + 2)}
    for name, ms in times.items():
        result[name] = spread(ms)
        if name in flop:
            result[name]["tflops"] = round(flop[name] / (result[name]["median_ms"] * 1e-3) / 1e12, 3)
            if peak:
                result[name]["of_measured_peak"] = round(result[name]["tflops"] / peak, 4)
    result["em_iteration"] = spread(fit)
    result["em_iteration"]["of_which_device_ms"] = round(result["posterior_joint"]["median_ms"] + result["accumulate_joint"]["median_ms"], 4)
    try:
        from sklearn.mixture import GaussianMixture
        import warnings
        gm = GaussianMixture(n_components=M, covariance_type="full", reg_covar=1e-6, max_iter=1, tol=0, weights_init=w0, means_init=mu0,
                             precisions_init=np.linalg.inv(cov0))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter(); gm.fit(z_host); t_fit = time.perf_counter() - t0
            t0 = time.perf_counter(); gm.predict_proba(z_host); t_e = time.perf_counter() - t0
        result["sklearn_cpu"] = dict(em_iteration_ms=round(t_fit * 1e3, 1), e_step_ms=round(t_e * 1e3, 1), threads=os.cpu_count())
    except ImportError:
        result["sklearn_cpu"] = None
    for name in list(calls) + ["em_iteration"]:
        r = result[name]
        extra = f"  {r['tflops']:.2f} TFLOP/s FP64" + (f" = {100 * r['of_measured_peak']:.1f} % of {peak}" if peak else "") if "tflops" in r else ""
        print(f"{name:18s} median {r['median_ms']:10.4f} ms  (min {r['min_ms']:.4f}, max {r['max_ms']:.4f}){extra}")
    if result["sklearn_cpu"]:
        print(f"sklearn GaussianMixture on the CPUs: E-step {result['sklearn_cpu']['e_step_ms']} ms, one EM iteration {result['sklearn_cpu']['em_iteration_ms']} ms")
    print(json.dumps(result))
    wh.close()


if __name__ == "__main__":
    main()
