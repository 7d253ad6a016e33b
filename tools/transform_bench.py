"""Cost of the parameter modification next to the analysis (include/world_hip.h: world_hip_modify_batch,
world_hip_resynthesize_batch), timed with HIP events on one GPU.

    python tools/transform_bench.py [--batch 12] [--seconds 10] [--fs 48000] [--reps 10]

Default shape: BASELINE.json configs[1], 12 utterances of 10 s at 48 kHz.  Prints one JSON line:
  analyze_ms, modify_ms (F0 scale + formant shift of every frame, out of place), synthesis_ms, resynthesize_ms (the one call),
  modify_share = modify / analyze, overhead = resynthesize / (analyze + modify + synthesis) - 1.
Every figure is the median of --reps timed repetitions after two warm-up calls of the same shape."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--fs", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    from world_amd import synth
    from world_amd.api import (CheapTrickOption, D4COption, HarvestOption, WorldHip, cheaptrick_fft_size, frame_count,
                               modifications)
    wh = WorldHip()
    fs = a.fs
    x = torch.stack([synth.utterance(i, fs, a.seconds) for i in range(a.batch)]).cuda().contiguous()
    B, L = x.shape
    xl = np.full(B, L, dtype=np.int32)
    fft = cheaptrick_fft_size(fs, 71.0)
    nf = np.full(B, frame_count(fs, L, 5.0), dtype=np.int32)
    F = int(nf[0])
    tpos = torch.empty((B, F), dtype=torch.float64, device=x.device)
    f0 = torch.empty_like(tpos)
    sp = torch.empty((B, F, fft // 2 + 1), dtype=torch.float64, device=x.device)
    aper = torch.empty_like(sp)
    yl = np.full(B, wh.resynthesis_length(fs, F, 5.0, 1.0), dtype=np.int32)
    y = torch.empty((B, int(yl[0])), dtype=torch.float64, device=x.device)
    mods = modifications(B, 1.5, 1.2)
    hopt, copt, dopt = HarvestOption(71.0, 800.0, 5.0), CheapTrickOption(-0.15, 71.0, fft), D4COption(0.85)
    ip = C.POINTER(C.c_int)

    def analyze():
        wh.analyze(x, fs, sp_out=sp, ap_out=aper, tpos_out=tpos, f0_out=f0)

    f0m, spm = torch.empty_like(f0), torch.empty_like(sp)

    def modify():
        wh.modify(f0, sp, nf, fs, fft, f0_scale=1.5, formant_shift=1.2, out=(f0m, spm))

    def synthesis():
        wh.synthesis(f0m, spm, aper, nf, fft, 5.0, fs, yl, check_pulses=False)

    def resynthesize():
        wh._check(wh.lib.world_hip_resynthesize_batch(wh._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(ip),
                                                      C.byref(hopt), C.byref(copt), C.byref(dopt), mods, 1.0,
                                                      yl.ctypes.data_as(ip), y.shape[1], y.data_ptr()), "resynthesize")

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        if wh.synthesis_pulses_dropped():
            raise RuntimeError("pulses dropped: the timed synthesis is not the whole synthesis")
        return float(np.median(ms))

    t_an = timed(analyze)
    t_mod = timed(modify)
    t_syn = timed(synthesis)
    t_re = timed(resynthesize)
    out = {"shape": f"{B} x {a.seconds:g} s at {fs} Hz", "frames": int(nf.sum()), "analyze_ms": round(t_an, 4),
           "modify_ms": round(t_mod, 4), "synthesis_ms": round(t_syn, 4), "resynthesize_ms": round(t_re, 4),
           "modify_share": round(t_mod / t_an, 5), "overhead": round(t_re / (t_an + t_mod + t_syn) - 1.0, 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
