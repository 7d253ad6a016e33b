"""Cost of the parameter modification next to the analysis (include/world_hip.h: world_hip_modify_batch,
world_hip_resynthesize_batch), timed with HIP events on one GPU.

    python tools/transform_bench.py [--batch 12] [--seconds 10] [--fs 48000] [--reps 10]

Default shape: BASELINE.json configs[1], 12 utterances of 10 s at 48 kHz.  Prints one JSON line:
  analyze_ms, modify_ms (F0 scale + formant shift of every frame, out of place), synthesis_ms, resynthesize_ms (the one call),
  modify_share = modify / analyze, overhead = resynthesize / (analyze + modify + synthesis) - 1.
Every figure is the median of --reps timed repetitions after two warm-up calls of the same shape.

    python tools/transform_bench.py --frames [--rounds 5] [--only c]

times the frame-wise route (world_hip_modify_frames_batch) beside the per-utterance one on the same analysis, in
alternating rounds of one process: (a) modify_batch with constant ratios, (b) modify_frames_batch with the same constants
as curves behind an identity map, (c) a 1.5 x uniform time map with ratios that vary per frame (c_with_ap: the
aperiodicity rows retimed as well).  a_spread is (max - min) / median of (a)'s per-round medians: what a difference
between (a) and (b) has to exceed to mean anything.  --only runs one of them alone (for a kernel trace)."""
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
    ap.add_argument("--frames", action="store_true", help="time modify_frames_batch beside modify_batch")
    ap.add_argument("--rounds", type=int, default=5, help="--frames: alternating rounds")
    ap.add_argument("--only", choices=("a", "b", "c", "c_with_ap"), default=None, help="--frames: run this one alone")
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

    if a.frames:
        analyze()
        O = int((F - 1) * 1.5) + 1
        dev = x.device
        ident = torch.arange(F, dtype=torch.float64, device=dev).repeat(B, 1)      # ([B, O] curves: the wrapper copies nothing)
        const = lambda v: torch.full((B, F), v, dtype=torch.float64, device=dev)
        gen = torch.Generator(device="cpu").manual_seed(1)
        vary = lambda lo, hi: (lo + (hi - lo) * torch.rand((B, O), dtype=torch.float64, generator=gen)).to(dev)
        stretch = (torch.arange(O, dtype=torch.float64, device=dev) * ((F - 1) / (O - 1))).repeat(B, 1)
        b_curves = dict(time_map=ident, f0_scale=const(1.5), formant_shift=const(1.2))
        c_curves = dict(time_map=stretch, f0_scale=vary(0.8, 1.6), formant_shift=vary(0.8, 1.3))
        c_gain = vary(0.8, 1.2)
        b_out = (torch.empty_like(f0), torch.empty_like(sp), None)
        c_out = (torch.empty((B, O), dtype=torch.float64, device=dev), torch.empty((B, O, sp.shape[2]), dtype=torch.float64, device=dev))
        c_ap = torch.empty_like(c_out[1])
        runs = {"a": modify,
                "b": lambda: wh.modify_frames(f0, sp, None, nf, fs, fft, out=b_out, validate=False, **b_curves),
                "c": lambda: wh.modify_frames(f0, sp, None, nf, fs, fft, out=(*c_out, None), validate=False, **c_curves),
                "c_with_ap": lambda: wh.modify_frames(f0, sp, aper, nf, fs, fft, out=(*c_out, c_ap), validate=False,
                                                      ap_gain=c_gain, **c_curves)}
        if a.only:
            runs = {a.only: runs[a.only]}
        per_round = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                per_round[k].append(timed(fn))
        row = 8 * (fft // 2 + 1)
        out = {"shape": f"{B} x {a.seconds:g} s at {fs} Hz", "frames": int(nf.sum()), "out_frames_c": B * O,
               "sp_bytes_a_b": 2 * int(nf.sum()) * row, "sp_bytes_c": 3 * B * O * row}
        for k, v in per_round.items():
            out[k + "_ms"] = round(float(np.median(v)), 4)
            out[k + "_rounds"] = [round(t, 4) for t in v]
        if "a" in per_round:
            out["a_spread"] = round((max(per_round["a"]) - min(per_round["a"])) / float(np.median(per_round["a"])), 4)
        print(json.dumps(out))
        return
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
