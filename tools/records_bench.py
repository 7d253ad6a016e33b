"""Synthesis from records beside the routes a caller had before (include/world_hip.h: world_hip_synthesis_records), timed
with HIP events on one GPU, in alternating rounds of one process.

    python tools/records_bench.py [--batch 12] [--seconds 10] [--fs 48000] [--dims 60] [--reps 5] [--rounds 5]

Default shape: 12 utterances of 10 s at 48 kHz, 60 coefficients.  The records come from world_hip_analyze_coded and
world_hip_analyze_packed of synthetic utterances.  Prints one JSON line of medians (ms):
  a  world_hip_decode_spectral_envelope + world_hip_decode_aperiodicity (on the coded columns, made contiguous outside the
     timed region) + world_hip_synthesis_batch
  b  world_hip_synthesis_records, wire 2
  c0 world_hip_unpack_results + world_hip_synthesis_batch      c  world_hip_synthesis_records, wire 0
a_spread / c0_spread are (max - min) / median of the yardstick's per-round medians: what a difference has to exceed to
mean anything.  staging_bytes is what wire 2 holds in the workspace; upload_bytes what a caller has to bring to the device
per route.  The uploads themselves are not timed."""
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
    ap.add_argument("--dims", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from world_amd import synth
    from world_amd.api import WorldHip, cheaptrick_fft_size, frame_count
    wh = WorldHip()
    L, ctx, fs, D = wh.lib, wh._context(), a.fs, a.dims
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))
    x = torch.stack([synth.utterance(i, fs, a.seconds) for i in range(a.batch)]).cuda().contiguous()
    B = x.shape[0]
    fft = cheaptrick_fft_size(fs, 71.0)
    nb = fft // 2 + 1
    ccols, pcols = L.world_hip_coded_columns(fs, D), L.world_hip_record_columns(fft, 0)
    nap = ccols - 2 - D
    f64 = dict(dtype=torch.float64, device=x.device)
    nf = np.full(B, frame_count(fs, x.shape[1], 5.0), dtype=np.int32)
    rows, F = int(nf.sum()), int(nf.max())
    coded = torch.empty((rows, ccols), **f64)
    packed = torch.empty((rows, pcols), **f64)
    wh.analyze_coded(x, fs, coded, number_of_dimensions=D)
    wh.analyze_packed(x, fs, packed)
    yl = np.array([int((int(n) - 1) * 5.0 / 1000.0 * fs) + 1 for n in nf], dtype=np.int32)
    Y = int(yl.max())
    y = torch.empty((B, Y), **f64)
    # (a)'s inputs: the coded columns as the dense [B][F][...] arrays the decode calls and synthesis_batch take
    mcep, bap, f0 = torch.zeros((B, F, D), **f64), torch.full((B, F, nap), -1.0, **f64), torch.zeros((B, F), **f64)
    at = 0
    for u, n in enumerate(nf):
        mcep[u, :n], bap[u, :n], f0[u, :n] = coded[at:at + n, 2:2 + D], coded[at:at + n, 2 + D:], coded[at:at + n, 1]
        at += int(n)
    sp, aper, tpos = torch.empty((B, F, nb), **f64), torch.empty((B, F, nb), **f64), torch.empty((B, F), **f64)
    ok = lambda rc: wh._check(rc, "records_bench")

    def route_a():
        ok(L.world_hip_decode_spectral_envelope(ctx, B * F, fs, fft, D, mcep.data_ptr(), sp.data_ptr()))
        ok(L.world_hip_decode_aperiodicity(ctx, B * F, fs, fft, bap.data_ptr(), aper.data_ptr()))
        ok(L.world_hip_synthesis_batch(ctx, B, fs, 5.0, fft, ip(nf), F, f0.data_ptr(), sp.data_ptr(), aper.data_ptr(), ip(yl), Y,
                                       y.data_ptr()))

    def route_b():
        ok(L.world_hip_synthesis_records(ctx, B, fs, 5.0, fft, ip(nf), 0, coded.data_ptr(), ccols, 2, D, ip(yl), Y, y.data_ptr()))

    def route_c0():
        ok(L.world_hip_unpack_results(ctx, B, ip(nf), F, nb, packed.data_ptr(), 0, tpos.data_ptr(), f0.data_ptr(), sp.data_ptr(),
                                      aper.data_ptr()))
        ok(L.world_hip_synthesis_batch(ctx, B, fs, 5.0, fft, ip(nf), F, f0.data_ptr(), sp.data_ptr(), aper.data_ptr(), ip(yl), Y,
                                       y.data_ptr()))

    def route_c():
        ok(L.world_hip_synthesis_records(ctx, B, fs, 5.0, fft, ip(nf), 0, packed.data_ptr(), pcols, 0, 0, ip(yl), Y, y.data_ptr()))

    routes = dict(a=route_a, b=route_b, c0=route_c0, c=route_c)
    held = {}
    for name, fn in routes.items():                                        # warm-up; the workspace each route settles at
        fn(); fn()
        torch.cuda.synchronize()
        assert wh.synthesis_pulses_dropped() == 0
        held[name] = int(L.world_hip_workspace_bytes(ctx))

    def timed(fn):
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))
    per_round = {k: [] for k in routes}
    for _ in range(a.rounds):
        for name, fn in routes.items():
            per_round[name].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in per_round.items()}
    spread = lambda k: (max(per_round[k]) - min(per_round[k])) / med[k]
    out = dict(tool="records_bench", batch=B, seconds=a.seconds, fs=fs, dims=D, frames=rows,
               **{k + "_ms": round(v, 4) for k, v in med.items()}, a_spread=round(spread("a"), 4), c0_spread=round(spread("c0"), 4),
               b_over_a=round(med["b"] / med["a"], 4), c_over_c0=round(med["c"] / med["c0"], 4),
               staging_bytes=rows * (8 + 16 * nb), workspace_bytes=held,
               upload_bytes=dict(dense=rows * (8 + 16 * nb), f64_records=rows * pcols * 8, f32_records=rows * (2 + nb) * 8,
                                 coded_records=rows * ccols * 8))
    print(json.dumps(out))
    wh.close()


if __name__ == "__main__":
    main()
