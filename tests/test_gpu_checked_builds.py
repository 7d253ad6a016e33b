"""The checked builds (world_amd/csrc/devrt.h: -DWH_JITTER, -DWH_LDS_POISON, -DWH_HBM_POISON; built by __graft_entry__.build()
into world_amd/variants/) must compute the SAME BITS as the product library.  The kernels alias LDS regions across phases and
place their barriers by hand; a missing barrier or a read of never-written LDS is invisible in normal runs (the wavefronts
of a workgroup arrive together; a fresh workgroup inherits plausible data) and used to be found by reading the code
(d4c_frame's select zeroed histograms other wavefronts were still reading).  With random multi-thousand-cycle
stalls behind every barrier and wave fence, or NaN patterns in every LDS byte a kernel did not write, such a bug changes
the result.

Two parts.  The five analysis workloads of round 6 (test_jitter_build_is_bit_identical, test_lds_poison_build_is_bit_identical)
stay as they were.  FAMILIES below runs every other kernel family of world_amd/csrc the same way, one parametrised case per
family so that a failure names it: product twice (a family that is not deterministic cannot be judged), jitter three times,
poison once, and once under WorldHip.profile to require that the kernels the family claims were launched.  The claims are
the coverage table: test_every_kernel_is_claimed_by_a_family (no GPU) reads the kernel sources and fails for a __global__
function that neither a family nor EXEMPT names, so a new kernel cannot ship without running under both builds.

Global memory gets the same treatment (-DWH_HBM_POISON: every carve of the arena and every reused device buffer refilled with
0xFF bytes -- NaN as a double, -1 as an int -- before the call writes it).  A fresh context hides a missing initialisation
(fresh pages are zero) and a reused one hides a read past what was written (the leftovers are the same call's, hence
correct), so: the five workloads in one hbm context (test_hbm_poison_build_is_bit_identical); a fourth leg of every
family, two hbm passes in one context, the second over the first's real leftovers; every family with a plain context in
ONE context, forwards and backwards, on the product and on the hbm library (test_families_share_one_context); and a family
over the drop-in symbols at shrinking and growing lengths (dropin-lengths).  The library's own counter of filled bytes must
rise, so that a misspelt macro is not a clean run.  test_every_carve_poisons_the_emulated_workspace (no GPU) pins the same
fills, which the host emulation does unconditionally, entry kind by entry kind."""
import glob
import os
import re
import time

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = os.path.join(ROOT, "world_amd", "variants")
CSRC = os.path.join(ROOT, "world_amd", "csrc")


def _lib(name):
    path = os.path.join(VARIANTS, f"libworld_hip_{name}.so")
    assert os.path.exists(path), f"{path} is missing: python -m world_amd.build --checked (or __graft_entry__.build()) builds it"
    return path


def _workloads():
    import torch
    from world_amd import synth
    out = []
    # configs[1]'s shape (48 kHz, Harvest + CheapTrick + D4C; 4096-point D4C transforms, 2048-point CheapTrick), ragged batch
    xs = [synth.vowel(48000, 1.3, seed=21, base_f0=120.0), synth.utterance(5, 48000, 0.9), synth.vowel(48000, 0.6, seed=4, base_f0=310.0)]
    L = max(x.numel() for x in xs)
    xb = torch.zeros((len(xs), L), dtype=torch.float64)
    for i, x in enumerate(xs):
        xb[i, :x.numel()] = x
    out.append(("48k harvest ragged", xb, 48000, [x.numel() for x in xs], dict(f0_method="harvest")))
    # configs[4]'s shape (16 kHz, DIO + StoneMask + CheapTrick 1024 + D4C 2048-point)
    xs = [synth.utterance(3, 16000, 1.1), synth.vowel(16000, 0.8, seed=9, base_f0=180.0)]
    L = max(x.numel() for x in xs)
    xb = torch.zeros((len(xs), L), dtype=torch.float64)
    for i, x in enumerate(xs):
        xb[i, :x.numel()] = x
    out.append(("16k dio ragged", xb, 16000, [x.numel() for x in xs], dict(f0_method="dio", q1=-0.15, threshold=0.85)))
    # a low voice at 48 kHz: D4C windows longer than half the transform, CheapTrick's longest smoothing segments
    out.append(("48k low voice", synth.vowel(48000, 0.8, seed=2, base_f0=62.0)[None].contiguous(), 48000, None, dict(f0_method="harvest", f0_floor=50.0)))
    # 22.05 kHz: Harvest's decimation ratio 3 (windows by rotation, not from the table), 2048-point D4C
    out.append(("22k harvest", synth.utterance(8, 22050, 0.8)[None].contiguous(), 22050, None, dict(f0_method="harvest")))
    # 176.4 kHz: the 16384-point D4C shape (sixteen wavefronts per workgroup, the group delay parked in global memory), windows
    # longer than half its transform, LoveTrain's run-time-length 16384-point transform, CheapTrick's 8192-point shape
    out.append(("176k dio low voice", synth.vowel(176400, 0.25, seed=6, base_f0=65.0)[None].contiguous(), 176400, None, dict(f0_method="dio", f0_floor=50.0)))
    return out


def _run(lib_path, workloads, repeats=1):
    import torch
    from world_amd.api import WorldHip
    wh = WorldHip(device=0, lib_path=lib_path)
    results = []
    for _ in range(repeats):
        res = []
        for name, x, fs, x_len, kw in workloads:
            tpos, f0, sp, ap, nf = wh.analyze(x.cuda(), fs, x_len=x_len, **kw)
            torch.cuda.synchronize()
            keep = []
            for u, n in enumerate(nf):                       # the valid frames only: padding is the caller's
                n = int(n)
                keep.append((tpos[u, :n].cpu().numpy(), f0[u, :n].cpu().numpy(), sp[u, :n].cpu().numpy(), ap[u, :n].cpu().numpy()))
            res.append(keep)
        results.append(res)
    wh.close()
    return results


def _same(a, b):
    return all(np.array_equal(x, y) for ua, ub in zip(a, b) for x, y in zip(ua, ub))


@gpu
def test_jitter_build_is_bit_identical():
    from world_amd.api import LIB_PATH
    work = _workloads()
    want = _run(LIB_PATH, work)[0]
    assert all(np.isfinite(arr).all() for wl in want for utt in wl for arr in utt)
    got = _run(_lib("jitter"), work, repeats=3)              # three passes: the stalls fall differently every time
    for rep, res in enumerate(got):
        for (name, *_), a, b in zip(work, want, res):
            assert _same(a, b), f"jitter build, pass {rep}, {name}: results differ from the product build's"


@gpu
def test_lds_poison_build_is_bit_identical():
    from world_amd.api import LIB_PATH
    work = _workloads()
    want = _run(LIB_PATH, work)[0]
    got = _run(_lib("poison"), work)[0]
    for (name, *_), a, b in zip(work, want, got):
        assert all(np.isfinite(arr).all() for utt in b for arr in utt), f"poison build, {name}: a NaN pattern reached the output"
        assert _same(a, b), f"poison build, {name}: results differ from the product build's"


@gpu
def test_hbm_poison_build_is_bit_identical():
    """the five workloads in ONE context of the -DWH_HBM_POISON library: every stage of every workload finds its workspace --
    grown by the 48 kHz batch, reused by the shorter shapes behind it -- refilled with 0xFF bytes"""
    from world_amd.api import LIB_PATH, load_library
    work = _workloads()
    want = _run(LIB_PATH, work)[0]
    counter = _poison_counter(load_library(_lib("hbm")))
    before = counter()
    got = _run(_lib("hbm"), work)[0]
    assert counter() > before, "hbm build: the poison counter did not rise"
    for (name, *_), a, b in zip(work, want, got):
        for ua, ub in zip(a, b):
            for x, y in zip(ua, ub):
                assert x.shape == y.shape and np.all(np.isfinite(y) | ~np.isfinite(x)), f"hbm build, {name}: a NaN pattern reached the output"
        assert _same(a, b), f"hbm build, {name}: results differ from the product build's"


# ==== every other kernel family ==============================================================================================
# A family is run(wh) -> [(name, numpy array), ...] on a WorldHip of the library under test (wh.lib_path names the file, for
# the drop-in symbols), built from deterministic inputs, returning only what the library promises to write: frames below
# n_frames, samples below the length, rows below `rows`.  Inputs are made once per process (_once) and shared by the runs.
_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def _pad(xs):
    """1-D torch signals -> ([B, L] zero-padded, lengths)"""
    import torch
    L = max(x.numel() for x in xs)
    xb = torch.zeros((len(xs), L), dtype=torch.float64)
    for i, x in enumerate(xs):
        xb[i, :x.numel()] = x
    return xb, [int(x.numel()) for x in xs]


def _signals(fs, specs):
    """specs: (kind, seconds, seed-or-index, base_f0) -> the padded batch on the host, made once"""
    from world_amd import synth

    def make():
        xs = [synth.vowel(fs, sec, seed=k, base_f0=f) if kind == "vowel" else synth.utterance(k, fs, sec) for kind, sec, k, f in specs]
        return _pad(xs)
    return _once(("signals", fs, tuple(specs)), make)


def _np(t):
    return t.detach().cpu().numpy()


def _frames(prefix, arrays, nf):
    """[(name, the valid frames of utterance u)] of tensors [B, F, ...]"""
    out = []
    for name, a in arrays:
        for u, n in enumerate(nf):
            out.append((f"{prefix}.{name}[{u}]", _np(a[u, :int(n)])))
    return out


def _params(fs, fft, nfs, seed0=0):
    """util.synth_params of a ragged batch: (f0 [B, F], sp, ap [B, F, fft/2+1] host arrays, padded with 0 / 1 / 1)"""
    from util import synth_params

    def make():
        F, nb = max(nfs), fft // 2 + 1
        f0, sp, ap = np.zeros((len(nfs), F)), np.ones((len(nfs), F, nb)), np.ones((len(nfs), F, nb))
        for u, n in enumerate(nfs):
            f0[u, :n], sp[u, :n], ap[u, :n] = synth_params(fs, n, fft, seed=seed0 + u)
        return f0, sp, ap
    return _once(("params", fs, fft, tuple(nfs), seed0), make)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- analysis routes outside the five workloads -----------------------------------------------------------------------------
def _analyze(wh, tag, fs, specs, **kw):
    xb, lens = _signals(fs, specs)
    tpos, f0, sp, ap, nf = wh.analyze(xb.cuda(), fs, x_len=lens, **kw)
    return _frames(tag, (("tpos", tpos), ("f0", f0), ("sp", sp), ("ap", ap)), nf)


def run_harvest_direct_form(wh):
    """tests/test_gpu_accuracy.py HV_CASES: at 16 kHz a 15 Hz floor puts the longest band filter past half a 4096-point
    block, so the bank runs in its direct form (hv_band_quirk, hv_band_events, hv_compact_events)"""
    return _analyze(wh, "16k floor 15", 16000, (("vowel", 0.4, 4, 110.0), ("utt", 0.3, 3, 0.0)), f0_method="harvest", f0_floor=15.0)


def run_harvest_ratio_1(wh):
    """HV_CASES: 11.025 kHz is analysed undecimated (hv_copy_signal, hv_partial_sums) and refined per frame.  Harvest
    alone: D4C refuses rates below 15.8 kHz"""
    xb, lens = _signals(11025, (("vowel", 0.4, 5, 150.0), ("utt", 0.3, 3, 0.0)))
    tpos, f0, nf = wh.harvest(xb.cuda(), 11025, x_len=lens)
    return _frames("11k", (("tpos", tpos), ("f0", f0)), nf)


def run_shared_device(wh):
    """the '48k low voice' workload on a shared_device context: one utterance keeps the narrow contour shapes"""
    assert wh.shared_device
    return _analyze(wh, "48k shared", 48000, (("vowel", 0.8, 2, 62.0),), f0_method="harvest", f0_floor=50.0)


def run_dio_speeds(wh):
    """DIO at speed 12 (decimated: dio_decimate_*) and at speed 1 (dio_copy_signal), then the stages one call each"""
    xb, lens = _signals(16000, (("utt", 0.4, 3, 0.0), ("vowel", 0.3, 9, 180.0)))
    x, out = xb.cuda(), []
    for speed in (12, 1):
        tpos, f0, nf = wh.dio(x, 16000, x_len=lens, speed=speed)
        out += _frames(f"dio speed {speed}", (("tpos", tpos), ("f0", f0)), nf)
    f0 = wh.stonemask(x, 16000, tpos, f0, nf, x_len=lens)
    sp = wh.cheaptrick(x, 16000, tpos, f0, nf, x_len=lens)
    ap = wh.d4c(x, 16000, tpos, f0, nf, 1024, x_len=lens)
    return out + _frames("stages", (("f0", f0), ("sp", sp), ("ap", ap)), nf)


def _block(wh, rows, cols):
    import torch
    return torch.zeros((rows, cols), dtype=torch.float64, device=wh.device)


def run_analyze_records(wh):
    """the coders fused into ct_frame and d4c_finish: coded records (60 dimensions) and packed records on both wires, ragged"""
    from world_amd.api import cheaptrick_fft_size, frame_count
    fs = 16000
    xb, lens = _signals(fs, (("vowel", 0.4, 7, 130.0), ("utt", 0.3, 3, 0.0)))
    x, fft = xb.cuda(), cheaptrick_fft_size(fs, 71.0)
    rows = sum(frame_count(fs, n, 5.0) for n in lens)
    out = []
    coded = _block(wh, rows, wh.lib.world_hip_coded_columns(fs, 60))
    assert sum(wh.analyze_coded(x, fs, coded, x_len=lens, number_of_dimensions=60)) == rows
    out.append(("coded records", _np(coded)))
    for wire in (0, 1):
        block = _block(wh, rows, wh.lib.world_hip_record_columns(fft, wire))
        assert sum(wh.analyze_packed(x, fs, block, x_len=lens)) == rows
        out.append((f"packed records wire {wire}", _np(block)))
    return out


def run_spectral_range(wh):
    """spectral_packed_range over an inner frame range, then a second range on the kept offset scans"""
    from world_amd.api import cheaptrick_fft_size
    fs = 16000
    xb, lens = _signals(fs, (("vowel", 0.4, 7, 130.0), ("utt", 0.3, 3, 0.0)))
    x, fft = xb.cuda(), cheaptrick_fft_size(fs, 71.0)
    tpos, f0, nf = wh.harvest(x, fs, x_len=lens)
    out = []
    for lo, hi, reuse in ((11, 40, False), (40, 53, True)):
        rows = int(sum(min(hi, int(n)) - min(lo, int(n)) for n in nf))
        block = _block(wh, rows, 2 + 2 * (fft // 2 + 1))
        assert wh.spectral_packed_range(x, fs, tpos, f0, nf, block, lo, hi, x_len=lens, reuse_offsets=reuse) == rows
        out.append((f"frames {lo}..{hi}", _np(block)))
    return out


def run_cheaptrick_fft_sizes(wh):
    """ct_frame at a caller-given fft_size: 48 kHz at 4096 (one step above the default) and at 8192"""
    fs = 48000
    xb, lens = _signals(fs, (("vowel", 0.3, 21, 120.0),))
    x = xb.cuda()
    tpos, f0, nf = wh.harvest(x, fs, x_len=lens)
    out = []
    for fft in (4096, 8192):
        sp = wh.cheaptrick(x, fs, tpos, f0, nf, x_len=lens, fft_size=fft)
        assert sp.shape[2] == fft // 2 + 1                                # (the size picks the template: cheaptrick.hip)
        out += _frames(f"fft {fft}", (("sp", sp),), nf)
    return out


# ---- synthesis ------------------------------------------------------------------------------------------------------------
def _synthesis(wh, fs, fft, nfs=(60, 47)):
    f0, sp, ap = _params(fs, fft, nfs)
    yl = [int(n * 5.0 / 1000.0 * fs) for n in nfs]
    y = wh.synthesis(_dev(f0), _dev(sp), _dev(ap), list(nfs), fft, 5.0, fs, yl)
    return [(f"y {fs}/{fft}[{u}]", _np(y[u, :n])) for u, n in enumerate(yl)]


def run_synthesis(wh):
    """ragged batch of two, voiced and unvoiced frames, 0.3 s: 16 kHz / 1024 and 48 kHz / 2048 (sy_pulse<4096>); then the
    shared randn table re-reduced on the device (rng_chunk_sums) against the host's sums"""
    out = _synthesis(wh, 16000, 1024) + _synthesis(wh, 48000, 2048)
    ok = wh.verify_tables()
    assert ok, "verify_tables(): the randn table on the device is not the host's stream"
    return out + [("verify_tables", np.array([float(ok)]))]


def run_synthesis_8192(wh):
    """48 kHz with fft_size 8192: lg_fft = 13 > 12 launches sy_pulse<8192>, whose spectrum C lives in global memory"""
    return _synthesis(wh, 48000, 8192)


def run_synthesize_records(wh):
    """Synthesis straight from f64, f32 and coded records (sy_stage_records decodes the coded rows in LDS)"""
    from world_amd.api import cheaptrick_fft_size, frame_count
    fs = 16000
    xb, lens = _signals(fs, (("vowel", 0.4, 7, 130.0), ("utt", 0.3, 3, 0.0)))
    x, fft = xb.cuda(), cheaptrick_fft_size(fs, 71.0)
    nf = [frame_count(fs, n, 5.0) for n in lens]
    yl = [int(n * 5.0 / 1000.0 * fs) for n in nf]
    out = []
    for wire, ndim in ((0, 0), (1, 0), (2, 25)):
        cols = wh.lib.world_hip_coded_columns(fs, ndim) if wire == 2 else wh.lib.world_hip_record_columns(fft, wire)
        block = _block(wh, sum(nf), cols)
        if wire == 2:
            wh.analyze_coded(x, fs, block, x_len=lens, number_of_dimensions=ndim)
        else:
            wh.analyze_packed(x, fs, block, x_len=lens)
        y = wh.synthesize_records(block, nf, fs, fft, 5.0, yl, wire=wire, number_of_dimensions=ndim)
        out += [(f"wire {wire} y[{u}]", _np(y[u, :n])) for u, n in enumerate(yl)]
    return out


# ---- real-time ------------------------------------------------------------------------------------------------------------
def run_realtime(wh):
    """three streams on chunk plans of their own (tests/test_realtime_cpu.py _stream_plans), a ring of 4 pointers that
    wraps several times, stream 2 fed with coded rows; then the drop-in WorldSynthesizer symbols of the same library"""
    from test_realtime_cpu import _lone_run, _stream_plans
    from world_amd.api import HostAPI
    fs, fft, bs, P, ndim = 16000, 1024, 64, 4, 25
    plans = _once(("rt plans",), lambda: _stream_plans(3, fs, fft, 48, seed=3))
    rt = wh.realtime(len(plans), fs, 5.0, fft, bs, P)
    dev = [(_dev(sp), _dev(ap)) for _, sp, ap, _ in plans]
    sp2, ap2 = dev[2]
    import torch
    coded = torch.cat([wh.code_spectral_envelope(sp2, fs, fft, ndim), wh.code_aperiodicity(ap2, fs, fft)], dim=1).contiguous()
    outs, pos, k, adds = [[] for _ in plans], [0] * len(plans), [0] * len(plans), [0] * len(plans)
    try:
        while True:
            busy = False
            for s, (f0, _, _, chunks) in enumerate(plans):
                if k[s] < len(chunks):
                    n, at = chunks[k[s]], pos[s]
                    if s == 2:
                        r = rt.add_coded(s, f0[at:at + n], coded[at:, :ndim], coded[at:, ndim:])
                    else:
                        r = rt.add(s, f0[at:at + n], dev[s][0][at:], dev[s][1][at:])
                    if r == 1:
                        pos[s] += n
                        k[s] += 1
                        adds[s] += 1
                    busy = True
            while True:
                out, produced = rt.synthesize()
                host = _np(out)
                for s in np.nonzero(produced)[0]:
                    outs[s].append(host[s].copy())
                if not produced.any():
                    break
            if not busy:
                break
    finally:
        rt.close()
    assert min(adds) > P, f"the rings did not wrap: {adds} adds into {P} pointers"
    res = [(f"stream {s}", np.concatenate(o)) for s, o in enumerate(outs)]
    assert all(a.size > 0 for _, a in res)
    lone = _lone_run(HostAPI(wh.lib_path), plans[0], fs, fft, bs, P)
    assert lone.size > 0
    return res + [("drop-in stream 0", lone)]


# ---- coders ---------------------------------------------------------------------------------------------------------------
CODER_SHAPES = [(16000, 1024), (48000, 2048), (48000, 4096), (16000, 128)]
CODER_DIMS = (1, 25, 60)
CODER_ROWS = 37


def run_coders(wh):
    """tests/test_codec.py's shapes, 37 rows.  The coder admits fft_size / 4 + 1 dimensions at the most: the 128-point
    shape takes its 33 in place of 60.  Every fourth decoded aperiodicity row is an aperiodic frame (mean band value above
    -0.5 dB), as there"""
    from backends import envelope
    from util import synth_params
    out = []
    for fs, fft in CODER_SHAPES:
        sp = _dev(_once(("envelope", fs, fft), lambda: envelope(fs, fft, CODER_ROWS, fs + fft)))
        ap = _dev(_once(("ap", fs, fft), lambda: synth_params(fs, CODER_ROWS, fft, seed=1)[2]))
        for ndim in sorted({min(d, fft // 4 + 1) for d in CODER_DIMS}):
            coded = wh.code_spectral_envelope(sp, fs, fft, ndim)
            back = wh.decode_spectral_envelope(coded, fs, fft)
            assert coded.shape == (CODER_ROWS, ndim) and back.shape == sp.shape
            out += [(f"{fs}/{fft}/{ndim} coded sp", _np(coded)), (f"{fs}/{fft}/{ndim} decoded sp", _np(back))]
        coded = wh.code_aperiodicity(ap, fs, fft)
        out.append((f"{fs}/{fft} coded ap", _np(coded)))
        coded[::4] = -0.3
        out.append((f"{fs}/{fft} decoded ap", _np(wh.decode_aperiodicity(coded, fs, fft))))
    return out


# ---- modification ---------------------------------------------------------------------------------------------------------
def run_modify(wh):
    """modify with an F0 scale, a formant shift and a log-F0 target (modify_f0's three reductions), f0_statistics, and
    resynthesize end to end"""
    fs, fft, nfs = 16000, 1024, (60, 47)
    f0, sp, _ = _params(fs, fft, nfs)
    d_f0, d_sp = _dev(f0), _dev(sp)
    out = [("f0 statistics", _np(wh.f0_statistics(d_f0, list(nfs))))]
    f0m, spm = wh.modify(d_f0, d_sp, list(nfs), fs, fft, f0_scale=[1.25, 0.8], formant_shift=[1.15, 0.87],
                         log_f0_target=([5.0, 4.7], [0.25, 0.1]))
    out += _frames("modify", (("f0", f0m), ("sp", spm)), nfs)
    xb, lens = _signals(fs, (("vowel", 0.4, 7, 130.0), ("utt", 0.3, 3, 0.0)))
    y, yl = wh.resynthesize(xb.cuda(), fs, x_len=lens, f0_scale=[1.2, 0.9], formant_shift=[0.9, 1.1], time_scale=1.25,
                            log_f0_target=([5.1, 4.9], [0.2, 0.15]))
    return out + [(f"resynthesize y[{u}]", _np(y[u, :int(n)])) for u, n in enumerate(yl)]


def run_modify_frames(wh):
    """modify_frames behind a non-integer time map with per-frame curves, and resynthesize_frames end to end"""
    import torch
    from world_amd.api import frame_count, uniform_time_map
    fs, fft, nfs, O = 16000, 1024, (60, 47), 71
    f0, sp, ap = _params(fs, fft, nfs)
    n_out = [71, 52]
    tm = torch.stack([torch.nn.functional.pad(uniform_time_map(n, o), (0, O - o)) for n, o in zip(nfs, n_out)])
    j = torch.arange(O, dtype=torch.float64, device=wh.device)
    curves = dict(f0_scale=(1.0 + 0.2 * torch.sin(j / 7.0))[None].repeat(2, 1), formant_shift=(1.0 + 0.1 * torch.cos(j / 11.0))[None].repeat(2, 1),
                  ap_gain=(0.8 + 0.4 * (j / O))[None].repeat(2, 1), f0_target=torch.where(j % 9 == 0, 200.0 + j, torch.zeros_like(j))[None].repeat(2, 1))
    outs = wh.modify_frames(_dev(f0), _dev(sp), _dev(ap), list(nfs), fs, fft, n_out=n_out, time_map=tm, **curves)
    out = _frames("modify_frames", zip(("f0", "sp", "ap"), outs), n_out)
    xb, lens = _signals(fs, (("vowel", 0.4, 7, 130.0), ("utt", 0.3, 3, 0.0)))
    nf = [frame_count(fs, n, 5.0) for n in lens]
    n_out = [int(nf[0] * 1.3), int(nf[1] * 0.8)]
    O = max(n_out)
    tm = torch.stack([torch.nn.functional.pad(uniform_time_map(n, o), (0, O - o)) for n, o in zip(nf, n_out)])
    j = torch.arange(O, dtype=torch.float64, device=wh.device)
    y, yl = wh.resynthesize_frames(xb.cuda(), fs, x_len=lens, n_out=n_out, time_map=tm, f0_scale=(1.0 + 0.1 * torch.sin(j / 5.0)),
                                   formant_shift=[1.1, 0.95])
    return out + [(f"resynthesize_frames y[{u}]", _np(y[u, :int(n)])) for u, n in enumerate(yl)]


# ---- alignment and morph --------------------------------------------------------------------------------------------------
ALIGN_PAIRS = [(17, 45), (130, 97)]                       # neither a multiple of align_cost's 16 x 32 tile
ALIGN_LONG = (2050, 2061)                                 # its longest diagonals pass kAlignAhead * kAlignDpThreads = 2048 cells


def _align_features(pairs, D, seed):
    def make():
        rng = np.random.default_rng(seed)
        Fa, Fb = max(p[0] for p in pairs), max(p[1] for p in pairs)
        a, b = np.zeros((len(pairs), Fa, D)), np.zeros((len(pairs), Fb, D))
        for u, (na, nb) in enumerate(pairs):
            walk = np.cumsum(rng.standard_normal((max(na, nb), D)), axis=0)
            a[u, :na] = walk[np.linspace(0, len(walk) - 1, na).astype(int)] + 0.1 * rng.standard_normal((na, D))
            b[u, :nb] = walk[np.linspace(0, len(walk) - 1, nb).astype(int)] + 0.1 * rng.standard_normal((nb, D))
        return a, b
    return _once(("align", tuple(pairs), D, seed), make)


def _align(wh, tag, pairs, D, seed):
    a, b = _align_features(pairs, D, seed)
    na, nb = [p[0] for p in pairs], [p[1] for p in pairs]
    path, path_len, summary, map_b, map_a = wh.align(_dev(a), _dev(b), na, nb)
    out = [(f"{tag} path_len", _np(path_len)), (f"{tag} summary", _np(summary))]
    for u, k in enumerate(_np(path_len)):
        out += [(f"{tag} path[{u}]", _np(path[u, :int(k)])), (f"{tag} map_b[{u}]", _np(map_b[u, :nb[u]])), (f"{tag} map_a[{u}]", _np(map_a[u, :na[u]]))]
    return out, path, path_len


def run_align(wh):
    out, _, _ = _align(wh, "ragged", ALIGN_PAIRS, 24, 5)
    assert min(ALIGN_LONG) > 2048
    long_out, _, _ = _align(wh, "long", [ALIGN_LONG], 3, 6)
    return out + long_out


def run_morph(wh):
    """morph along align's path: a constant rate, then per-frame rates as a cross-fade does"""
    import torch
    fs, fft = 16000, 1024
    _, path, path_len = _align(wh, "ragged", ALIGN_PAIRS, 24, 5)
    na, nb = [p[0] for p in ALIGN_PAIRS], [p[1] for p in ALIGN_PAIRS]
    A, B = _params(fs, fft, na, seed0=0), _params(fs, fft, nb, seed0=5)
    a, b = tuple(_dev(v) for v in A), tuple(_dev(v) for v in B)
    f0, sp, ap, no = wh.morph(a, b, na, nb, fs, fft, path=path, path_len=path_len, rate=0.3)
    out = _frames("constant", (("f0", f0), ("sp", sp), ("ap", ap)), no)
    O = max(wh.morph_length(x, y, 0.5) for x, y in zip(na, nb))
    fade = torch.linspace(0.0, 1.0, O, dtype=torch.float64, device=wh.device)
    f0, sp, ap, no, pos_a, pos_b = wh.morph(a, b, na, nb, fs, fft, path=path, path_len=path_len, time_rate=0.5, f0_rate=fade, sp_rate=fade,
                                            ap_rate=1.0 - fade, want_positions=True)
    return out + _frames("fade", (("f0", f0), ("sp", sp), ("ap", ap), ("pos_a", pos_a), ("pos_b", pos_b)), no)


# ---- resampling -----------------------------------------------------------------------------------------------------------
# (fs_in, fs_out): interpolation, a rational ratio, integer decimation by 3, by 4 (resample.inc: L == 1 and M a multiple of 4
# pads the LDS rows -- resample_decim_pad), equal rates
RESAMPLE_PAIRS = [(16000, 48000), (44100, 48000), (48000, 16000), (48000, 12000), (16000, 16000)]


def run_resample(wh):
    out = []
    for fs_in, fs_out in RESAMPLE_PAIRS:
        lens = [int(0.1 * fs_in) + 3, int(0.07 * fs_in)]
        x = _once(("noise", fs_in), lambda: 0.3 * np.random.default_rng(fs_in).standard_normal((2, max(lens))))
        for quality in ("best", "fast"):
            y, yl = wh.resample(_dev(x), fs_in, fs_out, x_len=lens, quality=quality)
            out += [(f"{fs_in}->{fs_out} {quality}[{u}]", _np(y[u, :int(n)])) for u, n in enumerate(yl)]
    return out


# ---- mel-cepstra ----------------------------------------------------------------------------------------------------------
def run_mcep(wh):
    """tests/test_mcep_gpu.py's shapes: 512-point envelopes, 67 rows (the last row tile is partial), orders 24 / 100 / 200
    (mcep_encode_64 / _128 / _256), back through mcep_decode, and one call on the strided view packed records give"""
    import torch
    from backends import envelope
    fft, rows, alpha = 512, 67, 0.42
    K = fft // 2 + 1
    sp = _dev(_once(("envelope", 16000, fft, rows), lambda: envelope(16000, fft, rows, 13)))
    out = []
    for order in (24, 100, 200):
        mc = wh.sp2mc(sp, order, alpha)
        out += [(f"sp2mc {order}", _np(mc)), (f"mc2sp {order}", _np(wh.mc2sp(mc, alpha, fft)))]
    block = torch.full((rows, 2 + 2 * K), -7.0, dtype=torch.float64, device=wh.device)
    block[:, 2:2 + K] = sp
    return out + [("sp2mc strided", _np(wh.sp2mc(block[:, 2:2 + K], 24, alpha)))]


# ---- deltas and MLPG ------------------------------------------------------------------------------------------------------
MLPG_LENS = (1, 2, 203)
MLPG_DIMS = (1, 60, 65)


def run_mlpg(wh):
    """window half-widths 0 / 1 / 2 (delta_rows_0 / _1 / _2; mlpg_static / mlpg_sweeps_2 / mlpg_sweeps_4), frames 1, 2 and
    203 in one ragged batch, a mask of several runs, per-frame, per-utterance and global variances"""
    import test_mlpg_cpu as cpu
    U, T = len(MLPG_LENS), max(MLPG_LENS)
    out = []
    for wname, win in cpu.WINDOWS.items():
        n_win = win.shape[0]
        for D in MLPG_DIMS:
            def make():
                rng = np.random.default_rng(100 * n_win + D)
                mask = rng.random((U, T)) < 0.9
                mask[2, 40:43] = mask[2, 90] = mask[2, 150:170] = False
                mask[2, 0] = mask[0, 0] = True
                return (rng.standard_normal((U, T, D)), mask, rng.standard_normal((U, T, n_win * D)), cpu.spread(rng, 3, (U, T, n_win * D)))
            c, mask, mean, var = _once(("mlpg", wname, D), make)
            d_mask, d_mean, d_var = _dev(mask), _dev(mean), _dev(var)
            windows = [list(r) for r in win]
            dl = wh.deltas(_dev(c), windows=windows, mask=d_mask, fill=cpu.FILL, n_frames=MLPG_LENS)
            out += _frames(f"{wname} D{D}", (("deltas", dl),), MLPG_LENS)
            for kind, v, m in (("frame", d_var, d_mask), ("utterance", d_var[:, 0].contiguous(), None), ("global", d_var[0, 0].contiguous(), d_mask)):
                gen = wh.mlpg(d_mean, v, windows=windows, mask=m, fill=cpu.FILL, n_frames=MLPG_LENS, precision=kind == "utterance")
                out += _frames(f"{wname} D{D} {kind}", (("mlpg", gen),), MLPG_LENS)
    return out


# ---- the Gaussian mixture -------------------------------------------------------------------------------------------------
def run_gmm(wh):
    """test_gmm_cpu.CONVERT in both modes (gmm_q, gmm_regress, gmm_posterior), ACCUMULATE (gmm_accumulate), and two
    iterations of the fit on two_clusters() from the given and from the default start"""
    import test_gmm_cpu as cpu
    from backends import OnGpu

    class GpuBackend(OnGpu, cpu.Backend):
        pass

    be = GpuBackend(wh)
    out = []
    for M, dx, dy, rows, strided in cpu.CONVERT:
        model, parts = cpu.prepared(be, M, dx, dy)
        d_model, x = be.model_dev(model), cpu.rows_near(parts, rows, 11)
        for mode in (0, 1):
            got = be.convert(M, dx, dy, d_model, x, mode=mode, slack=3 if strided else 0, before=1 if strided else 0)
            out += [(f"convert M{M} dx{dx} dy{dy} rows{rows} mode{mode} {k}", v) for k, v in got.items()]
    M, dx, dy, rows = 5, 17, 16, 130
    model, parts = cpu.prepared(be, M, dx, dy)
    gm = wh.gmm_prepare(*cpu.random_model(M, dx, dy, 1), dx)
    post, loglik = wh.gmm_posterior(gm, _dev(cpu.rows_near(parts, rows, 47)))
    out += [("posterior", _np(post)), ("posterior loglik", _np(loglik))]
    for M, P, rows in cpu.ACCUMULATE:
        for name, v in zip(("N", "S1", "G"), be.accumulate(*cpu.stats_inputs(M, P, rows), slack=2)):
            out.append((f"accumulate M{M} P{P} rows{rows} {name}", v))
    z, w0, mu0, cov0 = cpu.two_clusters()
    for tag, init in (("given start", (w0, mu0, cov0)), ("default start", None)):
        for name, v in zip(("w", "mu", "cov", "loglik"), wh.gmm_fit(_dev(z), 2, n_iter=2, reg=1e-6, init=init)):
            out.append((f"fit {tag} {name}", v))
    return out


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def run_plumbing(wh):
    import torch
    fs, fft, nfs = 16000, 1024, (23, 9)
    f0, sp, ap = _params(fs, fft, nfs)
    tpos = np.arange(max(nfs))[None].repeat(2, 0) * 0.005
    block = _block(wh, sum(nfs) + 2, 2 + 2 * (fft // 2 + 1))
    wh.pack_results(_dev(tpos), _dev(f0), _dev(sp), _dev(ap), list(nfs), block, first_row=1)
    out = [("packed", _np(block))]
    out += _frames("unpacked", zip(("tpos", "f0", "sp", "ap"), wh.unpack_results(block, list(nfs), first_row=1)), nfs)
    pcm = _once(("pcm",), lambda: np.random.default_rng(9).integers(-32768, 32768, 3001).astype(np.int16))
    out.append(("pcm16_to_double", _np(wh.pcm16_to_double(_dev(pcm)))))
    raw = _dev(pcm.view(np.uint8)[:3000])
    for nbit in (8, 16, 24):
        out.append((f"pcm_to_double {nbit}", _np(wh.pcm_to_double(raw, nbit))))
    out.append(("double_to_pcm16", _np(wh.double_to_pcm16(_dev(pcm.astype(np.float64) / 30000.0)))))
    # the per-frame transform alone: a 2048-point static plan, a 512-point run-time plan, radix 8 and radix 16 last stages
    for N, static, max_lr in ((2048, True, 3), (512, False, 3), (512, False, 4)):
        x = _dev(_once(("fft rows", N), lambda: np.random.default_rng(N).standard_normal((3, N))))
        spec = wh.probe_rfft(x, max_lr=max_lr, static_plan=static)
        out += [(f"rfft {N} {static} {max_lr}", _np(spec)), (f"irfft {N} {static} {max_lr}", _np(wh.probe_irfft(spec, max_lr=max_lr, static_plan=static)))]
    torch.cuda.synchronize()
    return out


# ---- fft.h's compositions in isolation (tests/test_gpu_fft_routes.py: ROUTES) -----------------------------------------------
def run_fft_routes(wh):
    """every mode of world_hip_probe_fft at 4096 points, and one more size wherever a mode's template differs by length (the
    compile-time plans, d4c_frame's shapes, a plan with a radix-2 / radix-4 remainder): the wave-local stages that drop
    workgroup barriers are what the jitter build is for"""
    import torch
    from test_gpu_fft_routes import ROUTES, threads_of
    out = []
    for route in ROUTES:
        sizes = {"twiddles": (11, 12, 13, 14), "dft8": (3,)}.get(route["kind"]) or \
            (tuple(route["lgs"]) if len(route["lgs"]) <= 4 else (6, 9, 12))
        for swz in route["swz"]:
            for lg in (g for g in sizes if g in route["lgs"]):
                n = 1 << lg
                shape = {"r2c": (3, n), "r2c_twice": (3, n), "c2r": (3, n // 2 + 1, 2)}.get(route["kind"], (3, n, 2))
                x = _once(("fft route rows", shape), lambda: np.random.default_rng(n + len(shape)).standard_normal(shape))
                if route["kind"] == "c2c_half":
                    x = x.copy(); x[:, n // 2 + 1:] = 0.0
                for max_lr in route["max_lr"]:
                    threads = threads_of(route, lg)
                    threads = threads[len(threads) // 2]
                    out.append((f"mode {route['mode']} swz {swz} lg {lg} max_lr {max_lr} threads {threads}",
                                _np(wh.probe_fft(route["mode"], _dev(x), max_lr=max_lr, threads=threads, swizzle=swz))))
    torch.cuda.synchronize()
    return out


# ---- D4C's band selection in isolation (tests/test_d4c_select_cpu.py) ---------------------------------------------------------
def run_d4c_select(wh):
    """the designed rows of test_d4c_select_cpu.py -- every route, every entry of the general routine, the ties, the positions
    of the threshold and the top key -- and its real-valued rows, at all four workgroup sizes, through block_excluding_largest
    (mode 0) and through the general routine directly (mode 1).  The select places its barriers by hand and its histograms
    alias a buffer the probe marks dead, as d4c_frame does: a missing barrier on a fallback route changes these bits"""
    import torch
    import test_d4c_select_cpu as cpu
    out = []
    for nt in cpu.NTS:
        work = [(b.name, b.K, cpu.realise(b.P, cpu.SCALES["2^-80"])) for b in cpu.batches_routes(nt) + cpu.batches_general(nt) + cpu.batches_positions(nt)]
        for name, K, keys in work + list(cpu.real_rows(nt)):
            d_keys = _dev(keys)
            for mode in (0, 1):
                out.append((f"NT {nt} {name} mode {mode}", _np(wh.probe_select(d_keys, K, mode=mode))))
    torch.cuda.synchronize()
    return out


# ---- Harvest's contour stage in isolation (tests/harvest_contour_cases.py) ----------------------------------------------------
def run_harvest_contour(wh):
    """made-up candidate maps through world_hip_probe_harvest_contour: the wide-slot map (252 slots: four per tracking lane, the
    ring of two), the many-section map (hc_merge out of HBM beside hc_merge in LDS, the smoother out of HBM) and a ragged batch
    (nc = 0, 2, 14; 1 .. 2600 frames).  The walks of hc_extend park their picks in a slice other wavefronts sum afterwards, and
    hc_merge and hc_smooth reuse the section table and the slices of the passes before: a missing barrier, a read of LDS or of
    workspace nobody wrote changes these bits"""
    import torch
    import backends
    import harvest_contour_cases as cases

    class OnWh(backends.OnGpu, cases.Backend):
        pass
    be, out = OnWh(wh), []
    for name in ("extend 252", "many sections", "ragged 5.0"):
        g = cases.group(name)
        for u, o in zip(g.utts, be.run(g)):
            out += [(f"{name} {u.name} {k}", np.array(o[k])) for k in cases.OUT_ROWS + ("pruned_cand", "pruned_score", "tpos", "f0")]
            out.append((f"{name} {u.name} sections", np.array(o["sec"][:2, :o["sec_n"][0]], dtype=np.float64)))
    torch.cuda.synchronize()
    return out


# ---- Harvest's candidate stage in isolation (tests/harvest_candidates_cases.py) ---------------------------------------------------
def run_harvest_candidates(wh):
    """made-up zero-crossing lists through world_hip_probe_harvest_candidates: the lists the proportional guess does not bracket
    (the eight 32-lane searches of a workgroup share their ballots two to a wavefront), the runs at the staged capacity (range[]
    is written by lanes 0 of eight groups and read by everybody across a barrier; staged and unstaged routes side by side), five
    ragged utterances in groups of two (the next group's lists overwrite the one before in the same workspace: a stale read
    changes the bits) and a 300-segment compaction (the scan's second trip, the flat copy's eight loads in flight)"""
    import torch
    import backends
    import harvest_candidates_cases as cases

    class OnWh(backends.OnGpu, cases.Backend):
        pass
    be, out = OnWh(wh), []
    for name, ev_group in (("guess misses", 40), ("cap edge", 40), ("groups", 2)):
        g = cases.group(name)
        for u, o in zip(g.utts, be.run_group(g, ev_group=ev_group)):
            out += [(f"{name} {u.name} {k}", np.array(o[k], dtype=np.float64)) for k in ("raw", "cand", "nc")]
    seg_events, seg_count, ev_cap, _ = cases.compaction_arrays("300 segments")
    h = be.run([10], np.full(12, 100.0), seg_events=seg_events, seg_count=seg_count, ev_cap=ev_cap, stages=1)
    out += [("300 segments events", np.array(h["events"])), ("300 segments ev_count", np.array(h["ev_count"], dtype=np.float64))]
    torch.cuda.synchronize()
    return out


# ---- Harvest's refinement stage in isolation (tests/harvest_refine_cases.py) ------------------------------------------------------
def run_harvest_refine(wh):
    """made-up candidate maps through world_hip_probe_harvest_refine on every route: the "caches" group (what hv_refine_frames
    keeps in registers and LDS from slot to slot and track to track), "edges" (windows clamped at the signal ends, the empties
    the first and last source frames own) and "batches" (ragged rows, frame counts that leave wavefronts of a workgroup idle).
    LDS poison is the interesting build: hv_refine's idle eighth lane group and its `more ? ... : 0` step read LDS whose
    values must be discarded, and the frame cache is read through a clamp"""
    import torch
    import backends
    import harvest_refine_cases as cases

    class OnWh(backends.OnGpu, cases.Backend):
        pass
    be, out = OnWh(wh), []
    for name in ("caches", "edges", "batches"):
        g = cases.group(name)
        for route in g.routes:
            res = be.run(g.utts, route, g.maxc) if g.batch else [be.run([u], route, g.maxc)[0] for u in g.utts]
            for u, o in zip(g.utts, res):
                out += [(f"{name} {u.name} route {route} {k}", o[k]) for k in ("refined", "score")]
    torch.cuda.synchronize()
    return out


# ---- the drop-in symbols at shrinking and growing lengths --------------------------------------------------------------------
DROPIN_SECONDS = (0.5, 0.2, 0.31)


def run_dropin_lengths(wh):
    """the reference's own entry points (HostAPI on the library under test, as run_realtime does) on one 16 kHz utterance cut
    to 0.5 s, 0.2 s and 0.31 s, in that order, through the library's one slot pool: the slot's device buffers and its resident
    copy of the signal are sized by the longest call so far, so the shorter calls run with a longer call's tail behind their
    data (and, from the second pass in a process on, the 0.5 s call with the 0.31 s call's data under its own)"""
    from world_amd import synth
    from world_amd.api import HostAPI
    fs, ndim = 16000, 25

    def make():
        full = synth.utterance(3, fs, max(DROPIN_SECONDS)).numpy()
        return [np.ascontiguousarray(full[:int(s * fs)]) for s in DROPIN_SECONDS]
    H = HostAPI(wh.lib_path)
    fft = H.cheaptrick_fft_size(fs)
    out = []
    for sec, x in zip(DROPIN_SECONDS, _once(("dropin cuts",), make)):
        tp, f0 = H.harvest(x, fs)
        tp_d, f0_d = H.dio(x, fs)
        f0_s = H.stonemask(x, fs, tp_d, f0_d)
        sp = H.cheaptrick(x, fs, tp, f0)
        ap = H.d4c(x, fs, tp, f0, fft)
        assert sp.shape == ap.shape == (len(f0), fft // 2 + 1) and (f0 > 0).any()
        y = H.synthesis(f0, sp, ap, fft, 5.0, fs, len(x))
        coded_sp, coded_ap = H.code_spectral_envelope(sp, fs, fft, ndim), H.code_aperiodicity(ap, fs, fft)
        out += [(f"{sec} s {name}", a) for name, a in (
            ("harvest tpos", tp), ("harvest f0", f0), ("dio tpos", tp_d), ("dio f0", f0_d), ("stonemask f0", f0_s), ("sp", sp), ("ap", ap),
            ("y", y), ("coded sp", coded_sp), ("decoded sp", H.decode_spectral_envelope(coded_sp, fs, fft)), ("coded ap", coded_ap),
            ("decoded ap", H.decode_aperiodicity(coded_ap, fs, fft)))]
    return out


# ---- the coverage table: which kernels (world_amd/csrc: __global__ void NAME) each family launches -------------------------
_CONTOUR = ("hc_step12_sections", "hc_extend", "hc_merge", "hc_smooth", "hc_output")
_HARVEST_TAIL = ("hv_remove_mean", "hv_raw_candidates", "hv_detect", "hv_prune") + _CONTOUR
_FUSED_SPECTRAL = ("spectral_prepare", "ct_frame", "d4c_lovetrain", "d4c_frame", "d4c_finish")
_SYNTHESIS = ("sy_increments", "sy_phase_serial", "sy_detect", "sy_compact", "sy_pulse", "sy_overlap_add")
_HARVEST_FFT = ("hv_decimate_fwd", "hv_decimate_bwd", "hv_band_spectra", "hv_block_spectra", "hv_band_events_fft") + _HARVEST_TAIL

# Measured on one MI355X, the whole test of a family (seven passes and four contexts): modify-frames 0.78 s,
# harvest-direct-form 0.68 s, gmm 0.24 s, realtime 0.17 s, mcep 0.14 s, synthesis 0.13 s, mlpg and shared-device 0.12 s, every
# other family below 0.1 s; one jitter pass 0.17 s (harvest-direct-form) and 0.03 s or less elsewhere.
# With the hbm leg (nine passes and five contexts): harvest-direct-form 0.85 s, modify-frames 0.82 s, mlpg 0.28 s, dropin-lengths
# 0.26 s, realtime 0.22 s, mcep 0.18 s, gmm 0.16 s, shared-device and synthesis 0.15 s, every other family 0.12 s or less; one
# hbm pass 0.17 s (harvest-direct-form) and 0.03 s or less elsewhere, filling 3 MiB (mcep) to 486 MiB (dropin-lengths: every
# slot buffer at every call); test_families_share_one_context 0.6 s on either library.
FAMILIES = {
    # name: (run, the kernels it must launch, WorldHip keyword arguments)
    "harvest-direct-form": (run_harvest_direct_form, ("hv_decimate_fwd", "hv_decimate_bwd", "hv_band_quirk", "hv_band_events", "hv_compact_events")
                            + _HARVEST_TAIL + _FUSED_SPECTRAL, {}),
    "harvest-ratio-1": (run_harvest_ratio_1, ("hv_copy_signal", "hv_partial_sums", "hv_refine_frames") + _HARVEST_TAIL, {}),
    "shared-device": (run_shared_device, _HARVEST_FFT + _FUSED_SPECTRAL, dict(shared_device=True)),
    "dio-speeds": (run_dio_speeds, ("dio_decimate_fwd", "dio_decimate_bwd", "dio_copy_signal", "dio_partial_sums", "dio_remove_mean", "dio_lowcut",
                                    "dio_nyquist_slices", "dio_nyquist_bins", "dio_band_quirk", "dio_band_events", "dio_compact_events",
                                    "dio_candidates", "dio_step1", "dio_step2", "dio_track_sweeps", "dio_time_axis", "sm_frame", "ct_prepare",
                                    "ct_frame", "d4c_prepare1", "d4c_lovetrain", "d4c_frame", "d4c_finish"), {}),
    "analyze-records": (run_analyze_records, _HARVEST_FFT + ("hv_refine",) + _FUSED_SPECTRAL + ("ct_frame_coded",), {}),
    "spectral-range": (run_spectral_range, ("ct_frame", "d4c_lovetrain", "d4c_frame", "d4c_finish"), {}),
    "cheaptrick-fft-sizes": (run_cheaptrick_fft_sizes, ("ct_prepare", "ct_frame"), {}),
    "synthesis": (run_synthesis, _SYNTHESIS + ("rng_stream_fill", "rng_chunk_sums"), {}),
    "synthesis-8192": (run_synthesis_8192, _SYNTHESIS, {}),
    "synthesize-records": (run_synthesize_records, ("sy_stage_records",) + _SYNTHESIS, {}),
    "realtime": (run_realtime, ("rt_pulse", "rt_overlap_add", "rt_store_rows", "rt_store_coded_rows", "codec_code_sp", "codec_code_ap"), {}),
    "coders": (run_coders, ("codec_code_sp", "codec_decode_sp", "codec_code_ap", "codec_decode_ap"), {}),
    "modify": (run_modify, ("modify_f0", "modify_warp_sp") + _SYNTHESIS, {}),
    "modify-frames": (run_modify_frames, ("modify_frames_f0", "modify_frames_sp", "modify_frames_ap") + _SYNTHESIS, {}),
    "align": (run_align, ("align_cost", "align_dp", "align_path"), {}),
    "morph": (run_morph, ("align_cost", "align_dp", "align_path", "morph_positions", "morph_frames_f0", "morph_frames_sp", "morph_frames_ap"), {}),
    "resample": (run_resample, ("resample_poly", "resample_decim", "resample_decim_pad", "resample_copy"), {}),
    "mcep": (run_mcep, ("mcep_encode_64", "mcep_encode_128", "mcep_encode_256", "mcep_decode"), {}),
    "mlpg": (run_mlpg, ("delta_rows_0", "delta_rows_1", "delta_rows_2", "mlpg_static", "mlpg_sweeps_2", "mlpg_sweeps_4"), {}),
    "gmm": (run_gmm, ("gmm_q", "gmm_regress", "gmm_posterior", "gmm_accumulate", "gmm_fill"), {}),
    "plumbing": (run_plumbing, ("ex_pack_rows", "ex_unpack_rows", "pcm16_to_double", "pcm_bytes_to_double", "double_to_pcm16",
                                "fft_probe_rfft<3, 11>", "fft_probe_irfft<3, 11>", "fft_probe_rfft<3>", "fft_probe_irfft<3>",
                                "fft_probe_rfft<4>", "fft_probe_irfft<4>"), {}),
    "fft-routes": (run_fft_routes, tuple(f"fft_route_rfft<{a}>" for a in ("0, 3", "0, 4", "1, 3", "0, 3, 10", "0, 3, 11", "0, 3, 12", "1, 3, 11"))
                   + tuple(f"fft_route_irfft<{a}>" for a in ("0, 3", "0, 4", "0, 3, 10", "0, 3, 11", "0, 3, 12"))
                   + tuple(f"fft_route_rfft_from<{a}>" for a in ("0, 3", "0, 3, 10", "0, 3, 11", "0, 3, 12"))
                   + ("fft_route_cfft<0>", "fft_route_cfft_from<0>", "fft_route_rfft_items<0, 12, 256, false>", "fft_route_rfft_items<1, 12, 256, true>",
                      "fft_route_irfft_items<0, 12, 256, true>", "fft_route_irfft_items<0, 12, 256, false>")
                   + tuple(f"fft_route_d4c_rfft<1, {n}, {n // 16}, {k}>" for n in (2048, 4096, 8192, 16384) for k in (0, 1, 2))
                   + tuple(f"fft_route_d4c_twiddles<1, {n}, {n // 16}>" for n in (2048, 4096, 8192, 16384))
                   + tuple(f"fft_route_dft8<{s}, {h}>" for s in (0, 1) for h in ("false", "true")), {}),
    "d4c-select": (run_d4c_select, tuple(f"d4c_select_probe<{nt}>" for nt in (128, 256, 512, 1024)), {}),
    "harvest-contour": (run_harvest_contour, ("hv_prune",) + _CONTOUR, {}),
    "harvest-candidates": (run_harvest_candidates, ("hv_compact_events", "hv_raw_candidates", "hv_detect"), {}),
    "harvest-refine": (run_harvest_refine, ("hv_refine", "hv_refine_frames"), {}),
    "dropin-lengths": (run_dropin_lengths, _HARVEST_TAIL + ("dio_candidates", "dio_track_sweeps", "sm_frame", "ct_frame", "d4c_lovetrain", "d4c_frame",
                                                            "d4c_finish", "codec_code_sp", "codec_decode_sp", "codec_code_ap", "codec_decode_ap")
                       + _SYNTHESIS, {}),
}
# (harvest-contour is not among them: the probe carves Harvest's back-half workspace at every call.)
# Families whose calls carve nothing from the arena and keep no buffer of their own between calls (cached tables apart): a
# second pass in the same context has nothing to refill, so the hbm build's counter need only rise in the first (the tables'
# allocation).  Every other family must see it rise in both passes.
NO_WORKSPACE = ("coders", "resample", "mcep", "plumbing", "fft-routes", "d4c-select", "harvest-refine")
# profile labels that are not the kernel's own name (devrt::launch_blocks("label", kernel<...>, ...))
LABELS = {"ct_frame_coded": "ct_frame"}
# kernels that run only while a process-wide table is built: asserted on the first pass of the jitter library, which nothing
# but this module loads (the product library's table may stand already when another module's context is still alive)
COLD_ONLY = ("rng_stream_fill",)
EXEMPT = {
    "mp_fill": "machine probe: measures the hardware (world_hip_probe_machine), no result to compare",
    "mp_touch": "machine probe: measures the hardware, no result to compare",
    "mp_chase": "machine probe: measures memory latency, no result to compare",
    "mp_fp64_load": "machine probe: measures the clock under FP64 load, no result to compare",
    "mp_lds": "machine probe: measures the LDS round trip, no result to compare",
}


def _kernel_of(label):
    """the __global__ function a profile label or a claim names: 'fft_probe_rfft<3, 11>' -> 'fft_probe_rfft'"""
    base = re.match(r"\(?\s*(\w+)", label).group(1)
    return LABELS.get(base, base)


def kernels_in_source():
    """every `__global__ void [__launch_bounds__(...)] [ATTRIBUTE_MACRO] name(` of world_amd/csrc/*.hip and *.inc"""
    pattern = re.compile(r"__global__\s+void\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?(?:[A-Z][A-Z0-9_]*\s+)?(\w+)\s*\(")
    names = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc"))):
        with open(path) as f:
            for name in pattern.findall(f.read()):
                names.setdefault(name, os.path.basename(path))
    return names


def claimed_kernels():
    return {_kernel_of(k) for _, kernels, _ in FAMILIES.values() for k in kernels}


def unclaimed_kernels(source, claimed, exempt):
    return sorted(k for k in source if k not in claimed and k not in exempt)


def test_every_kernel_is_claimed_by_a_family():
    source = kernels_in_source()
    assert len(source) > 100 and "d4c_frame" in source and "mcep_encode_64" in source and "align_dp" in source, "the scan lost the kernels"
    missing = unclaimed_kernels(source, claimed_kernels(), EXEMPT)
    assert not missing, ("kernels that no family of tests/test_gpu_checked_builds.py runs under the jitter and LDS-poison builds: "
                         + ", ".join(f"{k} ({source[k]})" for k in missing))
    stale = sorted(k for k in (claimed_kernels() | set(EXEMPT)) if k not in source)
    assert not stale, f"claimed or exempt, but no longer in world_amd/csrc: {stale}"
    assert all(k.startswith("mp_") and reason for k, reason in EXEMPT.items())
    # the scan itself: a kernel taken out of the table is reported
    assert unclaimed_kernels(source, claimed_kernels() - {"align_dp"}, EXEMPT) == ["align_dp"]


def _exports(path, symbol):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return any(line.split()[-1] == symbol for line in out.splitlines() if line.strip())


def test_every_carve_poisons_the_emulated_workspace():
    """The host emulation refills what -DWH_HBM_POISON refills (devrt::dpoison, 0xFF bytes = NaN / -1), always: the counter
    rises across a call of each entry kind -- begin_stage (Harvest), a spectral stage without and with reuse_offsets,
    hold_at_floor (resynthesize), a drop-in call -- by at least what that kind promises to fill, and the results stay what
    they were: the reused offsets and the LoveTrain pass survive a reuse call's fill, the analysis held at the floor survives
    the stages' fills above it.  Only the checked build exports the counter."""
    import ctypes as C
    from backends import emu_library, new_context
    from world_amd import synth
    from world_amd.api import LIB_PATH, CheapTrickOption, D4COption, HarvestOption, HostAPI, cheaptrick_fft_size, frame_count, modifications
    assert not _exports(LIB_PATH, "world_hip_debug_poisoned_bytes"), "the product library exports the checked build's counter"
    assert _exports(_lib("hbm"), "world_hip_debug_poisoned_bytes"), "libworld_hip_hbm.so was built without -DWH_HBM_POISON"
    L = emu_library()
    L.world_hip_debug_poisoned_bytes.restype = C.c_ulonglong
    poisoned = L.world_hip_debug_poisoned_bytes
    fs, ip = 16000, C.POINTER(C.c_int)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    h, c, d = HarvestOption(71.0, 800.0, 5.0), CheapTrickOption(-0.15, 71.0, cheaptrick_fft_size(fs, 71.0)), D4COption(0.85)
    fft, nb = c.fft_size, c.fft_size // 2 + 1

    def batch(seconds):
        xs = [synth.vowel(fs, s, seed=11 + u, base_f0=140.0 + 60 * u).numpy() for u, s in enumerate(seconds)]
        x = np.zeros((len(xs), max(len(v) for v in xs)))
        for u, v in enumerate(xs):
            x[u, :len(v)] = v
        xl = np.array([len(v) for v in xs], dtype=np.int32)
        return x, xl, np.array([frame_count(fs, int(n), 5.0) for n in xl], dtype=np.int32)

    ctx = new_context(L)
    try:
        def harvest(x, xl, nf):
            F = int(nf.max())
            tp, f0 = np.zeros((len(xl), F)), np.zeros((len(xl), F))
            assert L.world_hip_harvest_batch(ctx, len(xl), fs, vp(x), x.shape[1], xl.ctypes.data_as(ip), C.byref(h), F, vp(tp), vp(f0)) == 0
            return tp, f0

        # begin_stage: a long call sizes the arena, the short one behind it finds all of it refilled (and allocates nothing)
        harvest(*batch((0.3, 0.22)))
        x, xl, nf = batch((0.12, 0.09))
        B, F = len(xl), int(nf.max())
        cap, before = int(L.world_hip_workspace_bytes(ctx)), poisoned()
        tp, f0 = harvest(x, xl, nf)
        assert cap > 0 and int(L.world_hip_workspace_bytes(ctx)) == cap and poisoned() - before >= cap
        assert (f0 > 0).any() and np.isfinite(f0).all()
        tp_lone, f0_lone = harvest(x[:1, :xl[0]].copy(), xl[:1], nf[:1])
        assert np.array_equal(f0_lone[0], f0[0, :nf[0]])

        # the spectral stages, whole and in frame ranges: fresh claims are refilled; a reuse_offsets call refills nothing of
        # CheapTrick's (all it carves is the prepared offsets) and only the scratch behind D4C's prepared arrays
        args = (ctx, B, fs, vp(x), x.shape[1], xl.ctypes.data_as(ip), nf.ctypes.data_as(ip), F, vp(tp), vp(f0))
        sp_full, ap_full = np.zeros((B, F, nb)), np.zeros((B, F, nb))
        assert L.world_hip_cheaptrick_batch(*args, C.byref(c), vp(sp_full)) == 0
        assert L.world_hip_d4c_batch(*args, fft, C.byref(d), vp(ap_full)) == 0
        assert np.isfinite(sp_full).all() and np.isfinite(ap_full).all() and (ap_full[f0 > 0] < 0.5).any()
        sp, ap = np.full((B, F, nb), -1.0), np.full((B, F, nb), -1.0)
        rises = {}
        for lo, hi, reuse in ((0, 9, 0), (9, 17, 1), (17, F, 1)):
            before = poisoned()
            assert L.world_hip_cheaptrick_batch_range(*args, C.byref(c), lo, hi, reuse, vp(sp)) == 0, L.world_hip_last_error()
            rises["ct", reuse] = poisoned() - before
            before = poisoned()
            assert L.world_hip_d4c_batch_range(*args, fft, C.byref(d), lo, hi, reuse, vp(ap)) == 0, L.world_hip_last_error()
            rises["d4c", reuse] = poisoned() - before
        assert rises["ct", 0] >= 4 * B * F and rises["ct", 1] == 0
        assert rises["d4c", 1] >= 8 * 16 * B * F and rises["d4c", 0] >= rises["d4c", 1] + 8 * B * F + 4 * 2 * B * F
        for u, n in enumerate(nf):                                              # what the first range prepared was still intact
            assert np.array_equal(sp[u, :n], sp_full[u, :n]) and np.array_equal(ap[u, :n], ap_full[u, :n])

        # hold_at_floor: the whole arena before its carve; the analysis it holds there survives the stages above
        yl = np.array([L.world_hip_resynthesis_length(fs, int(n), 5.0, 1.0) for n in nf], dtype=np.int32)
        y = np.zeros((B, int(yl.max())))
        before = poisoned()
        assert L.world_hip_resynthesize_batch(ctx, B, fs, vp(x), x.shape[1], xl.ctypes.data_as(ip), C.byref(h), C.byref(c), C.byref(d),
                                              modifications(B, 1.0, 1.0, None), 1.0, yl.ctypes.data_as(ip), y.shape[1], vp(y)) == 0
        assert poisoned() - before >= int(L.world_hip_workspace_bytes(ctx))
        y2 = np.zeros_like(y)
        assert L.world_hip_synthesis_batch(ctx, B, fs, 5.0, fft, nf.ctypes.data_as(ip), F, vp(f0), vp(sp_full), vp(ap_full),
                                           yl.ctypes.data_as(ip), y.shape[1], vp(y2)) == 0
        assert np.array_equal(y, y2) and np.max(np.abs(y)) > 0

        # a drop-in call: the slot's buffers and the resident signal, a shorter signal behind a longer one
        H = HostAPI(L._name)
        x_long, x_short = np.ascontiguousarray(x[0, :xl[0]]), np.ascontiguousarray(x[1, :xl[1]])
        H.harvest(x_long, fs)
        before = poisoned()
        tp_d, f0_d = H.harvest(x_short, fs)
        assert poisoned() - before >= 8 * len(x_long) + 2 * 8 * int(nf[0])     # the resident signal's capacity, two frame buffers'
        assert np.array_equal(f0_d, f0[1, :nf[1]]) and np.array_equal(tp_d, tp[1, :nf[1]])
    finally:
        L.world_hip_destroy(ctx)


# ---- the helper -----------------------------------------------------------------------------------------------------------
def _open(lib_path, kw):
    from world_amd.api import WorldHip
    wh = WorldHip(device=0, lib_path=lib_path, **kw)
    wh.lib_path = lib_path
    return wh


def _poison_counter(lib):
    """world_hip_debug_poisoned_bytes of a loaded -DWH_HBM_POISON library: absent, the build is not what its name says"""
    import ctypes as C
    fn = getattr(lib, "world_hip_debug_poisoned_bytes", None)
    assert fn is not None, "the library does not export world_hip_debug_poisoned_bytes: it was not built with -DWH_HBM_POISON"
    fn.restype = C.c_ulonglong
    return fn


def _run_family(lib_path, run, kw, repeats=1, profile_first=False, poisoned=None):
    """-> ([result of each pass], {kernel: launches} of the first pass when profiled, seconds per pass); poisoned: a list
    that receives the bytes the library's dpoison filled during each pass (the hbm build)"""
    import torch
    wh = _open(lib_path, kw)
    results, launches, seconds = [], {}, []
    counter = _poison_counter(wh.lib) if poisoned is not None else None
    try:
        for rep in range(repeats):
            before = counter() if counter else 0
            t0 = time.perf_counter()
            if profile_first and rep == 0:
                got = []
                prof = wh.profile(lambda: got.append(run(wh)))
                res = got[0]
                for label, ms in prof.items():
                    launches[label] = launches.get(label, 0) + len(ms)
            else:
                res = run(wh)
            torch.cuda.synchronize()
            seconds.append(time.perf_counter() - t0)
            results.append(res)
            if counter:
                poisoned.append(counter() - before)
    finally:
        wh.close()
    return results, launches, seconds


def _differences(want, got):
    from backends import same_bits
    assert [n for n, _ in want] == [n for n, _ in got], "the passes returned different outputs"
    return [n for (n, a), (_, b) in zip(want, got) if not same_bits(a, b)]


def _no_poison_in(family, what, want, got):
    """finite wherever the product build's result is"""
    for (name, a), (_, b) in zip(want, got):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype.kind == "f":
            assert a.shape == b.shape and np.all(np.isfinite(b) | ~np.isfinite(a)), f"{family}: {what}, {name}: a NaN pattern reached the output"


def _launched(launches, claim):
    """a claim with template arguments names the profile label itself; a bare name any label of that kernel"""
    if "<" in claim:
        return any(label.strip("()") == claim for label in launches)
    return any(label == claim or _kernel_of(label) == claim for label in launches)


@gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_family_on_the_checked_builds(family):
    from world_amd.api import LIB_PATH
    run, kernels, kw = FAMILIES[family]
    (first, second), _, t_product = _run_family(LIB_PATH, run, kw, repeats=2)
    assert first, f"{family}: nothing to compare"
    _made.setdefault(("fresh", family), first)                # (test_families_share_one_context compares with it)
    bad = _differences(first, second)
    assert not bad, f"{family}: the product build is not deterministic in {bad[:8]}: the family cannot be judged"
    # routes: what the family claims was launched
    _, launches, _ = _run_family(LIB_PATH, run, kw, profile_first=True)
    missing = [k for k in kernels if k not in COLD_ONLY and not _launched(launches, k)]
    assert not missing, f"{family}: claims {missing}, launched {sorted(launches)}"
    # jitter: three passes, the stalls fall differently every time
    passes, cold, t_jitter = _run_family(_lib("jitter"), run, kw, repeats=3, profile_first=True)
    missing = [k for k in kernels if k in COLD_ONLY and not _launched(cold, k)]
    assert not missing, f"{family}: claims {missing}, the jitter build's first pass launched {sorted(cold)}"
    for rep, res in enumerate(passes):
        bad = _differences(first, res)
        assert not bad, f"{family}: jitter build, pass {rep}: {bad[:8]} differ from the product build's"
    # poison: no NaN pattern where the product build has a number, and the same bits
    (res,), _, t_poison = _run_family(_lib("poison"), run, kw)
    for (name, a), (_, b) in zip(first, res):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype.kind == "f":
            assert a.shape == b.shape and np.all(np.isfinite(b) | ~np.isfinite(a)), f"{family}: poison build, {name}: a NaN pattern reached the output"
    bad = _differences(first, res)
    assert not bad, f"{family}: poison build: {bad[:8]} differ from the product build's"
    # hbm: two passes in one context, every carve refilled with 0xFF bytes -- the first over fresh allocations, the second over
    # the first's real leftovers.  No NaN where the product build has a number, the product's bits, and fills that happened
    filled = []
    passes, _, t_hbm = _run_family(_lib("hbm"), run, kw, repeats=2, poisoned=filled)
    for rep, res in enumerate(passes):
        _no_poison_in(family, f"hbm build, pass {rep}", first, res)
        bad = _differences(first, res)
        assert not bad, f"{family}: hbm build, pass {rep}: {bad[:8]} differ from the product build's"
    assert len(filled) == 2 and filled[0] > 0 and (filled[1] > 0 or family in NO_WORKSPACE), \
        f"{family}: hbm build: the poison counter rose by {filled} bytes over the two passes"
    print(f"{family}: product {min(t_product):.2f} s, jitter {max(t_jitter):.2f} s a pass, poison {t_poison[0]:.2f} s, "
          f"hbm {max(t_hbm):.2f} s a pass ({max(filled) / 2 ** 20:.1f} MiB filled); {len(first)} outputs, {sum(launches.values())} launches")


def _fresh(family):
    """the family's result in a fresh context of the product library, computed once per process"""
    from world_amd.api import LIB_PATH
    run, _, kw = FAMILIES[family]
    return _once(("fresh", family), lambda: _run_family(LIB_PATH, run, kw)[0][0])


@gpu
@pytest.mark.parametrize("build", ["product", "hbm"])
def test_families_share_one_context(build):
    """Every family whose WorldHip takes no keyword arguments, in ONE context: in table order, then in reverse order, so that
    every stage meets the leftovers of another feature's calls -- MLPG's 1- and 2-frame utterances carve where a long Harvest arena lay, the
    drop-in slots and the cached tables are whatever the families before left -- and must still compute its fresh-context
    result.  On the product library this is the only test where a stage reads behind REAL foreign leftovers; on the hbm
    library the same sequence runs with every carve refilled.  (shared-device keeps a context of its own: its hint is a
    property of the context.)"""
    import torch
    from world_amd.api import LIB_PATH
    names = [f for f, (_, _, kw) in FAMILIES.items() if not kw]
    assert len(names) == len(FAMILIES) - 1 and "shared-device" not in names
    want = {f: _fresh(f) for f in names}
    wh = _open(LIB_PATH if build == "product" else _lib(build), {})
    counter = _poison_counter(wh.lib) if build == "hbm" else None
    t0 = time.perf_counter()
    try:
        for order, sequence in (("table order", names), ("reverse order", names[::-1])):
            before = counter() if counter else 0
            for f in sequence:
                res = FAMILIES[f][0](wh)
                torch.cuda.synchronize()
                if build == "hbm":
                    _no_poison_in(f, f"{build} build, shared context, {order}", want[f], res)
                bad = _differences(want[f], res)
                assert not bad, f"{f}: {build} build, shared context, {order}: {bad[:8]} differ from the fresh context's"
            assert counter is None or counter() > before, f"hbm build, shared context, {order}: the poison counter did not rise"
    finally:
        wh.close()
    print(f"shared context, {build}: {len(names)} families twice in {time.perf_counter() - t0:.2f} s")
