"""Parameter modification and one-call resynthesis on the MI355X (include/world_hip.h: world_hip_modify_batch,
world_hip_resynthesize_batch): against the reference's own test program, the NumPy statement of test_modify_cpu.py and
the separate library calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from backends import ROOT, read_wav, wh, write_wav  # noqa: F401 (wh: a fixture)
from test_modify_cpu import envelope, log_f0_stats, map_f0, rel, warp_rows
from util import load_golden

pytestmark = pytest.mark.gpu

REF_DIR = os.path.join(ROOT, "oracle", "_ref")


@pytest.mark.parametrize("args", [("1.5", "1.2"), ("0.7", "0.85"), ("2.0",)])
def test_reference_test_program_end_to_end(wh, tmp_path, args):
    """oracle/_ref/test_ref (the reference's test.cpp, unmodified) with its F0 / formant arguments against resynthesize()
    of the same WAV, both quantised to 16 bits: the drop-in test's bar (<= 1 LSB, < 1e-3 of the samples differ)"""
    import torch
    exe = os.path.join(REF_DIR, "test_ref")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/test_ref was not prebuilt (needs the reference tree at build time)")
    g = load_golden("vaiueo2d_harvest")
    src = tmp_path / "in.wav"
    write_wav(src, g["q"], g["fs"])
    r = subprocess.run([exe, str(src), "out.wav", *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "complete." in r.stdout, r.stdout + r.stderr
    want, fs = read_wav(tmp_path / "01out.wav")
    x = torch.from_numpy(g["x"]).to(wh.device)[None].contiguous()
    ratio = float(args[1]) if len(args) > 1 else 1.0
    y, yl = wh.resynthesize(x, fs, f0_scale=float(args[0]), formant_shift=ratio, f0_floor=40.0)
    got = wh.double_to_pcm16(y[0, :int(yl[0])]).cpu().numpy().astype(np.int32)
    assert got.shape == want.shape and want.size > 0
    diff = np.abs(got - want)
    assert diff.max() <= 1, f"max sample difference {diff.max()} LSB"
    assert np.mean(diff > 0) < 1e-3


@pytest.mark.parametrize("fs", [16000, 24000, 48000, 96000, 192000])
def test_modify_against_the_host_statement(wh, fs):
    import torch
    from world_amd.api import cheaptrick_fft_size
    fft = cheaptrick_fft_size(fs, 71.0)
    nb = fft // 2 + 1
    ratios = [0.5, 0.8, 1.25, 2.0, 0.87, 1.13, 1.0]
    scales = [1.0, 1.5, 0.7, 2.0, 1.0, 0.5, 1.2]
    nf = np.array([40, 13, 37, 1, 26, 40, 24], dtype=np.int32)
    B, F = len(ratios), int(nf.max())
    sp = np.full((B, F, nb), np.nan)
    f0 = np.full((B, F), np.nan)
    rng = np.random.default_rng(fs)
    for u in range(B):
        sp[u, :nf[u]] = envelope(fs, fft, int(nf[u]), seed=u)
        f0[u, :nf[u]] = np.where(rng.random(nf[u]) < 0.3, 0.0, rng.uniform(70, 400, nf[u]))
    d_sp, d_f0 = torch.from_numpy(sp).cuda(), torch.from_numpy(f0).cuda()
    f0_o, sp_o = wh.modify(d_f0, d_sp, nf, fs, fft, f0_scale=scales, formant_shift=ratios)
    got_sp, got_f0 = sp_o.cpu().numpy(), f0_o.cpu().numpy()
    for u in range(B):
        n = nf[u]
        assert rel(got_sp[u, :n], warp_rows(sp[u, :n], ratios[u], fs, fft)) <= 1e-13, (fs, ratios[u])
        if ratios[u] == 1.0:
            assert np.array_equal(got_sp[u, :n], sp[u, :n])
        assert np.array_equal(got_f0[u, :n], f0[u, :n] * scales[u])
        assert np.all(np.isnan(got_sp[u, n:])) and np.all(np.isnan(got_f0[u, n:]))
    # in place gives the same bits
    f0_i, sp_i = wh.modify(d_f0, d_sp, nf, fs, fft, f0_scale=scales, formant_shift=ratios, out="inplace")
    assert sp_i.data_ptr() == d_sp.data_ptr()
    assert torch.equal(torch.nan_to_num(sp_i, 7.0), torch.nan_to_num(sp_o, 7.0))
    assert torch.equal(torch.nan_to_num(f0_i, 7.0), torch.nan_to_num(f0_o, 7.0))


def test_log_f0_statistics_and_conversion(wh):
    import torch
    rng = np.random.default_rng(3)
    F = 2001
    f0 = np.exp(rng.normal(5.0, 0.25, (4, F)))
    f0[rng.random((4, F)) < 0.35] = 0.0
    f0[1] = 0.0                                                   # no voiced frame
    f0[2] = 0.0; f0[2, 100] = 150.0                               # one
    f0[3, ::3] = 240.0; f0[3, 1::3] = 240.0; f0[3, 2::3] = 0.0    # constant
    nf = np.array([F, F, 1500, F], dtype=np.int32)
    d = torch.from_numpy(f0).cuda()
    stats = wh.f0_statistics(d, nf).cpu().numpy()
    for u in range(4):
        want = log_f0_stats(f0[u, :nf[u]])
        assert stats[u, 0] == want[0]
        assert abs(stats[u, 1] - want[1]) <= 1e-12 * max(1.0, abs(want[1]))
        assert abs(stats[u, 2] - want[2]) <= 1e-12 * max(1.0, abs(want[2]))
    assert stats[3, 2] == 0.0
    target = ([5.3, 5.0, 4.0, 5.1], [0.15, 0.2, 0.1, 0.3])
    got, _ = wh.modify(d, None, nf, 16000, 1024, f0_scale=1.1, log_f0_target=target)
    got = got.cpu().numpy()
    for u in range(4):
        want = map_f0(f0[u, :nf[u]], 1.1, (target[0][u], target[1][u]))
        g = got[u, :nf[u]]
        assert np.array_equal(g == 0, want == 0)
        v = want != 0
        assert rel(g[v], want[v]) <= 1e-12


def _vowels(fs, seconds, seeds):
    import torch
    from world_amd import synth
    xs = [synth.vowel(fs, s, seed=k) for s, k in zip(seconds, seeds)]
    x = torch.zeros((len(xs), max(v.numel() for v in xs)), dtype=torch.float64)
    for u, v in enumerate(xs):
        x[u, :v.numel()] = v
    return x.cuda(), np.array([v.numel() for v in xs], dtype=np.int32)


@pytest.mark.parametrize("time_scale", [1.0, 0.5, 2.0])
def test_resynthesize_is_analyze_modify_synthesis(wh, time_scale):
    """bit for bit the three calls on the same context; and within the synthesis bar of the CPU oracle chain"""
    import torch
    from oracle.loader import best_oracle
    fs = 24000
    x, xl = _vowels(fs, (0.6, 0.45, 0.7), (3, 8, 21))
    scales, ratios = [1.5, 0.8, 1.0], [1.2, 0.85, 1.0]
    y, yl = wh.resynthesize(x, fs, x_len=xl, f0_scale=scales, formant_shift=ratios, time_scale=time_scale)
    tpos, f0, sp, ap, nf = wh.analyze(x, fs, x_len=xl)
    fft = sp.shape[-1] * 2 - 2
    f0m, spm = wh.modify(f0, sp, nf, fs, fft, f0_scale=scales, formant_shift=ratios)
    y2 = wh.synthesis(f0m, spm, ap, nf, fft, 5.0 * time_scale, fs, yl)
    for u in range(3):
        assert torch.equal(y[u, :yl[u]], y2[u, :yl[u]]), u
    o = best_oracle()
    xn = x.cpu().numpy()
    for u in range(3):
        xu = xn[u, :xl[u]]
        tp_o, f0_o = o.harvest(xu, fs)
        sp_o = o.cheaptrick(xu, fs, tp_o, f0_o, fft_size=fft)
        ap_o = o.d4c(xu, fs, tp_o, f0_o, fft)
        y_o = o.synthesis(f0_o * scales[u], warp_rows(sp_o, ratios[u], fs, fft), ap_o, fft, 5.0 * time_scale, fs, int(yl[u]))
        got = y[u, :yl[u]].cpu().numpy()
        assert np.max(np.abs(got - y_o)) <= 1e-6 * np.max(np.abs(y_o)), u


def test_capture_replay_and_stale_graph():
    """the one call captured into a HIP graph (on a stream of its own) replays bit for bit; after a larger batch has
    grown the context's workspace the graph is refused as stale"""
    import torch
    from world_amd.api import WorldHip
    fs = 16000
    wh = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            x, xl = _vowels(fs, (0.5, 0.35), (4, 9))
            y, yl = wh.resynthesize(x, fs, x_len=xl, f0_scale=1.3, formant_shift=0.9, time_scale=1.5)
            want = y.clone()
            out = torch.zeros_like(y)
            _captured(wh, x, fs, xl, out)                # (the shape has run: nothing left to allocate or upload)
            torch.cuda.synchronize()
            g = wh.capture(lambda: _captured(wh, x, fs, xl, out))
            for _ in range(2):
                out.fill_(-3.0)
                g.launch()
                torch.cuda.synchronize()
                for u in range(2):                       # (samples beyond an utterance's y_length are the caller's)
                    assert torch.equal(out[u, :yl[u]], want[u, :yl[u]])
                    assert bool((out[u, yl[u]:] == -3.0).all())
            before = wh.workspace_bytes()
            big, bl = _vowels(fs, (1.6, 1.2, 1.5, 1.1), (1, 2, 3, 5))    # a larger batch grows the workspace
            wh.resynthesize(big, fs, x_len=bl, f0_scale=1.3)
            torch.cuda.synchronize()
            assert wh.workspace_bytes() > before
            with pytest.raises(RuntimeError, match="stale graph"):
                g.launch()
    finally:
        if g is not None:
            g.close()
        wh.close()


def _captured(wh, x, fs, xl, out):
    """the library call alone (resynthesize()'s pulse check synchronises, which a capture may not do)"""
    import ctypes as C
    from world_amd.api import CheapTrickOption, D4COption, HarvestOption, cheaptrick_fft_size, frame_count, modifications
    B, L = x.shape
    yl = np.array([wh.resynthesis_length(fs, frame_count(fs, int(n), 5.0), 5.0, 1.5) for n in xl], dtype=np.int32)
    hopt, copt, dopt = HarvestOption(71.0, 800.0, 5.0), CheapTrickOption(-0.15, 71.0, cheaptrick_fft_size(fs)), D4COption(0.85)
    wh._check(wh.lib.world_hip_resynthesize_batch(wh._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(C.POINTER(C.c_int)),
                                                  C.byref(hopt), C.byref(copt), C.byref(dopt), modifications(B, 1.3, 0.9),
                                                  1.5, yl.ctypes.data_as(C.POINTER(C.c_int)), out.shape[1], out.data_ptr()),
              "resynthesize")


def test_raised_f0_beyond_the_default_pulse_capacity(wh):
    """f0 * 12 needs more pulses than the default capacity (a mean of 1200 Hz): resynthesize() repeats the call at the
    capacity the device asked for and returns what a call with that capacity set up front returns"""
    import torch
    fs = 16000
    x, xl = _vowels(fs, (0.5,), (6,))
    y, yl = wh.resynthesize(x, fs, x_len=xl, f0_scale=12.0)
    wh.set_synthesis_pulse_capacity(int(yl[0]) // 4)
    try:
        y2, _ = wh.resynthesize(x, fs, x_len=xl, f0_scale=12.0)
    finally:
        wh.set_synthesis_pulse_capacity(0)
    assert torch.equal(y, y2)
    # and the pulses really exceeded the default
    tpos, f0, sp, ap, nf = wh.analyze(x, fs, x_len=xl)
    f0s = f0[0, :nf[0]].cpu().numpy() * 12.0
    assert float(np.mean(np.where(f0s > 0, f0s, 500.0))) > 1200.0


def test_transform_tool_writes_what_the_python_path_computes(wh, tmp_path):
    import torch
    from world_amd import synth
    fs = 16000
    paths = []
    for k, sec in enumerate((0.4, 0.3)):
        q = np.round(synth.vowel(fs, sec, seed=30 + k).numpy() * 32768).clip(-32768, 32767).astype(np.int16)
        p = tmp_path / f"in{k}.wav"
        write_wav(p, q, fs)
        paths.append(str(p))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "world_amd.tools", "transform", *paths, "--outdir", str(out),
                        "--f0-scale", "1.4", "--formant-shift", "1.1", "--time-scale", "1.3"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for p in paths:
        x, fs_ = wh.wavread(p)
        y, yl = wh.resynthesize(x[None].contiguous(), fs_, f0_scale=1.4, formant_shift=1.1, time_scale=1.3)
        want = wh.double_to_pcm16(y[0, :int(yl[0])]).cpu().numpy().astype(np.int32)
        got, fs2 = read_wav(out / os.path.basename(p))
        assert fs2 == fs and np.array_equal(got, want)
