"""Frame-wise modification behind a time map on the MI355X (include/world_hip.h: world_hip_modify_frames_batch,
world_hip_resynthesize_frames_batch): the cases of test_modify_frames_cpu.py through the shipped library, batch
independence and graph replay, and the reference's own programs (oracle/_ref) as the yardstick."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_modify_frames_cpu as cpu
from backends import ROOT, OnGpu, gpu_backend, read_wav, wh, write_wav  # noqa: F401 (wh: a fixture)
from util import load_golden

pytestmark = pytest.mark.gpu

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
_ip = C.POINTER(C.c_int)


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


RATES = [48000, 192000]


@pytest.mark.parametrize("fs", RATES)
def test_identity_map_and_constant_curves_equal_modify_batch(be, fs):
    cpu.case_identity_map_and_constant_curves(be, fs)


@pytest.mark.parametrize("fs", RATES)
def test_integer_map_is_a_gather_of_modify_batch(be, fs):
    cpu.case_integer_map_is_a_gather(be, fs)


@pytest.mark.parametrize("fs", RATES)
def test_blend_only_is_bit_identical_to_the_statement(be, fs):
    cpu.case_blend_only(be, fs)


@pytest.mark.parametrize("fs", RATES)
def test_blend_and_per_frame_warp(be, fs):
    cpu.case_blend_and_per_frame_warp(be, fs)


@pytest.mark.parametrize("fs,fft", cpu.OFF_DEFAULT)
def test_identity_map_and_constant_curves_off_default_fft(be, fs, fft):
    cpu.case_identity_map_and_constant_curves(be, fs, fft)


@pytest.mark.parametrize("fs,fft", cpu.OFF_DEFAULT)
def test_blend_and_per_frame_warp_off_default_fft(be, fs, fft):
    cpu.case_blend_and_per_frame_warp(be, fs, fft)


@pytest.mark.parametrize("fs", RATES)
def test_padding_refusals_and_invalid_curve_values(be, fs):
    cpu.case_padding_and_refusals(be, fs)


# ---- batch independence, graph replay ------------------------------------------------------------------------------------
def _curved_batch(fs, fft, seed):
    rng = np.random.default_rng(seed)
    nf = np.array([30, 17, 44, 9], dtype=np.int32)
    f0, sp, ap = cpu.ragged(fs, fft, nf, seed=seed)
    no = np.array([45, 12, 44, 20], dtype=np.int32)
    O = int(no.max())
    curves = dict(time_map=np.stack([np.concatenate([np.linspace(0, nf[u] - 1, no[u]), np.zeros(O - no[u])]) for u in range(4)]),
                  f0_target=np.where(rng.random((4, O)) < 0.5, rng.uniform(80, 300, (4, O)), 0.0),
                  f0_scale=rng.uniform(0.5, 2.0, (4, O)), formant_shift=rng.uniform(0.7, 1.4, (4, O)),
                  ap_gain=rng.uniform(0.5, 1.5, (4, O)))
    target = ([5.3, 5.0, 4.8, 5.1], [0.15, 0.2, 0.1, 0.3])
    return nf, no, O, f0, sp, ap, curves, target


def test_an_utterance_alone_and_inside_a_batch(be):
    fs = 48000
    fft = cpu.fft_of(fs)
    nf, no, O, f0, sp, ap, curves, target = _curved_batch(fs, fft, 3)
    rc, b_f0, b_sp, b_ap = be.frames(fs, fft, nf, no, O, cpu.mods_of(4, 1.0, 1.0, target), f0=f0, sp=sp, ap=ap, **curves)
    assert rc == 0, be.error()
    for u in range(4):
        one = slice(u, u + 1)
        rc, a_f0, a_sp, a_ap = be.frames(fs, fft, nf[one], no[one], O, cpu.mods_of(1, 1.0, 1.0, (target[0][one], target[1][one])),
                                         f0=f0[one], sp=sp[one], ap=ap[one], **{k: v[one] for k, v in curves.items()})
        assert rc == 0, be.error()
        n = no[u]
        assert np.array_equal(a_f0[0, :n], b_f0[u, :n]) and np.array_equal(a_sp[0, :n], b_sp[u, :n])
        assert np.array_equal(a_ap[0, :n], b_ap[u, :n])


def test_graph_replay_gives_the_same_bits():
    """the call captured into a HIP graph (on a stream of its own) replays bit for bit: nothing is copied from the host"""
    import torch
    from world_amd.api import WorldHip, WorldHipFrameCurves
    fs = 48000
    fft = cpu.fft_of(fs)
    nf, no, O, f0, sp, ap, curves, target = _curved_batch(fs, fft, 8)
    wh = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            d = {k: torch.from_numpy(v).cuda() for k, v in dict(f0=f0, sp=sp, ap=ap, **curves).items()}
            outs = [torch.full((4, O) + tuple(d[k].shape[2:]), -3.0, dtype=torch.float64, device="cuda") for k in ("f0", "sp", "ap")]
            cv = WorldHipFrameCurves(**{"d_" + k: d[k].data_ptr() for k in curves})
            mods = cpu.mods_of(4, 1.0, 1.0, target)

            def call():
                wh._check(wh.lib.world_hip_modify_frames_batch(
                    wh._context(), 4, fs, fft, nf.ctypes.data_as(_ip), f0.shape[1], no.ctypes.data_as(_ip), O, mods, C.byref(cv),
                    d["f0"].data_ptr(), outs[0].data_ptr(), d["sp"].data_ptr(), outs[1].data_ptr(), d["ap"].data_ptr(),
                    outs[2].data_ptr()), "modify_frames")
            call()
            torch.cuda.synchronize()
            want = [o.clone() for o in outs]
            g = wh.capture(call)
            for _ in range(2):
                for o in outs:
                    o.fill_(-3.0)
                g.launch()
                torch.cuda.synchronize()
                for o, w in zip(outs, want):
                    assert torch.equal(o, w)
                for u in range(4):
                    assert bool((outs[1][u, no[u]:] == -3.0).all())
    finally:
        if g is not None:
            g.close()
        wh.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_python_layer_validates_and_matches_the_c_call(wh, be):
    import torch
    from world_amd.api import uniform_time_map
    fs = 48000
    fft = cpu.fft_of(fs)
    nf = np.array([20, 20], dtype=np.int32)
    f0, sp, ap = cpu.ragged(fs, fft, nf, seed=9)
    O = 30
    tm = uniform_time_map(20, O, device=wh.device)
    shift = torch.linspace(0.9, 1.2, O, dtype=torch.float64, device=wh.device)
    d = [torch.from_numpy(a).cuda() for a in (f0, sp, ap)]
    g_f0, g_sp, g_ap = wh.modify_frames(*d, nf, fs, fft, time_map=tm, formant_shift=shift, f0_scale=[1.5, 0.8])
    host = lambda t: np.tile(t.cpu().numpy(), (2, 1))
    rc, w_f0, w_sp, w_ap = be.frames(fs, fft, nf, O, O, cpu.mods_of(2, [1.5, 0.8]), f0=f0, sp=sp, ap=ap, time_map=host(tm),
                                     formant_shift=host(shift))
    assert rc == 0, be.error()
    for got, want in ((g_f0, w_f0), (g_sp, w_sp), (g_ap, w_ap)):
        assert np.array_equal(got.cpu().numpy(), want)
    for name, value in (("formant_shift", 0.0), ("formant_shift", float("nan")), ("f0_scale", -1.0), ("ap_gain", float("inf")),
                        ("time_map", float("nan"))):
        curve = torch.ones(O, dtype=torch.float64, device=wh.device)
        curve[7] = value
        kw = {"time_map": tm, name: curve}
        with pytest.raises(ValueError):
            wh.modify_frames(*d, nf, fs, fft, **kw)
        kw["n_out"] = 7                                                     # (the bad value lies beyond the frames in use)
        wh.modify_frames(*d, nf, fs, fft, **kw)


# ---- against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [("1.5", "1.2"), ("0.7", "0.85"), ("2.0",)])
def test_constant_curves_reproduce_the_reference_test_program(wh, tmp_path, args):
    """oracle/_ref/test_ref (the reference's test.cpp, unmodified) with its F0 / formant arguments against
    resynthesize_frames() with an identity map and the same constants as curves, both quantised to 16 bits: the bar
    tests/test_modify_gpu.py holds resynthesize() to (<= 1 LSB, < 1e-3 of the samples differ)"""
    import torch
    from world_amd.api import frame_count
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
    n = frame_count(fs, x.shape[1], 5.0)
    const = lambda v: torch.full((n,), float(v), dtype=torch.float64, device=wh.device)
    y, yl = wh.resynthesize_frames(x, fs, time_map=torch.arange(n, dtype=torch.float64, device=wh.device),
                                   f0_scale=const(args[0]), formant_shift=const(args[1] if len(args) > 1 else 1.0),
                                   f0_floor=40.0)
    got = wh.double_to_pcm16(y[0, :int(yl[0])]).cpu().numpy().astype(np.int32)
    assert got.shape == want.shape and want.size > 0
    diff = np.abs(got - want)
    print(f"args {args}: max {diff.max()} LSB, {np.mean(diff > 0):.3e} of the samples differ")
    assert diff.max() <= 1, f"max sample difference {diff.max()} LSB"
    assert np.mean(diff > 0) < 1e-3


@pytest.mark.parametrize("which", ["s = 2 j", "s = j / 2"])
def test_retimed_resynthesis_against_the_reference_synthesis(wh, which):
    """resynthesize_frames() with s_j = 2 j and s_j = j / 2 against the reference's Synthesis fed the same analysis retimed
    in NumPy (at these maps every blend is exact in binary): the bar tests/test_synthesis.py holds the GPU Synthesis to
    against the reference, 1e-8 of the peak"""
    import torch
    from oracle.loader import best_oracle
    from world_amd import synth
    fs = 48000
    fft = cpu.fft_of(fs)
    x = synth.vowel(fs, 0.5, seed=17).cuda()[None].contiguous()
    tpos, f0, sp, ap, nf = wh.analyze(x, fs)
    n = int(nf[0])
    n_out = (n + 1) // 2 if which == "s = 2 j" else 2 * n - 1
    s = np.arange(n_out) * (2.0 if which == "s = 2 j" else 0.5)
    y, yl = wh.resynthesize_frames(x, fs, time_map=torch.from_numpy(s).cuda())
    f0_r, sp_r, ap_r, _ = cpu.statement(f0[0, :n].cpu().numpy(), sp[0, :n].cpu().numpy(), ap[0, :n].cpu().numpy(), n_out, fs,
                                        fft, time_map=s)
    want = best_oracle().synthesis(f0_r, sp_r, ap_r, fft, 5.0, fs, int(yl[0]))
    got = y[0, :int(yl[0])].cpu().numpy()
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"{which}: {n} -> {n_out} frames, {int(yl[0])} samples, error {err:.3e} of the peak")
    assert np.max(np.abs(want)) > 1e-3
    assert np.max(np.abs(got - want)) <= 1e-8 * np.max(np.abs(want))


def test_transform_tool_duration_and_f0_from(wh, tmp_path):
    """python -m world_amd.tools transform --duration / --f0-from writes what the Python path computes"""
    import torch
    from world_amd import synth
    from world_amd.api import FileAPI, frame_count, uniform_time_map
    fs = 16000
    q = np.round(synth.vowel(fs, 0.4, seed=31).numpy() * 32768).clip(-32768, 32767).astype(np.int16)
    src = tmp_path / "in.wav"
    write_wav(src, q, fs)
    x, _ = wh.wavread(str(src))
    n = frame_count(fs, x.numel(), 5.0)
    track = np.where(np.arange(25) % 5 == 4, 0.0, np.linspace(120.0, 260.0, 25))
    FileAPI().write_f0(str(tmp_path / "tune.f0"), 5.0, np.arange(25) * 0.005, track)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "world_amd.tools", "transform", str(src), "--outdir", str(out), "--duration", "0.6",
                        "--f0-from", str(tmp_path / "tune.f0"), "--formant-shift", "1.1"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n_out = int(0.6 * 1000.0 / 5.0) + 1
    target = cpu.statement(track, None, None, n_out, fs, 0, time_map=uniform_time_map(25, n_out, device="cpu").numpy())[0]
    y, yl = wh.resynthesize_frames(x[None].contiguous(), fs, time_map=uniform_time_map(n, n_out, device=wh.device),
                                   f0_target=torch.from_numpy(target).cuda(), formant_shift=1.1)
    want = wh.double_to_pcm16(y[0, :int(yl[0])]).cpu().numpy().astype(np.int32)
    got, fs2 = read_wav(out / "in.wav")
    assert fs2 == fs and np.array_equal(got, want)
    assert abs(len(got) / fs - 0.6) <= 0.005
