"""Synthesis straight from records on the MI355X (include/world_hip.h: world_hip_synthesis_records,
world_hip_realtime_add_coded): the cases of test_synthesis_records_cpu.py through the shipped library -- the reference's
own decoders and Synthesis (oracle/_ref) as the yardstick where they were built, the port otherwise -- graph replay and the
command-line tool."""
import subprocess
import sys
import wave

import numpy as np
import pytest

import test_synthesis_records_cpu as cpu
from backends import ROOT, OnGpu, gpu_backend, wh  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


@pytest.fixture(scope="module")
def ref():
    from oracle.loader import best_oracle
    return best_oracle()


@pytest.mark.parametrize("fs,fft,ndim", cpu.SHAPES)
def test_coded_records_equal_decode_then_synthesis_and_the_reference(be, port_oracle, ref, fs, fft, ndim):
    cpu.case_coded_records(be, port_oracle, ref, fs, fft, ndim)


@pytest.mark.parametrize("wire", [0, 1])
@pytest.mark.parametrize("fs,fft,ndim", cpu.SHAPES)
def test_f64_and_f32_records_equal_unpack_then_synthesis(be, port_oracle, fs, fft, ndim, wire):
    cpu.case_plain_records(be, port_oracle, fs, fft, wire)


@pytest.mark.parametrize("name,fs,fft,ndim", cpu.GOLDEN_ROWS)
def test_recorded_coded_rows_equal_decode_then_synthesis(be, name, fs, fft, ndim):
    cpu.case_golden_rows(be, name, fs, fft, ndim)


def test_refusals_leave_the_context_as_new(be, port_oracle):
    cpu.case_refusals(be, port_oracle)


def test_pulse_capacity_is_that_of_synthesis_batch(be, port_oracle):
    cpu.case_pulse_capacity(be, port_oracle)


def test_realtime_add_coded_equals_decode_then_add(be, port_oracle):
    cpu.case_realtime(be, port_oracle)


def test_python_layer_matches_the_c_call(wh, be, port_oracle):
    import torch
    fs, fft, ndim = 48000, 2048, 60
    c = cpu.case_of(port_oracle, fs, fft, ndim)
    yl = cpu.y_lengths(fs, cpu.N_FRAMES)
    for wire in (0, 1, 2):
        rc, want = be.records(fs, fft, cpu.N_FRAMES, c["blocks"][wire], wire, ndim)
        assert rc == 0, be.error()
        got = wh.synthesize_records(torch.from_numpy(c["blocks"][wire]).cuda(), cpu.N_FRAMES, fs, fft, cpu.FP, yl, wire=wire,
                                    number_of_dimensions=ndim, first_row=cpu.FIRST_ROW)
        assert np.array_equal(got.cpu().numpy(), want)


def test_graph_replay_gives_the_same_bits_and_reads_the_block_anew(port_oracle):
    """condition 3: a captured call replays to the bits of the eager one; after the coded values in the same block were
    overwritten in place, a replay yields the new values' waveform"""
    import torch
    from world_amd.api import WorldHip
    fs, fft, ndim = 48000, 2048, 60
    c = cpu.case_of(port_oracle, fs, fft, ndim)
    nf, yl = cpu.N_FRAMES, cpu.y_lengths(fs, cpu.N_FRAMES)
    Y = int(yl.max())
    other = c["blocks"][2].copy()
    lo = cpu.FIRST_ROW
    other[lo:lo + 61, 2:] = c["blocks"][2][lo:lo + 61, 2:][::-1]         # utterance 0's frames in reverse order
    wh = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            block = torch.from_numpy(c["blocks"][2]).cuda()
            y = torch.zeros((3, Y), dtype=torch.float64, device="cuda")

            def call():
                wh._check(wh.lib.world_hip_synthesis_records(wh._context(), 3, fs, cpu.FP, fft, cpu.ip(nf), lo, block.data_ptr(),
                                                             block.shape[1], 2, ndim, cpu.ip(yl), Y, y.data_ptr()), "records")
            call()
            torch.cuda.synchronize()
            want = y.clone()
            g = wh.capture(call)
            y.zero_()
            g.launch()
            torch.cuda.synchronize()
            assert torch.equal(y, want)
            block.copy_(torch.from_numpy(other).cuda())
            call()
            torch.cuda.synchronize()
            want2 = y.clone()
            assert not torch.equal(want2, want)
            y.zero_()
            g.launch()
            torch.cuda.synchronize()
            assert torch.equal(y, want2)
    finally:
        if g is not None:
            g.close()
        wh.close()


def test_synthesis_tool_takes_the_records_route_for_coded_files(wh, tmp_path):
    """condition 7: analysis --code-sp 60 --code-ap, then synthesis, writes the bytes of the route through the Python
    decode calls"""
    import torch
    from world_amd import synth
    from world_amd.api import FileAPI
    fs = 16000
    q = np.round(synth.vowel(fs, 0.3, seed=5).numpy() * 32768).clip(-32768, 32767).astype(np.int16)
    with wave.open(str(tmp_path / "in.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(q.astype("<i2").tobytes())
    run = lambda *a: subprocess.run([sys.executable, "-m", "world_amd.tools", *a], cwd=ROOT, capture_output=True, text=True, timeout=300)
    r = run("analysis", str(tmp_path / "in.wav"), "--outdir", str(tmp_path), "--code-sp", "60", "--code-ap")
    assert r.returncode == 0, r.stdout + r.stderr
    stem = str(tmp_path / "in")
    r = run("synthesis", stem + ".f0", stem + ".sp", stem + ".ap", "-o", str(tmp_path / "got.wav"))
    assert r.returncode == 0, r.stdout + r.stderr
    files = FileAPI()
    fft, fp = int(files.header(stem + ".sp", "FFT ")), files.header(stem + ".sp", "FP  ")
    assert int(files.header(stem + ".sp", "NOD ")) == 60 and int(files.header(stem + ".ap", "NOD ")) > 0
    f0 = torch.from_numpy(files.read_f0(stem + ".f0")[1]).to(wh.device)[None]
    sp = wh.decode_spectral_envelope(torch.from_numpy(files.read_spectral_envelope(stem + ".sp")).to(wh.device)[None], fs, fft)
    ap = wh.decode_aperiodicity(torch.from_numpy(files.read_aperiodicity(stem + ".ap")).to(wh.device)[None], fs, fft)
    n = f0.shape[1]
    y_length = int(n * fp / 1000.0 * fs)
    y = wh.synthesis(f0, sp, ap, np.array([n], dtype=np.int32), fft, fp, fs, np.array([y_length], dtype=np.int32))
    wh.wavwrite(str(tmp_path / "want.wav"), y[0, :y_length], fs)
    got, want = open(tmp_path / "got.wav", "rb").read(), open(tmp_path / "want.wav", "rb").read()
    assert len(want) > 44 + 2 * 1000 and got == want
