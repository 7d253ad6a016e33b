"""Sampling-rate conversion on the MI355X (include/world_hip.h: world_hip_resample_batch): the cases of
test_resample_cpu.py through the shipped library, graph replay, the Python layer, and the tools' --fs / `resample`."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import test_resample_cpu as cpu
from backends import ROOT, OnGpu, gpu_backend, pcm16, read_wav, wh, write_wav  # noqa: F401 (wh: a fixture)
from util import utterance

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


# ---- the cases of the CPU file -------------------------------------------------------------------------------------------
def test_lengths_and_shapes(wh):
    cpu.case_lengths_and_shapes(wh.lib)


def test_host_arithmetic_refusals_write_nothing(wh):
    cpu.case_host_refusals(wh.lib)


def test_batch_refusals_write_nothing(be):
    cpu.case_batch_refusals(be)


@pytest.mark.parametrize("fs_in,fs_out,design", cpu.DESIGNS, ids=cpu.DESIGN_IDS)
def test_table_against_the_statement(wh, fs_in, fs_out, design):
    cpu.case_table(wh.lib, fs_in, fs_out, design)


@pytest.mark.parametrize("fs_in,fs_out,design", cpu.DESIGNS + [cpu.STEEP], ids=cpu.DESIGN_IDS + ["48000-1000-steep"])
def test_sum_bit_for_bit(be, fs_in, fs_out, design):
    cpu.case_sum(be, fs_in, fs_out, design)


def test_null_option_is_best(be):
    cpu.case_null_option_is_best(be)


def test_equal_rates_copy_bit_for_bit(be):
    cpu.case_equal_rates_copy(be)


def test_a_row_alone_in_a_batch_permuted_and_behind_other_ratios(be):
    cpu.case_independence(be)


def test_table_cache_turns_over(be):
    cpu.case_table_cache_turns_over(be)


@pytest.mark.parametrize("fs_in,fs_out,design", [(44100, 48000, cpu.BEST), (192000, 16000, cpu.FAST)], ids=["44100-48000-best", "192000-16000-fast"])
def test_nan_and_inf_spread_as_the_sum_spreads_them(be, fs_in, fs_out, design):
    cpu.case_hostile(be, fs_in, fs_out, design)


@pytest.mark.parametrize("fs_in,fs_out,design", cpu.DESIGNS[:11], ids=cpu.DESIGN_IDS[:11])
def test_the_filter_does_its_job(be, fs_in, fs_out, design):
    cpu.case_filter(be, fs_in, fs_out, design)


# ---- graph replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs_in,fs_out,design", [(44100, 48000, cpu.BEST), (192000, 16000, cpu.FAST)], ids=["44100-48000-best", "192000-16000-fast"])
def test_graph_replay_reads_the_new_inputs(fs_in, fs_out, design):
    """after one eager call the call is captured; the inputs are overwritten and the graph replayed: the outputs are the
    statement's on the new inputs, bit for bit (nothing is copied from the host, nothing is baked in but addresses); a
    ratio that never ran cannot be captured"""
    import torch
    from world_amd.api import WorldHip
    rows = cpu.rows_for(fs_in, fs_out, design)
    rows2 = [np.ascontiguousarray(r[::-1]) * 0.5 for r in rows]
    n = [len(r) for r in rows]
    n_out = [cpu.out_length(k, fs_in, fs_out) for k in n]
    X, Y = max(n) + 3, max(n_out) + 4

    def stored(rs):
        x = np.full((len(rs), X), cpu.SENTINEL)
        for u, r in enumerate(rs):
            x[u, :len(r)] = r
        return x
    w = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            be = GpuBackend(w)
            d_x, d_y = be.dev(stored(rows)), be.dev(np.full((len(rows), Y), cpu.SENTINEL))
            call = lambda: w._check(be.call(len(rows), fs_in, fs_out, design, d_x, X, n, d_y, Y), "resample")
            with pytest.raises(RuntimeError, match="never run before"):
                w.capture(call)
            call()
            torch.cuda.synchronize()
            c = cpu.lib_table(w.lib, fs_in, fs_out, design)
            cpu.check_rows(be.host(d_y), n_out, rows, fs_in, fs_out, c)
            g = w.capture(call)
            d_x.copy_(torch.from_numpy(stored(rows2)))
            d_y.fill_(cpu.SENTINEL)
            g.launch()
            torch.cuda.synchronize()
            cpu.check_rows(be.host(d_y), n_out, rows2, fs_in, fs_out, c)
    finally:
        if g is not None:
            g.close()
        w.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_python_layer_matches_the_c_call_and_validates_quality(wh, be):
    import torch
    from world_amd.api import resample_length
    fs_in, fs_out = 44100, 16000
    rows = cpu.rows_for(fs_in, fs_out, cpu.FAST)[3:7]
    n = [len(r) for r in rows]
    x = torch.zeros((len(rows), max(n)), dtype=torch.float64, device="cuda")
    for u, r in enumerate(rows):
        x[u, :n[u]] = torch.from_numpy(r)
    for quality, design in (("fast", cpu.FAST), ("best", cpu.BEST), (cpu.CUSTOM, cpu.CUSTOM), (list(cpu.CUSTOM), cpu.CUSTOM)):
        y, y_len = wh.resample(x, fs_in, fs_out, x_len=n, quality=quality)
        assert list(y_len) == [resample_length(k, fs_in, fs_out) for k in n] and y.shape == (len(rows), max(y_len))
        n_out, want = be.resample(rows, fs_in, fs_out, design)
        got = y.cpu().numpy()
        for u in range(len(rows)):
            assert cpu.same_bits(got[u, :n_out[u]], want[u, :n_out[u]]) and np.all(got[u, n_out[u]:] == 0.0)
    y, y_len = wh.resample(x, fs_in, fs_in, x_len=n)                              # equal rates: a copy
    assert list(y_len) == n and torch.equal(y, x)
    whole, whole_len = wh.resample(x, fs_in, fs_out)                              # x_len=None: the rows as they are
    assert list(whole_len) == [resample_length(max(n), fs_in, fs_out)] * len(rows)
    for bad in ("good", "", 3, (4, 0.9), (4, 0.9, 5.0, 1.0), (4.5, 0.9, 5.0), None):
        with pytest.raises(ValueError):
            wh.resample(x, fs_in, fs_out, x_len=n, quality=bad)
    for bad in ((0, 0.9, 5.0), (4, 1.5, 5.0), (4, 0.9, 41.0)):                    # the library's refusals come through
        with pytest.raises(RuntimeError, match="resample"):
            wh.resample(x, fs_in, fs_out, x_len=n, quality=bad)
    with pytest.raises(ValueError):
        wh.resample(x, 0, fs_out)
    with pytest.raises(ValueError):
        resample_length(0, fs_in, fs_out)
    from world_amd.api import WorldHip
    w = WorldHip()                                                                # (its own context: an empty table cache)
    try:
        w.resample(x, fs_in, fs_out, x_len=n, quality="fast")
        before = w.workspace_bytes()
        w.resample(x, fs_in, fs_out, x_len=n, quality="fast")                     # found again: nothing new
        assert w.workspace_bytes() == before
        w.resample(x, 32000, 48000, x_len=n, quality=(5, 0.9, 5.0))               # L = 3, W = 5: 3 x (10 doubles + 1 int)
        assert w.workspace_bytes() - before == 3 * 84
    finally:
        w.close()


# ---- the tools -----------------------------------------------------------------------------------------------------------
def _tool(*args):
    return subprocess.run([sys.executable, "-m", "world_amd.tools", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_wavs")
    return {fs: write_wav(d / f"u{fs}.wav", pcm16(utterance(fs, seconds, index)), fs)
            for fs, seconds, index in ((48000, 0.30, 2), (44100, 0.36, 3), (8000, 0.30, 2))}


def test_resample_tool_writes_what_the_python_path_computes(wh, wavs, tmp_path):
    r = _tool("resample", wavs[48000], wavs[44100], "--outdir", str(tmp_path), "--fs", "16000")
    assert r.returncode == 0, r.stdout + r.stderr
    for fs in (48000, 44100):
        got, rate = read_wav(tmp_path / os.path.basename(wavs[fs]))
        x = wh.wavread(wavs[fs])[0]
        y, y_len = wh.resample(x[None].contiguous(), fs, 16000)
        want = wh.double_to_pcm16(y[0, :y_len[0]]).cpu().numpy().astype(np.int32)
        assert rate == 16000 and np.array_equal(got, want) and np.abs(got).max() > 0
        # ... and those samples are the statement's on the decoded file, through the library's table
        c = cpu.lib_table(wh.lib, fs, 16000, cpu.BEST)
        assert cpu.same_bits(y[0].cpu().numpy(), cpu.resample(x.cpu().numpy(), fs, 16000, c))
    r = _tool("resample", wavs[48000], "--outdir", os.path.dirname(wavs[48000]), "--fs", "16000")
    assert r.returncode != 0 and "resample:" in r.stderr and "Traceback" not in r.stderr


def test_analysis_tool_with_fs_equals_resample_then_analyze(wh, wavs, tmp_path):
    from world_amd.api import FileAPI, cheaptrick_fft_size
    r = _tool("analysis", wavs[48000], "--outdir", str(tmp_path / "tool"), "--fs", "16000")
    assert r.returncode == 0, r.stdout + r.stderr
    x = wh.wavread(wavs[48000])[0]
    y, y_len = wh.resample(x[None].contiguous(), 48000, 16000)
    tpos, f0, sp, ap, nf = wh.analyze(y, 16000, x_len=y_len)
    files, n, fft = FileAPI(), int(nf[0]), cheaptrick_fft_size(16000, 71.0)
    os.makedirs(tmp_path / "here")
    stem = str(tmp_path / "here" / "u48000")
    files.write_f0(stem + ".f0", 5.0, tpos[0, :n].cpu().numpy(), f0[0, :n].cpu().numpy())
    files.write_spectral_envelope(stem + ".sp", sp[0, :n].cpu().numpy(), 16000, 5.0, fft, 0)
    files.write_aperiodicity(stem + ".ap", ap[0, :n].cpu().numpy(), 16000, 5.0, fft, 0)
    for ext in (".f0", ".sp", ".ap"):
        a, b = open(str(tmp_path / "tool" / "u48000") + ext, "rb").read(), open(stem + ext, "rb").read()
        assert a == b and len(a) > 100, ext


def test_analysis_tool_takes_an_8_khz_file_with_fs_only(wavs, tmp_path):
    from world_amd.api import FileAPI, frame_count, resample_length
    r = _tool("analysis", wavs[8000], "--outdir", str(tmp_path / "no"))
    assert r.returncode != 0 and not os.path.exists(tmp_path / "no" / "u8000.f0")          # below D4C's range, as before
    r = _tool("analysis", wavs[8000], "--outdir", str(tmp_path / "yes"), "--fs", "16000")
    assert r.returncode == 0, r.stdout + r.stderr
    with wave.open(wavs[8000]) as w:
        n = w.getnframes()
    files = FileAPI()
    f0 = files.read_f0(str(tmp_path / "yes" / "u8000.f0"))[1]
    assert len(f0) == frame_count(16000, resample_length(n, 8000, 16000), 5.0) and np.any(f0 > 0)
    assert int(files.header(str(tmp_path / "yes" / "u8000.sp"), "FS  ")) == 16000


def test_morph_tool_mixes_rates_with_fs_only(wh, wavs, tmp_path):
    from world_amd import tools
    out = tmp_path / "out.wav"
    r = _tool("morph", wavs[44100], wavs[48000], "-o", str(out))
    assert r.returncode != 0 and "has another sampling rate" in r.stderr and not out.exists()
    r = _tool("morph", wavs[44100], wavs[48000], "-o", str(out), "--fs", "48000")
    assert r.returncode == 0, r.stdout + r.stderr
    got, rate = read_wav(out)
    xa, xb = wh.wavread(wavs[44100])[0], wh.wavread(wavs[48000])[0]
    xa = wh.resample(xa[None].contiguous(), 44100, 48000)[0][0]
    y, y_len = tools.morph_waves(wh, xa, xb, 48000, 0.5)
    want = wh.double_to_pcm16(y[0, :y_len]).cpu().numpy().astype(np.int32)
    assert rate == 48000 and len(got) == y_len and np.array_equal(got, want) and np.abs(got).max() > 0


def test_mcd_and_align_to_mix_rates_with_fs_only(wavs, tmp_path):
    r = _tool("mcd", wavs[44100], wavs[48000])
    assert r.returncode != 0 and "mcd:" in r.stderr and "different sampling rates" in r.stderr
    r = _tool("mcd", wavs[44100], wavs[48000], "--fs", "16000", "--quality", "fast")
    assert r.returncode == 0 and " mcd " in r.stdout and "dB" in r.stdout, r.stdout + r.stderr
    r = _tool("transform", wavs[44100], "--outdir", str(tmp_path), "--align-to", wavs[48000])
    assert r.returncode != 0 and "has another sampling rate" in r.stderr and not os.listdir(tmp_path)
    r = _tool("transform", wavs[44100], "--outdir", str(tmp_path), "--align-to", wavs[48000], "--fs", "16000")
    assert r.returncode == 0, r.stdout + r.stderr
    got, rate = read_wav(tmp_path / "u44100.wav")
    assert rate == 16000 and np.abs(got).max() > 0
    # one output frame per frame of the other recording at 16 kHz: its duration, within a frame shift
    with wave.open(wavs[48000]) as w:
        seconds = w.getnframes() / 48000.0
    assert abs(len(got) / 16000.0 - seconds) <= 0.011


def test_tools_report_a_refused_ratio_without_a_traceback(wavs, tmp_path):
    """44 100 -> 48 001 Hz has too many phases: every tool that takes --fs says so and exits, nothing written"""
    out = str(tmp_path / "o")
    for tool, args in (("analysis", (wavs[44100], "--outdir", out)), ("transform", (wavs[44100], "--outdir", out)),
                       ("mcd", (wavs[44100], wavs[48000])), ("morph", (wavs[44100], wavs[48000], "-o", out + ".wav")),
                       ("resample", (wavs[44100], "--outdir", out))):
        r = _tool(tool, *args, "--fs", "48001")
        assert r.returncode != 0 and f"{tool}:" in r.stderr and "L = 48001" in r.stderr and "Traceback" not in r.stderr, (tool, r.stderr)
    assert not os.path.exists(out + ".wav") and not (os.path.isdir(out) and os.listdir(out))
