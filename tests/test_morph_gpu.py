"""Morph of two aligned utterances on the MI355X (include/world_hip.h: world_hip_morph_batch): the cases of
test_morph_cpu.py through the shipped library, graph replay, the Python layer, an utterance against its own time-stretched
resynthesis from the waveform to the waveform, and the morph tool."""
import subprocess
import sys
import wave

import numpy as np
import pytest

import test_morph_cpu as cpu
from backends import ROOT, OnGpu, gpu_backend, wh, write_wav  # noqa: F401 (wh: a fixture)
from util import utterance

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


@pytest.mark.parametrize("r", cpu.TIME_RATES)
def test_positions_are_the_statements_bit_for_bit(be, r):
    cpu.case_positions(be, r)


def test_time_rates_0_and_1_give_aligns_maps(be):
    cpu.case_end_rates_equal_aligns_maps(be)


def test_no_path_is_the_identity(be):
    cpu.case_no_path_is_the_identity(be)


@pytest.mark.parametrize("fft", [128, 1024])
@pytest.mark.parametrize("r", [0.0, 0.3, 1.0])
def test_the_mixed_batch_against_the_statement(be, fft, r):
    cpu.case_statement(be, 16000, fft, r)


def test_fft_2048_at_48_khz_against_the_statement(be):
    cpu.case_statement(be, 48000, 2048, 1.0 / 3.0)


@pytest.mark.parametrize("fft", [128, 1024])
def test_end_rates_equal_modify_frames_behind_aligns_maps(be, fft):
    cpu.case_cross_checks(be, 16000, fft)


@pytest.mark.parametrize("fft", [128, 1024])
def test_morph_of_an_utterance_with_itself(be, fft):
    cpu.case_morph_with_itself(be, 16000, fft)


def test_f0_voicing_table(be):
    cpu.case_voicing_table(be)


@pytest.mark.parametrize("fft", [128, 1024])
def test_rate_curves(be, fft):
    cpu.case_curves(be, 16000, fft)


def test_strides_sentinels_and_optional_triples(be):
    cpu.case_layout_and_optional_triples(be, 16000, 128)


def test_refusals_touch_nothing(be):
    cpu.case_refusals(be)


@pytest.mark.parametrize("fft", [128, 1024])
def test_a_garbage_path_stays_in_bounds_and_in_its_pair(be, fft):
    cpu.case_garbage_path(be, 16000, fft)


def test_a_pair_alone_inside_a_batch_and_permuted(be):
    cpu.case_batch_independence(be, 16000, 128)


# ---- graph replay --------------------------------------------------------------------------------------------------------
def test_graph_replay_reads_the_new_inputs():
    """after one eager call the call is captured; rows, F0, path and curve are overwritten and the graph replayed: the
    outputs are the statement's on the new inputs (nothing is copied from the host, nothing is baked in but addresses)"""
    import torch
    from world_amd.api import WorldHip, morphs
    fs, fft = 16000, 1024
    counts = ((5, 9), (40, 23), (30, 30))
    na, nb, A, B = cpu.batch(fs, fft, counts)
    P, O, S = 3, 40, 62
    rates = (0.4, 0.25, 0.5, 0.75)

    def stored(paths):
        s = np.full((P, S, 2), -99, dtype=np.int32)
        for u, q in enumerate(paths):
            s[u, :len(q)] = q
        return s, np.array([len(q) for q in paths], dtype=np.int32)
    paths, paths2 = cpu.hand_paths(counts, seed=1), cpu.hand_paths(counts, seed=2)
    rng = np.random.default_rng(3)
    curve, curve2 = rng.random((P, O)), rng.random((P, O))
    # the second set of inputs: the same shapes, other values (rows shuffled along the frames, F0 scaled)
    other = lambda T, n: tuple(np.ascontiguousarray(np.where(np.isnan(x), x, np.roll(x, 1, axis=1) if x.ndim == 3 else x * 1.1))
                               for x in T)
    A2, B2 = other(A, na), other(B, nb)
    for T, n in ((A2, na), (B2, nb)):                                   # the roll must not bring padding into the frames
        for x in T[1:]:
            for u in range(P):
                x[u, 0] = x[u, n[u] - 1] if n[u] > 1 else x[u, 0]
                assert np.all(np.isfinite(x[u, :n[u]]))
    wh = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            be = GpuBackend(wh)
            d_a, d_b = tuple(be.dev(x) for x in A), tuple(be.dev(x) for x in B)
            st, ln = stored(paths)
            d_path, d_len, d_curve = be.dev(st), be.dev(ln), be.dev(curve)
            outs = [be.dev(np.full((P, O) + x.shape[2:], cpu.SENTINEL)) for x in A] + [be.dev(np.full((P, O), cpu.SENTINEL)) for _ in range(2)]
            ms = morphs(P, *rates)
            call = lambda: wh._check(be.morph_call(P, fs, fft, na, 40, d_a, nb, 30, d_b, S, d_path, d_len, ms,
                                                   dict(d_sp_rate=d_curve), O, tuple(outs[:3]), tuple(outs[3:])), "morph")
            call()
            torch.cuda.synchronize()
            cpu.check_against_statement((0, *[be.host(o) for o in outs]), na, nb, A, B, paths, rates, dict(sp=curve))
            g = wh.capture(call)
            for d, h in zip(d_a + d_b, A2 + B2):
                d.copy_(torch.from_numpy(h))
            st2, ln2 = stored(paths2)
            d_path.copy_(torch.from_numpy(st2)); d_len.copy_(torch.from_numpy(ln2)); d_curve.copy_(torch.from_numpy(curve2))
            for o in outs:
                o.fill_(cpu.SENTINEL)
            g.launch()
            torch.cuda.synchronize()
            cpu.check_against_statement((0, *[be.host(o) for o in outs]), na, nb, A2, B2, paths2, rates, dict(sp=curve2))
    finally:
        if g is not None:
            g.close()
        wh.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_python_layer_matches_the_c_call_and_validates_curves(wh, be):
    import torch
    fs, fft = 16000, 1024
    counts = ((5, 9), (40, 23))
    na, nb, A, B = cpu.batch(fs, fft, counts)
    paths = cpu.hand_paths(counts)
    S = 62
    st = np.full((2, S, 2), -99, dtype=np.int32)
    for u, q in enumerate(paths):
        st[u, :len(q)] = q
    d_path = torch.from_numpy(st).cuda()
    d_len = torch.tensor([len(q) for q in paths], dtype=torch.int32, device="cuda")
    d_a, d_b = tuple(torch.from_numpy(x).cuda() for x in A), tuple(torch.from_numpy(x).cuda() for x in B)
    assert wh.morph_length(40, 23, 0.3) == cpu.morph_length(40, 23, 0.3)
    with pytest.raises(ValueError):
        wh.morph_length(40, 23, 1.5)
    O = cpu.morph_length(40, 23, 0.3)
    ramp = torch.linspace(0.0, 1.0, O, dtype=torch.float64, device="cuda")
    f0, sp, ap, no, pa, pb = wh.morph(d_a, d_b, na, nb, fs, fft, d_path, d_len, rate=0.6, time_rate=0.3, sp_rate=ramp,
                                      ap_rate=[0.2, 0.9], want_positions=True)
    assert list(no) == [cpu.morph_length(5, 9, 0.3), O] and f0.shape == (2, O) and sp.shape == (2, O, fft // 2 + 1)
    rates = (0.3, 0.6, 0.0, np.array([0.2, 0.9]))
    curves = dict(sp=np.tile(ramp.cpu().numpy(), (2, 1)))
    got = [x.cpu().numpy() for x in (f0, sp, ap, pa, pb)]
    for x, n in zip(got, [no] * 5):
        for u in range(2):
            assert np.all(x[u, n[u]:] == 0.0)
            x[u, n[u]:] = cpu.SENTINEL
    cpu.check_against_statement((0, *got), na, nb, A, B, paths, rates, curves)
    for value in (float("nan"), -0.1, 1.5, float("inf")):
        bad = ramp.clone()
        bad[3] = value
        with pytest.raises(ValueError):
            wh.morph(d_a, d_b, na, nb, fs, fft, d_path, d_len, f0_rate=bad)
    with pytest.raises(RuntimeError):
        wh.morph(d_a, d_b, na, nb, fs, fft, d_path, d_len, rate=1.5, time_rate=0.5)


# ---- from the waveform to the waveform -----------------------------------------------------------------------------------
def test_an_utterance_morphed_half_way_to_its_stretched_resynthesis(wh):
    """a synthetic utterance and its resynthesis at time_scale 1.5: analysed, coded to mel-cepstra, aligned without c0,
    morphed at 0.5 and synthesised -- finite, of world_hip_resynthesis_length(fs, morph_length, ...) samples, sA and sB
    non-decreasing and within their utterances"""
    import torch
    from world_amd import tools
    from world_amd.api import cheaptrick_fft_size
    fs = 16000
    fft = cheaptrick_fft_size(fs, 71.0)
    x = torch.from_numpy(utterance(fs, 0.4)).to(wh.device)[None].contiguous()
    y, yl = wh.resynthesize(x, fs, time_scale=1.5)
    xb = y[:, :int(yl[0])].contiguous()
    sides = []
    for sig in (x, xb):
        _, f0, sp, ap, nf = wh.analyze(sig, fs)
        sides.append(((f0, sp, ap), nf, wh.code_spectral_envelope(sp, fs, fft, tools.ALIGN_DIMS)))
    (a, nf_a, mc_a), (b, nf_b, mc_b) = sides
    assert int(nf_b[0]) > int(nf_a[0])
    path, path_len, _, _, _ = wh.align(mc_a[:, :, 1:], mc_b[:, :, 1:], nf_a, nf_b)
    f0, sp, ap, no, pa, pb = wh.morph(a, b, nf_a, nf_b, fs, fft, path, path_len, rate=0.5, want_positions=True)
    n = wh.morph_length(int(nf_a[0]), int(nf_b[0]), 0.5)
    assert list(no) == [n] and int(nf_a[0]) <= n <= int(nf_b[0])
    pa, pb = pa[0, :n].cpu().numpy(), pb[0, :n].cpu().numpy()
    K = int(path_len[0])
    want_a, want_b = cpu.positions(path[0, :K].cpu().numpy(), int(nf_a[0]), int(nf_b[0]), 0.5)
    assert np.array_equal(pa, want_a) and np.array_equal(pb, want_b)
    assert np.all(np.diff(pa) >= 0) and np.all(np.diff(pb) >= 0)
    assert pa[0] >= 0 and pa[-1] <= nf_a[0] - 1 and pb[0] >= 0 and pb[-1] <= nf_b[0] - 1
    assert bool(torch.isfinite(sp[0, :n]).all()) and bool((sp[0, :n] > 0).all()) and bool(torch.isfinite(f0[0, :n]).all())
    y_len = wh.lib.world_hip_resynthesis_length(fs, n, 5.0, 1.0)
    out = wh.synthesis(f0, sp, ap, no, fft, 5.0, fs, np.array([y_len], dtype=np.int32))
    assert out.shape == (1, y_len) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 1e-3
    # the same chain as the tool's function runs it
    y2, y2_len = tools.morph_waves(wh, x[0], xb[0], fs, 0.5)
    assert y2_len == y_len and torch.equal(y2, out)


def test_morph_tool_writes_what_the_python_path_computes(wh, tmp_path):
    from world_amd import synth, tools
    fs = 16000
    names = []
    for name, seconds, seed, rate in (("a", 0.30, 51, fs), ("b", 0.42, 52, fs), ("c", 0.30, 53, 22050)):
        q = np.round(synth.vowel(rate, seconds, seed=seed).numpy() * 32768).clip(-32768, 32767).astype(np.int16)
        names.append(str(tmp_path / (name + ".wav")))
        write_wav(names[-1], q, rate)
    out = tmp_path / "out.wav"
    run = lambda *args: subprocess.run([sys.executable, "-m", "world_amd.tools", "morph", *args], cwd=ROOT, capture_output=True,
                                       text=True, timeout=300)
    r = run(names[0], names[1], "-o", str(out), "--rate", "0.3", "--fade")
    assert r.returncode == 0, r.stdout + r.stderr
    with wave.open(str(out)) as w:
        got = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int32)
        assert w.getframerate() == fs
    xa, xb = wh.wavread(names[0])[0], wh.wavread(names[1])[0]
    y, y_len = tools.morph_waves(wh, xa, xb, fs, 0.3, fade=True)
    want = wh.double_to_pcm16(y[0, :y_len]).cpu().numpy().astype(np.int32)
    assert np.array_equal(got, want) and np.abs(got).max() > 0
    for args in ((names[0], names[2], "-o", str(out)), (names[0], names[1], "-o", str(out), "--rate", "1.5"),
                 (names[0], str(tmp_path / "missing.wav"), "-o", str(out))):
        r = run(*args)
        assert r.returncode != 0 and "morph:" in r.stderr and "Traceback" not in r.stderr, (args, r.stderr)
