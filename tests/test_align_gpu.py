"""Alignment by dynamic time warping on the MI355X (include/world_hip.h: world_hip_align_batch): the cases of
test_align_cpu.py through the shipped library, graph replay, the Python layer, an utterance against its own time-stretched
resynthesis, and the mcd tool."""
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

import test_align_cpu as cpu
from backends import ROOT, OnGpu, gpu_backend, wh, write_wav  # noqa: F401 (wh: a fixture)
from util import load_golden

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


def test_degenerate_pairs(be):
    cpu.case_degenerate(be)


def test_identical_sequences_give_the_diagonal(be):
    cpu.case_identical(be)


def test_repeated_frames_give_the_hold_pattern_and_mid_points(be):
    cpu.case_repeats(be)


def test_ties_follow_the_statement(be):
    cpu.case_ties(be)


@pytest.mark.parametrize("na,nb", cpu.EDGES)
def test_sizes_around_the_workgroup_tile_and_buffer_edges(be, na, nb):
    cpu.case_edge(be, na, nb)


@pytest.mark.parametrize("D", cpu.DIMS)
def test_dimensions(be, D):
    cpu.case_dims(be, D)


def test_addressing_strides_offsets_packed_rows_and_aliasing(be):
    cpu.case_addressing(be)


def test_a_pair_alone_inside_a_batch_and_permuted(be):
    cpu.case_batch_independence(be)


def test_each_output_is_optional(be):
    cpu.case_optional_outputs(be)


def test_refusals_touch_nothing(be):
    cpu.case_refusals(be)


def test_non_finite_features_stay_in_their_pair(be):
    cpu.case_non_finite(be)


def test_graph_replay_reads_the_new_inputs():
    """after one eager call the call is captured; the inputs are overwritten and the graph replayed: the outputs are those
    of an eager call on the new inputs (nothing is copied from the host, nothing is baked in but addresses)"""
    import torch
    from world_amd.api import WorldHip
    pairs, other = cpu.mixed_pairs(12), cpu.mixed_pairs(13)
    sa, sb, ar, na, br, nb, stride = cpu.dense(pairs)
    sa2, sb2 = cpu.dense(other)[:2]
    P, S, M = len(pairs), int(np.max(na + nb)) - 1, int(max(na.max(), nb.max()))
    wh = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            be = GpuBackend(wh)
            d_a, d_b = be.dev(sa), be.dev(sb)
            outs = be.buffers(P, S, M)
            call = lambda: wh._check(be.call(P, 5, d_a, 0, ar, na, stride, d_b, 0, br, nb, stride, S, M, outs), "align")
            call()
            torch.cuda.synchronize()
            for u, (A, B) in enumerate(pairs):
                cpu.check_pair({k: be.host(v) for k, v in outs.items()}, u, cpu.statement(A, B), len(A), len(B))
            g = wh.capture(call)
            d_a.copy_(torch.from_numpy(sa2)); d_b.copy_(torch.from_numpy(sb2))
            for v in outs.values():
                v.fill_(cpu.SENTINEL)
            g.launch()
            torch.cuda.synchronize()
            replayed = {k: be.host(v) for k, v in outs.items()}
            for v in outs.values():
                v.fill_(cpu.SENTINEL)
            call()
            torch.cuda.synchronize()
            for k, v in outs.items():
                assert np.array_equal(be.host(v), replayed[k]), k
            for u, (A, B) in enumerate(other):
                cpu.check_pair(replayed, u, cpu.statement(A, B), len(A), len(B))
    finally:
        if g is not None:
            g.close()
        wh.close()


def test_python_layer_on_dense_tensors_and_record_blocks(wh, be):
    import torch
    pairs = cpu.mixed_pairs(14)
    sa, sb, ar, na, br, nb, stride = cpu.dense(pairs, stride=9, off=2)
    a = torch.from_numpy(sa.reshape(len(pairs), -1, 9)).cuda()
    b = torch.from_numpy(sb.reshape(len(pairs), -1, 9)).cuda()
    path, path_len, summary, map_b, map_a = wh.align(a[:, :, 2:7], b[:, :, 2:7], na, nb)
    outs = dict(path=path.cpu().numpy(), path_len=path_len.cpu().numpy(), summary=summary.cpu().numpy())
    for u, (A, B) in enumerate(pairs):
        want = cpu.statement(A, B)
        K = len(want[1])
        assert outs["path_len"][u] == K and np.array_equal(outs["path"][u, :K], want[1]) and outs["summary"][u, 0] == want[0]
        assert np.array_equal(map_b[u, :len(B)].cpu().numpy(), want[2]) and np.array_equal(map_a[u, :len(A)].cpu().numpy(), want[3])
    # a block of records, both sides in it, columns sliced by view
    block = torch.from_numpy(np.random.default_rng(15).standard_normal((30, 12))).cuda()
    got = wh.align(block[:, 3:10], block[:, 3:10], [10, 8], [12, 10], a_row=[0, 22], b_row=[10, 0], want_path=False)
    assert got[0] is None
    rows = block.cpu().numpy()
    for u, (A, B) in enumerate(((rows[0:10, 3:10], rows[10:22, 3:10]), (rows[22:30, 3:10], rows[0:10, 3:10]))):
        want = cpu.statement(A, B)
        assert got[2][u, 0].item() == want[0] and got[1][u].item() == len(want[1])
        assert np.array_equal(got[3][u, :len(B)].cpu().numpy(), want[2])


def test_an_utterance_against_its_stretched_resynthesis(wh):
    """golden utterance -> analyze_coded; resynthesize at time_scale 1.5 -> analyze_coded; aligned with c0 skipped: the path
    is the statement's on the same coded rows, and map_b drives modify_frames to n_b frames.  How close the map lies to
    j / 1.5 is a property of the analysis, not of this kernel: printed, not asserted."""
    import torch
    from world_amd.api import cheaptrick_fft_size
    g = load_golden("vaiueo2d_harvest")
    fs, D = g["fs"], 25
    x = torch.from_numpy(g["x"]).to(wh.device)[None].contiguous()
    cols = wh.lib.world_hip_coded_columns(fs, D)

    def coded(sig):
        from world_amd.api import frame_count
        n = frame_count(fs, sig.shape[1], 5.0)
        block = torch.zeros((n, cols), dtype=torch.float64, device=wh.device)
        assert wh.analyze_coded(sig, fs, block, number_of_dimensions=D) == [n]
        return block, n

    blk_a, n_a = coded(x)
    y, yl = wh.resynthesize(x, fs, time_scale=1.5)
    blk_b, n_b = coded(y[:, :int(yl[0])].contiguous())
    path, path_len, summary, map_b, map_a = wh.align(blk_a[:, 3:2 + D], blk_b[:, 3:2 + D], [n_a], [n_b])
    want = cpu.statement(blk_a[:, 3:2 + D].cpu().numpy(), blk_b[:, 3:2 + D].cpu().numpy())
    K = int(path_len[0])
    assert K == len(want[1]) and np.array_equal(path[0, :K].cpu().numpy(), want[1])
    assert summary[0, 0].item() == want[0] and np.array_equal(map_b[0, :n_b].cpu().numpy(), want[2])
    tpos, f0, sp, ap, nf = wh.analyze(x, fs)
    assert int(nf[0]) == n_a
    fft = cheaptrick_fft_size(fs, 71.0)
    o_f0, o_sp, o_ap = wh.modify_frames(f0, sp, ap, nf, fs, fft, n_out=[n_b], time_map=map_b[:, :n_b].contiguous())
    assert o_f0.shape == (1, n_b) and o_sp.shape == (1, n_b, fft // 2 + 1) and o_ap.shape == o_sp.shape
    assert bool(torch.isfinite(o_sp).all()) and bool((o_sp > 0).all())
    voiced = (blk_b[:, 1] > 0).cpu().numpy()
    dev = np.abs(want[2] - np.arange(n_b) / 1.5)[voiced]
    print(f"stretched resynthesis: {n_a} x {n_b} frames, K {K}, mcd {summary[0, 2].item():.3f} dB, "
          f"median |map_b - j / 1.5| over {int(voiced.sum())} voiced frames: {np.median(dev):.3f} frames")


def test_mcd_tool_prints_what_the_python_call_gives(wh, tmp_path):
    from world_amd import synth, tools
    fs = 16000
    names = []
    for name, seconds, seed in (("ref", 0.40, 31), ("test", 0.55, 32)):
        q = np.round(synth.vowel(fs, seconds, seed=seed).numpy() * 32768).clip(-32768, 32767).astype(np.int16)
        write_wav(tmp_path / (name + ".wav"), q, fs)
        names.append(str(tmp_path / (name + ".wav")))
    r = subprocess.run([sys.executable, "-m", "world_amd.tools", "mcd", *names, "--dims", "25"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"frames (\d+) (\d+) path (\d+) mcd ([0-9.]+) dB", r.stdout)
    assert m, r.stdout
    (na, nb, K, mcd), = tools.mcd_pairs(wh, [tuple(names)], dims=25)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (na, nb, K)
    assert m.group(4) == f"{mcd:.6f}" and np.isfinite(mcd) and mcd > 0
    assert max(na, nb) <= K <= na + nb - 1


def test_transform_align_to_gives_the_other_recordings_timing(wh, tmp_path):
    """python -m world_amd.tools transform --align-to OTHER.wav: one output frame per frame of OTHER, the samples those of
    the Python path (analyze_coded both, align without c0, map_b as the time map); what cannot be combined with it, and an
    unreadable OTHER, end in a `transform:` message"""
    import torch
    from world_amd import synth, tools
    from world_amd.api import frame_count
    fs = 16000
    paths = {}
    for name, seconds, seed in (("in", 0.40, 41), ("other", 0.55, 42)):
        q = np.round(synth.vowel(fs, seconds, seed=seed).numpy() * 32768).clip(-32768, 32767).astype(np.int16)
        paths[name] = str(tmp_path / (name + ".wav"))
        write_wav(paths[name], q, fs)
    out = tmp_path / "out"
    run = lambda *more: subprocess.run([sys.executable, "-m", "world_amd.tools", "transform", paths["in"], "--outdir", str(out),
                                        "--align-to", *more], cwd=ROOT, capture_output=True, text=True, timeout=300)
    r = run(paths["other"], "--formant-shift", "1.1")
    assert r.returncode == 0, r.stdout + r.stderr
    with wave.open(str(out / "in.wav")) as w:
        got = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int32)
    x, _ = wh.wavread(paths["in"])
    o, _ = wh.wavread(paths["other"])
    n_a, n_b = frame_count(fs, x.numel(), 5.0), frame_count(fs, o.numel(), 5.0)
    assert len(got) == wh.lib.world_hip_resynthesis_length(fs, n_b, 5.0, 1.0)
    D = tools.ALIGN_DIMS
    blk_a = tools._coded_block(wh, x[None].contiguous(), fs, [x.numel()], 5.0, D)[0]
    blk_b = tools._coded_block(wh, o[None].contiguous(), fs, [o.numel()], 5.0, D)[0]
    map_b = wh.align(blk_a[:, 3:2 + D], blk_b[:, 3:2 + D], [n_a], [n_b], want_path=False)[3]
    assert map_b.shape == (1, n_b) and float(map_b[0, 0]) == 0.0 and float(map_b[0, -1]) <= n_a - 1
    y, yl = wh.resynthesize_frames(x[None].contiguous(), fs, n_out=[n_b], time_map=map_b.contiguous(), formant_shift=1.1)
    want = wh.double_to_pcm16(y[0, :int(yl[0])]).cpu().numpy().astype(np.int32)
    assert np.array_equal(got, want)
    for more in ((paths["other"], "--duration", "0.5"), (paths["other"], "--time-scale", "1.5"), (str(tmp_path / "missing.wav"),)):
        r = run(*more)
        assert r.returncode != 0 and "transform:" in r.stderr and "Traceback" not in r.stderr, (more, r.stderr)
