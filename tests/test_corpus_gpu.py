"""Training rows of a corpus on the MI355X (include/world_hip.h: world_hip_frame_power_batch / _select_frames_batch /
_gather_rows_batch / _joint_rows_batch): the cases of test_corpus_cpu.py through the shipped library -- there 64 lanes share
a row's partial sums, a workgroup of 256 scans a tile of the selection and groups of lanes copy rows in 16-byte words, none
of which the one-lane emulation exercises -- then graph replay, the Python layer and vc-train.  The bounds are
test_corpus_cpu.py's."""
import re

import numpy as np
import pytest

import test_corpus_cpu as cpu
import test_gmm_cpu as gmm
from backends import OnGpu, gpu_backend, same_bits, wh, write_wav  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


# ---- the cases of the CPU file -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft_size,lengths", cpu.POWER, ids=cpu.POWER_IDS)
def test_power_is_the_stated_order_and_within_the_summation_bound(be, fft_size, lengths):
    cpu.case_power(be, fft_size, lengths)


@pytest.mark.parametrize("T", cpu.SELECT_T)
def test_selection_equals_flatnonzero(be, T):
    cpu.case_select(be, T)


def test_selection_at_the_threshold_nan_and_ragged_batches(be):
    cpu.case_select_edges(be)


@pytest.mark.parametrize("D", cpu.GATHER_DIMS)
def test_gather_copies_bits_from_any_alignment(be, D):
    cpu.case_gather(be, D)


@pytest.mark.parametrize("D", cpu.GATHER_DIMS)
def test_joint_rows_follow_the_path_and_the_selections(be, D):
    cpu.case_joint(be, D)


def test_gate_gather_align_joint_is_the_numpy_composition(be):
    cpu.case_composition(be)


def test_an_utterance_depends_on_nothing_but_itself(be):
    """(alone, in a batch of three and of seven, first, in the middle and last)"""
    cpu.case_determinism(be)


def test_only_a_mean_without_power_takes_workspace(be):
    cpu.case_workspace(be)


def test_refusals_write_nothing_and_give_a_reason(be):
    cpu.case_refusals(be)


# ---- graph replay --------------------------------------------------------------------------------------------------------
def test_a_captured_replay_of_each_call_equals_the_eager_one():
    """after one eager call of the shape (the count arrays are then on the device) each call can be captured, and the replay
    gives the eager bits"""
    import torch
    from world_amd.api import WorldHip
    fft_size, bins, D = 128, 65, 7
    n = np.array([65, 130, 3], dtype=np.int32)
    U, F = len(n), int(n.max())
    rng = np.random.default_rng(3)
    w = WorldHip()
    s = torch.cuda.Stream()
    graphs = []
    try:
        with torch.cuda.stream(s):
            b = GpuBackend(w)
            sp = b.dev(np.stack([np.vstack([cpu.envelopes(fft_size, int(t), 90 + u), np.ones((F - int(t), bins))]) for u, t in enumerate(n)]))
            x = b.dev(rng.standard_normal((U, F, D + 1)))
            idx = b.dev(np.stack([rng.integers(-1, int(t) + 1, size=F) for t in n]).astype(np.int32))
            path = b.dev(np.stack([np.stack([rng.integers(0, int(t), size=2 * F), rng.integers(0, int(t), size=2 * F)], axis=1) for t in n]).astype(np.int32))
            K = np.array([2 * F, 5, 2 * F - 1], dtype=np.int32)
            z_row = np.concatenate([[0], np.cumsum(K[:-1])])
            power, mean = b.dev(np.full((U, F), cpu.SENTINEL)), b.dev(np.full(U, cpu.SENTINEL))
            index, count = b.dev(np.full((U, F), cpu.ISENT, dtype=np.int32)), b.dev(np.full(U, cpu.ISENT, dtype=np.int32))
            keep = b.dev(np.full((U, F), cpu.BSENT, dtype=np.uint8))
            rows, z = b.dev(np.full((U, F, D), cpu.SENTINEL)), b.dev(np.full((int(K.sum()), 2 * D + 1), cpu.SENTINEL))
            first = np.arange(U) * F
            S, I, B = cpu.SENTINEL, cpu.ISENT, cpu.BSENT
            calls = {
                "power": (lambda: b.call_power(U, fft_size, n, b.addr(sp), F * bins, bins, b.addr(power), F, b.addr(mean)), ((power, S), (mean, S))),
                "select": (lambda: b.call_select(U, n, b.addr(power), F, 1, 0.9, b.addr(mean), None, 0, b.addr(index), F, b.addr(count), b.addr(keep), F),
                           ((index, I), (count, I), (keep, B))),
                "gather": (lambda: b.call_gather(U, D, n, b.addr(x) + 8, F * (D + 1), D + 1, n, b.addr(idx), F, -1.0, b.addr(rows), F * D, D), ((rows, S),)),
                "joint": (lambda: b.call_joint(U, D, D, b.addr(x), first, n, D + 1, b.addr(x) + 8, first, n, D + 1, K, b.addr(path), 2 * F, b.addr(idx), n, F,
                                               None, None, 0, -2.0, b.addr(z), z_row, 2 * D + 1), ((z, S),)),
            }
            for name, (call, outs) in calls.items():              # (in this order: the selection reads the power call's outputs)
                w._check(call(), name)
                torch.cuda.synchronize()
                eager = [b.host(o).copy() for o, _ in outs]
                assert all(np.any(e != sentinel) for e, (_, sentinel) in zip(eager, outs)), f"{name}: nothing was written"
                g = w.capture(lambda: w._check(call(), name))
                graphs.append(g)
                for o, sentinel in outs:
                    o.fill_(sentinel)
                g.launch()
                torch.cuda.synchronize()
                for (o, _), e in zip(outs, eager):
                    assert np.array_equal(b.host(o).view(np.uint8), e.view(np.uint8)), f"{name}: the replay differs from the eager call"
    finally:
        for g in graphs:
            g.close()
        w.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_worldhip_corpus_calls_honour_views(wh, be):
    import torch
    pairs = cpu.gated_corpus()
    gate = 10.0 ** -2.0
    sides = []
    for s in (0, 1):
        sp, c, dyn = ([p[s][k] for p in pairs] for k in range(3))
        n = np.array([len(v) for v in sp], dtype=np.int32)
        P, F, bins, D = len(n), int(n.max()), sp[0].shape[1], c[0].shape[1]
        block = torch.full((P, F, 2 + bins + D + 1), cpu.SENTINEL, dtype=torch.float64, device=wh.device)     # records: [tpos, f0, sp, c, spare]
        for u in range(P):
            block[u, :n[u], 2:2 + bins] = torch.from_numpy(sp[u]).to(wh.device)
            block[u, :n[u], 2 + bins:2 + bins + D] = torch.from_numpy(c[u]).to(wh.device)
        power, mean = wh.frame_power(block[:, :, 2:2 + bins], n)
        want_p, want_m = be.power(sp, 2 * (bins - 1))
        assert all(same_bits(power[u, :n[u]].cpu().numpy(), want_p[u]) for u in range(P)) and same_bits(mean.cpu().numpy(), want_m)
        assert bool((power[0, n[0]:] == 0).all())
        one_p, one_m = wh.frame_power(block[1, :n[1], 2:2 + bins])
        assert same_bits(one_p.cpu().numpy(), want_p[1]) and one_m.dim() == 0 and same_bits([float(one_m)], want_m[1:2])
        index, count, keep = wh.select_frames(power, n, gate, scale=mean)
        want_i, want_c, want_k = be.select(want_p, gate, scale=want_m)
        k = count.cpu().numpy()
        assert np.array_equal(k, want_c) and all(np.array_equal(index[u, :k[u]].cpu().numpy(), want_i[u]) for u in range(P))
        assert all(np.array_equal(keep[u, :n[u]].cpu().numpy(), want_k[u]) for u in range(P))
        # a column of the records as the value (c0), masked by the keep of the power gate
        col = block[:, :, 2 + bins]
        i2, c2, k2 = wh.select_frames(col, n, -1.0, mask=keep)
        for u in range(P):
            w_i, w_k = cpu.rule_select(c[u][:, 0], -1.0, 1.0, want_k[u])
            assert np.array_equal(i2[u, :int(c2[u])].cpu().numpy(), w_i) and np.array_equal(k2[u, :n[u]].cpu().numpy(), w_k)
        statics = block[:, :, 2 + bins + 1:2 + bins + D]                   # without c0: an odd column for one side, even for the other
        kept = wh.gather_rows(statics, index, k, n_src=n)
        assert all(same_bits(kept[u, :k[u]].cpu().numpy(), c[u][want_i[u], 1:]) for u in range(P))
        out = torch.full((P, int(k.max()) + 1, D + 1), cpu.SENTINEL, dtype=torch.float64, device=wh.device)
        assert wh.gather_rows(statics, index, k, n_src=n, out=out[:, :, 1:D]).data_ptr() == out[:, :, 1:D].data_ptr()
        assert all(same_bits(out[u, :k[u], 1:D].cpu().numpy(), c[u][want_i[u], 1:]) for u in range(P))
        assert bool((out[:, :, 0] == cpu.SENTINEL).all()) and bool((out[:, :, D] == cpu.SENTINEL).all()) and bool((out[0, k[0]:] == cpu.SENTINEL).all())
        sides.append((dyn, n, index, k, kept, want_i))
    (da, na, ia, ka, fa, wa), (db, nb, ib, kb, fb, wb) = sides
    path, path_len, _, _, _ = wh.align(fa, fb, ka, kb)
    K = path_len.cpu().numpy()
    # a and b as blocks of rows with first rows, the path lengths as align's tensor
    a_row, b_row = (np.concatenate([[0], np.cumsum(n[:-1])]) for n in (na, nb))
    blk_a, blk_b = (torch.from_numpy(np.vstack(d)).to(wh.device) for d in (da, db))
    z = wh.joint_rows(blk_a, blk_b, path, path_len, sel_a=ia, sel_b=ib, a_row=a_row, b_row=b_row, n_a=na, n_b=nb, n_sel_a=ka, n_sel_b=kb)
    steps = [path[u, :K[u]].cpu().numpy() for u in range(len(K))]
    want = np.vstack([np.hstack([da[u][wa[u][p[:, 0]]], db[u][wb[u][p[:, 1]]]]) for u, p in enumerate(steps)])
    assert same_bits(z.cpu().numpy(), want)
    only_a = wh.joint_rows(blk_a, None, path, K, sel_a=ia, a_row=a_row, n_a=na, n_sel_a=ka)
    assert same_bits(only_a.cpu().numpy(), want[:, :da[0].shape[1]])
    with pytest.raises(RuntimeError, match="overlap"):
        wh.gather_rows(statics, index, k, n_src=n, out=block[:, :int(k.max()), 2 + bins + 1:2 + bins + D])
    with pytest.raises(ValueError, match="n_frames"):
        wh.frame_power(block[:, :, 2:2 + bins], [F + 1] * len(n))


# ---- the tools -----------------------------------------------------------------------------------------------------------
SILENCE = 0.1       # seconds of digital silence in front of and behind every utterance of the gated corpus


@pytest.fixture(scope="module")
def vc_files(wh, tmp_path_factory):
    """the two synthetic speakers of test_gmm_gpu.py's tool test as .mgc files, plain and with silence around every wav"""
    from world_amd import synth, tools
    dim = gmm.VC_ORDER + 1
    files = {}
    for kind, pad in (("plain", 0), ("padded", int(SILENCE * gmm.VC_FS))):
        root = tmp_path_factory.mktemp(kind)
        wavs = []
        for seed, base in gmm.VC_UTTERANCES:
            q = np.round(synth.vowel(gmm.VC_FS, 0.5, seed=seed, base_f0=base).numpy() * 32768).clip(-32768, 32767).astype("<i2")
            wavs.append(write_wav(str(root / f"src{seed}.wav"), np.concatenate([np.zeros(pad, dtype="<i2"), q, np.zeros(pad, dtype="<i2")]), gmm.VC_FS))
        tools.main(["features", *wavs, "--outdir", str(root), "--order", str(gmm.VC_ORDER)])
        src = [str(root / f"src{seed}.mgc") for seed, _ in gmm.VC_UTTERANCES]
        tgt = [str(root / f"tgt{seed}.mgc") for seed, _ in gmm.VC_UTTERANCES]
        for s, t in zip(src, tgt):
            gmm.vc_target(np.fromfile(s, dtype="<f4").reshape(-1, dim)).tofile(t)
        files[kind] = (src, tgt, root)
    return files


def _statics(wh, files, dim):
    import torch
    return [torch.from_numpy(np.fromfile(f, dtype="<f4").astype(np.float64).reshape(-1, dim)).to(wh.device) for f in files]


def parent_rows(wh, src, tgt, align_src=None):
    """the per-pair loop vc-train ran before the corpus stage existed: deltas, one align call per pair, torch indexing"""
    import torch
    from world_amd import tools
    rows = []
    for u, (s, t) in enumerate(zip(src, tgt)):
        xa, xb = wh.deltas(s, windows=tools.VC_WINDOWS), wh.deltas(t, windows=tools.VC_WINDOWS)
        a = s if align_src is None else align_src[u]
        path, path_len, _, _, _ = wh.align(a[None, :, 1:], t[None, :, 1:], [len(a)], [len(t)])
        steps = path[0, :int(path_len[0])].long()
        rows.append(torch.cat([xa[steps[:, 0]], xb[steps[:, 1]]], dim=1))
    return torch.cat(rows)


def _saved(path):
    with np.load(path) as f:
        return {k: f[k] for k in ("w", "mu", "cov", "loglik")}


def _train(args):
    from world_amd import tools
    tools.main(["vc-train", *args])


def test_vc_train_without_options_is_the_per_pair_loop_bit_for_bit(wh, vc_files, capsys):
    src, tgt, root = vc_files["plain"]
    dim = gmm.VC_ORDER + 1
    model = str(root / "model.npz")
    _train([*src, "--target", *tgt, "--dim", str(dim), "--mix", str(gmm.VC_MIX), "--iter", str(gmm.VC_ITER), "-o", model])
    z = parent_rows(wh, _statics(wh, src, dim), _statics(wh, tgt, dim))
    w, mu, cov, loglik = wh.gmm_fit(z, gmm.VC_MIX, n_iter=gmm.VC_ITER, reg=gmm.VC_REG)
    got = _saved(model)
    assert f"{len(z)} joint rows" in capsys.readouterr().out
    assert same_bits(got["w"], w) and same_bits(got["mu"], mu) and same_bits(got["cov"], cov) and same_bits(got["loglik"], loglik)


def test_vc_train_with_a_power_gate_leaves_the_silence_out(wh, vc_files, capsys):
    """the row count and the model are the restatement's -- NumPy's gate on the library's power, the library's align on the
    gathered rows, torch indexing -- and no joint row holds a frame that lies wholly in the silence.  One mixture: the gate
    keeps the onset and offset frames of every vowel, the default start puts a mean on row floor(rows / 4), which on this
    corpus of eight equal utterances is such a frame at the seam of two of them, and a mixture started there is starved in the
    first iteration (9 rows' worth of weight against the 101 that 100 dimensions need) -- a property of 820 rows and that start,
    measured on an MI355X, not of the gate."""
    import torch
    from world_amd import tools
    from world_amd.api import cheaptrick_fft_size
    src, tgt, root = vc_files["padded"]
    dim, gate_db, mix = gmm.VC_ORDER + 1, -20.0, 1
    model = str(root / "gated.npz")
    _train([*src, "--target", *tgt, "--dim", str(dim), "--mix", str(mix), "--iter", str(gmm.VC_ITER), "--power-gate", str(gate_db),
            "--fs", str(gmm.VC_FS), "-o", model])
    printed = capsys.readouterr().out
    fft_size, alpha = cheaptrick_fft_size(gmm.VC_FS), wh.mcep_alpha(gmm.VC_FS)
    rows, kept_frames, silent_rows = [], [], []
    quiet = int((SILENCE - 0.04) / 0.005)                              # frames whose 3-period window sees no speech (F0 >= 100 Hz)
    for s, t in zip(_statics(wh, src, dim), _statics(wh, tgt, dim)):
        xa, xb = wh.deltas(s, windows=tools.VC_WINDOWS), wh.deltas(t, windows=tools.VC_WINDOWS)
        keep = []
        for x in (s, t):
            power, mean = wh.frame_power(wh.mc2sp(x, alpha, fft_size))
            P, m = power.cpu().numpy(), float(mean)
            keep.append(np.flatnonzero(P >= np.float64(10.0 ** (gate_db / 10.0)) * np.float64(m)))
            silence = np.r_[0:quiet, len(P) - quiet:len(P)]
            assert 0 < len(keep[-1]) < len(P) and not np.isin(silence, keep[-1]).any(), "the gate kept a frame of the silence"
        ka, kb = (torch.from_numpy(k).to(wh.device) for k in keep)
        path, path_len, _, _, _ = wh.align(s[ka][None, :, 1:], t[kb][None, :, 1:], [len(ka)], [len(kb)])
        steps = path[0, :int(path_len[0])].long()
        rows.append(torch.cat([xa[ka[steps[:, 0]]], xb[kb[steps[:, 1]]]], dim=1))
        kept_frames.append(keep)
        silent_rows.append(xa[torch.from_numpy(np.r_[0:quiet, len(s) - quiet:len(s)]).to(wh.device)])
    z = torch.cat(rows)
    assert f"{len(z)} joint rows" in printed, printed
    # the tool's own rows: the same bits, and none of them starts with a silent source frame's [static, delta]
    a, b = (tools.vc_speaker(wh, _statics(wh, f, dim)) for f in (src, tgt))
    gates = [tools.vc_power_gate(wh, x[0], x[2], gmm.VC_FS, gate_db) for x in (a, b)]
    for g, side in zip(gates, (0, 1)):
        assert all(np.array_equal(g[0][u, :g[1][u]].cpu().numpy(), k[side]) for u, k in enumerate(kept_frames))
    z_tool, _ = tools.vc_joint_rows(wh, a, b, *gates)
    assert same_bits(z_tool.cpu().numpy(), z.cpu().numpy())
    silent = torch.cat(silent_rows)
    assert not bool((z_tool[:, None, :2 * dim] == silent[None]).all(dim=2).any()), "a joint row holds a frame of the silence"
    w, mu, cov, loglik = wh.gmm_fit(z, mix, n_iter=gmm.VC_ITER, reg=gmm.VC_REG)
    got = _saved(model)
    assert same_bits(got["w"], w) and same_bits(got["mu"], mu) and same_bits(got["cov"], cov) and same_bits(got["loglik"], loglik)
    with pytest.raises(SystemExit, match="--fs"):
        _train([*src, "--target", *tgt, "--dim", str(dim), "--power-gate", "-20", "-o", model])


def test_vc_train_realign_is_the_public_calls_made_by_hand(wh, vc_files, capsys):
    """one round: convert every source with the first fit (gmm_convert, mlpg), align the converted statics to the targets,
    rebuild the rows from the ORIGINAL source features, refit from the first fit.  Mechanics only: whether the realignment
    lowers the MCD on this toy corpus is printed, not asserted."""
    from world_amd import tools
    src, tgt, root = vc_files["plain"]
    dim = gmm.VC_ORDER + 1
    model = str(root / "realigned.npz")
    _train([*src, "--target", *tgt, "--dim", str(dim), "--mix", str(gmm.VC_MIX), "--iter", str(gmm.VC_ITER), "--realign", "1", "-o", model])
    printed = capsys.readouterr().out
    rounds = re.findall(r"round (\d+): (\d+) joint rows, mean log-likelihood (\S+), mean MCD along the paths (\S+) dB", printed)
    assert [r[0] for r in rounds] == ["0", "1"], printed
    print("vc-train --realign 1:", "; ".join(f"round {r[0]}: loglik {r[2]}, path MCD {r[3]} dB" for r in rounds))
    s, t = _statics(wh, src, dim), _statics(wh, tgt, dim)
    fit0 = wh.gmm_fit(parent_rows(wh, s, t), gmm.VC_MIX, n_iter=gmm.VC_ITER, reg=gmm.VC_REG)
    prepared = wh.gmm_prepare(*fit0[:3], 2 * dim)
    converted = []
    for x in s:
        mean, var = wh.gmm_convert(prepared, wh.deltas(x, windows=tools.VC_WINDOWS))
        converted.append(wh.mlpg(mean, var, windows=tools.VC_WINDOWS))
    w, mu, cov, loglik = wh.gmm_fit(parent_rows(wh, s, t, align_src=converted), gmm.VC_MIX, n_iter=gmm.VC_ITER, reg=gmm.VC_REG, init=fit0[:3])
    got = _saved(model)
    assert np.all(np.isfinite(fit0[3])) and np.all(np.isfinite(loglik)) and all(np.isfinite(float(r[2])) and np.isfinite(float(r[3])) for r in rounds)
    assert same_bits(got["w"], w) and same_bits(got["mu"], mu) and same_bits(got["cov"], cov) and same_bits(got["loglik"], loglik)
    with pytest.raises(SystemExit, match="--realign"):
        _train([*src, "--target", *tgt, "--dim", str(dim), "--realign", "-1", "-o", model])
