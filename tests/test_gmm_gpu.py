"""Joint-density Gaussian mixture on the MI355X (include/world_hip.h: world_hip_gmm_convert / _accumulate / _fit / _init):
the cases of test_gmm_cpu.py through the shipped library -- there four wavefronts share a workgroup's tile of 64 rows, the
model's chunks are fetched a chunk ahead into registers and the products run on v_mfma_f64_16x16x4_f64, none of which the
one-lane emulation exercises -- then graph replay, the Python layer and the tools.  The bounds are test_gmm_cpu.py's."""
import os
import wave

import numpy as np
import pytest

import test_gmm_cpu as cpu
from backends import OnGpu, gpu_backend, wh, write_wav  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


# ---- the cases of the CPU file -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,dx,dy", cpu.PREPARE[:2], ids=["M%d-Dx%d-Dy%d" % c for c in cpu.PREPARE[:2]])
def test_prepare_is_the_rule_in_140_bits(be, M, dx, dy):
    """(host arithmetic: the shipped library's build of it)"""
    cpu.case_prepare(be, M, dx, dy)


def test_prepare_and_update_refuse_by_mixture(be):
    cpu.case_prepare_refusals(be)


@pytest.mark.parametrize("M,dx,dy,rows,strided", cpu.CONVERT, ids=cpu.CONVERT_IDS)
def test_convert_is_the_rule(be, M, dx, dy, rows, strided):
    cpu.case_convert(be, M, dx, dy, rows, strided)


def test_modes_ties_and_far_rows(be):
    cpu.case_modes(be)


def test_a_row_depends_on_nothing_but_the_row(be):
    """(rows 15 / 16 are two lanes' rows of one wavefront, 63 / 64 two workgroups, 129 sits in the ragged third)"""
    cpu.case_row_independence(be)


@pytest.mark.parametrize("M,P,rows", cpu.ACCUMULATE, ids=["M%d-P%d-rows%d" % c for c in cpu.ACCUMULATE])
def test_accumulate_is_the_rule(be, M, P, rows):
    cpu.case_accumulate(be, M, P, rows)


def test_fit_is_the_single_calls_and_follows_the_restatement(be):
    cpu.case_fit(be)


def test_fit_against_sklearn(be):
    cpu.case_fit_sklearn(be)


def test_a_starved_mixture_is_refused(be):
    cpu.case_starved(be)


def test_init_is_the_default_start(be):
    cpu.case_init(be)


def test_refusals_write_nothing_and_give_a_reason(be):
    cpu.case_refusals(be)


def test_workspace_grows_once(be):
    cpu.case_workspace(be)


# ---- graph replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_a_captured_convert_equals_the_eager_one(mode):
    """after one eager call of the shape (the workspace then has the size) the call can be captured, and the replay gives
    the eager bits"""
    import torch
    from world_amd.api import WorldHip
    M, dx, dy, rows = 5, 17, 16, 130
    w = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            b = GpuBackend(w)
            model, parts = cpu.prepared(b, M, dx, dy)
            d_model, d_x = b.model_dev(model), b.dev(cpu.rows_near(parts, rows, 43))
            outs = [b.dev(np.full(shape, cpu.SENTINEL)) for shape in ((rows, dy), (rows, dy + 1), (rows, M), (rows,))]

            def call():
                w._check(b.call_convert(M, dx, dy, b.addr(d_model), rows, b.addr(d_x), dx, mode, b.addr(outs[0]), dy, b.addr(outs[1]),
                                        dy + 1, b.addr(outs[2]), M, b.addr(outs[3])), "gmm_convert")
            call()
            torch.cuda.synchronize()
            eager = [b.host(o) for o in outs]
            assert np.all(eager[0] != cpu.SENTINEL) and np.all(eager[1][:, dy] == cpu.SENTINEL) and np.all(eager[3] != cpu.SENTINEL)
            g = w.capture(call)
            for o in outs:
                o.fill_(cpu.SENTINEL)
            g.launch()
            torch.cuda.synchronize()
            assert all(cpu.same_bits(b.host(o), e) for o, e in zip(outs, eager))
    finally:
        if g is not None:
            g.close()
        w.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_worldhip_gmm_honours_views_with_row_strides(wh, be):
    import torch
    M, dx, dy, rows = 5, 17, 16, 130
    w, mu, cov = cpu.random_model(M, dx, dy, 1)
    model = wh.gmm_prepare(w, mu, cov, dx)
    host_model, parts = cpu.prepared(be, M, dx, dy)
    assert (model.M, model.dx, model.dy) == (M, dx, dy) and cpu.same_bits(model.data.cpu().numpy(), host_model)
    x = cpu.rows_near(parts, rows, 47)
    big = torch.full((rows, dx + 5), cpu.SENTINEL, dtype=torch.float64, device=wh.device)
    big[:, 2:2 + dx] = torch.from_numpy(x).to(wh.device)
    for mode, number in cpu.MODES.items():
        want = be.convert(M, dx, dy, be.model_dev(host_model), x, mode=number)
        mean, var = wh.gmm_convert(model, big[:, 2:2 + dx], mode=mode)
        assert cpu.same_bits(mean.cpu().numpy(), want["mean"]) and cpu.same_bits(var.cpu().numpy(), want["var"])
        # (two arrays: ranges are judged by their extents, so a mean and a variance interleaved in one array are refused)
        out, out_v = (torch.full((rows, dy + 3), cpu.SENTINEL, dtype=torch.float64, device=wh.device) for _ in range(2))
        got = wh.gmm_convert(model, big[:, 2:2 + dx], mode=mode, out=(out[:, :dy], out_v[:, 1:dy + 1]))
        assert got[0].data_ptr() == out.data_ptr()
        assert cpu.same_bits(out[:, :dy].cpu().numpy(), want["mean"]) and cpu.same_bits(out_v[:, 1:dy + 1].cpu().numpy(), want["var"])
        assert bool((out[:, dy:] == cpu.SENTINEL).all()) and bool((out_v[:, 0] == cpu.SENTINEL).all()) and bool((out_v[:, dy + 1:] == cpu.SENTINEL).all())
    post, loglik = wh.gmm_posterior(model, big[:, 2:2 + dx])
    assert cpu.same_bits(post.cpu().numpy(), want["post"]) and cpu.same_bits(loglik.cpu().numpy(), want["loglik"])
    # the pair is what mlpg consumes: dy = 16 is [static, delta] of 8 dimensions
    traj = wh.mlpg(mean, var, windows=wh.DEFAULT_WINDOWS[:2])
    assert traj.shape == (rows, 8) and bool(torch.isfinite(traj).all())
    with pytest.raises(ValueError, match="mode"):
        wh.gmm_convert(model, big[:, 2:2 + dx], mode="soft")
    with pytest.raises(RuntimeError, match="overlap"):
        wh.gmm_convert(model, big[:, 2:2 + dx], out=(big[:, :dy], out[:, :dy]))
    with pytest.raises(RuntimeError, match="overlap"):
        wh.gmm_convert(model, big[:, 2:2 + dx], out=(out[:, :dy], out[:, 1:dy + 1]))
    with pytest.raises(RuntimeError, match="mixture 1"):
        wh.gmm_prepare([0.5, 0.0] + [0.1] * 3, mu, cov, dx)
    # the fit: a strided view, a given start and the default one
    z, w0, mu0, cov0 = cpu.two_clusters()
    wide = torch.full((len(z), 6), cpu.SENTINEL, dtype=torch.float64, device=wh.device)
    wide[:, 1:4] = torch.from_numpy(z).to(wh.device)
    w3, mu3, cov3, ll3 = wh.gmm_fit(wide[:, 1:4], 2, n_iter=3, reg=1e-6, init=(w0, mu0, cov0))
    rc, w_b, mu_b, cov_b, ll_b = be.fit(z, 3, 1e-6, w0, mu0, cov0)
    assert rc == 0 and cpu.same_bits(w3, w_b) and cpu.same_bits(mu3, mu_b) and cpu.same_bits(cov3, cov_b) and cpu.same_bits(ll3, ll_b)
    rc, wi, mui, covi = be.init(z, 2)
    rc, w_b, mu_b, cov_b, ll_b = be.fit(z, 2, 1e-6, wi, mui, covi)
    w2, mu2, cov2, ll2 = wh.gmm_fit(wide[:, 1:4], 2, n_iter=2)
    assert rc == 0 and cpu.same_bits(w2, w_b) and cpu.same_bits(mu2, mu_b) and cpu.same_bits(cov2, cov_b) and cpu.same_bits(ll2, ll_b)
    with pytest.raises(RuntimeError, match="starved"):
        wh.gmm_fit(wide[:, 1:4], 3, n_iter=2, init=([0.4, 0.4, 0.2], np.vstack([mu0, [[500.0] * 3]]), np.stack([np.eye(3) * 4] * 3)))


# ---- the tools -----------------------------------------------------------------------------------------------------------
def test_tools_vc_train_and_vc_convert_end_to_end(wh, tmp_path):
    """two synthetic speakers: vowels at 16 kHz, 0.5 s each, order 24, and the same cepstra through a fixed affine map.  The
    conversion of the training source must come well below the unconverted distance to the target (converted < half of
    unconverted: test_gmm_cpu.py checks that the NumPy restatement meets this on the same input), and the converted .mgc
    drops into features-synthesis."""
    from world_amd import synth, tools
    dim = cpu.VC_ORDER + 1
    wavs = []
    for seed, base in cpu.VC_UTTERANCES:
        q = np.round(synth.vowel(cpu.VC_FS, 0.5, seed=seed, base_f0=base).numpy() * 32768).clip(-32768, 32767).astype("<i2")
        wavs.append(write_wav(str(tmp_path / f"src{seed}.wav"), q, cpu.VC_FS))
    tools.main(["features", *wavs, "--outdir", str(tmp_path), "--order", str(cpu.VC_ORDER)])
    src = [str(tmp_path / f"src{seed}.mgc") for seed, _ in cpu.VC_UTTERANCES]
    tgt = [str(tmp_path / f"tgt{seed}.mgc") for seed, _ in cpu.VC_UTTERANCES]
    for s, t in zip(src, tgt):
        cpu.vc_target(np.fromfile(s, dtype="<f4").reshape(-1, dim)).tofile(t)
    model = str(tmp_path / "model.npz")
    tools.main(["vc-train", *src, "--target", *tgt, "--dim", str(dim), "--mix", str(cpu.VC_MIX), "--iter", str(cpu.VC_ITER), "-o", model])
    with np.load(model) as f:
        assert f["w"].shape == (cpu.VC_MIX,) and f["mu"].shape == (cpu.VC_MIX, 4 * dim) and f["cov"].shape == (cpu.VC_MIX, 4 * dim, 4 * dim)
        assert int(f["dim"]) == dim and int(f["dx"]) == 2 * dim and np.all(np.diff(f["loglik"]) >= 0)
    before, after = [], []
    for seed, s, t in zip((u[0] for u in cpu.VC_UTTERANCES), src, tgt):
        out = str(tmp_path / f"conv{seed}.mgc")
        tools.main(["vc-convert", model, s, "--dim", str(dim), "-o", out])
        a, b, c = (np.fromfile(p, dtype="<f4").reshape(-1, dim) for p in (s, t, out))
        assert c.shape == a.shape and np.all(np.isfinite(c))
        before.append(cpu.mcd_db(a, b))
        after.append(cpu.mcd_db(c, b))
    print(f"MCD to the target: {np.mean(before):.3f} dB unconverted, {np.mean(after):.3f} dB converted")
    assert np.mean(after) < 0.5 * np.mean(before)
    seed = cpu.VC_UTTERANCES[0][0]
    stem, wav = str(tmp_path / f"src{seed}"), str(tmp_path / "converted.wav")
    n = np.fromfile(stem + ".lf0", dtype="<f4").size
    tools.main(["features-synthesis", stem + ".lf0", str(tmp_path / f"conv{seed}.mgc"), stem + ".bap", "--fs", str(cpu.VC_FS), "--order",
                str(cpu.VC_ORDER), "-o", wav])
    with wave.open(wav) as f:
        assert f.getframerate() == cpu.VC_FS and f.getnframes() == int(n * 5.0 / 1000.0 * cpu.VC_FS)
        assert np.abs(np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int32)).max() > 30
    with pytest.raises(SystemExit, match="as many"):
        tools.main(["vc-train", *src, "--target", tgt[0], "--dim", str(dim), "-o", model])
    with pytest.raises(SystemExit, match="trained on"):
        tools.main(["vc-convert", model, src[0], "--dim", str(dim + 1), "-o", str(tmp_path / "x")])
