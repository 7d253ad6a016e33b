"""Dynamic features and parameter generation on the MI355X (include/world_hip.h: world_hip_delta_batch /
world_hip_mlpg_batch): the cases of test_mlpg_cpu.py through the shipped library -- there 64 systems share a wavefront, the
observations are read ahead through register rings and the windows come from LDS, none of which the one-lane emulation
exercises -- then graph replay, the Python layer and the tools.  The bounds are test_mlpg_cpu.py's.
Measured on one MI355X: omega <= 2.63 * 2^-53 over the accuracy cases (the emulation's figures to the digit: fma() is the
fused operation in both); round trip 8.9e-16 = 8 * 2^-53 against scipy.linalg.solveh_banded's 1.8e-15 = 16 * 2^-53."""
import os
import wave

import numpy as np
import pytest

import test_mlpg_cpu as cpu
from backends import OnGpu, gpu_backend, wh, write_wav  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


# ---- the cases of the CPU file -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,D,wname,strided", cpu.DELTAS, ids=cpu.DELTA_IDS)
def test_deltas_are_the_statement(be, lens, D, wname, strided):
    """(the float64 restatement the emulation is held to as well: the GPU and the emulation agree bit for bit)"""
    cpu.case_deltas(be, lens, D, wname, strided)


_omegas = []


@pytest.mark.parametrize("lens,D,wname,kind,precision,s,strided", cpu.ACCURACY, ids=cpu.ACCURACY_IDS)
def test_generation_backward_error(be, lens, D, wname, kind, precision, s, strided):
    _omegas.append(cpu.case_accuracy(be, lens, D, wname, kind, precision, s, strided))
    print(f"largest omega so far: {max(_omegas) / cpu.U53:.2f} * 2^-53")


def test_generation_inverts_the_deltas(be):
    cpu.case_round_trip(be)


@pytest.mark.parametrize("wname", ["three", "five"])
@pytest.mark.parametrize("pattern", list(cpu.MASKS))
def test_a_run_of_present_frames_is_an_utterance_of_its_own(be, pattern, wname):
    cpu.case_mask(be, pattern, wname)


@pytest.mark.parametrize("wname", ["static", "three", "five"])
def test_a_column_depends_on_nothing_but_the_column(be, wname):
    """(column 64 of 130 is lane 0 of the second wavefront, 129 sits in the ragged third)"""
    cpu.case_independence(be, wname)


@pytest.mark.parametrize("wname", ["static", "three", "five"])
def test_a_poisoned_column_spoils_nothing_else(be, wname):
    cpu.case_poison(be, wname)


def test_refusals_write_nothing_and_give_a_reason(be):
    cpu.case_refusals(be)


def test_workspace_grows_once(be):
    cpu.case_workspace(be)


# ---- graph replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", ["static", "three", "five"])
def test_a_captured_call_equals_the_eager_one(wname):
    """after one eager call of the shape (the workspace then has the size, the frame counts are on the device) both
    calls can be captured, and the replay gives the eager bits"""
    import torch
    from world_amd.api import WorldHip
    rng = np.random.default_rng(41)
    win = cpu.WINDOWS[wname]
    n_win, lens, D = win.shape[0], (67, 30), 65
    T = max(lens)
    present = rng.random((2, T)) < 0.9
    w = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            b = GpuBackend(w)
            d_c = b.dev(rng.standard_normal((2, T, D)))
            d_mean, d_var = b.dev(rng.standard_normal((2, T, n_win * D))), b.dev(cpu.spread(rng, 3, (2, T, n_win * D)))
            d_mask = b.dev(present.astype(np.uint8))
            d_dl, d_gen = b.dev(np.full((2, T, n_win * D), cpu.SENTINEL)), b.dev(np.full((2, T, D), cpu.SENTINEL))

            def call():
                w._check(b.call_delta(2, D, win, lens, b.addr(d_mask), T, b.addr(d_c), T * D, D, cpu.FILL, b.addr(d_dl),
                                      T * n_win * D, n_win * D), "delta")
                w._check(b.call_mlpg(2, D, win, lens, b.addr(d_mask), T, b.addr(d_mean), T * n_win * D, n_win * D, b.addr(d_var),
                                     T * n_win * D, n_win * D, 0, cpu.FILL, b.addr(d_gen), T * D, D), "mlpg")
            call()
            torch.cuda.synchronize()
            eager = b.host(d_dl), b.host(d_gen)
            assert np.all(eager[0][0] != cpu.SENTINEL) and np.all(eager[1][1, 30:] == cpu.SENTINEL)
            g = w.capture(call)
            d_dl.fill_(cpu.SENTINEL)
            d_gen.fill_(cpu.SENTINEL)
            g.launch()
            torch.cuda.synchronize()
            assert cpu.same_bits(b.host(d_dl), eager[0]) and cpu.same_bits(b.host(d_gen), eager[1])
    finally:
        if g is not None:
            g.close()
        w.close()


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_worldhip_deltas_and_mlpg_honour_lengths_strides_and_layouts(wh, be):
    import torch
    rng = np.random.default_rng(43)
    lens, D, T = (40, 67, 9), 65, 67
    c = [rng.standard_normal((n, D)) for n in lens]
    masks = [rng.random(n) < 0.85 for n in lens]
    want_dl = be.deltas(c, cpu.W3, masks=masks)
    # [U][T][D] inside a wider tensor: utterance and row strides of the view
    big = torch.full((3, T + 2, D + 7), cpu.SENTINEL, dtype=torch.float64, device=wh.device)
    mask = torch.zeros((3, T), dtype=torch.bool, device=wh.device)
    for u, n in enumerate(lens):
        big[u, :n, 3:3 + D] = torch.from_numpy(c[u]).to(wh.device)
        mask[u, :n] = torch.from_numpy(masks[u]).to(wh.device)
    out = torch.full((3, T, 3 * D + 1), cpu.SENTINEL, dtype=torch.float64, device=wh.device)
    got = wh.deltas(big[:, :T, 3:3 + D], mask=mask, fill=cpu.FILL, n_frames=lens, out=out[:, :, :3 * D])
    assert got.data_ptr() == out.data_ptr()
    for u, n in enumerate(lens):
        assert cpu.same_bits(out[u, :n, :3 * D].cpu().numpy(), want_dl[u])
        assert bool((out[u, n:] == cpu.SENTINEL).all()) and bool((out[u, :, 3 * D:] == cpu.SENTINEL).all())
    # generation: per-frame, per-utterance and global variances, the precision flag, one utterance as [T][cols]
    mean = [rng.standard_normal((n, 3 * D)) for n in lens]
    var = [cpu.spread(rng, 3, (n, 3 * D)) for n in lens]
    d_mean = torch.zeros((3, T, 3 * D), dtype=torch.float64, device=wh.device)
    d_var = torch.ones((3, T, 3 * D), dtype=torch.float64, device=wh.device)
    for u, n in enumerate(lens):
        d_mean[u, :n] = torch.from_numpy(mean[u]).to(wh.device)
        d_var[u, :n] = torch.from_numpy(var[u]).to(wh.device)
    got = wh.mlpg(d_mean, d_var, mask=mask, fill=cpu.FILL, n_frames=lens)
    want = be.mlpg(mean, var, cpu.W3, masks=masks)
    for u, n in enumerate(lens):
        assert cpu.same_bits(got[u, :n].cpu().numpy(), want[u])
    per_utt = [v[0] for v in var]
    got = wh.mlpg(d_mean, torch.from_numpy(np.stack(per_utt)).to(wh.device), n_frames=lens, precision=True)
    want = be.mlpg(mean, per_utt, cpu.W3, precision=True)
    for u, n in enumerate(lens):
        assert cpu.same_bits(got[u, :n].cpu().numpy(), want[u])
    got = wh.mlpg(d_mean[1], torch.from_numpy(per_utt[0]).to(wh.device), windows=cpu.W5)
    assert got.shape == (T, D) and cpu.same_bits(got.cpu().numpy(), be.mlpg([mean[1]], per_utt[0], cpu.W5)[0])
    # the round trip through the defaults
    x = torch.from_numpy(c[1]).to(wh.device)
    dyn = wh.deltas(x)
    assert cpu.same_bits(dyn.cpu().numpy(), be.deltas([c[1]], cpu.W3)[0])
    back = wh.mlpg(dyn, d_var[1, :1])
    assert cpu.same_bits(back.cpu().numpy(), be.mlpg([dyn.cpu().numpy()], var[1][0], cpu.W3)[0])
    with pytest.raises(RuntimeError, match="identity"):
        wh.deltas(x, windows=[[0.5], [-0.5, 0.0, 0.5]])
    with pytest.raises(RuntimeError, match="overlap"):
        wh.deltas(big[0, :T, 0:2], out=big[0, :T, 2:8])
    with pytest.raises(ValueError):
        wh.mlpg(d_mean[:, :, :3 * D - 1], d_var[:, :, :3 * D - 1])


# ---- the tools -----------------------------------------------------------------------------------------------------------
FS, ORDER = 16000, 24


def test_tools_features_deltas_mlpg_and_back_to_audio(wh, tmp_path):
    from world_amd import synth, tools
    q = np.round(synth.vowel(FS, 0.5, seed=3).numpy() * 32768).clip(-32768, 32767).astype("<i2")
    q[-int(0.15 * FS):] = 0                                                  # unvoiced frames as well
    q[:int(0.05 * FS)] = 0
    path = write_wav(str(tmp_path / "vowel.wav"), q, FS)
    tools.main(["features", path, "--outdir", str(tmp_path), "--order", str(ORDER)])
    stem = str(tmp_path / "vowel")
    mgc, lf0 = np.fromfile(stem + ".mgc", dtype="<f4").reshape(-1, ORDER + 1), np.fromfile(stem + ".lf0", dtype="<f4")
    n, dim = len(lf0), ORDER + 1
    voiced = lf0 > -1e9
    assert np.any(voiced) and np.any(~voiced)
    tools.main(["deltas", stem + ".mgc", "--dim", str(dim), "-o", stem + ".mgc.dyn"])
    tools.main(["deltas", stem + ".lf0", "--lf0", "-o", stem + ".lf0.dyn"])
    dyn, ldyn = np.fromfile(stem + ".mgc.dyn", dtype="<f4").reshape(n, 3 * dim), np.fromfile(stem + ".lf0.dyn", dtype="<f4").reshape(n, 3)
    assert np.array_equal(dyn[:, :dim], mgc) and np.array_equal(ldyn[:, 0], lf0)
    assert np.all(ldyn[~voiced] == np.float32(-1e10)) and np.all(ldyn[voiced] > -1e9)
    assert np.allclose(dyn[1:-1, dim:2 * dim], 0.5 * (mgc[2:] - mgc[:-2]), atol=1e-6)
    # one row of variances for the whole file, any positive ones: the observations are consistent up to their rounding to
    # float32, d_mu <= 2^-25 |mu| each.  c - c* = R^-1 W' P d_mu and R >= P_static >= p_min I, so
    # |c - c*| <= ||.||_2 <= sqrt(p_max / p_min) sqrt(3 n) max |d_mu|; the result is rounded to float32 once more.
    rng = np.random.default_rng(47)
    rng.uniform(0.5, 2.0, 3 * dim).astype("<f4").tofile(stem + ".mgc.var")
    rng.uniform(0.5, 2.0, 3).astype("<f4").tofile(stem + ".lf0.var")
    out = tmp_path / "gen"
    os.makedirs(out)
    tools.main(["mlpg", stem + ".mgc.dyn", stem + ".mgc.var", "--dim", str(dim), "-o", str(out / "vowel.mgc")])
    tools.main(["mlpg", stem + ".lf0.dyn", stem + ".lf0.var", "--lf0", "-o", str(out / "vowel.lf0")])
    mgc2, lf02 = np.fromfile(str(out / "vowel.mgc"), dtype="<f4").reshape(n, dim), np.fromfile(str(out / "vowel.lf0"), dtype="<f4")

    def tolerance(var_file, observations, statics):
        v = np.fromfile(var_file, dtype="<f4").astype(np.float64)
        return (np.sqrt(v.max() / v.min()) * np.sqrt(3 * n) * float(np.abs(observations).max()) + float(np.abs(statics).max())) * 2.0 ** -25

    tol = tolerance(stem + ".mgc.var", dyn, mgc)
    print(f"mgc round trip: {float(np.abs(mgc2.astype(np.float64) - mgc).max()):.3e} (tolerance {tol:.3e})")
    assert np.all(np.abs(mgc2.astype(np.float64) - mgc) <= tol)
    assert np.array_equal(lf02 == np.float32(-1e10), ~voiced)
    tol = tolerance(stem + ".lf0.var", ldyn[voiced], lf0[voiced])
    print(f"lf0 round trip: {float(np.abs(lf02[voiced].astype(np.float64) - lf0[voiced]).max()):.3e} (tolerance {tol:.3e})")
    assert np.all(np.abs(lf02[voiced].astype(np.float64) - lf0[voiced]) <= tol)
    # a file of as many rows of variances is accepted too, and the result drops into features-synthesis
    np.tile(np.fromfile(stem + ".mgc.var", dtype="<f4"), n).tofile(stem + ".mgc.varT")
    tools.main(["mlpg", stem + ".mgc.dyn", stem + ".mgc.varT", "--dim", str(dim), "-o", str(out / "again.mgc")])
    assert np.array_equal(np.fromfile(str(out / "again.mgc"), dtype="<f4"), mgc2.reshape(-1))
    wav = str(tmp_path / "back.wav")
    tools.main(["features-synthesis", str(out / "vowel.lf0"), str(out / "vowel.mgc"), stem + ".bap", "--fs", str(FS), "--order", str(ORDER), "-o", wav])
    with wave.open(wav) as f:
        assert f.getframerate() == FS and f.getnframes() == int(n * 5.0 / 1000.0 * FS)
        assert np.abs(np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int32)).max() > 30
    with pytest.raises(SystemExit, match="multiple"):
        tools.main(["deltas", stem + ".mgc", "--dim", str(dim + 1), "-o", str(tmp_path / "x")])
    with pytest.raises(SystemExit, match="rows"):
        np.ones(2 * 3 * dim, dtype="<f4").tofile(stem + ".two")
        tools.main(["mlpg", stem + ".mgc.dyn", stem + ".two", "--dim", str(dim), "-o", str(tmp_path / "x")])
