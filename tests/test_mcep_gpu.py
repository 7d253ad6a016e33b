"""All-pass mel-cepstra on the MI355X (include/world_hip.h: world_hip_sp2mc / world_hip_mc2sp): the cases of
test_mcep_cpu.py through the shipped library -- there the sums run on v_mfma_f64_16x16x4_f64, whose lane maps only this file
exercises (the tables are asymmetric by nature: a row / column swap of the result map cannot pass the bounds) -- then graph
replay, the Python layer, the pipeline from a waveform and the tools."""
import os
import wave

import numpy as np
import pytest

import test_mcep_cpu as cpu
from backends import OnGpu, gpu_backend, wh, write_wav  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


# ---- the cases of the CPU file -------------------------------------------------------------------------------------------
def test_default_alpha_of_nine_rates(wh):
    cpu.case_alpha(wh.lib)
    assert wh.mcep_alpha(16000) == 0.41 and wh.mcep_alpha(48000) == 0.554
    with pytest.raises(ValueError):
        wh.mcep_alpha(0)


@pytest.mark.parametrize("fft_size,order,alpha", cpu.TABLE_SHAPES, ids=cpu.TABLE_IDS)
def test_tables_against_mpmath(wh, fft_size, order, alpha):
    cpu.case_tables(wh.lib, fft_size, order, alpha)


@pytest.mark.parametrize("fft_size,order,alpha", cpu.SHAPES, ids=cpu.SHAPE_IDS)
def test_encode_within_the_dot_product_bound(be, fft_size, order, alpha):
    cpu.case_encode(be, fft_size, order, alpha)


@pytest.mark.parametrize("fft_size,order,alpha", cpu.SHAPES, ids=cpu.SHAPE_IDS)
def test_decode_within_the_dot_product_bound(be, fft_size, order, alpha):
    cpu.case_decode(be, fft_size, order, alpha)


def test_full_order_unwarped_round_trip(be):
    cpu.case_round_trip(be)


@pytest.mark.parametrize("fft_size,order,alpha", [cpu.SHAPES[1], cpu.SHAPES[4]], ids=[cpu.SHAPE_IDS[1], cpu.SHAPE_IDS[4]])
def test_a_row_depends_on_nothing_but_the_row(be, fft_size, order, alpha):
    cpu.case_rows_are_independent(be, fft_size, order, alpha)


def test_refusals_write_nothing_and_name_the_argument(be):
    cpu.case_refusals(be)


def test_table_cache_turns_over(be):
    cpu.case_table_cache_turns_over(be)


def test_the_wide_kernels_agree_with_the_narrow_one(be):
    """65 .. 128 and 129 .. 256 coefficients run other instantiations (8 and 16 column tiles per wavefront): their first
    60 coefficients depend on the same table rows and the same sums as the 60-coefficient call's -- freqt's row m does not
    depend on the order -- so they are held to the same bound, and row 66 of 67 sits in the last, partial row tile"""
    fft_size, _, alpha = cpu.SHAPES[2]
    sp = cpu.envelopes(fft_size)
    for order in (100, 200):
        want, bound = cpu.encode_oracle(fft_size, order, alpha)
        got = be.run(False, sp, fft_size, order, alpha)
        err = np.abs(cpu.LD(got) - want)
        print(f"encode {fft_size}/{order}: max error / bound = {float(np.max(err / bound)):.4f}")
        assert np.all(err <= bound)
        assert cpu.same_bits(be.run(False, sp[66:67], fft_size, order, alpha), got[66:67])


# ---- graph replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", [False, True], ids=["sp2mc", "mc2sp"])
def test_a_captured_call_equals_the_eager_one(decode):
    """a shape that never ran cannot be captured (its table would have to be built and uploaded); after one eager call
    the captured call replays to the same bits"""
    import torch
    from world_amd.api import WorldHip
    fft_size, order, alpha = cpu.SHAPES[1]
    x = cpu.decode_inputs(fft_size, order, alpha) if decode else cpu.envelopes(fft_size)
    out_cols = fft_size // 2 + 1 if decode else order + 1
    w = WorldHip()
    s = torch.cuda.Stream()
    g = None
    try:
        with torch.cuda.stream(s):
            b = GpuBackend(w)
            d_in, d_out = b.dev(x), b.dev(np.full((len(x), out_cols + 2), cpu.SENTINEL))
            call = lambda: w._check(b.call(decode, len(x), fft_size, order, alpha, d_in.data_ptr(), x.shape[1],
                                           d_out.data_ptr(), out_cols + 2), "mcep")
            with pytest.raises(RuntimeError, match="never run before"):
                w.capture(call)
            call()
            torch.cuda.synchronize()
            eager = b.host(d_out)
            assert np.all(eager[:, :out_cols] != cpu.SENTINEL) and np.all(eager[:, out_cols:] == cpu.SENTINEL)
            g = w.capture(call)
            d_out.fill_(cpu.SENTINEL)
            g.launch()
            torch.cuda.synchronize()
            assert cpu.same_bits(b.host(d_out), eager)
    finally:
        if g is not None:
            g.close()
        w.close()


# ---- the Python layer, the pipeline and the tools ------------------------------------------------------------------------
FS, ORDER, SECONDS = 16000, 24, 0.5


@pytest.fixture(scope="module")
def vowel(wh, tmp_path_factory):
    """a 0.5 s, 16 kHz vowel as a 16-bit WAV file, read back the way the tools read it, analysed into packed records"""
    import torch
    from world_amd import synth
    from world_amd.api import cheaptrick_fft_size, frame_count
    path = str(tmp_path_factory.mktemp("mcep") / "vowel.wav")
    q = np.round(synth.vowel(FS, SECONDS, seed=3).numpy() * 32768).clip(-32768, 32767).astype("<i2")
    write_wav(path, q, FS)
    x = wh.wavread(path)[0]
    fft_size, n = cheaptrick_fft_size(FS, 71.0), frame_count(FS, x.numel(), 5.0)
    block = torch.zeros((n, wh.lib.world_hip_record_columns(fft_size, 0)), dtype=torch.float64, device=wh.device)
    assert list(wh.analyze_packed(x[None].contiguous(), FS, block)) == [n]
    return dict(path=path, x=x, n=n, fft_size=fft_size, block=block, samples=len(q))


def test_pipeline_from_packed_records_and_back_to_audio(wh, vowel):
    import torch
    n, fft_size, block = vowel["n"], vowel["fft_size"], vowel["block"]
    K, alpha = fft_size // 2 + 1, wh.mcep_alpha(FS)
    assert alpha == 0.41
    sp, ap, f0 = block[:, 2:2 + K], block[:, 2 + K:2 + 2 * K], block[:, 1]
    dense = wh.sp2mc(sp.contiguous(), ORDER, alpha)
    assert dense.shape == (n, ORDER + 1) and bool(torch.isfinite(dense).all())
    where_they_lie = wh.sp2mc(sp, ORDER, alpha)                                  # the view's row stride
    assert torch.equal(where_they_lie, dense)
    explicit = wh.sp2mc(block.view(-1)[2:], ORDER, alpha, row_stride=block.shape[1], rows=n, fft_size=fft_size)
    assert torch.equal(explicit, dense)
    # into coded-style records of the caller's: [tpos, f0, c0 .. c24, 5 bands]; nothing else of them is written
    records = torch.full((n, 2 + ORDER + 1 + 5), cpu.SENTINEL, dtype=torch.float64, device=wh.device)
    assert wh.sp2mc(sp, ORDER, alpha, out=records[:, 2:2 + ORDER + 1]) is not None
    assert torch.equal(records[:, 2:2 + ORDER + 1], dense)
    assert bool((records[:, :2] == cpu.SENTINEL).all()) and bool((records[:, 2 + ORDER + 1:] == cpu.SENTINEL).all())
    assert torch.equal(wh.sp2mc(sp.contiguous().reshape(1, n, K), ORDER, alpha), dense[None])   # leading dimensions are rows
    # ... and back: a smooth envelope close to the analysed one, and audio
    back = wh.mc2sp(dense, alpha, fft_size)
    assert back.shape == (n, K) and bool(torch.isfinite(back).all()) and bool((back > 0).all())
    assert torch.equal(wh.mc2sp(records[:, 2:2 + ORDER + 1], alpha, fft_size), back)
    y_length = int(n * 5.0 / 1000.0 * FS)
    y = wh.synthesis(f0[None].contiguous(), back[None], ap.contiguous()[None], np.array([n], dtype=np.int32), fft_size, 5.0,
                     FS, np.array([y_length], dtype=np.int32))
    assert y.shape == (1, y_length) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 1e-3
    with pytest.raises(RuntimeError, match="alpha"):
        wh.sp2mc(sp, ORDER, 0.95)
    with pytest.raises(RuntimeError, match="order"):
        wh.sp2mc(sp, 256, alpha)
    with pytest.raises(RuntimeError, match="overlap"):
        wh.sp2mc(block[:, 2:2 + K], ORDER, alpha, out=block[:, 2 + K:2 + K + ORDER + 1])


def test_features_tools_write_what_the_python_path_computes(wh, vowel, tmp_path, capsys):
    from world_amd import tools
    n, fft_size = vowel["n"], vowel["fft_size"]
    # the vowel, its last 0.15 s silent: the file has unvoiced frames as well
    with wave.open(vowel["path"]) as f:
        q = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").copy()
    q[-int(0.15 * FS):] = 0
    path = write_wav(str(tmp_path / "vowel.wav"), q, FS)
    tools.main(["features", path, "--outdir", str(tmp_path), "--order", str(ORDER)])
    stem = str(tmp_path / "vowel")
    _, f0, sp, ap, nf = wh.analyze(wh.wavread(path)[0][None].contiguous(), FS)
    assert int(nf[0]) == n
    want = wh.sp2mc(sp[0, :n], ORDER, wh.mcep_alpha(FS)).cpu().numpy().astype("<f4")
    mgc = np.fromfile(stem + ".mgc", dtype="<f4")
    assert mgc.size == n * (ORDER + 1) and np.array_equal(mgc.reshape(n, ORDER + 1), want)
    f0 = f0[0, :n].cpu().numpy()
    lf0 = np.fromfile(stem + ".lf0", dtype="<f4")
    assert lf0.size == n and np.any(f0 == 0) and np.any(f0 > 0)
    assert np.array_equal(lf0 == np.float32(-1e10), f0 == 0)
    assert np.array_equal(lf0[f0 > 0], np.log(f0[f0 > 0]).astype("<f4"))
    bap = np.fromfile(stem + ".bap", dtype="<f4")
    assert np.array_equal(bap.reshape(n, -1), wh.code_aperiodicity(ap[0, :n], FS, fft_size).cpu().numpy().astype("<f4"))
    out = str(tmp_path / "back.wav")
    tools.main(["features-synthesis", stem + ".lf0", stem + ".mgc", stem + ".bap", "--fs", str(FS), "--order", str(ORDER), "-o", out])
    with wave.open(out) as f:
        assert f.getframerate() == FS and f.getnframes() == int(n * 5.0 / 1000.0 * FS)
        assert np.abs(np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int32)).max() > 30
    # --alpha is honoured, and the MCD of a file with itself on these cepstra is zero along the diagonal
    tools.main(["features", path, "--outdir", str(tmp_path / "a"), "--order", "10", "--alpha", "0.35"])
    want = wh.sp2mc(sp[0, :n], 10, 0.35).cpu().numpy().astype("<f4")
    assert np.array_equal(np.fromfile(str(tmp_path / "a" / "vowel.mgc"), dtype="<f4").reshape(n, 11), want)
    capsys.readouterr()
    tools.main(["mcd", vowel["path"], vowel["path"], "--mcep", str(ORDER)])
    line = capsys.readouterr().out
    assert f"frames {n} {n} path " in line and " mcd 0.000000 dB" in line, line
    with pytest.raises(SystemExit, match="alpha"):
        tools.main(["features", vowel["path"], "--outdir", str(tmp_path / "b"), "--order", "10", "--alpha", "0.99"])
    assert not os.path.exists(tmp_path / "b" / "vowel.mgc")
