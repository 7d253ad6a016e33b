"""The spectral path where fft_size is NOT the natural size of the sampling rate.

fft_size is a caller's argument on every spectral entry point, and callers use it (1024 bins at 48 kHz; 2048 at 16, 22.05
and 24 kHz; 512 at 16 kHz).  The rest of the suite takes cheaptrick_fft_size(fs), so every kernel template is otherwise
only run at the one rate that leads to it by default.  What changes when fs and fft_size part ways is what the kernels
index with: CheapTrick's floor 3 fs / (fft - 3) (which frames fall to the 500 Hz default, how long the longest window
is), the smoothing segment's bounds, Synthesis' lowest_f0 = fs / fft_size + 1 (integer division), the per-(fs, fft)
tables of d4c_finish and the coders.

Criterion: tests/util.py (e_H against the long double oracle W, bounded by ACC_A e_R + ACC_C ulp), unchanged.  Every case
asserts the kernel that ran and log2(fft_size), which selects the template.  Pairs (fs, fft_size) the reference leaves
undefined are only ever REFUSED here: none is launched.

The F0 kinds per CheapTrick pair are chosen, not exhaustive: every pair runs `floor_edge` and, where the rate lets Harvest
find a contour in so short a signal, Harvest's own F0, plus ONE caller-made track picked for what the pair stresses (`low`
where the floor is low enough for 20-90 Hz windows to be long, `nyquist` where the smoothing segment is widest, `steps`
elsewhere).  Between them the nine pairs cover all five kinds.
"""
import math

import numpy as np
import pytest

from util import ACC_A, ACC_C, assert_accurate, ct_floor, discrete_agreement, lowest_f0  # noqa: F401
from util import offdefault_f0 as _f0, offdefault_seconds as _seconds, synth_inputs as _synth_inputs, utterance as _signal

pytestmark = pytest.mark.gpu

assert (ACC_A, ACC_C) == (4.0, 64.0)


@pytest.fixture(scope="module")
def wide():
    from oracle.loader import WideOracle, wide_is_wider
    if not wide_is_wider():
        pytest.skip(f"long double is not wider than double on this host (eps {np.finfo(np.longdouble).eps})")
    return WideOracle()


@pytest.fixture(scope="module")
def wh():
    import torch
    assert torch.cuda.is_available(), "this test needs the MI355X"
    from world_amd.api import WorldHip
    return WorldHip()


def _gpu(wh, fn):
    """run fn on the GPU under the kernel profiler: (fn's result as numpy, {kernel name: launches})"""
    import torch
    out = []
    prof = wh.profile(lambda: out.append(fn()))
    torch.cuda.synchronize()
    res = out[0]
    res = tuple(r.cpu().numpy() if hasattr(r, "cpu") else r for r in res) if isinstance(res, tuple) else res.cpu().numpy()
    return res, {k: len(v) for k, v in prof.items()}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _lg(n):
    lg = int(round(math.log2(n)))
    assert 1 << lg == n
    return lg


def d4c_exit_rows(ap):
    return np.all(np.asarray(ap) == 1.0 - 1e-12, axis=1)


def _check_d4c(what, h, r, w):
    w_only = discrete_agreement(f"{what} LoveTrain exits", d4c_exit_rows(h), d4c_exit_rows(r), d4c_exit_rows(w))
    assert_accurate(what, h, r, w, exclude_rows=w_only)


# ---------------------------------------------------------------- refusals: the pairs the reference leaves undefined
def test_batched_entry_points_refuse_undefined_pairs(wh):
    """run_cheaptrick, run_synthesis and the real-time create call refuse, with the smallest fft_size that works, BEFORE
    anything is uploaded or launched (nothing of such a pair ever runs on the GPU), and the context works afterwards"""
    import torch
    nf = 8
    tp, f0 = _dev(np.arange(nf) * 0.005)[None], _dev([0, 0, 150, 160, 0, 170, 0, 0])[None]
    for fs, fft, smallest in ((48000, 256, 512), (192000, 1024, 2048), (44100, 256, 512)):
        x = _dev(_signal(fs, 0.04))[None]
        with pytest.raises(RuntimeError, match=f"smallest fft_size for this fs is {smallest}"):
            wh.cheaptrick(x, fs, tp, f0, [nf], fft_size=fft)
        why = __import__("ctypes").create_string_buffer(256)
        assert wh.lib.world_hip_check_shape(fs, fft, why, 256) == 1 and b"CheapTrick" in why.value
    for fs, fft, smallest in ((96000, 128, 256), (192000, 256, 512)):
        nb = fft // 2 + 1
        sp, ap = _dev(np.full((1, nf, nb), 1e-4)), _dev(np.full((1, nf, nb), 0.5))
        with pytest.raises(RuntimeError, match=f"smallest fft_size for this fs is {smallest}"):
            wh.synthesis(f0, sp, ap, nf, fft, 5.0, fs, int(fs * 0.03))
        with pytest.raises(RuntimeError, match=f"smallest fft_size for this fs is {smallest}"):
            wh.realtime(1, fs, 5.0, fft, 64, 8)
    # the pairs next to them are served
    for fs, fft in ((48000, 512), (192000, 2048), (16000, 128)):
        x = _dev(_signal(fs, 0.04))[None]
        sp = wh.cheaptrick(x, fs, tp, f0, [nf], fft_size=fft)
        assert bool(torch.isfinite(sp).all()) and bool((sp > 0).all())
    wh.realtime(1, 96000, 5.0, 256, 64, 8).close()


# ---------------------------------------------------------------- CheapTrick: ct_frame<PER, LGN, T> by lg = log2(fft_size)
CT_CASES = [  # fs, fft, f0 kinds, lg and the template it selects
    (8000, 128, ("harvest", "floor_edge", "steps"), 7),       # generic <8, 0, 128>: the smallest transform
    (16000, 128, ("harvest", "floor_edge", "nyquist"), 7),    # floor 384 Hz: speech F0 lies below the floor
    (16000, 256, ("harvest", "floor_edge", "low"), 8),        # generic
    (48000, 512, ("harvest", "floor_edge", "steps"), 9),      # generic, at 4.4 times its usual rate
    (48000, 1024, ("harvest", "floor_edge", "nyquist"), 10),  # <8, 10, 128>: PER * threads = N, the window fills the registers
    (16000, 2048, ("harvest", "floor_edge", "steps"), 11),    # <8, 11, 256>: the TTS setting
    (22050, 4096, ("harvest", "floor_edge", "low"), 12),      # <16, 12, 256>
    (16000, 8192, ("low", "floor_edge"), 13),                 # <16, 0, 512>: floor 5.9 Hz, a 2401-sample window at 20 Hz
    (192000, 2048, ("harvest", "floor_edge", "steps"), 11),   # <8, 11, 256>: floor 282 Hz at the top rate
]


@pytest.mark.parametrize("fs,fft,kinds,lg", CT_CASES)
def test_cheaptrick_off_default(wh, ref_oracle, wide, fs, fft, kinds, lg):
    assert _lg(fft) == lg and fft != ref_oracle.cheaptrick_fft_size(fs)
    assert 2 * int(1.5 * fs / 500.0 + 0.5) + 1 <= fft                 # the pair is one the reference defines
    x = _signal(fs, _seconds(fs))
    floor = ct_floor(fs, fft)
    for kind in kinds:
        tp, f0 = _f0(kind, ref_oracle, x, fs, fft)
        nf = len(tp)
        if kind == "floor_edge":                                       # both sides of the floor, on adjacent frames
            assert np.any(f0 <= floor) and np.any(f0 > floor)
            assert 2 * int(1.5 * fs / f0[f0 > floor].min() + 0.5) + 1 >= fft - 3     # the longest window the size admits
        sp, prof = _gpu(wh, lambda: wh.cheaptrick(_dev(x)[None], fs, _dev(tp)[None], _dev(f0)[None], [nf], fft_size=fft))
        assert prof.get("ct_frame") == 1, prof
        assert sp.shape[-1] == fft // 2 + 1
        r = ref_oracle.cheaptrick(x, fs, tp, f0, fft_size=fft)
        w = wide.cheaptrick(x, fs, tp, f0, fft_size=fft)
        assert_accurate(f"cheaptrick off-default lg{lg} {fs}/{fft} {kind}", sp[0, :nf], r, w)


# ---------------------------------------------------------------- D4C: d4c_finish's output grid is the caller's fft_size
D4C_CASES = [(16000, 128, "harvest"), (16000, 8192, "steps"), (48000, 512, "harvest"), (48000, 16384, "steps"),
             (192000, 1024, "harvest")]


@pytest.mark.parametrize("threshold", [0.85, 0.0])
@pytest.mark.parametrize("fs,fft,kind", D4C_CASES)
def test_d4c_off_default(wh, ref_oracle, wide, fs, fft, kind, threshold):
    assert fft != ref_oracle.cheaptrick_fft_size(fs)
    x = _signal(fs, _seconds(fs))
    tp, f0 = _f0(kind, ref_oracle, x, fs, fft)
    nf = len(tp)
    ap, prof = _gpu(wh, lambda: wh.d4c(_dev(x)[None], fs, _dev(tp)[None], _dev(f0)[None], [nf], fft, threshold=threshold))
    assert prof.get("d4c_lovetrain") == 1 and prof.get("d4c_frame") == 1 and prof.get("d4c_finish") == 1, prof
    assert ap.shape[-1] == fft // 2 + 1
    r = ref_oracle.d4c(x, fs, tp, f0, fft, threshold=threshold)
    w = wide.d4c(x, fs, tp, f0, fft, threshold=threshold)
    _check_d4c(f"d4c off-default lg{_lg(fft)} {fs}/{fft} {kind} th={threshold}", ap[0, :nf], r, w)


def test_d4c_grids_nest_bit_for_bit(wh, ref_oracle):
    """no oracle: bin i of the fft_size N grid and bin 2 i of the 2 N grid lie at the same double i fs / N, so d4c_finish's
    knot and weight are the same and ap_2N[:, ::2] == ap_N bit for bit -- unless a table is keyed on less than (fs, fft)"""
    fs = 48000
    x = _signal(fs, 0.2)
    tp, f0 = ref_oracle.harvest(x, fs)
    assert np.any(f0 > 0)
    nf = len(tp)
    ap = {}
    for fft in (512, 1024, 2048, 1024, 512):                            # and back down: a cached grid must follow the size
        got = wh.d4c(_dev(x)[None], fs, _dev(tp)[None], _dev(f0)[None], [nf], fft).cpu().numpy()[0, :nf]
        if fft in ap:
            assert np.array_equal(got, ap[fft])
        ap[fft] = got
    assert not np.all(d4c_exit_rows(ap[512]))
    assert np.array_equal(ap[1024][:, ::2], ap[512]) and np.array_equal(ap[2048][:, ::2], ap[1024])


# ---------------------------------------------------------------- Synthesis: sy_pulse<4096> / <8192>, lowest_f0 = fs / fft + 1
# sy_pulse<NMAX>: 4096 up to fft_size 4096, 8192 beyond, where the pulse keeps its spectrum (complex) in its response slot
# -- the launcher picks it from lg alone (api.hip run_synthesis: resp_stride).  The profile reports the kernel's name, not its
# template arguments, so the template is pinned through lg, as for ct_frame.
SY_CASES = [(16000, 128, 4096), (16000, 256, 4096), (48000, 512, 4096), (48000, 1024, 4096), (16000, 4096, 4096),
            (16000, 8192, 8192), (48000, 8192, 8192)]


@pytest.mark.parametrize("fs,fft,nmax", SY_CASES)
def test_synthesis_off_default(wh, ref_oracle, wide, fs, fft, nmax):
    assert (8192 if _lg(fft) > 12 else 4096) == nmax and fft != ref_oracle.cheaptrick_fft_size(fs)
    assert fs // 500 + 1 <= fft
    x, f0, sp, ap = _synth_inputs(ref_oracle, fs, fft, 0.2)
    nf = len(f0)
    y, prof = _gpu(wh, lambda: wh.synthesis(_dev(f0)[None], _dev(sp)[None], _dev(ap)[None], nf, fft, 5.0, fs, len(x)))
    assert prof.get("sy_pulse") == 1, prof
    r = ref_oracle.synthesis(f0, sp, ap, fft, 5.0, fs, len(x))
    w = wide.synthesis(f0, sp, ap, fft, 5.0, fs, len(x))
    assert np.max(np.abs(r)) > 0
    assert_accurate(f"synthesis off-default sy_pulse<{nmax}> {fs}/{fft}", y[0, None, : len(x)], r[None], w[None], peak=True)


def test_synthesis_ragged_batch_equals_lone_calls(wh, ref_oracle):
    fs, fft = 48000, 1024
    a = _synth_inputs(ref_oracle, fs, fft, 0.2, 2)
    b = _synth_inputs(ref_oracle, fs, fft, 0.13, 3)
    nfs, ys = [len(a[1]), len(b[1])], [len(a[0]), len(b[0])]
    F, nb = max(nfs), fft // 2 + 1
    f0, sp, ap = np.zeros((2, F)), np.ones((2, F, nb)), np.ones((2, F, nb))
    for u, c in enumerate((a, b)):
        f0[u, : nfs[u]], sp[u, : nfs[u]], ap[u, : nfs[u]] = c[1], c[2], c[3]
    y = wh.synthesis(_dev(f0), _dev(sp), _dev(ap), nfs, fft, 5.0, fs, ys).cpu().numpy()
    for u, c in enumerate((a, b)):
        lone = wh.synthesis(_dev(c[1])[None], _dev(c[2])[None], _dev(c[3])[None], nfs[u], fft, 5.0, fs, ys[u]).cpu().numpy()
        assert np.any(lone != 0) and np.array_equal(y[u, : ys[u]], lone[0])


# ---------------------------------------------------------------- one context, changing pairs
def _all_stages(wh, x, tp, f0, fs, fft):
    nf = len(tp)
    xd, td, fd = _dev(x)[None], _dev(tp)[None], _dev(f0)[None]
    sp = wh.cheaptrick(xd, fs, td, fd, [nf], fft_size=fft)
    ap = wh.d4c(xd, fs, td, fd, [nf], fft)
    mc = wh.code_spectral_envelope(sp[0], fs, fft, 24)
    bap = wh.code_aperiodicity(ap[0], fs, fft)
    out = [sp, ap, mc, bap, wh.decode_spectral_envelope(mc, fs, fft), wh.decode_aperiodicity(bap, fs, fft),
           wh.synthesis(fd, sp, ap, nf, fft, 5.0, fs, len(x))]
    return [o.cpu().numpy() for o in out]


def test_one_context_across_changing_pairs(ref_oracle):
    """CheapTrick, D4C, both coders, both decoders and Synthesis on ONE context as (fs, fft_size) changes and comes back:
    each result is bit-identical to a fresh context's -- the cached aperiodicity grid, coder tables, DC remover and Nuttall
    window must follow both numbers, and tables must grow and shrink"""
    from world_amd.api import WorldHip
    wh = WorldHip()
    inputs = {}
    for fs, fft in ((16000, 1024), (16000, 2048), (48000, 1024), (16000, 1024)):
        if fs not in inputs:
            x = _signal(fs, 0.15)
            inputs[fs] = (x,) + tuple(ref_oracle.harvest(x, fs))
        x, tp, f0 = inputs[fs]
        got = _all_stages(wh, x, tp, f0, fs, fft)
        fresh_ctx = WorldHip()
        fresh = _all_stages(fresh_ctx, x, tp, f0, fs, fft)
        fresh_ctx.close()
        for name, g, f in zip(("sp", "ap", "mc", "bap", "sp decoded", "ap decoded", "y"), got, fresh):
            assert np.isfinite(g).all() and np.array_equal(g, f), (fs, fft, name)
    wh.close()


# ---------------------------------------------------------------- record layouts and the fused coders
@pytest.mark.parametrize("fs,fft", [(48000, 1024), (16000, 4096)])
def test_layouts_and_fused_coders_off_default(fs, fft):
    """analyze_packed on both wires equals the dense rows (f32: rounded once); analyze_coded equals the stand-alone coders
    on the dense rows bit for bit (the bound tests/test_codec.py holds 48 kHz / 2048 to), also at the largest
    number_of_dimensions accepted, fft_size / 4 + 1"""
    import torch
    from world_amd.api import WorldHip
    wh = WorldHip()
    nb = fft // 2 + 1
    lens = [int(0.2 * fs), int(0.13 * fs) + 7]
    x = torch.zeros((2, max(lens)), dtype=torch.float64)
    for u, n in enumerate(lens):
        x[u, :n] = torch.from_numpy(_signal(fs, 0.2, 2 + u)[:n])
    x = x.cuda().contiguous()
    tp, f0, sp, ap, nf = wh.analyze(x, fs, x_len=lens, fft_size=fft)
    assert sp.shape[-1] == nb and bool((f0 > 0).any())
    nf = [int(n) for n in nf]
    rows = sum(nf)
    for cols in (2 + 2 * nb, 2 + nb):
        block = torch.full((rows + 3, cols), -7.0, dtype=torch.float64, device="cuda")
        assert wh.analyze_packed(x, fs, block, first_row=2, x_len=lens, fft_size=fft) == nf
        torch.cuda.synchronize()
        assert torch.all(block[:2] == -7.0) and torch.all(block[2 + rows:] == -7.0)
        row = 2
        for u, n in enumerate(nf):
            rec = block[row:row + n]
            row += n
            assert torch.equal(rec[:, 0], tp[u, :n]) and torch.equal(rec[:, 1], f0[u, :n])
            if cols == 2 + 2 * nb:
                assert torch.equal(rec[:, 2:2 + nb], sp[u, :n]) and torch.equal(rec[:, 2 + nb:], ap[u, :n])
            else:
                narrow = rec[:, 2:].contiguous().view(torch.float32).reshape(n, -1)[:, : 2 * nb]
                assert torch.equal(narrow[:, :nb], sp[u, :n].float()) and torch.equal(narrow[:, nb:], ap[u, :n].float())
    for nd in (24, fft // 4 + 1):
        cols = wh.lib.world_hip_coded_columns(fs, nd)
        block = torch.full((rows + 2, cols), float("nan"), dtype=torch.float64, device="cuda")
        assert wh.analyze_coded(x, fs, block, first_row=1, x_len=lens, number_of_dimensions=nd, fft_size=fft) == nf
        torch.cuda.synchronize()
        assert bool(torch.isnan(block[0]).all()) and bool(torch.isnan(block[-1]).all())
        row = 1
        for u, n in enumerate(nf):
            rec = block[row:row + n]
            row += n
            assert torch.equal(rec[:, 2:2 + nd], wh.code_spectral_envelope(sp[u, :n], fs, fft, nd))
            assert torch.equal(rec[:, 2 + nd:], wh.code_aperiodicity(ap[u, :n], fs, fft))
    wh.close()
