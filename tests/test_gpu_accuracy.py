"""Every dispatch branch of the spectral and F0 kernels, held to the accuracy criterion of tests/util.py.

CheapTrick, D4C, StoneMask and Synthesis are compared with the long double oracle W (oracle/libworld_oracle_wide.so):
the GPU's element-wise error against W must stay within ACC_A times the reference's own error against W, plus ACC_C ulp,
at the median, the 99th percentile and the maximum of every row and bin.  Harvest and DIO are discrete selection: they are
compared with the reference at 1e-10 relative, with identical voiced / unvoiced decisions.

Every case asserts the kernel route it ran (WorldHip.profile's kernel names, and the transform size that picks the
template), so that a dispatch change cannot move a case onto another kernel unnoticed.  F0 comes from the reference's own
Harvest and from caller-made tracks in the style of tests/fuzz_given_f0.py.
"""
import math
import os

import numpy as np
import pytest

from util import assert_accurate, assert_f0_tight, discrete_agreement

pytestmark = pytest.mark.gpu


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


def _signal(fs, seconds, index=2):
    from world_amd import synth
    return synth.utterance(index, fs, seconds).numpy()


def _track(kind, fs, nf, seed):
    """caller-made F0 tracks (tests/fuzz_given_f0.py): steps, 20-90 Hz, sparse, and up to 0.4999 fs"""
    rng = np.random.default_rng(seed)
    if kind == "steps":
        f0 = np.repeat(rng.uniform(60.0, 600.0, nf // 7 + 1), 7)[:nf]
    elif kind == "low":
        f0 = rng.uniform(20.0, 90.0, nf)
    elif kind == "sparse":
        f0 = np.where(rng.random(nf) < 0.3, rng.uniform(80.0, 400.0, nf), 0.0)
    else:                                                              # "nyquist": fills ct_seg_cap
        f0 = rng.uniform(0.3 * fs, 0.4999 * fs, nf)
    f0[rng.random(nf) < 0.15] = 0.0
    return f0


def _f0(kind, ref, x, fs):
    tp, f0 = ref.harvest(x, fs)
    return tp, (f0 if kind == "harvest" else _track(kind, fs, len(tp), fs + len(kind)))


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
    return int(round(math.log2(n)))


def d4c_exit_rows(ap):
    return np.all(np.asarray(ap) == 1.0 - 1e-12, axis=1)


def stonemask_outcome(out, f0):
    out, f0 = np.asarray(out), np.asarray(f0)
    return np.where(out == 0.0, 0, np.where(out == f0, 1, 2))


# ---------------------------------------------------------------- CheapTrick: ct_frame<PER, LGN, T> by lg = log2(fft_size)
CT_CASES = [  # fs, f0_floor, f0 kinds, lg
    (11025, 71.0, ("harvest", "low"), 9),            # generic <8, 0, 128>
    (16000, 71.0, ("harvest", "nyquist"), 10),
    (48000, 71.0, ("harvest", "steps"), 11),
    (48000, 40.0, ("harvest", "sparse"), 12),
    (96000, 71.0, ("harvest", "low"), 12),
    (128000, 71.0, ("harvest",), 13),
    (192000, 71.0, ("steps",), 13),
]


@pytest.mark.parametrize("fs,f0_floor,kinds,lg", CT_CASES)
def test_cheaptrick_accuracy(wh, ref_oracle, wide, fs, f0_floor, kinds, lg):
    x = _signal(fs, 0.2 if fs < 100000 else 0.12)
    fft = ref_oracle.cheaptrick_fft_size(fs, f0_floor)
    assert _lg(fft) == lg
    for kind in kinds:
        tp, f0 = _f0(kind, ref_oracle, x, fs)
        nf = len(tp)
        sp, prof = _gpu(wh, lambda: wh.cheaptrick(_dev(x)[None], fs, _dev(tp)[None], _dev(f0)[None], [nf],
                                                  f0_floor=f0_floor, fft_size=fft))
        assert prof.get("ct_frame") == 1, prof
        r = ref_oracle.cheaptrick(x, fs, tp, f0, f0_floor=f0_floor, fft_size=fft)
        w = wide.cheaptrick(x, fs, tp, f0, f0_floor=f0_floor, fft_size=fft)
        assert_accurate(f"cheaptrick lg{lg} {fs} {kind}", sp[0, :nf], r, w)


# ---------------------------------------------------------------- D4C: d4c_lovetrain<lg_love> + d4c_frame<N, N/16>
def _d4c_lg(fs):
    n = int(2.0 ** (1 + int(math.log(4.0 * fs / 47.0 + 1) / math.log(2))))
    m = int(2.0 ** (1 + int(math.log(3.0 * fs / 40.0 + 1) / math.log(2))))
    return _lg(n), _lg(m)


D4C_CASES = [  # fs, f0 kind, threshold, log2 of the frame transform, log2 of LoveTrain's
    (16000, "harvest", 0.85, 11, 11),
    (22050, "low", 0.0, 11, 11),
    (44100, "harvest", 0.0, 12, 12),
    (48000, "steps", 0.85, 12, 12),
    (64000, "harvest", 0.85, 13, 13),
    (96000, "sparse", 0.85, 13, 13),
    (192000, "harvest", 0.85, 14, 14),
]


def _check_d4c(what, h, r, w):
    w_only = discrete_agreement(f"{what} LoveTrain exits", d4c_exit_rows(h), d4c_exit_rows(r), d4c_exit_rows(w))
    assert_accurate(what, h, r, w, exclude_rows=w_only)


@pytest.mark.parametrize("fs,kind,threshold,lg_n,lg_love", D4C_CASES)
def test_d4c_accuracy(wh, ref_oracle, wide, fs, kind, threshold, lg_n, lg_love):
    assert _d4c_lg(fs) == (lg_n, lg_love)
    x = _signal(fs, 0.2 if fs < 100000 else 0.08)
    tp, f0 = _f0(kind, ref_oracle, x, fs)
    nf, fft = len(tp), ref_oracle.cheaptrick_fft_size(fs)
    ap, prof = _gpu(wh, lambda: wh.d4c(_dev(x)[None], fs, _dev(tp)[None], _dev(f0)[None], [nf], fft, threshold=threshold))
    assert prof.get("d4c_lovetrain") == 1 and prof.get("d4c_frame") == 1, prof
    r = ref_oracle.d4c(x, fs, tp, f0, fft, threshold=threshold)
    w = wide.d4c(x, fs, tp, f0, fft, threshold=threshold)
    _check_d4c(f"d4c N=2^{lg_n} love=2^{lg_love} {fs} {kind} th={threshold}", ap[0, :nf], r, w)


def test_d4c_16384_split_launches(wh, ref_oracle, wide):
    """192 kHz: the group delay is parked in global memory, park_slots workgroups per launch (d4c.hip launch_d4c); a batch
    of more than 2048 frames needs several launches.  Sparse voicing keeps the oracles' share short."""
    fs, B, sec = 192000, 16, 0.7
    xs = [_signal(fs, sec, i) for i in range(B)]
    n = len(xs[0])
    nf = int(1000.0 * n / fs / 5.0) + 1
    assert B * nf > 2048
    tp = np.arange(nf) * 0.005
    f0s = [_track("sparse", fs, nf, 100 + i) * (np.arange(nf) % 5 == 0) for i in range(B)]
    fft = ref_oracle.cheaptrick_fft_size(fs)
    xb, tb, fb = _dev(np.stack(xs)), _dev(np.tile(tp, (B, 1))), _dev(np.stack(f0s))
    ap, prof = _gpu(wh, lambda: wh.d4c(xb, fs, tb, fb, [nf] * B, fft))
    assert prof.get("d4c_frame", 0) >= 2, prof
    for i in range(B):
        r = ref_oracle.d4c(xs[i], fs, tp, f0s[i], fft)
        w = wide.d4c(xs[i], fs, tp, f0s[i], fft)
        _check_d4c(f"d4c 16384 batch utt {i}", ap[i, :nf], r, w)


# ---------------------------------------------------------------- StoneMask
@pytest.mark.parametrize("fs,kinds", [(16000, ("harvest", "steps")), (192000, ("harvest", "low"))])
def test_stonemask_accuracy(wh, ref_oracle, wide, fs, kinds):
    x = _signal(fs, 0.3 if fs < 100000 else 0.15)
    for kind in kinds:
        tp, f0 = _f0(kind, ref_oracle, x, fs)
        h, prof = _gpu(wh, lambda: wh.stonemask(_dev(x)[None], fs, _dev(tp)[None], _dev(f0)[None], [len(tp)]))
        assert prof.get("sm_frame") == 1, prof
        h = h[0, : len(tp)]
        r, w = ref_oracle.stonemask(x, fs, tp, f0), wide.stonemask(x, fs, tp, f0)
        w_only = discrete_agreement(f"stonemask {fs} {kind}", *(stonemask_outcome(v, f0) for v in (h, r, w)))
        keep = np.setdiff1d(np.flatnonzero(stonemask_outcome(r, f0) == 2), w_only)
        assert keep.size > 0
        assert_accurate(f"stonemask {fs} {kind}", h[keep, None], r[keep, None], w[keep, None])


# ---------------------------------------------------------------- Synthesis: sy_pulse<4096> (fft <= 4096), <8192>
@pytest.mark.parametrize("fs,lg", [(48000, 11), (96000, 12), (192000, 13)])
def test_synthesis_accuracy(wh, ref_oracle, wide, fs, lg):
    x = _signal(fs, 0.3 if fs < 100000 else 0.15)
    tp, f0 = ref_oracle.harvest(x, fs)
    fft = ref_oracle.cheaptrick_fft_size(fs)
    assert _lg(fft) == lg
    sp = ref_oracle.cheaptrick(x, fs, tp, f0, fft_size=fft)
    ap = ref_oracle.d4c(x, fs, tp, f0, fft)
    nf = len(tp)
    y, prof = _gpu(wh, lambda: wh.synthesis(_dev(f0)[None], _dev(sp)[None], _dev(ap)[None], nf, fft, 5.0, fs, len(x)))
    assert prof.get("sy_pulse") == 1, prof
    r = ref_oracle.synthesis(f0, sp, ap, fft, 5.0, fs, len(x))
    w = wide.synthesis(f0, sp, ap, fft, 5.0, fs, len(x))
    assert_accurate(f"synthesis sy_pulse<{4096 if lg <= 12 else 8192}> {fs}", y[0, None, : len(x)], r[None], w[None],
                    peak=True)


# ---------------------------------------------------------------- Harvest against the reference, 1e-10
def _with_env(name, fn):
    """fn() with the route switch `name` set (as tests/test_refine_routes.py does), the environment restored after"""
    if name is None:
        return fn()
    old = os.environ.pop(name, None)
    try:
        os.environ[name] = "1"
        return fn()
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


HV_CASES = [  # fs, f0_floor, environment switch, shared_device, kernels that must run, kernels that must not
    (16000, 71.0, None, False, ("hv_refine", "hv_band_events_fft"), ("hv_refine_frames",)),
    (32000, 71.0, None, True, ("hv_refine",), ("hv_refine_frames",)),
    (48000, 71.0, None, False, ("hv_refine",), ("hv_refine_frames",)),
    (96000, 71.0, None, True, ("hv_refine",), ("hv_refine_frames",)),
    (44100, 71.0, None, False, ("hv_refine_frames",), ("hv_refine",)),
    (22050, 71.0, None, True, ("hv_refine_frames",), ("hv_refine",)),
    (48000, 71.0, "WORLD_HIP_REFINE_FRAMES", False, ("hv_refine_frames",), ("hv_refine",)),
    (48000, 71.0, "WORLD_HIP_REFINE_ROTATE", False, ("hv_refine_frames",), ("hv_refine",)),
    (16000, 15.0, None, False, ("hv_band_events",), ("hv_band_events_fft",)),    # taps past half a 4096-point block
    (16000, 71.0, "WORLD_HIP_HARVEST_FIR", True, ("hv_band_events",), ("hv_band_events_fft",)),
    (11025, 71.0, None, False, ("hv_refine_frames",), ()),                 # decimation ratio 1
    (192000, 71.0, None, True, (), ()),                                    # the largest decimation
]


@pytest.mark.parametrize("fs,f0_floor,switch,shared,must,must_not", HV_CASES)
def test_harvest_against_reference(ref_oracle, fs, f0_floor, switch, shared, must, must_not):
    import torch
    from world_amd.api import WorldHip
    wh = WorldHip(shared_device=shared)
    x = _signal(fs, 0.5 if fs < 100000 else 0.3, 4)
    (tp, f0, nf), prof = _with_env(switch, lambda: _gpu(wh, lambda: wh.harvest(_dev(x)[None], fs, f0_floor=f0_floor)))
    wh.close()
    torch.cuda.synchronize()
    for k in must:
        assert k in prof, (k, prof)
    for k in must_not:
        assert k not in prof, (k, prof)
    tp_r, f0_r = ref_oracle.harvest(x, fs, f0_floor=f0_floor)
    assert nf[0] == len(tp_r) and np.array_equal(tp[0, : nf[0]], tp_r)
    assert_f0_tight(f"harvest {fs} floor {f0_floor} {switch or ''} shared={shared}", f0[0, : nf[0]], f0_r)


# ---------------------------------------------------------------- DIO against the reference, 1e-10
def _band_lds_bytes(ntap):                      # bandfilter.h band_lds_bytes, kTile = 256 threads x 8 outputs
    pad8 = lambda i: i + (i >> 3)
    return 8 * ((ntap + 1) + pad8(2048 + 2 + ntap + 3 + 8) + 1 + pad8(2048 + 4) + 1 + 64)


@pytest.mark.parametrize("fs,speed,lowcut_in_global", [(16000, 1, False), (16000, 12, False), (192000, 1, True),
                                                       (192000, 12, False)])
def test_dio_against_reference(wh, ref_oracle, fs, speed, lowcut_in_global):
    cut = int(fs / speed / 50.0 + 0.5)
    assert (_band_lds_bytes(2 * cut + 1) > 160 * 1024) == lowcut_in_global        # dio.hip: dio_lowcut<true> beyond LDS
    x = _signal(fs, 0.5 if fs < 100000 else 0.3, 4)
    (tp, f0, nf), prof = _gpu(wh, lambda: wh.dio(_dev(x)[None], fs, speed=speed))
    assert "dio_lowcut" in prof, prof
    tp_r, f0_r = ref_oracle.dio(x, fs, speed=speed)
    assert nf[0] == len(tp_r) and np.array_equal(tp[0, : nf[0]], tp_r)
    assert_f0_tight(f"dio {fs} speed {speed}", f0[0, : nf[0]], f0_r)
