"""Parameter modification (reference test/test.cpp: ParameterModification) through the new C entry points of the
host-compiled kernels (tests/emu/libworld_emu.so; device memory is host memory there): world_hip_modify_batch,
world_hip_f0_statistics and world_hip_resynthesize_batch against a NumPy statement of the reference's arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

from backends import ROOT, envelope, lib, rel  # noqa: F401 (lib: a fixture)

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libworld_ref.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


# ---- the host statement (NumPy) ------------------------------------------------------------------------------------------
def interp1(x, y, xi):
    """matlabfunctions.cpp interp1: histc gives each query the largest k in [1, n-1] with x[k-1] <= xi (clamped), then
    y[k-1] + s (y[k] - y[k-1]), s = (xi - x[k-1]) / (x[k] - x[k-1]).  y may hold several rows (last axis)."""
    k = np.clip(np.searchsorted(x, xi, side="right"), 1, len(x) - 1)
    s = (xi - x[k - 1]) / (x[k] - x[k - 1])
    return y[..., k - 1] + s * (y[..., k] - y[..., k - 1])


def warp_rows(sp, ratio, fs, fft_size):
    """test.cpp:229-255 on rows sp [..., fft/2+1]"""
    if ratio == 1.0:
        return sp.copy()
    i = np.arange(fft_size // 2 + 1)
    x = ratio * i / fft_size * fs
    xi = i.astype(np.float64) / fft_size * fs
    out = np.exp(interp1(x, np.log(sp), xi))
    if ratio < 1.0:
        m = int(fft_size / 2.0 * ratio)
        out[..., m:] = out[..., m - 1:m]
    return out


def log_f0_stats(f0):
    """NumPy's two-pass statistics of ln f0 over the voiced frames (finite, > 0); none voiced: {0, 0, 0}"""
    v = f0[np.isfinite(f0) & (f0 > 0)]
    if v.size == 0:
        return 0.0, 0.0, 0.0
    lg = np.log(v)
    return float(v.size), float(np.mean(lg)), float(np.std(lg))


def map_f0(f0, scale, target=None):
    out = f0.copy()
    if target is not None:
        _, mu, sigma = log_f0_stats(f0)
        v = f0[np.isfinite(f0) & (f0 > 0)]
        if v.size and np.all(v == v[0]):
            sigma = 0.0                     # the contract: a constant track has sigma_s = 0 (voiced frames -> the target mean)
        voiced = np.isfinite(f0) & (f0 > 0)
        gain = target[1] / sigma if sigma > 0 else 0.0
        out[voiced] = np.exp(target[0] + (np.log(f0[voiced]) - mu) * gain)
    return out * scale


# ---- the emulated library ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.world_hip_create(0, None)
    assert c
    yield c
    lib.world_hip_destroy(c)


def mods_of(n, scale=1.0, ratio=1.0, target=None):
    from world_amd.api import modifications
    return modifications(n, scale, ratio, target)


def vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def modify(lib, ctx, f0, sp, nf, fs, fft_size, mods, f0_out=None, sp_out=None):
    """world_hip_modify_batch; out arrays default to in-place"""
    B, F = (f0 if f0 is not None else sp).shape[:2]
    nf = np.ascontiguousarray(nf, dtype=np.int32)
    f0_out = f0 if f0_out is None else f0_out
    sp_out = sp if sp_out is None else sp_out
    return lib.world_hip_modify_batch(ctx, B, fs, fft_size, nf.ctypes.data_as(_ip), F, mods, vp(f0), vp(f0_out), vp(sp),
                                      vp(sp_out))


def test_restatement_matches_the_reference_interp1():
    """The NumPy histc / interp1 against the reference's own interp1 (exported unmangled) on the warp's axes"""
    if not os.path.exists(REF_LIB):
        pytest.skip("oracle/_ref/libworld_ref.so was not built (needs the reference tree at build time)")
    ref = C.CDLL(REF_LIB)
    ref.interp1.argtypes = [_dp, _dp, C.c_int, _dp, C.c_int, _dp]
    ref.interp1.restype = None
    for fs, fft in ((16000, 1024), (48000, 2048), (192000, 8192)):
        y = np.log(envelope(fs, fft, 1, seed=fs)[0])
        i = np.arange(fft // 2 + 1)
        xi = i.astype(np.float64) / fft * fs
        for ratio in (0.5, 0.8, 0.93, 1.25, 1.7, 2.0):
            x = np.ascontiguousarray(ratio * i / fft * fs)
            want = np.zeros(i.size)
            ref.interp1(x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), i.size, xi.ctypes.data_as(_dp), i.size,
                        want.ctypes.data_as(_dp))
            assert np.array_equal(interp1(x, y, xi), want), (fs, ratio)


@pytest.mark.parametrize("fs", [16000, 24000, 48000, 96000, 192000])
def test_warp_of_a_ragged_batch(lib, ctx, fs):
    from world_amd.api import cheaptrick_fft_size
    fft = cheaptrick_fft_size(fs, 71.0)
    nb = fft // 2 + 1
    ratios = [0.5, 0.8, 1.25, 2.0, 0.87, 1.13, 1.0]          # knots hit exactly, in between, identity
    nf = np.array([9, 3, 7, 1, 6, 9, 4], dtype=np.int32)
    B, F = len(ratios), int(nf.max())
    sp = np.full((B, F, nb), np.nan)
    for u in range(B):
        sp[u, :nf[u]] = envelope(fs, fft, int(nf[u]), seed=u)
    out = np.full_like(sp, np.nan)
    assert modify(lib, ctx, None, sp, nf, fs, fft, mods_of(B, ratio=ratios), sp_out=out) == 0, lib.world_hip_last_error()
    for u, r in enumerate(ratios):
        want = warp_rows(sp[u, :nf[u]], r, fs, fft)
        got = out[u, :nf[u]]
        assert rel(got, want) <= 1e-13, (fs, r, rel(got, want))
        if r < 1.0:
            m = int(fft / 2.0 * r)
            assert np.array_equal(got[:, m:], np.repeat(got[:, m - 1:m], nb - m, axis=1))
        if r == 1.0:
            assert np.array_equal(got, sp[u, :nf[u]])
        assert np.all(np.isnan(out[u, nf[u]:])), "padding rows written"
    # in place: the same bits
    inplace = sp.copy()
    assert modify(lib, ctx, None, inplace, nf, fs, fft, mods_of(B, ratio=ratios)) == 0
    for u in range(B):
        assert np.array_equal(inplace[u, :nf[u]], out[u, :nf[u]])
        assert np.all(np.isnan(inplace[u, nf[u]:]))


def test_identity_leaves_rows_bitwise(lib, ctx):
    fs, fft = 16000, 1024
    sp = envelope(fs, fft, 10, seed=3).reshape(2, 5, -1)
    before = sp.copy()
    f0 = np.linspace(100, 200, 10).reshape(2, 5)
    f0_before = f0.copy()
    assert modify(lib, ctx, f0, sp, [5, 4], fs, fft, None) == 0
    assert np.array_equal(sp, before) and np.array_equal(f0, f0_before)
    out = np.zeros_like(sp)
    assert modify(lib, ctx, None, sp, [5, 5], fs, fft, mods_of(2), sp_out=out) == 0
    assert np.array_equal(out, sp)


def test_f0_scale_is_the_reference_multiply(lib, ctx):
    rng = np.random.default_rng(1)
    f0 = rng.uniform(60, 400, (3, 50))
    f0[:, ::7] = 0.0
    f0[1, 3], f0[2, 4] = np.nan, np.inf
    nf = np.array([50, 40, 50], dtype=np.int32)
    scales = [1.5, 0.7, 2.0]
    out = np.full_like(f0, -1.0)
    assert modify(lib, ctx, f0, None, nf, 16000, 0, mods_of(3, scale=scales), f0_out=out) == 0, lib.world_hip_last_error()
    for u, s in enumerate(scales):
        assert np.array_equal(out[u, :nf[u]], f0[u, :nf[u]] * s, equal_nan=True)
        assert np.all(out[u, nf[u]:] == -1.0)


def test_log_f0_statistics_and_conversion(lib, ctx):
    rng = np.random.default_rng(5)
    F = 300
    f0 = np.zeros((5, F))
    f0[0] = np.exp(rng.normal(5.0, 0.2, F)); f0[0, rng.random(F) < 0.3] = 0.0
    f0[1, 17] = 180.0                                             # one voiced frame
    # f0[2]: no voiced frame at all
    f0[3] = 220.0; f0[3, ::5] = 0.0                               # constant: sigma_s = 0
    f0[4] = np.exp(rng.normal(4.6, 0.3, F)); f0[4, 10] = np.nan; f0[4, 11] = np.inf; f0[4, 12] = -5.0
    nf = np.array([F, 200, F, F, 250], dtype=np.int32)
    stats = np.full((5, 3), -1.0)
    assert lib.world_hip_f0_statistics(ctx, 5, nf.ctypes.data_as(_ip), F, vp(f0), vp(stats)) == 0, lib.world_hip_last_error()
    for u in range(5):
        want = log_f0_stats(f0[u, :nf[u]])
        assert stats[u, 0] == want[0]
        assert abs(stats[u, 1] - want[1]) <= 1e-12 * max(1.0, abs(want[1])), u
        assert abs(stats[u, 2] - want[2]) <= 1e-12 * max(1.0, abs(want[2])), u
    target = ([5.3, 5.0, 4.0, 5.1, 4.4], [0.15, 0.2, 0.1, 0.3, 0.25])
    scales = [1.0, 1.2, 1.0, 0.5, 1.0]
    out = np.zeros_like(f0)
    assert modify(lib, ctx, f0, None, nf, 16000, 0, mods_of(5, scale=scales, target=target), f0_out=out) == 0
    for u in range(5):
        want = map_f0(f0[u, :nf[u]], scales[u], (target[0][u], target[1][u]))
        got = out[u, :nf[u]]
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0)
        ok = np.isfinite(want) & (want != 0)
        assert rel(got[ok], want[ok]) <= 1e-12, u
        assert np.array_equal(got[~ok], want[~ok], equal_nan=True)
    # one voiced frame, constant F0 (sigma_s = 0): voiced frames land on the target mean itself
    assert rel(out[1, 17:18], np.array([np.exp(5.0) * 1.2])) <= 1e-15
    const = out[3, :nf[3]][f0[3, :nf[3]] > 0]
    assert np.all(const == const[0]) and rel(const[:1], np.array([np.exp(5.1) * 0.5])) <= 1e-15


@pytest.mark.parametrize("bad", [
    dict(scale=np.nan), dict(scale=-1.0), dict(scale=np.inf), dict(ratio=0.0), dict(ratio=-1.2), dict(ratio=np.nan),
    dict(ratio=np.inf), dict(ratio=1.0 / 1024), dict(target=([np.nan], [0.1])), dict(target=([5.0], [-0.1])),
    dict(target=([5.0], [np.inf]))])
def test_invalid_modifications_are_refused_untouched(lib, ctx, bad):
    fs, fft = 16000, 1024
    sp = envelope(fs, fft, 4, seed=9).reshape(2, 2, -1)
    f0 = np.full((2, 2), 150.0)
    args = dict(scale=[1.0, bad.get("scale", 1.0)], ratio=[1.1, bad.get("ratio", 1.0)])
    target = bad.get("target")
    if target is not None:
        target = ([5.0, target[0][0]], [0.1, target[1][0]])
    sp0, f00 = sp.copy(), f0.copy()
    out_sp, out_f0 = np.full_like(sp, 7.0), np.full_like(f0, 7.0)
    rc = modify(lib, ctx, f0, sp, [2, 2], fs, fft, mods_of(2, args["scale"], args["ratio"], target), f0_out=out_f0,
                sp_out=out_sp)
    assert rc != 0 and lib.world_hip_last_error().decode()
    assert np.all(out_sp == 7.0) and np.all(out_f0 == 7.0)
    rc = modify(lib, ctx, f0, sp, [2, 2], fs, fft, mods_of(2, args["scale"], args["ratio"], target))
    assert rc != 0 and np.array_equal(sp, sp0) and np.array_equal(f0, f00)


def test_invalid_shapes_are_refused(lib, ctx):
    fs = 16000
    sp = envelope(fs, 1024, 2, seed=1).reshape(1, 2, -1)
    f0 = np.full((1, 2), 150.0)
    for fft in (1000, 64, 16384):
        assert modify(lib, ctx, None, sp, [2], fs, fft, mods_of(1, ratio=1.2)) != 0
    assert modify(lib, ctx, f0, None, [3], fs, 1024, mods_of(1, scale=2.0)) != 0          # n_frames > f_stride
    nf = np.array([2], dtype=np.int32)
    assert lib.world_hip_modify_batch(ctx, 1, fs, 1024, nf.ctypes.data_as(_ip), 2, mods_of(1), vp(f0), None, None,
                                      None) != 0
    assert np.all(f0 == 150.0)


# ---- the whole chain in one call -----------------------------------------------------------------------------------------
def _opts(fs, frame_period=5.0):
    from world_amd.api import CheapTrickOption, D4COption, HarvestOption, cheaptrick_fft_size
    return HarvestOption(71.0, 800.0, frame_period), CheapTrickOption(-0.15, 71.0, cheaptrick_fft_size(fs, 71.0)), \
        D4COption(0.85)


def _batch(fs):
    from world_amd import synth
    xs = [synth.vowel(fs, 0.3, seed=11).numpy(), synth.vowel(fs, 0.22, seed=5, base_f0=210.0).numpy()]
    x = np.zeros((2, max(len(v) for v in xs)))
    for u, v in enumerate(xs):
        x[u, :len(v)] = v
    return x, np.array([len(v) for v in xs], dtype=np.int32)


@pytest.mark.parametrize("time_scale", [1.0, 0.5, 2.0])
def test_resynthesize_equals_the_separate_calls(lib, ctx, time_scale):
    from world_amd.api import frame_count
    fs = 16000
    x, xl = _batch(fs)
    hopt, copt, dopt = _opts(fs)
    nb = copt.fft_size // 2 + 1
    nf = np.array([frame_count(fs, int(n), 5.0) for n in xl], dtype=np.int32)
    F = int(nf.max())
    mods = mods_of(2, scale=[1.5, 0.8], ratio=[1.2, 0.85])
    yl = np.array([lib.world_hip_resynthesis_length(fs, int(n), 5.0, time_scale) for n in nf], dtype=np.int32)
    assert list(yl) == [int((n - 1) * 5.0 * time_scale / 1000.0 * fs) + 1 for n in nf]
    Y = int(yl.max())
    y = np.zeros((2, Y))
    rc = lib.world_hip_resynthesize_batch(ctx, 2, fs, vp(x), x.shape[1], xl.ctypes.data_as(_ip), C.byref(hopt),
                                          C.byref(copt), C.byref(dopt), mods, time_scale, yl.ctypes.data_as(_ip), Y, vp(y))
    assert rc == 0, lib.world_hip_last_error()
    tpos, f0 = np.zeros((2, F)), np.zeros((2, F))
    sp, ap = np.zeros((2, F, nb)), np.zeros((2, F, nb))
    assert lib.world_hip_analyze_batch(ctx, 2, fs, vp(x), x.shape[1], xl.ctypes.data_as(_ip), C.byref(hopt), C.byref(copt),
                                       C.byref(dopt), F, vp(tpos), vp(f0), vp(sp), vp(ap)) == 0
    assert modify(lib, ctx, f0, sp, nf, fs, copt.fft_size, mods) == 0
    y2 = np.zeros((2, Y))
    assert lib.world_hip_synthesis_batch(ctx, 2, fs, 5.0 * time_scale, copt.fft_size, nf.ctypes.data_as(_ip), F, vp(f0),
                                         vp(sp), vp(ap), yl.ctypes.data_as(_ip), Y, vp(y2)) == 0
    assert np.array_equal(y, y2)
    assert np.max(np.abs(y)) > 0
    assert lib.world_hip_workspace_bytes(ctx) >= 2 * F * 8 * (2 + 2 * nb)


def test_resynthesize_refuses_invalid_parameters_untouched(lib, ctx):
    fs = 16000
    x, xl = _batch(fs)
    hopt, copt, dopt = _opts(fs)
    yl = np.array([100, 100], dtype=np.int32)
    y = np.full((2, 100), 3.0)

    def call(mods=None, time_scale=1.0, y_len=yl, c=copt, h=hopt):
        return lib.world_hip_resynthesize_batch(ctx, 2, fs, vp(x), x.shape[1], xl.ctypes.data_as(_ip), C.byref(h),
                                                C.byref(c), C.byref(dopt), mods, time_scale, y_len.ctypes.data_as(_ip),
                                                100, vp(y))
    from world_amd.api import CheapTrickOption, HarvestOption
    for kwargs in (dict(time_scale=0.0), dict(time_scale=-1.0), dict(time_scale=np.nan), dict(time_scale=np.inf),
                   dict(mods=mods_of(2, scale=[1.0, np.nan])), dict(mods=mods_of(2, ratio=[1.0, 0.0])),
                   dict(mods=mods_of(2, ratio=[1.0, 1e-4])), dict(mods=mods_of(2, target=([5.0, 5.0], [0.1, -1.0]))),
                   dict(y_len=np.array([100, 101], dtype=np.int32)), dict(y_len=np.array([0, 100], dtype=np.int32)),
                   dict(c=CheapTrickOption(-0.15, 71.0, 1000)), dict(h=HarvestOption(71.0, 800.0, np.nan))):
        assert call(**kwargs) != 0, kwargs
        assert lib.world_hip_last_error().decode(), kwargs
        assert np.all(y == 3.0), kwargs
    for fs_, n, fp, ts in ((0, 10, 5.0, 1.0), (16000, 0, 5.0, 1.0), (16000, 10, 0.0, 1.0), (16000, 10, 5.0, 0.0),
                           (16000, 10, 5.0, np.nan), (16000, 10, np.inf, 1.0)):
        assert lib.world_hip_resynthesis_length(fs_, n, fp, ts) == 0
    assert lib.world_hip_resynthesis_length(16000, 10, 5.0, 1.0) == int(9 * 5.0 / 1000.0 * 16000) + 1


# ---- the batch tool's output paths (checked before any GPU work) ---------------------------------------------------------
def _tool(argv):
    from world_amd import tools
    with pytest.raises(SystemExit) as e:
        tools.main(argv)
    assert e.value.code not in (0, None)


def test_transform_never_overwrites_an_input(tmp_path):
    src = tmp_path / "voice.wav"
    src.write_bytes(b"RIFF not really a wave")
    before = src.read_bytes()
    _tool(["transform", str(src), "--outdir", str(tmp_path), "--f0-scale", "1.5"])      # the input's own folder
    (tmp_path / "alias").symlink_to(tmp_path, target_is_directory=True)
    _tool(["transform", str(src), "--outdir", str(tmp_path / "alias")])                  # the same folder by another name
    _tool(["transform", str(src)])                                                         # no --outdir at all
    assert src.read_bytes() == before


def test_transform_refuses_two_inputs_with_one_output(tmp_path):
    from world_amd.tools import transform_outputs
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    ins = [str(tmp_path / "a" / "x.wav"), str(tmp_path / "b" / "x.wav")]
    with pytest.raises(ValueError):
        transform_outputs(ins, str(tmp_path / "out"))
    _tool(["transform", *ins, "--outdir", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()
    assert transform_outputs(ins[:1], str(tmp_path / "out")) == [str(tmp_path / "out" / "x.wav")]
