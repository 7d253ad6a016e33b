"""Frame-wise modification behind a time map (include/world_hip.h: world_hip_modify_frames_batch,
world_hip_resynthesize_frames_batch) through the host-compiled kernels (tests/emu/libworld_emu.so), against a NumPy
statement of the header's rules written here.  The cases are functions of a backend, so that tests/test_modify_frames_gpu.py
runs the same ones through the shipped library.

Tolerances.  The blend (1.0 - w) * a + w * b is the same IEEE operations in the same order under -ffp-contract=off:
equality.  Rows that went through the warp: 1e-13 relative, what tests/test_modify_cpu.py holds modify_warp_sp to (the
device log / exp differ from libm in the last bits).  F0 frames that went through the log-F0 conversion: 1e-12 relative,
what that file holds modify_f0 to.  Everything else (copies, one multiply, the clamp) is exact."""
import ctypes as C

import numpy as np
import pytest

import backends
from backends import cpu_backend, envelope, lib, rel  # noqa: F401 (lib: a fixture)

_ip = C.POINTER(C.c_int)
CURVES = ("time_map", "f0_target", "f0_scale", "formant_shift", "ap_gain")
AP_LO, AP_HI = 0.001, 1.0 - 1e-12


# ---- the host statement (NumPy) ------------------------------------------------------------------------------------------
def interp1(x, y, xi):
    """matlabfunctions.cpp interp1 (restated from tests/test_modify_cpu.py): histc gives each query the largest k in
    [1, n-1] with x[k-1] <= xi (clamped), then y[k-1] + s (y[k] - y[k-1]), s = (xi - x[k-1]) / (x[k] - x[k-1])"""
    k = np.clip(np.searchsorted(x, xi, side="right"), 1, len(x) - 1)
    s = (xi - x[k - 1]) / (x[k] - x[k - 1])
    return y[..., k - 1] + s * (y[..., k] - y[..., k - 1])


def warp_rows(sp, ratio, fs, fft_size):
    """test.cpp:229-255 on rows sp [..., fft/2+1] (restated from tests/test_modify_cpu.py)"""
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


def voiced(v):
    return np.isfinite(v) & (v > 0)


def convert_log_f0(f0, target):
    """the existing modify_f0 conversion of one utterance's source track: voiced frames -> exp(mean_t + (ln f0 - mu_s) *
    (sigma_s > 0 ? std_t / sigma_s : 0)) with the two-pass statistics of the voiced ln f0"""
    out = f0.copy()
    v = voiced(f0)
    if not v.any():
        return out
    lg = np.log(f0[v])
    mu, sigma = float(np.mean(lg)), float(np.std(lg))
    if np.all(f0[v] == f0[v][0]):
        sigma = 0.0
    gain = target[1] / sigma if sigma > 0 else 0.0
    out[v] = np.exp(target[0] + (lg - mu) * gain)
    return out


def source_position(time_map, n_out, n_src):
    s = np.arange(n_out, dtype=np.float64) if time_map is None else np.array(time_map[:n_out], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(s > 0, s, 0.0)                   # not > 0, NaN included: frame 0
    s = np.minimum(s, float(n_src - 1))
    k = np.floor(s).astype(np.int64)
    w = s - k
    k1 = np.minimum(k + 1, n_src - 1)
    return k, k1, w, (w != 0) & (k1 != k)


def blend_rows(rows, k, k1, w, blend):
    out = rows[k].copy()
    wb = w[blend][:, None]
    out[blend] = (1.0 - wb) * rows[k[blend]] + wb * rows[k1[blend]]
    return out


def valid_scale(v):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v) & (v >= 0), v, 1.0)


def valid_ratio(r, fft_size):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(r) & (r > 0) & (fft_size / 2.0 * r >= 1.0), r, 1.0)


def statement(f0, sp, ap, n_out, fs, fft_size, scale=1.0, ratio=1.0, target=None, time_map=None, f0_target=None,
              f0_scale=None, formant_shift=None, ap_gain=None):
    """The header's steps 1-8 for ONE utterance: f0 [n_src], sp / ap [n_src, nb] (any may be None), curves [>= n_out] or
    None, scale / ratio / target = its WorldHipModification.  -> (f0', sp', ap', converted) with n_out frames; converted
    marks the F0 frames whose value went through the log-F0 conversion."""
    n_src = len(next(a for a in (f0, sp, ap) if a is not None))
    k, k1, w, blend = source_position(time_map, n_out, n_src)
    f0_o = sp_o = ap_o = conv = None
    if sp is not None:
        rows = blend_rows(sp, k, k1, w, blend)
        r = valid_ratio(np.asarray(formant_shift[:n_out]), fft_size) if formant_shift is not None else np.full(n_out, ratio)
        sp_o = np.stack([warp_rows(rows[j], float(r[j]), fs, fft_size) for j in range(n_out)])
    if ap is not None:
        ap_o = blend_rows(ap, k, k1, w, blend)
        if ap_gain is not None:
            v = ap_o * valid_scale(np.asarray(ap_gain[:n_out]))[:, None]
            with np.errstate(invalid="ignore"):
                v = np.where(v > AP_LO, v, AP_LO)
                ap_o = np.where(v < AP_HI, v, AP_HI)
    if f0 is not None:
        src = convert_log_f0(f0, target) if target is not None else f0
        a, b = src[k], src[k1]
        va, vb = voiced(a), voiced(b)
        with np.errstate(invalid="ignore"):
            mixed = np.where(va & vb, (1.0 - w) * a + w * b,
                             np.where(va, np.where(1.0 - w > 0.5, a, 0.0), np.where(vb, np.where(w > 0.5, b, 0.0), 0.0)))
        f0_o = np.where(blend, mixed, a)
        conv = np.where(blend, (va | vb), va) & (target is not None) & voiced(f0_o)
        if f0_target is not None:
            t = np.asarray(f0_target[:n_out], dtype=np.float64)
            take = voiced(f0_o) & voiced(t)
            f0_o = np.where(take, t, f0_o)
            conv = conv & ~take
        f0_o = f0_o * (valid_scale(np.asarray(f0_scale[:n_out])) if f0_scale is not None else scale)
    return f0_o, sp_o, ap_o, conv


def fft_of(fs):
    from world_amd.api import cheaptrick_fft_size
    return cheaptrick_fft_size(fs, 71.0)


# ---- a backend: the two C calls on arrays that live where the library wants them ----------------------------------------
class Backend(backends.Backend):
    """world_hip_modify_batch / world_hip_modify_frames_batch on the arrays of backends.Backend"""

    def modify(self, fs, fft, nf, mods, f0=None, sp=None):
        """out of place -> (f0', sp') with NaN beyond"""
        B, F = (f0 if f0 is not None else sp).shape[:2]
        nf = np.ascontiguousarray(nf, dtype=np.int32)
        ins = [self.dev(a) if a is not None else None for a in (f0, sp)]
        outs = [self.dev(np.full(a.shape, np.nan)) if a is not None else None for a in (f0, sp)]
        rc = self.lib.world_hip_modify_batch(self.ctx, B, fs, fft, nf.ctypes.data_as(_ip), F, mods, self.ptr(ins[0]),
                                             self.ptr(outs[0]), self.ptr(ins[1]), self.ptr(outs[1]))
        assert rc == 0, self.error()
        return [self.host(o) if o is not None else None for o in outs]

    def frames(self, fs, fft, nf, no, O, mods=None, f0=None, sp=None, ap=None, inplace=False, fill=np.nan, **curves):
        """-> (rc, f0', sp', ap'): outputs [B, O(, nb)] pre-filled with `fill` (in place: the inputs' copies)"""
        from world_amd.api import WorldHipFrameCurves
        ref = next(a for a in (f0, sp, ap) if a is not None)
        B, F = ref.shape[:2]
        nf = np.ascontiguousarray(np.broadcast_to(nf, (B,)), dtype=np.int32)
        no = np.ascontiguousarray(np.broadcast_to(no, (B,)), dtype=np.int32)
        ins = [self.dev(a.copy()) if a is not None else None for a in (f0, sp, ap)]
        outs = ins if inplace else [self.dev(np.full((B, O) + a.shape[2:], fill)) if a is not None else None
                                    for a in (f0, sp, ap)]
        assert set(curves) <= set(CURVES)
        held = {"d_" + k: self.dev(np.asarray(v, dtype=np.float64)) for k, v in curves.items() if v is not None}
        for v in held.values():
            assert v.shape == (B, O)
        cv = WorldHipFrameCurves(**{k: self.ptr(v).value for k, v in held.items()})
        rc = self.lib.world_hip_modify_frames_batch(self.ctx, B, fs, fft, nf.ctypes.data_as(_ip), F, no.ctypes.data_as(_ip), O,
                                                    mods, C.byref(cv) if held else None, self.ptr(ins[0]), self.ptr(outs[0]),
                                                    self.ptr(ins[1]), self.ptr(outs[1]), self.ptr(ins[2]), self.ptr(outs[2]))
        return (rc, *[self.host(o) if o is not None else None for o in outs])


be = cpu_backend(Backend)


def mods_of(n, scale=1.0, ratio=1.0, target=None):
    from world_amd.api import modifications
    return modifications(n, scale, ratio, target)


def ragged(fs, fft, nf, seed):
    """a ragged batch: f0 with unvoiced stretches, envelopes, aperiodicities that also leave [0.001, 1 - 1e-12]; NaN
    beyond each utterance's frames"""
    rng = np.random.default_rng(seed)
    B, F, nb = len(nf), int(max(nf)), fft // 2 + 1
    f0, sp, ap = np.full((B, F), np.nan), np.full((B, F, nb), np.nan), np.full((B, F, nb), np.nan)
    for u, n in enumerate(nf):
        f0[u, :n] = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(70, 400, n))
        sp[u, :n] = envelope(fs, fft, int(n), seed=seed + u)
        ap[u, :n] = rng.uniform(-0.05, 1.05, (n, nb))
    return f0, sp, ap


def check_padding(outs, no):
    for o in outs:
        for u, n in enumerate(no):
            assert np.all(np.isnan(o[u, n:])), "frames at or beyond n_out were written"


# ---- the cases ----------------------------------------------------------------------------------------------------------
def case_identity_map_and_constant_curves(be, fs, fft=None):
    """1a: an identity map plus constant curves is world_hip_modify_batch with the same constants, bit for bit"""
    fft = fft or fft_of(fs)                   # (an explicit fft_size: off the rate's default)
    nf = np.array([9, 3, 7, 1, 6], dtype=np.int32)
    ratios, scales = [0.8, 1.25, 0.87, 2.0, 1.0], [1.5, 0.7, 1.0, 2.0, 1.2]
    f0, sp, ap = ragged(fs, fft, nf, seed=fs // 1000)
    B, F = f0.shape
    want_f0, want_sp = be.modify(fs, fft, nf, mods_of(B, scales, ratios), f0=f0, sp=sp)
    ident = np.tile(np.arange(F, dtype=np.float64), (B, 1))
    const = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[:, None], F, axis=1)
    for time_map in (ident, None):
        rc, g_f0, g_sp, g_ap = be.frames(fs, fft, nf, nf, F, None, f0=f0, sp=sp, ap=ap, time_map=time_map,
                                         f0_scale=const(scales), formant_shift=const(ratios))
        assert rc == 0, be.error()
        for u, n in enumerate(nf):
            assert np.array_equal(g_f0[u, :n], want_f0[u, :n]) and np.array_equal(g_sp[u, :n], want_sp[u, :n]), (fs, u)
            assert np.array_equal(g_ap[u, :n], ap[u, :n])
        check_padding((g_f0, g_sp, g_ap), nf)
    # the constants in mods instead of curves: the same bits again; in place (no map) as out of place
    rc, m_f0, m_sp, m_ap = be.frames(fs, fft, nf, nf, F, mods_of(B, scales, ratios), f0=f0, sp=sp, ap=ap, inplace=True)
    assert rc == 0, be.error()
    for u, n in enumerate(nf):
        assert np.array_equal(m_f0[u, :n], want_f0[u, :n]) and np.array_equal(m_sp[u, :n], want_sp[u, :n])
        assert np.array_equal(m_ap[u, :n], ap[u, :n])
    check_padding((m_f0, m_sp, m_ap), nf)


def case_integer_map_is_a_gather(be, fs):
    """1b: an integer-valued map (repeats, reversal, values that clamp) is a gather of the modify_batch result; ap rows
    without a gain are the gather of the input"""
    fft = fft_of(fs)
    nf = np.array([8, 5, 1], dtype=np.int32)
    ratios, scales = [1.2, 0.85, 0.9], [1.3, 1.0, 0.5]
    f0, sp, ap = ragged(fs, fft, nf, seed=7)
    B = 3
    done_f0, done_sp = be.modify(fs, fft, nf, mods_of(B, scales, ratios), f0=f0, sp=sp)
    maps = [np.array([7, 6, 5, 4, 3, 2, 1, 0, 0, 0, 3, 3, -2, 1e9, 9, 7.0]),          # reversal, repeats, out of range
            np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 5, 100, -1, -np.inf, np.inf]),
            np.array([0, 5, -1, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0])]
    O, no = 16, np.array([16, 14, 3], dtype=np.int32)
    rc, g_f0, g_sp, g_ap = be.frames(fs, fft, nf, no, O, mods_of(B, scales, ratios), f0=f0, sp=sp, ap=ap,
                                     time_map=np.stack(maps))
    assert rc == 0, be.error()
    for u in range(B):
        idx = np.clip(maps[u][:no[u]], 0, nf[u] - 1).astype(int)
        assert np.array_equal(g_f0[u, :no[u]], done_f0[u, idx]), (fs, u)
        assert np.array_equal(g_sp[u, :no[u]], done_sp[u, idx]), (fs, u)
        assert np.array_equal(g_ap[u, :no[u]], ap[u, idx]), (fs, u)
    check_padding((g_f0, g_sp, g_ap), no)


def case_blend_only(be, fs):
    """2: a fractional map with every ratio 1: sp, ap and f0 bit-identical to the statement, the voicing rules included"""
    fft = fft_of(fs)
    nf = np.array([10, 6, 1], dtype=np.int32)
    f0, sp, ap = ragged(fs, fft, nf, seed=21)
    #            0      1    2    3      4      5       6     7    8      9
    f0[0, :10] = [100.0, 0.0, 0.0, 200.0, 220.0, np.nan, 150.0, 0.0, 180.0, np.inf]
    maps = [np.array([0.5, 0.49, 0.51, 1.5, 2.5, 2.75, 2.25, 3.25, 4.5, 4.75, 5.5, 5.25, 6.5, 6.25, 7.5, 7.75, 8.5, 8.25,
                      8.75, 9.0, 3.0, 8.999, 0.0, 11.5]),
            np.linspace(0.0, 5.0, 24),
            np.array([0.0, 0.5, 0.9, 3.0] + [0.25] * 20)]                                 # one frame: always frame 0
    O, no = 24, np.array([24, 24, 5], dtype=np.int32)
    rc, g_f0, g_sp, g_ap = be.frames(fs, fft, nf, no, O, None, f0=f0, sp=sp, ap=ap, time_map=np.stack(maps))
    assert rc == 0, be.error()
    for u in range(3):
        w_f0, w_sp, w_ap, _ = statement(f0[u, :nf[u]], sp[u, :nf[u]], ap[u, :nf[u]], no[u], fs, fft, time_map=maps[u])
        assert np.array_equal(g_f0[u, :no[u]], w_f0, equal_nan=True), (fs, u, g_f0[u, :no[u]], w_f0)
        assert np.array_equal(g_sp[u, :no[u]], w_sp), (fs, u)
        assert np.array_equal(g_ap[u, :no[u]], w_ap), (fs, u)
    check_padding((g_f0, g_sp, g_ap), no)
    # the rules themselves, spelled out on utterance 0 (weights of frame k / k + 1 = 1 - w / w)
    got = dict(zip(maps[0], g_f0[0]))
    assert got[0.5] == 0.0 and got[0.49] == 100.0 and got[0.51] == 0.0        # voiced | unvoiced: strictly above 0.5
    assert got[1.5] == 0.0 and got[2.5] == 0.0 and got[2.75] == 200.0 and got[2.25] == 0.0
    assert got[3.25] == (1.0 - 0.25) * 200.0 + 0.25 * 220.0                    # both voiced
    assert got[4.5] == 0.0 and got[4.75] == 0.0 and got[5.5] == 0.0 and got[5.25] == 0.0   # NaN is not voiced
    assert got[8.25] == 180.0 and got[8.75] == 0.0                             # Inf is not voiced
    assert np.isinf(got[9.0]) and got[3.0] == 200.0 and np.isinf(got[11.5])    # whole positions: the frame as it is
    assert np.all(g_f0[2, :5] == f0[2, 0]) or np.isnan(f0[2, 0])


def case_blend_and_per_frame_warp(be, fs, fft=None):
    """3: a fractional map and a formant ratio per frame: 1e-13 against the statement; the top-bin fill of r < 1 and the
    rows with r == 1 exact"""
    fft = fft or fft_of(fs)                   # (an explicit fft_size: off the rate's default)
    nb = fft // 2 + 1
    nf = np.array([7, 4], dtype=np.int32)
    _, sp, _ = ragged(fs, fft, nf, seed=33)
    O, no = 12, np.array([12, 9], dtype=np.int32)
    maps = np.stack([np.linspace(0.0, 6.0, O), np.array([0, 0.3, 0.6, 1.0, 1.5, 2.2, 3.0, 2.9, 0.1, 0, 0, 0.0])])
    ratios = np.stack([np.array([0.5, 0.8, 1.0, 1.25, 2.0, 0.87, 1.13, 1.0, 0.93, 1.7, 1.0, 0.6]),
                       np.array([1.0, 1.1, 0.9, 1.0, 0.75, 1.0, 1.3, 0.95, 1.0, 1.0, 1.0, 1.0])])
    rc, _, g_sp, _ = be.frames(fs, fft, nf, no, O, None, sp=sp, time_map=maps, formant_shift=ratios)
    assert rc == 0, be.error()
    for u in range(2):
        _, want, _, _ = statement(None, sp[u, :nf[u]], None, no[u], fs, fft, time_map=maps[u], formant_shift=ratios[u])
        _, plain, _, _ = statement(None, sp[u, :nf[u]], None, no[u], fs, fft, time_map=maps[u])
        got = g_sp[u, :no[u]]
        assert rel(got, want) <= 1e-13, (fs, u, rel(got, want))
        for j in range(no[u]):
            r = ratios[u, j]
            if r == 1.0:
                assert np.array_equal(got[j], plain[j]), (fs, u, j)
            if r < 1.0:
                m = int(fft / 2.0 * r)
                assert np.all(got[j, m:] == got[j, m - 1]), (fs, u, j)
    check_padding((g_sp,), no)


def case_padding_and_refusals(be, fs):
    """5: every refused call leaves every output untouched; invalid device-side values give the identity for that frame"""
    fft = fft_of(fs)
    nf = np.array([4, 3], dtype=np.int32)
    f0, sp, ap = ragged(fs, fft, nf, seed=5)
    f0, sp, ap = np.nan_to_num(f0, nan=100.0), np.nan_to_num(sp, nan=1e-3), np.nan_to_num(ap, nan=0.5)
    O = 6
    tm = np.tile(np.linspace(0, 2.5, O), (2, 1))

    def refused(**kw):
        args = dict(nf=nf, no=np.array([6, 5]), O=O, mods=None, f0=f0, sp=sp, ap=ap, time_map=tm, fill=7.0)
        args.update(kw)
        rc, *outs = be.frames(fs, args.pop("fft", fft), args.pop("nf"), args.pop("no"), args.pop("O"), args.pop("mods"), **args)
        assert rc != 0 and be.error(), kw
        return outs
    for kw in (dict(no=np.array([6, 0])), dict(no=np.array([7, 5])), dict(no=np.array([6, -1])),
               dict(time_map=None, no=np.array([4, 2]), O=4), dict(time_map=None, no=np.array([4, 4]), O=4),
               dict(nf=np.array([5, 3])), dict(nf=np.array([4, 0])), dict(fft=1000), dict(fft=64), dict(fft=16384),
               dict(mods=mods_of(2, scale=[1.0, np.nan])), dict(mods=mods_of(2, ratio=[1.0, 0.0])),
               dict(mods=mods_of(2, ratio=[1.0, 1e-6])), dict(mods=mods_of(2, target=([5.0, 5.0], [0.1, -1.0])))):
        for o in refused(**kw):
            assert np.all(o == 7.0), kw
    # in place behind a time map: refused, the arrays as they were (f_stride == o_stride so that only the map decides)
    tm4 = np.tile(np.array([0, 0.5, 1.0, 1.5]), (2, 1))
    for o, a in zip(refused(no=np.array([4, 3]), O=4, time_map=tm4, inplace=True), (f0, sp, ap)):
        assert np.array_equal(o, a)
    # invalid values on the device: 1 for that frame, every other frame as without them
    no = np.array([6, 5], dtype=np.int32)
    good = dict(f0_scale=np.full((2, O), 1.5), formant_shift=np.full((2, O), 1.2), ap_gain=np.full((2, O), 0.9))
    rc, w_f0, w_sp, w_ap = be.frames(fs, fft, nf, no, O, None, f0=f0, sp=sp, ap=ap, time_map=tm, **good)
    assert rc == 0, be.error()
    rc, i_f0, i_sp, i_ap = be.frames(fs, fft, nf, no, O, None, f0=f0, sp=sp, ap=ap, time_map=tm)
    assert rc == 0, be.error()
    bad = {k: v.copy() for k, v in good.items()}
    bad["f0_scale"][0, [0, 2, 4]] = [np.nan, -1.0, np.inf]
    bad["formant_shift"][0, [0, 1, 2, 3, 5]] = [0.0, -1.2, np.nan, np.inf, 1.0 / fft]
    bad["ap_gain"][1, [0, 3, 4]] = [np.nan, -0.5, -np.inf]
    rc, g_f0, g_sp, g_ap = be.frames(fs, fft, nf, no, O, None, f0=f0, sp=sp, ap=ap, time_map=tm, **bad)
    assert rc == 0, be.error()
    for u in range(2):
        for j in range(no[u]):
            assert np.array_equal(g_f0[u, j], (i_f0 if not np.array_equal(bad["f0_scale"][u, j], 1.5) else w_f0)[u, j])
            assert np.array_equal(g_sp[u, j], (i_sp if not np.array_equal(bad["formant_shift"][u, j], 1.2) else w_sp)[u, j])
            if np.array_equal(bad["ap_gain"][u, j], 0.9):
                assert np.array_equal(g_ap[u, j], w_ap[u, j])
            else:                                       # a gain of 1, still within the bounds
                assert np.array_equal(g_ap[u, j], np.clip(i_ap[u, j], AP_LO, AP_HI))
    check_padding((g_f0, g_sp, g_ap), no)


# ---- the CPU suite -------------------------------------------------------------------------------------------------------
RATES = [16000, 48000, 192000]


@pytest.mark.parametrize("fs", RATES)
def test_identity_map_and_constant_curves_equal_modify_batch(be, fs):
    case_identity_map_and_constant_curves(be, fs)


@pytest.mark.parametrize("fs", RATES)
def test_integer_map_is_a_gather_of_modify_batch(be, fs):
    case_integer_map_is_a_gather(be, fs)


@pytest.mark.parametrize("fs", RATES)
def test_blend_only_is_bit_identical_to_the_statement(be, fs):
    case_blend_only(be, fs)


@pytest.mark.parametrize("fs", RATES)
def test_blend_and_per_frame_warp(be, fs):
    case_blend_and_per_frame_warp(be, fs)


# fft_size off the rate's default: the smallest transform at 16 kHz, the largest at 48 kHz (fft_of gives 1024 and 2048)
OFF_DEFAULT = [(16000, 128), (48000, 8192)]


@pytest.mark.parametrize("fs,fft", OFF_DEFAULT)
def test_identity_map_and_constant_curves_off_default_fft(be, fs, fft):
    assert fft != fft_of(fs)
    case_identity_map_and_constant_curves(be, fs, fft)


@pytest.mark.parametrize("fs,fft", OFF_DEFAULT)
def test_blend_and_per_frame_warp_off_default_fft(be, fs, fft):
    assert fft != fft_of(fs)
    case_blend_and_per_frame_warp(be, fs, fft)


def test_padding_refusals_and_invalid_curve_values(be):
    case_padding_and_refusals(be, 16000)


def test_target_f0_conversion_order_scale_and_ap_gain(be):
    """4: conversion on the source track, then the blend, the target, the scale; ap_gain within GetSafeAperiodicity's
    bounds.  Exact where the arithmetic is a copy or one multiply; converted frames to 1e-12"""
    fs, fft = 16000, 1024
    rng = np.random.default_rng(11)
    nf = np.array([60, 40, 30], dtype=np.int32)
    f0, _, ap = ragged(fs, fft, nf, seed=2)
    f0[2, :30] = 0.0                                                        # no voiced frame: nothing to convert
    O, no = 90, np.array([90, 50, 30], dtype=np.int32)
    tm = np.stack([np.linspace(0, 59, O), np.concatenate([np.linspace(0, 39, 50), np.zeros(40)]),
                   np.concatenate([np.arange(30.0), np.zeros(60)])])
    f0_target = rng.uniform(90, 300, (3, O))
    f0_target[:, ::4] = 0.0; f0_target[:, 1::8] = np.nan; f0_target[:, 3::16] = -5.0; f0_target[0, 2] = np.inf
    f0_scale = rng.uniform(0.5, 2.0, (3, O)); f0_scale[0, 5] = 0.0
    ap_gain = rng.uniform(0.0, 3.0, (3, O)); ap_gain[1, 7] = 0.0; ap_gain[0, 1] = 1.0
    target = ([5.3, 5.0, 4.0], [0.15, 0.2, 0.1])
    scales = [1.0, 1.2, 0.5]
    for curves, mods, tgt in ((dict(f0_target=f0_target, f0_scale=f0_scale, ap_gain=ap_gain), mods_of(3, scales, 1.0, target), target),
                              (dict(f0_target=f0_target, ap_gain=ap_gain), mods_of(3, scales), None),
                              (dict(f0_scale=f0_scale), mods_of(3, 1.0, 1.0, target), target),
                              (dict(), mods_of(3, scales, 1.0, target), target)):
        rc, g_f0, _, g_ap = be.frames(fs, fft, nf, no, O, mods, f0=f0, ap=ap, time_map=tm, **curves)
        assert rc == 0, be.error()
        for u in range(3):
            w_f0, _, w_ap, conv = statement(f0[u, :nf[u]], None, ap[u, :nf[u]], no[u], fs, fft, scale=scales[u],
                                            target=(tgt[0][u], tgt[1][u]) if tgt else None, time_map=tm[u],
                                            **{k: v[u] for k, v in curves.items()})
            got = g_f0[u, :no[u]]
            assert np.array_equal(got[~conv], w_f0[~conv], equal_nan=True), (u, list(curves))
            assert np.array_equal(got == 0, w_f0 == 0)
            live = conv & (w_f0 != 0)
            assert rel(got[live], w_f0[live]) <= 1e-12, (u, rel(got[live], w_f0[live]))
            assert np.array_equal(g_ap[u, :no[u]], w_ap), (u, list(curves))
            if "ap_gain" in curves:
                assert g_ap[u, :no[u]].min() >= AP_LO and g_ap[u, :no[u]].max() <= AP_HI
                assert np.any(g_ap[u, :no[u]] == AP_LO) and np.any(g_ap[u, :no[u]] == AP_HI)
            if "f0_target" in curves:                                        # voiced frames with a target ARE target * scale
                t = f0_target[u, :no[u]]
                sc = f0_scale[u, :no[u]] if "f0_scale" in curves else scales[u]
                took = (got != 0) & np.isfinite(t) & (t > 0) & np.isfinite(got)
                assert (took.any() or u == 2) and np.array_equal(got[took], (t * sc)[took])     # (2: nothing voiced)
        assert np.all(g_f0[2, :30] == 0.0)
        check_padding((g_f0, g_ap), no)


# ---- the whole chain in one call -----------------------------------------------------------------------------------------
def test_resynthesize_frames_equals_the_separate_calls(lib, be):
    """6: bit for bit analyze_batch -> modify_frames_batch -> synthesis_batch; and its refusals write nothing"""
    from world_amd import synth
    from world_amd.api import CheapTrickOption, D4COption, HarvestOption, WorldHipFrameCurves, frame_count
    fs = 16000
    fft = fft_of(fs)
    nb = fft // 2 + 1
    xs = [synth.vowel(fs, 0.3, seed=11).numpy(), synth.vowel(fs, 0.22, seed=5, base_f0=210.0).numpy()]
    x = np.zeros((2, max(len(v) for v in xs)))
    for u, v in enumerate(xs):
        x[u, :len(v)] = v
    xl = np.array([len(v) for v in xs], dtype=np.int32)
    hopt, copt, dopt = HarvestOption(71.0, 800.0, 5.0), CheapTrickOption(-0.15, 71.0, fft), D4COption(0.85)
    nf = np.array([frame_count(fs, int(n), 5.0) for n in xl], dtype=np.int32)
    F = int(nf.max())
    no = np.array([int(nf[0] * 1.5), int(nf[1] * 0.7)], dtype=np.int32)
    O = int(no.max())
    rng = np.random.default_rng(4)
    tm = np.stack([np.concatenate([np.linspace(0, nf[u] - 1, no[u]), np.zeros(O - no[u])]) for u in range(2)])
    curves = dict(d_time_map=tm, d_f0_scale=rng.uniform(0.8, 1.4, (2, O)), d_formant_shift=rng.uniform(0.85, 1.2, (2, O)),
                  d_ap_gain=rng.uniform(0.7, 1.3, (2, O)))
    cv = WorldHipFrameCurves(**{k: v.ctypes.data for k, v in curves.items()})
    mods = mods_of(2, scale=[1.1, 1.0], ratio=1.0, target=([5.2, 5.0], [0.2, 0.1]))
    yl = np.array([lib.world_hip_resynthesis_length(fs, int(n), 5.0, 1.0) for n in no], dtype=np.int32)
    Y = int(yl.max())
    ip = lambda a: a.ctypes.data_as(_ip)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def one_call(y, n_out=no, y_len=yl, curves=cv, fs=fs, copt=copt):
        return lib.world_hip_resynthesize_frames_batch(be.ctx, 2, fs, vp(x), x.shape[1], ip(xl), C.byref(hopt), C.byref(copt),
                                                       C.byref(dopt), mods, curves, ip(n_out), O, ip(y_len), Y, vp(y))
    y = np.zeros((2, Y))
    assert one_call(y) == 0, be.error()
    tpos, f0 = np.zeros((2, F)), np.zeros((2, F))
    sp, ap = np.zeros((2, F, nb)), np.zeros((2, F, nb))
    assert lib.world_hip_analyze_batch(be.ctx, 2, fs, vp(x), x.shape[1], ip(xl), C.byref(hopt), C.byref(copt), C.byref(dopt),
                                       F, vp(tpos), vp(f0), vp(sp), vp(ap)) == 0
    f0m, spm, apm = np.zeros((2, O)), np.zeros((2, O, nb)), np.zeros((2, O, nb))
    assert lib.world_hip_modify_frames_batch(be.ctx, 2, fs, fft, ip(nf), F, ip(no), O, mods, C.byref(cv), vp(f0), vp(f0m),
                                             vp(sp), vp(spm), vp(ap), vp(apm)) == 0, be.error()
    y2 = np.zeros((2, Y))
    assert lib.world_hip_synthesis_batch(be.ctx, 2, fs, 5.0, fft, ip(no), O, vp(f0m), vp(spm), vp(apm), ip(yl), Y, vp(y2)) == 0
    assert np.array_equal(y, y2) and np.max(np.abs(y)) > 0
    canary = np.full((2, Y), 3.0)
    for kw in (dict(y_len=yl - 1), dict(n_out=np.array([no[0], 1], dtype=np.int32)),
               dict(n_out=np.array([O + 1, no[1]], dtype=np.int32)), dict(curves=None)):    # (no map: n_out != n_frames)
        assert one_call(canary, **kw) != 0 and be.error(), kw
        assert np.all(canary == 3.0), kw
    # a pair (fs, fft_size) the reference leaves undefined is refused by the chain too, before any work ...
    assert one_call(canary, fs=48000, copt=CheapTrickOption(-0.15, 71.0, 256)) != 0
    assert "smallest fft_size for this fs is 512" in be.error() and np.all(canary == 3.0)
    # ... and an fft_size off the rate's default is served
    y3 = np.zeros((2, Y))
    assert one_call(y3, copt=CheapTrickOption(-0.15, 71.0, 256)) == 0, be.error()
    assert np.isfinite(y3).all() and np.max(np.abs(y3)) > 0 and not np.array_equal(y3, y)


# ---- the Python helpers (no library needed) ------------------------------------------------------------------------------
def test_time_map_helpers():
    import torch
    from world_amd.api import hold_time_map, uniform_time_map
    m = uniform_time_map(11, 21, device="cpu")
    assert m.dtype == torch.float64 and m.shape == (21,) and m[0] == 0 and m[-1] == 10 and m[1] == 0.5
    assert uniform_time_map(5, 1, device="cpu").tolist() == [0.0]
    h = hold_time_map(10, [(0, 0), (4, 4), (4, 8), (9, 13)], device="cpu")
    assert h.tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4, 5, 6, 7, 8, 9]
    assert hold_time_map(3, [(0, 0), (8, 4)], device="cpu").tolist() == [0, 2, 2, 2, 2]       # clamped to the source
    with pytest.raises(ValueError):
        hold_time_map(10, [(0, 1), (4, 4)], device="cpu")
    with pytest.raises(ValueError):
        hold_time_map(10, [(0, 0), (4, 4), (5, 4)], device="cpu")
