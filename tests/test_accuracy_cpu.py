"""The accuracy yardstick on the CPU.

1. The long double oracle (oracle/libworld_oracle_wide.so, "W") really is the more precise answer: its primitives are
   checked against mpmath at 40 digits on inputs whose outputs cancel (a large DC offset under an FFT, a prefix sum
   differenced at the noise floor, a mirror image that cancels its own spectrum), where the double build's rounding shows.
   W's error must be at least 100 times below the double build's.
2. The accuracy criterion of tests/util.py (e_H against W, bounded by e_R against W) on the emulated kernel units that
   tests/emu compiles as the GPU does (D4C, StoneMask, Synthesis), at 16 and 48 kHz, so that the metric itself is
   exercised without a GPU.  tests/test_gpu_accuracy.py runs it on the MI355X at every dispatch branch.
3. The same criterion with fft_size off the rate's default (CheapTrick on the classic emulation).
"""
import ctypes as C

import numpy as np
import pytest

from backends import emu  # noqa: F401 (a fixture)
from util import ACC_A, ACC_C, ULP, assert_accurate, ct_floor, discrete_agreement, rel_errors
from util import offdefault_f0 as _f0, synth_inputs as _synth_inputs, utterance as _signal

mpmath = pytest.importorskip("mpmath")


def _wide_or_skip():
    from oracle.loader import WideOracle, build, wide_is_wider
    if not wide_is_wider():
        pytest.skip(f"long double is not wider than double on this host (eps {np.finfo(np.longdouble).eps})")
    build()
    return WideOracle()


@pytest.fixture(scope="module")
def wide():
    return _wide_or_skip()


@pytest.fixture(scope="module")
def mp40():
    old = mpmath.mp.dps
    mpmath.mp.dps = 40
    yield mpmath.mp
    mpmath.mp.dps = old


# ---- 40-digit restatements of the primitives (inputs are the same doubles both builds see) ----
def _mp_fft(a, sign):
    """unscaled complex DFT, exp(sign 2 pi i jk / n), radix 2"""
    n = len(a)
    if n == 1:
        return list(a)
    even, odd = _mp_fft(a[0::2], sign), _mp_fft(a[1::2], sign)
    out = [None] * n
    for k in range(n // 2):
        t = mpmath.expjpi(mpmath.mpf(sign * 2 * k) / n) * odd[k]
        out[k], out[k + n // 2] = even[k] + t, even[k] - t
    return out


def _mp_rfft(x):
    X = _mp_fft([mpmath.mpc(float(v)) for v in x], -1)
    return X[: len(x) // 2 + 1]


def _mp_irfft_unscaled(X):
    n = 2 * (len(X) - 1)
    full = [mpmath.mpc(float(X[0].real))] + [mpmath.mpc(float(v.real), float(v.imag)) for v in X[1:-1]] + \
           [mpmath.mpc(float(X[-1].real))]
    full += [mpmath.conj(full[n - k]) for k in range(n // 2 + 1, n)]
    return [v.real for v in _mp_fft(full, +1)]


def _mp_interp1q(x0, dx, y, xi):
    """the bin is the double expression both builds use; the fraction and the value are exact"""
    out = []
    for q in xi:
        b = int((q - x0) / dx)
        frac = (mpmath.mpf(float(q)) - mpmath.mpf(x0)) / mpmath.mpf(dx) - b
        dy = y[b + 1] - y[b] if b < len(y) - 1 else 0
        out.append(y[b] + dy * frac)
    return out


def _mp_linear_smoothing(spec, width, fs, fft_size):
    half = fft_size // 2
    bnd = int(width * fft_size / fs) + 1
    seg, acc = [], mpmath.mpf(0)
    for i in range(half + 2 * bnd + 1):
        m = spec[bnd - i] if i < bnd else spec[i - bnd] if i < half + bnd else spec[half - (i - (half + bnd))]
        acc += mpmath.mpf(float(m)) * fs / fft_size
        seg.append(acc)
    axis = [i / fft_size * fs - width / 2.0 for i in range(half + 1)]
    origin, step = -(bnd - 0.5) * fs / fft_size, fs / fft_size
    lo = _mp_interp1q(origin, step, seg, axis)
    hi = _mp_interp1q(origin, step, seg, [a + width for a in axis])
    return [(h - l) / mpmath.mpf(width) for h, l in zip(hi, lo)]


def _mp_dc_correction(spec, f0, fs, fft_size):
    upper = 2 + int(f0 * fft_size / fs)
    axis = [i * fs / fft_size for i in range(upper)]
    y = [mpmath.mpf(float(v)) for v in spec[: upper + 1]]
    rep = _mp_interp1q(f0 - axis[0], -fs / fft_size, y, axis[: upper - 1])
    return [y[i] + rep[i] for i in range(upper - 1)] + [mpmath.mpf(float(v)) for v in spec[upper - 1:]]


def _mp_interp1(x, y, xi):
    out, c, n = [], 0, len(x)
    for q in xi:
        while c < n and x[c] <= q:
            c += 1
        k = min(max(c, 1), n - 1)
        s = (mpmath.mpf(float(q)) - float(x[k - 1])) / (mpmath.mpf(float(x[k])) - float(x[k - 1]))
        out.append(mpmath.mpf(float(y[k - 1])) + s * (mpmath.mpf(float(y[k])) - float(y[k - 1])))
    return out


def _errors(got, exact):
    """element-wise relative errors against the 40-digit answer (zeros of the exact answer are skipped)"""
    ex = np.array([float(v) for v in exact])
    err = np.array([float(abs(mpmath.mpf(float(g)) - e) / abs(e)) if e != 0 else 0.0 for g, e in zip(got, exact)])
    return err[ex != 0]


def _assert_wider(what, e_wide, e_double):
    mw, md = float(np.mean(e_wide)), float(np.mean(e_double))
    xw, xd = float(np.max(e_wide)), float(np.max(e_double))
    print(f"{what}: mean W {mw:.2e} double {md:.2e}; max W {xw:.2e} double {xd:.2e}")
    assert md > 0 and 100 * mw <= md, f"{what}: mean error W {mw:.3e} not 100x below double {md:.3e}"
    assert 100 * xw <= xd, f"{what}: max error W {xw:.3e} not 100x below double {xd:.3e}"


@pytest.mark.parametrize("n", [64, 512, 4096])
def test_wide_rfft_against_mpmath(wide, port_oracle, mp40, n):
    rng = np.random.default_rng(n)
    x = 1e6 + rng.standard_normal(n)          # the offset lands in bin 0 and cancels everywhere else
    exact = _mp_rfft(x)[1:]
    for part in ("real", "imag"):
        ex = [getattr(v, part) for v in exact[:-1]]
        e_w = _errors(getattr(wide.rfft(x), part)[1:-1], ex)
        e_d = _errors(getattr(port_oracle.rfft(x), part)[1:-1], ex)
        _assert_wider(f"rfft {n} {part}", e_w, e_d)


@pytest.mark.parametrize("n", [64, 512, 4096])
def test_wide_irfft_against_mpmath(wide, port_oracle, mp40, n):
    rng = np.random.default_rng(n + 1)
    x = rng.standard_normal(n)
    x[0] = 1e7                                 # a spike: every output but the first cancels it
    X = np.fft.rfft(x)
    exact = _mp_irfft_unscaled(X)[1:]
    _assert_wider(f"irfft {n}", _errors(wide.irfft_unscaled(X)[1:], exact),
                  _errors(port_oracle.irfft_unscaled(X)[1:], exact))


def test_wide_linear_smoothing_against_mpmath(wide, port_oracle, mp40):
    """a power spectrum with a 14-decade floor: the prefix sum is differenced far below its running total"""
    fs, fft_size, width = 16000, 1024, 2.0 / 3.0 * 143.7
    k = np.arange(fft_size // 2 + 1)
    rng = np.random.default_rng(7)
    spec = np.exp(-k / 12.0) * (1.0 + 0.5 * rng.random(len(k))) + 1e-14 * rng.random(len(k))
    exact = _mp_linear_smoothing(spec, width, fs, fft_size)
    _assert_wider("linear_smoothing", _errors(wide.linear_smoothing(spec, width, fs, fft_size), exact),
                  _errors(port_oracle.linear_smoothing(spec, width, fs, fft_size), exact))


def _dc_correction(o, spec, f0, fs, fft_size):
    from oracle.loader import _p
    spec = np.ascontiguousarray(spec, dtype=np.float64)
    out = np.zeros(fft_size // 2 + 1)
    o.lib.wo_dc_correction(_p(spec), C.c_double(f0), fs, fft_size, _p(out))
    return out


def test_wide_dc_correction_against_mpmath(wide, port_oracle, mp40):
    """a spectrum linear in frequency about f0 / 2 cancels its own mirror image: only the small term survives"""
    fs, fft_size, f0 = 48000, 2048, 431.3
    f = np.arange(fft_size // 2 + 1) * fs / fft_size
    spec = 1e3 * (f - f0 / 2.0) + 1e-6 * np.random.default_rng(3).random(len(f))
    exact = _mp_dc_correction(spec, f0, fs, fft_size)
    upper = 1 + int(f0 * fft_size / fs)
    _assert_wider("dc_correction", _errors(_dc_correction(wide, spec, f0, fs, fft_size)[:upper], exact[:upper]),
                  _errors(_dc_correction(port_oracle, spec, f0, fs, fft_size)[:upper], exact[:upper]))


def test_wide_interp1_against_mpmath(wide, port_oracle, mp40):
    """an alternating sequence of large values interpolated near its zero crossings"""
    rng = np.random.default_rng(11)
    x = np.cumsum(rng.uniform(0.5, 1.5, 200))
    y = 1e8 * (-1.0) ** np.arange(200) + rng.standard_normal(200)
    xi = np.sort((x[:-1] + x[1:]) / 2.0 + rng.uniform(-1e-3, 1e-3, 199))
    exact = _mp_interp1(x, y, xi)
    _assert_wider("interp1", _errors(wide.interp1(x, y, xi), exact), _errors(port_oracle.interp1(x, y, xi), exact))


# ---- the criterion on the emulated units ----
def _track(kind, fs, nf, seed):
    """F0 from the reference's Harvest or a caller-made track in the style of tests/fuzz_given_f0.py"""
    rng = np.random.default_rng(seed)
    if kind == "steps":
        f0 = np.repeat(rng.uniform(60.0, 600.0, nf // 7 + 1), 7)[:nf]
    elif kind == "low":
        f0 = rng.uniform(20.0, 90.0, nf)
    else:                                                              # sparse
        f0 = np.where(rng.random(nf) < 0.3, rng.uniform(80.0, 400.0, nf), 0.0)
    f0[rng.random(nf) < 0.15] = 0.0
    return f0


def d4c_exit_rows(ap):
    """rows LoveTrain (or F0 = 0) left at 1 - 1e-12 throughout"""
    return np.all(np.asarray(ap) == 1.0 - 1e-12, axis=1)


def stonemask_outcome(out, f0):
    """0 = unvoiced / out of range, 1 = fell back to the input F0, 2 = refined"""
    out, f0 = np.asarray(out), np.asarray(f0)
    return np.where(out == 0.0, 0, np.where(out == f0, 1, 2))


@pytest.mark.parametrize("fs", [16000, 48000])
@pytest.mark.parametrize("f0_kind", ["harvest", "steps", "low", "sparse"])
def test_emulated_units_against_wide_oracle(emu, ref_oracle, fs, f0_kind):
    wide = _wide_or_skip()
    from world_amd import synth
    x = synth.utterance(4 if f0_kind == "harvest" else 5, fs, 0.25).numpy()
    tp, f0 = ref_oracle.harvest(x, fs)
    if f0_kind != "harvest":
        f0 = _track(f0_kind, fs, len(tp), fs + len(f0_kind))
    fft = ref_oracle.cheaptrick_fft_size(fs)

    out = {k: o.stonemask(x, fs, tp, f0) for k, o in (("H", emu), ("R", ref_oracle), ("W", wide))}
    w_only = discrete_agreement(f"stonemask {fs} {f0_kind}", *(stonemask_outcome(out[k], f0) for k in "HRW"))
    refined = np.flatnonzero(stonemask_outcome(out["R"], f0) == 2)
    keep = np.setdiff1d(refined, w_only)
    if keep.size:
        assert_accurate(f"emu stonemask {fs} {f0_kind}", out["H"][keep, None], out["R"][keep, None], out["W"][keep, None])

    sp = ref_oracle.cheaptrick(x, fs, tp, f0, fft_size=fft)
    for th in (0.85, 0.0):
        ap = {k: o.d4c(x, fs, tp, f0, fft, threshold=th) for k, o in (("H", emu), ("R", ref_oracle), ("W", wide))}
        w_only = discrete_agreement(f"d4c exits {fs} {f0_kind} {th}", *(d4c_exit_rows(ap[k]) for k in "HRW"))
        assert_accurate(f"emu d4c {fs} {f0_kind} th={th}", ap["H"], ap["R"], ap["W"], exclude_rows=w_only)

    y = {k: o.synthesis(f0, sp, ap["R"], fft, 5.0, fs, len(x)) for k, o in (("H", emu), ("R", ref_oracle), ("W", wide))}
    assert_accurate(f"emu synthesis {fs} {f0_kind}", y["H"][None], y["R"][None], y["W"][None], peak=True)


# ---- fft_size off the rate's default (tests/test_gpu_offdefault_fft.py runs every template on the MI355X) ----
@pytest.mark.parametrize("fs,fft,kinds", [(16000, 128, ("harvest", "floor_edge")), (16000, 2048, ("harvest", "floor_edge"))])
def test_emulated_cheaptrick_off_default(emu, ref_oracle, wide, fs, fft, kinds):
    x = _signal(fs, 0.2)
    for kind in kinds:
        tp, f0 = _f0(kind, ref_oracle, x, fs, fft)
        if kind == "floor_edge":
            assert np.any(f0 <= ct_floor(fs, fft)) and np.any(f0 > ct_floor(fs, fft))
        h, r, w = (o.cheaptrick(x, fs, tp, f0, fft_size=fft) for o in (emu, ref_oracle, wide))
        assert_accurate(f"emu cheaptrick off-default {fs}/{fft} {kind}", h, r, w)


@pytest.mark.parametrize("threshold", [0.85, 0.0])
@pytest.mark.parametrize("fs,fft", [(16000, 128), (16000, 4096)])
def test_emulated_d4c_off_default(emu, ref_oracle, wide, fs, fft, threshold):
    x = _signal(fs, 0.2)
    tp, f0 = ref_oracle.harvest(x, fs)
    ap = {k: o.d4c(x, fs, tp, f0, fft, threshold=threshold) for k, o in (("H", emu), ("R", ref_oracle), ("W", wide))}
    w_only = discrete_agreement(f"d4c exits {fs}/{fft} {threshold}", *(d4c_exit_rows(ap[k]) for k in "HRW"))
    assert_accurate(f"emu d4c off-default {fs}/{fft} th={threshold}", ap["H"], ap["R"], ap["W"], exclude_rows=w_only)


def test_emulated_d4c_grids_nest_bit_for_bit(emu, ref_oracle, wide):
    """bin i of the fft_size N grid and bin 2 i of the 2 N grid are the same double i fs / N: ap_2N[:, ::2] == ap_N; and the
    cached grid follows fs at one fft_size"""
    fs = 16000
    x = _signal(fs, 0.2)
    tp, f0 = ref_oracle.harvest(x, fs)
    ap = {}
    for fft in (512, 1024, 2048, 512):
        got = emu.d4c(x, fs, tp, f0, fft)
        assert fft not in ap or np.array_equal(got, ap[fft])
        ap[fft] = got
    assert not np.all(d4c_exit_rows(ap[512]))
    assert np.array_equal(ap[1024][:, ::2], ap[512]) and np.array_equal(ap[2048][:, ::2], ap[1024])
    x2 = _signal(24000, 0.12)
    tp2, f02 = ref_oracle.harvest(x2, 24000)
    h, r, w = (o.d4c(x2, 24000, tp2, f02, 512) for o in (emu, ref_oracle, wide))       # the size of the last call, another rate
    w_only = discrete_agreement("d4c exits 24000/512", *(d4c_exit_rows(v) for v in (h, r, w)))
    assert_accurate("emu d4c off-default 24000/512 after 16000/512", h, r, w, exclude_rows=w_only)
    assert np.array_equal(emu.d4c(x, fs, tp, f0, 512), ap[512])


@pytest.mark.parametrize("fs,fft", [(16000, 256), (16000, 4096)])
def test_emulated_synthesis_off_default(emu, ref_oracle, wide, fs, fft):
    x, f0, sp, ap = _synth_inputs(ref_oracle, fs, fft, 0.2)        # (asserts voiced and default-F0 pulses)
    y = {k: o.synthesis(f0, sp, ap, fft, 5.0, fs, len(x)) for k, o in (("H", emu), ("R", ref_oracle), ("W", wide))}
    assert_accurate(f"emu synthesis off-default {fs}/{fft}", y["H"][None], y["R"][None], y["W"][None], peak=True)


def test_criterion_catches_a_float_slip(ref_oracle):
    """the criterion's own sanity: a result rounded through float at one bin, or all bins, fails it"""
    wide = _wide_or_skip()
    from world_amd import synth
    fs = 16000
    x = synth.utterance(2, fs, 0.2).numpy()
    tp, f0 = ref_oracle.harvest(x, fs)
    r = ref_oracle.d4c(x, fs, tp, f0, 1024)
    w = wide.d4c(x, fs, tp, f0, 1024)
    assert_accurate("d4c R vs itself", r, r, w, log=False)
    one = r.copy()
    i = np.unravel_index(np.argmax(rel_errors(r, w) * (r < 0.5)), r.shape)
    one[i] = np.float32(one[i] * (1 + 3e-8))
    with pytest.raises(AssertionError):
        assert_accurate("one bin in float", one, r, w, log=False)
    with pytest.raises(AssertionError):
        assert_accurate("all bins in float", r.astype(np.float32).astype(np.float64), r, w, log=False)
    assert ACC_A <= 10 and ACC_C <= 64 and ULP == 2.0 ** -52
