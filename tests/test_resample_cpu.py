"""Sampling-rate conversion (include/world_hip.h: world_hip_resample_batch and its host arithmetic) through the
host-compiled kernels (tests/emu/libworld_emu.so), against a NumPy statement of the header's rule written here.  The
reference has no resampler: the statement is the oracle.  The cases are functions of a backend, so that
tests/test_resample_gpu.py runs the same ones through the shipped library.

Tolerances.
  table   2e-14 absolute (the coefficients are at most 1 in magnitude): the float64 NumPy table (np.i0, np.sinc) and an
          80-bit evaluation by another route (series I0, split pi, integer arguments) differ by at most 4.3e-15 over these
          pairs and presets; the bar is about five times that.  Exactly 0.0 wherever |q| >= zeros * B.
  sum     with the library's own table: equality of every bit (NaN compared as equal).  acc = acc + x * c in ascending tap
          order under -ffp-contract=off is the same sequence of IEEE operations in NumPy and in the kernel.
  filter  BEST 2.5e-7, FAST 2e-4 (pass band at 0.1 and 0.5 of the lower Nyquist rate; BEST also at 0.8; alias of a sine at
          1.15 x the output Nyquist rate for the downward pairs): the bars were set from the float64 statement evaluated over
          exactly these pairs -- BEST worst error 4.6e-8 and worst alias 9.7e-8, FAST 7.1e-5 and 6.6e-5.  The sum is bit-equal
          to the statement and the table within 1e-14 of it, so the bars carry over.  With this file's own signal lengths
          and margins (2 W output samples left out at both ends, 500 or more compared) the cases print BEST 4.5e-8 / 9.7e-8
          and FAST 7.4e-5 / 6.6e-5, through the emulated kernels and on the GPU alike: a margin of 2.5-2.7x under the bars."""
import ctypes as C
import math

import numpy as np
import pytest

import backends
from backends import SENTINEL_F64 as SENTINEL, cached, cpu_backend, lib, same_bits  # noqa: F401 (lib: a fixture)

_ip = C.POINTER(C.c_int)
T = 256                              # outputs per workgroup at these ratios (resample.inc: kResampleThreads)
BEST = (64, 0.9475937167399596, 14.769656459379492)
FAST = (16, 0.85, 8.555504641634386)
CUSTOM = (4, 0.9, 5.0)
PAIRS = [(8000, 16000), (48000, 16000), (44100, 48000), (48000, 44100), (44100, 16000)]
FAST_ONLY = [(192000, 16000)]
# (fs_in, fs_out, design): the presets in full, the custom design at two pairs
DESIGNS = ([(a, b, BEST) for a, b in PAIRS] + [(a, b, FAST) for a, b in PAIRS + FAST_ONLY] +
           [(44100, 48000, CUSTOM), (48000, 16000, CUSTOM)])
DESIGN_IDS = ["%d-%d-%s" % (a, b, {BEST: "best", FAST: "fast", CUSTOM: "custom"}[d]) for a, b, d in DESIGNS]
# a decimation steep enough that 256 outputs' input span (255 * 48 + 768 doubles) exceeds a workgroup's LDS budget: the
# kernel then takes fewer outputs per workgroup (resample.inc: resample_plan)
STEEP = (48000, 1000, (8, 0.9, 6.0))
TABLE_TOL = 2e-14
BARS = {BEST: 2.5e-7, FAST: 2e-4}


# ---- the host statement (NumPy, float64) ---------------------------------------------------------------------------------
def ratio(fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g                                  # L, M


def shape(fs_in, fs_out, design):
    L, M = ratio(fs_in, fs_out)
    B = max(L, M)
    return L, M, -((-design[0] * B) // L)                           # W = ceil(zeros B / L)


def out_length(n_in, fs_in, fs_out):
    L, M = ratio(fs_in, fs_out)
    return -((-n_in * L) // M)                                      # (Python integers: exact)


def table(fs_in, fs_out, design):
    """c[p][i] = h(q), q = p + (W - 1 - i) L -> ([L, 2 W] float64, q, zeros * B)"""
    zeros, rolloff, beta = design
    L, M, W = shape(fs_in, fs_out, design)
    B = max(L, M)
    q = np.arange(L, dtype=np.int64)[:, None] + (W - 1 - np.arange(2 * W, dtype=np.int64)[None, :]) * L
    zb = zeros * B
    inside = np.abs(q) < zb
    u = np.where(inside, q / float(zb), 0.0)
    s = rolloff * min(L, M) / M
    h = s * np.sinc(rolloff * q / B) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta)
    return np.where(inside, h, 0.0), q, zb


def resample(x, fs_in, fs_out, c):
    """y[m] = sum over i, ascending, of x[k0 - W + 1 + i] * c[p][i]; acc = acc + x * c, each operation rounded"""
    L, M = ratio(fs_in, fs_out)
    W = c.shape[1] // 2
    m = np.arange(out_length(len(x), fs_in, fs_out), dtype=np.int64)
    k0, p = (m * M) // L, (m * M) % L
    assert k0.max() <= len(x) - 1
    xp = np.concatenate([np.zeros(W), np.asarray(x, dtype=np.float64), np.zeros(W)])     # +0.0 outside [0, n_in)
    acc = np.zeros(len(m))
    with np.errstate(all="ignore"):
        for i in range(2 * W):
            acc = acc + xp[k0 + 1 + i] * c[p, i]                   # xp index of k = k0 - W + 1 + i
    return acc


# ---- a backend: the C calls on arrays that live where the library wants them ---------------------------------------------
def option(design):
    from world_amd.api import WorldHipResampleOption
    return None if design is None else WorldHipResampleOption(int(design[0]), float(design[1]), float(design[2]))


def library_table(lib, fs_in, fs_out, design):
    """world_hip_resample_shape + _taps -> [L, 2 W]"""
    L, M, W = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    opt = option(design)
    ref = C.byref(opt) if opt is not None else None
    assert lib.world_hip_resample_shape(fs_in, fs_out, ref, C.byref(L), C.byref(M), C.byref(W)) == 0
    c = np.full((L.value, 2 * W.value), SENTINEL)
    assert lib.world_hip_resample_taps(fs_in, fs_out, ref, C.c_void_p(c.ctypes.data)) == 0
    return c


class Backend(backends.Backend):
    """world_hip_resample_batch on the arrays of backends.Backend"""

    def call(self, n_utt, fs_in, fs_out, design, d_x, x_stride, x_len, d_y, y_stride):
        """the C call itself on device arrays (None: NULL)"""
        opt = option(design)
        xl = None if x_len is None else np.ascontiguousarray(x_len, dtype=np.int32)
        return self.lib.world_hip_resample_batch(
            self.ctx, n_utt, fs_in, fs_out, C.byref(opt) if opt is not None else None,
            None if d_x is None else C.c_void_p(self.addr(d_x)), x_stride, None if xl is None else xl.ctypes.data_as(_ip),
            None if d_y is None else C.c_void_p(self.addr(d_y)), y_stride)

    def resample(self, rows, fs_in, fs_out, design, x_pad=5, y_pad=7):
        """rows: list of 1-D arrays -> (n_out per row, y [B, y_stride] on the host, pre-filled with SENTINEL)"""
        n = [len(r) for r in rows]
        n_out = [out_length(k, fs_in, fs_out) for k in n]
        x = np.full((len(rows), max(n) + x_pad), SENTINEL)
        for u, r in enumerate(rows):
            x[u, :n[u]] = r
        d_x, d_y = self.dev(x), self.dev(np.full((len(rows), max(n_out) + y_pad), SENTINEL))
        rc = self.call(len(rows), fs_in, fs_out, design, d_x, x.shape[1], n, d_y, max(n_out) + y_pad)
        assert rc == 0, self.error()
        return n_out, self.host(d_y)


be = cpu_backend(Backend)


# ---- inputs, made once and shared (never changed) ------------------------------------------------------------------------
def lengths_for(fs_in, fs_out, design):
    """{1, 2, W, 2 W + 1, 1000, 3001} and the input lengths that put n_out at T - 1, T, T + 1 and 2 T + 1 -- or, where the
    ratio cannot produce that count (8 -> 16 kHz gives even counts only), at the next count it can"""
    L, M, W = shape(fs_in, fs_out, design)
    n = [1, 2, W, 2 * W + 1, 1000, 3001]
    for target in (T - 1, T, T + 1, 2 * T + 1):
        n_in = -((-target * M) // L)                                # the shortest input with n_out >= target ...
        while out_length(n_in - 1, fs_in, fs_out) >= target and n_in > 1:
            n_in -= 1
        assert out_length(n_in, fs_in, fs_out) >= target > out_length(n_in - 1, fs_in, fs_out)
        n.append(n_in)
    return n


def rows_for(fs_in, fs_out, design):
    def make():
        rng = np.random.default_rng(fs_in + 3 * fs_out + design[0])
        return [rng.standard_normal(k) for k in lengths_for(fs_in, fs_out, design)]
    return cached(("rows", fs_in, fs_out, design), make)


def lib_table(lib, fs_in, fs_out, design):
    return cached(("table", id(lib), fs_in, fs_out, design), lambda: library_table(lib, fs_in, fs_out, design))


def check_rows(got, n_out, rows, fs_in, fs_out, c):
    for u, r in enumerate(rows):
        want = resample(r, fs_in, fs_out, c)
        assert len(want) == n_out[u]
        assert same_bits(got[u, :n_out[u]], want), (u, len(r), float(np.nanmax(np.abs(got[u, :n_out[u]] - want))))
        assert np.all(got[u, n_out[u]:] == SENTINEL), (u, "written beyond n_out")


# ---- the cases -----------------------------------------------------------------------------------------------------------
def case_lengths_and_shapes(lib):
    from world_amd.api import resample_length
    for fs_in, fs_out in PAIRS + FAST_ONLY + [(16000, 16000), (44100, 48001), (1, 1), (3, 2)]:
        for n in (1, 2, 7, 147, 148, 1000, 2 ** 30):
            want = out_length(n, fs_in, fs_out)
            want = want if want <= 2 ** 31 - 1 else -1
            assert lib.world_hip_resample_length(n, fs_in, fs_out) == want, (n, fs_in, fs_out)
            if want > 0:
                assert resample_length(n, fs_in, fs_out) == want
    for args in ((0, 8000, 16000), (-1, 8000, 16000), (10, 0, 16000), (10, 8000, 0), (10, -8000, 16000), (2 ** 30, 8000, 48000)):
        assert lib.world_hip_resample_length(*args) == -1, args
    assert lib.world_hip_resample_length(2 ** 31 - 1, 16000, 16000) == 2 ** 31 - 1
    for fs_in, fs_out, design in DESIGNS:
        L, M, W = C.c_int(), C.c_int(), C.c_int()
        opt = option(design)
        assert lib.world_hip_resample_shape(fs_in, fs_out, C.byref(opt), C.byref(L), C.byref(M), C.byref(W)) == 0
        assert (L.value, M.value, W.value) == shape(fs_in, fs_out, design)
    for (fs_in, fs_out, design), want in (((44100, 16000, BEST), (160, 441, 177)), ((192000, 16000, FAST), (1, 12, 192)),
                                          ((8000, 16000, BEST), (2, 1, 64)), ((44100, 48000, None), (160, 147, 64))):
        L, M, W = C.c_int(), C.c_int(), C.c_int()
        opt = option(design)
        assert lib.world_hip_resample_shape(fs_in, fs_out, C.byref(opt) if opt else None, C.byref(L), C.byref(M), C.byref(W)) == 0
        assert (L.value, M.value, W.value) == want
    from world_amd.api import WorldHipResampleOption
    for quality, want in ((0, BEST), (1, FAST)):
        o = WorldHipResampleOption(-1, -1.0, -1.0)
        lib.world_hip_resample_option(quality, C.byref(o))
        assert (o.zeros, o.rolloff, o.kaiser_beta) == want


# (fs_in, fs_out, design) the host arithmetic refuses, and a word its message must hold
BAD_SHAPES = [((0, 16000, BEST), "rates"), ((16000, 0, BEST), "rates"), ((-8000, 16000, BEST), "rates"),
              ((8000, 16000, (0, 0.9, 5.0)), "zeros"), ((8000, 16000, (257, 0.9, 5.0)), "zeros"),
              ((8000, 16000, (16, 0.0, 5.0)), "rolloff"), ((8000, 16000, (16, 1.0000001, 5.0)), "rolloff"),
              ((8000, 16000, (16, float("nan"), 5.0)), "rolloff"), ((8000, 16000, (16, 0.9, float("nan"))), "beta"),
              ((8000, 16000, (16, 0.9, float("inf"))), "beta"), ((8000, 16000, (16, 0.9, -0.1)), "beta"),
              ((8000, 16000, (16, 0.9, 40.5)), "beta"),
              ((48000, 1000, (256, 0.9, 5.0)), "taps"),                           # 2 W = 24576 > 4096
              ((44100, 48001, BEST), "L = 48001")]                                # L * 2 W = 6.1 M coefficients > 2^21


def case_host_refusals(lib):
    for (fs_in, fs_out, design), word in BAD_SHAPES:
        opt = option(design)
        L, M, W = C.c_int(-5), C.c_int(-5), C.c_int(-5)
        assert lib.world_hip_resample_shape(fs_in, fs_out, C.byref(opt), C.byref(L), C.byref(M), C.byref(W)) == 1
        assert word in lib.world_hip_last_error().decode(), (word, lib.world_hip_last_error().decode())
        assert (L.value, M.value, W.value) == (-5, -5, -5)
        c = np.full(64, SENTINEL)
        assert lib.world_hip_resample_taps(fs_in, fs_out, C.byref(opt), C.c_void_p(c.ctypes.data)) == 1
        assert np.all(c == SENTINEL)
    assert lib.world_hip_resample_taps(8000, 16000, None, None) == 1


def case_batch_refusals(be):
    """every refusal of the header, each with the output (and the input) left as it was"""
    x = np.arange(2 * 120, dtype=np.float64).reshape(2, 120) + 1.0
    d_x = be.dev(x)
    d_y = be.dev(np.full((2, 300), SENTINEL))
    ok = dict(n_utt=2, fs_in=8000, fs_out=16000, design=BEST, d_x=d_x, x_stride=120, x_len=[100, 120], d_y=d_y, y_stride=300)

    def refused(word, **change):
        a = dict(ok, **change)
        rc = be.call(a["n_utt"], a["fs_in"], a["fs_out"], a["design"], a["d_x"], a["x_stride"], a["x_len"], a["d_y"], a["y_stride"])
        assert rc == 1, change
        assert word in be.error(), (change, be.error())
        assert np.all(be.host(d_y) == SENTINEL) and np.array_equal(be.host(d_x), x), change

    refused("n_utt", n_utt=0)
    refused("n_utt", n_utt=-3)
    refused("null", d_x=None)
    refused("null", d_y=None)
    refused("null", x_len=None)
    refused("x_length", x_len=[100, 0])
    refused("x_length", x_len=[-1, 120])
    refused("x_length", x_len=[100, 121])                                       # beyond x_stride
    refused("y_stride", y_stride=239)                                           # 120 samples become 240
    refused("y_stride", fs_in=16000, fs_out=16000, y_stride=119)                # equal rates refuse alike
    for (fs_in, fs_out, design), word in BAD_SHAPES:
        refused(word, fs_in=fs_in, fs_out=fs_out, design=design, x_len=[1, 1])
    # an output range that overlaps the input range: the same array, and one that starts inside it
    both = be.dev(np.full((4, 300), SENTINEL))
    xl = np.array([100, 120], dtype=np.int32)
    for fs_out in (16000, 8000):
        for offset in (0, 8 * 450):                                             # (bytes into `both`: 1.5 rows)
            rc = be.lib.world_hip_resample_batch(be.ctx, 2, 8000, fs_out, None, C.c_void_p(be.addr(both)), 300,
                                                 xl.ctypes.data_as(_ip), C.c_void_p(be.addr(both) + offset), 300)
            assert rc == 1 and "overlap" in be.error(), (fs_out, offset)
            assert np.all(be.host(both) == SENTINEL)
    # and the call the refusals were variations of goes through
    assert be.call(**{k: ok[k] for k in ("n_utt", "fs_in", "fs_out", "design", "d_x", "x_stride", "x_len", "d_y", "y_stride")}) == 0, be.error()
    assert np.all(be.host(d_y)[0, :200] != SENTINEL) and np.all(be.host(d_y)[0, 200:] == SENTINEL)


def case_table(lib, fs_in, fs_out, design):
    want, q, zb = table(fs_in, fs_out, design)
    got = lib_table(lib, fs_in, fs_out, design)
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want)))
    print(f"table {fs_in} -> {fs_out} {design}: {got.shape}, max |library - statement| = {err:.3g}")
    assert err <= TABLE_TOL
    outside = np.abs(q) >= zb
    assert np.all(got[outside].view(np.uint64) == 0)                            # exactly +0.0
    assert float(np.max(np.abs(got))) <= 1.0


def case_sum(be, fs_in, fs_out, design):
    """with the library's own table: every output bit-equal to the statement's, the sentinel beyond n_out untouched"""
    rows = rows_for(fs_in, fs_out, design)
    n_out, got = be.resample(rows, fs_in, fs_out, design)
    assert got.shape[1] > max(n_out)
    check_rows(got, n_out, rows, fs_in, fs_out, lib_table(be.lib, fs_in, fs_out, design))


def case_null_option_is_best(be):
    rows = rows_for(44100, 48000, BEST)[3:5]
    n_out, a = be.resample(rows, 44100, 48000, None)
    _, b = be.resample(rows, 44100, 48000, BEST)
    assert same_bits(a, b)
    check_rows(a, n_out, rows, 44100, 48000, lib_table(be.lib, 44100, 48000, BEST))


def case_equal_rates_copy(be):
    rng = np.random.default_rng(5)
    rows = [rng.standard_normal(k) for k in (1, 255, 256, 257, 1000)]
    rows[3][5], rows[3][9], rows[3][11] = float("nan"), float("inf"), -0.0
    n_out, got = be.resample(rows, 22050, 22050, FAST)
    assert n_out == [len(r) for r in rows]
    for u, r in enumerate(rows):
        assert same_bits(got[u, :len(r)], r) and np.all(got[u, len(r):] == SENTINEL)


def case_independence(be):
    """a row's output is the same bits alone, in a batch, in a permuted batch, and with the cached table after calls at
    two other ratios"""
    fs_in, fs_out, design = 44100, 48000, BEST
    rows = rows_for(fs_in, fs_out, design)
    n_out, batch = be.resample(rows, fs_in, fs_out, design)
    for u in (0, 3, 5, len(rows) - 1):
        n1, alone = be.resample([rows[u]], fs_in, fs_out, design, x_pad=0, y_pad=0)
        assert n1 == [n_out[u]] and same_bits(alone[0, :n1[0]], batch[u, :n_out[u]])
    perm = np.random.default_rng(9).permutation(len(rows))
    n_p, permuted = be.resample([rows[u] for u in perm], fs_in, fs_out, design, x_pad=11, y_pad=1)
    for at, u in enumerate(perm):
        assert n_p[at] == n_out[u] and same_bits(permuted[at, :n_p[at]], batch[u, :n_out[u]])
    be.resample(rows[:3], 48000, 16000, FAST)
    be.resample(rows[:3], 8000, 16000, CUSTOM)
    _, again = be.resample(rows, fs_in, fs_out, design)
    assert same_bits(again, batch)


def case_table_cache_turns_over(be):
    """more ratios than the context keeps tables for, then the first again: the same bits"""
    rows = rows_for(48000, 16000, FAST)[2:5]
    _, first = be.resample(rows, 48000, 16000, FAST)
    for k, (fs_in, fs_out) in enumerate(((8000, 16000), (44100, 48000), (48000, 44100), (44100, 16000), (32000, 48000))):
        be.resample(rows[:1], fs_in, fs_out, (3 + k, 0.8, 4.0))
    _, again = be.resample(rows, 48000, 16000, FAST)
    assert same_bits(first, again)
    check_rows(again, [out_length(len(r), 48000, 16000) for r in rows], rows, 48000, 16000, lib_table(be.lib, 48000, 16000, FAST))


def case_hostile(be, fs_in, fs_out, design):
    """one NaN and one +Inf in a row: the non-finite outputs are exactly the statement's, every other output bit-equal,
    the neighbours unaffected, and the next call the same bits as in a fresh context"""
    rng = np.random.default_rng(21)
    L, M, W = shape(fs_in, fs_out, design)
    n = 6 * W + 700
    clean = [rng.standard_normal(k) for k in (n - 3, n, n + 5)]
    bad = [r.copy() for r in clean]
    bad[1][2 * W + 50] = float("nan")
    bad[1][n - W - 20] = float("inf")
    c = lib_table(be.lib, fs_in, fs_out, design)
    n_out, got = be.resample(bad, fs_in, fs_out, design)
    want = resample(bad[1], fs_in, fs_out, c)
    assert np.array_equal(np.isfinite(got[1, :n_out[1]]), np.isfinite(want))
    assert 0 < int(np.sum(~np.isfinite(want))) < len(want) // 2                 # it spreads 2 W taps wide and no further
    check_rows(got, n_out, bad, fs_in, fs_out, c)
    _, got_clean = be.resample(clean, fs_in, fs_out, design)
    assert same_bits(got[0], got_clean[0]) and same_bits(got[2], got_clean[2])
    with be.fresh() as other:
        _, fresh = other.resample(clean, fs_in, fs_out, design)
    assert same_bits(fresh, got_clean)
    assert np.all(np.isfinite(got_clean[:, :min(n_out)]))


def sine_rows(fs_in, fs_out, design, fracs):
    """unit sines at fracs x the lower Nyquist rate, long enough to leave 500 output samples between the margins"""
    L, M, W = shape(fs_in, fs_out, design)
    n_in = -((-(4 * W + 500) * M) // L)
    k = np.arange(n_in, dtype=np.float64)
    return [np.sin(2.0 * np.pi * (f * min(fs_in, fs_out) / 2.0) * k / fs_in) for f in fracs], 2 * W


def case_filter(be, fs_in, fs_out, design):
    """through the library: a unit sine in the pass band comes out as the analytic sine on the output grid, one above the
    output's Nyquist rate (downward pairs) comes out below the same bar; 2 W output samples at both ends are left out"""
    bar = BARS[design]
    fracs = [0.1, 0.5, 0.8] if design == BEST else [0.1, 0.5]
    rows, margin = sine_rows(fs_in, fs_out, design, fracs)
    n_out, got = be.resample(rows, fs_in, fs_out, design)
    m = np.arange(n_out[0], dtype=np.float64)
    assert n_out[0] - 2 * margin >= 500
    for u, f in enumerate(fracs):
        want = np.sin(2.0 * np.pi * (f * min(fs_in, fs_out) / 2.0) * m / fs_out)
        err = float(np.max(np.abs(got[u, :n_out[u]] - want)[margin:-margin]))
        print(f"filter {fs_in} -> {fs_out} {design[0]} zeros: sine at {f} x Nyquist, max error {err:.3g} (bar {bar:g})")
        assert err <= bar
    if fs_out < fs_in:
        k = np.arange(len(rows[0]), dtype=np.float64)
        alias = np.sin(2.0 * np.pi * (1.15 * fs_out / 2.0) * k / fs_in)
        n_a, out = be.resample([alias], fs_in, fs_out, design)
        level = float(np.max(np.abs(out[0, :n_a[0]])[margin:-margin]))
        print(f"filter {fs_in} -> {fs_out} {design[0]} zeros: alias of 1.15 x the output Nyquist rate {level:.3g} (bar {bar:g})")
        assert level <= bar


# ---- the tests -----------------------------------------------------------------------------------------------------------
def test_lengths_and_shapes(lib):
    case_lengths_and_shapes(lib)


def test_host_arithmetic_refusals_write_nothing(lib):
    case_host_refusals(lib)


def test_batch_refusals_write_nothing(be):
    case_batch_refusals(be)


@pytest.mark.parametrize("fs_in,fs_out,design", DESIGNS, ids=DESIGN_IDS)
def test_table_against_the_statement(lib, fs_in, fs_out, design):
    case_table(lib, fs_in, fs_out, design)


@pytest.mark.parametrize("fs_in,fs_out,design", DESIGNS + [STEEP], ids=DESIGN_IDS + ["48000-1000-steep"])
def test_sum_bit_for_bit(be, fs_in, fs_out, design):
    case_sum(be, fs_in, fs_out, design)


def test_null_option_is_best(be):
    case_null_option_is_best(be)


def test_equal_rates_copy_bit_for_bit(be):
    case_equal_rates_copy(be)


def test_a_row_alone_in_a_batch_permuted_and_behind_other_ratios(be):
    case_independence(be)


def test_table_cache_turns_over(be):
    case_table_cache_turns_over(be)


@pytest.mark.parametrize("fs_in,fs_out,design", [(44100, 48000, BEST), (192000, 16000, FAST)], ids=["44100-48000-best", "192000-16000-fast"])
def test_nan_and_inf_spread_as_the_sum_spreads_them(be, fs_in, fs_out, design):
    case_hostile(be, fs_in, fs_out, design)


@pytest.mark.parametrize("fs_in,fs_out,design", DESIGNS[:11], ids=DESIGN_IDS[:11])
def test_the_filter_does_its_job(be, fs_in, fs_out, design):
    case_filter(be, fs_in, fs_out, design)
