"""Every composition of csrc/fft.h's entry points that a stage kernel instantiates, in isolation (world_hip_probe_fft,
csrc/fft_probe_routes.inc: the same templates with the same template arguments), against the long-double oracle.

W = WideOracle.rfft / irfft_unscaled / cfft (long-double arithmetic, rounded once), R = the same calls of PortOracle (the
double build pinned to the reference), H = the probe.  The criterion is DESIGN.md section 6.1's, unchanged:
    quantile_q(e_H) <= 4 quantile_q(e_R) + 64 * 2^-52,  q in {0.5, 0.99, 1},
with e_X = |X - W| / |W| complex-wise on the impulse rows (every bin has modulus 1: a per-bin bound on one twiddle path) and
|X - W| / max_row |W| on random and real-output rows.  It is applied to the impulse rows and to the other rows of a case
separately (the maximum of either is then held to that array's own e_R, never to the looser of the two), per (mode, lg,
swizzle, max_lr, workgroup size); no row and no bin is left out.

CPU tests of this module: W itself against the closed form of a shifted impulse's spectrum, and the scan that holds the
table to the call sites of world_amd/csrc.
"""
import glob
import os
import re

import numpy as np
import pytest

from util import ACC_A, ACC_C, ACC_QUANTILES, ULP, _log_accuracy

gpu = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "world_amd", "csrc")
ANY = (64, 128, 256, 512, 1024)              # workgroup sizes of the modes that take theirs from the launch
N16 = "N/16"                                 # one radix-16's worth of points per thread: d4c_frame's shapes

# ---- the table: what the product's __global__ functions reach of fft.h ------------------------------------------------------
# mode: world_hip_probe_fft's (include/world_hip.h); entry: the fft.h entry points the composition calls; args: their template
# arguments; lgs: log2 of the transform lengths the callers can ask for; threads: ANY (a run-time value), a number or N16;
# twiddles: what the caller stages; swz: the slot maps it is compiled with (0 shipped, 1 d4c.hip); kind: the layouts --
# r2c / c2r / c2c, "c2c_half" a complex row zero beyond N/2, "r2c_twice" emits 2 X, "twiddles", "dft8".
# callers = () marks a composition no stage kernel runs: it is there for an equality fft.h promises.
# (No stage kernel passes an epilogue functor to block_cfft_dit_static, so none is probed.)
ROUTES = (
    dict(mode=1, entry=("block_rfft", "stage_twiddles"), args="<MAXLR>", max_lr=(3, 4), lgs=range(6, 15), threads=ANY, swz=(0,),
         twiddles="quarter-wave table of the N/2-point transform; the merge takes the fine twiddle", kind="r2c",
         callers=("cheaptrick.hip: ct_frame<.., 0, ..> (block_rfft<3>, 128 .. 8192 points)", "harvest.hip: hv_band_spectra, hv_block_spectra "
                  "(block_rfft<3>, 4096 points; the latter in the host emulation only)", "test hook: fft_probe max_lr 4")),
    dict(mode=1, entry=("block_rfft", "stage_twiddles"), args="<3>", max_lr=(3,), lgs=range(6, 15), threads=ANY, swz=(1,),
         twiddles="as above", kind="r2c", callers=("d4c.hip: d4c_lovetrain<0> (lg_love other than 11 and 12; 128 / 256 threads)",)),
    dict(mode=2, entry=("block_irfft", "stage_twiddles"), args="<MAXLR>", max_lr=(3, 4), lgs=range(6, 15), threads=ANY, swz=(0,),
         twiddles="quarter-wave table of the N/2-point transform", kind="c2r",
         callers=("cheaptrick.hip: ct_frame<.., 0, ..>", "synthesis.hip: pulse_response (sy_pulse, rt_pulse)",
                  "harvest.hip: hv_band_events_fft (host emulation only)", "test hook: fft_probe max_lr 4")),
    dict(mode=3, entry=("block_rfft_from", "stage_twiddles"), args="<3>", max_lr=(3,), lgs=range(6, 15), threads=ANY, swz=(0,),
         twiddles="quarter-wave table of the N/2-point transform", kind="r2c",
         callers=("synthesis.hip: minimum_phase, pulse_response's noise spectrum", "cheaptrick.hip: ct_frame<.., 0, ..> (the lifter's input)")),
    dict(mode=4, entry=("block_rfft", "stage_twiddles"), args="<4>", max_lr=(4,), lgs=range(6, 14), threads=ANY, swz=(0,),
         twiddles="quarter-wave table at N itself (the coders' table)", kind="r2c",
         callers=("codec.hip: codec_code_sp (64 .. 8192 points)", "cheaptrick.hip: ct_frame<.., true> (ct_frame_coded)")),
    dict(mode=5, entry=("block_cfft_dif", "stage_twiddles"), args="<4>, make_plan", max_lr=(4,), lgs=range(6, 14), threads=ANY, swz=(0,),
         twiddles="quarter-wave table at N", kind="c2c",
         callers=("codec.hip: decode_sp_row (codec_decode_sp, sy_stage_records, rt_store_coded_rows)",)),
    dict(mode=6, entry=("block_cfft_dif_from", "stage_twiddles"), args="<3>, make_plan_max(lg, 3)", max_lr=(3,), lgs=range(6, 14), threads=ANY,
         swz=(0,), twiddles="quarter-wave table one level coarser than the transform: the first stage takes the fine twiddle",
         kind="c2c_half", callers=("synthesis.hip: minimum_phase",)),
    dict(mode=7, entry=("block_rfft", "stage_twiddles"), args="<3, LGN>", max_lr=(3,), lgs=(10, 11, 12), threads=ANY, swz=(0,),
         twiddles="as mode 1", kind="r2c", static_of=1, callers=("cheaptrick.hip: ct_frame<.., 10 | 11 | 12, ..> (128, 256, 256 threads)",)),
    dict(mode=7, entry=("block_rfft", "stage_twiddles"), args="<3, 11>", max_lr=(3,), lgs=(11,), threads=ANY, swz=(1,),
         twiddles="as mode 1", kind="r2c", static_of=1, callers=("d4c.hip: d4c_lovetrain<11> (128 threads)",)),
    dict(mode=8, entry=("block_irfft", "stage_twiddles"), args="<3, LGN>", max_lr=(3,), lgs=(10, 11, 12), threads=ANY, swz=(0,),
         twiddles="as mode 2", kind="c2r", static_of=2, callers=("cheaptrick.hip: ct_frame<.., 10 | 11 | 12, ..>",)),
    dict(mode=9, entry=("block_rfft_from", "stage_twiddles"), args="<3, LGN>", max_lr=(3,), lgs=(10, 11, 12), threads=ANY, swz=(0,),
         twiddles="as mode 3", kind="r2c", static_of=3, callers=("cheaptrick.hip: ct_frame<.., 10 | 11 | 12, ..>",)),
    dict(mode=10, entry=("block_cfft_dif_static", "rfft_merge_items", "stage_twiddles"), args="<11, 3, 256> + <5, 256>", max_lr=(3,), lgs=(12,),
         threads=(256,), swz=(0,), twiddles="as mode 1", kind="r2c", static_of=1, callers=("harvest.hip: hv_block_spectra",)),
    dict(mode=11, entry=("irfft_pretwiddle_items_w", "mul_w16_fwd", "block_cfft_dit_static", "stage_twiddles"), args="<5, 256> + <11, 3, 256>",
         max_lr=(3,), lgs=(12,), threads=(256,), swz=(0,), twiddles="conj(wbase W16^m), wbase = twiddle(tid) at N from the table of N/2",
         kind="c2r", callers=("harvest.hip: hv_band_events_fft",)),
    dict(mode=12, entry=("irfft_pretwiddle_items", "block_cfft_dit_static", "stage_twiddles"), args="<5, 256> + <11, 3, 256>", max_lr=(3,),
         lgs=(12,), threads=(256,), swz=(0,), twiddles="as mode 2", kind="c2r", static_of=2, callers=()),
    dict(mode=13, entry=("block_cfft_dif_static", "rfft_merge_items_w", "mul_w16_fwd", "stage_twiddles"), args="<11, 3, 256> + <5, 256, true>",
         max_lr=(3,), lgs=(12,), threads=(256,), swz=(1,), twiddles="wbase W16^m, wbase = twiddle(tid) at N from the table of N/2",
         kind="r2c_twice", callers=("d4c.hip: d4c_lovetrain<12>",)),
    dict(mode=14, entry=("block_cfft_dif_static", "rfft_merge_items_rot", "mul_w16_fwd", "stage_twiddles", "stage_direct_twiddles"),
         args="<lg-1, 3, N/16> + <K, N/16>", max_lr=(3,), lgs=(11, 12, 13, 14), threads=N16, swz=(1,),
         twiddles="quarter-wave table TWO levels coarser than the merge's (D4C_TW_LEVEL), direct tables of the two inner radix-8 stages, "
                  "merge twiddles wbase W16^m", kind="r2c", callers=("d4c.hip: d4c_frame<2048, 128> .. <16384, 1024>",)),
    dict(mode=15, entry=("block_cfft_dif_static", "rfft_merge_items_rot", "mul_w16_fwd", "stage_twiddles", "stage_direct_twiddles"),
         args="<lg-1, 3, N/16> + <K, N/16, true>", max_lr=(3,), lgs=(11, 12, 13, 14), threads=N16, swz=(1,), twiddles="as mode 14",
         kind="r2c_twice", callers=("d4c.hip: d4c_frame (the band loop)",)),
    dict(mode=16, entry=("block_cfft_dif", "rfft_merge_items_rot", "stage_twiddles", "stage_direct_twiddles"), args="<3> + <K, N/16>", max_lr=(3,),
         lgs=(11, 12, 13, 14), threads=N16, swz=(1,), twiddles="as mode 14", kind="r2c", static_of=14, callers=()),
    dict(mode=17, entry=("stage_twiddles", "stage_direct_twiddles"), args="<N/16>", max_lr=(3,), lgs=(11, 12, 13, 14), threads=N16, swz=(1,),
         twiddles="the values themselves", kind="twiddles", callers=("d4c.hip: d4c_frame",)),
    dict(mode=18, entry=(), args="dft8<true>", max_lr=(3,), lgs=(3,), threads=(256,), swz=(0, 1), twiddles="none", kind="dft8",
         callers=("every radix-8 plan",)),
    dict(mode=19, entry=("dft8_head2",), args="<true>", max_lr=(3,), lgs=(3,), threads=(256,), swz=(0, 1), twiddles="none", kind="dft8",
         callers=("d4c.hip: d4c_frame (the band loop's pruned first stage)",)),
)
# fft.h entry points a stage kernel calls only through another entry point of this list (or not at all)
INNER_ONLY = ("block_cfft_dif_from_static", "block_cfft_dit", "rfft_merge", "irfft_pretwiddle")


def threads_of(route, lg):
    return ((1 << lg) // 16,) if route["threads"] == N16 else tuple(route["threads"])


# ---- CPU: the table against the call sites -------------------------------------------------------------------------------------
def fft_entry_points():
    """the block-level functions fft.h defines: transforms, merge / pre-twiddle steps, twiddle staging, the pruned butterfly"""
    with open(os.path.join(CSRC, "fft.h")) as f:
        text = f.read()
    return set(re.findall(r"__device__ __forceinline__ \w+ ((?:block_|rfft_merge|irfft_pretwiddle|stage_)\w*|dft8_head2|mul_w16_fwd)\s*\(", text))


def call_sites(entry_points):
    """(file, line, entry point) of every call in the stage kernels' sources (the probes and fft.h itself apart)"""
    pattern = re.compile(r"\b(" + "|".join(sorted(entry_points, key=len, reverse=True)) + r")\s*(?:<[^;]*?>)?\s*\(")
    sites = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc"))):
        name = os.path.basename(path)
        if name.startswith("fft_probe"):
            continue
        with open(path) as f:
            for no, line in enumerate(f, 1):
                code = line.split("//")[0]
                sites += [(name, no, m) for m in pattern.findall(code)]
    return sites


def rows_missing(sites, routes):
    have = {e for r in routes if r["callers"] for e in r["entry"]}
    return sorted({(f, e) for f, _, e in sites if e not in have})


def test_every_fft_call_site_has_a_row():
    eps = fft_entry_points()
    assert {"block_rfft", "block_irfft", "block_rfft_from", "block_cfft_dif", "block_cfft_dif_from", "block_cfft_dif_static",
            "block_cfft_dit_static", "rfft_merge_items", "rfft_merge_items_w", "rfft_merge_items_rot", "irfft_pretwiddle_items",
            "irfft_pretwiddle_items_w", "stage_twiddles", "stage_direct_twiddles", "dft8_head2", "mul_w16_fwd"} <= eps, eps
    sites = call_sites(eps)
    files = {f for f, _, _ in sites}
    assert len(sites) >= 30 and {"cheaptrick.hip", "codec.hip", "d4c.hip", "harvest.hip", "synthesis.hip"} <= files, "the scan lost the call sites"
    missing = rows_missing(sites, ROUTES)
    assert not missing, f"fft.h entry points called by a stage kernel with no row in ROUTES: {missing}"
    called = {e for _, _, e in sites}
    stale = sorted(e for r in ROUTES if r["callers"] for e in r["entry"] if e not in called)
    assert not stale, f"rows name entry points no stage kernel calls any more: {stale}"
    assert not [e for e in INNER_ONLY if e in called], "an entry point listed as inner-only has a call site of its own now"
    assert eps <= called | set(INNER_ONLY) | {"irfft_pretwiddle_items"}, sorted(eps - called)
    # the scan itself: a row taken out of the table is reported
    assert rows_missing(sites, [r for r in ROUTES if r["mode"] != 6]) == [("synthesis.hip", "block_cfft_dif_from")]
    for r in ROUTES:
        assert set(r["swz"]) <= {0, 1} and r["max_lr"] and len(r["lgs"]) and r["kind"] in KINDS, r["mode"]


# ---- inputs and references -----------------------------------------------------------------------------------------------------
def impulse_shifts(lg):
    n = 1 << lg
    m = {0, 1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 1}
    for j in range(lg):
        m |= {1 << j, (1 << j) + 1}
    return sorted(v for v in m if 0 <= v < n)


def single_bins(lg):
    """the impulse set of the half length, and the Nyquist bin: k in [0, N/2]"""
    return sorted(set(impulse_shifts(lg - 1)) | {1 << (lg - 1)})


N_RANDOM = 5                                 # four normal rows and one of 1e-12 amplitude


def _random_rows(rng, shape):
    x = rng.standard_normal((N_RANDOM,) + shape)
    x[-1] *= 1e-12
    return x


_cache = {}


def case(kind, lg, wide, port):
    """(input rows [batch, ...], W, R, number of leading impulse rows) of a layout at 2^lg points, computed once"""
    key = (kind, lg)
    if key in _cache:
        return _cache[key]
    n, h = 1 << lg, 1 << (lg - 1)
    rng = np.random.default_rng(1000 * lg + sorted(KINDS).index(kind))
    if kind == "r2c":
        shifts = impulse_shifts(lg)
        x = np.zeros((len(shifts), n))
        x[np.arange(len(shifts)), shifts] = 1.0
        x = np.concatenate([x, _random_rows(rng, (n,))])
        refs = [np.stack([o.rfft(row) for row in x]) for o in (wide, port)]
    elif kind == "c2r":
        rows = []
        for k in single_bins(lg):
            e = np.zeros(h + 1, dtype=np.complex128)
            e[k] = 1.0 + (0.75j if k in (0, h) else 0.0)             # the imaginary parts of DC and Nyquist must be ignored
            rows.append(e)
            if 0 < k < h:
                e = np.zeros(h + 1, dtype=np.complex128)
                e[k] = 1.0j
                rows.append(e)
        shifts = rows
        r = _random_rows(rng, (h + 1,)) + 1j * _random_rows(rng, (h + 1,))
        x = np.concatenate([np.stack(rows), r])
        refs = [np.stack([o.irfft_unscaled(row) for row in x]) for o in (wide, port)]
    elif kind in ("c2c", "c2c_half"):
        shifts = [m for m in impulse_shifts(lg) if kind == "c2c" or m <= h]
        x = np.zeros((len(shifts), n), dtype=np.complex128)
        x[np.arange(len(shifts)), shifts] = 1.0
        r = _random_rows(rng, (n,)) + 1j * _random_rows(rng, (n,))
        if kind == "c2c_half":
            r[:, h + 1:] = 0.0                                       # the caller's prefix: j <= N/2
        x = np.concatenate([x, r])
        refs = [np.stack([o.cfft(row) for row in x]) for o in (wide, port)]
    else:
        raise KeyError(kind)
    _cache[key] = (x, refs[0], refs[1], len(shifts))
    return _cache[key]


KINDS = ("r2c", "c2r", "c2c", "c2c_half", "r2c_twice", "twiddles", "dft8")


def errors(x, w, n_impulse, real_out):
    """e_X of the impulse rows (complex-wise; real output: by the row's peak) and of the other rows (by the row's peak)"""
    d = np.abs(x - w)
    peak = np.abs(w).max(axis=1, keepdims=True)
    first = d[:n_impulse] / (peak[:n_impulse] if real_out else np.abs(w[:n_impulse]))
    return first.ravel(), (d[n_impulse:] / peak[n_impulse:]).ravel()


def criterion(what, eh, er):
    """section 6.1's bound; prints and logs the quantiles (ulp) before it asserts"""
    qh, qr = np.quantile(eh, ACC_QUANTILES), np.quantile(er, ACC_QUANTILES)
    _log_accuracy(what, qh, qr, 0, eh.size)
    print(f"{what}: e_H {np.round(qh / ULP, 2).tolist()} ulp, e_R {np.round(qr / ULP, 2).tolist()} ulp at q = {list(ACC_QUANTILES)}")
    bound = ACC_A * qr + ACC_C * ULP
    failed = [q for q, a, b in zip(ACC_QUANTILES, qh, bound) if not a <= b]
    assert not failed, (f"{what}: e_H quantiles {qh.tolist()} exceed {ACC_A} * e_R {qr.tolist()} + {ACC_C} ulp at q = {failed}; "
                        f"worst element {int(np.argmax(eh))} of the flattened array: e_H {eh.max():.3e}")


def to_complex(a):
    return a[..., 0] + 1j * a[..., 1]


def to_pairs(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def check_route(probe, route, lg, swz, wide, port):
    """one (mode, lg, swizzle): every max_lr and workgroup size against W, and the scaling by 2^40 bit for bit.
    probe(mode, rows, max_lr, threads, swz) -> numpy array in the mode's output layout"""
    kind = route["kind"]
    layout = "r2c" if kind == "r2c_twice" else kind
    x, w, r, n_imp = case(layout, lg, wide, port)
    real_in, real_out = layout == "r2c", layout == "c2r"
    rows = x if real_in else to_pairs(x)
    for max_lr in route["max_lr"]:
        for threads in threads_of(route, lg):
            got = probe(route["mode"], rows, max_lr, threads, swz)
            big = probe(route["mode"], rows * 2.0 ** 40, max_lr, threads, swz)
            what = f"fft route mode {route['mode']} lg {lg} swz {swz} max_lr {max_lr} threads {threads}"
            assert np.array_equal(big, got * 2.0 ** 40), f"{what}: probe(2^40 x) != 2^40 probe(x)"
            h = got if real_out else to_complex(got)
            if kind == "r2c_twice":
                h = h * 0.5
            if layout == "r2c":                                      # r2c: the imaginary parts of DC and Nyquist are zero
                assert np.all(h[:, 0].imag == 0) and np.all(h[:, -1].imag == 0), what
            (eh_i, eh_r), (er_i, er_r) = errors(h, w, n_imp, real_out), errors(r, w, n_imp, real_out)
            criterion(what + " impulses", eh_i, er_i)
            criterion(what + " random", eh_r, er_r)


# ---- CPU: W itself ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles():
    from oracle.loader import PortOracle, WideOracle, build
    build()
    return WideOracle(), PortOracle()


LD_PI = np.longdouble("3.14159265358979323846264338327950288419716939937510")


def exact_twiddles(k, n):
    """e^{-2 pi i k / n} for integer arrays k, in long double with the argument reduced to [0, n)"""
    a = 2 * LD_PI * (np.asarray(k) % n).astype(np.longdouble) / np.longdouble(n)
    return np.cos(a), -np.sin(a)


@pytest.mark.parametrize("lg", range(6, 15))
def test_wide_oracle_matches_the_closed_form(oracles, lg):
    """x = delta[n - m]: X[k] = e^{-2 pi i (k m mod N) / N}; W equals it within 1 ulp (2^-52: the bins have modulus 1) at every bin"""
    from oracle.loader import wide_is_wider
    assert wide_is_wider() and np.finfo(np.longdouble).eps < 2.0 ** -60
    wide, _ = oracles
    n = 1 << lg
    k = np.arange(n // 2 + 1, dtype=np.int64)
    worst = 0.0
    for m in impulse_shifts(lg):
        x = np.zeros(n)
        x[m] = 1.0
        got = wide.rfft(x)
        c, s = exact_twiddles(k * m, n)
        err = np.hypot(got.real.astype(np.longdouble) - c, got.imag.astype(np.longdouble) - s)
        worst = max(worst, float(err.max()))
        assert err.max() <= ULP, (lg, m, int(np.argmax(err)), float(err.max()) / ULP)
        # and the inverse of that spectrum is N delta[n - m] (c2r, unscaled)
        back = wide.irfft_unscaled(got)
        assert np.abs(back - n * x).max() <= 2 * lg * ULP * n, (lg, m)
    z = np.zeros(n, dtype=np.complex128)
    z[3] = 1.0
    c, s = exact_twiddles(3 * np.arange(n, dtype=np.int64), n)
    got = wide.cfft(z)
    assert np.hypot(got.real.astype(np.longdouble) - c, got.imag.astype(np.longdouble) - s).max() <= ULP
    print(f"lg {lg}: W within {worst / ULP:.3f} ulp of the closed form")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wh():
    from world_amd.api import WorldHip
    return WorldHip()


@pytest.fixture(scope="module")
def probe(wh):
    import torch

    def run(mode, rows, max_lr, threads, swz):
        out = wh.probe_fft(mode, torch.from_numpy(np.ascontiguousarray(rows)).cuda(), max_lr=max_lr, threads=threads, swizzle=swz)
        return out.cpu().numpy()
    return run


TRANSFORMS = [(i, lg, swz) for i, r in enumerate(ROUTES) if r["kind"] not in ("twiddles", "dft8") for lg in r["lgs"] for swz in r["swz"]]


@gpu
@pytest.mark.parametrize("row,lg,swz", TRANSFORMS, ids=[f"mode{ROUTES[i]['mode']}-lg{lg}-swz{s}" for i, lg, s in TRANSFORMS])
def test_route_meets_the_criterion(probe, oracles, row, lg, swz):
    check_route(probe, ROUTES[row], lg, swz, *oracles)


def _same(probe, lg, swz, a, b, what, scale_a=1.0):
    """modes a and b on the same rows, bit for bit (a's output times scale_a)"""
    mode_a, lr_a, th_a = a
    mode_b, lr_b, th_b = b
    kind = next(r["kind"] for r in ROUTES if r["mode"] == mode_a)
    layout = "r2c" if kind == "r2c_twice" else kind
    x = case(layout, lg, None, None)[0] if (layout, lg) in _cache else None
    assert x is not None, "the criterion test of the mode builds the rows"
    rows = x if layout == "r2c" else to_pairs(x)
    ga, gb = probe(mode_a, rows, lr_a, th_a, swz) * scale_a, probe(mode_b, rows, lr_b, th_b, swz)
    bad = np.flatnonzero((ga != gb).reshape(len(ga), -1).any(axis=1))
    assert bad.size == 0, f"{what} at 2^{lg} points, swizzle {swz}: rows {bad[:8].tolist()} differ"


@gpu
def test_exact_relations(probe, oracles, wh):
    """what fft.h's comments promise bit for bit"""
    import torch
    wide, port = oracles
    # the older probe entries (fft_probe.hip's own kernels, world_hip_probe_rfft / _irfft) are modes 1, 2 and 7, 8
    for lg, static in ((6, False), (7, False), (11, False), (11, True), (14, False)):
        x = torch.from_numpy(case("r2c", lg, wide, port)[0]).cuda()
        spec = torch.from_numpy(to_pairs(case("c2r", lg, wide, port)[0])).cuda()
        for max_lr in ((3,) if static else (3, 4)):
            assert np.array_equal(wh.probe_rfft(x, max_lr=max_lr, threads=128, static_plan=static).cpu().numpy(),
                                  probe(7 if static else 1, x.cpu().numpy(), max_lr, 128, 0)), (lg, static, max_lr)
            assert np.array_equal(wh.probe_irfft(spec, max_lr=max_lr, threads=128, static_plan=static).cpu().numpy(),
                                  probe(8 if static else 2, spec.cpu().numpy(), max_lr, 128, 0)), (lg, static, max_lr)
    for lg in range(6, 15):
        case("r2c", lg, wide, port), case("c2r", lg, wide, port)
        for threads in (64, 256, 1024):
            _same(probe, lg, 0, (3, 3, threads), (1, 3, threads), "block_rfft_from != block_rfft")
    for lg in (10, 11, 12):                                  # static == run-time plan: every static size of the table
        for threads in (128, 256):
            _same(probe, lg, 0, (7, 3, threads), (1, 3, threads), "block_rfft<3, LGN> != block_rfft<3>")
            _same(probe, lg, 0, (8, 3, threads), (2, 3, threads), "block_irfft<3, LGN> != block_irfft<3>")
            _same(probe, lg, 0, (9, 3, threads), (3, 3, threads), "block_rfft_from<3, LGN> != block_rfft_from<3>")
    _same(probe, 11, 1, (7, 3, 128), (1, 3, 128), "block_rfft<3, 11> != block_rfft<3> under d4c.hip's swizzle")
    _same(probe, 12, 0, (10, 3, 256), (1, 3, 256), "static stages + rfft_merge_items != block_rfft<3>")
    _same(probe, 12, 0, (12, 3, 256), (2, 3, 256), "irfft_pretwiddle_items + static inverse != block_irfft<3>")
    for lg in (11, 12, 13, 14):
        t = (1 << lg) // 16
        _same(probe, lg, 1, (15, 3, t), (14, 3, t), "rfft_merge_items_rot<TWICE> / 2 != the plain merge", scale_a=0.5)
        _same(probe, lg, 1, (16, 3, t), (14, 3, t), "d4c_frame's route: run-time plan != static stages")


@gpu
@pytest.mark.parametrize("lg", [11, 12, 13, 14])
def test_d4c_twiddle_staging(probe, lg):
    """d4c_frame's twiddles: the direct tables equal twiddle()'s values bit for bit, and every level the kernel asks for --
    the two direct ones, the first stage's (one level finer than the table) and the merge's (two levels finer: the fine /
    fine2 products) -- meets the criterion against the exact value (R = the exact value rounded to double: e_R <= 1/2 ulp)"""
    n, t = 1 << lg, (1 << lg) // 16
    n_a, n_b = n >> 7, n >> 10
    got = to_complex(probe(17, np.zeros((3, n, 2)), 3, t, 1))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    g = got[0]
    assert np.array_equal(g[:n_a + n_b], g[n // 4:n // 4 + n_a + n_b]), "stage_direct_twiddles != twiddle()"
    used = np.zeros(n, dtype=bool)
    for what, at, count, level in (("direct a", 0, n_a, lg - 4), ("direct b", n_a, n_b, lg - 7), ("table a", n // 4, n_a, lg - 4),
                                   ("table b", n // 4 + n_a, n_b, lg - 7), ("fine", 3 * n // 8, n // 16, lg - 1), ("fine2", n // 2, n // 2, lg)):
        c, s = exact_twiddles(np.arange(count, dtype=np.int64), 1 << level)
        w = c.astype(np.float64) + 1j * s.astype(np.float64)
        eh = np.hypot(g[at:at + count].real.astype(np.longdouble) - c, g[at:at + count].imag.astype(np.longdouble) - s).astype(np.float64)
        er = np.hypot(w.real.astype(np.longdouble) - c, w.imag.astype(np.longdouble) - s).astype(np.float64)
        criterion(f"fft route mode 17 lg {lg} swz 1 {what}", eh, er)
        used[at:at + count] = True
    assert np.all(g[~used] == 0)


@gpu
@pytest.mark.parametrize("swz", [0, 1])
def test_dft8_head2_is_dft8_on_padded_input(probe, swz):
    rng = np.random.default_rng(8)
    z = np.zeros((64, 8), dtype=np.complex128)
    z[:, :2] = rng.standard_normal((64, 2)) + 1j * rng.standard_normal((64, 2))
    z[0, :2] = (1.0, 0.0); z[1, :2] = (0.0, 1.0); z[2, :2] = (1e-12j, -3.0); z[3, :2] = (1.0, 1.0); z[4, :2] = (1.0, -1.0)
    full = to_complex(probe(18, to_pairs(z), 3, 256, swz))
    junk = z.copy()
    junk[:, 2:] = 7.0                                                 # head2 reads the first two values only
    head = to_complex(probe(19, to_pairs(junk), 3, 256, swz))
    assert np.array_equal(head, full), "dft8_head2 != dft8 on (a0, a1, 0, ..): the sign of zeros aside"      # (-0.0 == 0.0)
    k = np.arange(8, dtype=np.int64)
    c, s = exact_twiddles(np.outer(k, k), 8)
    zl = z.astype(np.clongdouble)
    w = zl @ (c + 1j * s).astype(np.clongdouble)
    r = np.fft.fft(z, axis=1)
    peak = np.abs(w).max(axis=1, keepdims=True).astype(np.float64)
    criterion(f"fft route mode 19 lg 3 swz {swz}", (np.abs(head - w).astype(np.float64) / peak).ravel(),
              (np.abs(r - w).astype(np.float64) / peak).ravel())


@gpu
def test_whatever_is_not_in_the_table_is_refused(wh):
    import torch
    x = torch.zeros((2, 4096), dtype=torch.float64, device="cuda")
    for mode, max_lr, threads, swz in ((10, 3, 128, 0), (14, 3, 256, 0), (5, 4, 256, 1), (3, 4, 256, 0), (13, 3, 256, 0), (1, 3, 96, 0), (1, 3, 256, 2)):
        with pytest.raises(Exception, match="probe_fft"):
            wh.probe_fft(mode, x if mode != 5 else torch.zeros((2, 4096, 2), dtype=torch.float64, device="cuda"), max_lr=max_lr, threads=threads,
                         swizzle=swz)
    with pytest.raises(Exception, match="probe_fft"):
        wh.probe_fft(1, torch.zeros((2, 32), dtype=torch.float64, device="cuda"), max_lr=3, threads=64, swizzle=0)
