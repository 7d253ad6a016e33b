"""Shared helpers for the parity tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star tolerance: F0, spectral envelope and aperiodicity within 1e-4 relative;
# frame counts and temporal positions bit-exact.
RTOL = 1e-4


def load_golden(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    g["x"] = g["q"].astype(np.float64) / 32768.0
    for k in ("fs", "fft_size"):
        g[k] = int(g[k])
    for k in ("f0_floor_est", "frame_period", "q1", "threshold"):
        g[k] = float(g[k])
    g["f0_method"] = str(g["f0_method"])
    return g


def max_rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def assert_f0_close(f0, ref, rtol=RTOL, what="f0"):
    f0 = np.asarray(f0); ref = np.asarray(ref)
    assert f0.shape == ref.shape, what
    flips = int(np.sum((f0 > 0) != (ref > 0)))
    assert flips == 0, f"{what}: {flips} voiced/unvoiced flips"
    v = ref > 0
    assert max_rel(f0[v], ref[v]) <= rtol, f"{what}: rel err {max_rel(f0[v], ref[v])}"
    assert np.all(f0[~v] == 0.0)


def analyse(backend, g):
    """Run the golden fixture's pipeline on any backend exposing the loader API."""
    x, fs = g["x"], g["fs"]
    if g["f0_method"] == "harvest":
        tp, f0 = backend.harvest(x, fs, f0_floor=g["f0_floor_est"], frame_period=g["frame_period"])
        f0_est = None
    else:
        tp, f0_est = backend.dio(x, fs, f0_floor=g["f0_floor_est"], frame_period=g["frame_period"])
        f0 = backend.stonemask(x, fs, tp, f0_est)
    sp = backend.cheaptrick(x, fs, tp, f0, q1=g["q1"], f0_floor=71.0, fft_size=g["fft_size"])
    ap = backend.d4c(x, fs, tp, f0, g["fft_size"], threshold=g["threshold"])
    return tp, f0_est, f0, sp, ap


def check_against_golden(backend, g, rtol=RTOL, given_f0=False):
    """Full-pipeline check.  With given_f0 the spectral stages are fed the golden
    F0 (isolates CheapTrick/D4C from F0 differences)."""
    x, fs = g["x"], g["fs"]
    if given_f0:
        tp, f0 = g["tp"], g["f0"]
        sp = backend.cheaptrick(x, fs, tp, f0, q1=g["q1"], f0_floor=71.0, fft_size=g["fft_size"])
        ap = backend.d4c(x, fs, tp, f0, g["fft_size"], threshold=g["threshold"])
    else:
        tp, f0_est, f0, sp, ap = analyse(backend, g)
        assert np.array_equal(tp, g["tp"]), "temporal_positions must be bit-exact"
        if f0_est is not None:
            assert_f0_close(f0_est, g["f0_dio"], rtol, "dio f0")
        assert_f0_close(f0, g["f0"], rtol)
    rows = g["rows"]
    assert sp.shape == (len(g["f0"]), g["fft_size"] // 2 + 1)
    assert max_rel(sp[rows], g["sp_rows"]) <= rtol, f"spectrogram rel err {max_rel(sp[rows], g['sp_rows'])}"
    assert max_rel(ap[rows], g["ap_rows"]) <= rtol, f"aperiodicity rel err {max_rel(ap[rows], g['ap_rows'])}"
    assert max_rel(np.log(sp).sum(axis=1), g["sp_row_sums"]) <= rtol
    assert max_rel(ap.sum(axis=1), g["ap_row_sums"]) <= rtol


def synth_params(fs, nf, fft_size, seed=0):
    """Deterministic analysis-like parameters for the synthesis tests: an f0 contour with unvoiced
    gaps, a formant-shaped envelope, a rising aperiodicity (plain numpy arithmetic only)."""
    nb = fft_size // 2 + 1
    i = np.arange(nf, dtype=np.float64)
    f0 = 130.0 + 45.0 * np.sin(2 * np.pi * i / 83.0 + seed) + 8.0 * np.sin(2 * np.pi * i / 11.0)
    f0[(i % 67) < 12] = 0.0                                   # unvoiced stretches
    f0[-5:] = 0.0
    k = np.arange(nb, dtype=np.float64) * fs / fft_size
    env = np.zeros((nf, nb))
    for c, bw, a in ((700.0, 130.0, 1.0), (1220.0, 170.0, 0.5), (2600.0, 240.0, 0.25), (3500.0, 300.0, 0.1)):
        centre = c * (1.0 + 0.1 * np.sin(2 * np.pi * i / 140.0 + seed))[:, None]
        env += a / (1.0 + ((k[None, :] - centre) / bw) ** 2)
    sp = 1e-3 * env ** 2 + 1e-9
    ap = np.clip(0.02 + 0.9 * (k[None, :] / (fs / 2.0)) ** 1.5 * (1.0 + 0.2 * np.sin(i / 9.0))[:, None], 0.0, 1.0)
    ap[f0 == 0.0] = 1.0 - 1e-12
    return f0, sp, ap


# The host-arithmetic helpers of the reference's C API (frame counts, FFT sizes, floors, band counts, option defaults) for
# test_abi's sweep; tests/golden/make_golden.py stores the unmodified reference's answers in helpers.npz.
HELPER_ANSWERS = ("harvest_samples", "dio_samples", "init_q1", "init_f0_floor", "init_fft_size", "fft_size",
                  "f0_floor_for_fft_size", "aperiodicities")
OPTION_INITIALISERS = ("InitializeDioOption", "InitializeHarvestOption", "InitializeD4COption")


def bind_option_helpers(L):
    import ctypes
    from world_amd.api import CheapTrickOption
    L.GetSamplesForHarvest.argtypes = L.GetSamplesForDIO.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double]
    L.GetFFTSizeForCheapTrick.argtypes = [ctypes.c_int, ctypes.POINTER(CheapTrickOption)]
    L.GetF0FloorForCheapTrick.argtypes = [ctypes.c_int, ctypes.c_int]
    L.GetF0FloorForCheapTrick.restype = ctypes.c_double
    L.InitializeCheapTrickOption.argtypes = [ctypes.c_int, ctypes.POINTER(CheapTrickOption)]
    L.GetNumberOfAperiodicities.argtypes = [ctypes.c_int]
    return L


def option_helper_answers(L, fs, n, frame_period, f0_floor):
    """One case of the sweep on a library bound by bind_option_helpers: the values of HELPER_ANSWERS, in order."""
    import ctypes
    from world_amd.api import CheapTrickOption
    o = CheapTrickOption()
    L.InitializeCheapTrickOption(fs, ctypes.byref(o))
    init = (o.q1, o.f0_floor, o.fft_size)
    o.f0_floor = f0_floor
    size = L.GetFFTSizeForCheapTrick(fs, ctypes.byref(o))
    return (L.GetSamplesForHarvest(fs, n, frame_period), L.GetSamplesForDIO(fs, n, frame_period), *init, size,
            L.GetF0FloorForCheapTrick(fs, size), L.GetNumberOfAperiodicities(fs))


def option_defaults(L):
    """The bytes Initialize{Dio,Harvest,D4C}Option write, per initialiser."""
    import ctypes
    from world_amd.api import D4COption, DioOption, HarvestOption
    out = {}
    for cls, init in zip((DioOption, HarvestOption, D4COption), OPTION_INITIALISERS):
        a = cls()
        getattr(L, init)(ctypes.byref(a))
        out[init] = np.frombuffer(bytes(a), dtype=np.uint8)
    return out


# ---- accuracy against a more precise answer (tests/test_gpu_accuracy.py, tests/test_accuracy_cpu.py) ----------------------
# W = oracle/libworld_oracle_wide.so (long double value arithmetic, same discrete path), R = the unmodified reference,
# H = the code under test.  Per array, with e_X = |X - W| / |W| element-wise (Synthesis: / max|W|), for each quantile q:
#     quantile_q(e_H) <= ACC_A * quantile_q(e_R) + ACC_C * 2^-52
# The median catches a uniform loss of digits, the maximum a single bad bin or row.  A and c: DESIGN.md section 6.
ACC_A = 4.0
ACC_C = 64.0
ACC_QUANTILES = (0.5, 0.99, 1.0)
ULP = 2.0 ** -52


def rel_errors(a, w, peak=False):
    a = np.asarray(a, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    scale = np.max(np.abs(w)) if peak else np.abs(w)
    return np.abs(a - w) / np.maximum(scale, 1e-300)


def discrete_agreement(what, h, r, w, max_w_only=None):
    """Per-row discrete outcomes (V/UV, LoveTrain exit, StoneMask fallback ...): H and R must agree on every row; rows where
    W alone decides differently are returned (to be excluded from the value comparison), and there may be only a few."""
    h, r, w = (np.asarray(v) for v in (h, r, w))
    assert h.shape == r.shape == w.shape, what
    bad = np.flatnonzero(h != r)
    assert bad.size == 0, f"{what}: H and R decide differently on rows {bad[:10].tolist()} (of {bad.size})"
    w_only = np.flatnonzero(w != r)
    limit = max(2, len(r) // 50) if max_w_only is None else max_w_only
    assert w_only.size <= limit, f"{what}: the wide oracle alone decides differently on {w_only.size} rows (limit {limit})"
    return w_only


def accuracy_stats(h, r, w, peak=False, rows=None):
    """(e_H quantiles, e_R quantiles, worst index of e_H) over the selected rows (all rows when None)"""
    h, r, w = (np.asarray(v, dtype=np.float64) for v in (h, r, w))
    if rows is not None:
        h, r, w = h[rows], r[rows], w[rows]
    eh, er = rel_errors(h, w, peak), rel_errors(r, w, peak)
    worst = np.unravel_index(int(np.argmax(eh)), eh.shape) if eh.size else ()
    return np.quantile(eh, ACC_QUANTILES), np.quantile(er, ACC_QUANTILES), worst, eh, er


def assert_accurate(what, h, r, w, peak=False, exclude_rows=(), A=ACC_A, c=ACC_C, log=True):
    """The accuracy criterion above, on every row (but `exclude_rows`) and every bin.  Prints the worst element on failure."""
    h, r, w = (np.asarray(v, dtype=np.float64) for v in (h, r, w))
    assert h.shape == r.shape == w.shape, f"{what}: shapes {h.shape} {r.shape} {w.shape}"
    keep = np.ones(h.shape[0], dtype=bool)
    keep[list(exclude_rows)] = False
    index = np.flatnonzero(keep)
    assert index.size, f"{what}: nothing left to compare"
    qh, qr, worst, eh, er = accuracy_stats(h, r, w, peak, index)
    if log:
        _log_accuracy(what, qh, qr, len(exclude_rows), h.size)
    bound = A * qr + c * ULP
    failed = [q for q, a, b in zip(ACC_QUANTILES, qh, bound) if not a <= b]
    if failed:
        row = (int(index[worst[0]]),) + tuple(int(i) for i in worst[1:])
        msg = (f"{what}: e_H quantiles {qh.tolist()} exceed {A} * e_R {qr.tolist()} + {c} ulp at q = {failed}; "
               f"worst element {row}: e_H {eh[worst]:.3e}, e_R {er[worst]:.3e} (H {h[row]!r}, R {r[row]!r}, W {w[row]!r})")
        print(msg)
        raise AssertionError(msg)
    return qh, qr


def _log_accuracy(what, qh, qr, excluded, n):
    """WORLD_ACCURACY_LOG=<file>: one JSON line per checked array (the source of DESIGN.md section 6's table)"""
    path = os.environ.get("WORLD_ACCURACY_LOG")
    if path:
        import json
        with open(path, "a") as f:
            f.write(json.dumps({"what": what, "e_H": [float(v) for v in qh], "e_R": [float(v) for v in qr],
                                "excluded_rows": int(excluded), "elements": int(n)}) + "\n")


def assert_f0_tight(what, h, r, rtol=1e-10):
    """Harvest / DIO against the reference: identical V/UV, F0 within rtol relative on voiced frames."""
    h, r = np.asarray(h, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert h.shape == r.shape, what
    flips = np.flatnonzero((h > 0) != (r > 0))
    assert flips.size == 0, f"{what}: voiced/unvoiced differ at frames {flips[:10].tolist()}"
    v = r > 0
    assert v.any(), f"{what}: no voiced frame to compare"
    e = np.abs(h[v] - r[v]) / r[v]
    _log_accuracy(what, np.quantile(e, ACC_QUANTILES), np.zeros(3), 0, int(v.sum()))
    i = int(np.argmax(e))
    assert e[i] <= rtol, f"{what}: F0 rel err {e[i]:.3e} at frame {int(np.flatnonzero(v)[i])} (H {h[v][i]!r}, R {r[v][i]!r})"


# ---- fft_size off the rate's default (tests/test_gpu_offdefault_fft.py, tests/test_accuracy_cpu.py): signals, F0 tracks ----
def utterance(fs, seconds, index=2):
    from world_amd import synth
    return synth.utterance(index, fs, seconds).numpy()


def offdefault_seconds(fs):
    return 0.2 if fs < 100000 else 0.12


def ct_floor(fs, fft):
    return 3.0 * fs / (fft - 3.0)


def offdefault_track(kind, fs, fft, nf, seed):
    """caller-made F0 tracks as in tests/test_gpu_accuracy.py, and `floor_edge`: frames alternating between just below the
    floor 3 fs / (fft - 3) (analysed at the 500 Hz default), just above it (the longest window fft_size admits) and 1 %
    above, so that the default-F0 switch falls between adjacent frames"""
    rng = np.random.default_rng(seed)
    if kind == "floor_edge":
        floor = ct_floor(fs, fft)
        return np.resize([floor * (1 - 1e-12), floor * (1 + 1e-12), floor * 1.01], nf).astype(np.float64)
    if kind == "steps":
        f0 = np.repeat(rng.uniform(60.0, 600.0, nf // 7 + 1), 7)[:nf]
    elif kind == "low":
        f0 = rng.uniform(20.0, 90.0, nf)
    else:                                                              # "nyquist"
        f0 = rng.uniform(0.3 * fs, 0.4999 * fs, nf)
    f0[rng.random(nf) < 0.15] = 0.0
    return f0


def offdefault_f0(kind, ref, x, fs, fft):
    tp, f0 = ref.harvest(x, fs)
    return tp, (f0 if kind == "harvest" else offdefault_track(kind, fs, fft, len(tp), fs + fft + len(kind)))


def lowest_f0(fs, fft):
    return fs // fft + 1.0                                             # integer division (synthesis.cpp:361)


def synth_track(fs, fft, nf):
    """Frames on both sides of lowest_f0.  Below it (0.9 L) a frame is unvoiced by Synthesis' own rule.  `mid` lies between
    the integer-division L and fs / fft + 1 computed in floating point (voiced only under the reference's rule), on frames
    whose neighbours are voiced, so that every pulse spacing stays below fft_size: at a voiced / unvoiced boundary the
    reference interpolates F0 towards 0 and keeps the samples above half the voiced value, hence boundary frames at >= 2.5 L.
    High boundary and shoulder values also give voiced pulses within a short signal when L is a few Hz."""
    L, Lf = lowest_f0(fs, fft), fs / fft + 1.0
    mid = (L + Lf) / 2.0 if Lf > L else L * 1.003
    assert L <= mid and fs / mid < fft
    B, M = max(2.5 * L, 140.0), max(1.6 * L, 100.0)
    f0 = np.resize([0.9 * L, 0.9 * L, B, M, mid, mid, M, B, 0.0, 0.0], nf).astype(np.float64)
    f0[-3:] = 0.0
    return f0


def pulse_kinds(f0, fs, fft, n, frame_period=0.005):
    """(voiced pulses, default-F0 pulses) of the reference's time base (synthesis.cpp:224-321), in plain numpy"""
    L = lowest_f0(fs, fft)
    cf0 = np.where(f0 < L, 0.0, f0)
    cf0 = np.append(cf0, 2 * cf0[-1] - cf0[-2])
    vuv = (cf0 != 0).astype(np.float64)
    vuv[-1] = 2 * vuv[-2] - vuv[-3]
    t, ct = np.arange(n) / fs, np.arange(len(cf0)) * frame_period
    iv = np.interp(t, ct, vuv) > 0.5
    if0 = np.where(iv, np.interp(t, ct, cf0), 500.0)
    wrap = np.fmod(np.cumsum(2 * np.pi * if0 / fs), 2 * np.pi)
    at = np.flatnonzero(np.abs(np.diff(wrap)) > np.pi)
    gaps = np.diff(at)
    assert gaps.size and gaps.max() <= fft, "the case leaves the reference's noise buffer"
    return int(iv[at].sum()), int((~iv[at]).sum())


def synth_inputs(ref, fs, fft, seconds, index=2):
    x = utterance(fs, seconds, index)
    tp, _ = ref.harvest(x, fs)
    f0 = synth_track(fs, fft, len(tp))
    voiced, default = pulse_kinds(f0, fs, fft, len(x))
    assert voiced > 0 and default > 0, (voiced, default)
    sp = ref.cheaptrick(x, fs, tp, f0, fft_size=fft)
    ap = ref.d4c(x, fs, tp, f0, fft)
    return x, f0, sp, ap
