"""Python face of libworld_hip.so (ctypes; the library is the product, this file is
plumbing).

Two levels, mirroring include/world_hip.h:

* ``WorldHip``  -- the batched, device-resident API.  Inputs/outputs are torch
  CUDA(=HIP) tensors of dtype float64; work is enqueued on torch's current
  stream; nothing synchronises.
* module-level ``harvest / dio / stonemask / cheaptrick / d4c`` -- numpy in, numpy
  out, same argument meaning as the reference's C functions of the same names
  (they call the library's drop-in host-pointer entry points).

The extension must exist: importing this module on a machine where
``libworld_hip.so`` has not been built raises immediately (no fallback path).
"""
import ctypes as C
import os
import re
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# WORLD_HIP_LIB: another build of the library (tools/ab.py times variants built with other flags side by side)
LIB_PATH = os.environ.get("WORLD_HIP_LIB") or os.path.join(HERE, "libworld_hip.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class DioOption(C.Structure):        # include/world_hip.h (reference dio.h:16-23)
    _fields_ = [("f0_floor", C.c_double), ("f0_ceil", C.c_double), ("channels_in_octave", C.c_double),
                ("frame_period", C.c_double), ("speed", C.c_int), ("allowed_range", C.c_double)]


class HarvestOption(C.Structure):    # reference harvest.h:16-20
    _fields_ = [("f0_floor", C.c_double), ("f0_ceil", C.c_double), ("frame_period", C.c_double)]


class CheapTrickOption(C.Structure):  # reference cheaptrick.h:16-20
    _fields_ = [("q1", C.c_double), ("f0_floor", C.c_double), ("fft_size", C.c_int)]


class D4COption(C.Structure):        # reference d4c.h:16-18
    _fields_ = [("threshold", C.c_double)]


class WorldHipModification(C.Structure):   # include/world_hip.h (test.cpp's ParameterModification, per utterance)
    _fields_ = [("f0_scale", C.c_double), ("formant_shift", C.c_double), ("convert_log_f0", C.c_int),
                ("log_f0_mean", C.c_double), ("log_f0_std", C.c_double)]


def modifications(n_utt, f0_scale=1.0, formant_shift=1.0, log_f0_target=None):
    """WorldHipModification[n_utt] from scalars or per-utterance sequences; log_f0_target = (means, stds) or None"""
    scale = np.broadcast_to(np.asarray(f0_scale, dtype=np.float64), (n_utt,))
    ratio = np.broadcast_to(np.asarray(formant_shift, dtype=np.float64), (n_utt,))
    mods = (WorldHipModification * n_utt)()
    if log_f0_target is not None:
        mean = np.broadcast_to(np.asarray(log_f0_target[0], dtype=np.float64), (n_utt,))
        std = np.broadcast_to(np.asarray(log_f0_target[1], dtype=np.float64), (n_utt,))
    for u in range(n_utt):
        m = mods[u]
        m.f0_scale, m.formant_shift = float(scale[u]), float(ratio[u])
        if log_f0_target is not None:
            m.convert_log_f0, m.log_f0_mean, m.log_f0_std = 1, float(mean[u]), float(std[u])
    return mods


class WorldHipFrameCurves(C.Structure):    # include/world_hip.h: device arrays [n_utt][o_stride], or NULL
    _fields_ = [(name, C.c_void_p) for name in ("d_time_map", "d_f0_target", "d_f0_scale", "d_formant_shift", "d_ap_gain")]


class WorldHipMorph(C.Structure):          # include/world_hip.h: one pair's rates, each within [0, 1] (0 = A, 1 = B)
    _fields_ = [(name, C.c_double) for name in ("time_rate", "f0_rate", "sp_rate", "ap_rate")]


class WorldHipMorphCurves(C.Structure):    # include/world_hip.h: device arrays [n_pairs][o_stride], or NULL
    _fields_ = [(name, C.c_void_p) for name in ("d_f0_rate", "d_sp_rate", "d_ap_rate")]


class WorldHipResampleOption(C.Structure):  # include/world_hip.h: the resampler's filter design
    _fields_ = [("zeros", C.c_int), ("rolloff", C.c_double), ("kaiser_beta", C.c_double)]


RESAMPLE_QUALITIES = {"best": 0, "fast": 1}    # WORLD_HIP_RESAMPLE_BEST / _FAST


def morphs(n_pairs, time_rate=0.5, f0_rate=0.5, sp_rate=0.5, ap_rate=0.5):
    """WorldHipMorph[n_pairs] from scalars or per-pair sequences"""
    cols = [np.broadcast_to(np.asarray(v, dtype=np.float64), (n_pairs,)) for v in (time_rate, f0_rate, sp_rate, ap_rate)]
    out = (WorldHipMorph * n_pairs)()
    for u in range(n_pairs):
        out[u].time_rate, out[u].f0_rate, out[u].sp_rate, out[u].ap_rate = (float(c[u]) for c in cols)
    return out


def uniform_time_map(n_src, n_out, device="cuda"):
    """Time map [n_out] (float64, on `device`) that spreads n_src source frames evenly over n_out output frames: first
    onto first, last onto last."""
    import torch
    step = (n_src - 1) / (n_out - 1) if n_out > 1 else 0.0
    return (torch.arange(n_out, dtype=torch.float64, device=device) * step).clamp_(0.0, float(max(n_src - 1, 0)))


def hold_time_map(n_src, segments, device="cuda"):
    """Piecewise-linear time map through the anchors `segments` = [(src_frame, out_frame), ...] (out_frame strictly
    increasing from 0): [last out_frame + 1] source positions (float64, on `device`), clamped to [0, n_src - 1].  Two
    anchors with the same src_frame hold that frame; a steeper stretch plays its frames faster."""
    import torch
    src = np.asarray([a[0] for a in segments], dtype=np.float64)
    dst = np.asarray([a[1] for a in segments], dtype=np.float64)
    if len(segments) < 2 or dst[0] != 0 or np.any(np.diff(dst) <= 0) or np.any(dst != np.floor(dst)):
        raise ValueError("hold_time_map: at least two anchors, out_frame whole, starting at 0 and strictly increasing")
    xs, xd = torch.from_numpy(src).to(device), torch.from_numpy(dst).to(device)
    j = torch.arange(int(dst[-1]) + 1, dtype=torch.float64, device=device)
    k = torch.searchsorted(xd, j, right=True).clamp_(1, len(segments) - 1)
    w = (j - xd[k - 1]) / (xd[k] - xd[k - 1])
    return (xs[k - 1] + w * (xs[k] - xs[k - 1])).clamp_(0.0, float(max(n_src - 1, 0)))


# -- the real-time synthesiser (reference synthesisrealtime.h; include/world_hip.h declares the same layout) --
class RandnState(C.Structure):       # reference matlabfunctions.h
    _fields_ = [("g_randn_x", C.c_uint32), ("g_randn_y", C.c_uint32), ("g_randn_z", C.c_uint32), ("g_randn_w", C.c_uint32)]


class FftPlan(C.Structure):          # reference fft.h
    _fields_ = [("n", C.c_int), ("sign", C.c_int), ("flags", C.c_uint), ("c_in", C.c_void_p), ("in_", C.c_void_p),
                ("c_out", C.c_void_p), ("out", C.c_void_p), ("input", C.c_void_p), ("ip", C.c_void_p), ("w", C.c_void_p)]


class ForwardRealFFT(C.Structure):   # reference common.h
    _fields_ = [("fft_size", C.c_int), ("waveform", C.c_void_p), ("spectrum", C.c_void_p), ("forward_fft", FftPlan)]


class InverseRealFFT(C.Structure):   # reference common.h
    _fields_ = [("fft_size", C.c_int), ("waveform", C.c_void_p), ("spectrum", C.c_void_p), ("inverse_fft", FftPlan)]


class MinimumPhaseAnalysis(C.Structure):   # reference common.h
    _fields_ = [("fft_size", C.c_int), ("log_spectrum", C.c_void_p), ("minimum_phase_spectrum", C.c_void_p),
                ("cepstrum", C.c_void_p), ("inverse_fft", FftPlan), ("forward_fft", FftPlan)]


class WorldSynthesizer(C.Structure):  # reference synthesisrealtime.h
    _fields_ = [("fs", C.c_int), ("frame_period", C.c_double), ("buffer_size", C.c_int), ("number_of_pointers", C.c_int),
                ("fft_size", C.c_int), ("buffer", _dp), ("current_pointer", C.c_int), ("i", C.c_int),
                ("dc_remover", _dp), ("f0_length", _ip), ("f0_origin", _ip), ("spectrogram", C.c_void_p),
                ("aperiodicity", C.c_void_p), ("current_pointer2", C.c_int), ("head_pointer", C.c_int),
                ("synthesized_sample", C.c_int), ("handoff", C.c_int), ("handoff_phase", C.c_double),
                ("handoff_f0", C.c_double), ("last_location", C.c_int), ("cumulative_frame", C.c_int),
                ("current_frame", C.c_int), ("interpolated_vuv", C.c_void_p), ("pulse_locations", C.c_void_p),
                ("pulse_locations_index", C.POINTER(_ip)), ("number_of_pulses", _ip), ("impulse_response", _dp),
                ("randn_state", RandnState), ("minimum_phase", MinimumPhaseAnalysis),
                ("inverse_real_fft", InverseRealFFT), ("forward_real_fft", ForwardRealFFT)]


# the synthesiser's scalar control fields, in the order run_realtime_plan records them (after op, return value)
REALTIME_SCALARS = ("current_pointer", "i", "current_pointer2", "head_pointer", "synthesized_sample", "handoff",
                    "handoff_phase", "handoff_f0", "last_location", "cumulative_frame", "current_frame")
RT_ADD, RT_SYNTH, RT_LOCKED, RT_REFRESH = 0, 1, 2, 3


# -- the C boundary: prototypes are read from include/world_hip.h, the header api.hip is compiled against --
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "world_hip.h")
_SCALARS = {"void": None, "int": C.c_int, "double": C.c_double, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong, "unsigned int": C.c_uint}
# what a data pointer may point to, besides the header's own struct typedefs
_POINTEES = set(_SCALARS) | {"char", "unsigned char", "short"}
_parsed = None                                   # (ABI version, prototypes) of the installed header, read once per process


def _installed_header():
    global _parsed
    if _parsed is None:
        if not os.path.exists(HEADER_PATH):
            raise ImportError(f"{HEADER_PATH} is missing: the Python binding reads its prototypes from the header, "
                              "which travels with the package")
        with open(HEADER_PATH) as f:
            text = f.read()
        _parsed = (int(re.search(r"#[ \t]*define[ \t]+WORLD_HIP_ABI_VERSION[ \t]+(\d+)", text).group(1)), header_prototypes(text))
    return _parsed


def header_abi_version():
    """the header's WORLD_HIP_ABI_VERSION"""
    return _installed_header()[0]


def header_prototypes(text=None):
    """{name: (restype, [argtypes])} of every WORLD_HIP_API declaration in include/world_hip.h (or in `text`).  Scalars map by
    their C type, char * to c_char_p, a pointer to a struct this module mirrors under the same name to POINTER(mirror), every
    other pointer (data, handles, T **, the handler typedef) to c_void_p.  Anything else is an ImportError that names it."""
    if text is None:
        return _installed_header()[1]
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)       # no comments,
    src = re.sub(r"^[ \t]*#.*$", " ", src, flags=re.M)               # no preprocessor lines
    structs, handlers = set(), set()                                 # the header's struct and function-pointer typedefs
    for m in re.finditer(r"\btypedef\b([^;{]*)(?:\{[^}]*\})?([^;]*);", src):
        decl = m.group(1) + m.group(2)
        if "(" in decl:
            handlers.update(re.findall(r"\(\s*\*\s*(\w+)\s*\)", decl)[:1])
        elif decl.split()[:1] == ["struct"]:
            structs.add(decl.split()[-1])

    def ctype(decl, named, where):
        base, stars = " ".join(decl.split("*")[0].split()), decl.count("*")
        if named and not stars:                   # "int fs": the last word is the parameter's name
            base = " ".join(base.split()[:-1])
        if stars == 0 and base in _SCALARS and (base != "void" or not named):
            return _SCALARS[base]
        if stars == 0 and base in handlers:
            return C.c_void_p
        if stars == 1 and base == "char":
            return C.c_char_p
        mirror = globals().get(base)
        if stars == 1 and base in structs and isinstance(mirror, type) and issubclass(mirror, C.Structure):
            return C.POINTER(mirror)
        if stars and (base in _POINTEES or base in structs):
            return C.c_void_p
        raise ImportError(f"include/world_hip.h: {where}: unknown type in '{' '.join(decl.split())}'")

    out = {}
    for m in re.finditer(r"\bWORLD_HIP_API\b([^;{}]*)[;{}]", src):
        decl = " ".join(m.group(1).split())
        d = re.fullmatch(r"(.*?)(\w+) ?\(([^()]*)\)", re.sub(r"\bconst\b", "", decl)) if m.group(0).endswith(";") else None
        if not d or not d.group(1).strip():
            raise ImportError(f"include/world_hip.h: cannot parse the declaration 'WORLD_HIP_API {decl}'")
        ret, name, params = d.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (ctype(ret, False, name), [ctype(p, True, name) for p in params])
    return out


def bind_from_header(lib):
    """restype and argtypes, from the header, on every declared symbol `lib` exports; the ones it lacks (an older build, the
    reference's own) are skipped, so callers ask hasattr() before using a feature family"""
    for name, (restype, argtypes) in header_prototypes().items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


bind_realtime = bind_from_header      # (tests/golden/make_golden_realtime.py binds this library or a reference build under this name)


def run_realtime_plan(L, plan):
    """Drive one reference-style synthesiser through a chunk plan and record everything its contract covers.

    plan: fs, frame_period (ms), fft_size, buffer_size, number_of_pointers, f0 [F], sp / ap [F][fft/2+1], chunks (frame
    counts that add up to at most F) and optionally drain_every (Synthesis2 until 0, then IsLocked, after every k-th
    successful AddParameters and after every refused one; default 1), refresh_before (RefreshSynthesizer before adding
    that chunk; default -1), stop_on_lock (stop at the first IsLocked() == 1, as test.cpp's "Synthesis 3" does).

    Returns a dict: calls [n, 2 + len(REALTIME_SCALARS) + 4] (op, return value, the scalar fields, randn_state after the
    call), out (every successful Synthesis2's buffer[0, buffer_size), concatenated), pulses (the pulse indices of every
    added chunk, concatenated), pulse_counts, rings [adds][3][number_of_pointers] (f0_length, f0_origin,
    number_of_pulses after each successful add; slots not written yet read 0)."""
    fs, fp, fft, bs, P = (int(plan["fs"]), float(plan["frame_period"]), int(plan["fft_size"]), int(plan["buffer_size"]),
                          int(plan["number_of_pointers"]))
    f0, sp, ap = _f64(plan["f0"]), _f64(plan["sp"]), _f64(plan["ap"])
    chunks = [int(c) for c in plan["chunks"]]
    drain_every = int(plan.get("drain_every", 1))
    refresh_before = int(plan.get("refresh_before", -1))
    stop_on_lock = bool(plan.get("stop_on_lock", False))
    # the reference keeps the caller's row-pointer arrays (not the rows) until it synthesises: they live as long as the plan
    rows_sp, rows_ap = _rows(sp), _rows(ap)

    def at(rows, i):
        return C.cast(C.c_void_p(C.cast(rows, C.c_void_p).value + i * C.sizeof(_dp)), C.POINTER(_dp))

    s = WorldSynthesizer()
    L.InitializeSynthesizer(fs, fp, fft, bs, P, C.byref(s))
    calls, out, pulses, counts, rings = [], [], [], [], []

    def record(op, ret):
        r = s.randn_state
        calls.append([op, ret] + [getattr(s, k) for k in REALTIME_SCALARS] +
                     [r.g_randn_x, r.g_randn_y, r.g_randn_z, r.g_randn_w])

    def drain():
        while True:
            r = L.Synthesis2(C.byref(s))
            record(RT_SYNTH, r)
            if r == 0:
                break
            out.append(np.ctypeslib.as_array(s.buffer, shape=(bs,)).copy())
        locked = L.IsLocked(C.byref(s))
        record(RT_LOCKED, locked)
        return locked

    i = k = adds = 0
    refused = 0
    try:
        while k < len(chunks):
            if k == refresh_before and refused == 0:
                L.RefreshSynthesizer(C.byref(s))
                record(RT_REFRESH, 0)
                refresh_before = -1
            n = chunks[k]
            r = L.AddParameters(f0[i:].ctypes.data_as(_dp), n, at(rows_sp, i), at(rows_ap, i), C.byref(s))
            record(RT_ADD, r)
            if r == 1:
                slot = (s.head_pointer - 1) % P
                npu = s.number_of_pulses[slot]
                counts.append(npu)
                if npu:
                    pulses.extend(s.pulse_locations_index[slot][:npu])
                i += n; k += 1; adds += 1; refused = 0
                w = min(adds, P)             # (slots never written hold whatever the reference's new[] left there)
                rings.append([[s.f0_length[j] if j < w else 0 for j in range(P)],
                              [s.f0_origin[j] if j < w else 0 for j in range(P)],
                              [s.number_of_pulses[j] for j in range(P)]])
                if adds % drain_every != 0 and k < len(chunks):
                    continue
            else:
                refused += 1
                if refused > 1:
                    break                    # refused again after draining: the ring cannot move
            if drain() and stop_on_lock:
                break
    finally:
        L.DestroySynthesizer(C.byref(s))
    return {"calls": np.array(calls, dtype=np.float64).reshape(-1, 2 + len(REALTIME_SCALARS) + 4),
            "out": np.concatenate(out) if out else np.zeros(0), "pulses": np.array(pulses, dtype=np.int64),
            "pulse_counts": np.array(counts, dtype=np.int64), "rings": np.array(rings, dtype=np.int64).reshape(-1, 3, P)}


def _hip_runtime_first():
    """torch ships its own libamdhip64; load it BEFORE libworld_hip.so so the process
    ends up with exactly one HIP runtime (the one torch allocates device memory with)."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -m world_amd.build` "
                          "(hipcc, gfx950). There is no non-GPU fallback.")
    _hip_runtime_first()
    lib = C.CDLL(path)
    # the batched ABI of the header this binding reads (include/world_hip.h: WORLD_HIP_ABI_VERSION).  Libraries of round 5
    # (tools/ab.py loads those) have the same prototypes and no version symbol; anything else is refused rather than called
    # with shifted arguments
    abi, current = lib.world_hip_abi_version() if hasattr(lib, "world_hip_abi_version") else 5, header_abi_version()
    if abi not in (5, current):
        raise ImportError(f"{path}: batched ABI version {abi}, this binding speaks 5-{current}")
    lib.abi_version = abi
    return bind_from_header(lib)


def frame_count(fs, x_length, frame_period):
    """GetSamplesForHarvest / GetSamplesForDIO."""
    return int(1000.0 * x_length / fs / frame_period) + 1


def resample_length(n_in, fs_in, fs_out):
    """samples of n_in samples at fs_in after conversion to fs_out: ceil(n_in * L / M) with L / M = fs_out / fs_in in lowest
    terms (include/world_hip.h: world_hip_resample_length; host arithmetic)"""
    import math
    n_in, fs_in, fs_out = int(n_in), int(fs_in), int(fs_out)
    if n_in < 1 or fs_in < 1 or fs_out < 1:
        raise ValueError(f"resample_length: {n_in} samples, {fs_in} -> {fs_out} Hz")
    g = math.gcd(fs_in, fs_out)
    n = -((-n_in * (fs_out // g)) // (fs_in // g))
    if n > 2 ** 31 - 1:
        raise ValueError(f"resample_length: {n_in} samples at {fs_in} Hz are more than INT_MAX at {fs_out} Hz")
    return n


def resample_option(quality="best"):
    """"best", "fast" or a (zeros, rolloff, kaiser_beta) triple -> WorldHipResampleOption (the presets' values are the
    header's, written once here as well so that no library is needed to name them)"""
    if isinstance(quality, WorldHipResampleOption):
        return quality
    if isinstance(quality, str):
        if quality not in RESAMPLE_QUALITIES:
            raise ValueError(f"resample: quality {quality!r} is neither 'best' nor 'fast' nor a (zeros, rolloff, beta) triple")
        return WorldHipResampleOption(*{"best": (64, 0.9475937167399596, 14.769656459379492),
                                        "fast": (16, 0.85, 8.555504641634386)}[quality])
    try:
        zeros, rolloff, beta = quality
        if int(zeros) != zeros:
            raise ValueError
        return WorldHipResampleOption(int(zeros), float(rolloff), float(beta))
    except (TypeError, ValueError):
        raise ValueError(f"resample: quality {quality!r} is neither 'best' nor 'fast' nor a (zeros, rolloff, beta) triple") from None


def cheaptrick_fft_size(fs, f0_floor=71.0):
    import math
    return int(2.0 ** (1.0 + int(math.log(3.0 * fs / f0_floor + 1) / 0.69314718055994529)))


def _ints(v):
    a = np.ascontiguousarray(v, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp)


def _rows(a):
    """double** view over a dense 2-D array (the reference's row-pointer ABI).  The row addresses are computed by numpy
    and handed over as one pointer array (a Python loop over 2001 rows cost the caller milliseconds per call); the array
    object keeps itself alive on the ctypes pointer."""
    addr = (a.ctypes.data + a.strides[0] * np.arange(a.shape[0], dtype=np.uintp)).astype(np.uintp)
    ptrs = addr.ctypes.data_as(C.POINTER(_dp))
    ptrs._keep = addr
    return ptrs


class HostAPI:
    """numpy binding of the reference's 13-symbol C ABI.  It is the
    ctypes stub a user of the reference library would write; it works unchanged on
    libworld_hip.so (default) and on any build of the reference itself."""
    kind = "cabi"

    def __init__(self, path=LIB_PATH, hip_runtime=True):
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing (python -m world_amd.build); there is no fallback.")
        self.path = path
        if hip_runtime:                      # False only for CPU-only libraries (the reference build)
            _hip_runtime_first()
        self.lib = bind_from_header(C.CDLL(path))   # (the reference's build exports the same names with the same signatures)

    def frame_count(self, fs, n, frame_period):
        return frame_count(fs, n, frame_period)

    def cheaptrick_fft_size(self, fs, f0_floor=71.0):
        return cheaptrick_fft_size(fs, f0_floor)

    def harvest(self, x, fs, f0_floor=71.0, f0_ceil=800.0, frame_period=5.0):
        x = _f64(x)
        opt = HarvestOption(); self.lib.InitializeHarvestOption(C.byref(opt))
        opt.f0_floor, opt.f0_ceil, opt.frame_period = f0_floor, f0_ceil, frame_period
        nf = self.lib.GetSamplesForHarvest(fs, len(x), frame_period)
        tp = np.zeros(nf); f0 = np.zeros(nf)
        self.lib.Harvest(_p(x), len(x), fs, C.byref(opt), _p(tp), _p(f0))
        return tp, f0

    def dio(self, x, fs, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, frame_period=5.0,
            speed=1, allowed_range=0.1):
        x = _f64(x)
        opt = DioOption(); self.lib.InitializeDioOption(C.byref(opt))
        opt.f0_floor, opt.f0_ceil, opt.channels_in_octave = f0_floor, f0_ceil, channels_in_octave
        opt.frame_period, opt.speed, opt.allowed_range = frame_period, speed, allowed_range
        nf = self.lib.GetSamplesForDIO(fs, len(x), frame_period)
        tp = np.zeros(nf); f0 = np.zeros(nf)
        self.lib.Dio(_p(x), len(x), fs, C.byref(opt), _p(tp), _p(f0))
        return tp, f0

    def stonemask(self, x, fs, tp, f0):
        x, tp, f0 = _f64(x), _f64(tp), _f64(f0)
        out = np.zeros(len(f0))
        self.lib.StoneMask(_p(x), len(x), fs, _p(tp), _p(f0), len(f0), _p(out))
        return out

    def cheaptrick(self, x, fs, tp, f0, q1=-0.15, f0_floor=71.0, fft_size=None):
        x, tp, f0 = _f64(x), _f64(tp), _f64(f0)
        opt = CheapTrickOption(); self.lib.InitializeCheapTrickOption(fs, C.byref(opt))
        opt.q1, opt.f0_floor = q1, f0_floor
        opt.fft_size = fft_size or self.lib.GetFFTSizeForCheapTrick(fs, C.byref(opt))
        sp = np.zeros((len(f0), opt.fft_size // 2 + 1))
        self.lib.CheapTrick(_p(x), len(x), fs, _p(tp), _p(f0), len(f0), C.byref(opt), _rows(sp))
        return sp

    def d4c(self, x, fs, tp, f0, fft_size, threshold=0.85):
        x, tp, f0 = _f64(x), _f64(tp), _f64(f0)
        opt = D4COption(); self.lib.InitializeD4COption(C.byref(opt))
        opt.threshold = threshold
        ap = np.zeros((len(f0), fft_size // 2 + 1))
        self.lib.D4C(_p(x), len(x), fs, _p(tp), _p(f0), len(f0), fft_size, C.byref(opt), _rows(ap))
        return ap

    # -- synthesis (reference synthesis.h:30) --
    def synthesis(self, f0, sp, ap, fft_size, frame_period, fs, y_length):
        f0, sp, ap = _f64(f0), _f64(sp), _f64(ap)
        y = np.zeros(y_length)
        self.lib.Synthesis(_p(f0), len(f0), _rows(sp), _rows(ap), fft_size, frame_period, fs, y_length, _p(y))
        return y

    # -- real-time synthesis (reference synthesisrealtime.h) --
    def _rt(self):
        """the library for a raw call of a real-time symbol (they are bound with the rest)"""
        return self.lib

    def initialize_synthesizer(self, fs, frame_period, fft_size, buffer_size, number_of_pointers):
        s = WorldSynthesizer()
        self.lib.InitializeSynthesizer(fs, frame_period, fft_size, buffer_size, number_of_pointers, C.byref(s))
        return s

    def add_parameters(self, synth, f0, sp, ap):
        """AddParameters of one chunk; the row pointers only live for the call (this library copies the rows then)"""
        f0, sp, ap = _f64(f0), _f64(sp), _f64(ap)
        return self.lib.AddParameters(_p(f0), len(f0), _rows(sp), _rows(ap), C.byref(synth))

    def synthesis2(self, synth):
        """(return value, copy of buffer[0, buffer_size))"""
        r = self.lib.Synthesis2(C.byref(synth))
        return r, np.ctypeslib.as_array(synth.buffer, shape=(synth.buffer_size,)).copy()

    def is_locked(self, synth):
        return self.lib.IsLocked(C.byref(synth))

    def refresh_synthesizer(self, synth):
        self.lib.RefreshSynthesizer(C.byref(synth))

    def destroy_synthesizer(self, synth):
        self.lib.DestroySynthesizer(C.byref(synth))

    def realtime_plan(self, plan):
        """run_realtime_plan() on this library"""
        return run_realtime_plan(self.lib, plan)

    # -- codec (reference codec.h) --
    def number_of_aperiodicities(self, fs):
        return self.lib.GetNumberOfAperiodicities(fs)

    def code_aperiodicity(self, ap, fs, fft_size):
        ap = _f64(ap)
        out = np.zeros((ap.shape[0], self.number_of_aperiodicities(fs)))
        self.lib.CodeAperiodicity(_rows(ap), ap.shape[0], fs, fft_size, _rows(out))
        return out

    def decode_aperiodicity(self, coded, fs, fft_size):
        coded = _f64(coded)
        out = np.zeros((coded.shape[0], fft_size // 2 + 1))
        self.lib.DecodeAperiodicity(_rows(coded), coded.shape[0], fs, fft_size, _rows(out))
        return out

    def code_spectral_envelope(self, sp, fs, fft_size, ndim):
        sp = _f64(sp)
        out = np.zeros((sp.shape[0], ndim))
        self.lib.CodeSpectralEnvelope(_rows(sp), sp.shape[0], fs, fft_size, ndim, _rows(out))
        return out

    def decode_spectral_envelope(self, coded, fs, fft_size):
        coded = _f64(coded)
        out = np.zeros((coded.shape[0], fft_size // 2 + 1))
        self.lib.DecodeSpectralEnvelope(_rows(coded), coded.shape[0], fs, fft_size, coded.shape[1], _rows(out))
        return out

    # ---- the Gaussian mixture's host arithmetic (include/world_hip.h: world_hip_gmm_prepare / _model_parts / _update) ----
    def _gmm(self, name, *args):
        return getattr(self.lib, name)(*(a if isinstance(a, (int, float)) or a is None else a.ctypes.data for a in args))

    def _gmm_check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.world_hip_last_error().decode()}")

    def gmm_prepare(self, w, mu, cov, dx):
        """w [M], mu [M][P], cov [M][P][P], the source dimension -> the prepared model's doubles (the library's layout)"""
        w, mu, cov = _f64(w), _f64(mu), _f64(cov)
        M, P = (int(v) for v in mu.shape)
        n = self._gmm("world_hip_gmm_model_doubles", M, int(dx), P - int(dx))
        self._gmm_check(int(n < 0), "gmm_prepare")
        model = np.empty(n, dtype=np.float64)
        self._gmm_check(self._gmm("world_hip_gmm_prepare", M, int(dx), P - int(dx), w, mu, cov, model), "gmm_prepare")
        return model

    def gmm_model_parts(self, M, dx, dy, model):
        """-> {"c" [M], "mux" [M][dx], "muy" [M][dy], "U" [M][dx][dx], "A" [M][dy][dx], "v" [M][dy]}: what the device multiplies by"""
        out = dict(c=np.empty(M), mux=np.empty((M, dx)), muy=np.empty((M, dy)), U=np.empty((M, dx, dx)), A=np.empty((M, dy, dx)),
                   v=np.empty((M, dy)))
        self._gmm_check(self._gmm("world_hip_gmm_model_parts", int(M), int(dx), int(dy), _f64(model), *out.values()), "gmm_model_parts")
        return out

    def gmm_update(self, N, S1, G, shift, total_rows, reg=0.0):
        """the M-step's finish on the statistics of world_hip_gmm_accumulate -> (w, mu, cov)"""
        N, S1, G, shift = _f64(N), _f64(S1), _f64(G), _f64(shift)
        M, P = (int(v) for v in S1.shape)
        w, mu, cov = np.empty(M), np.empty((M, P)), np.empty((M, P, P))
        self._gmm_check(self._gmm("world_hip_gmm_update", M, P, N, S1, G, shift, float(total_rows), float(reg), w, mu, cov), "gmm_update")
        return w, mu, cov


class FileAPI:
    """numpy binding of the reference's tools/ library (tools/audioio.h, tools/parameterio.h;
    SURVEY.md 8f.2): WAV and F0 / SPEC / AP files.  Like HostAPI it works unchanged on
    libworld_hip.so (default) and on a build of the reference's own tools."""

    def __init__(self, path=LIB_PATH, hip_runtime=True):
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing (python -m world_amd.build); there is no fallback.")
        if hip_runtime:
            _hip_runtime_first()
        self.lib = bind_from_header(C.CDLL(path))

    @staticmethod
    def _s(path):
        return os.fsencode(path)

    def audio_length(self, path):
        return self.lib.GetAudioLength(self._s(path))

    def wavread(self, path):
        """-> (x, fs, nbit), or None where the reference prints an error and leaves x untouched."""
        n = self.audio_length(path)
        if n <= 0:
            return None
        x = np.zeros(n)
        fs, nbit = C.c_int(0), C.c_int(0)
        self.lib.wavread(self._s(path), C.byref(fs), C.byref(nbit), _p(x))
        return x, fs.value, nbit.value

    def wavwrite(self, path, x, fs, nbit=16):
        x = _f64(x)
        self.lib.wavwrite(_p(x), len(x), fs, nbit, self._s(path))

    def write_f0(self, path, frame_period, tpos, f0, text=False):
        tpos, f0 = _f64(tpos), _f64(f0)
        self.lib.WriteF0(self._s(path), len(f0), frame_period, _p(tpos), _p(f0), 1 if text else 0)

    def header(self, path, parameter):
        return self.lib.GetHeaderInformation(self._s(path), parameter.encode())

    def read_f0(self, path):
        n = int(self.header(path, "NOF "))
        tpos, f0 = np.zeros(n), np.zeros(n)
        return (tpos, f0) if self.lib.ReadF0(self._s(path), _p(tpos), _p(f0)) == 1 else None

    def _write_matrix(self, fn, path, m, fs, frame_period, fft_size, number_of_dimensions):
        m = _f64(m)
        fn(self._s(path), fs, m.shape[0], frame_period, fft_size, number_of_dimensions, _rows(m))

    def _read_matrix(self, fn, path):
        rows, fft, nod = (int(self.header(path, k)) for k in ("NOF ", "FFT ", "NOD "))
        m = np.zeros((rows, nod if nod else fft // 2 + 1))
        return m if fn(self._s(path), _rows(m)) == 1 else None

    def write_spectral_envelope(self, path, sp, fs, frame_period, fft_size, number_of_dimensions=0):
        self._write_matrix(self.lib.WriteSpectralEnvelope, path, sp, fs, frame_period, fft_size, number_of_dimensions)

    def write_aperiodicity(self, path, ap, fs, frame_period, fft_size, number_of_dimensions=0):
        self._write_matrix(self.lib.WriteAperiodicity, path, ap, fs, frame_period, fft_size, number_of_dimensions)

    def read_spectral_envelope(self, path):
        return self._read_matrix(self.lib.ReadSpectralEnvelope, path)

    def read_aperiodicity(self, path):
        return self._read_matrix(self.lib.ReadAperiodicity, path)


class GmmModel:
    """a prepared joint-density mixture on the device (WorldHip.gmm_prepare): M mixtures, dx source and dy target
    dimensions, `data` the model's doubles in the library's layout"""

    def __init__(self, M, dx, dy, data):
        self.M, self.dx, self.dy, self.data = M, dx, dy, data


class Graph:
    """a captured sequence of batched calls (WorldHip.capture): launch() replays it on the stream it was captured on"""

    def __init__(self, wh, ctx, handle):
        self.wh, self.ctx, self.handle = wh, ctx, handle

    def launch(self):
        self.wh._check(self.wh.lib.world_hip_graph_launch(self.ctx, self.handle), "graph_launch")

    def close(self):
        if self.handle:
            self.wh.lib.world_hip_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WorldHip:
    """Batched analysis on one GPU.  Tensors: x [B, L] float64 on the GPU."""

    def __init__(self, device=None, lib_path=LIB_PATH, shared_device=False):
        """shared_device: other jobs run on this GPU at the same time (world_hip.h: WORLD_HIP_HINT_SHARED_DEVICE) --
        single-utterance calls keep the narrow launch shapes.  Results never depend on it."""
        import torch
        self.torch = torch
        self.shared_device = bool(shared_device)
        if not torch.cuda.is_available():
            raise RuntimeError("WorldHip needs a GPU (torch.cuda.is_available() is False)")
        self.lib = load_library(lib_path)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._ctxs = {}                  # stream handle -> library context
        self._realtime = weakref.WeakSet()   # open RealtimeStreams: they use a context, so close() closes them first

    def _context(self):
        """One library context (workspace + stream binding) per torch stream in use, created lazily and kept:
        code that alternates streams on one WorldHip keeps one context per stream."""
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        ctx = self._ctxs.get(s)
        if ctx is None:
            ctx = self.lib.world_hip_create(self.device.index, C.c_void_p(s))
            if not ctx:
                raise RuntimeError("world_hip_create: " + self.lib.world_hip_last_error().decode())
            if self.shared_device and hasattr(self.lib, "world_hip_set_hint"):
                self.lib.world_hip_set_hint(C.c_void_p(ctx), 1)
            self._ctxs[s] = ctx
        return ctx

    @property
    def ctx(self):
        """the context of torch's current stream (None before the first call on it)"""
        return self._ctxs.get(self.torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        for rt in list(getattr(self, "_realtime", ())):
            rt.close()
        for ctx in self._ctxs.values():
            self.lib.world_hip_destroy(ctx)
        self._ctxs = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.world_hip_last_error().decode()}")

    def _prep(self, x, x_len):
        t = self.torch
        assert x.dtype == t.float64 and x.is_cuda and x.dim() == 2 and x.is_contiguous()
        assert x.device == self.device, f"x lives on {x.device}, this WorldHip on {self.device}"
        B, L = x.shape
        if x_len is None:
            x_len = [L] * B
        return B, L, np.ascontiguousarray(x_len, dtype=np.int32)

    def profile(self, fn):
        """Run fn() with per-kernel HIP-event timing; returns {kernel: [ms per launch, ...]}."""
        self.lib.world_hip_profile_enable(1)
        try:
            fn()
        finally:
            self.lib.world_hip_profile_enable(0)
        buf = C.create_string_buffer(1 << 22)
        if self.lib.world_hip_profile_collect(buf, len(buf)) < 0:
            raise RuntimeError("profile: " + self.lib.world_hip_last_error().decode())
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms = line.rsplit(None, 1)      # (a template's label has blanks: "(fft_probe_rfft<3, 11>) 0.01")
            out.setdefault(name, []).append(float(ms))
        return out

    def workspace_bytes(self):
        """bytes of device workspace held by this object's contexts (their arenas)"""
        return sum(int(self.lib.world_hip_workspace_bytes(c)) for c in self._ctxs.values())

    def noise_table_bytes(self):
        """bytes of the device's shared randn table (one per device and process)"""
        return int(self.lib.world_hip_noise_table_bytes(self._context()))

    def verify_tables(self):
        """re-reduce the shared randn table on the device and compare with the host's sums; True = intact"""
        return self.lib.world_hip_verify_tables(self._context()) == 0

    # ---- F0 ----
    def harvest(self, x, fs, x_len=None, f0_floor=71.0, f0_ceil=800.0, frame_period=5.0):
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        nf = np.array([frame_count(fs, int(n), frame_period) for n in xl], dtype=np.int32)
        F = int(nf.max())
        tpos = t.zeros((B, F), dtype=t.float64, device=x.device)
        f0 = t.zeros((B, F), dtype=t.float64, device=x.device)
        opt = HarvestOption(f0_floor, f0_ceil, frame_period)
        self._check(self.lib.world_hip_harvest_batch(self._context(), B, fs, x.data_ptr(), L,
                                                     xl.ctypes.data_as(_ip), C.byref(opt), F,
                                                     tpos.data_ptr(), f0.data_ptr()), "harvest")
        return tpos, f0, nf

    def dio(self, x, fs, x_len=None, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, frame_period=5.0,
            speed=1, allowed_range=0.1):
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        nf = np.array([frame_count(fs, int(n), frame_period) for n in xl], dtype=np.int32)
        F = int(nf.max())
        tpos = t.zeros((B, F), dtype=t.float64, device=x.device)
        f0 = t.zeros((B, F), dtype=t.float64, device=x.device)
        opt = DioOption(f0_floor, f0_ceil, channels_in_octave, frame_period, speed, allowed_range)
        self._check(self.lib.world_hip_dio_batch(self._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(_ip),
                                                 C.byref(opt), F, tpos.data_ptr(), f0.data_ptr()), "dio")
        return tpos, f0, nf

    def stonemask(self, x, fs, tpos, f0, n_frames, x_len=None):
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        out = t.zeros_like(f0)
        self._check(self.lib.world_hip_stonemask_batch(self._context(), B, fs, x.data_ptr(), L,
                                                       xl.ctypes.data_as(_ip), nf.ctypes.data_as(_ip), f0.shape[1],
                                                       tpos.data_ptr(), f0.data_ptr(), out.data_ptr()), "stonemask")
        return out

    # ---- spectral stages ----
    def cheaptrick(self, x, fs, tpos, f0, n_frames, x_len=None, q1=-0.15, f0_floor=71.0, fft_size=None, out=None):
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        fft_size = fft_size or cheaptrick_fft_size(fs, f0_floor)
        F = f0.shape[1]
        sp = out if out is not None else t.zeros((B, F, fft_size // 2 + 1), dtype=t.float64, device=x.device)
        opt = CheapTrickOption(q1, f0_floor, fft_size)
        self._check(self.lib.world_hip_cheaptrick_batch(self._context(), B, fs, x.data_ptr(), L,
                                                        xl.ctypes.data_as(_ip), nf.ctypes.data_as(_ip), F,
                                                        tpos.data_ptr(), f0.data_ptr(), C.byref(opt),
                                                        sp.data_ptr()), "cheaptrick")
        return sp

    def d4c(self, x, fs, tpos, f0, n_frames, fft_size, x_len=None, threshold=0.85, out=None):
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        F = f0.shape[1]
        ap = out if out is not None else t.zeros((B, F, fft_size // 2 + 1), dtype=t.float64, device=x.device)
        opt = D4COption(threshold)
        self._check(self.lib.world_hip_d4c_batch(self._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(_ip),
                                                 nf.ctypes.data_as(_ip), F, tpos.data_ptr(), f0.data_ptr(),
                                                 fft_size, C.byref(opt), ap.data_ptr()), "d4c")
        return ap

    def synthesis(self, f0, sp, ap, n_frames, fft_size, frame_period, fs, y_length, check_pulses=True):
        """reference Synthesis() on a batch: f0 [B, F], sp / ap [B, F, fft/2+1] (float64, device);
        n_frames and y_length are per-utterance ints; returns y [B, max(y_length)].  check_pulses=False skips the (synchronising)
        check that every pitch pulse found room in the workspace -- the caller then asks synthesis_pulses_dropped() itself"""
        t = self.torch
        f0, sp, ap = f0.contiguous(), sp.contiguous(), ap.contiguous()
        B, F = f0.shape
        nf = np.ascontiguousarray(np.broadcast_to(n_frames, (B,)), dtype=np.int32)
        yl = np.ascontiguousarray(np.broadcast_to(y_length, (B,)), dtype=np.int32)
        Y = int(yl.max())
        y = t.zeros((B, Y), dtype=t.float64, device=f0.device)
        def run():
            self._check(self.lib.world_hip_synthesis_batch(self._context(), B, fs, float(frame_period), fft_size,
                                                           nf.ctypes.data_as(_ip), F, f0.data_ptr(), sp.data_ptr(),
                                                           ap.data_ptr(), yl.ctypes.data_as(_ip), Y, y.data_ptr()),
                        "synthesis")
        run()
        if check_pulses:
            # the pulse count is data dependent and only known on the device: a call that had no room for some says so
            # (this synchronises); repeat it once with exactly the capacity it asked for -- never a silently truncated waveform
            need = self.synthesis_pulses_dropped()
            if need:
                if need > Y:
                    raise RuntimeError(f"synthesis: {need} pitch pulses for {Y} output samples")
                self.set_synthesis_pulse_capacity(need + 16)
                try:
                    run()
                    if self.synthesis_pulses_dropped():
                        raise RuntimeError("synthesis: pulses dropped even at the requested capacity")
                finally:
                    self.set_synthesis_pulse_capacity(0)
        return y

    def synthesize_records(self, block, n_frames, fs, fft_size, frame_period, y_length, wire=0, number_of_dimensions=0,
                           first_row=0, check_pulses=True):
        """Synthesis() straight from the records analyze_packed / analyze_coded write (include/world_hip.h:
        world_hip_synthesis_records): block [rows, cols] float64 on the device, utterance u's n_frames[u] records from row
        first_row + sum(n_frames[:u]).  wire 0: f64 records, 1: f32 records, 2: coded records with number_of_dimensions
        coefficients.  Returns y [B, max(y_length)]; check_pulses as synthesis()."""
        t = self.torch
        if not hasattr(self.lib, "world_hip_synthesis_records"):
            raise RuntimeError("this libworld_hip.so has no synthesis from records (world_hip_synthesis_records)")
        nf = np.ascontiguousarray(n_frames, dtype=np.int32).reshape(-1)
        B = len(nf)
        yl = np.ascontiguousarray(np.broadcast_to(y_length, (B,)), dtype=np.int32)
        Y = int(yl.max())
        assert block.dtype == t.float64 and block.dim() == 2 and block.is_contiguous() and block.is_cuda
        assert first_row >= 0 and first_row + int(nf.sum()) <= block.shape[0], "the block holds fewer records than n_frames asks for"
        y = t.zeros((B, Y), dtype=t.float64, device=block.device)

        def run():
            self._check(self.lib.world_hip_synthesis_records(self._context(), B, int(fs), float(frame_period), int(fft_size),
                                                             nf.ctypes.data_as(_ip), int(first_row), block.data_ptr(),
                                                             int(block.shape[1]), int(wire), int(number_of_dimensions),
                                                             yl.ctypes.data_as(_ip), Y, y.data_ptr()), "synthesize_records")
        run()
        if check_pulses:
            need = self.synthesis_pulses_dropped()          # (synchronises) -- as synthesis(): one repeat at the asked capacity
            if need:
                if need > Y:
                    raise RuntimeError(f"synthesize_records: {need} pitch pulses for {Y} output samples")
                self.set_synthesis_pulse_capacity(need + 16)
                try:
                    run()
                    if self.synthesis_pulses_dropped():
                        raise RuntimeError("synthesize_records: pulses dropped even at the requested capacity")
                finally:
                    self.set_synthesis_pulse_capacity(0)
        return y

    # ---- parameter modification (include/world_hip.h: world_hip_modify_batch; reference test.cpp ParameterModification) ----
    def _modify_lib(self):
        if not hasattr(self.lib, "world_hip_modify_batch"):
            raise RuntimeError("this libworld_hip.so has no parameter modification (world_hip_modify_batch)")
        return self.lib

    def f0_statistics(self, f0, n_frames):
        """f0 [B, F] float64 (device) -> [B, 3] {voiced frames, mean ln f0, std ln f0} over each utterance's voiced frames"""
        t = self.torch
        L = self._modify_lib()
        assert f0.dtype == t.float64 and f0.dim() == 2 and f0.is_contiguous() and f0.device == self.device
        B, F = f0.shape
        nf = np.ascontiguousarray(np.broadcast_to(n_frames, (B,)), dtype=np.int32)
        stats = t.empty((B, 3), dtype=t.float64, device=f0.device)
        self._check(L.world_hip_f0_statistics(self._context(), B, nf.ctypes.data_as(_ip), F, f0.data_ptr(), stats.data_ptr()),
                    "f0_statistics")
        return stats

    def modify(self, f0, sp, n_frames, fs, fft_size, f0_scale=1.0, formant_shift=1.0, log_f0_target=None, out=None):
        """test.cpp's ParameterModification on a batch: f0 [B, F] and / or sp [B, F, fft/2+1] (float64, device; either may
        be None).  f0_scale, formant_shift: scalars or per-utterance sequences; log_f0_target: (means, stds) of the voiced
        log F0 to map each utterance onto, or None.  out: None = new tensors, "inplace" = the inputs are overwritten, or a
        (f0_out, sp_out) pair.  Returns (f0', sp')."""
        t = self.torch
        L = self._modify_lib()
        ref = f0 if f0 is not None else sp
        assert ref is not None, "modify: nothing to modify"
        B, F = ref.shape[0], ref.shape[1]
        for a, dims in ((f0, 2), (sp, 3)):
            if a is not None:
                assert a.dtype == t.float64 and a.dim() == dims and a.is_contiguous() and a.device == self.device
                assert a.shape[:2] == (B, F)
        if sp is not None:
            assert sp.shape[2] == fft_size // 2 + 1
        if out == "inplace":
            f0_out, sp_out = f0, sp
        elif out is not None:
            f0_out, sp_out = out
        else:
            f0_out = t.empty_like(f0) if f0 is not None else None
            sp_out = t.empty_like(sp) if sp is not None else None
            # (rows beyond an utterance's frames are not written: carry the padding over)
            nf_min = int(np.min(n_frames))
            if nf_min < F:
                if f0_out is not None:
                    f0_out.copy_(f0)
                if sp_out is not None:
                    sp_out.copy_(sp)
        nf = np.ascontiguousarray(np.broadcast_to(n_frames, (B,)), dtype=np.int32)
        mods = modifications(B, f0_scale, formant_shift, log_f0_target)
        ptr = lambda a: a.data_ptr() if a is not None else None
        self._check(L.world_hip_modify_batch(self._context(), B, int(fs), int(fft_size), nf.ctypes.data_as(_ip), F, mods,
                                             ptr(f0), ptr(f0_out), ptr(sp), ptr(sp_out)), "modify")
        return f0_out, sp_out

    def resynthesis_length(self, fs, n_frames, frame_period=5.0, time_scale=1.0):
        return int(self._modify_lib().world_hip_resynthesis_length(int(fs), int(n_frames), float(frame_period),
                                                                    float(time_scale)))

    def resynthesize(self, x, fs, x_len=None, f0_scale=1.0, formant_shift=1.0, time_scale=1.0, log_f0_target=None,
                     frame_period=5.0, f0_floor=71.0, f0_ceil=800.0, q1=-0.15, threshold=0.85, out=None):
        """analyze -> modify -> synthesis in one library call (world_hip_resynthesize_batch): x [B, L] float64 (device) ->
        (y [B, max(y_length)], y_length).  f0_floor / f0_ceil are Harvest's (CheapTrick keeps 71 Hz, as analyze());
        synthesis runs at frame_period * time_scale.  Like synthesis(), a call whose pulses did not all fit is repeated
        once at the capacity the device asked for -- never a truncated waveform.  out: a preallocated y of that shape."""
        t = self.torch
        L = self._modify_lib()
        B, Lx, xl = self._prep(x, x_len)
        fft_size = cheaptrick_fft_size(fs, 71.0)
        yl = np.array([L.world_hip_resynthesis_length(int(fs), frame_count(fs, int(n), frame_period), float(frame_period),
                                                      float(time_scale)) for n in xl], dtype=np.int32)
        if int(yl.min()) < 1:
            raise ValueError(f"resynthesize: invalid frame_period {frame_period} / time_scale {time_scale}")
        Y = int(yl.max())
        y = out if out is not None else t.zeros((B, Y), dtype=t.float64, device=x.device)
        assert y.dtype == t.float64 and y.is_contiguous() and y.shape == (B, Y) and y.device == x.device
        mods = modifications(B, f0_scale, formant_shift, log_f0_target)
        hopt, copt, dopt = HarvestOption(f0_floor, f0_ceil, frame_period), CheapTrickOption(q1, 71.0, fft_size), D4COption(threshold)

        def run():
            self._check(L.world_hip_resynthesize_batch(self._context(), B, int(fs), x.data_ptr(), Lx, xl.ctypes.data_as(_ip),
                                                       C.byref(hopt), C.byref(copt), C.byref(dopt), mods, float(time_scale),
                                                       yl.ctypes.data_as(_ip), Y, y.data_ptr()), "resynthesize")
        run()
        need = self.synthesis_pulses_dropped()          # (synchronises) -- as synthesis(): one repeat at the asked capacity
        if need:
            if need > Y:
                raise RuntimeError(f"resynthesize: {need} pitch pulses for {Y} output samples")
            self.set_synthesis_pulse_capacity(need + 16)
            try:
                run()
                if self.synthesis_pulses_dropped():
                    raise RuntimeError("resynthesize: pulses dropped even at the requested capacity")
            finally:
                self.set_synthesis_pulse_capacity(0)
        return y, yl

    # ---- frame-wise modification behind a time map (include/world_hip.h: world_hip_modify_frames_batch) ----
    def _frames_lib(self):
        if not hasattr(self.lib, "world_hip_modify_frames_batch"):
            raise RuntimeError("this libworld_hip.so has no frame-wise modification (world_hip_modify_frames_batch)")
        return self.lib

    def _frame_curves(self, B, time_map, f0_target, f0_scale, formant_shift, ap_gain):
        """(the curves given, by WorldHipFrameCurves field; per-utterance f0_scale; per-utterance formant_shift; their
        common width O or None).  f0_scale / formant_shift given as tensors are curves; anything else is one value per
        utterance.  Curves are [B, O] float64 device tensors ([O]: shared by the batch)."""
        t = self.torch
        curves = dict(d_time_map=time_map, d_f0_target=f0_target, d_ap_gain=ap_gain,
                      d_f0_scale=f0_scale if t.is_tensor(f0_scale) else None,
                      d_formant_shift=formant_shift if t.is_tensor(formant_shift) else None)
        keep, O = {}, None
        for name, a in curves.items():
            if a is None:
                continue
            assert a.dtype == t.float64 and a.device == self.device, f"{name[2:]}: a float64 tensor on {self.device}"
            if a.dim() == 1:
                a = a[None].expand(B, -1)
            assert a.dim() == 2 and a.shape[0] == B, f"{name[2:]}: [B, O] or [O]"
            O = a.shape[1] if O is None else O
            assert a.shape[1] == O, "the curves disagree about the number of output frames"
            keep[name] = a.contiguous()
        return (keep, 1.0 if "d_f0_scale" in keep else f0_scale, 1.0 if "d_formant_shift" in keep else formant_shift, O)

    def _validate_curves(self, keep, n_out, fft_size):
        """The curve values of the frames below n_out, checked on the device (one reduction, one synchronisation): a value
        the library would replace by 1 raises instead.  f0_target is free: not finite or <= 0 means "keep this frame"."""
        t = self.torch
        bad = t.zeros((), dtype=t.bool, device=self.device)
        for name, a in keep.items():
            if name == "d_time_map":
                wrong = t.isnan(a)
            elif name == "d_f0_target":
                continue
            elif name == "d_formant_shift":
                wrong = ~t.isfinite(a) | ~(a > 0) | ~(fft_size / 2.0 * a >= 1.0)
            else:
                wrong = ~t.isfinite(a) | (a < 0)
            live = t.arange(a.shape[1], device=self.device)[None] < t.as_tensor(n_out, device=self.device)[:, None]
            bad = bad | (wrong & live).any()
        if keep and bool(bad):
            raise ValueError("a curve holds a value outside its range (time_map: NaN; f0_scale, ap_gain: not finite or < 0; "
                             "formant_shift: not finite, <= 0 or below 2 / fft_size)")

    def modify_frames(self, f0, sp, ap, n_frames, fs, fft_size, n_out=None, time_map=None, f0_target=None, f0_scale=1.0,
                      formant_shift=1.0, ap_gain=None, log_f0_target=None, out=None, validate=True):
        """Per-frame modification and time warping in one pass: f0 [B, F], sp / ap [B, F, fft/2+1] (float64, device; any
        may be None) -> (f0', sp', ap') with n_out[u] output frames each ([B, O] / [B, O, fft/2+1]).  time_map [B, O] or
        [O]: the source position of every output frame, in source frames (uniform_time_map, hold_time_map); None keeps
        the frames where they are (n_out = n_frames).  f0_target, ap_gain: curves or None; f0_scale, formant_shift: a
        curve (tensor), or one value per utterance as in modify().  n_out: frames per utterance, default all O.  out: None
        = new tensors (zero beyond n_out), "inplace" (without a time map only), or an (f0_out, sp_out, ap_out) triple."""
        t = self.torch
        L = self._frames_lib()
        ref = next((a for a in (f0, sp, ap) if a is not None), None)
        assert ref is not None, "modify_frames: nothing to modify"
        B, F = ref.shape[0], ref.shape[1]
        nb = fft_size // 2 + 1
        for a, dims in ((f0, 2), (sp, 3), (ap, 3)):
            if a is not None:
                assert a.dtype == t.float64 and a.dim() == dims and a.is_contiguous() and a.device == self.device
                assert a.shape[:2] == (B, F) and (dims == 2 or a.shape[2] == nb)
        nf = np.ascontiguousarray(np.broadcast_to(n_frames, (B,)), dtype=np.int32)
        keep, scale, ratio, O = self._frame_curves(B, time_map, f0_target, f0_scale, formant_shift, ap_gain)
        O = F if O is None else O
        if n_out is None:
            n_out = nf if time_map is None else O
        no = np.ascontiguousarray(np.broadcast_to(n_out, (B,)), dtype=np.int32)
        if validate:
            self._validate_curves(keep, no, fft_size)
        cv = WorldHipFrameCurves(**{name: a.data_ptr() for name, a in keep.items()})
        if out == "inplace":
            outs = (f0, sp, ap)
        elif out is not None:
            outs = tuple(out)
        else:
            shape = lambda a: (B, O) + tuple(a.shape[2:])
            outs = tuple(t.zeros(shape(a), dtype=t.float64, device=self.device) if a is not None else None
                         for a in (f0, sp, ap))
        for a, o in zip((f0, sp, ap), outs):
            assert (a is None) == (o is None)
            if o is not None:
                assert o.dtype == t.float64 and o.is_contiguous() and o.device == self.device
                assert o.shape == (B, O) + tuple(a.shape[2:])
        mods = modifications(B, scale, ratio, log_f0_target)
        ptr = lambda a: a.data_ptr() if a is not None else None
        self._check(L.world_hip_modify_frames_batch(self._context(), B, int(fs), int(fft_size), nf.ctypes.data_as(_ip), F,
                                                    no.ctypes.data_as(_ip), O, mods, C.byref(cv), ptr(f0), ptr(outs[0]),
                                                    ptr(sp), ptr(outs[1]), ptr(ap), ptr(outs[2])), "modify_frames")
        return outs

    def resynthesize_frames(self, x, fs, x_len=None, n_out=None, time_map=None, f0_target=None, f0_scale=1.0,
                            formant_shift=1.0, ap_gain=None, log_f0_target=None, frame_period=5.0, f0_floor=71.0,
                            f0_ceil=800.0, q1=-0.15, threshold=0.85, out=None, validate=True):
        """analyze -> modify_frames -> synthesis in one library call (world_hip_resynthesize_frames_batch): x [B, L] ->
        (y [B, max(y_length)], y_length).  The curves are as in modify_frames(), over the output frames; the duration
        comes from the time map alone (synthesis runs at frame_period).  Pulses that did not fit: as resynthesize()."""
        t = self.torch
        L = self._frames_lib()
        B, Lx, xl = self._prep(x, x_len)
        fft_size = cheaptrick_fft_size(fs, 71.0)
        nf = np.array([frame_count(fs, int(n), frame_period) for n in xl], dtype=np.int32)
        keep, scale, ratio, O = self._frame_curves(B, time_map, f0_target, f0_scale, formant_shift, ap_gain)
        O = int(nf.max()) if O is None else O
        if n_out is None:
            n_out = nf if time_map is None else O
        no = np.ascontiguousarray(np.broadcast_to(n_out, (B,)), dtype=np.int32)
        if validate:
            self._validate_curves(keep, no, fft_size)
        cv = WorldHipFrameCurves(**{name: a.data_ptr() for name, a in keep.items()})
        yl = np.array([L.world_hip_resynthesis_length(int(fs), int(n), float(frame_period), 1.0) for n in no], dtype=np.int32)
        if int(yl.min()) < 1:
            raise ValueError(f"resynthesize_frames: invalid frame_period {frame_period} / n_out {no}")
        Y = int(yl.max())
        y = out if out is not None else t.zeros((B, Y), dtype=t.float64, device=x.device)
        assert y.dtype == t.float64 and y.is_contiguous() and y.shape == (B, Y) and y.device == x.device
        mods = modifications(B, scale, ratio, log_f0_target)
        hopt, copt, dopt = HarvestOption(f0_floor, f0_ceil, frame_period), CheapTrickOption(q1, 71.0, fft_size), D4COption(threshold)

        def run():
            self._check(L.world_hip_resynthesize_frames_batch(self._context(), B, int(fs), x.data_ptr(), Lx,
                                                              xl.ctypes.data_as(_ip), C.byref(hopt), C.byref(copt),
                                                              C.byref(dopt), mods, C.byref(cv), no.ctypes.data_as(_ip), O,
                                                              yl.ctypes.data_as(_ip), Y, y.data_ptr()), "resynthesize_frames")
        run()
        need = self.synthesis_pulses_dropped()          # (synchronises) -- as resynthesize(): one repeat at the asked capacity
        if need:
            if need > Y:
                raise RuntimeError(f"resynthesize_frames: {need} pitch pulses for {Y} output samples")
            self.set_synthesis_pulse_capacity(need + 16)
            try:
                run()
                if self.synthesis_pulses_dropped():
                    raise RuntimeError("resynthesize_frames: pulses dropped even at the requested capacity")
            finally:
                self.set_synthesis_pulse_capacity(0)
        return y, yl

    # ---- alignment by dynamic time warping (include/world_hip.h: world_hip_align_batch) ----
    def align(self, a, b, n_a, n_b, a_row=None, b_row=None, want_path=True):
        """Which frame of A belongs to which frame of B: a, b are float64 device tensors of frames, either dense
        [P, F, D] (pair u's frames are a[u, :n_a[u]]) or a block of records [rows, D] with a_row / b_row naming each pair's
        first row.  Both may be views that slice the columns (block[:, 3:3 + 24]: mel-cepstra without c0): the row stride
        is the tensor's own.  -> (path [P, S, 2] int32 or None, path_len [P] int32, summary [P, 3] = {D, K, MCD in dB},
        map_b [P, max n_b], map_a [P, max n_a]); map_b[u, :n_b[u]] is modify_frames' time_map with A as the source."""
        t = self.torch
        if not hasattr(self.lib, "world_hip_align_batch"):
            raise RuntimeError("this libworld_hip.so has no alignment (world_hip_align_batch)")
        na = np.ascontiguousarray(np.atleast_1d(n_a), dtype=np.int32)
        nb = np.ascontiguousarray(np.atleast_1d(n_b), dtype=np.int32)
        P = len(na)
        assert len(nb) == P and P >= 1 and int(na.min()) >= 1 and int(nb.min()) >= 1

        def rows_of(x, first, counts, name):
            assert x.dtype == t.float64 and x.device == self.device and x.dim() in (2, 3), f"{name}: float64 [P, F, D] or [rows, D] on {self.device}"
            assert x.shape[-1] >= 1 and (x.shape[-1] == 1 or x.stride(-1) == 1), f"{name}: the columns of a frame must be adjacent"
            stride = x.stride(-2) if x.shape[-2] > 1 else max(x.shape[-1], x.stride(-2))
            assert stride >= x.shape[-1], f"{name}: rows overlap"
            if x.dim() == 3:
                assert first is None and x.shape[0] == P and int(counts.max()) <= x.shape[1], f"{name}: [P, F, D] with F >= the frame counts"
                assert P == 1 or x.stride(0) % stride == 0, f"{name}: the utterances must lie whole rows apart"
                first = np.arange(P, dtype=np.int64) * ((x.stride(0) // stride) if P > 1 else 0)
            else:
                first = np.zeros(1, dtype=np.int64) if first is None and P == 1 else first
                assert first is not None, f"{name}: a block of records needs {name}_row"
                first = np.ascontiguousarray(first, dtype=np.int64)
                assert len(first) == P and int(first.min()) >= 0 and int((first + counts).max()) <= x.shape[0]
            return first, int(stride)

        ar, a_stride = rows_of(a, a_row, na, "a")
        br, b_stride = rows_of(b, b_row, nb, "b")
        assert a.shape[-1] == b.shape[-1], "a and b disagree about the number of dimensions"
        S, Ma, Mb = int((na + nb).max()) - 1, int(na.max()), int(nb.max())
        M = max(Ma, Mb)
        path = t.zeros((P, S, 2), dtype=t.int32, device=self.device) if want_path else None
        path_len = t.zeros((P,), dtype=t.int32, device=self.device)
        summary = t.zeros((P, 3), dtype=t.float64, device=self.device)
        maps = t.zeros((2, P, M), dtype=t.float64, device=self.device)
        lp = C.POINTER(C.c_longlong)
        self._check(self.lib.world_hip_align_batch(self._context(), P, int(a.shape[-1]), a.data_ptr(), ar.ctypes.data_as(lp),
                                                   na.ctypes.data_as(_ip), a_stride, b.data_ptr(), br.ctypes.data_as(lp),
                                                   nb.ctypes.data_as(_ip), b_stride, S,
                                                   path.data_ptr() if want_path else None, path_len.data_ptr(),
                                                   summary.data_ptr(), M, maps[0].data_ptr(), maps[1].data_ptr()), "align")
        return path, path_len, summary, maps[0, :, :Mb], maps[1, :, :Ma]

    # ---- morph of two aligned utterances (include/world_hip.h: world_hip_morph_batch) ----
    def _morph_lib(self):
        if not hasattr(self.lib, "world_hip_morph_batch"):
            raise RuntimeError("this libworld_hip.so has no morph (world_hip_morph_batch)")
        return self.lib

    def morph_length(self, n_a, n_b, time_rate=0.5):
        """output frames of a morph of n_a against n_b frames at time_rate (host arithmetic)"""
        n = self._morph_lib().world_hip_morph_length(int(n_a), int(n_b), float(time_rate))
        if n < 1:
            raise ValueError(f"morph_length: {n_a} x {n_b} frames at time_rate {time_rate}")
        return n

    def morph(self, a, b, n_a, n_b, fs, fft_size, path=None, path_len=None, rate=0.5, time_rate=None, f0_rate=None,
              sp_rate=None, ap_rate=None, want_positions=False, validate=True, out=None):
        """The frames between two aligned utterances.  a, b = (f0 [P, F], sp [P, F, fft/2+1], ap likewise) of A and B
        (float64, device; a member may be None on both sides), n_a / n_b their frame counts, path / path_len what align()
        returned (None: aligned frame for frame, n_a == n_b).  Rates (0 = A, 1 = B; default: `rate`): time_rate a scalar
        or one value per pair; f0_rate, sp_rate, ap_rate a scalar, one value per pair, or a curve -- a float64 device
        tensor [P, O] or [O] with one value per output frame.  -> (f0', sp', ap', n_out) with n_out[u] =
        morph_length(n_a[u], n_b[u], time_rate[u]) frames each ([P, O] / [P, O, fft/2+1], zero beyond); with
        want_positions also (pos_a, pos_b) [P, O], the source positions of every output frame.  out: an (f0', sp', ap')
        triple of the caller's to write into (frames beyond n_out are left as they are)."""
        t = self.torch
        L = self._morph_lib()
        na = np.ascontiguousarray(np.atleast_1d(n_a), dtype=np.int32)
        nb_ = np.ascontiguousarray(np.atleast_1d(n_b), dtype=np.int32)
        P = len(na)
        assert len(nb_) == P and P >= 1
        bins = fft_size // 2 + 1
        Fa = Fb = None
        for x, y, dims in zip(a, b, (2, 3, 3)):
            assert (x is None) == (y is None), "morph: give a member on both sides or on neither"
            for z in (x, y):
                if z is not None:
                    assert z.dtype == t.float64 and z.dim() == dims and z.is_contiguous() and z.device == self.device
                    assert z.shape[0] == P and (dims == 2 or z.shape[2] == bins)
            if x is not None:
                Fa, Fb = (x.shape[1] if Fa is None else Fa), (y.shape[1] if Fb is None else Fb)
                assert x.shape[1] == Fa and y.shape[1] == Fb, "morph: the arrays of one side disagree about its frames"
        assert Fa is not None, "morph: nothing to morph"
        tr = np.broadcast_to(np.asarray(rate if time_rate is None else time_rate, dtype=np.float64), (P,))
        no = np.array([L.world_hip_morph_length(int(x), int(y), float(r)) for x, y, r in zip(na, nb_, tr)], dtype=np.int32)
        if int(no.min()) < 1:
            raise ValueError("morph: frame counts below 1 or a time_rate outside [0, 1]")
        O = int(no.max())
        keep, scalars = {}, {}
        for name, v in (("f0_rate", f0_rate), ("sp_rate", sp_rate), ("ap_rate", ap_rate)):
            v = rate if v is None else v
            if t.is_tensor(v):
                assert v.dtype == t.float64 and v.device == self.device, f"{name}: a float64 tensor on {self.device}"
                v = v[None].expand(P, -1) if v.dim() == 1 else v
                assert v.dim() == 2 and v.shape[0] == P and v.shape[1] >= O, f"{name}: [P, O] or [O] with O >= {O}"
                keep["d_" + name] = v
                scalars[name] = 0.0
            else:
                scalars[name] = v
        if keep:
            O = max(O, max(v.shape[1] for v in keep.values()))
            assert all(v.shape[1] == O for v in keep.values()), "the curves disagree about the number of output frames"
            keep = {k: v.contiguous() for k, v in keep.items()}
            if validate:                                    # one reduction, one synchronisation
                live = t.arange(O, device=self.device)[None] < t.as_tensor(no, device=self.device)[:, None]
                bad = t.zeros((), dtype=t.bool, device=self.device)
                for v in keep.values():
                    bad = bad | ((~t.isfinite(v) | (v < 0) | (v > 1)) & live).any()
                if bool(bad):
                    raise ValueError("a rate curve holds a value outside [0, 1] or not finite")
        ms = morphs(P, tr, scalars["f0_rate"], scalars["sp_rate"], scalars["ap_rate"])
        cv = WorldHipMorphCurves(**{k: v.data_ptr() for k, v in keep.items()})
        if path is not None:
            assert path_len is not None and path.dtype == t.int32 and path_len.dtype == t.int32
            assert path.dim() == 3 and path.shape[0] == P and path.shape[2] == 2 and path.is_contiguous() and path_len.is_contiguous()
            assert path.device == self.device and path_len.device == self.device and path_len.shape == (P,)
        if out is not None:
            outs = tuple(out)
            for x, o in zip(a, outs):
                assert (x is None) == (o is None)
                if o is not None:
                    assert o.dtype == t.float64 and o.is_contiguous() and o.device == self.device
                    assert o.shape == (P, O) + tuple(x.shape[2:])
        else:
            outs = tuple(t.zeros((P, O) + tuple(x.shape[2:]), dtype=t.float64, device=self.device) if x is not None else None
                         for x in a)
        pos = t.zeros((2, P, O), dtype=t.float64, device=self.device) if want_positions else None
        ptr = lambda x: x.data_ptr() if x is not None else None
        self._check(L.world_hip_morph_batch(self._context(), P, int(fs), int(fft_size), na.ctypes.data_as(_ip), Fa, ptr(a[0]),
                                            ptr(a[1]), ptr(a[2]), nb_.ctypes.data_as(_ip), Fb, ptr(b[0]), ptr(b[1]), ptr(b[2]),
                                            path.shape[1] if path is not None else 0, ptr(path),
                                            ptr(path_len) if path is not None else None, ms, C.byref(cv) if keep else None, O,
                                            ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                            pos[0].data_ptr() if want_positions else None,
                                            pos[1].data_ptr() if want_positions else None), "morph")
        return (*outs, no, pos[0], pos[1]) if want_positions else (*outs, no)

    # ---- the per-frame FFT in isolation (include/world_hip.h: world_hip_probe_rfft) ----
    def probe_rfft(self, x, max_lr=3, threads=0, out=None, static_plan=False):
        """x [batch, N] float64 -> [batch, N/2+1, 2] (re, im) by csrc/fft.h's block_rfft, one workgroup per row"""
        t = self.torch
        assert x.dtype == t.float64 and x.dim() == 2 and x.is_contiguous()
        batch, N = x.shape
        lg = N.bit_length() - 1
        assert 1 << lg == N
        out = out if out is not None else t.empty((batch, N // 2 + 1, 2), dtype=t.float64, device=x.device)
        self._check(self.lib.world_hip_probe_rfft(self._context(), lg, max_lr, threads, int(static_plan), batch, x.data_ptr(),
                                                  out.data_ptr()),
                    "probe_rfft")
        return out

    def probe_irfft(self, spec, max_lr=3, threads=0, out=None, static_plan=False):
        """spec [batch, N/2+1, 2] -> [batch, N] = N * irfft (the reference's unscaled c2r) by block_irfft"""
        t = self.torch
        assert spec.dtype == t.float64 and spec.dim() == 3 and spec.is_contiguous()
        batch, N = spec.shape[0], 2 * (spec.shape[1] - 1)
        lg = N.bit_length() - 1
        assert 1 << lg == N
        out = out if out is not None else t.empty((batch, N), dtype=t.float64, device=spec.device)
        self._check(self.lib.world_hip_probe_irfft(self._context(), lg, max_lr, threads, int(static_plan), batch, spec.data_ptr(),
                                                   out.data_ptr()),
                    "probe_irfft")
        return out

    # real rows in / spectra out, spectra in / real rows out, complex rows in and out (include/world_hip.h: world_hip_probe_fft)
    PROBE_FFT_REAL_IN = (1, 3, 4, 7, 9, 10, 13, 14, 15, 16)
    PROBE_FFT_REAL_OUT = (2, 8, 11, 12)

    def probe_fft(self, mode, x, max_lr=3, threads=256, swizzle=0):
        """one composition of csrc/fft.h's entry points per row of x, one workgroup each: x [batch, N] float64 ->
        [batch, N/2+1, 2] for the r2c modes, the reverse for the c2r modes, [batch, N, 2] -> [batch, N, 2] for the
        complex ones (mode 17 reads nothing: x gives the shape)"""
        t = self.torch
        assert x.dtype == t.float64 and x.is_contiguous()
        batch = x.shape[0]
        if mode in self.PROBE_FFT_REAL_IN:
            assert x.dim() == 2
            N, shape = x.shape[1], (batch, x.shape[1] // 2 + 1, 2)
        elif mode in self.PROBE_FFT_REAL_OUT:
            assert x.dim() == 3 and x.shape[2] == 2
            N = 2 * (x.shape[1] - 1)
            shape = (batch, N)
        else:
            assert x.dim() == 3 and x.shape[2] == 2
            N, shape = x.shape[1], tuple(x.shape)
        lg = N.bit_length() - 1
        assert 1 << lg == N
        out = t.empty(shape, dtype=t.float64, device=x.device)
        self._check(self.lib.world_hip_probe_fft(self._context(), mode, lg, max_lr, threads, swizzle, batch, x.data_ptr(),
                                                 out.data_ptr()), "probe_fft")
        return out

    def probe_select(self, keys, K, mode=0):
        """D4C's band selection alone (include/world_hip.h: world_hip_probe_select): keys [rows, threads, 10] float64 ->
        [rows, 3] = the sum of all slots but the K largest, the sum of all, the route (0 one pass, 1 two, 2 general)"""
        t = self.torch
        assert keys.dtype == t.float64 and keys.is_contiguous() and keys.dim() == 3 and keys.shape[2] == 10
        out = t.empty((keys.shape[0], 3), dtype=t.float64, device=keys.device)
        self._check(self.lib.world_hip_probe_select(self._context(), mode, keys.shape[1], K, keys.shape[0], keys.data_ptr(),
                                                    out.data_ptr()), "probe_select")
        return out

    def probe_harvest_contour(self, cand, score, nfb, nc, frame_period=5.0):
        """Harvest's back half alone (include/world_hip.h: world_hip_probe_harvest_contour): cand, score [n_utt, fb_stride, maxc]
        float64 refined candidates and scores, nfb and nc sequences of n_utt ints, fb_stride = (max(nfb) + 7) & ~7 -> a dict
        of tensors: pruned_cand, pruned_score (as cand), step2, step3, step4, basic_f0 [n_utt, fb_stride], sec_n [n_utt, 2],
        sec [n_utt, 6, max(nfb) // 2 + 4] (int32), tpos, f0 [n_utt, frames] and n_frames (a list).  What the call does not
        write -- rows past nfb[u], frames past n_frames[u] -- is NaN (-1 in the int tensors)."""
        t = self.torch
        assert cand.dtype == score.dtype == t.float64 and cand.is_contiguous() and score.is_contiguous()
        assert cand.dim() == 3 and cand.shape == score.shape and len(nfb) == len(nc) == cand.shape[0]
        n, stride, maxc = cand.shape
        nfb, nc = [int(v) for v in nfb], [int(v) for v in nc]
        frames = [int((f - 1) / frame_period) + 1 for f in nfb]
        sec_cap, f_stride = max(nfb) // 2 + 4, max(max(frames), 1)
        nan = lambda *shape: t.full(shape, float("nan"), dtype=t.float64, device=cand.device)
        out = dict(pruned_cand=nan(n, stride, maxc), pruned_score=nan(n, stride, maxc), step2=nan(n, stride), step3=nan(n, stride),
                   step4=nan(n, stride), sec_n=t.full((n, 2), -1, dtype=t.int32, device=cand.device),
                   sec=t.full((n, 6, sec_cap), -1, dtype=t.int32, device=cand.device), basic_f0=nan(n, stride),
                   tpos=nan(n, f_stride), f0=nan(n, f_stride))
        ints = lambda v: (C.c_int * n)(*v)
        self._check(self.lib.world_hip_probe_harvest_contour(
            self._context(), n, ints(nfb), ints(nc), maxc, stride, cand.data_ptr(), score.data_ptr(), frame_period, f_stride,
            out["pruned_cand"].data_ptr(), out["pruned_score"].data_ptr(), out["step2"].data_ptr(), out["step3"].data_ptr(),
            out["step4"].data_ptr(), sec_cap, out["sec_n"].data_ptr(), out["sec"].data_ptr(), out["basic_f0"].data_ptr(),
            out["tpos"].data_ptr(), out["f0"].data_ptr()), "probe_harvest_contour")
        out["n_frames"] = frames
        return out

    def probe_harvest_candidates(self, nfb, band_f0, seg_events=None, seg_count=None, raw=None, afs=8000.0, f0_floor=71.0,
                                 f0_ceil=800.0, ev_cap=None, ev_group=40, stages=7):
        """Harvest's middle alone (include/world_hip.h: world_hip_probe_harvest_candidates): seg_events [n_utt, nch * 4, nseg,
        seg_cap] float64 and seg_count [n_utt, nch * 4, nseg] int32 made-up zero-crossing lists (stages 1, 2), or raw [n_utt, nch,
        fb_stride] float64 made-up raw candidates (stage 4 alone), nfb a sequence of n_utt ints, band_f0 of nch floats,
        fb_stride = (max(nfb) + 7) & ~7 -> a dict of tensors: events, ev_count (stage 1 with nseg > 1), raw, cand [n_utt,
        fb_stride, maxc], nc [n_utt] (int32).  What the call does not write is NaN (-1 in the int tensors).  ev_cap: the
        capacity of a final list (default: seg_cap with one segment list, nseg * seg_cap otherwise)."""
        t = self.torch
        nfb, band_f0 = [int(v) for v in nfb], [float(v) for v in band_f0]
        n, nch, stride = len(nfb), len(band_f0), (max(nfb) + 7) & ~7
        maxc = int(nch / 10.0 + 0.5) * 7
        dev = (seg_events if seg_events is not None else raw).device
        nan = lambda *shape: t.full(shape, float("nan"), dtype=t.float64, device=dev)
        out, nseg, seg_cap = {}, 1, 1
        if stages & 3:
            assert seg_events.dtype == t.float64 and seg_count.dtype == t.int32 and seg_events.is_contiguous() and seg_count.is_contiguous()
            assert seg_events.dim() == 4 and seg_events.shape[:3] == seg_count.shape == (n, nch * 4, seg_events.shape[2])
            nseg, seg_cap = seg_events.shape[2:]
        ev_cap = int(ev_cap) if ev_cap is not None else (seg_cap if nseg == 1 else nseg * seg_cap)
        if (stages & 1) and nseg > 1:
            out["events"], out["ev_count"] = nan(n, nch * 4, ev_cap), t.full((n, nch * 4), -1, dtype=t.int32, device=dev)
        if stages & 2:
            out["raw"] = nan(n, nch, stride)
        elif stages & 4:
            assert raw.dtype == t.float64 and raw.is_contiguous() and raw.shape == (n, nch, stride)
            out["raw"] = raw
        if stages & 4:
            out["cand"], out["nc"] = nan(n, stride, maxc), t.full((n,), -1, dtype=t.int32, device=dev)
        ptr = lambda k: out[k].data_ptr() if k in out else None
        self._check(self.lib.world_hip_probe_harvest_candidates(
            self._context(), n, (C.c_int * n)(*nfb), afs, f0_floor, f0_ceil, nch, (C.c_double * nch)(*band_f0), maxc, stride, nseg,
            seg_cap, ev_cap, ev_group, stages, seg_events.data_ptr() if stages & 3 else None,
            seg_count.data_ptr() if stages & 3 else None, ptr("events"), ptr("ev_count"), ptr("raw"), ptr("cand"), ptr("nc")),
            "probe_harvest_candidates")
        return out

    def probe_harvest_refine(self, y, y_len, cand, nfb, nc, afs=8000.0, f0_floor=71.0, f0_ceil=800.0, route=0):
        """Harvest's refinement alone (include/world_hip.h: world_hip_probe_harvest_refine): y [n_utt, y_stride] float64 the
        decimated signals, cand [n_utt, fb_stride, maxc] float64 a made-up candidate map (slots below nc[u] of frames below
        nfb[u]: 0 or a value in [f0_floor, min(f0_ceil, afs / 2)]), y_len, nfb, nc sequences of n_utt ints, fb_stride =
        (max(nfb) + 7) & ~7 -> (refined, score), tensors shaped like cand.  What the call does not write is NaN.  route: 0 a
        Harvest call's own, 1 hv_refine, 2 hv_refine_frames on the window table, 3 hv_refine_frames by rotation."""
        t = self.torch
        y_len, nfb, nc = ([int(v) for v in a] for a in (y_len, nfb, nc))
        n = len(nfb)
        assert y.dtype == t.float64 and cand.dtype == t.float64 and y.is_contiguous() and cand.is_contiguous()
        assert len(y_len) == len(nc) == n and y.dim() == 2 and y.shape[0] == n and cand.dim() == 3 and cand.shape[0] == n
        refined, score = t.full_like(cand, float("nan")), t.full_like(cand, float("nan"))
        ints = lambda v: (C.c_int * n)(*v)
        self._check(self.lib.world_hip_probe_harvest_refine(
            self._context(), n, ints(y_len), ints(nfb), ints(nc), afs, f0_floor, f0_ceil, cand.shape[2], cand.shape[1], y.shape[1],
            route, y.data_ptr(), cand.data_ptr(), refined.data_ptr(), score.data_ptr()), "probe_harvest_refine")
        return refined, score

    # ---- multi-GPU exchange records (include/world_hip.h: world_hip_pack_results) ----
    def capture(self, fn):
        """Run fn() -- batched calls of this object on torch's current stream, on preallocated tensors, shapes that ran before --
        inside a HIP graph capture; returns a Graph whose launch() replays all of it with one host call."""
        ctx = self._context()
        self._check(self.lib.world_hip_graph_begin(ctx), "graph_begin")
        g = C.c_void_p()
        try:
            fn()
        except BaseException:
            # the capture must be ended whatever fn() did; a graph it still produced is destroyed, not leaked
            if self.lib.world_hip_graph_end(ctx, C.byref(g)) == 0 and g:
                self.lib.world_hip_graph_destroy(g)
            raise
        self._check(self.lib.world_hip_graph_end(ctx, C.byref(g)), "graph_end")
        return Graph(self, ctx, g)

    def analyze_packed(self, x, fs, block, first_row=0, x_len=None, frame_period=5.0, f0_floor=71.0, f0_ceil=800.0,
                       q1=-0.15, threshold=0.85, fft_size=None):
        """Harvest -> CheapTrick -> D4C of one batch written straight into packed records (no dense sp / ap, no pack
        pass): utterance u's n_frames[u] records start at block[first_row + sum(n_frames[:u])].  Returns n_frames."""
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        fft_size = fft_size or cheaptrick_fft_size(fs, 71.0)
        nb = fft_size // 2 + 1
        nf = [frame_count(fs, int(n), frame_period) for n in xl]
        cols = block.shape[-1]                       # 2 + 2 nb: f64 records; 2 + nb: the spectra as float32 (narrow wire)
        assert block.dtype == t.float64 and block.is_contiguous() and cols in (2 + 2 * nb, 2 + nb) and block.device == x.device
        assert first_row >= 0 and first_row + sum(nf) <= block.shape[0]
        hopt, copt, dopt = HarvestOption(f0_floor, f0_ceil, frame_period), CheapTrickOption(q1, 71.0, fft_size), D4COption(threshold)
        self._check(self.lib.world_hip_analyze_packed(self._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(_ip),
                                                      C.byref(hopt), C.byref(copt), C.byref(dopt), first_row,
                                                      block.data_ptr(), cols), "analyze_packed")
        return nf

    def analyze_coded(self, x, fs, block, first_row=0, x_len=None, frame_period=5.0, f0_floor=71.0, f0_ceil=800.0,
                      q1=-0.15, threshold=0.85, number_of_dimensions=60, fft_size=None):
        """Harvest -> CheapTrick -> D4C of one batch written as CODED records [tpos, f0, mel-cepstrum[D], band
        aperiodicity[nap]] (include/world_hip.h: world_hip_analyze_coded -- the reference's CodeSpectralEnvelope /
        CodeAperiodicity of the analysis, 31 x fewer bytes per frame at 48 kHz).  Returns n_frames."""
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        fft_size = fft_size or cheaptrick_fft_size(fs, 71.0)
        nf = [frame_count(fs, int(n), frame_period) for n in xl]
        cols = block.shape[-1]
        assert block.dtype == t.float64 and block.is_contiguous() and block.device == x.device
        assert cols == self.lib.world_hip_coded_columns(fs, number_of_dimensions), (cols, fs, number_of_dimensions)
        assert first_row >= 0 and first_row + sum(nf) <= block.shape[0]
        hopt, copt, dopt = HarvestOption(f0_floor, f0_ceil, frame_period), CheapTrickOption(q1, 71.0, fft_size), D4COption(threshold)
        self._check(self.lib.world_hip_analyze_coded(self._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(_ip),
                                                     C.byref(hopt), C.byref(copt), C.byref(dopt), number_of_dimensions,
                                                     first_row, block.data_ptr(), cols), "analyze_coded")
        return nf

    def spectral_packed_range(self, x, fs, tpos, f0, n_frames, block, frame_lo, frame_hi, first_row=0, x_len=None, q1=-0.15,
                              threshold=0.85, reuse_offsets=False):
        """CheapTrick + D4C of frames [frame_lo, frame_hi) of every utterance, given F0, straight into packed records
        (include/world_hip.h: world_hip_spectral_packed_range): bit-identical to the same rows of a whole-utterance call.
        reuse_offsets: an earlier call on this context had the same inputs and only another range -- its offset scans and
        LoveTrain pass are reused (the library checks that they are still there and were made for these buffers).
        Returns the number of records written."""
        t = self.torch
        B, L, xl = self._prep(x, x_len)
        fft_size = cheaptrick_fft_size(fs, 71.0)
        nb = fft_size // 2 + 1
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        F = tpos.shape[1]
        cols = block.shape[-1]
        rows = int(sum(min(frame_hi, int(n)) - min(frame_lo, int(n)) for n in nf))
        assert block.dtype == t.float64 and block.is_contiguous() and cols in (2 + 2 * nb, 2 + nb) and block.device == x.device
        assert tpos.is_contiguous() and f0.is_contiguous() and tpos.shape == f0.shape == (B, F)
        assert 0 <= frame_lo <= frame_hi and first_row >= 0 and first_row + rows <= block.shape[0]
        copt, dopt = CheapTrickOption(q1, 71.0, fft_size), D4COption(threshold)
        self._check(self.lib.world_hip_spectral_packed_range(self._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(_ip),
                                                             nf.ctypes.data_as(_ip), F, tpos.data_ptr(), f0.data_ptr(),
                                                             C.byref(copt), C.byref(dopt), frame_lo, frame_hi,
                                                             1 if reuse_offsets else 0, first_row, block.data_ptr(), cols),
                    "spectral_packed_range")
        return rows

    def pack_results(self, tpos, f0, sp, ap, n_frames, block, first_row=0):
        """valid frames of a batched analysis -> records [tpos, f0, sp row, ap row] in block[first_row:] (device)"""
        t = self.torch
        B, F = f0.shape
        nb = sp.shape[-1]
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        assert block.dtype == t.float64 and block.is_contiguous() and block.shape[-1] == 2 + 2 * nb
        assert first_row + int(nf.sum()) <= block.shape[0]
        assert all(a.is_contiguous() and a.dtype == t.float64 for a in (tpos, f0, sp, ap))
        self._check(self.lib.world_hip_pack_results(self._context(), B, nf.ctypes.data_as(_ip), F, nb, tpos.data_ptr(),
                                                    f0.data_ptr(), sp.data_ptr(), ap.data_ptr(), first_row,
                                                    block.data_ptr()), "pack_results")
        return block

    def unpack_results(self, block, n_frames, first_row=0):
        """the inverse: (tpos [B, F], f0 [B, F], sp [B, F, nb], ap [B, F, nb]) padded to the longest utterance"""
        t = self.torch
        nf = np.ascontiguousarray(n_frames, dtype=np.int32)
        B, F, nb = len(nf), int(nf.max()), (block.shape[-1] - 2) // 2
        tpos = t.zeros((B, F), dtype=t.float64, device=block.device)
        f0 = t.zeros_like(tpos)
        sp = t.zeros((B, F, nb), dtype=t.float64, device=block.device)
        ap = t.zeros_like(sp)
        self._check(self.lib.world_hip_unpack_results(self._context(), B, nf.ctypes.data_as(_ip), F, nb, block.data_ptr(),
                                                      first_row, tpos.data_ptr(), f0.data_ptr(), sp.data_ptr(),
                                                      ap.data_ptr()), "unpack_results")
        return tpos, f0, sp, ap

    def realtime(self, n_streams, fs, frame_period, fft_size, buffer_size, number_of_pointers):
        """n_streams real-time synthesisers (reference synthesisrealtime.cpp) on this GPU: see RealtimeStreams"""
        if not hasattr(self.lib, "world_hip_realtime_create"):
            raise RuntimeError("this libworld_hip.so has no real-time synthesis (world_hip_realtime_create)")
        rt = RealtimeStreams(self, n_streams, fs, frame_period, fft_size, buffer_size, number_of_pointers)
        self._realtime.add(rt)
        return rt

    def synthesis_pulses_dropped(self):
        """pulses per utterance the last synthesis calls had no room for (0 = all rendered); synchronises"""
        need = C.c_int(0)
        self._check(self.lib.world_hip_synthesis_pulses_dropped(self._context(), C.byref(need)), "synthesis_pulses_dropped")
        return need.value

    def set_synthesis_pulse_capacity(self, pulses_per_utterance):
        self._check(self.lib.world_hip_set_synthesis_pulse_capacity(self._context(), int(pulses_per_utterance)),
                    "set_synthesis_pulse_capacity")

    # ---- sampling-rate conversion (include/world_hip.h: world_hip_resample_batch) ----
    def resample(self, x, fs_in, fs_out, x_len=None, quality="best", out=None):
        """x [B, L] float64 on the device at fs_in -> (y [B, max(y_len)], y_len) at fs_out, y_len[u] =
        resample_length(x_len[u], fs_in, fs_out); zero beyond y_len.  quality: "best", "fast" or a (zeros, rolloff,
        kaiser_beta) triple.  Equal rates copy.  out: a [B, >= max(y_len)] tensor of the caller's to write into (samples
        beyond y_len are left as they are)."""
        t = self.torch
        if not hasattr(self.lib, "world_hip_resample_batch"):
            raise RuntimeError("this libworld_hip.so has no resampler (world_hip_resample_batch)")
        opt = resample_option(quality)
        B, L, xl = self._prep(x, x_len)
        if int(fs_in) < 1 or int(fs_out) < 1 or (B and int(xl.min()) < 1):
            raise ValueError(f"resample: {fs_in} -> {fs_out} Hz, lengths {xl.tolist()}")
        y_len = np.array([resample_length(n, fs_in, fs_out) for n in xl], dtype=np.int32)
        if out is None:
            out = t.zeros((B, int(y_len.max())), dtype=t.float64, device=x.device)
        assert out.dtype == t.float64 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == B and out.device == x.device
        self._check(self.lib.world_hip_resample_batch(self._context(), B, int(fs_in), int(fs_out), C.byref(opt), x.data_ptr(), L,
                                                      xl.ctypes.data_as(_ip), out.data_ptr(), out.shape[1]), "resample")
        return out, y_len

    def pcm16_to_double(self, pcm):
        """int16 samples (any shape) -> float64 / 32768, wavread()'s convention, on the device"""
        t = self.torch
        assert pcm.dtype == t.int16
        pcm = pcm.contiguous()
        x = t.empty(pcm.shape, dtype=t.float64, device=pcm.device)
        self._check(self.lib.world_hip_pcm16_to_double(self._context(), pcm.numel(), pcm.data_ptr(), x.data_ptr()),
                    "pcm16_to_double")
        return x

    def pcm_to_double(self, pcm_bytes, nbit):
        """uint8 tensor holding a WAV file's sample bytes (nbit/8 per sample, little endian) ->
        float64 samples exactly as wavread() decodes them, on the device"""
        t = self.torch
        assert pcm_bytes.dtype == t.uint8 and pcm_bytes.dim() == 1 and nbit // 8 >= 1
        pcm_bytes = pcm_bytes.contiguous()
        n = pcm_bytes.numel() // (nbit // 8)
        x = t.empty(n, dtype=t.float64, device=pcm_bytes.device)
        self._check(self.lib.world_hip_pcm_to_double(self._context(), n, nbit, pcm_bytes.data_ptr(), x.data_ptr()),
                    "pcm_to_double")
        return x

    def double_to_pcm16(self, x):
        """float64 samples -> the int16 values wavwrite() stores, on the device"""
        t = self.torch
        assert x.dtype == t.float64
        x = x.contiguous()
        q = t.empty(x.shape, dtype=t.int16, device=x.device)
        self._check(self.lib.world_hip_double_to_pcm16(self._context(), x.numel(), x.data_ptr(), q.data_ptr()),
                    "double_to_pcm16")
        return q

    def wav_layout(self, path):
        """Host-side header parse: (fs, nbit, samples, byte offset of the samples); raises where wavread() refuses."""
        fs, nbit, n, off = C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
        rc = self.lib.world_hip_wav_layout(os.fsencode(path), C.byref(fs), C.byref(nbit), C.byref(n), C.byref(off))
        if rc != 1:
            raise OSError(f"{path}: " + ("cannot be opened" if rc == 0 else "not a mono PCM WAV file"))
        return fs.value, nbit.value, n.value, off.value

    def wavread(self, path):
        """A WAV file -> (x on the device, fs): only the file's own bytes cross PCIe."""
        fs, nbit, n, off = self.wav_layout(path)
        raw = np.fromfile(path, dtype=np.uint8, offset=off, count=n * (nbit // 8))
        if raw.size != n * (nbit // 8):
            raise OSError(f"{path}: shorter than its header says")
        return self.pcm_to_double(self.torch.from_numpy(raw).to(self.device), nbit), fs

    def wavwrite(self, path, x, fs):
        """float64 samples on the device -> a 16-bit WAV file as wavwrite() would store them
        (quantised on the device; int16 crosses PCIe)."""
        q = self.double_to_pcm16(x.reshape(-1)).cpu().numpy()
        if self.lib.world_hip_wav_write_pcm16(os.fsencode(path), fs, q.size, q.ctypes.data) != 1:
            raise OSError(f"{path}: cannot be written")

    # ---- coders (reference codec.h): dense [..., cols] tensors, leading dims are rows ----
    def _codec(self, fn, what, src, fs, fft_size, out_cols, *dims):
        t = self.torch
        src = src.contiguous()
        rows = int(src.numel() // src.shape[-1])
        out = t.empty(tuple(src.shape[:-1]) + (out_cols,), dtype=t.float64, device=src.device)
        self._check(fn(self._context(), rows, fs, fft_size, *dims, src.data_ptr(), out.data_ptr()), what)
        return out

    def code_spectral_envelope(self, sp, fs, fft_size, number_of_dimensions):
        return self._codec(self.lib.world_hip_code_spectral_envelope, "code_spectral_envelope", sp, fs, fft_size,
                           number_of_dimensions, number_of_dimensions)

    def decode_spectral_envelope(self, coded, fs, fft_size):
        return self._codec(self.lib.world_hip_decode_spectral_envelope, "decode_spectral_envelope", coded, fs,
                           fft_size, fft_size // 2 + 1, int(coded.shape[-1]))

    def code_aperiodicity(self, ap, fs, fft_size):
        return self._codec(self.lib.world_hip_code_aperiodicity, "code_aperiodicity", ap, fs, fft_size,
                           self.lib.GetNumberOfAperiodicities(fs))

    def decode_aperiodicity(self, coded, fs, fft_size):
        return self._codec(self.lib.world_hip_decode_aperiodicity, "decode_aperiodicity", coded, fs, fft_size,
                           fft_size // 2 + 1)

    # ---- all-pass mel-cepstra (include/world_hip.h: world_hip_sp2mc / world_hip_mc2sp) ----
    def mcep_alpha(self, fs):
        """the all-pass constant whose warp lies closest to the mel scale at fs (0.41 at 16 kHz, 0.554 at 48 kHz)"""
        if not hasattr(self.lib, "world_hip_sp2mc"):
            raise RuntimeError("this libworld_hip.so has no mel-cepstrum (world_hip_sp2mc)")
        if int(fs) < 1:
            raise ValueError(f"mcep_alpha: fs {fs}")
        return float(self.lib.world_hip_mcep_alpha(int(fs)))

    def _mcep_rows(self, x, cols, row_stride, rows, what):
        """(rows, stride in doubles, leading shape) of the rows of `cols` doubles in x: a dense [..., cols] tensor, a 2-D
        view whose rows lie further apart (x.stride(0)), or -- row_stride given -- any tensor that starts at the first
        row's first double and reaches the last row's last"""
        t = self.torch
        assert x.dtype == t.float64 and x.is_cuda and x.device == self.device, f"{what}: float64 on {self.device}"
        if row_stride is not None:
            if rows is None:
                raise ValueError(f"{what}: row_stride needs rows")
            assert x.is_contiguous() and x.numel() >= (int(rows) - 1) * int(row_stride) + cols, f"{what}: the tensor ends before the last row"
            return int(rows), int(row_stride), (int(rows),)
        assert x.shape[-1] == cols and x.stride(-1) == 1, f"{what}: [..., {cols}] with adjacent columns"
        if x.dim() == 2 and not x.is_contiguous():
            return int(x.shape[0]), int(x.stride(0)), (int(x.shape[0]),)
        assert x.is_contiguous(), f"{what}: dense, or a 2-D view with a row stride"
        return int(x.numel() // cols), cols, tuple(x.shape[:-1])

    def _mcep(self, decode, src, in_cols, out_cols, fft_size, order, alpha, out, row_stride, rows):
        t = self.torch
        what = "mc2sp" if decode else "sp2mc"
        if not hasattr(self.lib, "world_hip_sp2mc"):
            raise RuntimeError("this libworld_hip.so has no mel-cepstrum (world_hip_sp2mc)")
        n, in_stride, lead = self._mcep_rows(src, in_cols, row_stride, rows, what)
        ret = out
        if out is None:
            out = ret = t.empty(lead + (out_cols,), dtype=t.float64, device=src.device)
            out_stride = out_cols
        else:
            assert out.dtype == t.float64 and out.device == src.device and out.dim() == 2 and out.shape[0] == n and \
                out.shape[1] >= out_cols and out.stride(1) == 1, f"{what}: out must be [{n}, >= {out_cols}] float64 with adjacent columns"
            out_stride = int(out.stride(0)) if n > 1 else max(int(out.stride(0)), out_cols)
        fn = self.lib.world_hip_mc2sp if decode else self.lib.world_hip_sp2mc
        self._check(fn(self._context(), n, int(fft_size), int(order), float(alpha), src.data_ptr(), in_stride, out.data_ptr(),
                       out_stride), what)
        return ret

    def sp2mc(self, sp, order, alpha, out=None, row_stride=None, rows=None, fft_size=None):
        """envelope rows -> mel-cepstra c_0 .. c_order by all-pass warping (SPTK's freqt of the cepstrum of ln sp).
        sp: [..., fft_size / 2 + 1] float64 on the device; a 2-D view with a larger row stride (block[:, 2:2 + K] of packed
        records) is read where it lies.  row_stride (with rows and fft_size): sp is any tensor starting at the first
        envelope.  out: a [rows, >= order + 1] tensor or view of the caller's (columns beyond order + 1 are left alone).
        Returns [..., order + 1], or out."""
        if fft_size is None:
            fft_size = 2 * (int(sp.shape[-1]) - 1)
        return self._mcep(False, sp, int(fft_size) // 2 + 1, int(order) + 1, fft_size, order, alpha, out, row_stride, rows)

    def mc2sp(self, mc, alpha, fft_size, out=None, row_stride=None, rows=None, order=None):
        """mel-cepstra -> envelope rows [..., fft_size / 2 + 1]: sp = |exp sum mc_m z~^-m|^2.  mc: [..., order + 1], a 2-D
        view with a larger row stride, or -- row_stride with rows and order -- any tensor starting at the first c_0."""
        if order is None:
            order = int(mc.shape[-1]) - 1
        return self._mcep(True, mc, int(order) + 1, int(fft_size) // 2 + 1, fft_size, order, alpha, out, row_stride, rows)

    # ---- dynamic features and parameter generation (include/world_hip.h: world_hip_delta_batch / world_hip_mlpg_batch) ----
    DEFAULT_WINDOWS = ((0.0, 1.0, 0.0), (-0.5, 0.0, 0.5), (1.0, -2.0, 1.0))

    @staticmethod
    def _windows(windows):
        """windows -> (float64 [n_win][2 L + 1], L): sequences of odd length, the shorter ones padded with zeros"""
        rows = [np.asarray(w, dtype=np.float64).reshape(-1) for w in (WorldHip.DEFAULT_WINDOWS if windows is None else windows)]
        if not rows or any(len(r) % 2 == 0 for r in rows):
            raise ValueError("windows: at least one, each of odd length")
        half = max(len(r) // 2 for r in rows)
        win = np.zeros((len(rows), 2 * half + 1), dtype=np.float64)
        for w, r in enumerate(rows):
            win[w, half - len(r) // 2:half + len(r) // 2 + 1] = r
        return win, half

    def _frames3(self, x, what):
        """[T][cols] or [U][T][cols] float64 on the device with adjacent columns -> the [U][T][cols] view"""
        t = self.torch
        assert x.dtype == t.float64 and x.is_cuda and x.device == self.device and x.dim() in (2, 3), f"{what}: [U][T][cols] float64 on {self.device}"
        x3 = x[None] if x.dim() == 2 else x
        assert x3.shape[2] == 1 or x3.stride(2) == 1, f"{what}: adjacent columns"
        return x3

    def _mlpg_call(self, generate, x, var, windows, mask, n_frames, precision, fill, out):
        t = self.torch
        what = "mlpg" if generate else "deltas"
        if not hasattr(self.lib, "world_hip_mlpg_batch"):
            raise RuntimeError("this libworld_hip.so has no parameter generation (world_hip_mlpg_batch)")
        win, half = self._windows(windows)
        n_win = win.shape[0]
        x3 = self._frames3(x, what)
        U, T, cols = (int(v) for v in x3.shape)
        if generate:
            if cols % n_win:
                raise ValueError(f"mlpg: {cols} columns are no multiple of the {n_win} windows")
            dim, out_cols = cols // n_win, cols // n_win
        else:
            dim, out_cols = cols, cols * n_win
        nf = np.full(U, T, dtype=np.int32) if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32).reshape(-1)
        if nf.shape != (U,) or (nf.size and int(nf.max()) > T):
            raise ValueError(f"{what}: n_frames must be {U} counts of at most {T}")
        m_ptr, m_us = None, 0
        if mask is not None:
            assert mask.device == x.device and mask.dtype in (t.bool, t.uint8), f"{what}: mask must be bool or uint8 on the device"
            m3 = mask[None] if mask.dim() == 1 else mask
            assert tuple(m3.shape) == (U, T) and (T == 1 or m3.stride(1) == 1), f"{what}: mask must be [{U}][{T}] with adjacent frames"
            m_ptr, m_us = m3.data_ptr(), int(m3.stride(0))
        v_ptr, v_us, v_rs = None, 0, 0
        if generate:
            assert var.dtype == t.float64 and var.device == x.device and var.shape[-1] == cols and \
                (cols == 1 or var.stride(-1) == 1), f"mlpg: var must be [..., {cols}] float64 with adjacent columns"
            if var.dim() == 1:                                       # one global row
                var = var[None, None]
            elif var.dim() == 2:                                     # one utterance's rows, or one row per utterance
                var = var[None] if x.dim() == 2 else var[:, None]
            assert var.dim() == 3 and var.shape[0] in (1, U) and var.shape[1] in (1, T), \
                f"mlpg: var must be [{U} or 1][{T} or 1][{cols}], [{U}][{cols}] or [{cols}]"
            v_ptr = var.data_ptr()
            v_us = int(var.stride(0)) if var.shape[0] > 1 else 0
            v_rs = int(var.stride(1)) if var.shape[1] > 1 else 0
        ret = out
        if out is None:
            out = t.empty((U, T, out_cols), dtype=t.float64, device=x.device)
            ret = out[0] if x.dim() == 2 else out
        o3 = self._frames3(out, what)
        assert tuple(o3.shape) == (U, T, out_cols), f"{what}: out must be [{U}][{T}][{out_cols}]"
        rs = lambda a, c: int(a.stride(1)) if a.shape[1] > 1 else max(int(a.stride(1)), c)
        us = lambda a: int(a.stride(0)) if a.shape[0] > 1 else 0
        if generate:
            rc = self.lib.world_hip_mlpg_batch(self._context(), U, dim, n_win, half, win.ctypes.data, nf.ctypes.data_as(_ip), m_ptr, m_us, x3.data_ptr(),
                                               us(x3), rs(x3, cols), v_ptr, v_us, v_rs, int(bool(precision)), float(fill),
                                               o3.data_ptr(), us(o3), rs(o3, out_cols))
        else:
            rc = self.lib.world_hip_delta_batch(self._context(), U, dim, n_win, half, win.ctypes.data, nf.ctypes.data_as(_ip), m_ptr, m_us,
                                                x3.data_ptr(), us(x3), rs(x3, cols), float(fill), o3.data_ptr(), us(o3),
                                                rs(o3, out_cols))
        self._check(rc, what)
        return ret

    def deltas(self, x, windows=None, mask=None, fill=0.0, n_frames=None, out=None):
        """statics -> [static, delta, delta-delta, ...]: x [U][T][D] (or [T][D]) float64 on the device, strides honoured;
        windows: sequences of odd length, the first the identity (default: [1], [-0.5 0 0.5], [1 -2 1]); mask [U][T] bool or
        uint8 marks the frames that exist (windows are truncated at the ends of every run), masked frames get `fill`;
        n_frames: per-utterance lengths (host).  Returns [U][T][n_win D] (or [T][n_win D]), or out."""
        return self._mlpg_call(False, x, None, windows, mask, n_frames, False, fill, out)

    def mlpg(self, mean, var, windows=None, mask=None, precision=False, fill=0.0, n_frames=None, out=None):
        """the maximum-likelihood static trajectory under predicted static / delta / delta-delta means and variances:
        mean [U][T][n_win D] (or [T][n_win D]); var of the same shape, [U][1][n_win D] or [U][n_win D] (one row per
        utterance) or [n_win D] (one global row); precision=True: var holds 1 / variance.  Returns [U][T][D] (or [T][D])."""
        return self._mlpg_call(True, mean, var, windows, mask, n_frames, precision, fill, out)

    # ---- joint-density Gaussian mixture (include/world_hip.h: world_hip_gmm_*) ----
    GMM_MODES = {"mixture": 0, "hard": 1}

    def _gmm_lib(self):
        if not hasattr(self.lib, "world_hip_gmm_convert"):
            raise RuntimeError("this libworld_hip.so has no Gaussian mixture (world_hip_gmm_convert)")
        return self.lib

    def _gmm_rows(self, x, cols, what):
        """a [rows][cols] float64 tensor or view on the device with adjacent columns -> (rows, row stride in doubles)"""
        t = self.torch
        assert x.dtype == t.float64 and x.is_cuda and x.device == self.device and x.dim() == 2 and x.shape[1] == cols and \
            (cols == 1 or x.stride(1) == 1), f"{what}: [rows][{cols}] float64 on {self.device} with adjacent columns"
        rows = int(x.shape[0])
        return rows, (int(x.stride(0)) if rows > 1 else max(int(x.stride(0)), cols))

    def gmm_prepare(self, w, mu, cov, dx):
        """host parameters w [M], mu [M][P], cov [M][P][P] (the lower triangle is read) and the source dimension dx -> the
        prepared model on the device (a GmmModel: .M, .dx, .dy, .data).  Host arithmetic and one copy."""
        lib = self._gmm_lib()
        w, mu, cov = _f64(w), _f64(mu), _f64(cov)
        M, P = (int(v) for v in mu.shape)
        dx = int(dx)
        if w.shape != (M,) or cov.shape != (M, P, P) or not 1 <= dx <= P:
            raise ValueError(f"gmm_prepare: w [{M}], mu [{M}][{P}], cov [{M}][{P}][{P}] and 1 <= dx <= {P}")
        n = int(lib.world_hip_gmm_model_doubles(M, dx, P - dx))
        if n < 0:
            raise RuntimeError("gmm_prepare: " + lib.world_hip_last_error().decode())
        host = np.empty(n, dtype=np.float64)
        self._check(lib.world_hip_gmm_prepare(M, dx, P - dx, w.ctypes.data, mu.ctypes.data, cov.ctypes.data, host.ctypes.data), "gmm_prepare")
        with self.torch.cuda.device(self.device):
            return GmmModel(M, dx, P - dx, self.torch.from_numpy(host).to(self.device))

    def _gmm_convert(self, model, x, mode, mean, var, post, loglik):
        rows, x_rs = self._gmm_rows(x, model.dx, "gmm: x")
        ptr = lambda a: None if a is None else a.data_ptr()
        rs = lambda a, c: 0 if a is None else self._gmm_rows(a, c, "gmm: out")[1]
        for a, c in ((mean, model.dy), (var, model.dy), (post, model.M)):
            assert a is None or a.shape[0] == rows, f"gmm: an output of {rows} rows"
        assert loglik is None or (loglik.dtype == self.torch.float64 and loglik.is_contiguous() and tuple(loglik.shape) == (rows,))
        self._check(self.lib.world_hip_gmm_convert(self._context(), model.M, model.dx, model.dy, model.data.data_ptr(), rows, x.data_ptr(), x_rs,
                                                   mode, ptr(mean), rs(mean, model.dy), ptr(var), rs(var, model.dy), ptr(post),
                                                   rs(post, model.M), ptr(loglik)), "gmm_convert")

    def gmm_convert(self, model, x, mode="mixture", out=None):
        """source rows x [rows][dx] (float64 on the device; a view with a row stride is read where it lies) -> the per-row
        (mean, var) [rows][dy] of the target under the model: mode "mixture" moment-matches the conditional mixture,
        "hard" takes the most likely component.  out: a (mean, var) pair of [rows][dy] tensors or views of the caller's.
        With x = [static, delta, ...] features the pair is what mlpg() consumes."""
        self._gmm_lib()
        if mode not in self.GMM_MODES:
            raise ValueError(f"gmm_convert: mode {mode!r} is neither 'mixture' nor 'hard'")
        if model.dy == 0:
            raise ValueError("gmm_convert: the model has no target part")
        t = self.torch
        if out is None:
            out = tuple(t.empty((int(x.shape[0]), model.dy), dtype=t.float64, device=x.device) for _ in range(2))
        mean, var = out
        self._gmm_convert(model, x, self.GMM_MODES[mode], mean, var, None, None)
        return mean, var

    def gmm_posterior(self, model, x):
        """-> (the responsibilities [rows][M], the log-likelihood [rows]) of the rows' source part under the model"""
        self._gmm_lib()
        t = self.torch
        rows = int(x.shape[0])
        post, loglik = t.empty((rows, model.M), dtype=t.float64, device=x.device), t.empty(rows, dtype=t.float64, device=x.device)
        self._gmm_convert(model, x, 0, None, None, post, loglik)
        return post, loglik

    def gmm_fit(self, z, n_mix, n_iter=20, reg=1e-6, init=None):
        """EM for a full-covariance mixture of n_mix components on the rows z [rows][P] (float64 on the device, strides
        honoured).  init: a (w, mu, cov) start (host arrays); None: world_hip_gmm_init's (means spread over the rows, the
        data's diagonal variance).  Returns host arrays (w [M], mu [M][P], cov [M][P][P], loglik [n_iter]: the mean
        log-likelihood before each update).  Waits for the device every iteration."""
        lib = self._gmm_lib()
        M = int(n_mix)
        rows, z_rs = self._gmm_rows(z, int(z.shape[1]), "gmm_fit: z")
        P = int(z.shape[1])
        if init is None:
            w, mu, cov = np.empty(M), np.empty((M, P)), np.empty((M, P, P))
            self._check(lib.world_hip_gmm_init(self._context(), M, P, rows, z.data_ptr(), z_rs, w.ctypes.data, mu.ctypes.data, cov.ctypes.data), "gmm_init")
        else:
            w, mu, cov = (np.array(a, dtype=np.float64, order="C") for a in init)
            if w.shape != (M,) or mu.shape != (M, P) or cov.shape != (M, P, P):
                raise ValueError(f"gmm_fit: init must be w [{M}], mu [{M}][{P}], cov [{M}][{P}][{P}]")
        loglik = np.empty(int(n_iter), dtype=np.float64)
        self._check(lib.world_hip_gmm_fit(self._context(), M, P, rows, z.data_ptr(), z_rs, int(n_iter), float(reg), w.ctypes.data, mu.ctypes.data,
                                          cov.ctypes.data, loglik.ctypes.data), "gmm_fit")
        return w, mu, cov, loglik

    # ---- training rows of a corpus (include/world_hip.h: world_hip_frame_power_batch .. world_hip_joint_rows_batch) ----
    def _corpus_lib(self):
        if not hasattr(self.lib, "world_hip_joint_rows_batch"):
            raise RuntimeError("this libworld_hip.so has no corpus stage (world_hip_joint_rows_batch)")
        return self.lib

    @staticmethod
    def _counts(n, U, most, what):
        nf = np.full(U, most, dtype=np.int32) if n is None else np.ascontiguousarray(np.atleast_1d(n), dtype=np.int32).reshape(-1)
        if nf.shape != (U,) or (nf.size and int(nf.max()) > most):
            raise ValueError(f"{what}: {U} counts of at most {most}")
        return nf

    @staticmethod
    def _stride(a, axis, least):
        """the stride of an axis, or `least` where the axis has one entry (its stride then means nothing)"""
        return int(a.stride(axis)) if a.shape[axis] > 1 else least

    def frame_power(self, sp, n_frames=None):
        """envelope rows sp [U][T][fft_size / 2 + 1] (or [T][bins]; float64 on the device, strides honoured) -> (power [U][T],
        mean [U]): each frame's mean spectral power and its mean over the utterance's n_frames[u] frames (entries beyond
        are 0).  A 2-D input gives power [T] and a 0-dim mean."""
        lib, t = self._corpus_lib(), self.torch
        x3 = self._frames3(sp, "frame_power")
        U, T, bins = (int(v) for v in x3.shape)
        nf = self._counts(n_frames, U, T, "frame_power: n_frames")
        power, mean = t.zeros((U, T), dtype=t.float64, device=sp.device), t.zeros(U, dtype=t.float64, device=sp.device)
        self._check(lib.world_hip_frame_power_batch(self._context(), U, 2 * (bins - 1), nf.ctypes.data_as(_ip), x3.data_ptr(),
                                                    self._stride(x3, 0, 0), self._stride(x3, 1, bins), power.data_ptr(), T, mean.data_ptr()),
                    "frame_power")
        return (power[0], mean[0]) if sp.dim() == 2 else (power, mean)

    def select_frames(self, values, n_frames, threshold, scale=None, mask=None):
        """the frames with mask != 0 and values >= threshold * scale[u]: values [U][T] (or [T]) float64 on the device, any
        strides (a column of a record is read where it lies); scale [U] float64 on the device or None; mask [U][T] bool or
        uint8.  -> (index [U][T] int32: the kept frames' numbers, ascending, in the first count[u] entries; count [U] int32;
        keep [U][T] uint8, the mask deltas() and mlpg() read).  Entries beyond are 0."""
        lib, t = self._corpus_lib(), self.torch
        assert values.dtype == t.float64 and values.device == self.device and values.dim() in (1, 2), f"select_frames: [U][T] float64 on {self.device}"
        v2 = values[None] if values.dim() == 1 else values
        U, T = (int(v) for v in v2.shape)
        nf = self._counts(n_frames, U, T, "select_frames: n_frames")
        s_ptr = None
        if scale is not None:
            scale = scale.reshape(-1)
            assert scale.dtype == t.float64 and scale.device == self.device and scale.is_contiguous() and scale.numel() == U, f"select_frames: scale [{U}] float64"
            s_ptr = scale.data_ptr()
        m_ptr, m_us = None, 0
        if mask is not None:
            assert mask.device == self.device and mask.dtype in (t.bool, t.uint8), "select_frames: mask must be bool or uint8 on the device"
            m2 = mask[None] if mask.dim() == 1 else mask
            assert tuple(m2.shape) == (U, T) and (T == 1 or m2.stride(1) == 1), f"select_frames: mask must be [{U}][{T}] with adjacent frames"
            m_ptr, m_us = m2.data_ptr(), self._stride(m2, 0, 0)
        index, count = t.zeros((U, T), dtype=t.int32, device=self.device), t.zeros(U, dtype=t.int32, device=self.device)
        keep = t.zeros((U, T), dtype=t.uint8, device=self.device)
        self._check(lib.world_hip_select_frames_batch(self._context(), U, nf.ctypes.data_as(_ip), v2.data_ptr(), self._stride(v2, 0, 0),
                                                      self._stride(v2, 1, 1), float(threshold), s_ptr, m_ptr, m_us, index.data_ptr(), T,
                                                      count.data_ptr(), keep.data_ptr(), T), "select_frames")
        return (index[0], count, keep[0]) if values.dim() == 1 else (index, count, keep)

    def gather_rows(self, x, index, n_out, fill=0.0, out=None, n_src=None):
        """out[u][i] = x[u][index[u][i]] for i < n_out[u] (host counts): x [U][T][D] (or [T][D]) float64 on the device,
        strides honoured; index [U][I] int32 on the device (select_frames' output).  A row whose index lies outside
        [0, n_src[u]) (default T) is `fill`.  Returns [U][max n_out][D] (zeros beyond n_out[u]), or out."""
        lib, t = self._corpus_lib(), self.torch
        x3 = self._frames3(x, "gather_rows")
        U, T, D = (int(v) for v in x3.shape)
        i2 = index[None] if index.dim() == 1 else index
        assert i2.dtype == t.int32 and i2.device == self.device and i2.dim() == 2 and i2.shape[0] == U and (i2.shape[1] == 1 or i2.stride(1) == 1), \
            f"gather_rows: index [{U}][I] int32 on {self.device} with adjacent entries"
        no = self._counts(n_out, U, int(i2.shape[1]), "gather_rows: n_out")
        ns = self._counts(n_src, U, T, "gather_rows: n_src")
        ret = out
        if out is None:
            out = t.zeros((U, int(no.max()), D), dtype=t.float64, device=self.device)
            ret = out[0] if x.dim() == 2 else out
        o3 = self._frames3(out, "gather_rows")
        assert o3.shape[0] == U and o3.shape[1] >= int(no.max()) and o3.shape[2] == D, f"gather_rows: out must be [{U}][>= {int(no.max())}][{D}]"
        self._check(lib.world_hip_gather_rows_batch(self._context(), U, D, ns.ctypes.data_as(_ip), x3.data_ptr(), self._stride(x3, 0, 0),
                                                    self._stride(x3, 1, D), no.ctypes.data_as(_ip), i2.data_ptr(), self._stride(i2, 0, 0),
                                                    float(fill), o3.data_ptr(), self._stride(o3, 0, 0), self._stride(o3, 1, D)), "gather_rows")
        return ret

    def _pair_rows(self, x, first, P, name):
        """frames [P][F][D] or a block [rows][D] with each pair's first row -> (first rows int64, row stride, rows each pair
        may reach to)"""
        t = self.torch
        assert x.dtype == t.float64 and x.device == self.device and x.dim() in (2, 3), f"{name}: float64 [P, F, D] or [rows, D] on {self.device}"
        assert x.shape[-1] >= 1 and (x.shape[-1] == 1 or x.stride(-1) == 1), f"{name}: the columns of a row must be adjacent"
        stride = self._stride(x, -2, max(int(x.shape[-1]), int(x.stride(-2))))
        assert stride >= x.shape[-1], f"{name}: rows overlap"
        if x.dim() == 3:
            assert first is None and x.shape[0] == P, f"{name}: [P, F, D]"
            assert P == 1 or x.stride(0) % stride == 0, f"{name}: the utterances must lie whole rows apart"
            return np.arange(P, dtype=np.int64) * ((x.stride(0) // stride) if P > 1 else 0), stride, np.full(P, x.shape[1], dtype=np.int64)
        first = np.zeros(1, dtype=np.int64) if first is None and P == 1 else first
        assert first is not None, f"{name}: a block of rows needs {name}_row"
        first = np.ascontiguousarray(first, dtype=np.int64)
        assert len(first) == P and int(first.min()) >= 0 and int(first.max()) < x.shape[0]
        return first, stride, x.shape[0] - first

    def joint_rows(self, a, b, path, path_len, sel_a=None, sel_b=None, a_row=None, b_row=None, out=None, n_a=None, n_b=None,
                   n_sel_a=None, n_sel_b=None, fill=0.0):
        """the joint rows [a, b] along DTW paths: a, b as align() takes them ([P, F, D] or a block [rows, D] with a_row /
        b_row; b may be None); path [P, S, 2] int32 and path_len [P] (host counts, or align()'s tensor) as align() returns
        them; sel_a / sel_b [P, I] int32 on the device: the frame numbers the path's indices stand for (select_frames'
        index), or None.  n_a / n_b: each side's rows per pair (default: all the tensor has from the pair's first row on),
        n_sel_*: the selections' lengths (default I).  An index out of range gives `fill` in that half of the row.
        -> z [sum of path_len][Da + Db] float64, pair u's rows from the sum of the path lengths before it; or out."""
        lib, t = self._corpus_lib(), self.torch
        if t.is_tensor(path_len):
            path_len = path_len.cpu().numpy()
        K = np.ascontiguousarray(np.atleast_1d(path_len), dtype=np.int32)
        P = len(K)
        assert path.dtype == t.int32 and path.device == self.device and path.dim() == 3 and path.shape[0] == P and path.shape[2] == 2 and \
            path[0].is_contiguous() and int(K.max()) <= path.shape[1], f"joint_rows: path [{P}][>= {int(K.max())}][2] int32 on {self.device}"
        assert P == 1 or path.stride(0) == 2 * path.shape[1], "joint_rows: the paths must lie p_stride cells apart"
        lp = C.POINTER(C.c_longlong)
        sides = []
        for x, first, n, sel, n_sel, name in ((a, a_row, n_a, sel_a, n_sel_a, "a"), (b, b_row, n_b, sel_b, n_sel_b, "b")):
            if x is None:
                assert name == "b", "joint_rows: a is required"
                sides.append((0, None, None, None, 0, None, None, 0))
                continue
            fr, stride, reach = self._pair_rows(x, first, P, name)
            cnt = reach.astype(np.int32) if n is None else np.ascontiguousarray(np.atleast_1d(n), dtype=np.int32)
            assert len(cnt) == P and bool(np.all(cnt <= reach)), f"joint_rows: n_{name} beyond the tensor"
            s_ptr, s_n, s_us = None, None, 0
            if sel is not None:
                assert sel.dtype == t.int32 and sel.device == self.device and sel.dim() == 2 and sel.shape[0] == P and \
                    (sel.shape[1] == 1 or sel.stride(1) == 1), f"joint_rows: sel_{name} [{P}][I] int32 on {self.device}"
                s_n = self._counts(n_sel, P, int(sel.shape[1]), f"joint_rows: n_sel_{name}")
                s_ptr, s_us = sel.data_ptr(), self._stride(sel, 0, 0)
            sides.append((int(x.shape[-1]), x.data_ptr(), fr, cnt, stride, s_ptr, s_n, s_us))
        (da, pa, fa, na, sa, qa, ma, ua), (db, pb, fb, nb, sb, qb, mb, ub) = sides
        z_row = np.concatenate([[0], np.cumsum(K[:-1], dtype=np.int64)]).astype(np.int64)
        rows = int(K.sum(dtype=np.int64))
        if out is None:
            out = t.empty((rows, da + db), dtype=t.float64, device=self.device)
        assert out.dtype == t.float64 and out.device == self.device and tuple(out.shape) == (rows, da + db) and (da + db == 1 or out.stride(1) == 1), \
            f"joint_rows: out must be [{rows}][{da + db}] float64"
        ip = lambda v: None if v is None else v.ctypes.data_as(_ip)
        self._check(lib.world_hip_joint_rows_batch(self._context(), P, da, db, pa, fa.ctypes.data_as(lp), ip(na), sa, pb,
                                                   None if fb is None else fb.ctypes.data_as(lp), ip(nb), sb, ip(K), path.data_ptr(),
                                                   int(path.shape[1]), qa, ip(ma), ua, qb, ip(mb), ub, float(fill), out.data_ptr(),
                                                   z_row.ctypes.data_as(lp), self._stride(out, 0, da + db)), "joint_rows")
        return out

    def probe_machine(self):
        """world_hip_probe_machine (include/world_hip.h): ~50 ms of microbenchmarks that characterise the box"""
        if not hasattr(self.lib, "world_hip_probe_machine"):
            return None
        v = (C.c_double * 8)()
        self._check(self.lib.world_hip_probe_machine(self._context(), v, 8), "probe_machine")
        keys = ("sclk_mhz_under_fp64_load", "fp64_fma_tflops", "chase_ns_2gb", "chase_ns_64mb_warm", "chase_ns_1mb_warm",
                "lds_trip_cycles_idle_cu", "lds_trip_cycles_loaded_cu", "compute_units")
        return {k: round(float(x), 2) for k, x in zip(keys, v)}

    def analyze(self, x, fs, x_len=None, f0_method="harvest", frame_period=5.0, f0_floor=71.0, f0_ceil=800.0,
                q1=-0.15, threshold=0.85, sp_out=None, ap_out=None, tpos_out=None, f0_out=None, fft_size=None):
        """The north-star pipeline: F0 (Harvest, or DIO+StoneMask) -> CheapTrick -> D4C.
        fft_size: CheapTrick's transform and both matrices' bins (default: the natural size of fs at a 71 Hz floor).
        sp_out / ap_out / tpos_out / f0_out (Harvest route): caller-owned result buffers of the right shape, reused from
        call to call -- the library writes every frame below an utterance's count and nothing else, so what lies beyond
        (the padding of a ragged batch) is the caller's."""
        if f0_method == "harvest":
            # one library call: Harvest, then CheapTrick beside D4C on two streams of the context
            t = self.torch
            B, L, xl = self._prep(x, x_len)
            fft_size = fft_size or cheaptrick_fft_size(fs, 71.0)
            nb = fft_size // 2 + 1
            nf = np.array([frame_count(fs, int(n), frame_period) for n in xl], dtype=np.int32)
            F = int(nf.max())
            # Fresh buffers are zero-filled only where a ragged batch leaves padding behind the shorter utterances'
            # frames: every frame below nf[u] is written by the stages (hc_output; ct_frame / d4c_finish write whole rows),
            # and a fill is a launch of its own per array and job (round 4's kernel trace: two per job for tpos / f0).
            new = t.zeros if int(nf.min()) < F else t.empty
            tpos = tpos_out if tpos_out is not None else new((B, F), dtype=t.float64, device=x.device)
            f0 = f0_out if f0_out is not None else new((B, F), dtype=t.float64, device=x.device)
            assert tpos.shape == (B, F) and f0.shape == (B, F) and tpos.is_contiguous() and f0.is_contiguous()
            sp = sp_out if sp_out is not None else new((B, F, nb), dtype=t.float64, device=x.device)
            ap = ap_out if ap_out is not None else new((B, F, nb), dtype=t.float64, device=x.device)
            assert sp.shape == (B, F, nb) and ap.shape == (B, F, nb) and sp.is_contiguous() and ap.is_contiguous()
            hopt, copt, dopt = HarvestOption(f0_floor, f0_ceil, frame_period), CheapTrickOption(q1, 71.0, fft_size), D4COption(threshold)
            self._check(self.lib.world_hip_analyze_batch(self._context(), B, fs, x.data_ptr(), L, xl.ctypes.data_as(_ip),
                                                         C.byref(hopt), C.byref(copt), C.byref(dopt), F, tpos.data_ptr(),
                                                         f0.data_ptr(), sp.data_ptr(), ap.data_ptr()), "analyze")
            return tpos, f0, sp, ap, nf
        elif f0_method == "dio":
            tpos, f0_raw, nf = self.dio(x, fs, x_len, f0_floor, f0_ceil, frame_period=frame_period)
            f0 = self.stonemask(x, fs, tpos, f0_raw, nf, x_len)
        else:
            raise ValueError(f0_method)
        fft_size = fft_size or cheaptrick_fft_size(fs, 71.0)
        sp = self.cheaptrick(x, fs, tpos, f0, nf, x_len, q1=q1, fft_size=fft_size, out=sp_out)
        ap = self.d4c(x, fs, tpos, f0, nf, fft_size, x_len, threshold=threshold, out=ap_out)
        return tpos, f0, sp, ap, nf


def analyze_sharded_c(lib, ctxs, xs, fs, block_ptrs, rows_capacity, sub_batch=32, frame_period=5.0, f0_floor=71.0,
                      f0_ceil=800.0, q1=-0.15, threshold=0.85, wire=0):
    """world_hip_analyze_sharded (include/world_hip.h): ONE process, several contexts (normally one per GPU), the job's
    utterances as host arrays.  ctxs: library contexts; xs: list of 1-D float64 numpy arrays; block_ptrs: one device
    pointer per context to rows_capacity x world_hip_record_columns(fft, wire) doubles (wire 0: f64 records, 1: the
    spectra as float32).  Returns where [n_utt, 3] = (context index, first row, n_frames): every block then holds ALL
    records at those rows."""
    n = len(xs)
    fft_size = cheaptrick_fft_size(fs, 71.0)
    cols = lib.world_hip_record_columns(fft_size, wire)
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    vp = C.c_void_p
    xp = (vp * max(1, n))(*[x.ctypes.data for x in xs])
    xl = np.ascontiguousarray([len(x) for x in xs], dtype=np.int32)
    cp = (vp * len(ctxs))(*ctxs)
    bp = (vp * len(ctxs))(*block_ptrs)
    where = np.zeros((max(1, n), 3), dtype=np.int64)
    hopt, copt, dopt = HarvestOption(f0_floor, f0_ceil, frame_period), CheapTrickOption(q1, 71.0, fft_size), D4COption(threshold)
    rc = lib.world_hip_analyze_sharded(len(ctxs), cp, n, fs, xp, xl.ctypes.data_as(_ip), C.byref(hopt), C.byref(copt),
                                       C.byref(dopt), sub_batch, bp, rows_capacity, cols,
                                       where.ctypes.data_as(C.POINTER(C.c_longlong)))
    if rc != 0:
        raise RuntimeError("analyze_sharded: " + lib.world_hip_last_error().decode())
    return where[:n]


class RealtimeStreams:
    """world_hip_realtime_*: n_streams independent streams, each behaving as one reference WorldSynthesizer.

    add(stream, f0, sp, ap): one chunk; f0 host (numpy / list), sp / ap [frames, fft/2+1] float64 CUDA tensors (copied into
    the stream's frame store on the current stream); returns 1, or 0 when the stream's ring is full.
    add_coded(stream, f0, coded_sp, coded_ap): the same for coded rows (mel-cepstrum / band aperiodicity), decoded on the way in.
    synthesize(): (out [n_streams, buffer_size] CUDA tensor, produced [n_streams] numpy bool) -- Synthesis2 of every stream.
    is_locked(stream), refresh(stream), close()."""

    def __init__(self, wh, n_streams, fs, frame_period, fft_size, buffer_size, number_of_pointers):
        self.wh, self.lib, self.torch = wh, wh.lib, wh.torch
        self.n_streams, self.buffer_size, self.bins = int(n_streams), int(buffer_size), int(fft_size) // 2 + 1
        self.ctx = wh._context()
        h = C.c_void_p()
        wh._check(self.lib.world_hip_realtime_create(self.ctx, self.n_streams, int(fs), float(frame_period), int(fft_size),
                                                     self.buffer_size, int(number_of_pointers), C.byref(h)),
                  "world_hip_realtime_create")
        self.h = h

    def _ok(self, r, what):
        if r < 0:
            raise RuntimeError(f"{what}: {self.lib.world_hip_last_error().decode()}")
        return r

    def add(self, stream, f0, sp, ap):
        t = self.torch
        f0 = _f64(f0)
        for a in (sp, ap):
            assert a.dtype == t.float64 and a.is_cuda and a.dim() == 2 and a.shape[1] >= self.bins and a.stride(1) == 1
        assert sp.shape[0] >= len(f0) and ap.shape[0] >= len(f0) and sp.stride(0) == ap.stride(0)
        return self._ok(self.lib.world_hip_realtime_add(self.h, int(stream), _p(f0), len(f0), C.c_void_p(sp.data_ptr()),
                                                        C.c_void_p(ap.data_ptr()), sp.stride(0)), "world_hip_realtime_add")

    def add_coded(self, stream, f0, coded_sp, coded_ap):
        """add() of one chunk whose rows are coded: coded_sp [frames, number_of_dimensions] and coded_ap [frames, bands]
        float64 CUDA tensors with the same row stride (e.g. column slices of analyze_coded's records), decoded straight
        into the stream's frame store (world_hip_realtime_add_coded)"""
        t = self.torch
        if not hasattr(self.lib, "world_hip_realtime_add_coded"):
            raise RuntimeError("this libworld_hip.so has no world_hip_realtime_add_coded")
        f0 = _f64(f0)
        for a in (coded_sp, coded_ap):
            assert a.dtype == t.float64 and a.is_cuda and a.dim() == 2 and a.stride(1) == 1 and a.shape[0] >= len(f0)
        assert coded_sp.stride(0) == coded_ap.stride(0), "coded_sp and coded_ap rows must lie the same stride apart"
        return self._ok(self.lib.world_hip_realtime_add_coded(self.h, int(stream), _p(f0), len(f0),
                                                              C.c_void_p(coded_sp.data_ptr()), int(coded_sp.shape[1]),
                                                              C.c_void_p(coded_ap.data_ptr()), coded_sp.stride(0)),
                        "world_hip_realtime_add_coded")

    def synthesize(self):
        t = self.torch
        out = t.empty((self.n_streams, self.buffer_size), dtype=t.float64, device=self.wh.device)
        produced = np.zeros(self.n_streams, dtype=np.int32)
        self._ok(self.lib.world_hip_realtime_synthesize(self.h, C.c_void_p(out.data_ptr()), produced.ctypes.data_as(_ip)),
                 "world_hip_realtime_synthesize")
        return out, produced.astype(bool)

    def is_locked(self, stream):
        return bool(self._ok(self.lib.world_hip_realtime_is_locked(self.h, int(stream)), "world_hip_realtime_is_locked"))

    def refresh(self, stream):
        self._ok(self.lib.world_hip_realtime_refresh(self.h, int(stream)), "world_hip_realtime_refresh")

    def close(self):
        """(WorldHip.close() calls this first: the object uses one of its contexts)"""
        if self.h:
            self.lib.world_hip_realtime_destroy(self.h)
            self.h = None
            self.wh._realtime.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
