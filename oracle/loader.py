"""ctypes loaders for the CPU oracles -- TEST INFRASTRUCTURE ONLY.

Two interchangeable back ends with one Python surface:

* ``PortOracle``  -- oracle/libworld_oracle.so, this repo's plain-C restatement.
* ``WideOracle``  -- oracle/libworld_oracle_wide.so, the same source with its value
  arithmetic in long double (-DWO_WIDE): the more precise answer the accuracy
  tests measure both the GPU and the reference against.
* ``RefContour``  -- oracle/_ref/libworld_ref_contour.so, the reference's contour stage of Harvest
  on made-up candidates (oracle/harvest_contour_ref.cpp).
* ``RefCandidates`` -- oracle/_ref/libworld_ref_candidates.so, the reference's candidate stage of Harvest
  on made-up zero-crossing lists (oracle/harvest_candidates_ref.cpp).
* ``RefRefine``   -- oracle/_ref/libworld_ref_refine.so, the reference's refinement stage of Harvest on a
  made-up candidate map (oracle/harvest_refine_ref.cpp).
* ``RefOracle``   -- oracle/_ref/libworld_ref*.so, the UNMODIFIED reference
  compiled in place from /root/reference by oracle/Makefile (present whenever
  it was built in the container; the .so travels to the GPU box).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import
this module.  Nothing under world_amd/ does.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def build(quiet=True):
    """Compile the restatement (and the in-place reference when available)."""
    subprocess.run(["make", "-s", "-f", os.path.join(HERE, "Makefile")],
                   check=True, stdout=subprocess.DEVNULL if quiet else None)


class _Base:
    kind = "?"

    def frame_count(self, fs, n, frame_period):
        return int(1000.0 * n / fs / frame_period) + 1

    def cheaptrick_fft_size(self, fs, f0_floor=71.0):
        import math
        return int(2.0 ** (1.0 + int(math.log(3.0 * fs / f0_floor + 1) / 0.69314718055994529)))


# world_oracle.h: WO_HC_*, in order
HC_COUNTERS = ("sections", "rejected", "kept", "compacted", "merge_disjoint", "merge_contained", "merge_s1_gt", "merge_s1_eq",
               "merge_s1_lt", "merge_out_of_order", "bridged", "extend_stopped", "extend_full_reach", "extend_tie",
               "extend_at_range", "extend_hit_after_3")


# world_oracle.h: WO_HR_*: a slot's report is hw, first, lgN, nh, idx[6], gate, zero_power; and the gate's values
HR_HW, HR_FIRST, HR_LGN, HR_NH, HR_IDX, HR_GATE, HR_ZERO_POWER, HR_WIDTH = 0, 1, 2, 3, 4, 10, 11, 12
HR_PASSED, HR_FLOOR, HR_CEIL, HR_SCORE, HR_EMPTY = range(5)


class PortOracle(_Base):
    kind = "port"

    def __init__(self, path=None):
        path = path or os.path.join(HERE, "libworld_oracle.so")
        if not os.path.exists(path):
            build()
        self.lib = L = C.CDLL(path)
        L.wo_randn.restype = C.c_double
        L.wo_frame_count.restype = C.c_int
        L.wo_frame_count.argtypes = [C.c_int, C.c_int, C.c_double]
        L.wo_harvest.argtypes = [_dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, _dp, _dp]
        if hasattr(L, "wo_harvest_contour"):
            L.wo_harvest_contour.argtypes = [_dp, _dp, C.c_int, C.c_int, C.c_double] + [_dp] * 8 + [C.POINTER(C.c_int)]
            L.wo_harvest_smooth.argtypes = [_dp, C.c_int, _dp]
        if hasattr(L, "wo_harvest_candidates"):
            L.wo_harvest_candidates.restype = C.c_int
            L.wo_harvest_candidates.argtypes = [_dp, C.POINTER(C.c_int), C.c_int, C.c_double, _dp, C.c_int, C.c_int, C.c_double,
                                                C.c_double, _dp, _dp, C.c_int]
        if hasattr(L, "wo_harvest_refine"):
            L.wo_harvest_refine.restype = None
            L.wo_harvest_refine.argtypes = [_dp, C.c_int, C.c_double, _dp, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _dp, _dp,
                                            C.POINTER(C.c_int)]
        L.wo_dio.argtypes = [_dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                             C.c_int, C.c_double, _dp, _dp]
        L.wo_stonemask.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp]
        L.wo_cheaptrick.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_int, _dp]
        L.wo_d4c.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _dp]
        L.wo_rfft.argtypes = [C.c_int, _dp, _dp, _dp]
        L.wo_irfft_unscaled.argtypes = [C.c_int, _dp, _dp, _dp]
        if hasattr(L, "wo_cfft"):
            L.wo_cfft.argtypes = [C.c_int, _dp, _dp, C.c_int]
        L.wo_interp1.argtypes = [_dp, _dp, C.c_int, _dp, C.c_int, _dp]
        L.wo_decimate.argtypes = [_dp, C.c_int, C.c_int, _dp]
        L.wo_linear_smoothing.argtypes = [_dp, C.c_double, C.c_int, C.c_int, _dp]
        L.wo_dc_correction.argtypes = [_dp, C.c_double, C.c_int, C.c_int, _dp]
        L.wo_round.argtypes = [C.c_double]
        L.wo_nuttall.argtypes = [C.c_int, _dp]
        L.wo_synthesis.argtypes = [_dp, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, _dp]
        L.wo_number_of_aperiodicities.argtypes = [C.c_int]
        L.wo_code_aperiodicity.argtypes = [_dp, C.c_int, C.c_int, C.c_int, _dp]
        L.wo_decode_aperiodicity.argtypes = [_dp, C.c_int, C.c_int, C.c_int, _dp]
        L.wo_code_spectral_envelope.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp]
        L.wo_decode_spectral_envelope.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp]

    # -- primitives --
    def randn(self, count):
        st = (C.c_uint32 * 4)()
        self.lib.wo_randn_seed(st)
        return np.array([self.lib.wo_randn(st) for _ in range(count)])

    def rfft(self, x):
        x = _f64(x); n = len(x)
        re = np.zeros(n // 2 + 1); im = np.zeros(n // 2 + 1)
        self.lib.wo_rfft(n, _p(x), _p(re), _p(im))
        return re + 1j * im

    def irfft_unscaled(self, X):
        n = 2 * (len(X) - 1)
        re = _f64(X.real); im = _f64(X.imag); out = np.zeros(n)
        self.lib.wo_irfft_unscaled(n, _p(re), _p(im), _p(out))
        return out

    def cfft(self, z, sign=-1):
        """unscaled complex transform of z (a power of two long): sign -1 forward, +1 backward"""
        z = np.asarray(z, dtype=np.complex128)
        re, im = _f64(z.real).copy(), _f64(z.imag).copy()
        self.lib.wo_cfft(len(z), _p(re), _p(im), sign)
        return re + 1j * im

    def interp1(self, x, y, xi):
        x, y, xi = _f64(x), _f64(y), _f64(xi)
        yi = np.zeros(len(xi))
        self.lib.wo_interp1(_p(x), _p(y), len(x), _p(xi), len(xi), _p(yi))
        return yi

    def decimate(self, x, r):
        x = _f64(x)
        y = np.zeros(len(x))
        self.lib.wo_decimate(_p(x), len(x), r, _p(y))
        return y[: (len(x) - 1) // r + 1]

    def linear_smoothing(self, spec, width, fs, fft_size):
        spec = _f64(spec); out = np.zeros(fft_size // 2 + 1)
        self.lib.wo_linear_smoothing(_p(spec), width, fs, fft_size, _p(out))
        return out

    # -- analysis path --
    def harvest(self, x, fs, f0_floor=71.0, f0_ceil=800.0, frame_period=5.0):
        x = _f64(x); nf = self.frame_count(fs, len(x), frame_period)
        tp = np.zeros(nf); f0 = np.zeros(nf)
        self.lib.wo_harvest(_p(x), len(x), fs, f0_floor, f0_ceil, frame_period, _p(tp), _p(f0))
        return tp, f0

    def harvest_contour(self, cand, score, frame_period=5.0):
        """Harvest from the refined candidates on: cand, score [nf, nslot] at 1 ms -> a dict of pruned_cand, pruned_score
        [nf, nslot], step2, step3, step4, smooth [nf], tpos, f0 at frame_period and counters, {name: times the branch was
        taken} (HC_COUNTERS: world_oracle.h's WO_HC_*)"""
        cand, score = _f64(cand), _f64(score)
        nf, nslot = cand.shape
        assert score.shape == cand.shape and nf >= 1
        n = int((nf - 1) / frame_period) + 1
        o = dict(pruned_cand=np.zeros((nf, nslot)), pruned_score=np.zeros((nf, nslot)), step2=np.zeros(nf), step3=np.zeros(nf),
                 step4=np.zeros(nf), smooth=np.zeros(nf), tpos=np.zeros(n), f0=np.zeros(n))
        count = (C.c_int * len(HC_COUNTERS))()
        got = self.lib.wo_harvest_contour(_p(cand), _p(score), nf, nslot, frame_period, *(_p(o[k]) for k in (
            "pruned_cand", "pruned_score", "step2", "step3", "step4", "smooth", "tpos", "f0")), count)
        assert got == n
        o["counters"] = dict(zip(HC_COUNTERS, count))
        return o

    def smooth_f0(self, f0):
        f0 = _f64(f0); out = np.zeros(len(f0))
        self.lib.wo_harvest_smooth(_p(f0), len(f0), _p(out))
        return out

    def harvest_candidates(self, nf, band_f0, edges=None, counts=None, raw=None, afs=8000.0, f0_floor=71.0, f0_ceil=800.0):
        """Harvest's candidate stage on made-up lists: edges [nch, 4, ev_cap] fine edges, counts [nch, 4] (or raw [nch, nf]
        given: detection alone) -> raw [nch, nf], cand [nf, maxc], nc"""
        return _harvest_candidates(nf, band_f0, edges, counts, raw, lambda e, c, cap, b, nch, maxc, r, cand: (
            self.lib.wo_harvest_candidates(e, c, cap, afs, b, nch, nf, f0_floor, f0_ceil, r, _p(cand), maxc), cand), maxc_wide=False)

    def harvest_refine(self, y, cand, afs=8000.0, f0_floor=71.0, f0_ceil=800.0):
        """Harvest's refinement stage on a made-up map: y the decimated signal, cand [nf, nc] -> dict(refined, score [nf, 7 nc],
        raw [nf, 7 nc, 2] the values before the gate, report [nf, 7 nc, HR_WIDTH] int32: world_oracle.h's WO_HR_*)"""
        y, cand = _f64(y), _f64(cand)
        nf, nc = cand.shape
        refined, score = np.zeros((nf, 7 * nc)), np.zeros((nf, 7 * nc))
        raw, report = np.zeros((nf, 7 * nc, 2)), np.zeros((nf, 7 * nc, HR_WIDTH), dtype=np.int32)
        self.lib.wo_harvest_refine(_p(y), len(y), afs, _p(cand), nf, nc, f0_floor, f0_ceil, _p(refined), _p(score), _p(raw),
                                   report.ctypes.data_as(C.POINTER(C.c_int)))
        return dict(refined=refined, score=score, raw=raw, report=report)

    def dio(self, x, fs, f0_floor=71.0, f0_ceil=800.0, channels_in_octave=2.0, frame_period=5.0,
            speed=1, allowed_range=0.1):
        x = _f64(x); nf = self.frame_count(fs, len(x), frame_period)
        tp = np.zeros(nf); f0 = np.zeros(nf)
        self.lib.wo_dio(_p(x), len(x), fs, f0_floor, f0_ceil, channels_in_octave, frame_period,
                        speed, allowed_range, _p(tp), _p(f0))
        return tp, f0

    def stonemask(self, x, fs, tp, f0):
        x, tp, f0 = _f64(x), _f64(tp), _f64(f0)
        out = np.zeros(len(f0))
        self.lib.wo_stonemask(_p(x), len(x), fs, _p(tp), _p(f0), len(f0), _p(out))
        return out

    def cheaptrick(self, x, fs, tp, f0, q1=-0.15, f0_floor=71.0, fft_size=None):
        x, tp, f0 = _f64(x), _f64(tp), _f64(f0)
        fft_size = fft_size or self.cheaptrick_fft_size(fs, f0_floor)
        sp = np.zeros((len(f0), fft_size // 2 + 1))
        self.lib.wo_cheaptrick(_p(x), len(x), fs, _p(tp), _p(f0), len(f0), q1, fft_size, _p(sp))
        return sp

    def d4c(self, x, fs, tp, f0, fft_size, threshold=0.85):
        x, tp, f0 = _f64(x), _f64(tp), _f64(f0)
        ap = np.zeros((len(f0), fft_size // 2 + 1))
        self.lib.wo_d4c(_p(x), len(x), fs, _p(tp), _p(f0), len(f0), fft_size, threshold, _p(ap))
        return ap

    # -- synthesis --
    def synthesis(self, f0, sp, ap, fft_size, frame_period, fs, y_length):
        f0, sp, ap = _f64(f0), _f64(sp), _f64(ap)
        y = np.zeros(y_length)
        self.lib.wo_synthesis(_p(f0), len(f0), _p(sp), _p(ap), fft_size, frame_period, fs, y_length, _p(y))
        return y

    # -- codec --
    def number_of_aperiodicities(self, fs):
        return self.lib.wo_number_of_aperiodicities(fs)

    def code_aperiodicity(self, ap, fs, fft_size):
        ap = _f64(ap); out = np.zeros((ap.shape[0], self.number_of_aperiodicities(fs)))
        self.lib.wo_code_aperiodicity(_p(ap), ap.shape[0], fs, fft_size, _p(out))
        return out

    def decode_aperiodicity(self, coded, fs, fft_size):
        coded = _f64(coded); out = np.zeros((coded.shape[0], fft_size // 2 + 1))
        self.lib.wo_decode_aperiodicity(_p(coded), coded.shape[0], fs, fft_size, _p(out))
        return out

    def code_spectral_envelope(self, sp, fs, fft_size, ndim):
        sp = _f64(sp); out = np.zeros((sp.shape[0], ndim))
        self.lib.wo_code_spectral_envelope(_p(sp), sp.shape[0], fs, fft_size, ndim, _p(out))
        return out

    def decode_spectral_envelope(self, coded, fs, fft_size):
        coded = _f64(coded); out = np.zeros((coded.shape[0], fft_size // 2 + 1))
        self.lib.wo_decode_spectral_envelope(_p(coded), coded.shape[0], fs, fft_size, coded.shape[1], _p(out))
        return out


def wide_is_wider():
    """long double is wider than double on this host (x86-64: 64-bit mantissa); else WideOracle is just PortOracle"""
    return float(np.finfo(np.longdouble).eps) < float(np.finfo(np.float64).eps)


class WideOracle(PortOracle):
    kind = "wide"

    def __init__(self, path=None):
        path = path or os.path.join(HERE, "libworld_oracle_wide.so")
        if not os.path.exists(path):
            build()
        super().__init__(path)


# The generic binding of the reference's 13-symbol C ABI lives in the product's
# Python mirror (world_amd/api.py: HostAPI); the oracle side only points it at
# the in-place build of the reference.
from world_amd.api import HostAPI as WorldCABI  # noqa: E402


def _cpu_has(flag):
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return flag in line.split()
    except OSError:
        pass
    return False


class RefOracle(WorldCABI):
    kind = "reference"

    def __init__(self, optimized=False):
        name = "libworld_ref_o3.so" if optimized and _cpu_has("avx2") and _cpu_has("fma") else "libworld_ref.so"
        path = os.path.join(HERE, "_ref", name)
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.flags = "-O3 -march=x86-64-v3" if name.endswith("_o3.so") else "-O1 (reference makefile:6)"
        super().__init__(path, hip_runtime=False)


class RefContour:
    """oracle/_ref/libworld_ref_contour.so: the reference's own RemoveUnreliableCandidates, FixStep1 .. 4, FixF0Contour and
    SmoothF0Contour on made-up candidates (oracle/harvest_contour_ref.cpp includes the reference's harvest.cpp in place)"""
    kind = "reference"
    path = os.path.join(HERE, "_ref", "libworld_ref_contour.so")

    @classmethod
    def available(cls):
        return os.path.exists(cls.path)

    def __init__(self):
        if not self.available():
            raise FileNotFoundError(self.path)
        self.lib = C.CDLL(self.path)
        self.lib.ref_harvest_contour.argtypes = [_dp, _dp, C.c_int, C.c_int] + [_dp] * 7
        self.lib.ref_harvest_contour.restype = None
        self.lib.ref_smooth_f0.argtypes = [_dp, C.c_int, _dp]
        self.lib.ref_smooth_f0.restype = None

    def harvest_contour(self, cand, score):
        """as PortOracle.harvest_contour, without the frames at frame_period (Harvest() subsamples inline), and with
        FixF0Contour called whole held to its stages called one by one"""
        cand, score = _f64(cand), _f64(score)
        nf, nslot = cand.shape
        assert score.shape == cand.shape and nf >= 1
        o = dict(pruned_cand=np.zeros((nf, nslot)), pruned_score=np.zeros((nf, nslot)), step2=np.zeros(nf), step3=np.zeros(nf),
                 step4=np.zeros(nf), whole=np.zeros(nf), smooth=np.zeros(nf))
        self.lib.ref_harvest_contour(_p(cand), _p(score), nf, nslot, *(_p(o[k]) for k in (
            "pruned_cand", "pruned_score", "step2", "step3", "step4", "whole", "smooth")))
        assert o["whole"].tobytes() == o["step4"].tobytes(), "FixF0Contour is not its stages in a row"
        del o["whole"]
        return o

    def smooth_f0(self, f0):
        f0 = _f64(f0); out = np.zeros(len(f0))
        self.lib.ref_smooth_f0(_p(f0), len(f0), _p(out))
        return out


def _harvest_candidates(nf, band_f0, edges, counts, raw, call, maxc_wide):
    """the argument handling PortOracle.harvest_candidates and RefCandidates.harvest_candidates share; cand rows are maxc wide,
    or nch wide and cut to maxc (the reference's Sub2 does not check its cap)"""
    band_f0 = _f64(band_f0)
    nch = len(band_f0)
    maxc = int(nch / 10.0 + 0.5) * 7
    if edges is not None:
        edges, counts = _f64(edges), np.ascontiguousarray(counts, dtype=np.int32)
        assert edges.ndim == 3 and edges.shape[:2] == counts.shape == (nch, 4) and counts.max(initial=0) <= edges.shape[2]
        raw = np.zeros((nch, nf))
        e, c, cap = _p(edges), counts.ctypes.data_as(C.POINTER(C.c_int)), edges.shape[2]
    else:
        raw = np.array(_f64(raw))
        assert raw.shape == (nch, nf)
        e, c, cap = None, None, 0
    cand = np.zeros((nf, nch if maxc_wide else maxc))
    nc, cand = call(e, c, cap, _p(band_f0), nch, maxc, _p(raw), cand)
    assert nc <= maxc
    return dict(raw=raw, cand=np.ascontiguousarray(cand[:, :maxc]), nc=int(nc))


class RefCandidates:
    """oracle/_ref/libworld_ref_candidates.so: the reference's own GetF0CandidateContour, DetectOfficialF0Candidates and
    ZeroCrossingEngine (oracle/harvest_candidates_ref.cpp includes the reference's harvest.cpp in place)"""
    kind = "reference"
    path = os.path.join(HERE, "_ref", "libworld_ref_candidates.so")

    @classmethod
    def available(cls):
        return os.path.exists(cls.path)

    def __init__(self):
        if not self.available():
            raise FileNotFoundError(self.path)
        self.lib = C.CDLL(self.path)
        self.lib.ref_harvest_candidates.restype = C.c_int
        self.lib.ref_harvest_candidates.argtypes = [_dp, C.POINTER(C.c_int), C.c_int, C.c_double, _dp, C.c_int, C.c_int, C.c_double,
                                                    C.c_double, C.c_int, _dp, _dp]
        self.lib.ref_zero_crossing_engine.restype = C.c_int
        self.lib.ref_zero_crossing_engine.argtypes = [_dp, C.c_int, C.c_double, _dp, _dp]

    def harvest_candidates(self, nf, band_f0, edges=None, counts=None, raw=None, afs=8000.0, f0_floor=71.0, f0_ceil=800.0):
        """as PortOracle.harvest_candidates"""
        return _harvest_candidates(nf, band_f0, edges, counts, raw, lambda e, c, cap, b, nch, maxc, r, cand: (
            self.lib.ref_harvest_candidates(e, c, cap, afs, b, nch, nf, f0_floor, f0_ceil, maxc, r, _p(cand)), cand), maxc_wide=True)

    def zero_crossing_engine(self, signal, fs):
        """ZeroCrossingEngine on a signal -> (interval locations, intervals)"""
        signal = _f64(signal)
        loc, val = np.zeros(len(signal)), np.zeros(len(signal))
        n = self.lib.ref_zero_crossing_engine(_p(signal), len(signal), fs, _p(loc), _p(val))
        return loc[:n], val[:n]


class RefRefine:
    """oracle/_ref/libworld_ref_refine.so: the reference's own OverlapF0Candidates, RefineF0Candidates and GetRefinedF0
    (oracle/harvest_refine_ref.cpp includes the reference's harvest.cpp in place)"""
    kind = "reference"
    path = os.path.join(HERE, "_ref", "libworld_ref_refine.so")

    @classmethod
    def available(cls):
        return os.path.exists(cls.path)

    def __init__(self):
        if not self.available():
            raise FileNotFoundError(self.path)
        self.lib = C.CDLL(self.path)
        self.lib.ref_harvest_refine.restype = None
        self.lib.ref_harvest_refine.argtypes = [_dp, C.c_int, C.c_double, _dp, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _dp]
        self.lib.ref_harvest_refine_one.restype = None
        self.lib.ref_harvest_refine_one.argtypes = [_dp, C.c_int] + [C.c_double] * 5 + [_dp, _dp]

    def harvest_refine(self, y, cand, afs=8000.0, f0_floor=71.0, f0_ceil=800.0):
        """as PortOracle.harvest_refine, refined and score alone"""
        y, cand = _f64(y), _f64(cand)
        nf, nc = cand.shape
        refined, score = np.zeros((nf, 7 * nc)), np.zeros((nf, 7 * nc))
        self.lib.ref_harvest_refine(_p(y), len(y), afs, _p(cand), nf, nc, f0_floor, f0_ceil, _p(refined), _p(score))
        return dict(refined=refined, score=score)

    def refine_one(self, y, pos, f0, afs=8000.0, f0_floor=71.0, f0_ceil=800.0):
        """GetRefinedF0 on one candidate at one position -> (refined, score)"""
        y, out = _f64(y), np.zeros(2)
        self.lib.ref_harvest_refine_one(_p(y), len(y), afs, pos, f0, f0_floor, f0_ceil, _p(out), _p(out[1:]))
        return float(out[0]), float(out[1])


def ref_available():
    return os.path.exists(os.path.join(HERE, "_ref", "libworld_ref.so"))


def best_oracle():
    """The real reference when its prebuilt .so is present, else the port."""
    return RefOracle() if ref_available() else PortOracle()


# ---- whole-box CPU baseline: one analysis per worker process ---------------------------
def parallel_analyses(x, fs, frame_period, fft_size, procs, timeout=300, optimized=False):
    """Run `procs` full analyses concurrently, each in its own `python oracle/cpu_worker.py`
    process (no GPU runtime, own heap), all starting at the same wall-clock instant.
    Returns (total frames, wall seconds from the common start to the last finish, build flags)."""
    import tempfile
    import time as _t
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.npy")
        np.save(path, np.ascontiguousarray(x, dtype=np.float64))
        lib = "libworld_ref_o3.so" if optimized and _cpu_has("avx2") and _cpu_has("fma") else "libworld_ref.so"
        flags = "-O3 -march=x86-64-v3" if lib.endswith("_o3.so") else "-O1 (reference makefile:6)"
        if not os.path.exists(os.path.join(HERE, "_ref", lib)):
            flags = "gcc -O2 restatement"
        cmd = [sys.executable, os.path.join(HERE, "cpu_worker.py"), path, str(fs), str(frame_period), str(fft_size),
               "-", lib]
        ps = [subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for _ in range(procs)]
        for p in ps:                                   # every worker has its library and input loaded ...
            if p.stdout.readline().strip() != "ready":
                raise RuntimeError("cpu_worker did not come up")
        start_at = _t.time() + 0.25                    # ... before the common start is named
        for p in ps:
            p.stdin.write(repr(start_at) + "\n")
            p.stdin.flush()
        frames, t_end = 0, start_at
        for p in ps:
            out, _ = p.communicate(timeout=timeout)
            n, t0, t1 = out.split()[-3:]
            frames += int(n)
            t_end = max(t_end, float(t1))
    return frames, t_end - start_at, flags
