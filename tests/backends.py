"""What the tests/test_X_cpu.py / tests/test_X_gpu.py pairs share: the emulated library, the backend
a feature's C calls hang on and its torch form, the fixtures both files import by name, and a few small helpers.  No
assertion here judges the library: those stay in the test files."""
import ctypes as C
import os
import subprocess
import wave
from contextlib import contextmanager

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
SENTINEL_F64 = -7.0


# ---- the emulated library (tests/emu: the kernel sources compiled for the host) -------------------------------------------
def emu_library_path():
    subprocess.run(["make", "-s", "-f", os.path.join(EMU_DIR, "Makefile")], check=True)
    return os.path.join(EMU_DIR, "libworld_emu.so")


def emu_library():
    from world_amd.api import load_library
    return load_library(emu_library_path())


def emu_host():
    from world_amd.api import HostAPI
    return HostAPI(emu_library_path())


def new_context(lib):
    c = lib.world_hip_create(0, None)
    if not c:
        raise RuntimeError("world_hip_create failed: " + lib.world_hip_last_error().decode())
    return c


# ---- the backend: arrays that live where the library wants them ----------------------------------------------------------
class Backend:
    """A library and one context of it.  A feature subclasses this with its C calls.  Here device memory is host memory;
    OnGpu puts it on the card.
      dev(a)    a C-contiguous COPY of the host array a in device memory, its dtype kept: the library never writes into the
                caller's array, which may be shared and read-only
      host(d)   the device array as a NumPy array
      addr(d)   its address as an integer
      ptr(d, doubles=0)   the same as a c_void_p, `doubles` float64 further on; None for None
      fresh()   a backend of the same type on a context of its own, destroyed on the way out"""

    def __init__(self, lib, ctx):
        self.lib, self.ctx = lib, ctx

    def _place(self, a):
        return a

    def dev(self, a):
        return self._place(np.array(a, order="C"))

    def host(self, d):
        return d

    def addr(self, d):
        return d.ctypes.data

    def ptr(self, d, doubles=0):
        return None if d is None else C.c_void_p(self.addr(d) + 8 * doubles)

    def error(self):
        return self.lib.world_hip_last_error().decode()

    @contextmanager
    def fresh(self):
        c = new_context(self.lib)
        try:
            yield type(self)(self.lib, c)
        finally:
            self.lib.world_hip_destroy(c)


class OnGpu:
    """class GpuBackend(OnGpu, cpu.Backend): the feature's calls on torch tensors, made from a WorldHip"""

    def __init__(self, wh):
        super().__init__(wh.lib, wh._context())

    def _place(self, a):
        import torch
        return torch.from_numpy(a).cuda()

    def host(self, d):
        return d.cpu().numpy()

    def addr(self, d):
        return d.data_ptr()

    @contextmanager
    def fresh(self):
        from world_amd.api import WorldHip
        w = WorldHip()
        try:
            yield type(self)(w)
        finally:
            w.close()


# ---- fixtures, imported by name (pytest registers what a test module imports) ---------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return emu_library()


@pytest.fixture(scope="module")
def emu():
    return emu_host()


def cpu_backend(cls):
    """the CPU file's `be`: cls on a context of the emulated library"""
    @pytest.fixture(scope="module", name="be")
    def be(lib):
        c = new_context(lib)
        yield cls(lib, c)
        lib.world_hip_destroy(c)
    return be


@pytest.fixture(scope="module")
def wh():
    import torch
    if not torch.cuda.is_available():
        raise AssertionError("these tests need the MI355X")
    from world_amd.api import WorldHip
    w = WorldHip()
    yield w
    w.close()


def gpu_backend(cls):
    """the GPU file's `be`: cls on the module's WorldHip"""
    @pytest.fixture(scope="module", name="be")
    def be(wh):
        return cls(wh)
    return be


# ---- comparisons and inputs ----------------------------------------------------------------------------------------------
def same_bits(a, b):
    """every element bit-equal, NaN compared as equal"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def rel(a, b):
    """the largest |a - b| / |b|"""
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def smooth_envelope(fs, fft_size, rows, seed):
    """smooth positive formant-shaped rows with a tilt, varying from row to row"""
    rng = np.random.default_rng(seed)
    return 1e-3 * _formants(rng, fs, fft_size, rows) ** 2 + 1e-9


def envelope(fs, fft_size, rows, seed):
    """positive, formant-shaped rows with a tilt and some ripple"""
    rng = np.random.default_rng(seed)
    env = _formants(rng, fs, fft_size, rows)
    return 1e-3 * env ** 2 * (1.0 + 0.3 * rng.uniform(0, 1, env.shape)) + 1e-9


def _formants(rng, fs, fft_size, rows):
    k = np.arange(fft_size // 2 + 1) * fs / fft_size
    env = np.zeros((rows, k.size))
    for c, bw, a in ((700.0, 130.0, 1.0), (1220.0, 170.0, 0.5), (2600.0, 240.0, 0.25), (3500.0, 300.0, 0.1)):
        centre = c * (1.0 + 0.1 * rng.uniform(-1, 1, rows))[:, None]
        env += a / (1.0 + ((k[None, :] - centre) / bw) ** 2)
    return env


_cache = {}


def cached(key, make):
    """make() once per key; the arrays of its value (alone, or in a tuple or list) are made read-only"""
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ---- 16-bit WAV files ----------------------------------------------------------------------------------------------------
def pcm16(x):
    """float samples in [-1, 1) -> int16, rounded and clipped"""
    return np.round(np.asarray(x) * 32768).clip(-32768, 32767).astype("<i2")


def write_wav(path, samples, fs):
    """int16 samples, one channel -> the path as str"""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(samples).astype("<i2").tobytes())
    return str(path)


def read_wav(path):
    """-> (the samples as int32, the sampling rate)"""
    with wave.open(str(path)) as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int32), w.getframerate()
