"""The C-ABI library: builds for gfx950 (hipcc cross-compiles without a GPU), loads,
and exports every symbol include/world_hip.h declares.  No compute calls here."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from world_amd import build
    return build.build()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    return sorted(set(re.findall(r"WORLD_HIP_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)))


def test_header_declares_the_reference_api():
    names = declared_symbols()
    for must in ["Dio", "InitializeDioOption", "GetSamplesForDIO", "Harvest", "InitializeHarvestOption",
                 "GetSamplesForHarvest", "StoneMask", "CheapTrick", "InitializeCheapTrickOption",
                 "GetFFTSizeForCheapTrick", "GetF0FloorForCheapTrick", "D4C", "InitializeD4COption"]:
        assert must in names          # the 13 symbols of SURVEY.md 8b
    for must in ["GetNumberOfAperiodicities", "CodeAperiodicity", "DecodeAperiodicity", "CodeSpectralEnvelope",
                 "DecodeSpectralEnvelope", "Synthesis"]:
        assert must in names          # every public symbol of codec.o


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in declared_symbols():
        assert hasattr(lib, name), name


def test_option_helpers_are_host_arithmetic(lib_path):
    """these never touch the GPU, so they can be checked here"""
    from world_amd.api import CheapTrickOption, DioOption, HarvestOption, load_library
    lib = load_library(lib_path)
    h = HarvestOption(); lib.InitializeHarvestOption(ctypes.byref(h))
    assert (h.f0_floor, h.f0_ceil, h.frame_period) == (71.0, 800.0, 5.0)
    d = DioOption(); lib.InitializeDioOption(ctypes.byref(d))
    assert (d.f0_floor, d.f0_ceil, d.channels_in_octave, d.frame_period, d.speed, d.allowed_range) == \
        (71.0, 800.0, 2.0, 5.0, 1, 0.1)
    c = CheapTrickOption(); lib.InitializeCheapTrickOption(48000, ctypes.byref(c))
    assert (c.q1, c.f0_floor, c.fft_size) == (-0.15, 71.0, 2048)
    lib.InitializeCheapTrickOption(16000, ctypes.byref(c)); assert c.fft_size == 1024
    assert lib.GetSamplesForHarvest(22050, 17500, 5.0) == 159
    assert lib.GetF0FloorForCheapTrick(48000, 2048) == 3.0 * 48000 / (2048 - 3.0)


def test_missing_library_fails_loudly(tmp_path):
    from world_amd.api import HostAPI, load_library
    with pytest.raises(ImportError):
        load_library(str(tmp_path / "nope.so"))
    with pytest.raises(ImportError):
        HostAPI(str(tmp_path / "nope.so"))


def test_batch_tools_refuse_to_run_without_a_gpu(tmp_path):
    """The command-line tools have no CPU path either: without a GPU they stop with an error
    before touching any file (here: CPU-only container; skipped where a GPU is present)."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "world_amd.tools", "analysis", "absent.wav", "--outdir", str(tmp_path / "o")],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs a GPU" in r.stderr
    assert not (tmp_path / "o").exists()


def test_option_and_size_helpers_agree_with_the_reference_build(lib_path):
    """The host-arithmetic helpers (frame counts, FFT sizes, floors, band counts, option defaults) of
    libworld_hip.so against the answers of the unmodified reference (tests/golden/helpers.npz) on a sweep of
    sampling rates, lengths, frame periods and floors; exact equality (they size every caller-owned buffer).
    Where the in-place build of the reference is present, it must give the stored answers too."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from util import GOLDEN, HELPER_ANSWERS, OPTION_INITIALISERS, bind_option_helpers, option_defaults, option_helper_answers
    from oracle.loader import ref_available
    g = np.load(os.path.join(GOLDEN, "helpers.npz"))
    libs = [bind_option_helpers(ctypes.CDLL(lib_path))]
    if ref_available():
        libs.append(bind_option_helpers(ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libworld_ref.so"))))
    cases = list(zip(g["fs"].tolist(), g["n"].tolist(), g["frame_period"].tolist(), g["f0_floor"].tolist()))
    assert len(cases) == 2000
    for L in libs:
        for i, (fs, n, fp, floor) in enumerate(cases):
            got = option_helper_answers(L, int(fs), int(n), fp, floor)
            assert got == tuple(g[k][i] for k in HELPER_ANSWERS), (L._name, fs, n, fp, floor)
        defaults = option_defaults(L)
        for init in OPTION_INITIALISERS:
            assert np.array_equal(defaults[init], g[init]), (L._name, init)


def test_forwarding_headers_compile_like_the_reference_tree(tmp_path):
    """include/world/*.h (and the tools/ headers): a caller written against the reference's header tree --
    #include "world/dio.h" ... -- compiles against this repository's include/ alone, as C and as C++, and sees
    every drop-in symbol with the reference's signature (reference src/world/*.h)"""
    import subprocess
    src = tmp_path / "caller.c"
    src.write_text('''
#include "world/dio.h"
#include "world/harvest.h"
#include "world/stonemask.h"
#include "world/cheaptrick.h"
#include "world/d4c.h"
#include "world/codec.h"
#include "world/synthesis.h"
#include "world/macrodefinitions.h"
#include "audioio.h"
#include "parameterio.h"
WORLD_BEGIN_C_DECLS
int uses_everything(const double *x, int n, int fs, double *tp, double *f0, double **sp, double **ap, double *y);
WORLD_END_C_DECLS
int uses_everything(const double *x, int n, int fs, double *tp, double *f0, double **sp, double **ap, double *y) {
  DioOption d; HarvestOption h; CheapTrickOption c; D4COption a;
  InitializeDioOption(&d); InitializeHarvestOption(&h); InitializeCheapTrickOption(fs, &c); InitializeD4COption(&a);
  int nf = GetSamplesForHarvest(fs, n, h.frame_period) + 0 * GetSamplesForDIO(fs, n, d.frame_period);
  Harvest(x, n, fs, &h, tp, f0); Dio(x, n, fs, &d, tp, f0); StoneMask(x, n, fs, tp, f0, nf, f0);
  c.fft_size = GetFFTSizeForCheapTrick(fs, &c); (void)GetF0FloorForCheapTrick(fs, c.fft_size);
  CheapTrick(x, n, fs, tp, f0, nf, &c, sp); D4C(x, n, fs, tp, f0, nf, c.fft_size, &a, ap);
  CodeAperiodicity((const double *const *)ap, nf, fs, c.fft_size, ap); DecodeAperiodicity((const double *const *)ap, nf, fs, c.fft_size, ap);
  CodeSpectralEnvelope((const double *const *)sp, nf, fs, c.fft_size, 4, sp); DecodeSpectralEnvelope((const double *const *)sp, nf, fs, c.fft_size, 4, sp);
  Synthesis(f0, nf, (const double *const *)sp, (const double *const *)ap, c.fft_size, h.frame_period, fs, n, y);
  wavwrite(y, n, fs, 16, "o.wav"); (void)GetAudioLength("o.wav"); WriteF0("o.f0", nf, 5.0, tp, f0, 0);
  return GetNumberOfAperiodicities(fs);
}
''')
    inc = os.path.join(ROOT, "include")
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        r = subprocess.run([cc, std, "-x", "c" if cc == "gcc" else "c++", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_shape_limits_are_answered_on_the_host():
    """world_hip_check_shape: the limits of the GPU path as pure host arithmetic -- what the drop-in symbols
    check before any GPU work"""
    import ctypes as C
    from world_amd.api import load_library
    lib = load_library()
    why = C.create_string_buffer(256)
    assert lib.world_hip_check_shape(48000, 2048, why, 256) == 0 and why.value == b""
    assert lib.world_hip_check_shape(16000, 1024, why, 256) == 0
    assert lib.world_hip_check_shape(192000, 8192, why, 256) == 0                 # round 5: StoneMask's indices as bytes, D4C's 16384-point shape
    assert lib.world_hip_check_shape(250000, 8192, why, 256) == 1 and b"StoneMask" in why.value     # the first limit met
    assert lib.world_hip_check_shape(96000, 8192, why, 256) == 0                  # round 4: CheapTrick runs 8192 points
    assert lib.world_hip_check_shape(96000, 16384, why, 256) == 1 and b"CheapTrick" in why.value
    assert lib.world_hip_check_shape(48000, 1000, why, 256) == 1 and b"power of two" in why.value
    assert lib.world_hip_check_shape(120000, 4096, why, 256) == 0
    assert lib.world_hip_check_shape(200000, 8192, why, 256) == 1 and b"D4C" in why.value and b"192 kHz" in why.value
    assert lib.world_hip_check_shape(8000, 512, why, 256) == 1 and b"15.8" in why.value
    assert lib.world_hip_check_shape(96000, 4096, why, 256) == 0
    # the pair (fs, fft_size): an unvoiced frame's 500 Hz window, 2 round(1.5 fs / 500) + 1 samples, and the unvoiced pulse
    # spacing, fs / 500 + 1, must fit fft_size (the reference writes past its fft_size-long buffers otherwise)
    for fs, fft, smallest in ((48000, 256, 512), (192000, 1024, 2048), (44100, 256, 512), (96000, 128, 1024)):
        assert lib.world_hip_check_shape(fs, fft, why, 256) == 1, (fs, fft)
        assert b"CheapTrick" in why.value and b"smallest fft_size for this fs is %d" % smallest in why.value, why.value
    for fs, fft in ((48000, 512), (192000, 2048), (16000, 128), (16000, 256), (16000, 8192), (22050, 4096), (44100, 512)):
        assert lib.world_hip_check_shape(fs, fft, why, 256) == 0 and why.value == b"", (fs, fft, why.value)
    assert lib.world_hip_check_shape(42499, 256, why, 256) == 0      # a 255-sample window
    assert lib.world_hip_check_shape(42500, 256, why, 256) == 1      # 2 * 128 + 1 = 257


def test_abi_version_and_hint_are_exported_and_consistent(lib_path):
    """round 6: the batched ABI carries a version a binding checks before it binds prototypes; the header's macro
    and the library agree; the launch-geometry hint is part of the ABI and refuses a null context"""
    from world_amd.api import header_abi_version, load_library
    lib = load_library(lib_path)
    text = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    want = int(re.search(r"#define\s+WORLD_HIP_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.world_hip_abi_version() == want == 6 == header_abi_version() == lib.abi_version
    assert int(re.search(r"#define\s+WORLD_HIP_HINT_SHARED_DEVICE\s+(\d+)", text).group(1)) == 1
    assert lib.world_hip_set_hint(None, 1) == -1


# ---- the Python binding reads its prototypes from the header (world_amd.api.header_prototypes / bind_from_header) ----------
def stripped_header():
    """include/world_hip.h without comments and preprocessor lines (this file's own reading, not the binding's)"""
    text = open(os.path.join(ROOT, "include", "world_hip.h")).read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


def declared_arities():
    """{name: number of parameters}, counted by commas"""
    out = {}
    for name, params in re.findall(r"\bWORLD_HIP_API\b[^;(]*?(\w+)\s*\(([^)]*)\)\s*;", stripped_header()):
        out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def test_the_reader_finds_every_declaration():
    from world_amd.api import header_prototypes
    tokens = len(re.findall(r"\bWORLD_HIP_API\b", stripped_header()))     # (its two #define lines are gone)
    protos = header_prototypes()
    assert len(protos) == tokens >= 134
    assert sorted(protos) == declared_symbols()
    assert {name: len(args) for name, (_, args) in protos.items()} == declared_arities()


def test_every_exported_symbol_is_fully_bound(lib_path):
    from world_amd.api import header_prototypes, load_library
    lib = load_library(lib_path)
    arity = declared_arities()
    for name, (restype, argtypes) in header_prototypes().items():
        fn = getattr(lib, name)                  # (test_library_exports_every_declared_symbol: all of them are there)
        assert fn.argtypes is not None and len(fn.argtypes) == arity[name], name
        assert list(fn.argtypes) == argtypes and fn.restype == restype, name


def test_pinned_prototypes_guard_the_type_map():
    from world_amd.api import HarvestOption, header_prototypes
    c, vp, i = ctypes, ctypes.c_void_p, ctypes.c_int
    p = header_prototypes()
    assert p["world_hip_harvest_batch"] == (i, [vp, i, i, vp, i, vp, c.POINTER(HarvestOption), i, vp, vp])
    assert p["world_hip_last_error"] == (c.c_char_p, [])
    assert p["world_hip_workspace_bytes"] == (c.c_ulonglong, [vp])
    assert p["world_hip_mcep_alpha"] == (c.c_double, [i])
    assert p["world_hip_destroy"] == (None, [vp])
    assert p["world_hip_check_shape"] == (i, [i, i, c.c_char_p, i])
    assert p["world_hip_analyze_sharded"][1][0] is i and p["world_hip_analyze_sharded"][1][11] is c.c_longlong
    assert p["world_hip_analyze_sharded"][1].count(c.c_longlong) == 1
    assert p["world_hip_set_error_handler"] == (None, [vp, vp])          # the function-pointer typedef
    assert p["world_hip_realtime_rng_jump"] == (None, [vp, c.c_ulonglong, vp])


def test_unknown_types_and_unparsable_declarations_fail_loudly():
    from world_amd.api import header_prototypes
    ok = "typedef struct { int a; } Opt;\nWORLD_HIP_API int fine(const Opt *o, unsigned long long n);\n"
    assert header_prototypes(ok)["fine"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_ulonglong])
    for text, word in ((ok + "WORLD_HIP_API int odd(int n, size_t bytes);", "size_t bytes"),
                       (ok + "WORLD_HIP_API float odd(int n);", "float"),
                       (ok + "WORLD_HIP_API int odd(const Unknown *p);", "Unknown"),
                       (ok + "WORLD_HIP_API int odd(int);", "odd"),
                       (ok + "WORLD_HIP_API int odd(void (*callback)(int), int n);", "odd"),
                       (ok + "WORLD_HIP_API int odd(int n) { return n; }", "odd"),
                       (ok + "WORLD_HIP_API int odd[4];", "odd")):
        with pytest.raises(ImportError, match=re.escape(word)):
            header_prototypes(text)


def test_a_missing_header_says_where_it_is_expected(tmp_path, monkeypatch):
    from world_amd import api
    monkeypatch.setattr(api, "HEADER_PATH", str(tmp_path / "include" / "world_hip.h"))
    monkeypatch.setattr(api, "_parsed", None)
    with pytest.raises(ImportError, match=re.escape(str(tmp_path / "include" / "world_hip.h"))):
        api.header_prototypes()


def test_struct_mirrors_match_the_header(tmp_path):
    """every ctypes.Structure of world_amd.api named like a typedef of the header: its size and every field's offset are
    what gcc gives the header's struct (field names and order from the Python class: one the header lacks does not compile)"""
    import subprocess
    from world_amd import api
    typedefs = set(re.findall(r"\}\s*(\w+)\s*;", stripped_header()))
    mirrors = {name: cls for name, cls in vars(api).items()
               if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and name in typedefs}
    assert len(mirrors) >= 14 and {"DioOption", "WorldHipMorphCurves", "WorldSynthesizer"} <= set(mirrors)
    lines, want = [], {}
    for name, cls in mirrors.items():
        want[name] = ctypes.sizeof(cls)
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            want[f"{name}.{field}"] = getattr(cls, field).offset
            lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "world_hip.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
