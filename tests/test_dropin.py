"""The drop-in layer's own behaviour (world_amd/csrc/dropin.inc): re-entrancy from host threads, the resident input
signal, chunked transfers through pinned staging, the error handler, and the context's small-array slabs and graph
generations.  CPU half: the host-compiled library (tests/emu); GPU half: libworld_hip.so through the C ABI.
Reference behaviour these mirror: the reference is re-entrant and stateless (src/cheaptrick.cpp:205-206,
src/d4c.cpp:345-346) and reads `x` afresh on every call."""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from backends import EMU_DIR, ROOT, emu_host as _emu

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_LIB = os.path.join(EMU_DIR, "libworld_emu.so")


def _signal(fs, seconds, seed):
    from world_amd import synth
    return np.ascontiguousarray(synth.utterance(seed, fs, seconds).numpy())


def _analyse(H, x, fs):
    tp, f0 = H.harvest(x, fs)
    fft = H.cheaptrick_fft_size(fs)
    return tp, f0, H.cheaptrick(x, fs, tp, f0, fft_size=fft), H.d4c(x, fs, tp, f0, fft)


def _stats(lib):
    a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
    lib.world_hip_dropin_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _separate_rows(H, name, x, fs, tp, f0, fft, *extra):
    """CheapTrick / D4C into rows that are SEPARATE allocations (test/test.cpp:148-151), not one dense block"""
    from world_amd.api import CheapTrickOption, D4COption
    nb = fft // 2 + 1
    rows = [np.full(nb + 3, np.nan) for _ in range(len(f0))]          # + 3: rows are neither adjacent nor equally spaced
    ptrs = (C.POINTER(C.c_double) * len(f0))(*[r.ctypes.data_as(C.POINTER(C.c_double)) for r in rows])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    if name == "CheapTrick":
        opt = CheapTrickOption(); H.lib.InitializeCheapTrickOption(fs, C.byref(opt)); opt.fft_size = fft
        H.lib.CheapTrick(dp(x), len(x), fs, dp(tp), dp(f0), len(f0), C.byref(opt), ptrs)
    else:
        opt = D4COption(); H.lib.InitializeD4COption(C.byref(opt))
        H.lib.D4C(dp(x), len(x), fs, dp(tp), dp(f0), len(f0), fft, C.byref(opt), ptrs)
    assert all(np.isnan(r[nb:]).all() for r in rows)                    # nothing written beyond a row
    return np.stack([r[:nb] for r in rows])


def _check_threads(H, fs, seconds, n_threads, rounds):
    xs = [_signal(fs, seconds, 10 + i) for i in range(n_threads)]
    serial = [_analyse(H, x, fs) for x in xs]
    out = [[None] * rounds for _ in range(n_threads)]
    errors = []

    def work(i):
        try:
            for r in range(rounds):
                out[i][r] = _analyse(H, xs[i], fs)
        except Exception as e:                                          # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(n_threads)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    assert not errors, errors
    for i in range(n_threads):
        for r in range(rounds):
            for a, b in zip(out[i][r], serial[i]):
                assert np.array_equal(a, b), f"thread {i} round {r}"
    return dt, xs


# ---------------------------------------------------------------------------------------------------------
# CPU: the host-compiled library
# ---------------------------------------------------------------------------------------------------------
def test_emulated_dropin_calls_from_four_host_threads_are_bit_identical():
    H = _emu()
    _check_threads(H, 16000, 0.25, 4, 2)
    slots, hits, misses = _stats(H.lib)
    assert 1 <= slots <= 4 and hits > 0


def test_emulated_resident_signal_follows_an_in_place_edit():
    """Harvest(x) -> edit ONE sample of x in place -> CheapTrick(x) must analyse the edited signal (the content hash
    covers every sample), and an unchanged x must be found resident"""
    H = _emu()
    fs = 16000
    x = _signal(fs, 0.3, 5)
    tp, f0 = H.harvest(x, fs)
    fft = H.cheaptrick_fft_size(fs)
    _, h0, m0 = _stats(H.lib)
    sp = H.cheaptrick(x, fs, tp, f0, fft_size=fft)
    _, h1, m1 = _stats(H.lib)
    assert h1 == h0 + 1 and m1 == m0                                    # same pointer, length, content: no upload
    x[len(x) // 2] += 0.25                                              # one sample, in place
    sp_edit = H.cheaptrick(x, fs, tp, f0, fft_size=fft)
    _, h2, m2 = _stats(H.lib)
    assert m2 == m1 + 1                                                 # uploaded again
    fresh = H.cheaptrick(x.copy(), fs, tp, f0, fft_size=fft)            # another pointer: certainly uploaded
    assert np.array_equal(sp_edit, fresh) and not np.array_equal(sp_edit, sp)


def test_emulated_separate_rows_match_dense_rows():
    H = _emu()
    fs = 16000
    x = _signal(fs, 0.4, 7)
    tp, f0, sp, ap = _analyse(H, x, fs)
    fft = H.cheaptrick_fft_size(fs)
    assert np.array_equal(_separate_rows(H, "CheapTrick", x, fs, tp, f0, fft), sp)
    assert np.array_equal(_separate_rows(H, "D4C", x, fs, tp, f0, fft), ap)


HANDLER = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p, C.c_void_p)


def _check_error_handler(H):
    """a shape the GPU path refuses reaches the installed handler, the process survives, the outputs stay untouched,
    and the library works afterwards"""
    seen = []
    cb = HANDLER(lambda fn, msg, user: seen.append((fn.decode(), msg.decode())))
    H.lib.world_hip_set_error_handler(cb, None)
    try:
        fs = 16000
        x = _signal(fs, 0.2, 3)
        tp, f0 = H.harvest(x, fs)
        from world_amd.api import CheapTrickOption
        opt = CheapTrickOption(); H.lib.InitializeCheapTrickOption(fs, C.byref(opt))
        opt.fft_size = 1000                                             # not a power of two: refused before any GPU work
        sp = np.full((len(f0), 501), -7.0)
        from world_amd.api import _rows, _p
        H.lib.CheapTrick(_p(x), len(x), fs, _p(tp), _p(f0), len(f0), C.byref(opt), _rows(sp))
        assert len(seen) == 1 and seen[0][0] == "CheapTrick" and "fft_size 1000" in seen[0][1]
        assert np.all(sp == -7.0)
        ap = np.full((len(f0), 513), -7.0)
        from world_amd.api import D4COption
        dopt = D4COption(); H.lib.InitializeD4COption(C.byref(dopt))
        H.lib.D4C(_p(x), len(x), 8000, _p(tp), _p(f0), len(f0), 1024, C.byref(dopt), _rows(ap))   # fs below D4C's floor
        assert len(seen) == 2 and seen[1][0] == "D4C" and "15.8 kHz" in seen[1][1]
        assert np.all(ap == -7.0)
        fft = H.cheaptrick_fft_size(fs)
        assert np.isfinite(H.cheaptrick(x, fs, tp, f0, fft_size=fft)).all()   # the library still works
        assert len(seen) == 2
    finally:
        H.lib.world_hip_set_error_handler(HANDLER(0), None)
    return cb


def test_emulated_error_handler_receives_shape_refusals():
    _check_error_handler(_emu())


# (fs, fft_size) pairs on both sides of the rule of DESIGN.md 7: the reference sizes its buffers by fft_size and fills
# them by fs, so an unvoiced frame's 500 Hz window (CheapTrick) and the unvoiced pulse spacing (Synthesis, the real-time
# synthesiser) must fit fft_size.  Refused pairs name the smallest fft_size that works.
CT_REFUSED = [(48000, 256, 512), (192000, 1024, 2048), (44100, 256, 512)]
CT_ACCEPTED = [(48000, 512), (16000, 128), (8000, 128)]
SY_REFUSED = [(96000, 128, 256), (192000, 256, 512)]
SY_ACCEPTED = [(96000, 256), (16000, 128)]


def _check_pair_refusals(H):
    """CheapTrick(), Synthesis() and InitializeSynthesizer() refuse the pairs the reference leaves undefined, through the
    error handler and with the outputs untouched, and serve the pairs next to them"""
    from world_amd.api import CheapTrickOption, WorldSynthesizer, _p, _rows
    seen = []
    cb = HANDLER(lambda fn, msg, user: seen.append((fn.decode(), msg.decode())))
    H.lib.world_hip_set_error_handler(cb, None)
    try:
        nf = 8
        tp = np.arange(nf) * 0.005
        f0 = np.array([0.0, 0.0, 150.0, 160.0, 0.0, 170.0, 0.0, 0.0])
        for fs, fft, smallest in CT_REFUSED:
            x = _signal(fs, 0.04, 3)
            opt = CheapTrickOption(); H.lib.InitializeCheapTrickOption(fs, C.byref(opt)); opt.fft_size = fft
            sp = np.full((nf, fft // 2 + 1), -7.0)
            del seen[:]
            H.lib.CheapTrick(_p(x), len(x), fs, _p(tp), _p(f0), nf, C.byref(opt), _rows(sp))
            assert len(seen) == 1 and seen[0][0] == "CheapTrick", (fs, fft, seen)
            assert f"smallest fft_size for this fs is {smallest}" in seen[0][1], seen
            assert np.all(sp == -7.0)
        for fs, fft in CT_ACCEPTED:
            x = _signal(fs, 0.04, 3)
            del seen[:]
            sp = H.cheaptrick(x, fs, tp, f0, fft_size=fft)
            assert not seen and np.isfinite(sp).all() and np.all(sp > 0), (fs, fft, seen)
        for fs, fft, smallest in SY_REFUSED:
            nb = fft // 2 + 1
            y = np.full(int(fs * 0.03), -7.0)
            del seen[:]
            H.lib.Synthesis(_p(f0), nf, _rows(np.full((nf, nb), 1e-4)), _rows(np.full((nf, nb), 0.5)), fft, 5.0, fs, len(y), _p(y))
            assert len(seen) == 1 and seen[0][0] == "Synthesis", (fs, fft, seen)
            assert f"smallest fft_size for this fs is {smallest}" in seen[0][1], seen
            assert np.all(y == -7.0)
            s = WorldSynthesizer()
            H._rt().InitializeSynthesizer(fs, 5.0, fft, 64, 8, C.byref(s))
            assert len(seen) == 2 and seen[1][0] == "InitializeSynthesizer" and f"is {smallest}" in seen[1][1], seen
        for fs, fft in SY_ACCEPTED:
            nb = fft // 2 + 1
            del seen[:]
            y = H.synthesis(f0, np.full((nf, nb), 1e-4), np.full((nf, nb), 0.5), fft, 5.0, fs, int(fs * 0.03))
            assert not seen and np.isfinite(y).all() and np.any(y != 0.0), (fs, fft, seen)
            s = H.initialize_synthesizer(fs, 5.0, fft, 64, 8)
            assert not seen
            H.destroy_synthesizer(s)
    finally:
        H.lib.world_hip_set_error_handler(HANDLER(0), None)
    return cb


def test_emulated_pairs_of_fs_and_fft_size_the_reference_leaves_undefined_are_refused():
    H = _emu()
    _check_pair_refusals(H)
    why = C.create_string_buffer(256)
    for fs, fft, smallest in CT_REFUSED:
        assert H.lib.world_hip_check_shape(fs, fft, why, 256) == 1 and str(smallest).encode() in why.value
    assert H.lib.world_hip_check_shape(48000, 512, why, 256) == 0 and H.lib.world_hip_check_shape(16000, 128, why, 256) == 0


def test_default_error_policy_prints_and_aborts():
    """no handler installed: the reason on stderr, then abort() -- never a silent CPU result"""
    _emu()
    code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r)\n"
            "from world_amd.api import HostAPI\n"
            "H = HostAPI(%r)\n"
            "x = np.zeros(4000); tp = np.zeros(41); f0 = np.zeros(41)\n"
            "H.cheaptrick(x, 16000, tp, f0, fft_size=1000)\n"
            "print('survived')\n" % (ROOT, EMU_LIB))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "survived" not in r.stdout
    assert "libworld_hip: CheapTrick failed" in r.stderr and "fft_size 1000" in r.stderr


def _slab_stress(lib_path, env_extra, out):
    env = dict(os.environ, **env_extra)
    subprocess.run([sys.executable, os.path.join(HERE, "slab_stress.py"), lib_path, out], check=True, env=env, timeout=1500)
    return np.load(out)


def test_emulated_small_array_slabs_chain_and_recycle(tmp_path):
    """distinct length vectors beyond one slab must never invalidate pointers a call already holds.  The same
    ragged batched calls with (a) the default 4 MB slab, (b) 1 KB slabs that chain after every few arrays, (c) a budget of
    one byte, which drops the whole set at the start of every stage: identical results"""
    _emu()
    a = _slab_stress(EMU_LIB, {}, str(tmp_path / "a.npz"))
    b = _slab_stress(EMU_LIB, {"WORLD_HIP_SMALL_SLAB": "1024"}, str(tmp_path / "b.npz"))
    c = _slab_stress(EMU_LIB, {"WORLD_HIP_SMALL_SLAB": "512", "WORLD_HIP_SMALL_BUDGET": "1"}, str(tmp_path / "c.npz"))
    for k in a.files:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert int(b["slabs"]) == int(a["slabs"])                          # (bookkeeping value only: same call count)
    # Harvest's zero-crossing lists exist for one GROUP of utterances at a time (harvest.hip: launch_harvest): groups of one
    # and of two utterances (the batches have three: a ragged last group) give the same records as the whole batch at once
    d = _slab_stress(EMU_LIB, {"WORLD_HIP_EVENT_GROUP": "1"}, str(tmp_path / "d.npz"))
    e = _slab_stress(EMU_LIB, {"WORLD_HIP_EVENT_GROUP": "2"}, str(tmp_path / "e.npz"))
    for k in a.files:
        assert np.array_equal(a[k], d[k]) and np.array_equal(a[k], e[k]), k


def _lifecycle(lib_path, env_extra, out, *args):
    env = dict(os.environ, WORLD_HIP_DROPIN_COPY_MIN_BYTES="4096", **env_extra)     # the helper threads take part in these small copies
    subprocess.run([sys.executable, os.path.join(HERE, "dropin_lifecycle.py"), lib_path, out, *args], check=True, env=env, timeout=900)
    return np.load(out)


def _check_lifecycle(lib_path, tmp_path, fork):
    a = _lifecycle(lib_path, {}, str(tmp_path / "a.npz"), *(["fork"] if fork else []))
    # world_hip_shutdown(): everything released, and a cold restart computes the same arrays
    assert int(a["shutdown_rc"]) == 0 and int(a["slots_before"]) >= 1 and int(a["slots_after"]) == 0
    for k in ("tp", "f0", "sp", "ap"):
        assert np.array_equal(a[k], a[k + "2"]), k
    if fork:
        assert int(a["child"]) == 0, f"the forked child's analysis: status {int(a['child'])}"
    # WORLD_HIP_DROPIN_WIRE=f32: the rows cross as float and are widened on the host -- the f64 rows rounded ONCE
    b = _lifecycle(lib_path, {"WORLD_HIP_DROPIN_WIRE": "f32"}, str(tmp_path / "b.npz"))
    assert np.array_equal(a["tp"], b["tp"]) and np.array_equal(a["f0"], b["f0"])
    assert np.array_equal(b["sp"], a["sp"].astype(np.float32).astype(np.float64))
    assert np.array_equal(b["ap"], a["ap"].astype(np.float32).astype(np.float64))
    # ... the same with the rows travelling range by range (both stages) and with helpers that never spin / no helpers
    c = _lifecycle(lib_path, {"WORLD_HIP_DROPIN_WIRE": "f32", "WORLD_HIP_DROPIN_RANGES": "2", "WORLD_HIP_DROPIN_SPIN_US": "0"},
                   str(tmp_path / "c.npz"))
    d = _lifecycle(lib_path, {"WORLD_HIP_DROPIN_RANGES": "2", "WORLD_HIP_DROPIN_COPY_THREADS": "0"}, str(tmp_path / "d.npz"))
    assert np.array_equal(c["sp"], b["sp"]) and np.array_equal(c["ap"], b["ap"])
    assert np.array_equal(d["sp"], a["sp"]) and np.array_equal(d["ap"], a["ap"])


def test_emulated_dropin_shutdown_restart_fork_and_narrow_wire(tmp_path):
    """VERDICT r04 item 7 / ADVICE r04: world_hip_shutdown() joins the helpers and frees the slots (and the next call starts
    over, same results); a child forked after drop-in calls runs its own analysis (fresh copy pool and slots: the parent's
    threads do not exist there); WORLD_HIP_DROPIN_WIRE=f32 returns the f64 rows rounded once to float."""
    _emu()
    _check_lifecycle(EMU_LIB, tmp_path, fork=True)


@pytest.mark.gpu
def test_dropin_shutdown_restart_and_narrow_wire_on_the_gpu(tmp_path):
    from world_amd.api import LIB_PATH
    _check_lifecycle(LIB_PATH, tmp_path, fork=False)          # (a forked child cannot use the parent's HIP runtime at all)


# ---------------------------------------------------------------------------------------------------------
# GPU: libworld_hip.so
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_concurrent_dropin_calls_from_host_threads(tmp_path):
    """four host threads through Harvest + CheapTrick + D4C at once -- bit-identical to serial calls
    (Python threads: the GIL is released inside the library), and, timed from a plain C++ caller the way the reference's
    users call the library (examples/dropin_bench.cpp: separately allocated rows), more than 1.5 x the aggregate
    throughput of one thread doing the same work"""
    import json
    from world_amd import build as hip_build, synth
    from world_amd.api import HostAPI
    H = HostAPI()
    fs = 48000
    _check_threads(H, fs, 2.0, 4, 2)
    slots, hits, _ = _stats(H.lib)
    assert slots >= 2 and hits > 0
    exe = os.path.join(ROOT, "examples", "dropin_bench")
    if not os.path.exists(exe):
        hip_build.build_examples()
    xf = tmp_path / "x.f64"
    synth.vowel(fs, 10.0, seed=12345).numpy().astype(np.float64).tofile(str(xf))
    r = subprocess.run([exe, str(xf), str(fs), "8", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(d)
    assert d["all_results_identical"] and d["frames"] == 2001
    assert d["separate_rows_ms"] / d["threads_ms_per_utterance"] > 1.5, d
    assert d["fresh_rows_ms"] < 3.0 * d["separate_rows_ms"], d         # a single thread on new buffers creates no new slots


@pytest.mark.gpu
def test_resident_signal_follows_an_in_place_edit_on_the_gpu():
    from world_amd.api import HostAPI
    H = HostAPI()
    fs = 48000
    x = _signal(fs, 1.0, 5)
    tp, f0 = H.harvest(x, fs)
    fft = H.cheaptrick_fft_size(fs)
    sp = H.cheaptrick(x, fs, tp, f0, fft_size=fft)
    ap = H.d4c(x, fs, tp, f0, fft)
    x[len(x) // 3] += 0.25
    sp_edit, ap_edit = H.cheaptrick(x, fs, tp, f0, fft_size=fft), H.d4c(x, fs, tp, f0, fft)
    x2 = x.copy()
    assert np.array_equal(sp_edit, H.cheaptrick(x2, fs, tp, f0, fft_size=fft)) and not np.array_equal(sp_edit, sp)
    assert np.array_equal(ap_edit, H.d4c(x2, fs, tp, f0, fft)) and not np.array_equal(ap_edit, ap)


@pytest.mark.gpu
def test_separate_rows_match_dense_rows_on_the_gpu(ref_oracle):
    """2001 separately allocated rows (the reference's own calling convention) through the chunked, double-buffered
    D2H and the helper threads == one dense matrix == the reference"""
    from world_amd.api import HostAPI
    from util import max_rel
    H = HostAPI()
    fs = 48000
    x = _signal(fs, 10.0, 2)
    tp, f0, sp, ap = _analyse(H, x, fs)
    fft = H.cheaptrick_fft_size(fs)
    assert np.array_equal(_separate_rows(H, "CheapTrick", x, fs, tp, f0, fft), sp)
    assert np.array_equal(_separate_rows(H, "D4C", x, fs, tp, f0, fft), ap)
    tp_r, f0_r = ref_oracle.harvest(x, fs)
    assert np.array_equal(tp, tp_r) and np.array_equal(f0 > 0, f0_r > 0)
    assert max_rel(sp, ref_oracle.cheaptrick(x, fs, tp_r, f0_r, fft_size=fft)) <= 1e-4
    assert max_rel(ap, ref_oracle.d4c(x, fs, tp_r, f0_r, fft)) <= 1e-4


@pytest.mark.gpu
def test_error_handler_receives_shape_refusals_on_the_gpu():
    from world_amd.api import HostAPI
    _check_error_handler(HostAPI())


@pytest.mark.gpu
def test_pairs_of_fs_and_fft_size_the_reference_leaves_undefined_are_refused_on_the_gpu():
    from world_amd.api import HostAPI
    _check_pair_refusals(HostAPI())


@pytest.mark.gpu
def test_small_array_slabs_chain_and_recycle_on_the_gpu(tmp_path):
    from world_amd.api import LIB_PATH
    a = _slab_stress(LIB_PATH, {}, str(tmp_path / "a.npz"))
    b = _slab_stress(LIB_PATH, {"WORLD_HIP_SMALL_SLAB": "1024"}, str(tmp_path / "b.npz"))
    c = _slab_stress(LIB_PATH, {"WORLD_HIP_SMALL_SLAB": "512", "WORLD_HIP_SMALL_BUDGET": "1"}, str(tmp_path / "c.npz"))
    for k in a.files:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


@pytest.mark.gpu
def test_stale_graph_is_refused_not_replayed():
    """a captured job whose context later had to reallocate (a larger batch grows the arena) must not be
    replayed into freed memory: graph_launch fails with "stale graph"; re-captured, it runs and is bit-identical"""
    import torch
    from world_amd import synth
    from world_amd.api import WorldHip, cheaptrick_fft_size, frame_count
    fs = 48000
    nb = cheaptrick_fft_size(fs) // 2 + 1
    wh = WorldHip()
    x1 = synth.utterance(2, fs, 0.6)[None].cuda().contiguous()
    b1 = torch.zeros((frame_count(fs, x1.shape[1], 5.0), 2 + 2 * nb), dtype=torch.float64, device="cuda")
    xb = torch.stack([synth.utterance(i, fs, 1.5) for i in range(4)]).cuda().contiguous()
    bb = torch.zeros((4 * frame_count(fs, xb.shape[1], 5.0), 2 + 2 * nb), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        wh.analyze_packed(x1, fs, b1)
        wh.analyze_packed(x1, fs, b1)
        torch.cuda.synchronize()
        ref = b1.clone()
        g = wh.capture(lambda: wh.analyze_packed(x1, fs, b1))
        b1.fill_(-3.0); g.launch(); torch.cuda.synchronize()
        assert torch.equal(b1, ref)
        wh.analyze_packed(x1, fs, b1)                       # the same shape again: nothing moves, the graph stays valid
        g.launch(); torch.cuda.synchronize()
        wh.analyze_packed(xb, fs, bb)                       # a larger job: the arena is regrown
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="stale graph"):
            g.launch()
        g.close()
        wh.analyze_packed(x1, fs, b1)
        g2 = wh.capture(lambda: wh.analyze_packed(x1, fs, b1))
        b1.fill_(-3.0); g2.launch(); torch.cuda.synchronize()
        assert torch.equal(b1, ref)
        g2.close()


def _check_cheaptrick_8192(H, oracle, cases):
    from util import max_rel
    from world_amd import synth
    for fs, seconds, floor in cases:
        x = synth.vowel(fs, seconds, seed=31, base_f0=120.0).numpy()
        tp, f0 = oracle.harvest(x, fs)
        fft = H.cheaptrick_fft_size(fs, floor)
        assert fft == 8192
        sp = H.cheaptrick(x, fs, tp, f0, f0_floor=floor, fft_size=fft)
        sp_o = oracle.cheaptrick(x, fs, tp, f0, f0_floor=floor, fft_size=fft)
        assert sp.shape == sp_o.shape == (len(f0), 4097)
        assert max_rel(sp, sp_o) <= 1e-6, (fs, floor, max_rel(sp, sp_o))


def test_emulated_cheaptrick_fft_size_8192(port_oracle):
    """the reference takes any power of two (src/cheaptrick.cpp:200-229); fft_size 8192 -- f0 floors below
    35 Hz at 48 kHz, default options above 96 kHz -- used to be refused"""
    _check_cheaptrick_8192(_emu(), port_oracle, [(48000, 0.12, 30.0)])


@pytest.mark.gpu
def test_cheaptrick_fft_size_8192_on_the_gpu(ref_oracle):
    from world_amd.api import HostAPI
    _check_cheaptrick_8192(HostAPI(), ref_oracle, [(48000, 0.6, 30.0), (96000, 0.4, 40.0), (192000, 0.25, 71.0)])


def _check_frame_ranges(lib_path, device):
    """the stages' rows of a frame range == the same rows of the whole call, bit for bit (dense and packed, both wire
    formats; with and without reusing the offsets of the previous call)"""
    from world_amd import synth
    from world_amd.api import CheapTrickOption, D4COption, HarvestOption, cheaptrick_fft_size, frame_count, load_library
    L = load_library(lib_path)
    fs = 16000
    fft = cheaptrick_fft_size(fs)
    nb = fft // 2 + 1
    xs = [synth.utterance(6, fs, 0.9).numpy(), synth.utterance(9, fs, 0.55).numpy()]
    B, Lmax = 2, max(len(x) for x in xs)
    xh = np.zeros((B, Lmax)); [xh[i].__setitem__(slice(0, len(x)), x) for i, x in enumerate(xs)]
    xl = np.array([len(x) for x in xs], dtype=np.int32)
    nf = np.array([frame_count(fs, int(n), 5.0) for n in xl], dtype=np.int32)
    F = int(nf.max())
    if device:
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        host = lambda t: t.cpu().numpy()
        ptr = lambda t: t.data_ptr()
        sync = torch.cuda.synchronize
    else:
        up = lambda a: np.ascontiguousarray(a).copy()
        host = lambda a: a
        ptr = lambda a: a.ctypes.data
        sync = lambda: None
    ip = C.POINTER(C.c_int)
    ctx = L.world_hip_create(0, None)
    try:
        x = up(xh)
        tp, f0 = up(np.zeros((B, F))), up(np.zeros((B, F)))
        h, c, d = HarvestOption(71.0, 800.0, 5.0), CheapTrickOption(-0.15, 71.0, fft), D4COption(0.85)
        args = (ctx, B, fs, ptr(x), Lmax, xl.ctypes.data_as(ip))
        assert L.world_hip_harvest_batch(*args, C.byref(h), F, ptr(tp), ptr(f0)) == 0
        sp, ap = up(np.full((B, F, nb), -1.0)), up(np.full((B, F, nb), -1.0))
        assert L.world_hip_cheaptrick_batch(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), C.byref(c), ptr(sp)) == 0
        assert L.world_hip_d4c_batch(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), fft, C.byref(d), ptr(ap)) == 0
        sync()
        sp_full, ap_full = host(sp).copy(), host(ap).copy()
        # dense rows, three ranges, the second and third reusing the first call's offsets / LoveTrain pass
        sp2, ap2 = up(np.full((B, F, nb), -1.0)), up(np.full((B, F, nb), -1.0))
        cuts = [(64, 128), (0, 64), (128, 1 << 30)]
        for i, (lo, hi) in enumerate(cuts):
            assert L.world_hip_cheaptrick_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), C.byref(c), lo, hi, int(i > 0), ptr(sp2)) == 0
        for i, (lo, hi) in enumerate(cuts):
            assert L.world_hip_d4c_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), fft, C.byref(d), lo, hi, int(i > 0), ptr(ap2)) == 0
        sync()
        assert np.array_equal(host(sp2), sp_full) and np.array_equal(host(ap2), ap_full)
        # packed records of a range that cuts through both utterances
        lo, hi = 70, 150
        rows = int(sum(min(hi, n) - min(lo, n) for n in nf))
        for wire in (0, 1):
            cols = L.world_hip_record_columns(fft, wire)
            block = up(np.full((rows + 2, cols), np.nan))
            rc = L.world_hip_spectral_packed_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), C.byref(c), C.byref(d), lo, hi,
                                                   0, 1, ptr(block), cols)
            assert rc == 0, L.world_hip_last_error().decode()
            sync()
            rec = host(block)
            assert np.isnan(rec[0]).all() and np.isnan(rec[rows + 1]).all()          # nothing outside [first_row, first_row + rows)
            row = 1
            tph, f0h = host(tp), host(f0)
            for u in range(B):
                a, b = min(lo, int(nf[u])), min(hi, int(nf[u]))
                r = rec[row:row + b - a]
                assert np.array_equal(r[:, 0], tph[u, a:b]) and np.array_equal(r[:, 1], f0h[u, a:b])
                if wire == 0:
                    assert np.array_equal(r[:, 2:2 + nb], sp_full[u, a:b]) and np.array_equal(r[:, 2 + nb:], ap_full[u, a:b])
                else:
                    f32 = np.ascontiguousarray(r[:, 2:]).view(np.float32)
                    assert np.array_equal(f32[:, :nb], sp_full[u, a:b].astype(np.float32))
                    assert np.array_equal(f32[:, nb:2 * nb], ap_full[u, a:b].astype(np.float32))
                row += b - a
            assert row == 1 + rows
        # ranges of the two stages ALTERNATING while reusing: their prepared arrays occupy disjoint workspace
        sp3, ap3 = up(np.full((B, F, nb), -1.0)), up(np.full((B, F, nb), -1.0))
        for i, (lo, hi) in enumerate(cuts):
            assert L.world_hip_cheaptrick_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), C.byref(c), lo, hi, int(i > 0), ptr(sp3)) == 0
            assert L.world_hip_d4c_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), fft, C.byref(d), lo, hi, int(i > 0), ptr(ap3)) == 0
        sync()
        assert np.array_equal(host(sp3), sp_full) and np.array_equal(host(ap3), ap_full)
        # ... and packed sub-ranges reusing what the first one prepared (what a rank of analyze_long_sharded does)
        cols = L.world_hip_record_columns(fft, 0)
        tot = int(nf.sum())
        block = up(np.full((tot, cols), np.nan))
        row = 0
        for i, (lo, hi) in enumerate(sorted(cuts)):
            rc = L.world_hip_spectral_packed_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), C.byref(c), C.byref(d), lo, hi,
                                                   int(i > 0), row, ptr(block), cols)
            assert rc == 0, L.world_hip_last_error().decode()
            row += int(sum(min(hi, n) - min(lo, n) for n in nf))
        sync()
        rec, row = host(block), 0
        for lo, hi in sorted(cuts):
            for u in range(B):
                a, b = min(lo, int(nf[u])), min(hi, int(nf[u]))
                assert np.array_equal(rec[row:row + b - a, 2:2 + nb], sp_full[u, a:b])
                assert np.array_equal(rec[row:row + b - a, 2 + nb:], ap_full[u, a:b])
                row += b - a
        # reuse is CHECKED, not trusted: another stage in between, other buffers or another option -> an error, not garbage
        def refused(rc):
            return rc != 0 and b"reuse_offsets" in L.world_hip_last_error()
        assert L.world_hip_harvest_batch(*args, C.byref(h), F, ptr(tp), ptr(f0)) == 0            # overwrites the workspace
        assert refused(L.world_hip_cheaptrick_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), C.byref(c), 0, 8, 1, ptr(sp3)))
        assert refused(L.world_hip_d4c_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), fft, C.byref(d), 0, 8, 1, ptr(ap3)))
        assert L.world_hip_d4c_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), fft, C.byref(d), 0, 8, 0, ptr(ap3)) == 0
        f0_other = up(host(f0).copy())
        assert refused(L.world_hip_d4c_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0_other), fft, C.byref(d), 8, 16, 1, ptr(ap3)))
        d_other = D4COption(0.5)
        assert refused(L.world_hip_d4c_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), fft, C.byref(d_other), 8, 16, 1, ptr(ap3)))
        assert L.world_hip_d4c_batch_range(*args, nf.ctypes.data_as(ip), F, ptr(tp), ptr(f0), fft, C.byref(d), 8, 16, 1, ptr(ap3)) == 0
        sync()
        assert np.array_equal(host(ap3)[:, :16], ap_full[:, :16])
    finally:
        L.world_hip_destroy(ctx)


def test_emulated_frame_ranges_are_bit_identical_to_the_whole_call():
    _emu()
    _check_frame_ranges(EMU_LIB, device=False)


@pytest.mark.gpu
def test_frame_ranges_are_bit_identical_to_the_whole_call_on_the_gpu():
    from world_amd.api import LIB_PATH
    _check_frame_ranges(LIB_PATH, device=True)


@pytest.mark.gpu
def test_long_utterance_frames_sharded_on_one_gpu():
    """world_amd.distributed.analyze_long_sharded without a process group (one rank owns every frame; sub-ranges of 512
    frames): a 12 s utterance, bit-identical to WorldHip.analyze"""
    import torch
    from world_amd import distributed as wd, synth
    from world_amd.api import WorldHip
    fs = 48000
    x = torch.cat([synth.utterance(40 + i, fs, 4.0) for i in range(3)]).cuda()
    tp, f0, sp, ap = wd.analyze_long_sharded(x, fs, sub_frames=512)
    tp1, f01, sp1, ap1, nf1 = WorldHip().analyze(x[None].contiguous(), fs)
    k = int(nf1[0])
    assert tp.shape[0] == k and torch.equal(tp, tp1[0, :k]) and torch.equal(f0, f01[0, :k])
    assert torch.equal(sp, sp1[0, :k]) and torch.equal(ap, ap1[0, :k])
