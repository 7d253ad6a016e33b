"""Real-time synthesis on the GPU (reference src/synthesisrealtime.cpp): the drop-in WorldSynthesizer symbols and the
batched world_hip_realtime_* streams of libworld_hip.so against the unmodified reference's recordings
(tests/golden/realtime.npz) and against each other."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_realtime_cpu import FIX, NAMES, _lone_run, _stream_plans, check_against_fixture, plan_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from world_amd.api import HostAPI
    return HostAPI()


@pytest.fixture(scope="module")
def wh():
    import torch
    from world_amd.api import WorldHip
    assert torch.cuda.is_available()
    w = WorldHip(device=0)
    yield w
    w.close()


@pytest.mark.parametrize("name", NAMES)
def test_realtime_reproduces_the_reference(hip, name):
    check_against_fixture(hip.realtime_plan(plan_of(name)), name, 1e-10)


def test_small_and_large_render_batches_give_the_same_buffers(hip):
    """"Synthesis 2" (every frame at once: the whole utterance renders in one batch) and "Synthesis 3" (one frame per
    add: a small batch every few calls) of the same parameters"""
    a = hip.realtime_plan(plan_of("all_at_once"))["out"]
    b = hip.realtime_plan(plan_of("frame_by_frame"))["out"]
    assert a.size > 0 and np.array_equal(a, b)


def test_one_pulse_at_a_time_equals_render_ahead(hip, monkeypatch):
    """batches of one pulse render no further than each call's buffer needs (no render-ahead): same control, same bits"""
    ahead = hip.realtime_plan(plan_of("random_chunks_48k"))
    monkeypatch.setenv("WORLD_HIP_REALTIME_BATCH_PULSES", "1")
    single = hip.realtime_plan(plan_of("random_chunks_48k"))
    assert np.array_equal(ahead["calls"], single["calls"]) and np.array_equal(ahead["out"], single["out"])
    check_against_fixture(single, "random_chunks_48k", 1e-10)


def _run_streams(wh, plans, fs, fft, bs, P, profile=False):
    """every stream follows its own chunk plan; one synthesize() per round until nothing is produced.  Returns outputs per
    stream and, with profile, the kernel launches of each synthesize() call"""
    import torch
    rt = wh.realtime(len(plans), fs, 5.0, fft, bs, P)
    dev = [(torch.from_numpy(sp).cuda(), torch.from_numpy(ap).cuda()) for _, sp, ap, _ in plans]
    outs = [[] for _ in plans]
    pos, k = [0] * len(plans), [0] * len(plans)
    launches = []
    try:
        while True:
            busy = False
            for s, (f0, _, _, chunks) in enumerate(plans):
                if k[s] < len(chunks):
                    n = chunks[k[s]]
                    if rt.add(s, f0[pos[s]:pos[s] + n], dev[s][0][pos[s]:], dev[s][1][pos[s]:]) == 1:
                        pos[s] += n
                        k[s] += 1
                    busy = True
            while True:
                if profile:
                    got = {}
                    prof = wh.profile(lambda: got.setdefault("r", rt.synthesize()))
                    launches.append(sum(len(v) for v in prof.values()))
                    out, produced = got["r"]
                else:
                    out, produced = rt.synthesize()
                host = out.cpu().numpy()
                for s in np.nonzero(produced)[0]:
                    outs[s].append(host[s].copy())
                if not produced.any():
                    break
            if not busy:
                break
    finally:
        rt.close()
    return [np.concatenate(o) if o else np.zeros(0) for o in outs], launches


@pytest.mark.parametrize("n", [1, 7, 64])
def test_batched_streams_match_lone_synthesizers(hip, wh, n):
    fs, fft, bs, P = 48000, 2048, 256, 16
    plans = _stream_plans(n, fs, fft, 24, seed=n)
    got, _ = _run_streams(wh, plans, fs, fft, bs, P)
    for s, plan in enumerate(plans):
        want = _lone_run(hip, plan, fs, fft, bs, P)
        assert want.size > 0 and np.array_equal(got[s], want), f"stream {s} of {n}"


def test_streams_beyond_one_render_batch(hip, wh, monkeypatch):
    """8 streams each add a whole utterance in one call; their pulses need many render batches (the limit is lowered to 5
    pulses, fewer than the streams' next buffers need together): every stream still gets its lone synthesiser's output"""
    monkeypatch.setenv("WORLD_HIP_REALTIME_BATCH_PULSES", "5")
    fs, fft, bs, P = 48000, 2048, 256, 4
    plans = [(f0, sp, ap, [len(f0)]) for f0, sp, ap, _ in _stream_plans(8, fs, fft, 200, seed=3)]
    got, launches = _run_streams(wh, plans, fs, fft, bs, P, profile=True)
    assert launches[0] > 2                            # the first call rendered in more than one batch
    monkeypatch.delenv("WORLD_HIP_REALTIME_BATCH_PULSES")
    for s, plan in enumerate(plans):
        want = _lone_run(hip, plan, fs, fft, bs, P)
        assert want.size > 0 and np.array_equal(got[s], want), f"stream {s}"


def test_drop_in_synthesizer_across_shutdown(tmp_path):
    """world_hip_shutdown() in the middle of a stream leaves the synthesiser working (it owns its context).  (The fork
    half runs on the emulated library: test_realtime_cpu.py; a forked child cannot use the parent's HIP runtime.)"""
    from world_amd.api import LIB_PATH
    out = str(tmp_path / "lc.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "realtime_lifecycle.py"), LIB_PATH, out], check=True,
                   timeout=600)
    r = np.load(out)
    assert int(r["shutdown_rc"]) == 0 and r["first"].size > 0
    assert np.array_equal(r["first"], r["second"])


def test_launches_per_synthesize_do_not_depend_on_the_stream_count(wh):
    fs, fft, bs, P = 48000, 2048, 256, 16
    base = _stream_plans(1, fs, fft, 24, seed=5)[0]
    counts = {}
    for n in (1, 7, 64):
        _, launches = _run_streams(wh, [base] * n, fs, fft, bs, P, profile=True)
        counts[n] = launches
    assert counts[1] == counts[7] == counts[64], counts
    assert max(counts[1]) <= 2 and sum(counts[1]) > 0


FRESH = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from world_amd.api import HostAPI
from test_realtime_cpu import plan_of
np.save({out!r}, HostAPI().realtime_plan(plan_of("hop10_22k"))["out"])
"""


def test_hostile_parameters_return_and_leave_no_trace(hip, tmp_path):
    base = plan_of("hop10_22k")
    f0, sp, ap = base["f0"].copy(), base["sp"].copy(), base["ap"].copy()
    hostile = []
    for what in ("nan_f0", "inf_f0", "huge_f0", "nan_sp", "inf_sp", "nan_ap"):
        a, b, c = f0.copy(), sp.copy(), ap.copy()
        if what == "nan_f0": a[5:9] = np.nan
        if what == "inf_f0": a[3] = np.inf
        if what == "huge_f0": a[7:12] = 1e300
        if what == "nan_sp": b[4:8] = np.nan
        if what == "inf_sp": b[10, :] = np.inf
        if what == "nan_ap": c[2:6] = np.nan
        hostile.append(dict(base, f0=a, sp=b, ap=c))
    for plan in hostile:
        hip.realtime_plan(plan)                           # returns from every entry point
    after = hip.realtime_plan(base)["out"]
    out = tmp_path / "fresh.npy"
    subprocess.run([sys.executable, "-c", FRESH.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=str(out))],
                   check=True, timeout=600)
    fresh = np.load(out)
    assert after.size > 0 and np.array_equal(after, fresh)
    assert np.array_equal(after.shape, FIX["hop10_22k.out"].shape)
