"""Helper of tests/test_realtime_cpu.py and tests/test_realtime_gpu.py (a subprocess, so that a fork() is safe to try):
   realtime_lifecycle.py <library> <out.npz> [fork]
A drop-in WorldSynthesizer runs a chunk plan; world_hip_shutdown() is called in the middle of its stream, and the stream
goes on: its output must equal an uninterrupted run.  With `fork` (the emulated library only, as in dropin_lifecycle.py:
a forked child cannot use the parent's HIP runtime at all), a child forked after the parent's calls runs a fresh
synthesiser on the same plan and reports through its exit status whether it got the same output."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import synth_params                                        # noqa: E402
from world_amd.api import HostAPI                                    # noqa: E402

lib_path, out = sys.argv[1], sys.argv[2]
do_fork = len(sys.argv) > 3 and sys.argv[3] == "fork"
H = HostAPI(lib_path)
fs, fft, bs, P = 16000, 1024, 64, 8
f0, sp, ap = synth_params(fs, 60, fft, seed=9)
chunks = [4] * 15


def run(shutdown_after=-1):
    s = H.initialize_synthesizer(fs, 5.0, fft, bs, P)
    got, rc, pos = [], None, 0
    for k, n in enumerate(chunks):
        assert H.add_parameters(s, f0[pos:pos + n], sp[pos:pos + n], ap[pos:pos + n]) == 1
        pos += n
        while True:
            r, buf = H.synthesis2(s)
            if not r:
                break
            got.append(buf)
        if k == shutdown_after:
            rc = H.lib.world_hip_shutdown()
    H.destroy_synthesizer(s)
    return np.concatenate(got), rc


first, _ = run()
second, rc = run(shutdown_after=6)
assert np.array_equal(first, second)
child = -1
if do_fork:
    pid = os.fork()
    if pid == 0:
        try:
            third, _ = run()
            os._exit(0 if np.array_equal(first, third) else 3)
        except BaseException:                                        # noqa: BLE001
            os._exit(4)
    _, status = os.waitpid(pid, 0)
    child = os.WEXITSTATUS(status) if os.WIFEXITED(status) else 100 + os.WTERMSIG(status)
    third, _ = run()                                                 # the parent goes on as before
    assert np.array_equal(first, third)
np.savez(out, first=first, second=second, shutdown_rc=rc, child=child)
