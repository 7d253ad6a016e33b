"""Is the reference DEFINED on every case of tests/test_gpu_offdefault_fft.py?

    python oracle/asan_reference.py

builds the unmodified reference's sources with -fsanitize=address (host code only) into a temporary directory and runs
every (fs, fft_size, F0 kind) of the module's CheapTrick, D4C and Synthesis tables through it in a child process: a case
with a report may not stay in the tables.  It also checks, with the reference and the long double oracle alone, that the
wide oracle decides few enough D4C rows differently (tests/util.discrete_agreement's own limit).  Nothing built here is kept.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF = os.environ.get("WORLD_REF", "/root/reference")


def child(so):
    import numpy as np
    import test_gpu_offdefault_fft as T
    from oracle.loader import WideOracle
    from util import discrete_agreement
    from world_amd.api import HostAPI
    ref, wide = HostAPI(so, hip_runtime=False), WideOracle()
    for fs, fft, kinds, _ in T.CT_CASES:
        x = T._signal(fs, T._seconds(fs))
        for kind in kinds:
            tp, f0 = T._f0(kind, ref, x, fs, fft)
            assert np.isfinite(ref.cheaptrick(x, fs, tp, f0, fft_size=fft)).all()
            print("asan: cheaptrick", fs, fft, kind, "ok", flush=True)
    for fs, fft, kind in T.D4C_CASES:
        x = T._signal(fs, T._seconds(fs))
        tp, f0 = T._f0(kind, ref, x, fs, fft)
        for th in (0.85, 0.0):
            r, w = ref.d4c(x, fs, tp, f0, fft, threshold=th), wide.d4c(x, fs, tp, f0, fft, threshold=th)
            rows = T.d4c_exit_rows(r)
            w_only = discrete_agreement("R, W", rows, rows, T.d4c_exit_rows(w))
            print("asan: d4c", fs, fft, kind, th, "ok; W-only rows", len(w_only), "of", len(tp), flush=True)
    for fs, fft, _ in T.SY_CASES:
        x, f0, sp, ap = T._synth_inputs(ref, fs, fft, 0.2)
        assert np.isfinite(ref.synthesis(f0, sp, ap, fft, 5.0, fs, len(x))).all()
        print("asan: synthesis", fs, fft, "ok", flush=True)


def main():
    if "--child" in sys.argv:
        return child(sys.argv[-1])
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libref_asan.so")
        src = os.path.join(REF, "src")
        srcs = sorted(os.path.join(src, f) for f in os.listdir(src) if f.endswith(".cpp"))
        subprocess.run(["g++", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=address", "-I", src, "-o", so, *srcs, "-lm"], check=True)
        libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
        preload = " ".join(v for v in (libasan, os.environ.get("LD_PRELOAD", "")) if v)   # in front of what is preloaded already
        env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", so], env=env, check=True)
        print("no report")


if __name__ == "__main__":
    main()
