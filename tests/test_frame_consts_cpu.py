"""tests/test_gpu_frame_consts.py's equality on the host emulation: cheaptrick.hip and d4c.hip with their frames' uniform
constants read from the records the offset scans leave (the shipped route), and with WORLD_HIP_INKERNEL_CONSTS, every
thread evaluating them.  The same bits, for F0 tracks that take every branch of the two stages."""
import os

import numpy as np
import pytest

from backends import emu, same_bits  # noqa: F401 (emu: a fixture)

SWITCH = "WORLD_HIP_INKERNEL_CONSTS"


def _both_routes(run):
    old = os.environ.pop(SWITCH, None)
    try:
        records = run()
        os.environ[SWITCH] = "1"
        inkernel = run()
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old
    return records, inkernel


def _inputs(fs, seconds):
    from world_amd import synth
    from world_amd.api import frame_count
    x = synth.utterance(2, fs, seconds).numpy()
    nf = frame_count(fs, len(x), 5.0)
    vals = [0.0, 35.0, 45.0, 60.0, 90.0, 140.0, 800.0, 0.5 * fs + 1000.0, float("nan")]
    f0 = np.array([vals[k % len(vals)] for k in range(nf)])
    f0[0], f0[-1] = 140.0, 90.0                     # a voiced frame at both ends of the utterance
    return x, np.arange(nf) * 0.005, f0


@pytest.mark.parametrize("fs,fft", [(16000, 1024), (48000, 2048)])
def test_emulated_cheaptrick_routes_are_bit_identical(emu, fs, fft):
    x, tp, f0 = _inputs(fs, 0.1)
    rec, ker = _both_routes(lambda: emu.cheaptrick(x, fs, tp, f0, fft_size=fft, f0_floor=3.0 * fs / (fft - 3.0)))
    assert same_bits(rec, ker)                      # (NaN == NaN: a frame whose F0 lies above fs / 2 may hold some)
    assert np.isfinite(rec[f0 <= 0.5 * fs]).all()


@pytest.mark.parametrize("fs,fft", [(16000, 1024), (48000, 2048)])
def test_emulated_d4c_routes_are_bit_identical(emu, fs, fft):
    x, tp, f0 = _inputs(fs, 0.1)
    rec, ker = _both_routes(lambda: emu.d4c(x, fs, tp, f0, fft))
    assert same_bits(rec, ker)
    body = (rec < 1.0 - 1e-12).any(axis=1)
    assert body.any() and (~body).any()             # frames that went through d4c_frame, and frames that did not
