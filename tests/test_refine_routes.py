"""Harvest's two candidate-refinement kernels compute the same bits.  Where a millisecond is a whole number of
analysis samples (16 / 48 kHz input: 8 kHz after decimation) the candidate-major hv_refine runs; WORLD_HIP_REFINE_FRAMES
routes the same windows through the frame-major hv_refine_frames instead.  Both must give bit-identical F0 -- at a
1 ms hop, so that every refined frame reaches the output -- including utterances shorter than the seven frames a
candidate spreads over and frame counts that are a multiple of nothing in particular."""
import os

import numpy as np
import pytest

from backends import emu  # noqa: F401 (a fixture)

SWITCH = "WORLD_HIP_REFINE_FRAMES"


def _signals(fs):
    from world_amd import synth
    out = []
    for i, sec in enumerate((0.004, 0.0061, 0.0397, 0.2113, 0.6029)):
        x = synth.utterance(i, fs, 1.0).numpy()[: max(1, int(round(sec * fs)))].copy()
        out.append(x)
    return out


def _both_routes(run):
    old = os.environ.pop(SWITCH, None)
    try:
        new = run()
        os.environ[SWITCH] = "1"
        frames = run()
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old
    return new, frames


@pytest.mark.parametrize("fs", [48000, 16000])
def test_emulated_routes_are_bit_identical(emu, fs):
    for x in _signals(fs)[:4]:
        new, frames = _both_routes(lambda: emu.harvest(x, fs, frame_period=1.0))
        assert np.array_equal(new[0], frames[0]) and np.array_equal(new[1], frames[1]), len(x)


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [48000, 16000])
def test_gpu_routes_are_bit_identical(fs):
    import torch
    assert torch.cuda.is_available(), "this test needs the MI355X"
    from world_amd.api import WorldHip
    wh = WorldHip()
    xs = _signals(fs)
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    batch = np.zeros((len(xs), int(lens.max())))
    for i, x in enumerate(xs):
        batch[i, : len(x)] = x
    xb = torch.from_numpy(batch).cuda()

    def run():
        tp, f0, nf = wh.harvest(xb, fs, x_len=lens, frame_period=1.0)
        torch.cuda.synchronize()
        return tp.cpu().numpy(), f0.cpu().numpy(), nf

    new, frames = _both_routes(run)
    assert np.array_equal(new[2], frames[2])
    assert np.array_equal(new[0], frames[0])
    assert np.array_equal(new[1], frames[1])
    assert (new[1] > 0).any()                     # the comparison saw voiced frames
