"""The frame kernels' workgroup-uniform constants, computed once per frame, against the same kernels computing them in
every thread.

ct_frame, d4c_lovetrain and d4c_frame read what depends on a frame's F0, its position, fs and the transform length alone
from a record the offset scan leaves per frame (stage_params.h: CtFrameRec, D4cFrameRec; prepare.h holds every expression
once), what depends on the launch alone from their parameter blocks (host arithmetic), and hv_band_events_fft its two phase
steps from the per-(utterance, band) constants.  WORLD_HIP_INKERNEL_CONSTS routes a call through the instantiations that
evaluate all of that themselves, as every thread did before the records existed.  The two routes run the same IEEE
operations on the same operands, so every output must be the SAME BITS -- for every static transform size of each kernel
(16 / 22.05 kHz: 1024 and 2048 points, 44.1 / 48 kHz: 2048 and 4096, 96 kHz: 8192 and the run-time-length LoveTrain,
176.4 kHz: the 16384-point shapes), for F0 tracks handed to the stages directly so that every branch is taken (unvoiced,
below D4C's 40 and 47 Hz floors, windows longer than half the transform, above fs / 2, NaN), at both ends of an utterance
and in a ragged batch.  One case is also held to the oracle, one runs on the poisoned-workspace build."""
import os

import numpy as np
import pytest

from backends import wh  # noqa: F401 (a fixture)
from util import RTOL, assert_f0_close, max_rel

pytestmark = pytest.mark.gpu

SWITCH = "WORLD_HIP_INKERNEL_CONSTS"
RATES = [16000, 22050, 44100, 48000, 96000, 176400]
SECONDS = (0.3, 0.21, 0.13)                        # a ragged batch of three lengths
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _f0_values(fs):
    # unvoiced; below D4C's LoveTrain floor (40 Hz) and its body floor (47 Hz) -- both below CheapTrick's own floor at most
    # rates; 60 and 90 Hz (D4C windows of 4 periods longer than half the 4096-point transform at 48 kHz); a usual voice; the
    # estimators' ceiling; above fs / 2; NaN
    return [0.0, 35.0, 45.0, 60.0, 90.0, 140.0, 800.0, 0.5 * fs + 1000.0, float("nan")]


def _batch(fs):
    """-> x [3, L], x_len, tpos [3, F], f0 [3, F], n_frames: every F0 value of _f0_values in turn, a voiced frame at
    both ends of every utterance"""
    import torch
    from world_amd import synth
    from world_amd.api import frame_count
    xs = [synth.utterance(i, fs, s) for i, s in enumerate(SECONDS)]
    lens = np.array([x.numel() for x in xs], dtype=np.int32)
    xb = torch.zeros((len(xs), int(lens.max())), dtype=torch.float64)
    for i, x in enumerate(xs):
        xb[i, :x.numel()] = x
    nf = np.array([frame_count(fs, int(n), 5.0) for n in lens], dtype=np.int32)
    F = int(nf.max())
    vals = _f0_values(fs)
    tpos = np.zeros((len(xs), F))
    f0 = np.zeros((len(xs), F))
    for u, n in enumerate(nf):
        tpos[u, :n] = np.arange(n) * 0.005
        f0[u, :n] = [vals[(k + 2 * u) % len(vals)] for k in range(n)]
        f0[u, 0], f0[u, n - 1] = 140.0, 90.0
    return xb, lens, torch.from_numpy(tpos), torch.from_numpy(f0), nf


def _valid(t, nf):
    return [t[u, :int(n)] for u, n in enumerate(nf)]


def _assert_same(what, a, b, nf):
    import torch
    # bit patterns: torch.equal on the values would call a NaN unequal to itself, and the rows of a frame whose F0 lies above
    # fs / 2 may hold some (the reference indexes beyond its arrays there: prepare.h)
    for u, (x, y) in enumerate(zip(_valid(a, nf), _valid(b, nf))):
        x, y = x.contiguous(), y.contiguous()
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), f"{what}, utterance {u}: the two routes differ"


def _spectral(wh, fs, xb, lens, tpos, f0, nf):
    import torch
    from world_amd.api import cheaptrick_fft_size
    # (96 kHz and above: CheapTrick's 8192-point shape; below, the rate's natural size: 1024 / 2048 points)
    fft = 8192 if fs >= 96000 else cheaptrick_fft_size(fs)
    x, tp, f = xb.cuda(), tpos.cuda(), f0.cuda()
    sp = wh.cheaptrick(x, fs, tp, f, nf, x_len=lens, fft_size=fft, f0_floor=3.0 * fs / (fft - 3.0))
    ap = wh.d4c(x, fs, tp, f, nf, fft, x_len=lens)
    torch.cuda.synchronize()
    return sp.cpu(), ap.cpu()


@pytest.mark.parametrize("fs", RATES)
def test_spectral_stages_given_f0_are_bit_identical(wh, fs):
    xb, lens, tpos, f0, nf = _batch(fs)
    (sp_r, ap_r), (sp_k, ap_k) = _both_routes(lambda: _spectral(wh, fs, xb, lens, tpos, f0, nf))
    _assert_same(f"CheapTrick at {fs} Hz", sp_r, sp_k, nf)
    _assert_same(f"D4C at {fs} Hz", ap_r, ap_k, nf)
    # the comparison saw frames that went through d4c_frame, and frames that did not
    body = [(a < 1.0 - 1e-12).any(dim=1) for a in _valid(ap_r, nf)]
    assert any(b.any() for b in body) and any((~b).any() for b in body)


@pytest.mark.parametrize("fs", RATES)
def test_analyze_through_harvest_is_bit_identical(wh, fs):
    import torch
    xb, lens, *_ = _batch(fs)

    def run():
        tpos, f0, sp, ap, nf = wh.analyze(xb.cuda(), fs, x_len=lens, f0_method="harvest")
        torch.cuda.synchronize()
        return tpos.cpu(), f0.cpu(), sp.cpu(), ap.cpu(), np.array(nf)

    rec, ker = _both_routes(run)
    assert np.array_equal(rec[4], ker[4])
    for name, a, b in zip(("tpos", "f0", "sp", "ap"), rec, ker):
        _assert_same(f"analyze at {fs} Hz, {name}", a, b, rec[4])
    assert any((f > 0).any() for f in _valid(rec[1], rec[4]))       # Harvest found voiced frames: the filter bank mattered


def test_frame_ranges_with_reused_offsets_are_bit_identical(wh):
    """the records live with the offsets: a later call that reuses them (another frame range, skip_prepare) reads what the
    first call's scan wrote -- packed records of two ranges, the second with reuse_offsets"""
    import torch
    from world_amd.api import cheaptrick_fft_size
    fs = 48000
    xb, lens, tpos, f0, nf = _batch(fs)
    x, tp, f = xb.cuda(), tpos.cuda().contiguous(), f0.cuda().contiguous()
    nb = cheaptrick_fft_size(fs) // 2 + 1
    cut = 17

    def run():
        block = torch.full((int(nf.sum()), 2 + 2 * nb), -7.0, dtype=torch.float64, device="cuda")
        rows = wh.spectral_packed_range(x, fs, tp, f, nf, block, 0, cut, x_len=lens)
        rows += wh.spectral_packed_range(x, fs, tp, f, nf, block, cut, int(nf.max()), first_row=rows, x_len=lens, reuse_offsets=True)
        torch.cuda.synchronize()
        assert rows == int(nf.sum())
        return block.cpu()

    rec, ker = _both_routes(run)
    assert torch.equal(rec.view(torch.int64), ker.view(torch.int64))        # (bit patterns: the records' heads hold the NaN F0s)


def test_records_route_matches_the_oracle():
    """the shipped route against the CPU oracle, at the tolerance of tests/test_gpu_parity.py"""
    from oracle.loader import best_oracle
    from world_amd import synth
    from world_amd.api import HostAPI
    assert SWITCH not in os.environ
    hip, oracle = HostAPI(), best_oracle()
    fs = 48000
    x = synth.vowel(fs, 0.3, seed=fs + 7).numpy()
    tp_o, f0_o = oracle.harvest(x, fs)
    tp, f0 = hip.harvest(x, fs)
    assert np.array_equal(tp, tp_o)
    assert_f0_close(f0, f0_o)
    fft = hip.cheaptrick_fft_size(fs)
    assert max_rel(hip.cheaptrick(x, fs, tp_o, f0_o, fft_size=fft), oracle.cheaptrick(x, fs, tp_o, f0_o, fft_size=fft)) <= RTOL
    assert max_rel(hip.d4c(x, fs, tp_o, f0_o, fft), oracle.d4c(x, fs, tp_o, f0_o, fft)) <= RTOL


def test_poisoned_workspace_build_is_bit_identical(wh):
    """-DWH_HBM_POISON (tests/test_gpu_checked_builds.py): every carve of the workspace is refilled with 0xFF bytes before
    the call writes it -- a record field a reader takes before its producer wrote it, or of a frame the producer skipped,
    is a NaN or a -1 there.  Two passes in one context, the second over the first's leftovers."""
    import torch
    from world_amd.api import WorldHip
    lib = os.path.join(ROOT, "world_amd", "variants", "libworld_hip_hbm.so")
    assert os.path.exists(lib), f"{lib} is missing: __graft_entry__.build() builds it"
    assert SWITCH not in os.environ
    fs = 48000
    xb, lens, tpos, f0, nf = _batch(fs)
    want = _spectral(wh, fs, xb, lens, tpos, f0, nf)
    tpos_w, f0_w, sp_w, ap_w, nf_w = wh.analyze(xb.cuda(), fs, x_len=lens, f0_method="harvest")
    torch.cuda.synchronize()
    hbm = WorldHip(device=0, lib_path=lib)
    try:
        for rep in range(2):
            got = _spectral(hbm, fs, xb, lens, tpos, f0, nf)
            _assert_same(f"hbm build, pass {rep}, CheapTrick", want[0], got[0], nf)
            _assert_same(f"hbm build, pass {rep}, D4C", want[1], got[1], nf)
            tpos_h, f0_h, sp_h, ap_h, nf_h = hbm.analyze(xb.cuda(), fs, x_len=lens, f0_method="harvest")
            torch.cuda.synchronize()
            assert np.array_equal(np.array(nf_w), np.array(nf_h))
            for name, a, b in (("f0", f0_w, f0_h), ("sp", sp_w, sp_h), ("ap", ap_w, ap_h)):
                _assert_same(f"hbm build, pass {rep}, analyze {name}", a.cpu(), b.cpu(), nf_w)
    finally:
        hbm.close()
