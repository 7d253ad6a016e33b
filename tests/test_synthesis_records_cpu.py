"""Synthesis straight from records (include/world_hip.h: world_hip_synthesis_records, world_hip_realtime_add_coded) through
the host-compiled kernels (tests/emu/libworld_emu.so).  The cases are functions of a backend, so that
tests/test_synthesis_records_gpu.py runs the same ones through the shipped library.

Bars.  Against the three-step route (unpack_results, or the two decode calls, then synthesis_batch), an utterance alone
and the real-time streams: equality -- each pair runs the same device functions on the same values under
-ffp-contract=off.  Wire 1's three-step route widens the f32 records to f64 records on the host first (exact), since
world_hip_unpack_results reads f64 records only.  Against the reference's DecodeSpectralEnvelope + DecodeAperiodicity +
Synthesis: 1e-8 of the waveform's peak, what tests/test_synthesis.py holds Synthesis itself to.

Shapes.  Three utterances per batch -- 61 frames voiced with a gap, 21 frames unvoiced of which some are aperiodic (mean band
value above -0.5 dB: CheckVUV's branch), and the minimum of 2 frames -- from first_row = 3 of a block whose other rows are
NaN; 16 kHz (one band, 512-point decode transform), 48 kHz (five bands), 192 kHz (sy_pulse<8192>, 4096-point decode
transform) and 48 kHz at fft 1024 as the off-default pair; 24 and 60 coefficients.

Fixtures.  The rows of these batches are synthetic envelopes coded by the port oracle: tests/golden/synthesis.npz holds
waveforms only, no parameter rows, and tests/golden/codec.npz holds 12 coded rows per recording at 16 and 48 kHz -- too few
for the 61-frame utterance, none at 192 kHz and none aperiodic.  Where they fit they are used: case_golden_rows synthesises
the 12 recorded mel-cepstrum and band-aperiodicity rows of the 16 and 48 kHz recordings as one utterance."""
import ctypes as C
import os

import numpy as np
import pytest

import backends
from backends import ROOT, cpu_backend, lib, smooth_envelope as envelope  # noqa: F401 (lib: a fixture)

_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
FP = 5.0
FIRST_ROW = 3
N_FRAMES = np.array([61, 21, 2], dtype=np.int32)
SHAPES = [(16000, 1024, 24), (48000, 2048, 60), (192000, 8192, 24), (48000, 1024, 60)]      # (fs, fft_size, coefficients)


def ip(a):
    return a.ctypes.data_as(_ip)


# ---- fixtures: computed once per shape, shared, never modified -------------------------------------------------------------
def y_lengths(fs, nf):
    return np.array([int((int(n) - 1) * FP / 1000.0 * fs) + 1 for n in nf], dtype=np.int32)


_CASES = {}


def case_of(oracle, fs, fft, ndim):
    """-> dict: f0 (per utterance), dense sp / ap rows, their coded rows (the port's CodeSpectralEnvelope / CodeAperiodicity),
    and the three blocks (wire 0, 1, 2) with the records from FIRST_ROW and NaN everywhere else"""
    key = (fs, fft, ndim)
    if key in _CASES:
        return _CASES[key]
    nb, total = fft // 2 + 1, int(N_FRAMES.sum())
    f0 = [np.linspace(150.0, 220.0, 61), np.zeros(21), np.array([120.0, 0.0])]
    f0[0][25:31] = 0.0                                                   # one gap
    sp = envelope(fs, fft, total, seed=fs + ndim)
    frq = np.arange(nb) / (nb - 1.0)
    ap = np.clip(0.01 + 0.6 * frq[None, :] ** 2 * np.linspace(0.5, 1.0, total)[:, None], 0.001, 0.9)
    ap[61:82] = 0.7
    ap[61 + 4:61 + 9] = 0.98                                             # 20 log10 = -0.18 dB: aperiodic frames
    mcep = oracle.code_spectral_envelope(sp, fs, fft, ndim)
    bap = oracle.code_aperiodicity(ap, fs, fft)
    assert np.any(bap[61:82].mean(axis=1) > -0.5) and np.any(bap[61:82].mean(axis=1) <= -0.5) and np.all(bap[:61].mean(axis=1) < -0.5)
    head = np.stack([np.arange(total) * FP / 1000.0, np.concatenate(f0)], axis=1)
    rows = FIRST_ROW + total + 2

    def block(body):
        b = np.full((rows, body.shape[1]), np.nan)
        b[FIRST_ROW:FIRST_ROW + total] = body
        return b
    narrow = np.concatenate([sp, ap], axis=1).astype(np.float32)        # [total, 2 nb] floats = nb doubles
    c = dict(fs=fs, fft=fft, ndim=ndim, nb=nb, f0=f0, sp=sp, ap=ap, mcep=mcep, bap=bap,
             blocks={0: block(np.concatenate([head, sp, ap], axis=1)),
                     1: block(np.concatenate([head, np.ascontiguousarray(narrow).view(np.float64)], axis=1)),
                     2: block(np.concatenate([head, mcep, bap], axis=1))})
    _CASES[key] = c
    return c


def widened(block1, nb):
    """f32 records -> the f64 records holding the same values (exact)"""
    rows = np.ascontiguousarray(block1[:, 2:]).view(np.float32).astype(np.float64)
    return np.concatenate([block1[:, :2], rows], axis=1)


def dense(parts, nf, cols):
    """per-utterance row blocks back to back -> [B, F, cols] with NaN beyond each utterance's frames"""
    out = np.full((len(nf), int(max(nf)), cols), np.nan)
    at = 0
    for u, n in enumerate(nf):
        out[u, :n] = parts[at:at + n]
        at += n
    return out


# ---- a backend: the C calls on arrays that live where the library wants them -----------------------------------------------
class Backend(backends.Backend):
    """the records calls on the arrays of backends.Backend, every one of them float64"""

    def dev(self, a):
        return super().dev(np.asarray(a, dtype=np.float64))

    def records(self, fs, fft, nf, block, wire, ndim, first_row=FIRST_ROW, cols=None, yl=None, d_block=True):
        """world_hip_synthesis_records -> (rc, y [B, Y]); y starts as zeros"""
        nf = np.ascontiguousarray(nf, dtype=np.int32)
        yl = y_lengths(fs, nf) if yl is None else yl
        Y = int(yl.max())
        d = self.dev(block)
        y = self.dev(np.zeros((len(nf), Y)))
        rc = self.lib.world_hip_synthesis_records(self.ctx, len(nf), fs, FP, fft, ip(nf), first_row, self.ptr(d) if d_block else None,
                                                  block.shape[1] if cols is None else cols, wire, ndim, ip(yl), Y, self.ptr(y))
        return rc, self.host(y)

    def synthesis(self, fs, fft, nf, f0, sp, ap):
        """world_hip_synthesis_batch on dense [B, F(, nb)] arrays"""
        nf = np.ascontiguousarray(nf, dtype=np.int32)
        yl = y_lengths(fs, nf)
        Y = int(yl.max())
        d = [self.dev(a) for a in (f0, sp, ap)]
        y = self.dev(np.zeros((len(nf), Y)))
        rc = self.lib.world_hip_synthesis_batch(self.ctx, len(nf), fs, FP, fft, ip(nf), f0.shape[1], self.ptr(d[0]), self.ptr(d[1]),
                                                self.ptr(d[2]), ip(yl), Y, self.ptr(y))
        assert rc == 0, self.error()
        return self.host(y)

    def decode(self, fs, fft, mcep, bap):
        """world_hip_decode_spectral_envelope / _aperiodicity on contiguous coded rows -> (sp, ap) [rows, nb]"""
        rows, nb = mcep.shape[0], fft // 2 + 1
        d_m, d_b = self.dev(mcep), self.dev(bap)
        sp, ap = self.dev(np.zeros((rows, nb))), self.dev(np.zeros((rows, nb)))
        assert self.lib.world_hip_decode_spectral_envelope(self.ctx, rows, fs, fft, mcep.shape[1], self.ptr(d_m), self.ptr(sp)) == 0, self.error()
        assert self.lib.world_hip_decode_aperiodicity(self.ctx, rows, fs, fft, self.ptr(d_b), self.ptr(ap)) == 0, self.error()
        return self.host(sp), self.host(ap)

    def unpack(self, block, nf, nb, first_row=FIRST_ROW):
        """world_hip_unpack_results -> (f0 [B, F], sp, ap [B, F, nb]); NaN beyond each utterance's frames"""
        nf = np.ascontiguousarray(nf, dtype=np.int32)
        B, F = len(nf), int(nf.max())
        d = self.dev(block)
        outs = [self.dev(np.full(s, np.nan)) for s in ((B, F), (B, F), (B, F, nb), (B, F, nb))]
        rc = self.lib.world_hip_unpack_results(self.ctx, B, ip(nf), F, nb, self.ptr(d), first_row, *[self.ptr(o) for o in outs])
        assert rc == 0, self.error()
        return [self.host(o) for o in outs[1:]]

    def pulses_dropped(self):
        need = C.c_int(-1)
        assert self.lib.world_hip_synthesis_pulses_dropped(self.ctx, C.byref(need)) == 0, self.error()
        return need.value

    def set_capacity(self, n):
        assert self.lib.world_hip_set_synthesis_pulse_capacity(self.ctx, n) == 0, self.error()


be = cpu_backend(Backend)


# ---- the three-step routes ------------------------------------------------------------------------------------------------
def three_step_coded(be, c, nf=N_FRAMES, lo=0):
    n = int(np.sum(nf))
    sp, ap = be.decode(c["fs"], c["fft"], c["mcep"][lo:lo + n], c["bap"][lo:lo + n])
    f0 = dense(np.concatenate(c["f0"])[lo:lo + n, None], nf, 1)[:, :, 0]
    return be.synthesis(c["fs"], c["fft"], nf, f0, dense(sp, nf, c["nb"]), dense(ap, nf, c["nb"]))


def valid(y, fs, nf=N_FRAMES):
    return [y[u, :n] for u, n in enumerate(y_lengths(fs, nf))]


def same(a, b, fs, nf=N_FRAMES):
    return all(np.array_equal(p, q) for p, q in zip(valid(a, fs, nf), valid(b, fs, nf)))


# ---- the cases ------------------------------------------------------------------------------------------------------------
def case_coded_records(be, oracle, ref, fs, fft, ndim):
    """conditions 1 (wire 2) and 2, and the reference's decoders + Synthesis as the yardstick (`ref`)"""
    c = case_of(oracle, fs, fft, ndim)
    rc, y = be.records(fs, fft, N_FRAMES, c["blocks"][2], 2, ndim)
    assert rc == 0, be.error()
    assert be.pulses_dropped() == 0
    assert not np.isnan(y).any()                                          # the poisoned rows around the records were not read
    assert same(y, three_step_coded(be, c), fs)
    at = 0
    for u, n in enumerate(N_FRAMES):                                      # alone, from a block of its own, first_row = 0
        own = c["blocks"][2][FIRST_ROW + at:FIRST_ROW + at + n]
        rc, one = be.records(fs, fft, [n], own, 2, ndim, first_row=0)
        assert rc == 0, be.error()
        assert np.array_equal(one[0, :y_lengths(fs, [n])[0]], valid(y, fs)[u]), u
        at += n
    at = 0
    for u, n in enumerate(N_FRAMES):
        sp, ap = ref.decode_spectral_envelope(c["mcep"][at:at + n], fs, fft), ref.decode_aperiodicity(c["bap"][at:at + n], fs, fft)
        want = ref.synthesis(c["f0"][u], sp, ap, fft, FP, fs, int(y_lengths(fs, [n])[0]))
        got, peak = valid(y, fs)[u], float(np.max(np.abs(want)))
        err = float(np.max(np.abs(got - want)))
        print(f"fs {fs} fft {fft} D {ndim} utterance {u}: peak {peak:.3e}, error {err / peak if peak else err:.3e} of the peak")
        assert u == 2 or peak > 1e-4
        assert err <= 1e-8 * peak
        at += n


def case_golden_rows(be, name, fs, fft, ndim):
    """condition 1 (wire 2) on the coded rows recorded from the reference's coders (tests/golden/codec.npz)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "codec.npz"))
    mcep, bap = z[f"{name}.mcep{ndim}"], z[f"{name}.bap"]
    n = mcep.shape[0]
    f0 = np.linspace(110.0, 180.0, n)
    f0[5:7] = 0.0
    block = np.full((FIRST_ROW + n + 2, 2 + ndim + bap.shape[1]), np.nan)
    block[FIRST_ROW:FIRST_ROW + n] = np.concatenate([np.arange(n)[:, None] * FP / 1000.0, f0[:, None], mcep, bap], axis=1)
    rc, y = be.records(fs, fft, [n], block, 2, ndim)
    assert rc == 0, be.error()
    assert be.pulses_dropped() == 0
    assert not np.isnan(y).any() and np.max(np.abs(y)) > 0
    c = dict(fs=fs, fft=fft, nb=fft // 2 + 1, mcep=mcep, bap=bap, f0=[f0])
    assert same(y, three_step_coded(be, c, nf=[n]), fs, nf=[n])


def case_plain_records(be, oracle, fs, fft, wire):
    """conditions 1 (wires 0 and 1) and 2"""
    c = case_of(oracle, fs, fft, 24 if fs != 48000 or fft != 2048 else 60)
    block = c["blocks"][wire]
    rc, y = be.records(fs, fft, N_FRAMES, block, wire, 0)
    assert rc == 0, be.error()
    assert be.pulses_dropped() == 0
    assert not np.isnan(y).any()
    f0, sp, ap = be.unpack(block if wire == 0 else widened(block, c["nb"]), N_FRAMES, c["nb"])
    assert same(y, be.synthesis(fs, fft, N_FRAMES, f0, sp, ap), fs)
    at = 0
    for u, n in enumerate(N_FRAMES):
        rc, one = be.records(fs, fft, [n], block[FIRST_ROW + at:FIRST_ROW + at + n], wire, 0, first_row=0)
        assert rc == 0, be.error()
        assert np.array_equal(one[0, :y_lengths(fs, [n])[0]], valid(y, fs)[u]), u
        at += n


def case_refusals(be, oracle):
    """condition 5: each refusal carries a message; the next valid call equals one on a fresh context"""
    fs, fft, ndim = 48000, 2048, 60
    c = case_of(oracle, fs, fft, ndim)
    b2, b0 = c["blocks"][2], c["blocks"][0]
    one = np.array([61, 1, 2], dtype=np.int32)
    refused = [
        dict(fs=fs, fft=fft, nf=N_FRAMES, block=b2, wire=2, ndim=ndim, cols=b2.shape[1] + 1),         # cols / wire
        dict(fs=fs, fft=fft, nf=N_FRAMES, block=b0, wire=0, ndim=0, cols=b2.shape[1]),
        dict(fs=fs, fft=fft, nf=N_FRAMES, block=b0, wire=1, ndim=0),
        dict(fs=fs, fft=fft, nf=one, block=b2, wire=2, ndim=ndim, yl=y_lengths(fs, N_FRAMES)),         # n_frames[u] = 1
        dict(fs=192000, fft=1024, nf=N_FRAMES, block=np.zeros((90, 2 + 2 * 513)), wire=0, ndim=0),     # (fs, fft_size)
        dict(fs=fs, fft=fft, nf=N_FRAMES, block=b2, wire=2, ndim=0),                                   # ndim 0
        dict(fs=fs, fft=fft, nf=N_FRAMES, block=b2, wire=2, ndim=ndim, d_block=False),                 # null block
    ]
    with be.fresh() as clean:
        rc, want = clean.records(fs, fft, N_FRAMES, b2, 2, ndim)
        assert rc == 0, clean.error()
    with be.fresh() as used:
        for kw in refused:
            rc, y = used.records(**kw)
            assert rc != 0, kw
            assert used.error(), kw
            assert not y.any()                                            # nothing was written
            rc, got = used.records(fs, fft, N_FRAMES, b2, 2, ndim)
            assert rc == 0, used.error()
            assert np.array_equal(got, want), kw


def case_pulse_capacity(be, oracle):
    """condition 6: the capacity semantics are synthesis_batch's"""
    fs, fft, ndim = 16000, 1024, 24
    c = case_of(oracle, fs, fft, ndim)
    nf = N_FRAMES[1:2]                                                    # the all-unvoiced utterance
    own = c["blocks"][2][FIRST_ROW + 61:FIRST_ROW + 82]
    try:
        be.set_capacity(8)
        rc, _ = be.records(fs, fft, nf, own, 2, ndim, first_row=0)
        assert rc == 0, be.error()
        need = be.pulses_dropped()
        assert need > 8
        three_step_coded(be, c, nf, lo=61)
        assert be.pulses_dropped() == need                                # synthesis_batch reports the same count
        be.set_capacity(need)
        rc, y = be.records(fs, fft, nf, own, 2, ndim, first_row=0)
        assert rc == 0, be.error()
        assert be.pulses_dropped() == 0
        assert same(y, three_step_coded(be, c, nf, lo=61), fs, nf)
        assert be.pulses_dropped() == 0
    finally:
        be.set_capacity(0)


def case_realtime(be, oracle):
    """condition 4: a 40-frame stream per stream, in chunks, buffer_size 64, 2 streams, 3 ring slots (so adds find the
    ring full): add_coded against decode + add over every call"""
    fs, fft, ndim = 16000, 1024, 24
    c = case_of(oracle, fs, fft, ndim)
    nb, cols, L = c["nb"], c["blocks"][2].shape[1], be.lib
    rec = [c["blocks"][2][FIRST_ROW:FIRST_ROW + 40], c["blocks"][2][FIRST_ROW + 41:FIRST_ROW + 81]]   # (stream 1: voiced into unvoiced)
    chunks = [[5, 15, 3, 17], [1, 20, 19]]
    d_rec = [be.dev(r) for r in rec]
    dec = []
    for r in rec:
        sp, ap = be.decode(fs, fft, r[:, 2:2 + ndim], r[:, 2 + ndim:])
        dec.append((be.dev(sp), be.dev(ap)))
    hs = [C.c_void_p(), C.c_void_p()]
    for h in hs:
        assert L.world_hip_realtime_create(be.ctx, 2, fs, FP, fft, 64, 3, C.byref(h)) == 0, be.error()
    try:
        pos, k = [0, 0], [0, 0]
        bufs = [be.dev(np.zeros((2, 64))) for _ in hs]
        produced = [np.zeros(2, dtype=np.int32) for _ in hs]
        full = samples = 0
        for _ in range(400):
            for s in range(2):
                if k[s] == len(chunks[s]):
                    continue
                n, at = chunks[s][k[s]], pos[s]
                f0 = np.ascontiguousarray(rec[s][at:at + n, 1])
                ra = L.world_hip_realtime_add_coded(hs[0], s, f0.ctypes.data_as(_dp), n, be.ptr(d_rec[s], at * cols + 2), ndim,
                                                    be.ptr(d_rec[s], at * cols + 2 + ndim), cols)
                rb = L.world_hip_realtime_add(hs[1], s, f0.ctypes.data_as(_dp), n, be.ptr(dec[s][0], at * nb),
                                              be.ptr(dec[s][1], at * nb), nb)
                assert ra == rb and ra in (0, 1), (ra, rb, be.error())
                full += ra == 0
                if ra == 1:
                    pos[s] += n
                    k[s] += 1
            for h, buf, pr in zip(hs, bufs, produced):
                assert L.world_hip_realtime_synthesize(h, be.ptr(buf), ip(pr)) == 0, be.error()
            assert np.array_equal(produced[0], produced[1])
            assert np.array_equal(be.host(bufs[0]), be.host(bufs[1]))
            for s in range(2):
                assert L.world_hip_realtime_is_locked(hs[0], s) == L.world_hip_realtime_is_locked(hs[1], s) >= 0
            samples += 64 * int(produced[0].sum())
            if k == [len(chunks[0]), len(chunks[1])] and not produced[0].any():
                break
        assert k == [4, 3] and full > 0 and samples >= 2 * 64 * 40        # both streams ran to their ends; a full ring was met
        assert L.world_hip_realtime_add_coded(hs[0], 0, None, 1, be.ptr(d_rec[0], 2), ndim, be.ptr(d_rec[0], 2 + ndim), cols) == -1
        assert L.world_hip_realtime_add_coded(hs[0], 0, rec[0][:1, 1].copy().ctypes.data_as(_dp), 1, be.ptr(d_rec[0], 2), 0,
                                              be.ptr(d_rec[0], 2 + ndim), cols) == -1 and "number_of_dimensions" in be.error()
    finally:
        for h in hs:
            L.world_hip_realtime_destroy(h)


# ---- the tests --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,fft,ndim", SHAPES)
def test_coded_records_equal_decode_then_synthesis_and_the_reference(be, port_oracle, fs, fft, ndim):
    case_coded_records(be, port_oracle, port_oracle, fs, fft, ndim)


@pytest.mark.parametrize("wire", [0, 1])
@pytest.mark.parametrize("fs,fft,ndim", SHAPES)
def test_f64_and_f32_records_equal_unpack_then_synthesis(be, port_oracle, fs, fft, ndim, wire):
    case_plain_records(be, port_oracle, fs, fft, wire)


GOLDEN_ROWS = [("vowel16k_dio", 16000, 1024, 24), ("vowel48k_harvest", 48000, 2048, 60)]


@pytest.mark.parametrize("name,fs,fft,ndim", GOLDEN_ROWS)
def test_recorded_coded_rows_equal_decode_then_synthesis(be, name, fs, fft, ndim):
    case_golden_rows(be, name, fs, fft, ndim)


def test_refusals_leave_the_context_as_new(be, port_oracle):
    case_refusals(be, port_oracle)


def test_pulse_capacity_is_that_of_synthesis_batch(be, port_oracle):
    case_pulse_capacity(be, port_oracle)


def test_realtime_add_coded_equals_decode_then_add(be, port_oracle):
    case_realtime(be, port_oracle)


def test_staging_is_counted_in_the_workspace(lib, port_oracle):
    """wire 0 stages nothing; wires 1 and 2 hold 8 + 16 nb bytes per frame below the synthesis stage's arrays"""
    fs, fft, ndim = 48000, 2048, 60
    c = case_of(port_oracle, fs, fft, ndim)
    held = {}
    for wire in (0, 2):
        ctx = lib.world_hip_create(0, None)
        try:
            rc, _ = Backend(lib, ctx).records(fs, fft, N_FRAMES, c["blocks"][wire], wire, ndim)
            assert rc == 0
            held[wire] = lib.world_hip_workspace_bytes(ctx)
        finally:
            lib.world_hip_destroy(ctx)
    staged = int(N_FRAMES.sum()) * (8 + 16 * c["nb"])
    assert held[2] - held[0] >= staged
