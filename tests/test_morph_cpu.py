"""Morph of two aligned utterances (include/world_hip.h: world_hip_morph_batch, world_hip_morph_length) through the
host-compiled kernels (tests/emu/libworld_emu.so), against a NumPy statement of the header's rules written here.  The
reference has no morph: the statement is the oracle.  The cases are functions of a backend, so that
tests/test_morph_gpu.py runs the same ones through the shipped library.  Paths come from hand-made monotone walks (long
horizontal and vertical runs included) and from the emulated world_hip_align_batch.

Tolerances.  Positions, the blends (1.0 - w) * a + w * b and (1.0 - rho) * a + rho * b and every rho == 0 / rho == 1 /
w == 0 shortcut are the same IEEE operations in the same order under -ffp-contract=off: equality.  Rows and F0 that went
through log / exp: 1e-13 relative, the bar tests/test_modify_cpu.py holds modify_warp_sp to (the device log / exp differ
from libm in the last bits)."""
import ctypes as C

import numpy as np
import pytest

import test_align_cpu as al
import test_modify_frames_cpu as mf
from backends import SENTINEL_F64 as SENTINEL, cpu_backend, lib, rel  # noqa: F401 (lib: a fixture)

_ip = C.POINTER(C.c_int)
COUNTS = [(1, 1), (1, 7), (7, 1), (5, 9), (40, 23), (300, 517)]
TIME_RATES = [0.0, 1e-9, 0.25, 0.3, 1.0 / 3.0, 0.5, 0.9, 1.0 - 1e-9, 1.0]
TOL = 1e-13


# ---- the host statement (NumPy) ------------------------------------------------------------------------------------------
def morph_length(na, nb, r):
    return int(np.floor((1.0 - r) * (na - 1) + r * (nb - 1))) + 1


def positions(path, na, nb, r):
    """header steps 1-2 for one pair: path [K, 2] (None: frame for frame) -> (sA, sB), each [n_out]"""
    n_out = morph_length(na, nb, r)
    m = np.arange(n_out, dtype=np.float64)
    if path is None:
        return m.copy(), m.copy()
    i, j = path[:, 0].astype(np.int64), path[:, 1].astype(np.int64)
    t = (1.0 - r) * i + r * j
    assert np.all(np.diff(t) >= 0), "rounding must leave t non-decreasing"
    lo = np.searchsorted(t, m, side="left")
    hi = np.searchsorted(t, m, side="right") - 1
    assert lo.max() < len(t)
    before = np.maximum(lo - 1, 0)
    with np.errstate(all="ignore"):
        w = (m - t[before]) / (t[lo] - t[before])
        between_a = i[before] + w * (i[lo] - i[before])
        between_b = j[before] + w * (j[lo] - j[before])
    at = t[lo] == m
    assert np.all(at | (lo > 0))
    sa = np.where(at, 0.5 * (i[lo] + i[hi]), between_a)
    sb = np.where(at, 0.5 * (j[lo] + j[hi]), between_b)
    return np.minimum(np.maximum(sa, 0.0), na - 1.0), np.minimum(np.maximum(sb, 0.0), nb - 1.0)


def rate_of(curve, scalar, n_out):
    """header step 4: the curve's value (not finite: 0, else clamped) or the pair's own"""
    if curve is None:
        return np.full(n_out, float(scalar))
    v = np.asarray(curve[:n_out], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), np.minimum(np.maximum(v, 0.0), 1.0), 0.0)


def rows_at(rows, s):
    k, k1, w, blend = mf.source_position(s, len(s), len(rows))
    return mf.blend_rows(rows, k, k1, w, blend)


def f0_at(f0, s):
    return mf.statement(f0, None, None, len(s), 0, 0, time_map=s)[0]


def mix(a, b, rho, geometric):
    """header steps 5-7 on rows (or F0 values) already voiced on both sides; rho broadcasts over the bins"""
    with np.errstate(all="ignore"):
        mixed = np.exp((1.0 - rho) * np.log(a) + rho * np.log(b)) if geometric else (1.0 - rho) * a + rho * b
    return np.where(rho == 0.0, a, np.where(rho == 1.0, b, mixed))


def statement(A, B, path, rates, curves=None):
    """One pair.  A, B = (f0 [n], sp [n, nb], ap [n, nb]) (members may be None), rates = (time, f0, sp, ap), curves =
    dict(f0=, sp=, ap=) of per-frame arrays.  -> (f0', sp', ap', sA, sB, through) with n_out frames; through marks the F0
    frames that went through log / exp."""
    curves = curves or {}
    na, nb = len(next(x for x in A if x is not None)), len(next(x for x in B if x is not None))
    sa, sb = positions(path, na, nb, rates[0])
    n_out = len(sa)
    f0 = sp = ap = through = None
    if A[0] is not None:
        rho = rate_of(curves.get("f0"), rates[1], n_out)
        fa, fb = f0_at(A[0], sa), f0_at(B[0], sb)
        va, vb = mf.voiced(fa), mf.voiced(fb)
        with np.errstate(all="ignore"):
            geo = np.exp((1.0 - rho) * np.log(fa) + rho * np.log(fb))
        between = np.where(va & vb, geo, np.where(va, np.where(1.0 - rho > 0.5, fa, 0.0),
                                                   np.where(vb, np.where(rho > 0.5, fb, 0.0), 0.0)))
        f0 = np.where(rho == 0.0, fa, np.where(rho == 1.0, fb, between))
        through = va & vb & (rho != 0.0) & (rho != 1.0)
    if A[1] is not None:
        sp = mix(rows_at(A[1], sa), rows_at(B[1], sb), rate_of(curves.get("sp"), rates[2], n_out)[:, None], True)
    if A[2] is not None:
        ap = mix(rows_at(A[2], sa), rows_at(B[2], sb), rate_of(curves.get("ap"), rates[3], n_out)[:, None], False)
    return f0, sp, ap, sa, sb, through


# ---- a backend: the C calls on arrays that live where the library wants them ---------------------------------------------
class Backend(al.Backend):
    """world_hip_morph_batch (and, from tests/test_align_cpu.py, world_hip_align_batch) on the arrays of backends.Backend"""

    def vp(self, d):
        return C.c_void_p(self.addr(d)) if d is not None else None

    def morph_call(self, P, fs, fft, na, a_stride, d_a, nb, b_stride, d_b, p_stride, d_path, d_len, morphs, curves, O, outs,
                   d_pos):
        """the C call itself on device arrays: d_a / d_b / outs = (f0, sp, ap) with None members, curves = dict of device
        arrays by WorldHipMorphCurves field, d_pos = (pos_a, pos_b)"""
        from world_amd.api import WorldHipMorphCurves
        arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.int32)
        na, nb = arr(na), arr(nb)
        ptr = lambda v: None if v is None else v.ctypes.data_as(_ip)
        cv = WorldHipMorphCurves(**{k: self.addr(v) for k, v in curves.items()}) if curves else None
        return self.lib.world_hip_morph_batch(
            self.ctx, P, fs, fft, ptr(na), a_stride, self.vp(d_a[0]), self.vp(d_a[1]), self.vp(d_a[2]), ptr(nb), b_stride,
            self.vp(d_b[0]), self.vp(d_b[1]), self.vp(d_b[2]), p_stride, self.vp(d_path), self.vp(d_len), morphs,
            C.byref(cv) if cv is not None else None, O, self.vp(outs[0]), self.vp(outs[1]), self.vp(outs[2]),
            self.vp(d_pos[0]), self.vp(d_pos[1]))

    def morph(self, fs, fft, na, nb, A, B, paths, rates, curves=None, O=None, want=(True, True, True), want_pos=(True, True),
              p_stride=None):
        """A, B = (f0 [P, Fa], sp [P, Fa, nb], ap) host arrays (None members allowed, and dropped where `want` says so);
        paths = list of [K, 2] arrays, or None (no path); rates = (time, f0, sp, ap), scalars or per pair; curves =
        dict(f0=, sp=, ap=) of [P, O] host arrays.  -> (rc, f0', sp', ap', pos_a, pos_b) on the host, pre-filled with
        SENTINEL (None where not asked for)"""
        from world_amd.api import morphs
        P = len(na)
        first = lambda T: next(x for x in T if x is not None)
        a_stride, b_stride = first(A).shape[1], first(B).shape[1]
        if O is None:
            O = max(morph_length(int(x), int(y), float(r)) for x, y, r in zip(na, nb, np.broadcast_to(rates[0], (P,)))) + 2
        d_path = d_len = None
        if paths is not None:
            p_stride = int(np.max(np.add(na, nb))) + 1 if p_stride is None else p_stride
            store = np.full((P, p_stride, 2), -99, dtype=np.int32)
            for u, q in enumerate(paths):
                store[u, :len(q)] = q
            d_path, d_len = self.dev(store), self.dev(np.array([len(q) for q in paths], dtype=np.int32))
        pick = lambda T: tuple(self.dev(x) if x is not None and w else None for x, w in zip(T, want))
        d_a, d_b = pick(A), pick(B)
        outs = tuple(self.dev(np.full((P, O) + x.shape[2:], SENTINEL)) if x is not None and w else None for x, w in zip(A, want))
        d_pos = tuple(self.dev(np.full((P, O), SENTINEL)) if w else None for w in want_pos)
        d_cv = {"d_%s_rate" % k: self.dev(np.ascontiguousarray(v, dtype=np.float64)) for k, v in (curves or {}).items()}
        for v in d_cv.values():
            assert tuple(v.shape) == (P, O)
        rc = self.morph_call(P, fs, fft, na, a_stride, d_a, nb, b_stride, d_b, p_stride or 0, d_path, d_len, morphs(P, *rates),
                             d_cv, O, outs, d_pos)
        return (rc, *[self.host(o) if o is not None else None for o in outs + d_pos])

    def modify_frames(self, fs, fft, nf, no, O, f0, sp, ap, time_map):
        """world_hip_modify_frames_batch with a time map alone -> (f0', sp', ap'), SENTINEL beyond"""
        from world_amd.api import WorldHipFrameCurves
        B, F = f0.shape
        nf, no = np.ascontiguousarray(nf, dtype=np.int32), np.ascontiguousarray(no, dtype=np.int32)
        ins = [self.dev(a) for a in (f0, sp, ap)]
        outs = [self.dev(np.full((B, O) + a.shape[2:], SENTINEL)) for a in (f0, sp, ap)]
        tm = self.dev(np.ascontiguousarray(time_map, dtype=np.float64))
        cv = WorldHipFrameCurves(d_time_map=self.addr(tm))
        rc = self.lib.world_hip_modify_frames_batch(self.ctx, B, fs, fft, nf.ctypes.data_as(_ip), F, no.ctypes.data_as(_ip), O,
                                                    None, C.byref(cv), self.vp(ins[0]), self.vp(outs[0]), self.vp(ins[1]),
                                                    self.vp(outs[1]), self.vp(ins[2]), self.vp(outs[2]))
        assert rc == 0, self.error()
        return [self.host(o) for o in outs]


be = cpu_backend(Backend)


# ---- inputs, made once and shared (never changed) ------------------------------------------------------------------------
def random_path(rng, na, nb, stay=0.0):
    """a monotone walk from (0, 0) to (na - 1, nb - 1); stay = the chance to repeat the last step's direction (long runs)"""
    i = j = 0
    cells, last = [(0, 0)], 0
    while (i, j) != (na - 1, nb - 1):
        moves = [d for d in (0, 1, 2) if (d == 2 or i < na - 1) and (d == 1 or j < nb - 1)]
        d = last if last in moves and rng.random() < stay else moves[rng.integers(len(moves))]
        i, j, last = i + (d != 2), j + (d != 1), d
        cells.append((i, j))
    return np.array(cells, dtype=np.int32)


def run_path(na, nb):
    """all of A's steps, then all of B's: one vertical and one horizontal run as long as they can be"""
    return np.array([(i, 0) for i in range(na)] + [(na - 1, j) for j in range(1, nb)], dtype=np.int32)


_batches, _aligned = {}, {}


def batch(fs, fft, counts=tuple(COUNTS)):
    """(na, nb, A, B): the ragged sides of tests/test_modify_frames_cpu.py (unvoiced stretches, aperiodicities that leave
    [0.001, 1 - 1e-12], NaN beyond each pair's frames)"""
    key = (fs, fft, counts)
    if key not in _batches:
        na, nb = np.array([c[0] for c in counts], dtype=np.int32), np.array([c[1] for c in counts], dtype=np.int32)
        _batches[key] = (na, nb, mf.ragged(fs, fft, na, seed=fft + 1), mf.ragged(fs, fft, nb, seed=fft + 77))
        for side in _batches[key][2:]:
            for x in side:
                x.setflags(write=False)
    return _batches[key]


def hand_paths(counts=COUNTS, seed=5):
    rng = np.random.default_rng(seed)
    return [random_path(rng, na, nb, stay=0.8 if u % 2 else 0.0) for u, (na, nb) in enumerate(counts)]


def aligned(be, counts=tuple(COUNTS), seed=3):
    """paths and both maps of world_hip_align_batch on random features that drift: (paths, map_b [P, M], map_a [P, M])"""
    key = (id(be), counts, seed)
    if key not in _aligned:
        rng = np.random.default_rng(seed)
        pairs = [(np.cumsum(rng.standard_normal((na, 3)), axis=0), np.cumsum(rng.standard_normal((nb, 3)), axis=0))
                 for na, nb in counts]
        outs = al.run_dense(be, pairs)
        paths = [outs["path"][u, :outs["path_len"][u]].copy() for u in range(len(counts))]
        for u, (na, nb) in enumerate(counts):
            al.check_monotone(outs["path"][u], outs["path_len"][u], na, nb)
        _aligned[key] = (paths, outs["map_b"], outs["map_a"])
    return _aligned[key]


def check_pair_rows(got, want, u, n, exact, what):
    g = got[u, :n]
    if exact:
        assert np.array_equal(g, want, equal_nan=True), (what, u)
    else:
        assert rel(g, want) <= TOL, (what, u, rel(g, want))
    assert np.all(got[u, n:] == SENTINEL), f"{what}: frames at or beyond n_out were written (pair {u})"


def check_against_statement(got, na, nb, A, B, paths, rates, curves=None, exact=False):
    """every output of be.morph() that was asked for against the statement, pair by pair"""
    rc, g_f0, g_sp, g_ap, g_pa, g_pb = got
    P = len(na)
    per = lambda v, u: float(np.broadcast_to(v, (P,))[u])
    for u in range(P):
        side = lambda T, n: tuple(x[u, :n] if x is not None else None for x in T)
        cv = {k: v[u] for k, v in (curves or {}).items()}
        w_f0, w_sp, w_ap, sa, sb, through = statement(side(A, na[u]), side(B, nb[u]), None if paths is None else paths[u],
                                                      [per(r, u) for r in rates], cv)
        n = len(sa)
        assert n == morph_length(int(na[u]), int(nb[u]), per(rates[0], u))
        if g_pa is not None:
            check_pair_rows(g_pa, sa, u, n, True, "pos_a")
        if g_pb is not None:
            check_pair_rows(g_pb, sb, u, n, True, "pos_b")
        if g_f0 is not None:
            g = g_f0[u, :n]
            assert np.array_equal(g[~through], w_f0[~through], equal_nan=True), ("f0", u)
            assert rel(g[through], w_f0[through]) <= (0.0 if exact else TOL), ("f0", u, rel(g[through], w_f0[through]))
            assert np.all(g_f0[u, n:] == SENTINEL)
        if g_sp is not None:
            check_pair_rows(g_sp, w_sp, u, n, exact, "sp")
        if g_ap is not None:
            check_pair_rows(g_ap, w_ap, u, n, True, "ap")


# ---- the cases -----------------------------------------------------------------------------------------------------------
def case_positions(be, r):
    """1: positions bit for bit on hand-made walks (random, with long runs, one run per side) and on align's paths; n_out
    is world_hip_morph_length and the count of frames written; sA and sB non-decreasing and in bounds"""
    counts = COUNTS + [(9, 30), (30, 9)]
    na, nb = np.array([c[0] for c in counts], dtype=np.int32), np.array([c[1] for c in counts], dtype=np.int32)
    runs = [run_path(a, b) for a, b in counts]
    for paths in (hand_paths(counts), runs, aligned(be)[0] + runs[len(COUNTS):]):
        rc, _, _, _, pa, pb = be.morph(16000, 128, na, nb, (np.zeros((len(counts), 300)), None, None),
                                       (np.zeros((len(counts), 517)), None, None), paths, (r, 0.5, 0.5, 0.5),
                                       want=(False, False, False))
        assert rc == 0, be.error()
        for u, (a, b) in enumerate(counts):
            sa, sb = positions(paths[u], a, b, r)
            n = be.lib.world_hip_morph_length(a, b, r)
            assert n == len(sa) and np.count_nonzero(pa[u] != SENTINEL) == n and np.count_nonzero(pb[u] != SENTINEL) == n
            assert np.array_equal(pa[u, :n], sa) and np.array_equal(pb[u, :n], sb), (r, u)
            assert np.all(np.diff(sa) >= 0) and np.all(np.diff(sb) >= 0)
            assert sa[0] >= 0 and sb[0] >= 0 and sa[-1] <= a - 1 and sb[-1] <= b - 1


def case_end_rates_equal_aligns_maps(be):
    """1: time_rate 0 gives sA = m and sB = align's d_map_a bit for bit; time_rate 1 the mirror image"""
    paths, map_b, map_a = aligned(be)
    na, nb = np.array([c[0] for c in COUNTS], dtype=np.int32), np.array([c[1] for c in COUNTS], dtype=np.int32)
    zeros = lambda F: (np.zeros((len(COUNTS), F)), None, None)
    for r in (0.0, 1.0):
        rc, _, _, _, pa, pb = be.morph(16000, 128, na, nb, zeros(300), zeros(517), paths, (r, 0, 0, 0), want=(False,) * 3)
        assert rc == 0, be.error()
        for u, (a, b) in enumerate(COUNTS):
            if r == 0.0:
                assert np.array_equal(pa[u, :a], np.arange(a, dtype=np.float64)) and np.array_equal(pb[u, :a], map_a[u, :a])
                assert np.all(pa[u, a:] == SENTINEL) and np.all(pb[u, a:] == SENTINEL)
            else:
                assert np.array_equal(pb[u, :b], np.arange(b, dtype=np.float64)) and np.array_equal(pa[u, :b], map_b[u, :b])
                assert np.all(pa[u, b:] == SENTINEL) and np.all(pb[u, b:] == SENTINEL)


def case_no_path_is_the_identity(be):
    """1: d_path == NULL: sA = sB = m"""
    n = np.array([1, 7, 40, 300], dtype=np.int32)
    zeros = (np.zeros((4, 300)), None, None)
    for r in (0.0, 0.5, 1.0):
        rc, _, _, _, pa, pb = be.morph(16000, 128, n, n, zeros, zeros, None, (r, 0.5, 0.5, 0.5), want=(False,) * 3)
        assert rc == 0, be.error()
        for u in range(4):
            assert be.lib.world_hip_morph_length(int(n[u]), int(n[u]), r) == n[u]
            m = np.arange(n[u], dtype=np.float64)
            assert np.array_equal(pa[u, :n[u]], m) and np.array_equal(pb[u, :n[u]], m)
            assert np.all(pa[u, n[u]:] == SENTINEL) and np.all(pb[u, n[u]:] == SENTINEL)


def case_statement(be, fs, fft, r):
    """the whole morph of the mixed batch against the statement, rates different per member and per pair"""
    na, nb, A, B = batch(fs, fft)
    P = len(na)
    rates = (r, np.linspace(0.1, 0.9, P), np.linspace(0.8, 0.2, P), np.linspace(0.35, 0.65, P))
    paths = hand_paths()
    got = be.morph(fs, fft, na, nb, A, B, paths, rates)
    assert got[0] == 0, be.error()
    check_against_statement(got, na, nb, A, B, paths, rates)


def case_cross_checks(be, fs, fft):
    """2: feature rates 0 with time_rate 1 are modify_frames_batch(A, time_map = d_map_b), feature rates 1 with time_rate 0
    modify_frames_batch(B, time_map = d_map_a): bit for bit, f0, sp and ap"""
    na, nb, A, B = batch(fs, fft)
    paths, map_b, map_a = aligned(be)
    for rate, tr, src, nf, no, tmap in ((0.0, 1.0, A, na, nb, map_b), (1.0, 0.0, B, nb, na, map_a)):
        rc, g_f0, g_sp, g_ap, _, _ = be.morph(fs, fft, na, nb, A, B, paths, (tr, rate, rate, rate))
        assert rc == 0, be.error()
        O = g_f0.shape[1]
        tm = np.zeros((len(na), O))
        tm[:, :min(O, tmap.shape[1])] = tmap[:, :O]
        w_f0, w_sp, w_ap = be.modify_frames(fs, fft, nf, no, O, *src, time_map=tm)
        for u in range(len(na)):
            n = no[u]
            assert np.array_equal(g_f0[u, :n], w_f0[u, :n], equal_nan=True), (rate, u)
            assert np.array_equal(g_sp[u, :n], w_sp[u, :n]) and np.array_equal(g_ap[u, :n], w_ap[u, :n]), (rate, u)
            assert np.all(g_f0[u, n:] == SENTINEL) and np.all(g_sp[u, n:] == SENTINEL) and np.all(g_ap[u, n:] == SENTINEL)


def case_morph_with_itself(be, fs, fft):
    """3: an utterance against itself, frame for frame: sp and F0 within 1e-13 of the input at any rate, ap within 4 ulp"""
    n = np.array([1, 7, 40, 300], dtype=np.int32)
    f0, sp, ap = mf.ragged(fs, fft, n, seed=13)
    ap = np.clip(ap, 0.001, 1.0 - 1e-12)
    A = (f0, sp, ap)
    rng = np.random.default_rng(1)
    O = 300
    for rates, curves in (((0.5, 0.3, 0.3, 0.3), None), ((0.5, 1.0 / 3.0, 0.9, 1e-9), None),
                          ((0.5, 0, 0, 0), dict(f0=rng.random((4, O)), sp=rng.random((4, O)), ap=rng.random((4, O))))):
        rc, g_f0, g_sp, g_ap, _, _ = be.morph(fs, fft, n, n, A, A, None, rates, curves, O=O)
        assert rc == 0, be.error()
        for u in range(4):
            k = n[u]
            v = f0[u, :k] > 0
            assert np.array_equal(g_f0[u, :k][~v], f0[u, :k][~v]) and rel(g_f0[u, :k][v], f0[u, :k][v]) <= TOL
            assert rel(g_sp[u, :k], sp[u, :k]) <= TOL, rel(g_sp[u, :k], sp[u, :k])
            assert np.all(np.abs(g_ap[u, :k] - ap[u, :k]) <= 4 * np.spacing(ap[u, :k]))


def case_voicing_table(be):
    """4: voiced / unvoiced on either side at rho just below, at and just above 0.5 (and at plainly separated rates)"""
    lo, hi = np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)
    rhos = [0.25, 0.49, lo, 0.5, hi, 0.51, 0.75, 0.0, 1.0]
    sides = [(100.0, 200.0), (100.0, 0.0), (0.0, 200.0), (0.0, 0.0), (100.0, np.nan), (np.inf, 200.0), (np.nan, np.inf)]
    fa = np.repeat([s[0] for s in sides], len(rhos))[None]
    fb = np.repeat([s[1] for s in sides], len(rhos))[None]
    curve = np.tile(rhos, len(sides))[None]
    n = np.array([fa.shape[1]], dtype=np.int32)
    got = be.morph(16000, 128, n, n, (fa, None, None), (fb, None, None), None, (0.5, 0.5, 0.5, 0.5), dict(f0=curve), O=int(n[0]))
    assert got[0] == 0, be.error()
    check_against_statement(got, n, n, (fa, None, None), (fb, None, None), None, (0.5, 0.5, 0.5, 0.5), dict(f0=curve))
    table = got[1][0].reshape(len(sides), len(rhos))
    both, only_a, only_b, none = table[0], table[1], table[2], table[3]
    assert abs(both[3] - np.sqrt(100.0 * 200.0)) <= TOL * both[3] and both[7] == 100.0 and both[8] == 200.0
    assert list(only_a[[0, 1, 3, 4, 5, 6, 7, 8]]) == [100.0, 100.0, 0.0, 0.0, 0.0, 0.0, 100.0, 0.0]     # weight 1 - rho above 0.5
    assert only_a[2] == (100.0 if 1.0 - lo > 0.5 else 0.0)
    assert list(only_b[[0, 1, 2, 3, 4, 5, 6, 7, 8]]) == [0.0, 0.0, 0.0, 0.0, 200.0, 200.0, 200.0, 0.0, 200.0]  # weight rho above 0.5
    assert np.all(none == 0.0)
    assert table[4][0] == 100.0 and table[4][6] == 0.0 and np.isnan(table[4][8])      # NaN is not voiced; rho == 1 passes it through
    assert table[5][0] == 0.0 and table[5][6] == 200.0 and np.isinf(table[5][7])      # nor is Inf; rho == 0 passes it through
    assert np.all(table[6][:7] == 0.0)


def case_curves(be, fs, fft):
    """5: per-frame ramps; NaN and out-of-range curve values neutralised for their frame only; a scalar given as a constant
    curve gives the same bits"""
    na, nb, A, B = batch(fs, fft)
    P = len(na)
    paths = hand_paths()
    r = 0.3
    plain = be.morph(fs, fft, na, nb, A, B, paths, (r, 0.25, 0.5, 0.75))
    assert plain[0] == 0, be.error()
    O = plain[1].shape[1]
    const = be.morph(fs, fft, na, nb, A, B, paths, (r, 0.9, 0.9, 0.9), O=O,
                     curves=dict(f0=np.full((P, O), 0.25), sp=np.full((P, O), 0.5), ap=np.full((P, O), 0.75)))
    assert const[0] == 0, be.error()
    for g, w in zip(const[1:], plain[1:]):
        assert np.array_equal(g, w, equal_nan=True)
    ramp = np.tile(np.linspace(0.0, 1.0, O), (P, 1))
    curves = dict(f0=ramp.copy(), sp=ramp[:, ::-1].copy(), ap=ramp ** 2)
    good = be.morph(fs, fft, na, nb, A, B, paths, (r, 0, 0, 0), curves, O=O)
    assert good[0] == 0, be.error()
    check_against_statement(good, na, nb, A, B, paths, (r, 0, 0, 0), curves)
    bad = {k: v.copy() for k, v in curves.items()}
    spots = {0: np.nan, 2: -0.5, 3: 1.5, 5: np.inf, 8: -np.inf}
    for k in bad:
        for at, v in spots.items():
            bad[k][P - 1, at] = v
            bad[k][P - 2, at + 1] = v
    got = be.morph(fs, fft, na, nb, A, B, paths, (r, 0, 0, 0), bad, O=O)
    assert got[0] == 0, be.error()
    check_against_statement(got, na, nb, A, B, paths, (r, 0, 0, 0), bad)
    changed = np.zeros((P, O), dtype=bool)
    for at in spots:
        changed[P - 1, at] = changed[P - 2, at + 1] = True
    for g, w in zip(got[1:4], good[1:4]):                   # every other frame as without them
        assert np.array_equal(g[~changed], w[~changed], equal_nan=True)
    # what a neutralised value stands for: NaN / Inf -> 0 (side A), below 0 -> 0, above 1 -> 1 (side B)
    sa, sb = positions(paths[P - 1], int(na[P - 1]), int(nb[P - 1]), r)
    rows_a, rows_b = rows_at(A[1][P - 1, :na[P - 1]], sa), rows_at(B[1][P - 1, :nb[P - 1]], sb)
    for at, v in spots.items():
        assert np.array_equal(got[2][P - 1, at], rows_b[at] if v == 1.5 else rows_a[at]), at


def case_layout_and_optional_triples(be, fs, fft):
    """6: strides larger than the counts, sentinels beyond n_out, each triple and each position array optional"""
    na, nb, A, B = batch(fs, fft)
    paths = hand_paths()
    rates = (0.4, 0.3, 0.6, 0.5)
    full = be.morph(fs, fft, na, nb, A, B, paths, rates, O=400, p_stride=900)
    assert full[0] == 0, be.error()
    check_against_statement(full, na, nb, A, B, paths, rates)
    pad = lambda T, extra: tuple(np.concatenate([x, np.full((x.shape[0], extra) + x.shape[2:], np.nan)], axis=1) for x in T)
    wide = be.morph(fs, fft, na, nb, pad(A, 5), pad(B, 11), paths, rates, O=400, p_stride=900)
    assert wide[0] == 0, be.error()
    for g, w in zip(wide[1:], full[1:]):
        assert np.array_equal(g, w, equal_nan=True)
    for gone in range(3):
        want = tuple(k != gone for k in range(3))
        part = be.morph(fs, fft, na, nb, A, B, paths, rates, O=400, p_stride=900, want=want, want_pos=(gone != 0, gone != 1))
        assert part[0] == 0, be.error()
        for k, (g, w) in enumerate(zip(part[1:], full[1:])):
            absent = (k < 3 and k == gone) or (k == 3 and gone == 0) or (k == 4 and gone == 1)
            assert (g is None) if absent else np.array_equal(g, w, equal_nan=True), (gone, k)
    none = be.morph(fs, fft, na, nb, A, B, paths, rates, O=400, want=(False,) * 3, want_pos=(False, False))
    assert none[0] == 0 and all(x is None for x in none[1:])


def case_refusals(be):
    """6: every refusal, with nothing written"""
    from world_amd.api import morphs
    fs, fft = 16000, 128
    counts = ((5, 9), (40, 23))
    na, nb, A, B = batch(fs, fft, counts)
    P, Fa, Fb, O, S = 2, 40, 23, 40, 62
    paths = hand_paths(counts)
    store = np.full((P, S, 2), -99, dtype=np.int32)
    for u, q in enumerate(paths):
        store[u, :len(q)] = q
    d_a, d_b = tuple(be.dev(x) for x in A), tuple(be.dev(x) for x in B)
    d_path, d_len = be.dev(store), be.dev(np.array([len(q) for q in paths], dtype=np.int32))
    shapes = [(P, O), (P, O, fft // 2 + 1), (P, O, fft // 2 + 1), (P, O), (P, O)]
    fresh = lambda: [be.dev(np.full(s, SENTINEL)) for s in shapes]
    curve = be.dev(np.full((P, O), 0.5))
    good = dict(P=P, fs=fs, fft=fft, na=na, a_stride=Fa, d_a=d_a, nb=nb, b_stride=Fb, d_b=d_b, p_stride=S, d_path=d_path,
                d_len=d_len, morphs=morphs(P, 0.5), curves={}, O=O)

    def call(outs, **change):
        kw = {**good, **change}
        return be.morph_call(outs=tuple(outs[:3]), d_pos=tuple(outs[3:]), **kw)
    outs = fresh()
    assert call(outs) == 0, be.error()
    assert be.lib.world_hip_morph_length(0, 5, 0.5) == -1 and be.lib.world_hip_morph_length(5, 0, 0.5) == -1
    for r in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
        assert be.lib.world_hip_morph_length(5, 9, r) == -1
    rate = lambda **kw: morphs(P, **{**dict(time_rate=0.5, f0_rate=0.5, sp_rate=0.5, ap_rate=0.5), **kw})
    nine = np.array([9, 23], dtype=np.int32)
    bad = [(dict(P=0), "n_pairs"), (dict(P=-1), "n_pairs"), (dict(P=65536), "n_pairs"), (dict(na=None), "null"),
           (dict(nb=None), "null"), (dict(morphs=None), "null"), (dict(na=[5, 0]), "frames"), (dict(nb=[-1, 23]), "frames"),
           (dict(a_stride=39), "strides"), (dict(b_stride=22), "strides"), (dict(p_stride=61), "p_stride"),
           (dict(d_len=None), "d_path_len"), (dict(d_path=None, d_len=None), "without a path"), (dict(O=30), "o_stride"),
           (dict(morphs=rate(time_rate=[0.5, 1.5])), "rate"), (dict(morphs=rate(f0_rate=[-0.1, 0.5])), "rate"),
           (dict(morphs=rate(sp_rate=[0.5, np.nan])), "rate"), (dict(morphs=rate(ap_rate=[np.inf, 0.5])), "rate"),
           (dict(fft=100), "fft_size"), (dict(fft=64), "fft_size"), (dict(fft=16384), "fft_size"), (dict(fs=0), "fs"),
           (dict(d_a=(None, d_a[1], d_a[2])), "d_f0"), (dict(d_b=(d_b[0], None, d_b[2])), "d_sp"),
           (dict(d_a=(d_a[0], d_a[1], None), d_b=(d_b[0], d_b[1], None)), "d_ap")]
    for change, word in bad:
        outs = fresh()
        assert call(outs, **change) != 0, f"{change} was accepted"
        assert word in be.error(), (change, be.error())
        for o in outs:
            assert np.all(be.host(o) == SENTINEL), f"{change}: an output was touched"
    # an output given without its inputs, and outputs that alias an input or each other
    outs = fresh()
    assert be.morph_call(outs=(None, outs[1], outs[2]), d_pos=(outs[3], outs[4]), **good) != 0 and "d_f0" in be.error()
    same = be.dev(np.array(A[0][:, :O]))
    for kw, word in ((dict(d_a=(same, d_a[1], d_a[2]), outs=(same, outs[1], outs[2]), d_pos=(outs[3], outs[4])), "d_f0_a"),
                     (dict(curves=dict(d_f0_rate=curve), outs=tuple(outs[:3]), d_pos=(curve, outs[4])), "d_f0_rate"),
                     (dict(outs=tuple(outs[:3]), d_pos=(outs[3], outs[3])), "d_pos_b"),
                     (dict(outs=(outs[0], outs[1], outs[1]), d_pos=(outs[3], outs[4])), "d_ap_out")):
        before = np.array(be.host(same))
        assert be.morph_call(**{**good, **kw}) != 0 and "overlaps" in be.error() and word in be.error(), (word, be.error())
        assert np.array_equal(be.host(same), before, equal_nan=True)
    for o in outs:
        assert np.all(be.host(o) == SENTINEL)
    # without a path equal counts are served, and the call after the refusals is a fresh one's
    outs = fresh()
    assert call(outs, d_path=None, d_len=None, na=nine, a_stride=23, d_a=d_b) == 0, be.error()
    outs2 = fresh()
    assert call(outs2) == 0, be.error()
    got = (0, *[be.host(o) for o in outs2])
    check_against_statement(got, na, nb, A, B, paths, (0.5, 0.5, 0.5, 0.5))


def case_garbage_path(be, fs, fft):
    """6: a path align did not write -- indices out of range, K = 0, K above p_stride, no order at all -- gives positions
    within bounds and finite rows, and leaves the neighbouring pairs' outputs bit-identical"""
    counts = ((40, 23), (5, 9), (40, 23))
    na, nb, A, B = batch(fs, fft, counts)
    paths = hand_paths(counts)
    rates = (0.3, 0.5, 0.5, 0.5)
    clean = be.morph(fs, fft, na, nb, A, B, paths, rates, O=45, p_stride=70)
    assert clean[0] == 0, be.error()
    rng = np.random.default_rng(9)
    store = np.full((3, 70, 2), -99, dtype=np.int32)
    for u, q in enumerate(paths):
        store[u, :len(q)] = q
    wild = rng.integers(-1000, 1000, (70, 2)).astype(np.int32)
    wild[::7] = np.iinfo(np.int32).max
    wild[3::7] = np.iinfo(np.int32).min
    d_a, d_b = tuple(be.dev(x) for x in A), tuple(be.dev(x) for x in B)
    from world_amd.api import morphs
    for garbage, K in ((wild, 13), (wild, 0), (wild, -5), (wild, 10 ** 9), (store[1][::-1].copy(), len(paths[1])),
                       (store[1], 0), (store[1], 10 ** 6), (np.zeros((70, 2), dtype=np.int32), 70)):
        s = store.copy()
        s[1] = garbage
        lens = np.array([len(paths[0]), K, len(paths[2])], dtype=np.int32)
        outs = [be.dev(np.full(x.shape, SENTINEL)) for x in clean[1:]]
        rc = be.morph_call(3, fs, fft, na, 40, d_a, nb, 23, d_b, 70, be.dev(s), be.dev(lens), morphs(3, *rates), {}, 45,
                           tuple(outs[:3]), tuple(outs[3:]))
        assert rc == 0, be.error()
        g_f0, g_sp, g_ap, g_pa, g_pb = [be.host(o) for o in outs]
        for g, w in zip((g_f0, g_sp, g_ap, g_pa, g_pb), clean[1:]):
            assert np.array_equal(g[0], w[0], equal_nan=True) and np.array_equal(g[2], w[2], equal_nan=True), K
        n = morph_length(5, 9, 0.3)
        assert np.all((g_pa[1, :n] >= 0) & (g_pa[1, :n] <= 4)) and np.all((g_pb[1, :n] >= 0) & (g_pb[1, :n] <= 8)), K
        assert np.all(np.isfinite(g_sp[1, :n])) and np.all(np.isfinite(g_ap[1, :n]))
        for g in (g_f0, g_sp, g_ap, g_pa, g_pb):
            assert np.all(g[1, n:] == SENTINEL)


def case_batch_independence(be, fs, fft):
    """7: a pair alone against the same pair in a batch, and a permuted batch"""
    na, nb, A, B = batch(fs, fft)
    P = len(na)
    paths = hand_paths()
    O = 520
    rng = np.random.default_rng(4)
    rates = (np.linspace(0.2, 0.8, P), np.linspace(0.1, 0.9, P), 0.5, np.linspace(0.6, 0.4, P))
    curves = dict(sp=rng.random((P, O)))
    whole = be.morph(fs, fft, na, nb, A, B, paths, rates, curves, O=O)
    assert whole[0] == 0, be.error()

    def subset(order):
        take = lambda T: tuple(np.ascontiguousarray(x[order]) for x in T)
        got = be.morph(fs, fft, na[order], nb[order], take(A), take(B), [paths[u] for u in order],
                       tuple(np.broadcast_to(r, (P,))[order] for r in rates), dict(sp=curves["sp"][order]), O=O)
        assert got[0] == 0, be.error()
        for at, u in enumerate(order):
            for g, w in zip(got[1:], whole[1:]):
                assert np.array_equal(g[at], w[u], equal_nan=True), (order, u)
    for u in range(P):
        subset([u])
    subset([3, 0, 5, 2, 1, 4])


# ---- the CPU runs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", TIME_RATES)
def test_positions_are_the_statements_bit_for_bit(be, r):
    case_positions(be, r)


def test_time_rates_0_and_1_give_aligns_maps(be):
    case_end_rates_equal_aligns_maps(be)


def test_no_path_is_the_identity(be):
    case_no_path_is_the_identity(be)


@pytest.mark.parametrize("fft", [128, 1024])
@pytest.mark.parametrize("r", [0.0, 0.3, 1.0])
def test_the_mixed_batch_against_the_statement(be, fft, r):
    case_statement(be, 16000, fft, r)


def test_fft_2048_at_48_khz_against_the_statement(be):
    case_statement(be, 48000, 2048, 1.0 / 3.0)


@pytest.mark.parametrize("fft", [128, 1024])
def test_end_rates_equal_modify_frames_behind_aligns_maps(be, fft):
    case_cross_checks(be, 16000, fft)


@pytest.mark.parametrize("fft", [128, 1024])
def test_morph_of_an_utterance_with_itself(be, fft):
    case_morph_with_itself(be, 16000, fft)


def test_f0_voicing_table(be):
    case_voicing_table(be)


@pytest.mark.parametrize("fft", [128, 1024])
def test_rate_curves(be, fft):
    case_curves(be, 16000, fft)


def test_strides_sentinels_and_optional_triples(be):
    case_layout_and_optional_triples(be, 16000, 128)


def test_refusals_touch_nothing(be):
    case_refusals(be)


@pytest.mark.parametrize("fft", [128, 1024])
def test_a_garbage_path_stays_in_bounds_and_in_its_pair(be, fft):
    case_garbage_path(be, 16000, fft)


def test_a_pair_alone_inside_a_batch_and_permuted(be):
    case_batch_independence(be, 16000, 128)


def test_position_workspace_is_counted(lib):
    """without d_pos_a / d_pos_b the positions live in the context's workspace: 2 n_pairs o_stride doubles"""
    c = lib.world_hip_create(0, None)
    try:
        be = Backend(lib, c)
        na, nb, A, B = batch(16000, 128)
        before = lib.world_hip_workspace_bytes(c)
        got = be.morph(16000, 128, na, nb, A, B, hand_paths(), (0.5, 0.5, 0.5, 0.5), O=600, want_pos=(False, False))
        assert got[0] == 0, be.error()
        check_against_statement(got, na, nb, A, B, hand_paths(), (0.5, 0.5, 0.5, 0.5))
        after = lib.world_hip_workspace_bytes(c)
        assert after >= before and after >= 2 * len(na) * 600 * 8
    finally:
        lib.world_hip_destroy(c)
