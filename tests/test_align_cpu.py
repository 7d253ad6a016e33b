"""Alignment by dynamic time warping (include/world_hip.h: world_hip_align_batch) through the host-compiled kernels
(tests/emu/libworld_emu.so), against a NumPy statement of the header's rules written here.  The cases are functions of a
backend, so that tests/test_align_gpu.py runs the same ones through the shipped library.

Tolerances.  Every step is a specified IEEE operation (subtract, multiply, add in ascending k, square root, add, compare),
so the paths, K, both maps and D are compared bit for bit; mcd_db to 2 ulp (the constant (10 / ln 10) sqrt(2) may be
spelled with another rounding)."""
import ctypes as C

import numpy as np
import pytest

import backends
from backends import cpu_backend, lib  # noqa: F401 (lib: a fixture)

_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_longlong)
OUTPUTS = ("path", "path_len", "summary", "map_b", "map_a")
SENTINEL = -7


# ---- the host statement (NumPy) ------------------------------------------------------------------------------------------
def local_cost(A, B):
    """c(i, j) = sqrt(sum over k ascending of (a_k - b_k) * (a_k - b_k)): a loop over k, separate * and +"""
    s = np.zeros((len(A), len(B)))
    with np.errstate(all="ignore"):
        for k in range(A.shape[1]):
            d = A[:, k][:, None] - B[:, k][None, :]
            s = s + d * d
        return np.sqrt(s)


def statement(A, B):
    """A [n_a, D], B [n_b, D] -> (D(n_a-1, n_b-1), path [K, 2], map_b [n_b], map_a [n_a]): the recurrence diagonal by
    diagonal; the first of (diagonal, i - 1, j - 1) that attains the minimum is taken -- a later candidate replaces an
    earlier one only if it is strictly smaller (so never when either is NaN)"""
    na, nb = len(A), len(B)
    c = local_cost(A, B)
    D = np.zeros((na, nb))
    frm = np.zeros((na, nb), dtype=np.int8)
    with np.errstate(all="ignore"):
        for d in range(na + nb - 1):
            i = np.arange(max(0, d - (nb - 1)), min(d, na - 1) + 1)
            j = d - i
            best, code = np.zeros(len(i)), np.full(len(i), 3)
            m = (i > 0) & (j > 0)
            best[m], code[m] = D[i[m] - 1, j[m] - 1], 0
            for which, m, pi, pj in ((1, i > 0, np.maximum(i - 1, 0), j), (2, j > 0, i, np.maximum(j - 1, 0))):
                v = D[pi, pj]
                take = m & ((code == 3) | (v < best))
                best[take], code[take] = v[take], which
            D[i, j] = np.where(code == 3, c[i, j], c[i, j] + best)
            frm[i, j] = code
    i, j, back = na - 1, nb - 1, []
    while True:
        back.append((i, j))
        if i == 0 and j == 0:
            break
        f = frm[i, j]
        i, j = i - (f != 2), j - (f != 1)
    path = np.array(back[::-1], dtype=np.int32)
    map_b = np.array([0.5 * (path[path[:, 1] == q, 0].min() + path[path[:, 1] == q, 0].max()) for q in range(nb)]) \
        if nb <= 600 else _mid_points(path[:, 1], path[:, 0], nb)
    map_a = np.array([0.5 * (path[path[:, 0] == q, 1].min() + path[path[:, 0] == q, 1].max()) for q in range(na)]) \
        if na <= 600 else _mid_points(path[:, 0], path[:, 1], na)
    return D[na - 1, nb - 1], path, map_b, map_a


def _mid_points(key, val, n):
    lo, hi = np.full(n, np.iinfo(np.int64).max), np.full(n, -1)
    np.minimum.at(lo, key, val)
    np.maximum.at(hi, key, val)
    return 0.5 * (lo + hi)


def mcd_db(D, K):
    return 10 / np.log(10) * np.sqrt(2) * D / K


# ---- a backend: the C call on arrays that live where the library wants them ---------------------------------------------
class Backend(backends.Backend):
    """world_hip_align_batch on the arrays of backends.Backend"""

    def buffers(self, P, p_stride, map_stride, want=OUTPUTS):
        shapes = dict(path=((P, p_stride, 2), np.int32), path_len=((P,), np.int32), summary=((P, 3), np.float64),
                      map_b=((P, map_stride), np.float64), map_a=((P, map_stride), np.float64))
        return {k: self.dev(np.full(shapes[k][0], SENTINEL, dtype=shapes[k][1])) for k in want}

    def call(self, P, n_dims, d_a, a_off, a_row, na, a_stride, d_b, b_off, b_row, nb, b_stride, p_stride, map_stride, outs):
        """the C call itself: d_a / d_b device arrays, *_off doubles into them, outs = {name: device array} (absent: NULL)"""
        arr = lambda v, dt: None if v is None else np.ascontiguousarray(v, dtype=dt)
        a_row, b_row, na, nb = arr(a_row, np.int64), arr(b_row, np.int64), arr(na, np.int32), arr(nb, np.int32)
        ptr = lambda v, tp: None if v is None else v.ctypes.data_as(tp)
        o = lambda k: C.c_void_p(self.addr(outs[k])) if k in outs else None
        return self.lib.world_hip_align_batch(
            self.ctx, P, n_dims, None if d_a is None else C.c_void_p(self.addr(d_a) + 8 * a_off), ptr(a_row, _lp), ptr(na, _ip),
            a_stride, None if d_b is None else C.c_void_p(self.addr(d_b) + 8 * b_off), ptr(b_row, _lp), ptr(nb, _ip), b_stride,
            p_stride, o("path"), o("path_len"), o("summary"), map_stride, o("map_b"), o("map_a"))

    def align(self, store_a, store_b, n_dims, a_row, na, a_stride, b_row, nb, b_stride, a_off=0, b_off=0, want=OUTPUTS,
              p_stride=None, map_stride=None):
        """store_a / store_b: flat float64 arrays (store_b None: B lives in A's array, d_a and d_b alias) -> (rc, outputs
        on the host, pre-filled with SENTINEL)"""
        P = len(na)
        p_stride = int(np.max(np.add(na, nb))) + 2 if p_stride is None else p_stride
        map_stride = int(max(np.max(na), np.max(nb))) + 3 if map_stride is None else map_stride
        d_a = self.dev(store_a)
        d_b = d_a if store_b is None else self.dev(store_b)
        outs = self.buffers(P, p_stride, map_stride, want)
        rc = self.call(P, n_dims, d_a, a_off, a_row, na, a_stride, d_b, b_off, b_row, nb, b_stride, p_stride, map_stride, outs)
        return rc, {k: self.host(v) for k, v in outs.items()}


be = cpu_backend(Backend)


# ---- helpers -------------------------------------------------------------------------------------------------------------
def frames_of(store, off, row, n, stride, n_dims):
    """the frames the addressing rule names: frame i = the n_dims doubles at off + (row + i) * stride"""
    at = off + (row + np.arange(n))[:, None] * stride + np.arange(n_dims)[None, :]
    return store[at]


def dense(pairs, stride=None, off=0, seed=0):
    """pairs [(A, B)] -> the dense layout: (store_a, store_b, a_row, na, b_row, nb, stride), NaN wherever no frame lies"""
    D = pairs[0][0].shape[1]
    stride = stride or D
    out = []
    for side in (0, 1):
        F = max(len(p[side]) for p in pairs)
        s = np.full((len(pairs), F, stride), np.nan)
        for u, p in enumerate(pairs):
            s[u, :len(p[side]), off:off + D] = p[side]
        out.append((s.reshape(-1), np.arange(len(pairs)) * F, np.array([len(p[side]) for p in pairs], dtype=np.int32)))
    return out[0][0], out[1][0], out[0][1], out[0][2], out[1][1], out[1][2], stride


def check_pair(outs, u, want, na, nb, finite=True):
    """pair u of the outputs against the statement's (D, path, map_b, map_a), and the sentinels beyond its counts"""
    D, path, map_b, map_a = want
    K = len(path)
    if "path_len" in outs:
        assert outs["path_len"][u] == K
    if "path" in outs:
        assert np.array_equal(outs["path"][u, :K], path), f"pair {u}: the path differs"
        assert np.all(outs["path"][u, K:] == SENTINEL), "path rows beyond K were written"
    if "summary" in outs:
        s = outs["summary"][u]
        assert s[1] == K
        if finite:
            assert s[0] == D, (s[0], D)
            m = mcd_db(D, K)
            assert abs(s[2] - m) <= 2 * np.spacing(abs(m)), (s[2], m)
    if "map_b" in outs:
        assert np.array_equal(outs["map_b"][u, :nb], map_b)
        assert np.all(outs["map_b"][u, nb:] == SENTINEL), "map_b entries beyond n_b were written"
    if "map_a" in outs:
        assert np.array_equal(outs["map_a"][u, :na], map_a)
        assert np.all(outs["map_a"][u, na:] == SENTINEL), "map_a entries beyond n_a were written"


def run_dense(be, pairs, stride=None, off=0, want=OUTPUTS):
    D = pairs[0][0].shape[1]
    sa, sb, ar, na, br, nb, stride = dense(pairs, stride, off)
    rc, outs = be.align(sa, sb, D, ar, na, stride, br, nb, stride, a_off=off, b_off=off, want=want)
    assert rc == 0, be.error()
    return outs


def check_dense(be, pairs, stride=None, off=0):
    outs = run_dense(be, pairs, stride, off)
    wants = [statement(A, B) for A, B in pairs]
    for u, (A, B) in enumerate(pairs):
        check_pair(outs, u, wants[u], len(A), len(B))
    return outs, wants


def random_pair(rng, na, nb, D):
    return rng.standard_normal((na, D)), rng.standard_normal((nb, D))


# ---- the cases -----------------------------------------------------------------------------------------------------------
def case_degenerate(be):
    rng = np.random.default_rng(1)
    check_dense(be, [random_pair(rng, na, nb, 3) for na, nb in ((1, 1), (1, 5), (5, 1), (2, 2))])


def case_identical(be):
    A = np.random.default_rng(2).standard_normal((37, 5))
    outs, wants = check_dense(be, [(A, A.copy())])
    assert outs["summary"][0, 0] == 0.0 and outs["path_len"][0] == 37
    assert np.array_equal(outs["path"][0, :37], np.stack([np.arange(37)] * 2, axis=1))
    assert np.array_equal(outs["map_b"][0, :37], np.arange(37.0)) and np.array_equal(outs["map_a"][0, :37], np.arange(37.0))


def case_repeats(be):
    """B = A with frames held by a known pattern: only the cells (hold[j], j) cost nothing, so D == 0 pins the path to
    them; the held side's map holds the mid-points of the runs"""
    A = np.random.default_rng(3).standard_normal((9, 4))
    hold = np.array([0, 0, 1, 2, 2, 2, 3, 4, 5, 5, 5, 5, 6, 7, 8, 8])
    B = A[hold]
    mid = np.array([0.5 * (np.flatnonzero(hold == i).min() + np.flatnonzero(hold == i).max()) for i in range(9)])
    outs, _ = check_dense(be, [(A, B), (B, A)])
    assert outs["summary"][0, 0] == 0.0 and outs["summary"][1, 0] == 0.0
    assert outs["path_len"][0] == 16 and np.array_equal(outs["path"][0, :16], np.stack([hold, np.arange(16)], axis=1))
    assert np.array_equal(outs["map_b"][0, :16], hold.astype(np.float64)) and np.array_equal(outs["map_a"][0, :9], mid)
    assert np.array_equal(outs["map_b"][1, :9], mid) and np.array_equal(outs["map_a"][1, :16], hold.astype(np.float64))


def case_ties(be):
    rng = np.random.default_rng(4)
    pairs = [(rng.integers(0, 3, (na, 2)).astype(np.float64), rng.integers(0, 3, (nb, 2)).astype(np.float64))
             for na, nb in ((9, 11), (12, 7), (8, 8), (20, 21))]
    pairs.append((np.zeros((6, 2)), np.zeros((7, 2))))      # every cell ties: the diagonal wins, then i - 1
    check_dense(be, pairs)


# sizes around the DP workgroup (512 threads), the cost tile (16 x 32), the cells fetched ahead (4 x 512 = 2048 per
# diagonal) and a long side against a short one (the diagonal buffers hold the SHORTER side + 1: no diagonal is chunked)
EDGES = [(255, 257), (256, 256), (257, 255), (300, 70), (70, 300), (513, 64), (515, 520), (16, 32), (17, 33), (3000, 40),
         (2050, 2060)]


def case_edge(be, na, nb):
    check_dense(be, [random_pair(np.random.default_rng(na * 7919 + nb), na, nb, 3)])


DIMS = [1, 24, 59, 60, 256]


def case_dims(be, D):
    rng = np.random.default_rng(D)
    check_dense(be, [random_pair(rng, 33, 47, D), random_pair(rng, 18, 5, D)])


def case_addressing(be):
    rng = np.random.default_rng(6)
    # a row stride larger than n_dims, and a column offset
    check_dense(be, [random_pair(rng, 21, 30, 6), random_pair(rng, 40, 17, 6)], stride=11, off=3)
    # a packed block of coded records [tpos, f0, c0, c1 .. c7, bands x 3]: utterances by prefix sum, c0 skipped, d_a == d_b
    counts, cols, D = np.array([7, 12, 5, 9]), 2 + 8 + 3, 7
    block = rng.standard_normal((counts.sum(), cols))
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ua, ub = np.array([0, 2, 3, 1]), np.array([1, 0, 3, 2])
    rc, outs = be.align(block.reshape(-1), None, D, first[ua], counts[ua], cols, first[ub], counts[ub], cols, a_off=3, b_off=3)
    assert rc == 0, be.error()
    for u in range(4):
        A = frames_of(block.reshape(-1), 3, first[ua[u]], counts[ua[u]], cols, D)
        B = frames_of(block.reshape(-1), 3, first[ub[u]], counts[ub[u]], cols, D)
        assert np.array_equal(A, block[first[ua[u]]:first[ua[u]] + counts[ua[u]], 3:10])
        check_pair(outs, u, statement(A, B), len(A), len(B))
    assert outs["summary"][2, 0] == 0.0                     # (utterance 3 against itself)


def mixed_pairs(seed):
    rng = np.random.default_rng(seed)
    return [random_pair(rng, na, nb, 5) for na, nb in ((40, 55), (3, 90), (130, 7), (1, 1), (64, 64))]


def case_batch_independence(be):
    pairs = mixed_pairs(7)
    outs, wants = check_dense(be, pairs)
    for u, pair in enumerate(pairs):
        alone = run_dense(be, [pair])
        check_pair(alone, 0, wants[u], len(pair[0]), len(pair[1]))
        K = alone["path_len"][0]
        assert np.array_equal(alone["summary"][0], outs["summary"][u]) and np.array_equal(alone["path"][0, :K], outs["path"][u, :K])
    order = [3, 0, 4, 2, 1]
    shuffled = run_dense(be, [pairs[u] for u in order])
    for at, u in enumerate(order):
        K = outs["path_len"][u]
        assert shuffled["path_len"][at] == K and np.array_equal(shuffled["path"][at, :K], outs["path"][u, :K])
        assert np.array_equal(shuffled["summary"][at], outs["summary"][u])
        na, nb = len(pairs[u][0]), len(pairs[u][1])
        assert np.array_equal(shuffled["map_b"][at, :nb], outs["map_b"][u, :nb])
        assert np.array_equal(shuffled["map_a"][at, :na], outs["map_a"][u, :na])


def case_optional_outputs(be):
    pairs = mixed_pairs(8)
    full = run_dense(be, pairs)
    for gone in OUTPUTS:
        part = run_dense(be, pairs, want=tuple(k for k in OUTPUTS if k != gone))
        assert gone not in part
        for k, v in part.items():
            assert np.array_equal(v, full[k]), f"without {gone}, {k} changed"
    sa, sb, ar, na, br, nb, stride = dense(pairs)
    rc, none = be.align(sa, sb, 5, ar, na, stride, br, nb, stride, want=())
    assert rc == 0 and none == {}


def case_refusals(be):
    pairs = mixed_pairs(9)[:2]
    sa, sb, ar, na, br, nb, stride = dense(pairs)
    d_a, d_b = be.dev(sa), be.dev(sb)
    P, S, M = 2, int(np.max(na + nb)) - 1, int(max(na.max(), nb.max()))
    limit = be.lib.world_hip_align_workspace_cells()
    assert limit == 1 << 26
    good = dict(P=P, n_dims=5, d_a=d_a, a_off=0, a_row=ar, na=na, a_stride=stride, d_b=d_b, b_off=0, b_row=br, nb=nb,
                b_stride=stride, p_stride=S, map_stride=M)
    outs = be.buffers(P, S, M)
    assert be.call(outs=outs, **good) == 0, be.error()
    # (what is wrong, a word the message must hold: the refusal has to be the right one)
    bad = [(dict(P=0), "n_pairs"), (dict(P=-1), "n_pairs"), (dict(d_a=None), "null"), (dict(d_b=None), "null"),
           (dict(a_row=None), "null"), (dict(b_row=None), "null"), (dict(na=None), "null"), (dict(nb=None), "null"),
           (dict(na=[na[0], 0]), "frames"), (dict(nb=[-3, nb[1]]), "frames"), (dict(n_dims=0), "n_dims"),
           (dict(n_dims=257), "n_dims"), (dict(a_stride=4), "strides"), (dict(b_stride=4), "strides"),
           (dict(a_row=[0, -1]), "negative row"), (dict(b_row=[-5, 0]), "negative row"), (dict(p_stride=S - 1), "p_stride"),
           (dict(map_stride=M - 1), "map_stride"),
           (dict(na=[8193, na[1]], nb=[8192, nb[1]], p_stride=20000, map_stride=9000), "cells")]
    for change, word in bad:
        outs = be.buffers(P, change.get("p_stride", S), change.get("map_stride", M))
        rc = be.call(outs=outs, **{**good, **change})
        assert rc != 0, f"{change} was accepted"
        assert word in be.error(), (change, be.error())
        for k, v in outs.items():
            assert np.all(be.host(v) == SENTINEL), f"{change}: {k} was touched"
    # each map has its own condition: map_b needs n_b entries, map_a n_a.  The pairs are 40 x 55 and 3 x 90, so a stride
    # of 89 is short for map_b alone (n_b = 90) and fine for map_a (n_a <= 40); for the mirrored pairs the other way round
    assert M == 90 and int(na.max()) == 40
    for flipped, short, fine, word in ((False, "map_b", "map_a", "n_b"), (True, "map_a", "map_b", "n_a")):
        g = dict(good, d_a=d_b, d_b=d_a, a_row=br, b_row=ar, na=nb, nb=na) if flipped else good
        only = lambda k: {n: v for n, v in be.buffers(P, S, 89).items() if n != k}
        outs = only(fine)
        assert be.call(outs=outs, **{**g, "map_stride": 89}) != 0 and "map_stride" in be.error() and word in be.error(), be.error()
        assert all(np.all(be.host(v) == SENTINEL) for v in outs.values())
        assert be.call(outs=only(short), **{**g, "map_stride": 89}) == 0, be.error()
    # a stride that is short only for an output that is not asked for is no reason to refuse
    outs = {k: v for k, v in be.buffers(P, S, M).items() if k != "path"}
    assert be.call(outs=outs, **{**good, "p_stride": 0}) == 0, be.error()
    outs = {k: v for k, v in be.buffers(P, S, M).items() if not k.startswith("map")}
    assert be.call(outs=outs, **{**good, "map_stride": 0}) == 0, be.error()
    # and the call after the refusals is a fresh one's
    outs = be.buffers(P, S, M)
    assert be.call(outs=outs, **good) == 0
    for u, (A, B) in enumerate(pairs):
        check_pair({k: be.host(v) for k, v in outs.items()}, u, statement(A, B), len(A), len(B))


def check_monotone(path, K, na, nb):
    p = path[:K].astype(np.int64)
    assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (na - 1, nb - 1)
    assert np.all((p >= 0) & (p < [na, nb]))
    step = np.diff(p, axis=0)
    assert np.all((step >= 0) & (step <= 1)) and np.all(step.sum(axis=1) >= 1)


def case_non_finite(be):
    rng = np.random.default_rng(10)
    clean = random_pair(rng, 45, 38, 4)
    A, B = random_pair(rng, 50, 61, 4)
    A[7, 1] = np.nan; A[20:23] = np.inf; B[3, 0] = np.inf; B[40, 2] = np.nan; B[60] = np.nan
    want = statement(*clean)
    for pairs, at in (([(A, B), clean], 1), ([clean, (A, B)], 0)):
        outs = run_dense(be, pairs)
        check_pair(outs, at, want, 45, 38)
        dirty = 1 - at
        K = outs["path_len"][dirty]
        assert 61 <= K <= 50 + 61 - 1 and outs["summary"][dirty, 1] == K
        check_monotone(outs["path"][dirty], K, 50, 61)
        assert np.all(outs["path"][dirty, K:] == SENTINEL)
        for name, n, m in (("map_b", 61, 50), ("map_a", 50, 61)):
            v = outs[name][dirty]
            assert np.all((v[:n] >= 0) & (v[:n] <= m - 1)) and np.all(np.diff(v[:n]) >= 0) and np.all(v[n:] == SENTINEL)
        check_pair(outs, dirty, statement(A, B), 50, 61, finite=False)     # (and it is the statement's path, NaN rule included)
    check_pair(run_dense(be, [clean]), 0, want, 45, 38)                    # the next call: as a fresh one


# ---- the CPU runs ----------------------------------------------------------------------------------------------------
def test_degenerate_pairs(be):
    case_degenerate(be)


def test_identical_sequences_give_the_diagonal(be):
    case_identical(be)


def test_repeated_frames_give_the_hold_pattern_and_mid_points(be):
    case_repeats(be)


def test_ties_follow_the_statement(be):
    case_ties(be)


@pytest.mark.parametrize("na,nb", EDGES)
def test_sizes_around_the_workgroup_tile_and_buffer_edges(be, na, nb):
    case_edge(be, na, nb)


@pytest.mark.parametrize("D", DIMS)
def test_dimensions(be, D):
    case_dims(be, D)


def test_addressing_strides_offsets_packed_rows_and_aliasing(be):
    case_addressing(be)


def test_a_pair_alone_inside_a_batch_and_permuted(be):
    case_batch_independence(be)


def test_each_output_is_optional(be):
    case_optional_outputs(be)


def test_refusals_touch_nothing(be):
    case_refusals(be)


def test_non_finite_features_stay_in_their_pair(be):
    case_non_finite(be)


def test_workspace_is_counted_and_groups_bound_it(lib):
    """the workspace comes from the context's arena: 9 bytes per cell and the walk, for the pairs of one call"""
    c = lib.world_hip_create(0, None)
    try:
        be = Backend(lib, c)
        before = lib.world_hip_workspace_bytes(c)
        rng = np.random.default_rng(11)
        check_dense(be, [random_pair(rng, 300, 200, 2)])
        after = lib.world_hip_workspace_bytes(c)
        assert after >= before and after >= 9 * 300 * 200
        check_dense(be, [random_pair(rng, 100, 100, 2)])
        assert lib.world_hip_workspace_bytes(c) == after
    finally:
        lib.world_hip_destroy(c)
