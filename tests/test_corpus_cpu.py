"""Training rows of a corpus (include/world_hip.h: world_hip_frame_power_batch / _select_frames_batch / _gather_rows_batch /
_joint_rows_batch) through the host-compiled kernels (tests/emu/libworld_emu.so).  The reference has no such function: THE
HEADER'S STATEMENT IS THE ORACLE, written out here a second time in NumPy.  The cases are functions of a backend, so that
tests/test_corpus_gpu.py runs the same ones through the shipped library.

Bounds (u = 2^-53; none comes from the code under test; the power cases print their largest error / bound).
  power, exact   the header fixes the order of every addition (64 partial sums by index modulo 64, then the tree 32, 16, ..
                 1), so the NumPy restatement of that order is compared bit for bit.
  power, wide    against np.longdouble: every term is non-negative, so a sum of K rounded additions in any order lies within
                 (K + 4) u relative.  P_t is one such sum over the bins and three more operations: (bins + 6) u.  mean_u adds
                 T of them and divides: (T + bins + 10) u.
  selection, gathers   integers and copied bits: equality.
"""
import ctypes as C

import numpy as np
import pytest

import backends
from backends import SENTINEL_F64 as SENTINEL, cpu_backend, lib, same_bits  # noqa: F401 (lib: a fixture)

LD = np.longdouble
U53 = 2.0 ** -53
_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_longlong)
ISENT, BSENT = -7, 0xAB          # what index / count and keep arrays hold before a call
INT_MAX = 2 ** 31 - 1


def _i(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.int32).ctypes.data_as(_ip)


def _l(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.int64).ctypes.data_as(_lp)


def _p(a):
    return None if a is None else C.c_void_p(int(a))


# ---- a backend: the C calls on arrays that live where the library wants them ---------------------------------------------
class Backend(backends.Backend):
    """the four calls (and world_hip_align_batch, for the composition) on the arrays of backends.Backend; the call_*
    methods take addresses (None: NULL) and host count arrays"""

    def workspace(self):
        return int(self.lib.world_hip_workspace_bytes(self.ctx))

    def call_power(self, n_utt, fft_size, n_frames, sp, sp_us, sp_rs, power, power_us, mean):
        return self.lib.world_hip_frame_power_batch(self.ctx, n_utt, fft_size, _i(n_frames), _p(sp), sp_us, sp_rs, _p(power), power_us, _p(mean))

    def call_select(self, n_utt, n_frames, value, value_us, value_s, threshold, scale, mask, mask_us, index, index_us, count, keep, keep_us):
        return self.lib.world_hip_select_frames_batch(self.ctx, n_utt, _i(n_frames), _p(value), value_us, value_s, float(threshold), _p(scale),
                                                      _p(mask), mask_us, _p(index), index_us, _p(count), _p(keep), keep_us)

    def call_gather(self, n_utt, dim, n_src, x, x_us, x_rs, n_out, index, index_us, fill, out, out_us, out_rs):
        return self.lib.world_hip_gather_rows_batch(self.ctx, n_utt, dim, _i(n_src), _p(x), x_us, x_rs, _i(n_out), _p(index), index_us,
                                                    float(fill), _p(out), out_us, out_rs)

    def call_joint(self, n_pairs, dim_a, dim_b, a, a_row, n_a, a_rs, b, b_row, n_b, b_rs, path_len, path, p_stride, sel_a, n_sel_a,
                   sel_a_us, sel_b, n_sel_b, sel_b_us, fill, z, z_row, z_rs):
        return self.lib.world_hip_joint_rows_batch(self.ctx, n_pairs, dim_a, dim_b, _p(a), _l(a_row), _i(n_a), a_rs, _p(b), _l(b_row), _i(n_b),
                                                   b_rs, _i(path_len), _p(path), p_stride, _p(sel_a), _i(n_sel_a), sel_a_us, _p(sel_b),
                                                   _i(n_sel_b), sel_b_us, float(fill), _p(z), _l(z_row), z_rs)

    # -- the calls on host data, every output in a sentinel-filled array that is checked where it must not change
    def power(self, sp, fft_size, slack=0, column=0, want=("power", "mean")):
        """sp: a list of [T][bins] arrays -> (power: a list of [T], mean [U]).  The rows lie in one block of records
        [U][F + 1][column + bins + slack], all SENTINEL beyond the rows"""
        U, bins = len(sp), fft_size // 2 + 1
        n = np.array([len(s) for s in sp], dtype=np.int32)
        F, W = int(n.max()) + 1, column + bins + slack
        block = np.full((U, F, W), SENTINEL)
        for u, s in enumerate(sp):
            block[u, :len(s), column:column + bins] = s
        d_sp = self.dev(block)
        power, mean = self.dev(np.full((U, F + 2), SENTINEL)), self.dev(np.full(U + 1, SENTINEL))
        rc = self.call_power(U, fft_size, n, self.addr(d_sp) + 8 * column, F * W, W, self.addr(power) if "power" in want else None, F + 2,
                             self.addr(mean) if "mean" in want else None)
        assert rc == 0, self.error()
        assert same_bits(self.host(d_sp), block), "the input changed"
        got_p, got_m = self.host(power), self.host(mean)
        assert got_m[U] == SENTINEL and all(np.all(got_p[u, n[u]:] == SENTINEL) for u in range(U)), "written beyond the frames"
        if "power" not in want:
            assert np.all(got_p == SENTINEL)
        return [np.array(got_p[u, :n[u]]) for u in range(U)], np.array(got_m[:U])

    def select(self, values, threshold, scale=None, masks=None, stride=1, want=("index", "count", "keep")):
        """values: a list of [T] arrays -> (index: a list of [count], count [U], keep: a list of [T] uint8)"""
        U = len(values)
        n = np.array([len(v) for v in values], dtype=np.int32)
        F = int(n.max()) + 2
        block = np.full((U, F, stride), SENTINEL)
        for u, v in enumerate(values):
            block[u, :len(v), stride - 1] = v
        d_v = self.dev(block)
        d_scale = None if scale is None else self.dev(np.asarray(scale, dtype=np.float64))
        d_mask = None
        if masks is not None:
            m = np.full((U, F), 1, dtype=np.uint8)
            for u, k in enumerate(masks):
                m[u, :len(k)] = k
            d_mask = self.dev(m)
        index, count, keep = self.dev(np.full((U, F), ISENT, dtype=np.int32)), self.dev(np.full(U + 1, ISENT, dtype=np.int32)), \
            self.dev(np.full((U, F), BSENT, dtype=np.uint8))
        a = lambda d, k=None: None if d is None or (k is not None and k not in want) else self.addr(d)
        rc = self.call_select(U, n, self.addr(d_v) + 8 * (stride - 1), F * stride, stride, threshold, a(d_scale), a(d_mask), F, a(index, "index"), F,
                              a(count, "count"), a(keep, "keep"), F)
        assert rc == 0, self.error()
        assert same_bits(self.host(d_v), block), "the input changed"
        gi, gc, gk = self.host(index), self.host(count), self.host(keep)
        assert gc[U] == ISENT
        out_i, out_k = [], []
        for u in range(U):
            c = int(gc[u]) if "count" in want else int(np.sum(gi[u] != ISENT))
            assert 0 <= c <= n[u]
            assert np.all(gi[u, c:] == ISENT), "index entries at or beyond the count were written"
            assert np.all(gk[u, n[u]:] == BSENT), "keep entries beyond the frames were written"
            out_i.append(np.array(gi[u, :c]))
            out_k.append(np.array(gk[u, :n[u]]))
        return out_i, np.array(gc[:U]), out_k

    def gather(self, x, index, fill=0.0, column=0, slack=0, out_column=0, out_slack=0, n_src=None):
        """x: a list of [T][D] arrays, index: a list of int arrays -> a list of [len(index[u])][D].  Source rows at double
        `column` of records column + D + slack wide, output rows at `out_column` of rows out_column + D + out_slack wide"""
        U, D = len(x), x[0].shape[1]
        n = np.array([len(v) for v in x], dtype=np.int32)
        k = np.array([len(i) for i in index], dtype=np.int32)
        F, I, W, OW = int(n.max()), int(k.max()) + 1, column + D + slack, out_column + D + out_slack
        block = np.full((U, F, W), SENTINEL)
        for u, v in enumerate(x):
            block[u, :len(v), column:column + D] = v
        idx = np.full((U, I), ISENT, dtype=np.int32)
        for u, i in enumerate(index):
            idx[u, :len(i)] = i
        d_x, d_i = self.dev(block), self.dev(idx)
        out = self.dev(np.full((U, I, OW), SENTINEL))
        rc = self.call_gather(U, D, n if n_src is None else n_src, self.addr(d_x) + 8 * column, F * W, W, k, self.addr(d_i), I, fill,
                              self.addr(out) + 8 * out_column, I * OW, OW)
        assert rc == 0, self.error()
        assert same_bits(self.host(d_x), block), "the input changed"
        got = self.host(out)
        assert np.all(got[:, :, :out_column] == SENTINEL) and np.all(got[:, :, out_column + D:] == SENTINEL), "written beyond the row"
        assert all(np.all(got[u, k[u]:] == SENTINEL) for u in range(U)), "rows at or beyond n_out were written"
        return [np.array(got[u, :k[u], out_column:out_column + D]) for u in range(U)]

    def joint(self, A, B, paths, sel_a=None, sel_b=None, fill=0.0, column=0, slack=0, z_slack=0, n_a=None, n_b=None):
        """A, B: lists of [n][Da], [n][Db] arrays (B None: dim_b = 0), paths: a list of [K][2] int arrays, sel_*: lists of int
        arrays -> z [sum K][Da + Db].  A and B are blocks of records, each pair's rows behind the previous pair's and one
        spare row; the pairs' ranges of z abut, one guard row of SENTINEL lies behind the last"""
        P, Da = len(A), A[0].shape[1]
        Db = 0 if B is None else B[0].shape[1]
        K = np.array([len(p) for p in paths], dtype=np.int32)
        S = int(K.max()) + 1
        cells = np.full((P, S, 2), ISENT, dtype=np.int32)
        for u, p in enumerate(paths):
            cells[u, :len(p)] = p
        d_path = self.dev(cells)

        def side(rows, dim):
            n = np.array([len(r) for r in rows], dtype=np.int32)
            first = np.concatenate([[0], np.cumsum(n[:-1] + 1)]).astype(np.int64)
            W = column + dim + slack
            block = np.full((int(first[-1]) + int(n[-1]) + 1, W), SENTINEL)
            for f, r in zip(first, rows):
                block[f:f + len(r), column:column + dim] = r
            return self.dev(block), first, n, W

        def selection(sel):
            if sel is None:
                return None, None, 0
            n = np.array([len(s) for s in sel], dtype=np.int32)
            a = np.full((P, int(n.max()) + 1), ISENT, dtype=np.int32)
            for u, s in enumerate(sel):
                a[u, :len(s)] = s
            return self.dev(a), n, a.shape[1]

        d_a, a_row, na, aw = side(A, Da)
        d_b, b_row, nb, bw = side(B, Db) if Db else (None, None, None, 0)
        d_sa, n_sa, sa_us = selection(sel_a)
        d_sb, n_sb, sb_us = selection(sel_b)
        rows, ZW = int(K.sum()), Da + Db + z_slack
        z_row = np.concatenate([[0], np.cumsum(K[:-1])]).astype(np.int64)
        z = self.dev(np.full((rows + 1, ZW), SENTINEL))
        ad = lambda d, off=0: None if d is None else self.addr(d) + 8 * off
        rc = self.call_joint(P, Da, Db, ad(d_a, column), a_row, na if n_a is None else n_a, aw, ad(d_b, column), b_row, nb if n_b is None else n_b,
                             bw, K, ad(d_path), S, ad(d_sa), n_sa, sa_us, ad(d_sb), n_sb, sb_us, fill, ad(z), z_row, ZW)
        assert rc == 0, self.error()
        got = self.host(z)
        assert np.all(got[rows] == SENTINEL) and np.all(got[:, Da + Db:] == SENTINEL), "written beyond the rows or the row"
        return np.array(got[:rows, :Da + Db])

    def align(self, A, B):
        """the library's own alignment of the pairs (lists of [n][D] arrays) -> a list of paths [K][2]"""
        P, D = len(A), A[0].shape[1]
        na, nb = (np.array([len(r) for r in rows], dtype=np.int32) for rows in (A, B))
        a_row, b_row = (np.concatenate([[0], np.cumsum(n[:-1])]).astype(np.int64) for n in (na, nb))
        d_a, d_b = self.dev(np.vstack(A)), self.dev(np.vstack(B))
        S = int((na + nb).max())
        path, path_len = self.dev(np.zeros((P, S, 2), dtype=np.int32)), self.dev(np.zeros(P, dtype=np.int32))
        rc = self.lib.world_hip_align_batch(self.ctx, P, D, _p(self.addr(d_a)), _l(a_row), _i(na), D, _p(self.addr(d_b)), _l(b_row), _i(nb), D, S,
                                            _p(self.addr(path)), _p(self.addr(path_len)), None, 0, None, None)
        assert rc == 0, self.error()
        cells, K = self.host(path), self.host(path_len)
        return [np.array(cells[u, :K[u]]) for u in range(P)]


be = cpu_backend(Backend)


# ---- the statement --------------------------------------------------------------------------------------------------------
def rule_sum64(x):
    """the header's order: 64 partial sums by index modulo 64, ascending, from +0.0; then partial j takes partial j + s for
    s = 32, 16 .. 1"""
    x = np.asarray(x, dtype=np.float64)
    pad = np.zeros(-len(x) % 64)                                       # (+0.0 added to a sum that began at +0.0: the same sum)
    part = np.zeros(64)
    for row in np.concatenate([x, pad]).reshape(-1, 64):
        part = part + row
    s = 32
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def rule_power(sp, fft_size):
    """(P [T], mean) of envelope rows [T][bins] in the header's order"""
    half = fft_size // 2
    P = np.empty(len(sp))
    for t, row in enumerate(sp):
        inner = np.array(row[:half])
        inner[0] = 0.0                                                 # bins 0 and N / 2 stand apart
        P[t] = ((row[0] + row[half]) + 2.0 * rule_sum64(inner)) / fft_size
    return P, rule_sum64(P) / len(sp)


def wide_power(sp, fft_size):
    half = fft_size // 2
    w = LD(sp)
    P = (w[:, 0] + w[:, half] + 2 * w[:, 1:half].sum(axis=1)) / fft_size
    return P, P.sum() / len(sp)


def rule_select(values, threshold, scale=1.0, mask=None):
    with np.errstate(invalid="ignore"):
        keep = np.asarray(values) >= np.float64(threshold) * np.float64(scale)
    if mask is not None:
        keep = keep & (np.asarray(mask) != 0)
    return np.flatnonzero(keep).astype(np.int32), keep.astype(np.uint8)


def rule_gather(x, index, n_src, fill):
    out = np.full((len(index), x.shape[1]), fill)
    ok = (np.asarray(index) >= 0) & (np.asarray(index) < n_src)
    out[ok] = x[np.asarray(index)[ok]]
    return out


def rule_joint(A, B, path, sel_a, sel_b, fill, n_a=None, n_b=None):
    def half(x, steps, sel, n):
        if x is None:
            return np.empty((len(steps), 0))
        n = len(x) if n is None else n
        steps = np.asarray(steps, dtype=np.int64)
        if sel is not None:
            ok = (steps >= 0) & (steps < len(sel))
            through = np.full(len(steps), -1, dtype=np.int64)
            through[ok] = np.asarray(sel, dtype=np.int64)[steps[ok]]
            steps = through
        return rule_gather(x, steps, n, fill)
    return np.hstack([half(A, path[:, 0], sel_a, n_a), half(B, path[:, 1], sel_b, n_b)])


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def envelopes(fft_size, T, seed):
    return backends.cached(("corpus-sp", fft_size, T, seed), lambda: backends.envelope(16000, fft_size, T, seed))


def rows_of(T, D, seed):
    """distinct, recognisable doubles, a NaN with a payload and a negative zero among them"""
    x = np.random.default_rng(seed).standard_normal((T, D))
    x.reshape(-1)[0] = -0.0
    if x.size > 2:
        x.reshape(-1)[2:3].view(np.uint64)[:] = 0x7FF8000000ABCDEF
    return x


# ---- the cases ------------------------------------------------------------------------------------------------------------
POWER = [(128, (1, 2, 63)), (128, (64, 65, 257)), (1024, (1, 2, 63)), (1024, (64, 65, 257))]
POWER_IDS = ["fft%d-T%s" % (f, "_".join(map(str, t))) for f, t in POWER]


def case_power(be, fft_size, lengths):
    sp = [envelopes(fft_size, T, 3 + T) for T in lengths]
    bins = fft_size // 2 + 1
    got_p, got_m = be.power(sp, fft_size, slack=3, column=2)
    worst_p = worst_m = 0.0
    for u, s in enumerate(sp):
        want_p, want_m = rule_power(s, fft_size)
        assert same_bits(got_p[u], want_p), f"utterance {u}: P is not the stated order's"
        assert same_bits(got_m[u:u + 1], [want_m]), f"utterance {u}: the mean is not the stated order's"
        wp, wm = wide_power(s, fft_size)
        bp, bm = (bins + 6) * U53 * wp, (len(s) + bins + 10) * U53 * wm
        worst_p = max(worst_p, float(np.max(np.abs(LD(got_p[u]) - wp) / bp)))
        worst_m = max(worst_m, float(abs(LD(got_m[u]) - wm) / bm))
    print(f"power fft_size={fft_size} T={lengths}: max error / bound: P {worst_p:.4f}, mean {worst_m:.4f}")
    assert worst_p <= 1 and worst_m <= 1
    # dense rows at an even offset, either output alone: the same bits
    dense_p, dense_m = be.power(sp, fft_size)
    assert all(same_bits(a, b) for a, b in zip(dense_p, got_p)) and same_bits(dense_m, got_m), "the strides change the power"
    only_m = be.power(sp, fft_size, slack=1, column=1, want=("mean",))[1]
    only_p = be.power(sp, fft_size, want=("power",))[0]
    assert same_bits(only_m, got_m) and all(same_bits(a, b) for a, b in zip(only_p, got_p)), "the outputs asked for change them"


SELECT_T = [1, 63, 64, 65, 255, 256, 257, 1025, 4097]


def patterns(T, rng):
    yield "all", np.ones(T, dtype=bool)
    yield "none", np.zeros(T, dtype=bool)
    yield "first", np.arange(T) == 0
    yield "last", np.arange(T) == T - 1
    yield "alternating", np.arange(T) % 2 == 1
    yield "random", rng.random(T) < 0.5


def case_select(be, T):
    rng = np.random.default_rng(100 + T)
    names, values = zip(*[(name, np.where(keep, 2.0, 0.5) * rng.uniform(0.9, 1.1, T)) for name, keep in patterns(T, rng)])
    index, count, keep = be.select(list(values), 1.5)
    for u, name in enumerate(names):
        want_i, want_k = rule_select(values[u], 1.5)
        assert np.array_equal(index[u], want_i) and count[u] == len(want_i) and np.array_equal(keep[u], want_k), f"T={T}, {name}"
    # the mask is ANDed; a column of a record; a scale per utterance; any one output alone
    masks = [rng.random(T) < 0.7 for _ in values]
    scale = rng.uniform(0.5, 2.0, len(values))
    index, count, keep = be.select(list(values), 1.2, scale=scale, masks=masks, stride=3)
    for u in range(len(values)):
        want_i, want_k = rule_select(values[u], 1.2, scale[u], masks[u])
        assert np.array_equal(index[u], want_i) and count[u] == len(want_i) and np.array_equal(keep[u], want_k), f"T={T}, masked {names[u]}"
    for one in ("index", "count", "keep"):
        i1, c1, k1 = be.select(list(values), 1.2, scale=scale, masks=masks, stride=2, want=(one,))
        if one == "index":
            assert all(np.array_equal(a, b) for a, b in zip(i1, index))
        if one == "count":
            assert np.array_equal(c1, count)
        if one == "keep":
            assert all(np.array_equal(a, b) for a, b in zip(k1, keep))


def case_select_edges(be):
    threshold, scale = 0.1, np.array([3.0, 7.0, 1.0 / 3.0])
    limit = np.float64(threshold) * scale                               # rounded once
    values = [np.array([lim, np.nextafter(lim, -np.inf), np.nextafter(lim, np.inf), np.nan, np.inf, -np.inf, -lim]) for lim in limit]
    index, count, keep = be.select(values, threshold, scale=scale)
    for u in range(3):
        assert np.array_equal(index[u], [0, 2, 4]) and count[u] == 3 and np.array_equal(keep[u], [1, 0, 1, 0, 1, 0, 0]), (u, index[u])
    # a NaN scale keeps nothing in its utterance and leaves the others alone; a NaN threshold keeps nothing anywhere
    index, count, keep = be.select(values, threshold, scale=np.array([3.0, np.nan, 1.0 / 3.0]))
    assert np.array_equal(count, [3, 0, 3]) and not keep[1].any() and np.array_equal(index[2], [0, 2, 4])
    index, count, keep = be.select(values, np.nan)
    assert np.array_equal(count, [0, 0, 0]) and not any(k.any() for k in keep)
    # three utterances of different lengths in one call (the sentinels beyond count[u] and n_frames[u] are select()'s checks)
    rng = np.random.default_rng(5)
    values = [rng.standard_normal(T) for T in (4097, 1, 300)]
    index, count, keep = be.select(values, 0.25)
    for u, v in enumerate(values):
        want_i, want_k = rule_select(v, 0.25)
        assert np.array_equal(index[u], want_i) and count[u] == len(want_i) and np.array_equal(keep[u], want_k)


GATHER_DIMS = [1, 2, 3, 25, 60, 201]


def case_gather(be, D):
    rng = np.random.default_rng(200 + D)
    x = [rows_of(T, D, 7 * T + D) for T in (70, 1, 33)]
    index = [rng.integers(0, len(v), size=k).astype(np.int32) for v, k in zip(x, (130, 5, 1))]
    index[0][[3, 64, 129]] = [-1, len(x[0]), INT_MAX]                   # rows of `fill` between intact neighbours
    index[2][0] = -INT_MAX - 1
    fill = -123.5
    want = [rule_gather(v, i, len(v), fill) for v, i in zip(x, index)]
    for column, out_column in ((0, 0), (1, 0), (2, 1), (3, 1), (1, 1)):    # odd: 8-byte aligned only
        got = be.gather(x, index, fill=fill, column=column, slack=2 + (D % 2), out_column=out_column, out_slack=1)
        assert all(same_bits(g, w) for g, w in zip(got, want)), f"D={D}, source column {column}, output column {out_column}"
    # n_src below the rows the array has: the rows beyond count as out of range
    got = be.gather(x, index, fill=fill, n_src=[40, 1, 20])
    assert all(same_bits(g, rule_gather(v, i, n, fill)) for g, v, i, n in zip(got, x, index, (40, 1, 20)))


def random_path(na, nb, rng):
    cells, i, j = [(0, 0)], 0, 0
    while (i, j) != (na - 1, nb - 1):
        step = rng.integers(0, 3)
        i, j = min(i + (step != 2), na - 1), min(j + (step != 1), nb - 1)
        cells.append((i, j))
    return np.array(cells, dtype=np.int32)


def case_joint(be, D):
    rng = np.random.default_rng(300 + D)
    Db = max(1, D - 1)
    full_a = [rows_of(T, D, 11 * T + D) for T in (50, 9)]
    full_b = [rows_of(T, Db, 13 * T + D) for T in (41, 12)]
    fill = 7.25
    # without selections: the path's indices are the rows
    paths = [random_path(len(a), len(b), rng) for a, b in zip(full_a, full_b)]
    paths[0][[5, 6]] = [[-1, 3], [2, len(full_b[0])]]                  # one half each out of range
    want = np.vstack([rule_joint(a, b, p, None, None, fill) for a, b, p in zip(full_a, full_b, paths)])
    for column in (0, 1, 2, 3):
        got = be.joint(full_a, full_b, paths, fill=fill, column=column, slack=1 + column, z_slack=column % 2)
        assert same_bits(got, want), f"D={D}, column {column}"
    # with selections on both sides, on one side, and with entries that point nowhere
    sel_a = [np.sort(rng.choice(len(a), size=max(1, len(a) // 2), replace=False)).astype(np.int32) for a in full_a]
    sel_b = [np.sort(rng.choice(len(b), size=max(1, 2 * len(b) // 3), replace=False)).astype(np.int32) for b in full_b]
    paths = [random_path(len(sa), len(sb), rng) for sa, sb in zip(sel_a, sel_b)]
    paths[1][1] = [len(sel_a[1]), INT_MAX]                              # beyond the selections' lengths
    sel_a[0][2], sel_b[0][1] = len(full_a[0]), -1                       # selected frames that do not exist
    for sa, sb in ((sel_a, sel_b), (sel_a, None), (None, sel_b)):
        ps = [random_path(len(a) if sa is None else len(sa[u]), len(b) if sb is None else len(sb[u]), rng) for u, (a, b) in enumerate(zip(full_a, full_b))] \
            if sa is None or sb is None else paths
        want = np.vstack([rule_joint(a, b, p, None if sa is None else sa[u], None if sb is None else sb[u], fill)
                          for u, (a, b, p) in enumerate(zip(full_a, full_b, ps))])
        got = be.joint(full_a, full_b, ps, sel_a=sa, sel_b=sb, fill=fill, column=1, slack=2, z_slack=1)
        assert same_bits(got, want), f"D={D}, selections {sa is not None} / {sb is not None}"
    # dim_b = 0
    ps = [random_path(len(a), len(a), rng) for a in full_a]
    want = np.vstack([rule_joint(a, None, p, None, None, fill) for a, p in zip(full_a, ps)])
    assert same_bits(be.joint(full_a, None, ps, fill=fill, column=3, slack=1), want), f"D={D}, dim_b = 0"


def gated_corpus(fft_size=128, lengths=((65, 70), (130, 1 + 63), (64, 257)), D=5, seed=17):
    """pairs of utterances: envelope rows whose loudness falls to silence at both ends and once inside, and features"""
    rng = np.random.default_rng(seed)
    pairs = []
    for u, (na, nb) in enumerate(lengths):
        sides = []
        for s, n in enumerate((na, nb)):
            loud = np.ones(n)
            loud[:n // 8] = loud[n - n // 6:] = 1e-7
            loud[n // 2:n // 2 + n // 10] = 1e-7
            sp = envelopes(fft_size, n, 31 * u + s) * loud[:, None]
            c = np.cumsum(rng.standard_normal((n, D)), axis=0) * 0.1 + np.log(loud)[:, None] * np.arange(D) * 0.01
            sides.append((sp, c, np.hstack([c, np.gradient(c, axis=0)])))
        pairs.append(sides)
    return pairs


def case_composition(be, fft_size=128):
    """gate -> gather -> align on the gathered rows -> joint rows with the selections, against NumPy on the same steps (the
    path is the library's own alignment of the NumPy-gathered rows)"""
    pairs = gated_corpus(fft_size)
    gate = 10.0 ** (-20.0 / 10.0)
    got_sel, got_feat, want_sel, want_feat = [], [], [], []
    for s in (0, 1):
        sp, c = [p[s][0] for p in pairs], [p[s][1] for p in pairs]
        power, mean = be.power(sp, fft_size, slack=1, column=2)
        index, count, keep = be.select(power, gate, scale=mean)
        got_sel.append(index)
        got_feat.append(be.gather([x[:, 1:] for x in c], index, column=3, slack=1))
        ws = []
        for u, e in enumerate(sp):
            P, m = rule_power(e, fft_size)
            ws.append(rule_select(P, gate, m)[0])
            assert 0 < len(ws[u]) < len(e), "the gate keeps everything or nothing: the case checks nothing"
            assert np.array_equal(index[u], ws[u]) and count[u] == len(ws[u])
        want_sel.append(ws)
        want_feat.append([x[w, 1:] for x, w in zip(c, ws)])
        assert all(same_bits(g, w) for g, w in zip(got_feat[s], want_feat[s]))
    paths = be.align(want_feat[0], want_feat[1])
    assert all(np.array_equal(a, b) for a, b in zip(be.align(got_feat[0], got_feat[1]), paths))
    dyn_a, dyn_b = [p[0][2] for p in pairs], [p[1][2] for p in pairs]
    z = be.joint(dyn_a, dyn_b, paths, sel_a=got_sel[0], sel_b=got_sel[1], column=1, slack=1)
    want = np.vstack([np.hstack([a[sa[p[:, 0]]], b[sb[p[:, 1]]]]) for a, b, p, sa, sb in zip(dyn_a, dyn_b, paths, want_sel[0], want_sel[1])])
    assert same_bits(z, want)
    silent = [np.setdiff1d(np.arange(len(p[0][0])), w) for p, w in zip(pairs, want_sel[0])]
    assert all(not np.isin(sa[p[:, 0]], q).any() for p, sa, q in zip(paths, want_sel[0], silent)), "a gated frame is in a joint row"
    return z


def case_determinism(be):
    """an utterance's outputs alone, in a batch of seven and at another position of it: the same bits"""
    fft_size = 128
    sp = [envelopes(fft_size, T, 50 + T) for T in (65, 3, 257, 64, 1, 130, 66)]
    whole_p, whole_m = be.power(sp, fft_size, slack=1)
    rng = np.random.default_rng(9)
    x = [rows_of(len(s), 7, len(s)) for s in sp]
    idx = [rng.integers(0, len(s), size=len(s) + 3).astype(np.int32) for s in sp]
    whole_i, whole_c, whole_k = be.select(whole_p, 0.8, scale=whole_m)
    whole_g = be.gather(x, idx, column=1)
    for order in ([2], [5, 2, 0], list(range(6, -1, -1))):
        at = order.index(2)
        p, m = be.power([sp[u] for u in order], fft_size, column=2)
        assert same_bits(p[at], whole_p[2]) and same_bits(m[at:at + 1], whole_m[2:3]), f"power in the batch {order}"
        i, c, k = be.select([whole_p[u] for u in order], 0.8, scale=whole_m[order], stride=2)
        assert np.array_equal(i[at], whole_i[2]) and c[at] == whole_c[2] and np.array_equal(k[at], whole_k[2]), f"selection in the batch {order}"
        g = be.gather([x[u] for u in order], [idx[u] for u in order], column=3, slack=2)
        assert same_bits(g[at], whole_g[2]), f"gather in the batch {order}"
    paths = [random_path(len(a), len(a), rng) for a in x]
    whole_z = be.joint(x, x, paths)
    first = int(sum(len(p) for p in paths[:2]))
    for order in ([2], [5, 2, 0]):
        at = order.index(2)
        z = be.joint([x[u] for u in order], [x[u] for u in order], [paths[u] for u in order], column=1, slack=1)
        skip = int(sum(len(paths[u]) for u in order[:at]))
        assert same_bits(z[skip:skip + len(paths[2])], whole_z[first:first + len(paths[2])]), f"joint rows in the batch {order}"
    with be.fresh() as b2:
        assert all(same_bits(a, b) for a, b in zip(b2.power(sp, fft_size)[0], whole_p)), "a second context differs"


def case_workspace(be):
    """only a mean without d_power takes workspace, and a repeat of the shape takes no more"""
    sp = [envelopes(128, T, 70 + T) for T in (300, 17)]
    with be.fresh() as b:
        w0 = b.workspace()
        both = b.power(sp, 128)
        b.select(both[0], 1.0, scale=both[1])
        b.gather([s[:, :9] for s in sp], [np.arange(0, len(s), 2, dtype=np.int32) for s in sp])
        assert b.workspace() == w0, "a call that needs no workspace took some"
        mean = b.power(sp, 128, want=("mean",))[1]
        w1 = b.workspace()
        assert w1 - w0 >= 8 * 2 * 300 and same_bits(mean, both[1])
        b.power(sp, 128, want=("mean",))
        assert b.workspace() == w1, "the workspace grew on a repeat of the shape"


def case_refusals(be):
    """every refusal of the header's list: 1, a reason, nothing written"""
    U, T, D, fft_size = 2, 5, 3, 128
    bins = fft_size // 2 + 1
    n = np.array([T, T - 1], dtype=np.int32)
    d_in = be.dev(np.ones((U, T, bins + 2)))
    d_scale, d_mask = be.dev(np.ones(U)), be.dev(np.ones((U, T), dtype=np.uint8))
    d_idx = be.dev(np.zeros((U, T), dtype=np.int32))
    d_path = be.dev(np.zeros((U, 2 * T, 2), dtype=np.int32))
    outs = {}

    def fresh_outputs():
        outs.clear()
        outs.update(f64=be.dev(np.full((U, 2 * T, 2 * D + 2), SENTINEL)), f64b=be.dev(np.full(U * T + 1, SENTINEL)),
                    i32=be.dev(np.full((U, T), ISENT, dtype=np.int32)), i32b=be.dev(np.full(U + 1, ISENT, dtype=np.int32)),
                    u8=be.dev(np.full((U, T), BSENT, dtype=np.uint8)))

    def untouched():
        return all(np.all(be.host(outs[k]) == v) for k, v in (("f64", SENTINEL), ("f64b", SENTINEL), ("i32", ISENT), ("i32b", ISENT), ("u8", BSENT)))

    def refused(call, base, reason, **change):
        fresh_outputs()
        a = base()
        for k, v in change.items():
            a[k] = v(a) if callable(v) else v
        rc = call(**a)
        assert rc == 1, f"{reason}: accepted"
        assert be.error(), reason
        assert untouched(), f"{reason}: an output was written"

    # power
    base = lambda: dict(n_utt=U, fft_size=fft_size, n_frames=n, sp=be.addr(d_in), sp_us=T * (bins + 2), sp_rs=bins + 2,
                        power=be.addr(outs["f64b"]), power_us=T, mean=be.addr(outs["f64"]))
    for reason, change in (("n_utt = 0", dict(n_utt=0)), ("NULL n_frames", dict(n_frames=None)), ("NULL d_sp", dict(sp=None)),
                           ("a count of 0", dict(n_frames=[T, 0])), ("fft_size 64", dict(fft_size=64)), ("fft_size 192", dict(fft_size=192)),
                           ("fft_size 16384", dict(fft_size=16384)), ("a row stride below the row", dict(sp_rs=bins - 1)),
                           ("a negative utterance stride", dict(sp_us=-1)), ("a negative power stride", dict(power_us=-1)),
                           ("utterances of the power run into each other", dict(power_us=T - 1)),
                           ("the power is the input", dict(power=lambda a: a["sp"])), ("the mean lies in the power", dict(mean=lambda a: a["power"] + 8))):
        refused(be.call_power, base, "power: " + reason, **change)
    # selection
    base = lambda: dict(n_utt=U, n_frames=n, value=be.addr(d_in), value_us=T * (bins + 2), value_s=bins + 2, threshold=0.5,
                        scale=be.addr(d_scale), mask=be.addr(d_mask), mask_us=T, index=be.addr(outs["i32"]), index_us=T,
                        count=be.addr(outs["i32b"]), keep=be.addr(outs["u8"]), keep_us=T)
    for reason, change in (("n_utt = 0", dict(n_utt=0)), ("NULL n_frames", dict(n_frames=None)), ("NULL d_value", dict(value=None)),
                           ("a count of 0", dict(n_frames=[0, T])), ("value_stride 0", dict(value_s=0)), ("a negative value stride", dict(value_us=-1)),
                           ("a negative mask stride", dict(mask_us=-1)), ("a negative index stride", dict(index_us=-1)),
                           ("a negative keep stride", dict(keep_us=-1)), ("utterances of the index run into each other", dict(index_us=T - 1)),
                           ("utterances of keep run into each other", dict(keep_us=T - 1)),
                           ("the count lies in the index", dict(count=lambda a: a["index"] + 4)), ("keep is the mask", dict(keep=lambda a: a["mask"])),
                           ("the index is the values", dict(index=lambda a: a["value"]))):
        refused(be.call_select, base, "selection: " + reason, **change)
    # gather
    base = lambda: dict(n_utt=U, dim=D, n_src=n, x=be.addr(d_in), x_us=T * (bins + 2), x_rs=bins + 2, n_out=n, index=be.addr(d_idx),
                        index_us=T, fill=0.0, out=be.addr(outs["f64"]), out_us=T * (2 * D + 2), out_rs=2 * D + 2)
    for reason, change in (("n_utt = 0", dict(n_utt=0)), ("dim = 0", dict(dim=0)), ("dim above INT_MAX / 8", dict(dim=INT_MAX // 8 + 1)),
                           ("NULL n_src", dict(n_src=None)), ("NULL n_out", dict(n_out=None)), ("NULL d_in", dict(x=None)),
                           ("NULL d_index", dict(index=None)), ("NULL d_out", dict(out=None)), ("n_src of 0", dict(n_src=[T, 0])),
                           ("n_out of 0", dict(n_out=[0, T])), ("a source row stride below the row", dict(x_rs=D - 1)),
                           ("an output row stride below the row", dict(out_rs=D - 1)), ("a negative source stride", dict(x_us=-1)),
                           ("a negative output stride", dict(out_us=-1)), ("a negative index stride", dict(index_us=-1)),
                           ("utterances of the index run into each other", dict(index_us=T - 1)),
                           ("utterances of the output run into each other", dict(out_us=(T - 1) * (2 * D + 2))),
                           ("the output is the input", dict(out=lambda a: a["x"])), ("the output is the index", dict(out=lambda a: a["index"]))):
        refused(be.call_gather, base, "gather: " + reason, **change)
    # joint rows
    rows = [0, T]
    base = lambda: dict(n_pairs=U, dim_a=D, dim_b=D, a=be.addr(d_in), a_row=rows, n_a=n, a_rs=bins + 2, b=be.addr(d_in) + 8 * D, b_row=rows,
                        n_b=n, b_rs=bins + 2, path_len=[2 * T - 1, T], path=be.addr(d_path), p_stride=2 * T, sel_a=be.addr(d_idx), n_sel_a=n,
                        sel_a_us=T, sel_b=None, n_sel_b=None, sel_b_us=0, fill=0.0, z=be.addr(outs["f64"]), z_row=[0, 2 * T - 1], z_rs=2 * D + 2)
    for reason, change in (("n_pairs = 0", dict(n_pairs=0)), ("dim_a = 0", dict(dim_a=0)), ("dim_b = -1", dict(dim_b=-1)),
                           ("dim_a + dim_b above INT_MAX / 8", dict(dim_a=INT_MAX // 16 + 1, dim_b=INT_MAX // 16 + 1)),
                           ("NULL d_a", dict(a=None)), ("NULL d_b with dim_b > 0", dict(b=None)), ("NULL a_row", dict(a_row=None)),
                           ("NULL b_row", dict(b_row=None)), ("NULL n_a", dict(n_a=None)), ("NULL n_b", dict(n_b=None)),
                           ("NULL path_len", dict(path_len=None)), ("NULL d_path", dict(path=None)), ("NULL z_row", dict(z_row=None)),
                           ("NULL d_z", dict(z=None)), ("a selection without its lengths", dict(n_sel_a=None)),
                           ("n_a of 0", dict(n_a=[0, T])), ("n_b of 0", dict(n_b=[T, 0])), ("a path length of 0", dict(path_len=[0, T])),
                           ("a selection of 0 entries", dict(n_sel_a=[T, 0])), ("a path length above p_stride", dict(path_len=[2 * T + 1, T])),
                           ("a's row stride below the row", dict(a_rs=D - 1)), ("b's row stride below the row", dict(b_rs=D - 1)),
                           ("z's row stride below the row", dict(z_rs=2 * D - 1)), ("a negative first row of a", dict(a_row=[0, -1])),
                           ("a negative first row of b", dict(b_row=[-1, 0])), ("a negative first row of z", dict(z_row=[-1, 2 * T])),
                           ("a negative selection stride", dict(sel_a_us=-1)), ("selections that run into each other", dict(sel_a_us=T - 1)),
                           ("pairs of z that run into each other", dict(z_row=[0, 2 * T - 2])),
                           ("pairs of z that run into each other, the later pair first", dict(z_row=[T - 1, 0])),
                           ("z is an input", dict(z=lambda a: a["a"])), ("z is the path", dict(z=lambda a: a["path"]))):
        refused(be.call_joint, base, "joint rows: " + reason, **change)
    # the accepted form of each base, and a context that is NULL
    fresh_outputs()
    assert be.call_joint(**base()) == 0, be.error()
    assert be.lib.world_hip_frame_power_batch(None, 1, 128, None, None, 0, 0, None, 0, None) == 2


# ---- tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft_size,lengths", POWER, ids=POWER_IDS)
def test_power_is_the_stated_order_and_within_the_summation_bound(be, fft_size, lengths):
    case_power(be, fft_size, lengths)


@pytest.mark.parametrize("T", SELECT_T)
def test_selection_equals_flatnonzero(be, T):
    case_select(be, T)


def test_selection_at_the_threshold_nan_and_ragged_batches(be):
    case_select_edges(be)


@pytest.mark.parametrize("D", GATHER_DIMS)
def test_gather_copies_bits_from_any_alignment(be, D):
    case_gather(be, D)


@pytest.mark.parametrize("D", GATHER_DIMS)
def test_joint_rows_follow_the_path_and_the_selections(be, D):
    case_joint(be, D)


def test_gate_gather_align_joint_is_the_numpy_composition(be):
    case_composition(be)


def test_an_utterance_depends_on_nothing_but_itself(be):
    case_determinism(be)


def test_only_a_mean_without_power_takes_workspace(be):
    case_workspace(be)


def test_refusals_write_nothing_and_give_a_reason(be):
    case_refusals(be)
