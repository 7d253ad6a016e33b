"""Dynamic features and maximum-likelihood parameter generation (include/world_hip.h: world_hip_delta_batch /
world_hip_mlpg_batch) through the host-compiled kernels (tests/emu/libworld_emu.so) and the host refusals.  The reference has
no such function: THE HEADER'S STATEMENT IS THE ORACLE, written out here a second time in numpy and mpmath.  The cases are
functions of a backend, so that tests/test_mlpg_gpu.py runs the same ones through the shipped library.

Bounds (the statement's; none comes from the code under test).
  deltas      |o - exact| <= (2 L + 1) 2^-53 sum |win| |c| per element (a sum of at most 2 L + 1 rounded products), and the
              bits of the statement's own arithmetic in float64 -- products and sums rounded one by one in ascending tau --
              which is what makes the GPU and the emulation agree bit for bit: both are held to the same numpy restatement.
  generation  R = W' P W and r = W' P mu are formed exactly (mpmath, 200 bits) per (u, d) system; the component-wise backward
              error omega = max_i |r - R c|_i / (|R| |c| + |r|)_i of the library's c must be at most 16 * 2^-53.  A plain
              float64 banded L D L' reaches 3.2 * 2^-53 at these shapes and spreads (T = 67, five taps); the factor 5 is
              for another summation order and FMA contraction.  No forward error is tested: at a spread of 10^+-6 the
              systems are so ill-conditioned that numpy.linalg.solve is off by 1e4 .. 1e5 ulp.
  round trip  mlpg(deltas(c)) = c whatever the variances (the observations are consistent): the error may be 8 times that
              of scipy.linalg.solveh_banded on the same systems.
  Measured in the host emulation: omega <= 2.63 * 2^-53 over the accuracy cases below; round trip 8.9e-16 (8 * 2^-53)
  against scipy's 1.8e-15 (16 * 2^-53).
"""
import ctypes as C

import numpy as np
import pytest

import backends
from backends import SENTINEL_F64 as SENTINEL, cpu_backend, lib, same_bits  # noqa: F401 (lib: a fixture)

LD = np.longdouble
U53 = 2.0 ** -53
FILL = -1e10
OMEGA_MAX = 16 * U53

W1 = np.array([[1.0]])
W3 = np.array([[0.0, 1.0, 0.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]])
W5 = np.array([[0.0, 0.0, 1.0, 0.0, 0.0], [-0.2, -0.1, 0.0, 0.1, 0.2], [0.285714, -0.142857, -0.285714, -0.142857, 0.285714]])
WINDOWS = {"static": W1, "three": W3, "five": W5}


# ---- the statement --------------------------------------------------------------------------------------------------------
def counts(present, t, tau):
    """does the term (t, tau) count: every frame from t to t + tau inside the utterance and present"""
    lo, hi = min(t, t + tau), max(t, t + tau)
    return lo >= 0 and hi < len(present) and bool(np.all(present[lo:hi + 1]))


def rule_deltas(c, win, present, fill):
    """(the statement's float64 arithmetic, the exact value in long double, the bound's sum |win| |c|), each [T][n_win D]"""
    T, D = c.shape
    n_win, L = win.shape[0], win.shape[1] // 2
    f64 = np.full((T, n_win * D), fill)
    ld = np.full((T, n_win * D), fill, dtype=LD)
    mag = np.zeros((T, n_win * D))
    for t in range(T):
        if not present[t]:
            continue
        for w in range(n_win):
            acc, exact, m = np.zeros(D), np.zeros(D, dtype=LD), np.zeros(D)
            for tau in range(-L, L + 1):
                if counts(present, t, tau):
                    acc = acc + win[w, tau + L] * c[t + tau]
                    exact = exact + LD(win[w, tau + L]) * LD(c[t + tau])
                    m = m + abs(win[w, tau + L]) * np.abs(c[t + tau])
            f64[t, w * D:(w + 1) * D], ld[t, w * D:(w + 1) * D], mag[t, w * D:(w + 1) * D] = acc, exact, m
    return f64, ld, mag


def omega_of(chat, mu, pv, precision, win, present):
    """the component-wise backward error of chat [T] for the system of one (u, d): mu, pv [T][n_win]; R and r exact"""
    import mpmath
    mpmath.mp.prec = 200
    mpf = mpmath.mpf
    T = len(chat)
    n_win, L = win.shape[0], win.shape[1] // 2
    R, r = {}, [mpf(0)] * T
    for t in range(T):
        if not present[t]:
            continue
        for w in range(n_win):
            p = mpf(float(pv[t, w])) if precision else 1 / mpf(float(pv[t, w]))
            terms = [(t + tau, mpf(float(win[w, tau + L]))) for tau in range(-L, L + 1)
                     if win[w, tau + L] != 0 and counts(present, t, tau)]
            pm = p * mpf(float(mu[t, w]))
            for i, a in terms:
                r[i] += a * pm
                for j, b in terms:
                    R[i, j] = R.get((i, j), 0) + p * a * b
    res, den = list(r), [abs(x) for x in r]
    for (i, j), v in R.items():
        cj = mpf(float(chat[j]))
        res[i] -= v * cj
        den[i] += abs(v) * abs(cj)
    return max(float(abs(res[i]) / den[i]) for i in range(T) if present[i])


def runs_of(present):
    """[(first, past the last)] of every maximal run of present frames"""
    out, t, T = [], 0, len(present)
    while t < T:
        if present[t]:
            e = t
            while e < T and present[e]:
                e += 1
            out.append((t, e))
            t = e
        else:
            t += 1
    return out


# ---- a backend: the C calls on arrays that live where the library wants them ---------------------------------------------
class Backend(backends.Backend):
    """world_hip_delta_batch / _mlpg_batch on the arrays of backends.Backend"""

    def workspace(self):
        return int(self.lib.world_hip_workspace_bytes(self.ctx))

    @staticmethod
    def _p(a):
        return None if a is None else C.c_void_p(a)

    @staticmethod
    def _ints(a):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))

    def call_delta(self, n_utt, dim, win, n_frames, mask, mask_us, c, c_us, c_rs, fill, out, out_us, out_rs, n_win=None, half=None):
        """the C call itself on addresses (None: NULL); win: float64 [n_win][2 L + 1] or None"""
        win = None if win is None else np.ascontiguousarray(win, dtype=np.float64)
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        return self.lib.world_hip_delta_batch(
            self.ctx, n_utt, dim, win.shape[0] if n_win is None else n_win, win.shape[1] // 2 if half is None else half,
            None if win is None else win.ctypes.data, self._ints(nf), self._p(mask), mask_us, self._p(c), c_us, c_rs, fill, self._p(out),
            out_us, out_rs)

    def call_mlpg(self, n_utt, dim, win, n_frames, mask, mask_us, mean, mean_us, mean_rs, var, var_us, var_rs, precision, fill,
                  out, out_us, out_rs, n_win=None, half=None):
        win = None if win is None else np.ascontiguousarray(win, dtype=np.float64)
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        return self.lib.world_hip_mlpg_batch(
            self.ctx, n_utt, dim, win.shape[0] if n_win is None else n_win, win.shape[1] // 2 if half is None else half,
            None if win is None else win.ctypes.data, self._ints(nf), self._p(mask), mask_us, self._p(mean), mean_us, mean_rs, self._p(var),
            var_us, var_rs, int(precision), fill, self._p(out), out_us, out_rs)

    @staticmethod
    def _rows(xs, cols, slack, extra):
        """the utterances xs ([T_u][cols] each) in one [U][max T + extra][cols + slack] array full of SENTINEL"""
        tm = max(len(x) for x in xs) + extra
        a = np.full((len(xs), tm, cols + slack), SENTINEL)
        for u, x in enumerate(xs):
            a[u, :len(x), :cols] = x
        return a

    @staticmethod
    def _mask(masks, n, tm):
        """[U][tm] bytes: the masks, and 1 (present) beyond n_frames -- the library must go by n_frames there"""
        if masks is None:
            return None
        m = np.ones((n, tm), dtype=np.uint8)
        for u, k in enumerate(masks):
            m[u, :len(k)] = np.asarray(k, dtype=np.uint8) * 3           # (any non-zero byte means present)
        return m

    def _finish(self, rc, d_out, host_out, lens, cols, inputs):
        assert rc == 0, self.error()
        out = self.host(d_out)
        for u, n in enumerate(lens):
            assert np.all(out[u, :n, cols:] == SENTINEL), "written beyond the row"
            assert np.all(out[u, n:] == SENTINEL), "written beyond n_frames"
        for d, h in inputs:
            assert same_bits(self.host(d).astype(np.float64), np.asarray(h, dtype=np.float64)), "an input changed"
        return [np.array(out[u, :n, :cols]) for u, n in enumerate(lens)]

    def deltas(self, cs, win, masks=None, fill=FILL, slack=0):
        """cs: the utterances' statics [T_u][D] -> their [T_u][n_win D].  slack > 0: rows lie further apart and the
        arrays have rows beyond n_frames, all SENTINEL, and what the call should not have written is checked to be there"""
        lens, D, n_win = [len(c) for c in cs], cs[0].shape[1], win.shape[0]
        extra = 2 if slack else 0
        xin, out = self._rows(cs, D, slack, extra), self._rows([np.full((n, n_win * D), SENTINEL) for n in lens], n_win * D, slack, extra)
        m = self._mask(masks, len(cs), xin.shape[1])
        d_in, d_out, d_m = self.dev(xin), self.dev(out), None if m is None else self.dev(m)
        rc = self.call_delta(len(cs), D, win, lens, None if m is None else self.addr(d_m), 0 if m is None else m.shape[1],
                             self.addr(d_in), xin.shape[1] * xin.shape[2], xin.shape[2], fill, self.addr(d_out),
                             out.shape[1] * out.shape[2], out.shape[2])
        return self._finish(rc, d_out, out, lens, n_win * D, [(d_in, xin)] + ([] if m is None else [(d_m, m)]))

    def mlpg(self, means, var, win, masks=None, precision=False, fill=FILL, slack=0):
        """means: the utterances' [T_u][n_win D]; var: a list of [T_u][n_win D] (per frame), a list of [n_win D] (one row per
        utterance) or one [n_win D] (global) -> the utterances' [T_u][D]"""
        lens, cols = [len(x) for x in means], means[0].shape[1]
        D = cols // win.shape[0]
        extra = 2 if slack else 0
        xin, out = self._rows(means, cols, slack, extra), self._rows([np.full((n, D), SENTINEL) for n in lens], D, slack, extra)
        if isinstance(var, np.ndarray):
            v, v_us, v_rs = self._rows([var[None]], cols, slack, 0), 0, 0
        elif var[0].ndim == 1:
            v = self._rows([x[None] for x in var], cols, slack, 0)
            v_us, v_rs = v.shape[2], 0
        else:
            v = self._rows(var, cols, slack + 1, extra)                 # (a stride of its own)
            v_us, v_rs = v.shape[1] * v.shape[2], v.shape[2]
        m = self._mask(masks, len(means), xin.shape[1])
        d_in, d_v, d_out, d_m = self.dev(xin), self.dev(v), self.dev(out), None if m is None else self.dev(m)
        rc = self.call_mlpg(len(means), D, win, lens, None if m is None else self.addr(d_m), 0 if m is None else m.shape[1],
                            self.addr(d_in), xin.shape[1] * xin.shape[2], xin.shape[2], self.addr(d_v), v_us, v_rs, precision, fill,
                            self.addr(d_out), out.shape[1] * out.shape[2], out.shape[2])
        return self._finish(rc, d_out, out, lens, D, [(d_in, xin), (d_v, v)] + ([] if m is None else [(d_m, m)]))


be = cpu_backend(Backend)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def spread(rng, s, shape):
    """precisions (or variances) drawn from 10^U(-s, s)"""
    return 10.0 ** rng.uniform(-s, s, shape)


def var_of_kind(rng, kind, s, lens, cols):
    if kind == "frame":
        return [spread(rng, s, (n, cols)) for n in lens]
    if kind == "utt":
        return [spread(rng, s, cols) for _ in lens]
    return spread(rng, s, cols)


def var_rows(var, u, n):
    """the [n][cols] variances utterance u is solved under"""
    if isinstance(var, np.ndarray):
        return np.broadcast_to(var, (n, var.shape[0]))
    return np.broadcast_to(var[u], (n, var[u].shape[-1]))


# (frames per utterance, D, windows, variances, the precision flag, spread s, strided)
ACCURACY = [
    ((67, 5), 3, "five", "frame", True, 6, False),
    ((67, 5), 3, "five", "frame", False, 3, True),
    ((67, 5), 3, "five", "utt", False, 0, True),
    ((67, 5), 3, "three", "frame", False, 6, True),
    ((67, 5), 3, "three", "global", True, 3, False),
    ((67, 5), 3, "three", "frame", True, 0, False),
    ((67, 5), 3, "static", "frame", False, 6, True),
    ((67, 5), 3, "static", "utt", True, 3, False),
    ((67, 5), 3, "static", "global", False, 0, False),
    ((5,), 130, "three", "global", True, 3, False),
    ((3, 2, 5), 65, "five", "frame", False, 6, True),
    ((1, 2, 3), 65, "three", "utt", False, 3, True),
    ((1,), 1, "five", "frame", True, 6, False),
    ((2,), 1, "three", "global", False, 0, True),
    ((3, 1, 2), 3, "static", "frame", True, 6, True),
]
ACCURACY_IDS = ["%s-D%d-%s-%s-%s-s%d-%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3], "prec" if c[4] else "var", c[5],
                                               "strided" if c[6] else "dense") for c in ACCURACY]
DELTAS = [((67, 5), 3, "five", True), ((67,), 65, "three", False), ((3, 1, 2), 130, "five", True), ((1, 2, 5), 3, "three", True),
          ((2,), 1, "static", False), ((5, 3), 65, "static", True)]
DELTA_IDS = ["%s-D%d-%s-%s" % ("x".join(map(str, c[0])), c[1], c[2], "strided" if c[3] else "dense") for c in DELTAS]

MASKS = {
    "all-present": lambda T: np.ones(T, dtype=bool),
    "all-masked": lambda T: np.zeros(T, dtype=bool),
    "first-and-last-masked": lambda T: np.array([0 < t < T - 1 for t in range(T)]),
    "alternating": lambda T: np.arange(T) % 2 == 0,
    "runs-1-2-3": lambda T: np.array(([1, 0, 1, 1, 0, 1, 1, 1, 0] * (T // 9 + 1))[:T], dtype=bool),
}


# ---- the cases ------------------------------------------------------------------------------------------------------------
def case_deltas(be, lens, D, wname, strided):
    rng = np.random.default_rng(11)
    win = WINDOWS[wname]
    L = win.shape[1] // 2
    cs = [rng.standard_normal((n, D)) for n in lens]
    masks = [rng.random(n) < 0.8 for n in lens] if strided else None
    got = be.deltas(cs, win, masks=masks, slack=3 if strided else 0)
    worst = 0.0
    for u, n in enumerate(lens):
        present = masks[u] if masks else np.ones(n, dtype=bool)
        f64, exact, mag = rule_deltas(cs[u], win, present, FILL)
        bound = (2 * L + 1) * U53 * mag
        err = np.abs(LD(got[u]) - exact)
        worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
        assert np.all(err <= bound), "beyond (2 L + 1) 2^-53 sum |win| |c|"
        assert same_bits(got[u], f64), "not the statement's float64 arithmetic"
    print(f"deltas {lens} D={D} {wname}: max error / bound = {worst:.3f}")


def accuracy_inputs(lens, D, wname, kind, s):
    rng = np.random.default_rng(5)
    cols = WINDOWS[wname].shape[0] * D
    means = [rng.standard_normal((n, cols)) for n in lens]
    return means, var_of_kind(rng, kind, s, lens, cols)


def case_accuracy(be, lens, D, wname, kind, precision, s, strided):
    win = WINDOWS[wname]
    n_win = win.shape[0]
    means, var = accuracy_inputs(lens, D, wname, kind, s)
    got = be.mlpg(means, var, win, precision=precision, slack=2 if strided else 0)
    worst = 0.0
    for u, n in enumerate(lens):
        v = var_rows(var, u, n)
        for d in range(D):
            om = omega_of(got[u][:, d], means[u][:, d::D][:, :n_win], v[:, d::D][:, :n_win], precision, win, np.ones(n, dtype=bool))
            worst = max(worst, om)
    print(f"mlpg {lens} D={D} {wname} {kind} s={s}: omega = {worst / U53:.2f} * 2^-53")
    assert worst <= OMEGA_MAX
    return worst


def case_round_trip(be):
    from scipy.linalg import solveh_banded
    rng = np.random.default_rng(3)
    T, D, win = 67, 3, W3
    c = rng.standard_normal((T, D))
    obs = be.deltas([c], win)[0]
    assert same_bits(obs, rule_deltas(c, win, np.ones(T, dtype=bool), FILL)[0])
    prec = spread(rng, 0, (T, 3 * D))
    got = be.mlpg([obs], [prec], win, precision=True)[0]
    W = np.zeros((3, T, T))
    for w in range(3):
        for t in range(T):
            for tau in (-1, 0, 1):
                if 0 <= t + tau < T:
                    W[w, t, t + tau] = win[w, tau + 1]
    ref = np.empty_like(c)
    for d in range(D):
        R = sum(W[w].T @ (prec[:, w * D + d, None] * W[w]) for w in range(3))
        r = sum(W[w].T @ (prec[:, w * D + d] * obs[:, w * D + d]) for w in range(3))
        ab = np.zeros((3, T))
        for k in range(3):
            ab[2 - k, k:] = np.diagonal(R, k)
        ref[:, d] = solveh_banded(ab, r)
    e_lib, e_ref = float(np.max(np.abs(got - c))), float(np.max(np.abs(ref - c)))
    print(f"round trip: library {e_lib:.3e} ({e_lib / U53:.1f} * 2^-53), scipy.linalg.solveh_banded {e_ref:.3e} ({e_ref / U53:.1f} * 2^-53)")
    assert e_lib <= 8 * e_ref


def case_mask(be, pattern, wname):
    rng = np.random.default_rng(17)
    T, D, win = 31, 3, WINDOWS[wname]
    n_win = win.shape[0]
    present = MASKS[pattern](T)
    c = rng.standard_normal((T, D))
    mean, var = rng.standard_normal((T, n_win * D)), spread(rng, 3, (T, n_win * D))
    dl = be.deltas([c], win, masks=[present], slack=1)[0]
    gen = be.mlpg([mean], [var], win, masks=[present], slack=1)[0]
    assert np.all(dl[~present] == FILL) and np.all(gen[~present] == FILL)
    assert not np.any(dl[present] == FILL) and not np.any(gen[present] == FILL)
    for a, b in runs_of(present):
        assert same_bits(dl[a:b], be.deltas([c[a:b]], win)[0]), f"deltas: run [{a}, {b}) is not an utterance of its own"
        assert same_bits(gen[a:b], be.mlpg([mean[a:b]], [var[a:b]], win)[0]), f"mlpg: run [{a}, {b}) is not an utterance of its own"
        om = max(omega_of(gen[a:b, d], mean[a:b, d::D], var[a:b, d::D], False, win, np.ones(b - a, dtype=bool)) for d in range(D))
        assert om <= OMEGA_MAX
    # the masked rows are never read: NaN there changes nothing
    c2, mean2, var2 = c.copy(), mean.copy(), var.copy()
    c2[~present] = mean2[~present] = var2[~present] = np.nan
    assert same_bits(be.deltas([c2], win, masks=[present])[0], dl)
    assert same_bits(be.mlpg([mean2], [var2], win, masks=[present])[0], gen)


def case_independence(be, wname):
    """a column alone, inside a batch, at another d, with other strides, in a second context: the same bits"""
    rng = np.random.default_rng(23)
    win = WINDOWS[wname]
    n_win = win.shape[0]
    T, D = 67, 130
    mean, var = rng.standard_normal((T, n_win * D)), spread(rng, 3, (T, n_win * D))
    present = rng.random(T) < 0.9
    col = lambda a, d: np.ascontiguousarray(a[:, d::D][:, :n_win])                     # the D = 1 problem of column d
    whole = be.mlpg([mean], [var], win, masks=[present])[0]
    for d in (0, 63, 64, 129):
        alone = be.mlpg([col(mean, d)], [col(var, d)], win, masks=[present])[0]
        assert same_bits(alone[:, 0], whole[:, d]), f"column {d} of {D} differs from the column alone"
    other = [rng.standard_normal((5, n_win * D)), rng.standard_normal((40, n_win * D))]
    batch = be.mlpg([other[0], mean, other[1]], [spread(rng, 3, (5, n_win * D)), var, spread(rng, 3, (40, n_win * D))], win,
                    masks=[np.ones(5, dtype=bool), present, np.ones(40, dtype=bool)], slack=5)
    assert same_bits(batch[1], whole), "the batch or the strides change a column"
    with be.fresh() as b2:
        assert same_bits(b2.mlpg([mean], [var], win, masks=[present])[0], whole), "a second context differs"
    c = rng.standard_normal((T, D))
    dl = be.deltas([c], win, masks=[present])[0]
    assert same_bits(be.deltas([other[0][:, :D], c], win, masks=[np.ones(5, dtype=bool), present], slack=2)[1], dl)
    assert same_bits(be.deltas([c[:, 64:65]], win, masks=[present])[0], dl[:, 64::D])
    return mean, var, present, whole


def case_poison(be, wname):
    """a variance that is not finite and positive spoils its own column only, and the next call is a fresh one"""
    rng = np.random.default_rng(29)
    win = WINDOWS[wname]
    n_win = win.shape[0]
    T, D = 13, 65
    mean, var = rng.standard_normal((T, n_win * D)), spread(rng, 0, (T, n_win * D))
    clean = be.mlpg([mean], [var], win)[0]
    bad = {3: 0.0, 17: -1.0, 40: np.nan, 64: np.inf}
    for flag in (False, True):
        clean_f = be.mlpg([mean], [var], win, precision=flag)[0]
        v = var.copy()
        for k, (d, x) in enumerate(bad.items()):
            v[5, (k % n_win) * D + d] = x
        got = be.mlpg([mean], [v], win, precision=flag)[0]
        keep = np.array([d not in bad for d in range(D)])
        assert same_bits(got[:, keep], clean_f[:, keep]), "a poisoned column changed another one"
        assert same_bits(be.mlpg([mean], [var], win, precision=flag)[0], clean_f), "the call after a poisoned one differs"
    assert same_bits(be.mlpg([mean], [var], win)[0], clean)


def case_refusals(be):
    T, D, win = 5, 3, W3
    cols = 3 * D
    mean, var = np.ones((1, T + 1, cols + 2)), np.ones((1, T + 1, cols + 2))
    out_g, out_d = np.full((1, T + 1, D + 2), SENTINEL), np.full((1, T + 1, cols + 2), SENTINEL)
    stat = np.ones((1, T + 1, D + 2))
    d_mean, d_var, d_stat = be.dev(mean), be.dev(var), be.dev(stat)
    d_mask = be.dev(np.ones((1, T + 1), dtype=np.uint8))
    bad_id = W3.copy(); bad_id[0] = [0.0, 0.5, 0.0]
    off_id = W3.copy(); off_id[0] = [0.5, 1.0, 0.0]
    nan_w = W3.copy(); nan_w[2, 0] = np.nan
    inf_w = W3.copy(); inf_w[1, 2] = np.inf

    def both(change, reason):
        """the same bad argument through both calls: 1 is returned, a reason given, nothing written"""
        for generate in (False, True):
            d_out = be.dev(out_g if generate else out_d)
            a = dict(n_utt=1, dim=D, win=win, n_frames=[T], mask=be.addr(d_mask), mask_us=T + 1, fill=FILL, out=be.addr(d_out),
                     out_us=(T + 1) * ((D if generate else cols) + 2), out_rs=(D if generate else cols) + 2)
            if generate:
                a.update(mean=be.addr(d_mean), mean_us=(T + 1) * (cols + 2), mean_rs=cols + 2, var=be.addr(d_var),
                         var_us=(T + 1) * (cols + 2), var_rs=cols + 2, precision=0)
            else:
                a.update(c=be.addr(d_stat), c_us=(T + 1) * (D + 2), c_rs=D + 2)
            ok = dict(a)
            change(a, generate, d_out)
            if a.keys() == ok.keys() and all(a[k] is ok[k] for k in a):
                continue                                               # (an argument the other call does not have)
            rc = (be.call_mlpg if generate else be.call_delta)(**a)
            assert rc == 1, f"{reason}: accepted by {'mlpg' if generate else 'delta'}"
            assert be.error(), reason
            assert np.all(be.host(d_out) == SENTINEL), f"{reason}: the output was written"

    def setter(**kw):
        return lambda a, generate, d_out: a.update(kw)

    both(setter(n_utt=0), "n_utt < 1")
    both(setter(dim=0), "dim < 1")
    both(setter(n_frames=[0]), "n_frames[u] < 1")
    both(setter(win=None, n_win=3, half=1), "NULL win")
    both(setter(n_frames=None), "NULL n_frames")
    both(setter(out=None), "NULL d_out")
    both(lambda a, g, o: a.update(mean=None) if g else a.update(c=None), "NULL input")
    both(lambda a, g, o: a.update(var=None) if g else None, "NULL d_var")
    both(setter(n_win=0), "n_win = 0")
    both(setter(win=np.vstack([W3, W3[1:]]), n_win=5), "n_win = 5")
    both(setter(half=3, win=np.zeros((3, 7))), "half_width = 3")
    both(setter(half=-1), "half_width = -1")
    both(setter(win=nan_w), "a NaN coefficient")
    both(setter(win=inf_w), "an infinite coefficient")
    both(setter(win=bad_id), "window 0 is 0.5 at tau = 0")
    both(setter(win=off_id), "window 0 is not 0 at tau = -1")
    both(lambda a, g, o: a.update(mean_rs=cols - 1) if g else a.update(c_rs=D - 1), "an input row stride below the row")
    both(lambda a, g, o: a.update(out_rs=(D if g else cols) - 1), "an output row stride below the row")
    both(lambda a, g, o: a.update(var_rs=cols - 1) if g else None, "a variance row stride below the row and not 0")
    both(lambda a, g, o: a.update(out=a["mean"] if g else a["c"]), "the output is the input")
    both(lambda a, g, o: a.update(out=a["var"] + 8 * (cols + 2)) if g else None, "the output lies inside the variances")
    both(lambda a, g, o: a.update(mean=be.addr(o) + 8, mean_rs=cols, mean_us=0) if g else a.update(c=be.addr(o) + 8), "the input overlaps the output")
    # two utterances whose output rows would run into each other
    for generate in (False, True):
        oc = D if generate else cols
        d_out = be.dev(np.full((2, T, oc), SENTINEL))
        d_in = be.dev(np.ones((2, T, cols if generate else D)))
        if generate:
            rc = be.call_mlpg(2, D, win, [T, T], None, 0, be.addr(d_in), T * cols, cols, be.addr(d_var), 0, 0, 0, FILL, be.addr(d_out),
                              (T - 1) * oc, oc)
        else:
            rc = be.call_delta(2, D, win, [T, T], None, 0, be.addr(d_in), T * D, D, FILL, be.addr(d_out), (T - 1) * oc, oc)
        assert rc == 1 and be.error() and np.all(be.host(d_out) == SENTINEL)
    assert be.lib.world_hip_mlpg_batch(None, 1, D, 3, 1, win.ctypes.data, None, None, 0, None, 0, cols, None, 0,
                                       0, 0, FILL, None, 0, D) == 2
    # ... and what is allowed: a variance row stride of 0, with and without an utterance stride
    d_out = be.dev(out_g)
    assert be.call_mlpg(1, D, win, [T], None, 0, be.addr(d_mean), 0, cols + 2, be.addr(d_var), 0, 0, 0, FILL, be.addr(d_out), 0, D + 2) == 0, be.error()
    assert np.all(be.host(d_out)[0, :T, :D] != SENTINEL) and np.all(be.host(d_out)[0, T:] == SENTINEL)


def case_workspace(be):
    """the sweeps keep [max T][2 L + 1][n_utt D] doubles; a repeat of the shape, the static windows and the deltas need none"""
    rng = np.random.default_rng(31)
    with be.fresh() as b:
        lens, D = (300, 20), 130
        w0 = b.workspace()
        c = [rng.standard_normal((n, D)) for n in lens]
        b.deltas(c, W5)
        b.mlpg([rng.standard_normal((n, D)) for n in lens], spread(rng, 0, D), W1)
        assert b.workspace() == w0, "the deltas or the static windows took workspace"
        mean, var = [rng.standard_normal((n, 3 * D)) for n in lens], spread(rng, 0, 3 * D)
        first = b.mlpg(mean, var, W3)
        w1 = b.workspace()
        assert w1 - w0 >= 8 * 300 * 3 * 2 * D, "the workspace did not grow by the factor and the right-hand side"
        assert same_bits(np.vstack(b.mlpg(mean, var, W3)), np.vstack(first))
        assert b.workspace() == w1, "the workspace grew on a repeat of the shape"
        b.mlpg(mean, var, W5[:, :], precision=True)
        w2 = b.workspace()
        assert w2 - w0 >= 8 * 300 * 5 * 2 * D and w2 >= w1


# ---- tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,D,wname,strided", DELTAS, ids=DELTA_IDS)
def test_deltas_are_the_statement(be, lens, D, wname, strided):
    case_deltas(be, lens, D, wname, strided)


@pytest.mark.parametrize("lens,D,wname,kind,precision,s,strided", ACCURACY, ids=ACCURACY_IDS)
def test_generation_backward_error(be, lens, D, wname, kind, precision, s, strided):
    case_accuracy(be, lens, D, wname, kind, precision, s, strided)


def test_generation_inverts_the_deltas(be):
    case_round_trip(be)


@pytest.mark.parametrize("wname", ["three", "five"])
@pytest.mark.parametrize("pattern", list(MASKS))
def test_a_run_of_present_frames_is_an_utterance_of_its_own(be, pattern, wname):
    case_mask(be, pattern, wname)


@pytest.mark.parametrize("wname", ["static", "three", "five"])
def test_a_column_depends_on_nothing_but_the_column(be, wname):
    case_independence(be, wname)


@pytest.mark.parametrize("wname", ["static", "three", "five"])
def test_a_poisoned_column_spoils_nothing_else(be, wname):
    case_poison(be, wname)


def test_refusals_write_nothing_and_give_a_reason(be):
    case_refusals(be)


def test_workspace_grows_once(be):
    case_workspace(be)
