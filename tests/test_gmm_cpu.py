"""Joint-density Gaussian mixture (include/world_hip.h: world_hip_gmm_prepare / _convert / _accumulate / _update / _fit /
_init) through the host-compiled kernels (tests/emu/libworld_emu.so) and the host arithmetic.  The reference has no such
function: THE HEADER'S STATEMENT IS THE ORACLE, written out here a second time in np.longdouble (and, for the prepared model,
in mpmath at 140 bits) on the very doubles world_hip_gmm_model_parts hands back.  The cases are functions of a backend, so
that tests/test_gmm_gpu.py runs the same ones through the shipped library.

Bounds (u = 2^-53; none comes from the code under test; every case prints its largest error / bound).
  prepare     an entry is the exact value's rounding, u |exact|, plus the long-double working error.  Cholesky and the
              triangular inverse in a precision eps have the normwise forward error c n kappa eps to first order (Higham,
              Accuracy and Stability, Th. 10.3 and 8.5); with eps = 2^-64, kappa <= 10^4 and c = 4:
              |got - exact| <= u |exact| + 4 n kappa 2^-64 max |part|, n = Dx + Dy.
  dot         a sum of K rounded products in any order: (K + 4) u sum |terms| (test_mcep_cpu.py's statement).
  z, e        dz_j = (Dx + 4) u sum_k |U_jk| |d_k|;  de_i = (Dx + 4) u (|mu_y| + sum_k |A_ik| |d_k|)_i.
  q           q = c - sum z^2 / 2:  bq = sum_j (|z_j| + dz_j) dz_j + (Dx + 4) u sum z^2 / 2 + 2 u (|c| + |q|).
  loglik      a convex combination of the q's errors to first order, then exp, the sum of M terms in [0, 1], ln, one
              addition:  bl = max_m bq + (M + 8) u (1 + |ln s|) + 2 u |loglik|.
  gamma       d gamma / gamma = dq_m - sum_k gamma_k dq_k to first order, the rounded q_m - q_max, exp, the sum, the
              division:  bg_m = gamma_m (2 max bq + (M + 8 + |q_m - q_max|) u) (+ 1e-300: the subnormals).
  mean        mode 0: sum_m (bg_m |e_m| + gamma_m de_m) + (M + 4) u sum_m gamma_m |e_m|;  mode 1 and M = 1: de.
  var         mode 0: sum_m (bg_m (v + e^2) + 2 gamma_m |e_m| de_m) + (M + 6) u sum_m gamma_m (v + e^2)
              + 2 |mean| bmean + 2 u mean^2;  mode 1: exact (a copy of v).
  statistics  (rows + 4) u sum_t |gamma d_i d_j| (and |gamma d_j|, |gamma|): a dot product of inner length rows.
  fit         the issue's: within 4 x the deviation that the float64 NumPy restatement of the same iterations shows from
              the long-double one (printed beside the library's).
Measured (largest error / bound over the cases below; the host emulation and one MI355X agree to the digits given): prepare
0.03, q 0.12, e 0.33, loglik 0.054, gamma 0.073, mean 0.059, var 0.036, statistics 0.075.  Fit, three iterations, the largest
deviation from the long-double restatement: w 3.1e-16 (NumPy 9.2e-17), mu 2.7e-16 (2.0e-16), cov 1.4e-15 (1.4e-15), loglik
7.4e-16 (8.2e-16); sklearn's own 1.3e-16, 2.7e-15, 1.5e-15.
"""
import ctypes as C

import numpy as np
import pytest

import backends
from backends import SENTINEL_F64 as SENTINEL, cpu_backend, emu, lib, same_bits  # noqa: F401 (emu, lib: fixtures)

LD = np.longdouble
U53 = 2.0 ** -53
MODES = {"mixture": 0, "hard": 1}


# ---- a backend: the C calls on arrays that live where the library wants them ---------------------------------------------
class Backend(backends.Backend):
    """the world_hip_gmm_* calls on the arrays of backends.Backend"""

    def workspace(self):
        return int(self.lib.world_hip_workspace_bytes(self.ctx))

    @staticmethod
    def _h(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    # -- host arithmetic
    def prepare(self, w, mu, cov, dx):
        """-> (rc, the prepared model as host doubles)"""
        w, mu, cov = (np.ascontiguousarray(a, dtype=np.float64) for a in (w, mu, cov))
        M, P = mu.shape
        n = self.lib.world_hip_gmm_model_doubles(M, dx, P - dx)
        assert n > 0, self.error()
        model = np.full(n, SENTINEL)
        rc = self.lib.world_hip_gmm_prepare(M, dx, P - dx, self._h(w), self._h(mu), self._h(cov), self._h(model))
        return rc, model

    def parts(self, M, dx, dy, model):
        out = dict(c=np.empty(M), mux=np.empty((M, dx)), muy=np.empty((M, dy)), U=np.empty((M, dx, dx)), A=np.empty((M, dy, dx)),
                   v=np.empty((M, dy)))
        assert self.lib.world_hip_gmm_model_parts(M, dx, dy, self._h(model), *(self._h(out[k]) for k in ("c", "mux", "muy", "U", "A", "v"))) == 0
        return out

    def update(self, N, S1, G, shift, total, reg):
        """-> (rc, w, mu, cov); the outputs are full of SENTINEL beforehand"""
        M, P = S1.shape
        w, mu, cov = np.full(M, SENTINEL), np.full((M, P), SENTINEL), np.full((M, P, P), SENTINEL)
        rc = self.lib.world_hip_gmm_update(M, P, self._h(N), self._h(S1), self._h(G), self._h(np.ascontiguousarray(shift)), float(total),
                                           float(reg), self._h(w), self._h(mu), self._h(cov))
        return rc, w, mu, cov

    # -- the device calls
    def call_convert(self, M, dx, dy, model, rows, x, x_rs, mode, mean, mean_rs, var, var_rs, post, post_rs, loglik):
        """the C call itself on addresses (None: NULL)"""
        p = lambda a: None if a is None else C.c_void_p(a)
        return self.lib.world_hip_gmm_convert(self.ctx, M, dx, dy, p(model), rows, p(x), x_rs, mode, p(mean), mean_rs, p(var), var_rs,
                                              p(post), post_rs, p(loglik))

    def call_accumulate(self, M, P, rows, z, z_rs, post, post_rs, shift, N, S1, G):
        p = lambda a: None if a is None else C.c_void_p(a)
        return self.lib.world_hip_gmm_accumulate(self.ctx, M, P, rows, p(z), z_rs, p(post), post_rs, p(shift), p(N), p(S1), p(G))

    def model_dev(self, model):
        return self.dev(model)

    def convert(self, M, dx, dy, d_model, x, mode=0, slack=0, want=("mean", "var", "post", "loglik"), before=0):
        """x [rows][dx] -> {"mean", "var", "post", "loglik"} (those wanted).  slack > 0: rows lie further apart, and every
        array has `before` rows ahead of and two rows behind the call's, all SENTINEL; what the call should not have
        written is checked to be there"""
        rows = len(x)
        extra = 2 if slack else 0
        xin = np.full((before + rows + extra, dx + slack), SENTINEL)
        xin[before:before + rows, :dx] = x
        cols = dict(mean=dy, var=dy, post=M, loglik=1)
        if dy == 0:
            want = [k for k in want if k in ("post", "loglik")]
        host = {k: np.full((before + rows + extra, cols[k] + (slack + i if k != "loglik" else 0)), SENTINEL) for i, k in enumerate(want)}
        dev = {k: self.dev(a) for k, a in host.items()}
        d_x = self.dev(xin)
        a = lambda k: self.addr(dev[k]) + 8 * before * host[k].shape[1] if k in dev else None
        rs = lambda k: host[k].shape[1] if k in dev else 0
        rc = self.call_convert(M, dx, dy, self.addr(d_model), rows, self.addr(d_x) + 8 * before * xin.shape[1], xin.shape[1], mode,
                               a("mean"), rs("mean"), a("var"), rs("var"), a("post"), rs("post"), a("loglik"))
        assert rc == 0, self.error()
        assert same_bits(self.host(d_x), xin), "the input changed"
        out = {}
        for k in want:
            got = self.host(dev[k])
            assert np.all(got[:before] == SENTINEL) and np.all(got[before + rows:] == SENTINEL), f"{k}: written outside the rows"
            assert np.all(got[:, cols[k]:] == SENTINEL), f"{k}: written beyond the row"
            out[k] = np.array(got[before:before + rows, :cols[k]])
        if "loglik" in out:
            out["loglik"] = out["loglik"][:, 0]
        return out

    def accumulate(self, z, post, shift, slack=0):
        """-> (N [M], S1 [M][P], G [M][P][P]); the three lie in one SENTINEL-filled array each, a guard double behind"""
        rows, P = z.shape
        M = post.shape[1]
        zin, pin = np.full((rows, P + slack), SENTINEL), np.full((rows, M + 2 * slack), SENTINEL)
        zin[:, :P], pin[:, :M] = z, post
        d_z, d_p, d_s = self.dev(zin), self.dev(pin), self.dev(np.ascontiguousarray(shift, dtype=np.float64))
        outs = [self.dev(np.full(n + 1, SENTINEL)) for n in (M, M * P, M * P * P)]
        rc = self.call_accumulate(M, P, rows, self.addr(d_z), zin.shape[1], self.addr(d_p), pin.shape[1], self.addr(d_s), *(self.addr(o) for o in outs))
        assert rc == 0, self.error()
        N, S1, G = (self.host(o) for o in outs)
        assert N[-1] == SENTINEL and S1[-1] == SENTINEL and G[-1] == SENTINEL, "written beyond the statistics"
        return np.array(N[:-1]), np.array(S1[:-1]).reshape(M, P), np.array(G[:-1]).reshape(M, P, P)

    def fit(self, z, n_iter, reg, w, mu, cov, slack=0, with_loglik=True):
        """-> (rc, w, mu, cov, loglik [n_iter])"""
        rows, P = z.shape
        zin = np.full((rows, P + slack), SENTINEL)
        zin[:, :P] = z
        d_z = self.dev(zin)
        w, mu, cov = (np.array(a, dtype=np.float64, order="C") for a in (w, mu, cov))
        ll = np.full(max(n_iter, 1), SENTINEL)
        rc = self.lib.world_hip_gmm_fit(self.ctx, len(w), P, rows, C.c_void_p(self.addr(d_z)), zin.shape[1], n_iter, float(reg), self._h(w),
                                        self._h(mu), self._h(cov), self._h(ll) if with_loglik else None)
        return rc, w, mu, cov, ll

    def init(self, z, M, slack=0):
        rows, P = z.shape
        zin = np.full((rows, P + slack), SENTINEL)
        zin[:, :P] = z
        d_z = self.dev(zin)
        w, mu, cov = np.full(M, SENTINEL), np.full((M, P), SENTINEL), np.full((M, P, P), SENTINEL)
        rc = self.lib.world_hip_gmm_init(self.ctx, M, P, rows, C.c_void_p(self.addr(d_z)), zin.shape[1], self._h(w), self._h(mu), self._h(cov))
        return rc, w, mu, cov


be = cpu_backend(Backend)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def random_model(M, dx, dy, seed, cond=1e3):
    """weights, means and joint covariances [M][P][P] whose condition number is `cond`"""
    rng = np.random.default_rng(seed)
    P = dx + dy
    w = rng.uniform(0.5, 1.5, M)
    w /= w.sum()
    mu = rng.standard_normal((M, P))
    cov = np.empty((M, P, P))
    for m in range(M):
        q, _ = np.linalg.qr(rng.standard_normal((P, P)))
        lam = np.logspace(0, -np.log10(cond), P) if P > 1 else np.ones(1)
        s = (q * lam) @ q.T
        cov[m] = 0.5 * (s + s.T)
    return w, mu, cov


def prepared(be, M, dx, dy, seed=1):
    """(the model's host doubles, its parts) of random_model(M, dx, dy, seed)"""
    def make():
        rc, model = be.prepare(*random_model(M, dx, dy, seed), dx)
        assert rc == 0, be.error()
        return model, be.parts(M, dx, dy, model)
    return backends.cached(("gmm-model", type(be).__name__, M, dx, dy, seed), make)


def rows_near(parts, rows, seed, spread=1.0):
    """rows drawn around the mixtures' source means"""
    rng = np.random.default_rng(seed)
    M, dx = parts["mux"].shape
    return parts["mux"][rng.integers(0, M, rows)] + spread * rng.standard_normal((rows, dx))


# ---- the statement --------------------------------------------------------------------------------------------------------
def rule_convert(parts, x):
    """the rule in long double on the model's parts: a dict of q, e [rows][M](...), gamma, loglik, best, mean / var of both
    modes, and the bounds of the module's docstring under the same names with a leading b"""
    c, mux, muy, U, A, v = (parts[k] for k in ("c", "mux", "muy", "U", "A", "v"))
    M, dx = mux.shape
    dy = muy.shape[1]
    rows = len(x)
    q, bq = np.empty((rows, M), dtype=LD), np.empty((rows, M), dtype=LD)
    e, de = np.empty((rows, M, dy), dtype=LD), np.empty((rows, M, dy), dtype=LD)
    for m in range(M):
        d = LD(x - mux[m])                                              # (rounded: the rule's d)
        z = d @ LD(U[m]).T
        dz = (dx + 4) * U53 * (np.abs(d) @ np.abs(LD(U[m])).T)
        ss = 0.5 * np.sum(z * z, axis=1)
        q[:, m] = LD(c[m]) - ss
        bq[:, m] = np.sum((np.abs(z) + dz) * dz, axis=1) + (dx + 4) * U53 * ss + 2 * U53 * (abs(c[m]) + np.abs(q[:, m]))
        e[:, m] = LD(muy[m]) + d @ LD(A[m]).T
        de[:, m] = (dx + 4) * U53 * (np.abs(LD(muy[m])) + np.abs(d) @ np.abs(LD(A[m])).T)
    best = np.argmax(q, axis=1)
    qmax = q[np.arange(rows), best]
    ex = np.exp(q - qmax[:, None])
    s = ex.sum(axis=1)
    loglik = qmax + np.log(s)
    gamma = ex / s[:, None]
    mbq = bq.max(axis=1)
    bl = mbq + (M + 8) * U53 * (1 + np.abs(np.log(s))) + 2 * U53 * np.abs(loglik)
    bg = gamma * (2 * mbq[:, None] + (M + 8 + np.abs(q - qmax[:, None])) * U53) + LD(1e-300)
    vv = LD(v)[None] + e * e
    mean0 = np.sum(gamma[:, :, None] * e, axis=1)
    bmean0 = np.sum(bg[:, :, None] * np.abs(e) + gamma[:, :, None] * de, axis=1) + (M + 4) * U53 * np.sum(gamma[:, :, None] * np.abs(e), axis=1)
    second = np.sum(gamma[:, :, None] * vv, axis=1)
    var0 = second - mean0 * mean0
    bvar0 = (np.sum(bg[:, :, None] * vv + 2 * gamma[:, :, None] * np.abs(e) * de, axis=1) + (M + 6) * U53 * second
             + 2 * np.abs(mean0) * bmean0 + 2 * U53 * mean0 * mean0)
    pick = np.arange(rows)
    return dict(q=q, bq=bq, e=e, de=de, best=best, loglik=loglik, bloglik=bl, post=gamma, bpost=bg,
                mean=[mean0, e[pick, best]], bmean=[bmean0, de[pick, best]], var=[var0, LD(v)[best]], bvar=[bvar0, np.zeros((rows, dy), dtype=LD)],
                margin=np.sort(q, axis=1)[:, -1] - (np.sort(q, axis=1)[:, -2] if M > 1 else -np.inf))


def worst(got, exact, bound):
    """the largest |got - exact| / bound (0 / 0 counts as 0)"""
    err = np.abs(LD(got) - exact)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def rule_stats(z, post, shift):
    """(N, S1, G) in long double and the bound's sums of magnitudes"""
    rows, P = z.shape
    M = post.shape[1]
    N, S1, G = np.empty(M, dtype=LD), np.empty((M, P), dtype=LD), np.empty((M, P, P), dtype=LD)
    mN, mS1, mG = np.empty(M, dtype=LD), np.empty((M, P), dtype=LD), np.empty((M, P, P), dtype=LD)
    for m in range(M):
        g, d = LD(post[:, m]), LD(z) - LD(shift[m])
        N[m], S1[m], G[m] = g.sum(), g @ d, (d * g[:, None]).T @ d
        mN[m], mS1[m], mG[m] = np.abs(g).sum(), np.abs(g) @ np.abs(d), np.abs(d * g[:, None]).T @ np.abs(d)
    k = (rows + 4) * U53
    return (N, S1, G), (k * mN, k * mS1, k * mG)


def lower_chol_inv(S, T):
    """(L, L^-1) of the symmetric positive definite S in the arithmetic of dtype T"""
    n = len(S)
    L, U = np.zeros((n, n), dtype=T), np.zeros((n, n), dtype=T)
    for i in range(n):
        for j in range(i + 1):
            s = S[i, j] - np.dot(L[i, :j], L[j, :j])
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    for j in range(n):
        for i in range(j, n):
            s = T(1 if i == j else 0) - np.dot(L[i, j:i], U[j:i, j])
            U[i, j] = s / L[i, i]
    return L, U


def rule_em(z, w, mu, cov, n_iter, reg, T):
    """n_iter iterations of the rule's EM in the arithmetic of dtype T -> (w, mu, cov, loglik [n_iter], the smallest N seen)"""
    z, w, mu, cov = T(z), T(w).copy(), T(mu).copy(), T(cov).copy()
    rows, P = z.shape
    M = len(w)
    ln2pi = np.log(T(2) * np.arccos(T(-1)))
    ll, n_min = [], np.inf
    for _ in range(n_iter):
        q = np.empty((rows, M), dtype=T)
        for m in range(M):
            L, U = lower_chol_inv(cov[m], T)
            y = (z - mu[m]) @ U.T
            q[:, m] = np.log(w[m]) - T(P) / 2 * ln2pi - np.sum(np.log(np.diag(L))) - np.sum(y * y, axis=1) / 2
        qmax = q.max(axis=1)
        ex = np.exp(q - qmax[:, None])
        s = ex.sum(axis=1)
        ll.append((qmax + np.log(s)).sum() / rows)
        g = ex / s[:, None]
        for m in range(M):
            d = z - mu[m]
            N = g[:, m].sum()
            n_min = min(n_min, float(N))
            delta = (g[:, m] @ d) / N
            w[m], mu[m] = N / rows, mu[m] + delta
            cov[m] = (d * g[:, m, None]).T @ d / N - np.outer(delta, delta) + T(reg) * np.eye(P, dtype=T)
    return w, mu, cov, np.array(ll, dtype=T), n_min


def two_clusters(rows=400, seed=7):
    """rows of a 2-mixture, 3-dimensional joint Gaussian with well-separated means, and a start near it"""
    rng = np.random.default_rng(seed)
    means = np.array([[-3.0, 0.0, 2.0], [3.0, 1.0, -2.0]])
    a = np.array([[1.0, 0.3, 0.0], [0.0, 0.8, 0.2], [0.1, 0.0, 0.6]])
    which = rng.random(rows) < 0.4
    z = np.where(which[:, None], means[0], means[1]) + rng.standard_normal((rows, 3)) @ a.T
    w0 = np.array([0.5, 0.5])
    mu0 = np.array([[-1.0, 0.0, 0.5], [1.0, 0.5, -0.5]])
    cov0 = np.stack([np.eye(3) * 4.0] * 2)
    return z, w0, mu0, cov0


# ---- the cases ------------------------------------------------------------------------------------------------------------
PREPARE = [(1, 1, 1), (2, 3, 3), (2, 17, 16), (1, 33, 0), (2, 16, 33), (5, 3, 1)]


def case_prepare(be, M, dx, dy):
    import mpmath
    mpmath.mp.prec = 140
    mpf = mpmath.mpf
    w, mu, cov = random_model(M, dx, dy, 3, cond=1e4)
    cov_upper_poisoned = cov.copy()
    cov_upper_poisoned[:, np.triu_indices(dx + dy, 1)[0], np.triu_indices(dx + dy, 1)[1]] = np.nan      # only the lower triangle is read
    rc, model = be.prepare(w, mu, cov_upper_poisoned, dx)
    assert rc == 0, be.error()
    got = be.parts(M, dx, dy, model)
    assert same_bits(got["mux"], mu[:, :dx]) and same_bits(got["muy"], mu[:, dx:])
    n, kappa = dx + dy, 1e4
    work = 4 * n * kappa * 2.0 ** -64
    ratio = 0.0
    for m in range(M):
        S = mpmath.matrix(cov[m].tolist())
        Sxx = S[:dx, :dx]
        L = mpmath.cholesky(Sxx)
        U = mpmath.inverse(L)
        c = mpmath.log(mpf(float(w[m]))) - mpf(dx) / 2 * mpmath.log(2 * mpmath.pi) - sum(mpmath.log(L[i, i]) for i in range(dx))
        exact = {"c": [c], "U": [U[i, j] if j <= i else mpf(0) for i in range(dx) for j in range(dx)]}
        if dy:
            Syx = S[dx:, :dx]
            A = Syx * (U.T * U)
            vd = [S[dx + i, dx + i] - sum(A[i, j] * Syx[i, j] for j in range(dx)) for i in range(dy)]
            exact["A"], exact["v"] = [A[i, j] for i in range(dy) for j in range(dx)], vd
        for k, ex in exact.items():
            g = np.asarray(got[k][m], dtype=np.float64).reshape(-1)
            scale = max(abs(float(x)) for x in ex)
            for gi, xi in zip(g, ex):
                bound = U53 * abs(xi) + work * scale
                err = abs(mpf(float(gi)) - xi)
                ratio = max(ratio, float(err / bound)) if bound else ratio
                assert err <= bound, f"{k} of mixture {m}: {float(err):.3e} beyond {float(bound):.3e}"
        assert np.all(np.triu(got["U"][m], 1) == 0)
    print(f"prepare M={M} Dx={dx} Dy={dy}: max error / bound = {ratio:.4f}")


def case_prepare_refusals(be):
    w, mu, cov = random_model(3, 2, 2, 5)
    bad = cov.copy()
    bad[1, 1, 0] = 5.0                                                   # Sxx of mixture 1 is no longer positive definite
    rc, model = be.prepare(w, mu, bad, 2)
    assert rc == 1 and "mixture 1" in be.error() and np.all(model == SENTINEL), be.error()
    w0 = w.copy()
    w0[2] = 0.0
    rc, model = be.prepare(w0, mu, cov, 2)
    assert rc == 1 and "mixture 2" in be.error() and np.all(model == SENTINEL)
    bad = cov.copy()
    bad[0, 3, 3] = 1e-9                                                  # Syy below what x explains: v < 0
    rc, model = be.prepare(w, mu, bad, 2)
    assert rc == 1 and "mixture 0" in be.error() and np.all(model == SENTINEL)
    wn = w.copy()
    wn[0] = np.nan
    assert be.prepare(wn, mu, cov, 2)[0] == 1 and "mixture 0" in be.error()
    # a negative reg, and one that is not finite
    N, S1, G = np.full(3, 10.0), np.zeros((3, 4)), np.stack([np.eye(4) * 10] * 3)
    for reg in (-1e-6, np.nan, np.inf):
        rc, w2, mu2, cov2 = be.update(N, S1, G, mu, 30, reg)
        assert rc == 1 and "reg" in be.error() and np.all(w2 == SENTINEL) and np.all(mu2 == SENTINEL) and np.all(cov2 == SENTINEL)
    assert be.lib.world_hip_gmm_model_doubles(0, 1, 1) < 0 and be.lib.world_hip_gmm_model_doubles(1, 129, 0) < 0
    assert be.lib.world_hip_gmm_model_doubles(257, 1, 0) < 0 and be.lib.world_hip_gmm_model_doubles(1, 1, 129) < 0


# (M, Dx, Dy, rows, strided)
CONVERT = [(1, 1, 1, 1, False), (2, 3, 3, 63, True), (5, 16, 17, 65, True), (17, 17, 16, 130, False), (2, 33, 33, 65, True),
           (5, 33, 0, 130, True), (17, 3, 1, 130, True), (1, 16, 3, 63, False), (2, 1, 33, 130, True), (5, 17, 0, 1, False)]
CONVERT_IDS = ["M%d-Dx%d-Dy%d-rows%d-%s" % (c[0], c[1], c[2], c[3], "strided" if c[4] else "dense") for c in CONVERT]


def case_convert(be, M, dx, dy, rows, strided):
    model, parts = prepared(be, M, dx, dy)
    d_model = be.model_dev(model)
    x = rows_near(parts, rows, 11)
    want = rule_convert(parts, x)
    figures = {}
    for mode in (0, 1):
        got = be.convert(M, dx, dy, d_model, x, mode=mode, slack=3 if strided else 0, before=1 if strided else 0)
        figures["loglik"] = worst(got["loglik"], want["loglik"], want["bloglik"])
        figures["gamma"] = worst(got["post"], want["post"], want["bpost"])
        assert figures["loglik"] <= 1 and figures["gamma"] <= 1, figures
        if M == 1:
            figures["q"] = worst(got["loglik"], want["q"][:, 0], want["bq"][:, 0])
            assert figures["q"] <= 1, figures
        if dy:
            if mode == 1:
                # (a row whose two best mixtures lie within the bound of q may pick either: none does at these shapes)
                assert np.all(want["margin"] > 2 * want["bq"].max(axis=1))
                assert same_bits(got["var"], parts["v"][want["best"]]), "mode 1: var is not v of the most likely mixture"
                figures["e"] = worst(got["mean"], want["mean"][1], want["bmean"][1])
                assert figures["e"] <= 1, figures
            else:
                figures["mean"] = worst(got["mean"], want["mean"][0], want["bmean"][0])
                figures["var"] = worst(got["var"], want["var"][0], want["bvar"][0])
                assert figures["mean"] <= 1 and figures["var"] <= 1, figures
    print(f"convert M={M} Dx={dx} Dy={dy} rows={rows}: max error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in figures.items()))
    return figures


def case_modes(be):
    # M = 1: both modes are the same numbers
    model, parts = prepared(be, 1, 17, 16)
    d_model = be.model_dev(model)
    x = rows_near(parts, 65, 13)
    a, b = be.convert(1, 17, 16, d_model, x, mode=0), be.convert(1, 17, 16, d_model, x, mode=1)
    assert same_bits(a["mean"], b["mean"]) and same_bits(a["post"], np.ones((65, 1))) and same_bits(a["loglik"], b["loglik"])
    assert np.all(np.abs(a["var"] - b["var"]) <= 4 * U53 * (parts["v"][0] + 2 * a["mean"] ** 2)), "M = 1: v + e^2 - e^2 is not v"
    # two identical mixtures (different target parts): a tie, and the lower index wins
    w, mu, cov = random_model(2, 3, 3, 17)
    w[:] = 0.5
    mu[1, :3], cov[1] = mu[0, :3], cov[0]
    mu[1, 3:] = mu[0, 3:] + 100.0
    rc, model = be.prepare(w, mu, cov, 3)
    assert rc == 0, be.error()
    parts = be.parts(2, 3, 3, model)
    x = rows_near(parts, 63, 19)
    hard = be.convert(2, 3, 3, be.model_dev(model), x, mode=1)
    assert same_bits(hard["post"], np.full((63, 2), 0.5))
    assert np.all(np.abs(hard["mean"] - mu[0, 3:]) < 50), "a tie did not pick the lower index"
    want = rule_convert(dict(parts, c=parts["c"][:1], mux=parts["mux"][:1], muy=parts["muy"][:1], U=parts["U"][:1], A=parts["A"][:1], v=parts["v"][:1]), x)
    assert worst(hard["mean"], want["mean"][1], want["bmean"][1]) <= 1
    # a row 10^3 standard deviations from every mean: a finite loglik, and gamma is a distribution
    for M in (2, 5, 17):
        model, parts = prepared(be, M, 3, 3)
        sd = np.sqrt(max(np.linalg.inv(parts["U"][m]).max() ** 2 for m in range(M)) * 3)
        x = rows_near(parts, 4, 23)
        x[1] += 1e3 * sd
        x[2] -= 1e3 * sd
        got = be.convert(M, 3, 3, be.model_dev(model), x)
        assert np.all(np.isfinite(got["loglik"])) and np.all(got["loglik"][1:3] < -1e5)
        assert np.all(np.isfinite(got["mean"])) and np.all(np.isfinite(got["var"]))
        total = np.sum(LD(got["post"]), axis=1)
        print(f"far rows, M={M}: |sum gamma - 1| = {float(np.max(np.abs(total - 1))) / U53:.2f} * 2^-53 (allowed {4 * M})")
        assert np.all(got["post"] >= 0) and np.all(np.abs(total - 1) <= 4 * U53 * M)


def case_row_independence(be):
    """the same rows alone, inside a batch of 130 and at another position: the same bits; a NaN row spoils no other"""
    M, dx, dy = 5, 17, 16
    model, parts = prepared(be, M, dx, dy)
    d_model = be.model_dev(model)
    x = rows_near(parts, 130, 29)
    keys = ("mean", "var", "post", "loglik")
    for mode in (0, 1):
        whole = be.convert(M, dx, dy, d_model, x, mode=mode)
        for t in (0, 15, 16, 63, 64, 129):
            alone = be.convert(M, dx, dy, d_model, x[t:t + 1], mode=mode, slack=2)
            assert all(same_bits(alone[k][0], whole[k][t]) for k in keys), f"row {t} alone differs"
        moved = be.convert(M, dx, dy, d_model, np.vstack([x[70:], x[:70]]), mode=mode, slack=5, before=3)
        assert all(same_bits(np.concatenate([moved[k][60:], moved[k][:60]]), whole[k]) for k in keys), "a row's position changes it"
        part = be.convert(M, dx, dy, d_model, x[:65], mode=mode, want=("mean", "loglik"))
        assert same_bits(part["mean"], whole["mean"][:65]) and same_bits(part["loglik"], whole["loglik"][:65]), "rows or the outputs asked for change a row"
        with be.fresh() as b2:
            again = b2.convert(M, dx, dy, b2.model_dev(model), x, mode=mode)
            assert all(same_bits(again[k], whole[k]) for k in keys), "a second context differs"
        bad = x.copy()
        bad[17, 3], bad[64, 0], bad[129, dx - 1] = np.nan, np.inf, np.nan
        got = be.convert(M, dx, dy, d_model, bad, mode=mode, slack=1)
        keep = np.ones(130, dtype=bool)
        keep[[17, 64, 129]] = False
        assert all(same_bits(got[k][keep], whole[k][keep]) for k in keys), "a row that is not finite changed another row"
        assert all(same_bits(be.convert(M, dx, dy, d_model, x, mode=mode)[k], whole[k]) for k in keys), "the call after differs"


ACCUMULATE = [(1, 1, 1), (2, 3, 63), (5, 16, 65), (2, 33, 130), (17, 17, 130), (2, 66, 65)]


def stats_inputs(M, P, rows, seed=31):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, P)) + 3.0
    post = rng.random((rows, M)) ** 3
    post /= post.sum(axis=1, keepdims=True)
    shift = 3.0 + 0.1 * rng.standard_normal((M, P))
    return z, post, shift


def case_accumulate(be, M, P, rows):
    z, post, shift = stats_inputs(M, P, rows)
    got = be.accumulate(z, post, shift, slack=2)
    exact, bound = rule_stats(z, post, shift)
    ratio = max(worst(g, e, b) for g, e, b in zip(got, exact, bound))
    print(f"accumulate M={M} P={P} rows={rows}: max error / bound = {ratio:.4f}")
    assert ratio <= 1
    assert same_bits(got[2], np.swapaxes(got[2], 1, 2)), "G is not bit-symmetric"
    again = be.accumulate(z, post, shift)
    assert all(same_bits(a, b) for a, b in zip(again, got)), "a repeat (or the strides) changes the statistics"
    with be.fresh() as b2:
        assert all(same_bits(a, b) for a, b in zip(b2.accumulate(z, post, shift), got)), "a second context differs"
    if rows >= 2:                                                       # two shards add to the whole
        cut = rows // 3 + 1
        a, b = be.accumulate(z[:cut], post[:cut], shift), be.accumulate(z[cut:], post[cut:], shift)
        for x, y, e, bd in zip(a, b, exact, bound):
            assert np.all(np.abs(LD(x) + LD(y) - e) <= bd + U53 * np.abs(e)), "two shards do not add to the whole"


def by_hand(be, z, w, mu, cov, reg):
    """one iteration through the single calls -> (rc of update, w, mu, cov, the mean log-likelihood before it)"""
    M, P = mu.shape
    rc, model = be.prepare(w, mu, cov, P)
    assert rc == 0, be.error()
    got = be.convert(M, P, 0, be.model_dev(model), z)
    N, S1, G = be.accumulate(z, got["post"], mu)
    total = LD(0)
    for v in got["loglik"]:
        total = total + LD(v)
    return be.update(N, S1, G, mu, len(z), reg) + (float(total / len(z)),)


def case_fit(be):
    z, w0, mu0, cov0 = two_clusters()
    reg = 1e-6
    # the restatement itself does not starve a mixture on this data, and its likelihood does not fall
    w_ld, mu_ld, cov_ld, ll_ld, n_min = rule_em(z, w0, mu0, cov0, 3, reg, LD)
    w_np, mu_np, cov_np, ll_np, _ = rule_em(z, w0, mu0, cov0, 3, reg, np.float64)
    assert n_min > 50 and np.all(np.diff(ll_ld) >= 0) and np.all(np.diff(ll_np) >= 0)
    # one iteration is the single calls, bit for bit
    rc, w1, mu1, cov1, ll1 = be.fit(z, 1, reg, w0, mu0, cov0, slack=2)
    assert rc == 0, be.error()
    rc_h, w_h, mu_h, cov_h, ll_h = by_hand(be, z, w0, mu0, cov0, reg)
    assert rc_h == 0 and same_bits(w1, w_h) and same_bits(mu1, mu_h) and same_bits(cov1, cov_h) and same_bits(ll1, [ll_h])
    # three iterations
    rc, w3, mu3, cov3, ll3 = be.fit(z, 3, reg, w0, mu0, cov0)
    assert rc == 0, be.error()
    print("loglik per iteration:", ll3)
    assert np.all(np.diff(ll3) >= 0), "the likelihood fell"
    for name, lib_v, np_v, ld_v in (("w", w3, w_np, w_ld), ("mu", mu3, mu_np, mu_ld), ("cov", cov3, cov_np, cov_ld), ("loglik", ll3, ll_np, ll_ld)):
        e_lib, e_np = float(np.max(np.abs(LD(lib_v) - ld_v))), float(np.max(np.abs(LD(np_v) - ld_v)))
        print(f"fit, {name}: library {e_lib:.3e}, float64 NumPy restatement {e_np:.3e} from the long-double restatement")
        assert e_lib <= 4 * e_np, name
    rc, _, _, _, ll_none = be.fit(z, 2, reg, w0, mu0, cov0, with_loglik=False)
    assert rc == 0 and np.all(ll_none == SENTINEL)
    return z, w0, mu0, cov0, (w3, mu3, cov3), (w_ld, mu_ld, cov_ld)


def case_fit_sklearn(be):
    mixture = pytest.importorskip("sklearn.mixture")
    z, w0, mu0, cov0 = two_clusters()
    reg = 1e-6
    w_ld, mu_ld, cov_ld, _, _ = rule_em(z, w0, mu0, cov0, 3, reg, LD)
    rc, w3, mu3, cov3, _ = be.fit(z, 3, reg, w0, mu0, cov0)
    assert rc == 0, be.error()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = mixture.GaussianMixture(n_components=2, covariance_type="full", reg_covar=reg, max_iter=3, tol=0, weights_init=w0,
                                     means_init=mu0, precisions_init=np.linalg.inv(cov0)).fit(z)
    for name, lib_v, sk_v, ld_v in (("w", w3, sk.weights_, w_ld), ("mu", mu3, sk.means_, mu_ld), ("cov", cov3, sk.covariances_, cov_ld)):
        e_lib, e_sk = float(np.max(np.abs(LD(lib_v) - ld_v))), float(np.max(np.abs(LD(sk_v) - ld_v)))
        print(f"fit, {name}: library {e_lib:.3e}, sklearn {e_sk:.3e} from the long-double restatement")
        assert e_lib <= 4 * e_sk, name


def case_starved(be):
    """M = 3 on two clusters, the third mixture far from every row: refused by name, the parameters as they were"""
    z, w0, mu0, cov0 = two_clusters()
    w = np.array([0.4, 0.4, 0.2])
    mu = np.vstack([mu0, [[500.0, 500.0, 500.0]]])
    cov = np.stack([np.eye(3) * 4.0] * 3)
    rc, w1, mu1, cov1, ll = be.fit(z, 3, 1e-6, w, mu, cov)
    assert rc == 1 and "mixture 2" in be.error() and "starved" in be.error(), be.error()
    assert same_bits(w1, w) and same_bits(mu1, mu) and same_bits(cov1, cov), "a refused fit changed the parameters"
    assert np.all(ll == SENTINEL)
    N, S1, G = np.array([10.0, 3.9]), np.zeros((2, 3)), np.stack([np.eye(3)] * 2)
    rc, w2, mu2, cov2 = be.update(N, S1, G, mu0, 14, 0.0)
    assert rc == 1 and "mixture 1" in be.error() and np.all(w2 == SENTINEL) and np.all(cov2 == SENTINEL)


def case_init(be):
    rng = np.random.default_rng(37)
    rows, P, M = 130, 5, 4
    z = rng.standard_normal((rows, P)) * np.arange(1, P + 1) + 10.0
    rc, w, mu, cov = be.init(z, M, slack=3)
    assert rc == 0, be.error()
    assert same_bits(w, np.full(M, 1.0 / M))
    assert same_bits(mu, z[[(2 * m + 1) * rows // (2 * M) for m in range(M)]])
    var = np.var(LD(z), axis=0)
    for m in range(M):
        assert np.all(cov[m][~np.eye(P, dtype=bool)] == 0)
        assert np.all(np.abs(LD(np.diag(cov[m])) - var) <= (rows + 8) * U53 * np.mean((LD(z) - LD(z[0])) ** 2, axis=0))
    rc, w, mu, cov, _ = be.fit(z, 2, 1e-6, w, mu, cov)
    assert rc == 0, be.error()


def case_refusals(be):
    M, dx, dy, rows = 2, 3, 3, 5
    model, parts = prepared(be, M, dx, dy)
    d_model = be.model_dev(model)
    d_x = be.dev(np.ones((rows + 1, dx + 2)))
    shapes = dict(mean=(rows + 1, dy + 2), var=(rows + 1, dy + 2), post=(rows + 1, M + 2), loglik=(rows + 1,))

    def refused(reason, **change):
        outs = {k: be.dev(np.full(s, SENTINEL)) for k, s in shapes.items()}
        a = dict(M=M, dx=dx, dy=dy, model=be.addr(d_model), rows=rows, x=be.addr(d_x), x_rs=dx + 2, mode=0, mean=be.addr(outs["mean"]),
                 mean_rs=dy + 2, var=be.addr(outs["var"]), var_rs=dy + 2, post=be.addr(outs["post"]), post_rs=M + 2, loglik=be.addr(outs["loglik"]))
        for k, v in change.items():
            a[k] = v(a, outs) if callable(v) else v
        rc = be.call_convert(**a)
        assert rc == 1, f"{reason}: accepted"
        assert be.error(), reason
        assert all(np.all(be.host(o) == SENTINEL) for o in outs.values()), f"{reason}: an output was written"

    refused("NULL d_model", model=None)
    refused("NULL d_x", x=None)
    refused("M = 0", M=0)
    refused("M = 257", M=257)
    refused("Dx = 0", dx=0)
    refused("Dx = 129", dx=129)
    refused("Dy = -1", dy=-1)
    refused("Dy = 129", dy=129)
    refused("rows = 0", rows=0)
    refused("x stride below the row", x_rs=dx - 1)
    refused("mean stride below the row", mean_rs=dy - 1)
    refused("var stride below the row", var_rs=dy - 1)
    refused("post stride below the row", post_rs=M - 1)
    refused("mode 2", mode=2)
    refused("mode -1", mode=-1)
    refused("d_mean with Dy = 0", dy=0, var=None)
    refused("d_var with Dy = 0", dy=0, mean=None)
    refused("the mean is the input", mean=lambda a, o: a["x"])
    refused("the posterior lies in the model", post=lambda a, o: a["model"] + 8)
    refused("two outputs overlap", var=lambda a, o: a["mean"] + 8)
    refused("loglik lies in the posterior", loglik=lambda a, o: a["post"] + 8 * (M + 2))
    assert be.lib.world_hip_gmm_convert(None, M, dx, dy, None, rows, None, dx, 0, None, 0, None, 0, None, 0, None) == 2
    # every output is optional
    assert be.call_convert(M, dx, dy, be.addr(d_model), rows, be.addr(d_x), dx + 2, 0, None, 0, None, 0, None, 0, None) == 0, be.error()

    # accumulate
    P = 3
    d_z, d_post, d_shift = be.dev(np.ones((rows, P + 1))), be.dev(np.full((rows, M + 1), 0.5)), be.dev(np.zeros((M, P)))

    def refused_acc(reason, **change):
        outs = dict(N=be.dev(np.full(M, SENTINEL)), S1=be.dev(np.full((M, P), SENTINEL)), G=be.dev(np.full((M, P, P), SENTINEL)))
        a = dict(M=M, P=P, rows=rows, z=be.addr(d_z), z_rs=P + 1, post=be.addr(d_post), post_rs=M + 1, shift=be.addr(d_shift),
                 N=be.addr(outs["N"]), S1=be.addr(outs["S1"]), G=be.addr(outs["G"]))
        for k, v in change.items():
            a[k] = v(a, outs) if callable(v) else v
        rc = be.call_accumulate(**a)
        assert rc == 1 and be.error(), f"{reason}: accepted"
        assert all(np.all(be.host(o) == SENTINEL) for o in outs.values()), f"{reason}: an output was written"

    for name in ("z", "post", "shift", "N", "S1", "G"):
        refused_acc(f"NULL {name}", **{name: None})
    refused_acc("M = 0", M=0)
    refused_acc("P = 0", P=0)
    refused_acc("P = 129", P=129)
    refused_acc("rows = 0", rows=0)
    refused_acc("z stride below the row", z_rs=P - 1)
    refused_acc("post stride below the row", post_rs=M - 1)
    refused_acc("G is the input", G=lambda a, o: a["z"])
    refused_acc("S1 lies in G", S1=lambda a, o: a["G"] + 8)
    refused_acc("N is the shift", N=lambda a, o: a["shift"])

    # fit and init
    z, w0, mu0, cov0 = two_clusters(60)
    d_zz = be.dev(z)
    h = Backend._h

    def refused_fit(reason, M=2, P=3, rows=60, zp=True, z_rs=3, n_iter=1, reg=1e-6, w=True, mu=True, cov=True):
        wv, muv, cv, ll = w0.copy(), mu0.copy(), cov0.copy(), np.full(3, SENTINEL)
        rc = be.lib.world_hip_gmm_fit(be.ctx, M, P, rows, C.c_void_p(be.addr(d_zz)) if zp else None, z_rs, n_iter, reg, h(wv) if w else None,
                                      h(muv) if mu else None, h(cv) if cov else None, h(ll))
        assert rc == 1 and be.error(), f"{reason}: accepted"
        assert same_bits(wv, w0) and same_bits(muv, mu0) and same_bits(cv, cov0) and np.all(ll == SENTINEL), f"{reason}: something was written"

    refused_fit("n_iter = 0", n_iter=0)
    refused_fit("a negative reg", reg=-1.0)
    refused_fit("reg is NaN", reg=float("nan"))
    refused_fit("reg is infinite", reg=float("inf"))
    refused_fit("NULL d_z", zp=False)
    refused_fit("NULL w", w=False)
    refused_fit("NULL mu", mu=False)
    refused_fit("NULL cov", cov=False)
    refused_fit("M = 0", M=0)
    refused_fit("P = 0", P=0)
    refused_fit("rows = 0", rows=0)
    refused_fit("a stride below the row", z_rs=2)
    wv, muv, cv = np.full(2, SENTINEL), np.full((2, 3), SENTINEL), np.full((2, 3, 3), SENTINEL)
    for kw in (dict(M=0), dict(rows=0), dict(z_rs=2), dict(P=129)):
        a = dict(M=2, P=3, rows=60, z_rs=3)
        a.update(kw)
        assert be.lib.world_hip_gmm_init(be.ctx, a["M"], a["P"], a["rows"], C.c_void_p(be.addr(d_zz)), a["z_rs"], h(wv), h(muv), h(cv)) == 1 and be.error()
    assert be.lib.world_hip_gmm_init(be.ctx, 2, 3, 60, None, 3, h(wv), h(muv), h(cv)) == 1
    assert be.lib.world_hip_gmm_init(be.ctx, 2, 3, 60, C.c_void_p(be.addr(d_zz)), 3, None, h(muv), h(cv)) == 1
    assert np.all(wv == SENTINEL) and np.all(muv == SENTINEL) and np.all(cv == SENTINEL)


def case_workspace(be):
    """convert keeps q / gamma [rows][M] and the best mixture [rows]; a repeat of the shape needs no more; accumulate none"""
    M, dx, dy, rows = 17, 17, 16, 3000
    model, parts = prepared(be, M, dx, dy)
    x = rows_near(parts, rows, 41)
    with be.fresh() as b:
        w0 = b.workspace()
        z, post, shift = stats_inputs(2, 3, 63)
        b.accumulate(z, post, shift)
        assert b.workspace() == w0, "accumulate took workspace"
        d_model = b.model_dev(model)
        first = b.convert(M, dx, dy, d_model, x)
        w1 = b.workspace()
        assert w1 - w0 >= 8 * rows * M + 4 * rows, "the workspace did not grow by q and the best mixture"
        again = b.convert(M, dx, dy, d_model, x, mode=0)
        assert all(same_bits(again[k], first[k]) for k in first)
        b.convert(M, dx, dy, d_model, x[:100], mode=1)
        assert b.workspace() == w1, "the workspace grew on a repeat of the shape, or on a smaller one"


def case_hostapi(host):
    """HostAPI's host calls are the C calls"""
    w, mu, cov = random_model(2, 3, 2, 53)
    model = host.gmm_prepare(w, mu, cov, 3)
    parts = host.gmm_model_parts(2, 3, 2, model)
    assert same_bits(parts["mux"], mu[:, :3]) and np.all(parts["v"] > 0) and parts["A"].shape == (2, 2, 3)
    with pytest.raises(RuntimeError, match="mixture 1"):
        host.gmm_prepare([0.5, -0.5], mu, cov, 3)
    w2, mu2, cov2 = host.gmm_update(np.full(2, 10.0), np.ones((2, 5)), np.stack([np.eye(5) * 20] * 2), mu, 20, reg=0.5)
    assert same_bits(w2, [0.5, 0.5]) and np.allclose(mu2, mu + 0.1) and np.allclose(cov2[0], np.eye(5) * 2.5 - 0.01)
    with pytest.raises(RuntimeError, match="starved"):
        host.gmm_update(np.full(2, 5.0), np.ones((2, 5)), np.stack([np.eye(5)] * 2), mu, 10)


# ---- voice conversion end to end: the data of the GPU file's tool test, and its NumPy restatement ---------------------------
VC_FS, VC_ORDER, VC_MIX, VC_ITER, VC_REG = 16000, 24, 2, 3, 1e-6
# (seed, base F0) of world_amd.synth.vowel, 0.5 s each: 808 joint rows of 100 dimensions, so that neither of the two mixtures
# falls below the 101 rows' worth of weight a full covariance needs (four utterances starve one in the restatement itself)
VC_UTTERANCES = tuple((seed, 100.0 + 12.0 * i) for i, seed in enumerate(range(3, 19, 2)))


def vc_target(mgc):
    """the other "speaker": a fixed affine map of the source's cepstra (float32 in, float32 out, as the files are)"""
    d = np.arange(mgc.shape[1])
    return (mgc.astype(np.float64) * (1.0 + 0.25 * np.cos(0.7 * d)) + 0.4 * np.sin(1.3 * d + 0.5)).astype("<f4")


def mcd_db(a, b):
    """the mean over the frames of 10 / ln 10 sqrt(2 sum over c1 .. of (a - b)^2)"""
    d = np.asarray(a, dtype=np.float64)[:, 1:] - np.asarray(b, dtype=np.float64)[:, 1:]
    return float(np.mean(10.0 / np.log(10.0) * np.sqrt(2.0 * np.sum(d * d, axis=1))))


def vc_delta_matrix(T):
    """W [2 T][T]: the statics and the [-0.5 0 0.5] deltas, the window truncated at the ends (the header's rule)"""
    W = np.zeros((2, T, T))
    W[0] = np.eye(T)
    for t in range(T):
        if t > 0:
            W[1, t, t - 1] = -0.5
        if t + 1 < T:
            W[1, t, t + 1] = 0.5
    return W


def vc_restatement(src, tgt):
    """the tools' chain in float64 NumPy on the source / target .mgc arrays (frame t of one belongs to frame t of the
    other: the target is made frame by frame) -> the converted arrays"""
    D = src[0].shape[1]
    dyn = lambda c: np.hstack([c, vc_delta_matrix(len(c))[1] @ c])
    z = np.vstack([np.hstack([dyn(s.astype(np.float64)), dyn(t.astype(np.float64))]) for s, t in zip(src, tgt)])
    rows, P = z.shape
    M, dx = VC_MIX, 2 * D
    w0 = np.full(M, 1.0 / M)
    mu0 = z[[(2 * m + 1) * rows // (2 * M) for m in range(M)]]
    cov0 = np.stack([np.diag(np.var(z, axis=0))] * M)
    w, mu, cov, ll, n_min = rule_em(z, w0, mu0, cov0, VC_ITER, VC_REG, np.float64)
    assert n_min >= P + 1, f"the restatement starves a mixture ({n_min} rows' worth of weight)"
    out = []
    for s in src:
        x = dyn(s.astype(np.float64))
        T = len(x)
        q, e, v = np.empty((T, M)), np.empty((T, M, dx)), np.empty((M, dx))
        for m in range(M):
            Sxx, Syx, Syy = cov[m][:dx, :dx], cov[m][dx:, :dx], cov[m][dx:, dx:]
            A = np.linalg.solve(Sxx, Syx.T).T
            d = x - mu[m, :dx]
            q[:, m] = np.log(w[m]) - 0.5 * np.linalg.slogdet(Sxx)[1] - 0.5 * np.sum(d * np.linalg.solve(Sxx, d.T).T, axis=1)
            e[:, m], v[m] = mu[m, dx:] + d @ A.T, np.diag(Syy - A @ Syx.T)
        g = np.exp(q - q.max(axis=1, keepdims=True))
        g /= g.sum(axis=1, keepdims=True)
        mean = np.sum(g[:, :, None] * e, axis=1)
        var = np.sum(g[:, :, None] * (v[None] + e * e), axis=1) - mean * mean
        W = vc_delta_matrix(T)
        c = np.empty((T, D))
        for k in range(D):
            p = [1.0 / var[:, n * D + k] for n in range(2)]
            R = sum(W[n].T @ (p[n][:, None] * W[n]) for n in range(2))
            c[:, k] = np.linalg.solve(R, sum(W[n].T @ (p[n] * mean[:, n * D + k]) for n in range(2)))
        out.append(c)
    return out


def case_vc_restatement(host):
    """the condition of the GPU file's tool test -- converted < half of unconverted -- holds for the NumPy restatement on
    that input (the source cepstra here come from the emulated analysis and the host's sp2mc table)"""
    from world_amd import synth
    fft_size, P1 = 1024, VC_ORDER + 1
    table = np.empty((P1, fft_size // 2 + 1))
    alpha = host.lib.world_hip_mcep_alpha(VC_FS)
    assert host.lib.world_hip_mcep_tables(fft_size, VC_ORDER, alpha, table.ctypes.data, None) == 0
    src = []
    for seed, base in VC_UTTERANCES:
        x = synth.vowel(VC_FS, 0.5, seed=seed, base_f0=base).numpy()
        tp, f0 = host.harvest(x, VC_FS)
        src.append((np.log(host.cheaptrick(x, VC_FS, tp, f0)) @ table.T).astype("<f4"))
    tgt = [vc_target(s) for s in src]
    conv = vc_restatement(src, tgt)
    before = np.mean([mcd_db(s, t) for s, t in zip(src, tgt)])
    after = np.mean([mcd_db(c, t) for c, t in zip(conv, tgt)])
    print(f"NumPy restatement: MCD to the target {before:.3f} dB unconverted, {after:.3f} dB converted")
    assert after < 0.5 * before


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_hostapi_host_calls(emu):
    case_hostapi(emu)


def test_the_numpy_restatement_of_the_conversion_halves_the_mcd(emu):
    case_vc_restatement(emu)


@pytest.mark.parametrize("M,dx,dy", PREPARE, ids=["M%d-Dx%d-Dy%d" % c for c in PREPARE])
def test_prepare_is_the_rule_in_140_bits(be, M, dx, dy):
    case_prepare(be, M, dx, dy)


def test_prepare_and_update_refuse_by_mixture(be):
    case_prepare_refusals(be)


@pytest.mark.parametrize("M,dx,dy,rows,strided", CONVERT, ids=CONVERT_IDS)
def test_convert_is_the_rule(be, M, dx, dy, rows, strided):
    case_convert(be, M, dx, dy, rows, strided)


def test_modes_ties_and_far_rows(be):
    case_modes(be)


def test_a_row_depends_on_nothing_but_the_row(be):
    case_row_independence(be)


@pytest.mark.parametrize("M,P,rows", ACCUMULATE, ids=["M%d-P%d-rows%d" % c for c in ACCUMULATE])
def test_accumulate_is_the_rule(be, M, P, rows):
    case_accumulate(be, M, P, rows)


def test_fit_is_the_single_calls_and_follows_the_restatement(be):
    case_fit(be)


def test_fit_against_sklearn(be):
    case_fit_sklearn(be)


def test_a_starved_mixture_is_refused(be):
    case_starved(be)


def test_init_is_the_default_start(be):
    case_init(be)


def test_refusals_write_nothing_and_give_a_reason(be):
    case_refusals(be)


def test_workspace_grows_once(be):
    case_workspace(be)
