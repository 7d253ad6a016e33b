"""All-pass mel-cepstra (include/world_hip.h: world_hip_sp2mc / world_hip_mc2sp and their host arithmetic) through the
host functions of the built library and the host-compiled kernels (tests/emu/libworld_emu.so).  SPTK is not at hand and
the reference has no such function: THE HEADER'S STATEMENT IS THE ORACLE, written out here a second time with mpmath at 42
digits (140 bits) and np.longdouble.  The cases are functions of a backend, so that tests/test_mcep_gpu.py runs the same ones
through the shipped library.

Oracles.
  exact tables  A by the header's recursion and cos / atan2 in mpmath; the product A F in exact integer arithmetic on values
                scaled by 2^140 (rounding 2^-140 per factor).  Used for the table test (the first three shapes and the
                alpha = 0 shape).
  long double   M by the same statement in np.longdouble (cos from mpmath, rounded to 64 bits): its error is about K 2^-64 of
                a row's absolute sum, and the table test holds it to a sixteenth of the table bound against the exact
                tables: 2^-56 max |row| per entry, an eighth or less of ONE of the K + 4 roundings the bound below allows.
                D is always mpmath's, rounded to long double.  Used as the "exact table" of the encode / decode bounds at every shape (the exact product at
                2048 / 59 would take a minute of big-integer arithmetic).
  logs          mpmath, rounded to long double.
Bounds (the statement's; none comes from the code under test).
  table   |table - exact| <= 2^-52 max_k |row|, per row: long double rounded once to double lands within 2^-53 of the row's
          largest entry; the other half is the margin for the long-double sums.
  encode  |mc_m - oracle_m| <= (K + 4) 2^-53 sum_k |M[m][k]| |ln sp_k|: the dot-product bound in any summation order, with or
          without FMA, plus one rounding each for ln and the table.
  decode  |ln(sp) - sum_m D[k][m] mc_m| <= (P + 4) 2^-53 sum_m |D[k][m]| |mc_m| + 4 2^-53 (the last term: exp).
Inputs: envelopes exp(-8 - 6 f + 3 cos 7 f + noise), f = k / H; the noise is 0.5 N(0, 1) per bin plus a level of 0, 4 or 9 per
row, so that ln sp has both signs (the curve alone stays below -5) over about 40 dB within a row."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import backends
from backends import SENTINEL_F64 as SENTINEL, cached, cpu_backend, lib, same_bits  # noqa: F401 (lib: a fixture)

LD = np.longdouble
SHAPES = [(128, 24, 0.42), (256, 39, 0.554), (512, 59, -0.3), (128, 0, 0.41), (128, 64, 0.0), (2048, 59, 0.554)]
SHAPE_IDS = ["%d-%d-%g" % s for s in SHAPES]
TABLE_SHAPES = SHAPES[:3] + [SHAPES[4]]
TABLE_IDS = SHAPE_IDS[:3] + [SHAPE_IDS[4]]
ROWS = (1, 17, 67)
ALPHAS = {8000: 0.312, 16000: 0.41, 22050: 0.455, 24000: 0.466, 32000: 0.504, 44100: 0.544, 48000: 0.554, 96000: 0.63,
          192000: 0.693}
U = 2.0 ** -53
BITS = 140

# ---- the statement, in mpmath ---------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.prec = BITS + 20
    return mpmath


def mp_to_ld(x):
    """an mpmath number -> the nearest long double (two doubles, added in long double)"""
    mp = _mp()
    d1 = float(x)
    return LD(d1) + LD(float(x - mp.mpf(d1)))


def int_to_ld(v, bits):
    """v / 2^bits, v a Python integer -> long double"""
    d1 = float(Fraction(v, 1 << bits))
    return LD(d1) + LD(float(Fraction(v, 1 << bits) - Fraction(d1)))


def mp_cos_table(H):
    mp = _mp()
    return [mp.cos(mp.pi * j / H) for j in range(2 * H)]


def mp_warped(H, alpha):
    mp = _mp()
    a = mp.mpf(alpha)
    w = [mp.pi * k / H for k in range(H + 1)]
    return [x + 2 * mp.atan2(a * mp.sin(x), 1 - a * mp.cos(x)) for x in w]


def exact_tables(fft_size, order, alpha):
    """(M [P][K], D [K][P]) as long doubles, rounded from the exact values"""
    def make():
        mp = _mp()
        N, H = fft_size, fft_size // 2
        K, P = H + 1, order + 1
        a = mp.mpf(alpha)
        A = [[mp.mpf(0)] * K for _ in range(P)]
        A[0][0] = mp.mpf(1)
        for n in range(1, K):
            A[0][n] = a * A[0][n - 1]
            if P > 1:
                A[1][n] = (1 - a * a) * A[0][n - 1] + a * A[1][n - 1]
            for m in range(2, P):
                A[m][n] = A[m - 1][n - 1] + a * (A[m][n - 1] - A[m - 1][n])
        scale = mp.mpf(2) ** BITS
        w2 = [1 if n in (0, H) else 2 for n in range(K)]                       # 2 w
        Ai = np.array([[int(mp.nint(A[m][n] * scale)) * w2[n] for n in range(K)] for m in range(P)], dtype=object)
        ci = [int(mp.nint(c * scale)) for c in mp_cos_table(H)]
        Fi = np.array([[ci[(n * k) % (2 * H)] * w2[k] for k in range(K)] for n in range(K)], dtype=object)
        Mi = Ai.dot(Fi)                                                        # = M * 2^(2 BITS) * 2 N  (2 w_n 2 w_k N / 2)
        shift = 2 * BITS + 1 + int(np.log2(N))
        M = np.array([[int_to_ld(int(v), shift) for v in row] for row in Mi], dtype=LD)
        return M, exact_decode_table(fft_size, order, alpha)
    return cached(("exact", fft_size, order, alpha), make)


def exact_decode_table(fft_size, order, alpha):
    """D [K][P] from mpmath, rounded to long double"""
    def make():
        mp = _mp()
        wt = mp_warped(fft_size // 2, alpha)
        return np.array([[mp_to_ld(2 * mp.cos(m * w)) for m in range(order + 1)] for w in wt], dtype=LD)
    return cached(("D", fft_size, order, alpha), make)


def ld_encode_table(fft_size, order, alpha):
    """M [P][K] by the statement in long double (see the docstring)"""
    def make():
        N, H = fft_size, fft_size // 2
        K, P = H + 1, order + 1
        a = LD(alpha)
        A = np.zeros((P, K), dtype=LD)
        A[0, 0] = 1
        for n in range(1, K):
            A[0, n] = a * A[0, n - 1]
            if P > 1:
                A[1, n] = (1 - a * a) * A[0, n - 1] + a * A[1, n - 1]
            for m in range(2, P):
                A[m, n] = A[m - 1, n - 1] + a * (A[m, n - 1] - A[m - 1, n])
        cosT = np.array([mp_to_ld(c) for c in mp_cos_table(H)], dtype=LD)
        w = np.ones(K, dtype=LD)
        w[0] = w[H] = LD(0.5)
        idx = (np.arange(K, dtype=np.int64)[:, None] * np.arange(K, dtype=np.int64)[None, :]) % (2 * H)
        F = cosT[idx] * w[:, None] * w[None, :] * (LD(2) / N)
        M = A.dot(F)
        return M
    return cached(("ld", fft_size, order, alpha), make)


def envelopes(fft_size):
    """67 rows [K], shared and never changed"""
    def make():
        H = fft_size // 2
        rng = np.random.default_rng(fft_size)
        f = np.arange(H + 1) / H
        level = np.array([0.0, 4.0, 9.0])[np.arange(max(ROWS)) % 3]
        return np.exp(-8.0 - 6.0 * f + 3.0 * np.cos(7.0 * f) + 0.5 * rng.standard_normal((max(ROWS), H + 1)) + level[:, None])
    return cached(("sp", fft_size), make)


def mp_logs(fft_size):
    """ln of envelopes(fft_size) by mpmath -> long double"""
    def make():
        mp = _mp()
        sp = envelopes(fft_size)
        return np.array([[mp_to_ld(mp.log(mp.mpf(float(v)))) for v in row] for row in sp], dtype=LD)
    return cached(("ln", fft_size), make)


def encode_oracle(fft_size, order, alpha):
    """(mc [67][P] long double, bound [67][P])"""
    def make():
        M = ld_encode_table(fft_size, order, alpha)
        ln = mp_logs(fft_size)
        K = fft_size // 2 + 1
        return ln.dot(M.T), (K + 4) * LD(U) * np.abs(ln).dot(np.abs(M).T)
    return cached(("enc", fft_size, order, alpha), make)


# ---- a backend: the C calls on arrays that live where the library wants them ---------------------------------------------
class Backend(backends.Backend):
    """world_hip_sp2mc / _mc2sp on the arrays of backends.Backend"""

    def call(self, decode, rows, fft_size, order, alpha, in_ptr, in_stride, out_ptr, out_stride):
        """the C call itself on addresses (None: NULL)"""
        fn = self.lib.world_hip_mc2sp if decode else self.lib.world_hip_sp2mc
        return fn(self.ctx, rows, fft_size, order, alpha, None if in_ptr is None else C.c_void_p(in_ptr), in_stride,
                  None if out_ptr is None else C.c_void_p(out_ptr), out_stride)

    def run(self, decode, x, fft_size, order, alpha, in_stride=None, out_stride=None, in_col0=0):
        """x [rows][cols] -> the output rows [rows][out_cols].  The input rows lie in_stride doubles apart from column in_col0
        of an array filled with SENTINEL; the output array has out_stride columns and two more rows, filled with SENTINEL,
        and what the call should not have written is checked to be there still."""
        rows, cols = x.shape
        K, P = fft_size // 2 + 1, order + 1
        out_cols = K if decode else P
        assert cols == (P if decode else K)
        in_stride = in_stride or cols
        out_stride = out_stride or out_cols
        xin = np.full((rows, in_stride), SENTINEL)
        xin[:, in_col0:in_col0 + cols] = x
        d_in, d_out = self.dev(xin), self.dev(np.full((rows + 2, out_stride), SENTINEL))
        rc = self.call(decode, rows, fft_size, order, alpha, self.addr(d_in) + 8 * in_col0, in_stride, self.addr(d_out), out_stride)
        assert rc == 0, self.error()
        out = self.host(d_out)
        assert np.all(out[:rows, out_cols:] == SENTINEL), "written beyond the row"
        assert np.all(out[rows:] == SENTINEL), "written beyond `rows`"
        assert same_bits(self.host(d_in), xin), "the input changed"
        return np.array(out[:rows, :out_cols])


be = cpu_backend(Backend)


def library_tables(lib, fft_size, order, alpha):
    def make():
        K, P = fft_size // 2 + 1, order + 1
        M, D = np.full((P, K), SENTINEL), np.full((K, P), SENTINEL)
        assert lib.world_hip_mcep_tables(fft_size, order, alpha, C.c_void_p(M.ctypes.data), C.c_void_p(D.ctypes.data)) == 0
        M2, D2 = np.full((P, K), SENTINEL), np.full((K, P), SENTINEL)       # either may be NULL
        assert lib.world_hip_mcep_tables(fft_size, order, alpha, C.c_void_p(M2.ctypes.data), None) == 0
        assert lib.world_hip_mcep_tables(fft_size, order, alpha, None, C.c_void_p(D2.ctypes.data)) == 0
        assert same_bits(M, M2) and same_bits(D, D2)
        return M, D
    return cached(("lib", id(lib), fft_size, order, alpha), make)


# ---- the cases -----------------------------------------------------------------------------------------------------------
def case_alpha(lib):
    for fs, want in ALPHAS.items():
        assert lib.world_hip_mcep_alpha(fs) == want, (fs, lib.world_hip_mcep_alpha(fs))
    assert np.isnan(lib.world_hip_mcep_alpha(0)) and np.isnan(lib.world_hip_mcep_alpha(-16000))


def case_tables(lib, fft_size, order, alpha):
    M, D = library_tables(lib, fft_size, order, alpha)
    Mx, Dx = exact_tables(fft_size, order, alpha)
    for name, got, exact, ld in (("M", M, Mx, ld_encode_table(fft_size, order, alpha)), ("D", D, Dx, Dx)):
        top = np.max(np.abs(exact), axis=1)
        err = np.abs(LD(got) - exact)
        worst = float(np.max(err / (2 * LD(U) * top[:, None])))
        oracle_gap = float(np.max(np.abs(ld - exact) / (2 * LD(U) * top[:, None])))
        print(f"tables {fft_size}/{order}/{alpha}: {name} max |library - exact| = {worst:.3f} of 2^-52 max|row|; "
              f"the long-double oracle {oracle_gap:.2e} of it")
        assert np.all(err <= 2 * LD(U) * top[:, None]), name
        assert oracle_gap <= 2.0 ** -4, name                    # the oracle of the encode / decode cases: see the docstring
    if alpha == 0.0:
        H = fft_size // 2
        m, k = np.meshgrid(np.arange(order + 1), np.arange(H + 1), indexing="ij")
        zero = (2 * m * k) % (2 * H) == H                       # cos(pi m k / H) = 0
        assert zero.any()
        assert np.all(np.abs(M[zero]) <= 2 * U * np.broadcast_to(np.max(np.abs(M), axis=1)[:, None], M.shape)[zero])
        assert np.all(np.abs(D.T[zero]) <= 2 * U * 2.0)


def strides_for(K, P):
    return ((None, None), (K + 5, P + 3))


def case_encode(be, fft_size, order, alpha):
    K, P = fft_size // 2 + 1, order + 1
    sp = envelopes(fft_size)
    want, bound = encode_oracle(fft_size, order, alpha)
    assert np.any(np.log(sp) > 0) and np.any(np.log(sp) < 0)
    for rows in ROWS:
        for sp_stride, mc_stride in strides_for(K, P):
            got = be.run(False, sp[:rows], fft_size, order, alpha, sp_stride, mc_stride)
            err = np.abs(LD(got) - want[:rows])
            print(f"encode {fft_size}/{order}/{alpha} rows {rows} strides {sp_stride}, {mc_stride}: "
                  f"max error / bound = {float(np.max(err / bound[:rows])):.4f}")
            assert np.all(err <= bound[:rows])


def decode_inputs(fft_size, order, alpha):
    return cached(("mc", fft_size, order, alpha), lambda: np.array(encode_oracle(fft_size, order, alpha)[0], dtype=np.float64))


def decode_bound(D, mc):
    return (D.shape[1] + 4) * LD(U) * np.abs(LD(mc)).dot(np.abs(D).T) + 4 * LD(U)


def case_decode(be, fft_size, order, alpha):
    K, P = fft_size // 2 + 1, order + 1
    D = exact_decode_table(fft_size, order, alpha)
    mc = decode_inputs(fft_size, order, alpha)
    want, bound = LD(mc).dot(D.T), decode_bound(D, mc)
    for rows in ROWS:
        for sp_stride, mc_stride in strides_for(K, P):
            got = be.run(True, mc[:rows], fft_size, order, alpha, mc_stride, sp_stride)
            assert np.all(np.isfinite(got)) and np.all(got > 0)
            err = np.abs(np.log(LD(got)) - want[:rows])
            print(f"decode {fft_size}/{order}/{alpha} rows {rows} strides {mc_stride}, {sp_stride}: "
                  f"max error / bound = {float(np.max(err / bound[:rows])):.4f}")
            assert np.all(err <= bound[:rows])


def case_round_trip(be):
    """order = H and alpha = 0: nothing is truncated and nothing warped, so decode(encode(sp)) = sp within the two bounds"""
    fft_size, order, alpha = SHAPES[4]
    assert order == fft_size // 2 and alpha == 0.0
    D = exact_decode_table(fft_size, order, alpha)
    sp, ln = envelopes(fft_size), mp_logs(fft_size)
    mc = be.run(False, sp, fft_size, order, alpha)
    back = be.run(True, mc, fft_size, order, alpha)
    bound = decode_bound(D, mc) + encode_oracle(fft_size, order, alpha)[1].dot(np.abs(D).T)
    err = np.abs(np.log(LD(back)) - ln)
    print(f"round trip {fft_size}/{order}: max |ln back - ln sp| / bound = {float(np.max(err / bound)):.4f}, "
          f"max relative change {float(np.max(np.abs(back / sp - 1))):.3g}")
    assert np.all(err <= bound)


def case_rows_are_independent(be, fft_size, order, alpha):
    """a row alone, a subset, the rows inside packed records, and the neighbours of a poisoned row: the same bits as in the
    67-row call"""
    K, P = fft_size // 2 + 1, order + 1
    sp, mc = envelopes(fft_size), decode_inputs(fft_size, order, alpha)
    subset = [66, 3, 40, 17, 16, 5, 31]
    for decode, x in ((False, sp), (True, mc)):
        full = be.run(decode, x, fft_size, order, alpha)
        for r in (0, 15, 16, 17, 31, 32, 63, 64, 66):
            assert same_bits(be.run(decode, x[r:r + 1], fft_size, order, alpha), full[r:r + 1]), (decode, r)
        assert same_bits(be.run(decode, x[subset], fft_size, order, alpha), full[subset]), decode
        with be.fresh() as other:
            assert same_bits(other.run(decode, x[:17], fft_size, order, alpha), full[:17])
        bad = np.array(x)
        bad[5, 0], bad[5, x.shape[1] // 2], bad[5, -1] = 0.0, -1.0, float("nan")
        got = be.run(decode, bad, fft_size, order, alpha)
        keep = np.arange(len(x)) != 5
        assert same_bits(got[keep], full[keep]), decode
    # the envelopes of packed f64 records [tpos, f0, sp[K], ap[K]], read where they lie; the coefficients written into
    # coded-style records [tpos, f0, mc[P], bap[5]]
    full = be.run(False, sp, fft_size, order, alpha)
    cols = be.lib.world_hip_record_columns(fft_size, 0)
    assert cols == 2 + 2 * K
    assert same_bits(be.run(False, sp, fft_size, order, alpha, in_stride=cols, out_stride=2 + P + 5, in_col0=2), full)


def case_refusals(be):
    """every refusal of the header: an error, the reason names the argument, and nothing is written"""
    fft_size, order, alpha = SHAPES[0]
    K, P = fft_size // 2 + 1, order + 1
    for decode in (False, True):
        cols_in, cols_out = (P, K) if decode else (K, P)
        x = envelopes(fft_size)[:3, :cols_in]
        d_in, d_out = be.dev(x), be.dev(np.full((3, cols_out), SENTINEL))
        ok = dict(rows=3, fft_size=fft_size, order=order, alpha=alpha, in_ptr=be.addr(d_in), in_stride=cols_in,
                  out_ptr=be.addr(d_out), out_stride=cols_out)

        def refused(word, **change):
            a = dict(ok, **change)
            assert be.call(decode, **a) == 1, change
            assert word in be.error() and ("mc2sp" if decode else "sp2mc") in be.error(), (change, be.error())
            assert np.all(be.host(d_out) == SENTINEL) and same_bits(be.host(d_in), x), change

        refused("rows", rows=0)
        refused("rows", rows=-2)
        refused("null", in_ptr=None)
        refused("null", out_ptr=None)
        for bad in (0, 64, 100, 129, 16384, -128):
            refused("fft_size", fft_size=bad)
        for bad in (-1, fft_size // 2 + 1, 255):
            refused("order", order=bad)
        refused("order", order=-1, in_stride=4096, out_stride=4096)
        refused("order", order=256, fft_size=1024, in_stride=4096, out_stride=4096)
        for bad in (float("nan"), float("inf"), -float("inf"), 0.9000001, -0.95, 1.0):
            refused("alpha", alpha=bad)
        refused("mc_row_stride" if decode else "sp_row_stride", in_stride=cols_in - 1)
        refused("sp_row_stride" if decode else "mc_row_stride", out_stride=cols_out - 1)
        refused("stride", in_stride=0)
        refused("stride", out_stride=-cols_out)
        both = be.dev(np.full((8, K + P), 1.0))
        for offset in (0, 8 * cols_in, 8 * (2 * (K + P) + 3)):  # the same start, the input's first row end, somewhere inside
            rc = be.call(decode, 3, fft_size, order, alpha, be.addr(both), K + P, be.addr(both) + offset, K + P)
            assert rc == 1 and "overlap" in be.error(), (decode, offset)
            assert np.all(be.host(both) == 1.0)
        assert be.call(decode, **ok) == 0, be.error()
        assert np.all(be.host(d_out) != SENTINEL)
    M = np.full((P, K), SENTINEL)
    for bad, word in (((100, order, alpha), "fft_size"), ((fft_size, 65, alpha), "order"), ((fft_size, order, 0.95), "alpha")):
        assert be.lib.world_hip_mcep_tables(*bad, C.c_void_p(M.ctypes.data), None) == 1
        assert word in be.error() and np.all(M == SENTINEL)


def case_table_cache_turns_over(be):
    """more shapes than the context keeps tables for, then the first again: the same bits, and the workspace count moves
    with the tables"""
    fft_size, order, alpha = SHAPES[2]
    sp = envelopes(fft_size)[:5]
    with be.fresh() as b:
        base = b.lib.world_hip_workspace_bytes(b.ctx)
        first = b.run(False, sp, fft_size, order, alpha)
        one = b.lib.world_hip_workspace_bytes(b.ctx) - base
        assert one >= 8 * (fft_size // 2 + 1) * (order + 1)
        b.run(False, sp, fft_size, order, alpha)
        assert b.lib.world_hip_workspace_bytes(b.ctx) - base == one           # found again
        for k in range(6):
            b.run(False, sp, fft_size, order + 1 + 20 * k, alpha + 0.01 * k)  # (61 .. 161 coefficients: all three widths)
        assert same_bits(b.run(False, sp, fft_size, order, alpha), first)


# ---- the tests -----------------------------------------------------------------------------------------------------------
def test_default_alpha_of_nine_rates(lib):
    case_alpha(lib)


@pytest.mark.parametrize("fft_size,order,alpha", TABLE_SHAPES, ids=TABLE_IDS)
def test_tables_against_mpmath(lib, fft_size, order, alpha):
    case_tables(lib, fft_size, order, alpha)


@pytest.mark.parametrize("fft_size,order,alpha", SHAPES, ids=SHAPE_IDS)
def test_encode_within_the_dot_product_bound(be, fft_size, order, alpha):
    case_encode(be, fft_size, order, alpha)


@pytest.mark.parametrize("fft_size,order,alpha", SHAPES, ids=SHAPE_IDS)
def test_decode_within_the_dot_product_bound(be, fft_size, order, alpha):
    case_decode(be, fft_size, order, alpha)


def test_full_order_unwarped_round_trip(be):
    case_round_trip(be)


@pytest.mark.parametrize("fft_size,order,alpha", [SHAPES[1], SHAPES[4]], ids=[SHAPE_IDS[1], SHAPE_IDS[4]])
def test_a_row_depends_on_nothing_but_the_row(be, fft_size, order, alpha):
    case_rows_are_independent(be, fft_size, order, alpha)


def test_refusals_write_nothing_and_name_the_argument(be):
    case_refusals(be)


def test_table_cache_turns_over(be):
    case_table_cache_turns_over(be)
