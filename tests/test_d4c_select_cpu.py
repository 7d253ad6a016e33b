"""D4C's band selection alone (include/world_hip.h: world_hip_probe_select; world_amd/csrc/d4c.hip: block_excluding_largest and
the general routine block_smallest_sum behind it), on the wave-accurate host emulation (tests/emu: the shipped wave collectives).
The cases are functions of a backend, so that tests/test_d4c_select_gpu.py runs the same ones through the shipped library.

The statement.  A row is 10 NT slot values.  Sorted ascending, `partial` is the sum of the 10 NT - K smallest and `total` the
sum of all.  THE STATEMENT IS THE ORACLE: statement() sorts in plain Python and sums with math.fsum (exact whenever the exact
sum is a double) or fractions.Fraction.  Keys are finite doubles with the sign bit clear.

Two kinds of expectation; neither comes from the code under test.
  lattice   every key is an integer multiple of one power of two 2^e and total / 2^e < 2^53 (asserted on the host,
            lattice_precondition): every partial sum in every order is exact, so both outputs must equal the statement's BIT FOR
            BIT.  Every lattice row runs at four scales -- its smallest key at 2^-1022 (as low as keeps every key normal), at
            2^-80 (where a real 4 |X|^2 sits), at 2^0 and at 2^900; the scale is a uniform shift of the exponent fields, so
            the route must not change and the outputs only by that factor (each scale is held to its own statement).
  real      4 |X|^2 of numpy.fft.rfft of Nuttall-windowed random slices in d4c_frame's ownership, and log-uniform draws over
            12 decades: |got - exact| <= (n - 1) 2^-53 exact, n the non-zero terms -- the bound of a sum of non-negative terms
            in ANY order.  The host first asserts that the K-th and (K+1)-th largest keys differ by more than four times that
            bound, so a wrong exclusion cannot hide inside it.
Every row NAMES the route it must take (0 one pass, 1 two passes, 2 the general routine) and the probe's report is held to it.
The designed rows name it by construction; the real-valued rows by route_rule(), the documented rule (d4c.hip's comment above
block_excluding_largest) restated on the high words -- which the designed rows check too, so the rule is itself tested.
Mode 1 (the general routine called directly) runs on every row: bit for bit the statement on lattice rows, inside the bound
on real ones.

How the lattice rows are built.  A row is written as RELATIVE bit patterns (exponent fields 1 .. 6; 0 = the padding value 0.0)
whose mantissas use the top b bits only; realise() shifts the exponent fields to the scale.  Every thread gets one key at or
above the floor FL (the `uppers`: what the fast path histograms), the designs differ in how the uppers' high words lie:
  one pass     distinct fine bins 1024 high words apart (s0 = 7 .. 10), random neighbours merged into shared bins -- never the
               K-th largest's
  two passes   consecutive high words (2^s1 apart) and ONE outlier that makes the range 2^(10 + s0) - 1: 2^s0 / 2^s1 keys
               in every fine bin, one each in the 256-bin pass; s0 = 3 and 8 (s1 = 0) and 10 (s1 = 2)
  general      K = NT + 1; every upper in one high word (tp == fl); consecutive high words (s0 = 0) with the threshold pair
               differing by the lattice's lowest low-word bit; the two-pass rows with such a pair; exact ties of 2, 3, 5, 7
               across the threshold ((remaining + 1) thr with remaining = 0 .. 3); every slot of every thread in one high word
               (hmin == hmax on real minima); all real keys equal; thresholds that need five or six passes (more than kSelHists)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import backends
from backends import SENTINEL_F64 as SENTINEL, cached, cpu_backend, lib, same_bits  # noqa: F401 (lib: a fixture)

NTS = (128, 256, 512, 1024)
SLOTS = 10
U = 2.0 ** -53
FL = 4 << 20                                   # the floor's relative high word: exponent field 4, mantissa 0
SCALES = {"2^-1022": 1, "2^-80": 1023 - 80, "2^0": 1023, "2^900": 1023 + 900}      # exponent field of a row's smallest key


# ---- the statement --------------------------------------------------------------------------------------------------------
def statement(row, K, exact=False):
    """(partial, total) of one row [NT][10]: floats by math.fsum, or Fractions"""
    s = np.sort(np.asarray(row, dtype=np.float64).ravel()).tolist()
    keep = s[:len(s) - K]
    if exact:
        return sum(map(Fraction, keep), Fraction(0)), sum(map(Fraction, s), Fraction(0))
    return math.fsum(keep), math.fsum(s)


def served_k():
    """{NT: every K = bnd + 1 that a rate from 15.8 to 192 kHz produces}, by api.hip's expressions (setup_d4c: fft_d4c, wl,
    band_bnd) and d4c_frame's call (bnd + 1)"""
    def make():
        out = {}
        for fs in range(15800, 192001):
            n = int(2.0 ** (1.0 + int(math.log(4.0 * fs / 47.0 + 1) / math.log(2.0))))
            wl = int(3000.0 * n / fs) * 2 + 1
            out.setdefault(n // 16, set()).add(int(n * 8.0 / wl + 0.5) + 1)
        return {nt: sorted(ks) for nt, ks in out.items()}
    return cached(("served K",), make)


def route_rule(row, K):
    """the documented rule on the high words of slots 0 .. 8: floor = the smallest of the threads' maxima, top = the largest
    key; 1024 linear bins of 2^s0 high words over [floor, top]; the K-th key from the top alone in its bin: one pass; else
    256 bins over that bin's range: two passes; anything else, NT < K or top == floor: the general routine"""
    hi = (np.ascontiguousarray(row).view(np.uint64) >> np.uint64(32)).astype(np.int64)[:, :9]
    nt = hi.shape[0]
    tmax = hi.max(axis=1)
    fl, tp = int(tmax.min()), int(tmax.max())
    if nt < K or tp == fl:
        return 2
    s0 = max((tp - fl).bit_length() - 10, 0)
    h = np.concatenate([hi[:, :8].ravel(), hi[:1, 8]])
    h = h[h >= fl]
    b = (h - fl) >> s0
    bin0 = int(np.sort(b)[::-1][K - 1])
    if int((b == bin0).sum()) == 1:
        return 0
    if s0 == 0:
        return 2
    s1 = max(s0 - 8, 0)
    d = (h[b == bin0] - (fl + (bin0 << s0))) >> s1
    bin1 = int(np.sort(d)[::-1][K - int((b > bin0).sum()) - 1])
    return 1 if int((d == bin1).sum()) == 1 else 2


# ---- lattice rows as relative bit patterns ----------------------------------------------------------------------------------
def realise(P, field):
    """relative patterns [.., NT, 10] (int64; 0 = 0.0) -> doubles whose smallest key has exponent field `field`"""
    P = np.asarray(P, dtype=np.int64)
    shift = field - int((P[P > 0] >> 52).min())
    return np.where(P > 0, P + (shift << 52), 0).astype(np.int64).view(np.float64)


def lattice_precondition(keys, field, b):
    """every key an integer multiple of 2^e, e = (field - 1023) - b, and every row's total / 2^e below 2^53"""
    e = field - 1023 - b
    m = np.ldexp(keys, -e)
    assert np.all(np.isfinite(keys)) and not np.any(np.signbit(keys)) and np.all(m == np.rint(m)) and np.all(m < 2.0 ** 53)
    totals = m.astype(np.int64).reshape(len(keys), -1).sum(axis=1)
    assert np.all(totals < 2 ** 53), "the lattice is too fine for exact sums"
    nz = keys[keys > 0]
    assert nz.size and nz.min() >= 2.0 ** (field - 1023) and nz.min() < 2.0 ** (field - 1022)


def low_word(rng, b):
    """a random low word on the lattice of b mantissa bits (b > 20)"""
    return int(rng.integers(0, 1 << (b - 20))) << (52 - b)


def key_of(h, lo=0):
    return (int(h) << 32) | int(lo)


def uppers_one_pass(nt, K, rng, b):
    """descending patterns: fine bins of their own 1024 high words apart, random ranks moved into the bin below -- never
    the top, the floor, rank K or into rank K's bin"""
    M = min(nt + nt // 2, 1024)
    off = [j << 10 for j in range(M - 1, -1, -1)]
    for r in range(2, M - 1):                                  # rank r (1-based) joins rank r + 1
        if r != K and r + 1 != K and rng.random() < 0.3:
            off[r - 1] = ((M - 1 - r) << 10) + 1
    return [key_of(FL + o, low_word(rng, b)) for o in off]


def uppers_two_pass(nt, K, rng, b, s0):
    """one outlier at 2^(10 + s0) - 1 above the floor; the others 2^s1 apart from the floor up, whole fine bins of them"""
    per_bin = min(1 << s0, 256)
    regular = per_bin * ((nt + per_bin - 1) // per_bin)
    u = 1 << max(s0 - 8, 0)
    off = [(1 << (10 + s0)) - 1] + [j * u for j in range(regular - 1, -1, -1)]
    assert off[1] < off[0]
    return [key_of(FL + o, low_word(rng, b)) for o in off]


def uppers_flat(nt, K, rng, b):
    """consecutive high words: s0 = 0"""
    M = min(nt + nt // 2, 1024)
    return [key_of(FL + o, low_word(rng, b)) for o in range(M - 1, -1, -1)]


def uppers_one_word(nt, K, rng, b):
    """every upper in the floor's high word, distinct low words: tp == fl"""
    M = nt + nt // 2
    los = sorted((int(v) for v in rng.choice(1 << (b - 20), size=M, replace=False)), reverse=True)
    return [key_of(FL, lo << (52 - b)) for lo in los]


def with_pair(D, K, b):
    """ranks K and K + 1 (K - 1 and K where K + 1 is the floor) share a high word and differ by the lattice's lowest bit"""
    D = list(D)
    i = K - 1 if K < len(D) - 1 else K - 2                    # D[i], D[i + 1]: the pair, neither the top nor the floor
    assert 1 <= i and i + 1 < len(D) - 1
    unit = 1 << (52 - b)
    hi, lo = D[i] >> 32, max(D[i] & 0xFFFFFFFF, unit)
    D[i], D[i + 1] = key_of(hi, lo), key_of(hi, lo - unit)
    return D


def with_ties(D, K, g, a):
    """g equal keys of which the a largest ranks are excluded: ranks K - a + 1 .. K - a + g"""
    D = list(D)
    first = K - a
    assert 1 <= first and first + g - 1 < len(D) - 1
    for j in range(1, g):
        D[first + j] = D[first]
    return D


def place_row(nt, D, rng, b, place=None, slot8_zero=False):
    """-> patterns [NT][10]: D (descending uppers) one to a thread first -- rank r at place[r] = (thread, slot) where given, the
    lowest alone in its thread, which makes it the floor -- the others in free owned slots; every other owned slot (0 .. 7,
    thread 0's slot 8 unless slot8_zero) holds a random key below the floor; slot 9 and the other threads' slot 8 hold 0"""
    place = dict(place or {})
    M = len(D)
    assert M >= nt
    row = np.zeros((nt, SLOTS), dtype=np.int64)
    has = np.zeros(nt, dtype=bool)
    for r, (t, s) in place.items():
        assert row[t, s] == 0 and (s < 8 or (s == 8 and t == 0))
        row[t, s] = D[r - 1]
        has[t] = True
    if M in place:
        tf = place[M][0]
        assert sum(1 for t, _ in place.values() if t == tf) == 1
    else:
        tf = int(rng.choice(np.nonzero(~has)[0]))
        row[tf, int(rng.integers(0, 8))] = D[M - 1]
        has[tf] = True
    rest = [D[r - 1] for r in range(1, M) if r not in place]
    order = rng.permutation(len(rest))
    rest = [rest[i] for i in order]
    for t in np.nonzero(~has)[0]:
        row[t, int(rng.integers(0, 8))] = rest.pop()
    open_ = row == 0
    open_[:, 9] = open_[tf] = False
    open_[1:, 8] = False
    open_[0, 8] &= not slot8_zero
    free = np.argwhere(open_)
    assert len(free) >= len(rest)
    for t, s in free[rng.permutation(len(free))[:len(rest)]]:
        row[t, s] = rest.pop()
    small = (rng.integers(1 << 20, FL, size=(nt, SLOTS)) << 32) | (rng.integers(0, 1 << (b - 20), size=(nt, SLOTS)) << (52 - b))
    fill = row == 0
    fill[:, 9] = False
    fill[1:, 8] = False
    fill[0, 8] &= not slot8_zero
    return np.where(fill, small, row)


class Batch:
    """rows of one launch: relative patterns [rows][NT][10], the K, the route each row must take, the lattice's depth b"""

    def __init__(self, name, K, rows, routes, b):
        self.name, self.K, self.P, self.routes, self.b = name, K, np.stack(rows), np.array(routes, dtype=np.float64), b


def ks_of(nt):
    """the ends of the served range and, while a row is cheap on the emulator, one value inside it"""
    ks = served_k()[nt]
    return (ks[0], ks[len(ks) // 2], ks[-1]) if nt <= 256 else (ks[0], ks[-1])


def batches_routes(nt):
    """required cases 1 .. 3: the three routes and the four entries of the general routine, at the served K of ks_of()"""
    def make():
        rng = np.random.default_rng(1000 + nt)
        out, b = [], 28
        for K in ks_of(nt):
            rows = [place_row(nt, uppers_one_pass(nt, K, rng, b), rng, b) for _ in range(3)]
            out.append(Batch(f"one pass K{K}", K, rows, [0] * 3, b))
            for s0 in (3, 8, 10):
                rows = [place_row(nt, uppers_two_pass(nt, K, rng, b, s0), rng, b) for _ in range(2)]
                out.append(Batch(f"two passes s0={s0} K{K}", K, rows, [1] * 2, b))
            rows = [place_row(nt, uppers_one_word(nt, K, rng, 34), rng, 34) for _ in range(2)]
            out.append(Batch(f"general tp == fl K{K}", K, rows, [2] * 2, 34))
            rows = [place_row(nt, with_pair(uppers_flat(nt, K, rng, b), K, b), rng, b) for _ in range(2)]
            out.append(Batch(f"general s0 == 0 pair K{K}", K, rows, [2] * 2, b))
            rows = [place_row(nt, with_pair(uppers_two_pass(nt, K, rng, b, s0), K, b), rng, b) for s0 in (3, 8, 10)]
            out.append(Batch(f"general pair after the second pass K{K}", K, rows, [2] * 3, b))
        K = nt + 1
        rows = [place_row(nt, uppers_one_pass(nt, K, rng, b), rng, b), place_row(nt, uppers_two_pass(nt, K, rng, b, 8), rng, b),
                place_row(nt, uppers_flat(nt, K, rng, b), rng, b)]
        out.append(Batch(f"general threads < K K{K}", K, rows, [2] * 3, b))
        return out
    return cached(("select routes", nt), make)


TIES = ((2, 1), (3, 1), (3, 2), (5, 2), (7, 3), (4, 4))          # (equal keys, how many of them are excluded)


def batches_general(nt):
    """required case 4: inside the general routine"""
    def make():
        rng = np.random.default_rng(2000 + nt)
        out = []
        ks = served_k()[nt]
        # every slot in one high word, low words varied, no slot 0: thread 0 ten keys; the others ten, or nine (slot 8 at 0)
        b = 34
        for tag, nine in (("ten slots", False), ("nine slots", True)):
            rows = []
            for _ in range(2 if nt <= 256 else 1):
                lo = rng.integers(0, 1 << (b - 20), size=(nt, SLOTS)).astype(np.int64) << (52 - b)
                row = (np.int64(FL) << 32) | lo
                if nine:
                    row[1:, 8] = 0
                rows.append(row)
            for K in (ks[0], nt, nt + 1):                       # nt >= K + 1: the floor stands for the minimum; otherwise the true minimum
                out.append(Batch(f"one high word, {tag} K{K}", K, rows, [2] * len(rows), b))
        # more than kSelHists passes: with padding in the row the digits start at the top key's leading bit (bit 54 .. 62 with
        # the scale), the uppers share their high word and the threshold pair everything down to the lattice's last bit, 18
        K = ks[-1]
        rows = [place_row(nt, with_pair(uppers_one_word(nt, K, rng, b), K, b), rng, b) for _ in range(2)]
        out.append(Batch(f"five or six passes K{K}", K, rows, [2] * 2, b))
        # exact ties across the threshold, on the uppers of every design in turn (rank K is one of the g equal keys in every
        # pair of TIES: its bin never holds one key)
        designs = (uppers_flat, uppers_one_word, lambda *args: uppers_two_pass(*args, 8), uppers_one_pass)
        for i, K in enumerate((ks[0], ks[-1])):
            rows = [place_row(nt, with_ties(designs[(i + j) % 4](nt, K, rng, b), K, g, a), rng, b) for j, (g, a) in enumerate(TIES)]
            if nt <= 256:
                rows += [place_row(nt, with_ties(designs[(i + j + 2) % 4](nt, K, rng, b), K, g, a), rng, b) for j, (g, a) in enumerate(TIES)]
            out.append(Batch(f"ties K{K}", K, rows, [2] * len(rows), b))
        # all real keys equal
        row = np.zeros((nt, SLOTS), dtype=np.int64)
        row[:, :8] = key_of(FL + 77, 5 << 24)
        row[0, 8] = row[0, 0]
        for K in (1, ks[0], nt + 1, 8 * nt + 1, 10 * nt):
            out.append(Batch(f"all equal K{K}", K, [row], [2], b))
        return out
    return cached(("select general", nt), make)


def positions(nt):
    """required case 5: (thread, slot) of the threshold (rank K) and of the top key"""
    last = nt - 1
    out = [dict(thr=(5, s), top=(nt // 2 + 3, (s + 3) % 8)) for s in range(8)]                    # each owned slot, both keys
    out += [dict(thr=(0, 8), top=(63, 5)), dict(thr=(63, 5), top=(0, 8)),                          # thread 0's slot 8; lane 63 of the first wavefront
            dict(thr=(64, 2), top=(last, 6)), dict(thr=(last, 6), top=(64, 2)),                    # lane 0; the last thread (lane 63 of the last wavefront)
            dict(thr=(nt - 64, 3), top=(17, 0)), dict(thr=(17, 0), top=(nt - 64, 3)),              # lane 0 of the last wavefront; the first wavefront
            dict(thr=(0, 0), top=(nt - 40, 7), slot8_zero=True)]                                   # slot 8 = 0, the padding value
    return out


def batches_positions(nt):
    def make():
        rng = np.random.default_rng(3000 + nt)
        b, K = 28, served_k()[nt][-1]
        out = []
        for name, uppers, route in (("one pass", uppers_one_pass, 0), ("two passes", lambda *a: uppers_two_pass(*a, 8), 1),
                                    ("general", lambda *a: with_pair(uppers_flat(*a), K, b), 2)):
            rows = [place_row(nt, uppers(nt, K, rng, b), rng, b, place={K: p["thr"], 1: p["top"]}, slot8_zero=p.get("slot8_zero", False))
                    for p in positions(nt)]
            out.append(Batch(f"positions, {name} K{K}", K, rows, [route] * len(rows), b))
        return out
    return cached(("select positions", nt), make)


def batches_k(nt):
    """required case 6: K = 1, K = NT and every served K: a one-pass and a two-pass row each at 128 and 256 threads, the two
    in turn where a row costs more on the emulator; the scales taken in turn"""
    def make():
        rng = np.random.default_rng(4000 + nt)
        b, out = 28, []
        for i, K in enumerate([1, 1, nt, nt] + served_k()[nt]):
            rows = [place_row(nt, uppers_one_pass(nt, K, rng, b), rng, b), place_row(nt, uppers_two_pass(nt, K, rng, b, (3, 8, 10)[K % 3]), rng, b)]
            routes = [0, 1 if K > 1 else 0]                                                         # (K = 1 is the outlier itself, alone in its bin)
            if nt > 256:
                rows, routes = rows[i % 2:i % 2 + 1], routes[i % 2:i % 2 + 1]
            out.append(Batch(f"K{K}", K, rows, routes, b))
        return out
    return cached(("select K", nt), make)


# ---- real-valued rows -----------------------------------------------------------------------------------------------------
def nuttall(n):
    t = np.arange(n) / (n - 1.0)
    return 0.355768 - 0.487396 * np.cos(2 * np.pi * t) + 0.144232 * np.cos(4 * np.pi * t) - 0.012604 * np.cos(6 * np.pi * t)


def owned(nt, bins):
    """bins [8 NT + 1] -> [NT][10] in d4c_frame's ownership: item m of thread t is bin t + m NT and, below N / 4, bin N / 2 - that"""
    q = 4 * nt
    row = np.zeros((nt, SLOTS))
    t = np.arange(nt)
    for m in range(4):
        row[:, 2 * m] = bins[t + m * nt]
        row[:, 2 * m + 1] = bins[2 * q - (t + m * nt)]
    row[0, 8] = bins[q]
    return row


def real_rows(nt):
    """[(name, K, rows [r][NT][10])]: spectra at the two ends of the shape's rates, log-uniform draws"""
    def make():
        rng = np.random.default_rng(5000 + nt)
        ks = served_k()[nt]
        n = 16 * nt
        out = []
        for K in (ks[0], ks[-1]):
            wl = int(round(8.0 * n / (K - 1))) | 1                       # (K - 1 = mround(8 N / wl), wl odd)
            rows = []
            for _ in range(3):
                x = np.zeros(n)
                x[:wl] = rng.standard_normal(wl) * nuttall(wl) * 10.0 ** rng.uniform(-6, -2)
                rows.append(owned(nt, 4.0 * np.abs(np.fft.rfft(x)) ** 2))
            out.append((f"spectra K{K}", K, np.stack(rows)))
            rows = []
            for _ in range(3):
                row = np.zeros((nt, SLOTS))
                row[:, :8] = 10.0 ** rng.uniform(-9, 3, (nt, 8))
                row[0, 8] = 10.0 ** rng.uniform(-9, 3)
                rows.append(row)
            out.append((f"log-uniform K{K}", K, np.stack(rows)))
        return out
    return cached(("select real", nt), make)


# ---- the backend ------------------------------------------------------------------------------------------------------------
class Backend(backends.Backend):
    """world_hip_probe_select on the arrays of backends.Backend"""

    def call(self, mode, threads, K, rows, keys_ptr, out_ptr):
        """the C call itself on addresses (None: NULL)"""
        return self.lib.world_hip_probe_select(self.ctx, mode, threads, K, rows, None if keys_ptr is None else C.c_void_p(keys_ptr),
                                               None if out_ptr is None else C.c_void_p(out_ptr))

    def run(self, mode, keys, K):
        """keys [rows][NT][10] -> out [rows][3]; two more output rows keep SENTINEL, and the keys stay what they were"""
        keys = np.ascontiguousarray(keys, dtype=np.float64)
        rows, nt, slots = keys.shape
        assert slots == SLOTS
        d_keys, d_out = self.dev(keys), self.dev(np.full((rows + 2, 3), SENTINEL))
        rc = self.call(mode, nt, K, rows, self.addr(d_keys), self.addr(d_out))
        assert rc == 0, self.error()
        out = self.host(d_out)
        assert np.all(out[rows:] == SENTINEL), "written beyond the rows"
        assert same_bits(self.host(d_keys), keys), "the keys were written"
        return out[:rows].copy()


be = cpu_backend(Backend)


# ---- the cases --------------------------------------------------------------------------------------------------------------
def lattice_reference(batch, scale):
    """(keys, [rows][2] by the statement) of a batch at a scale: computed once, shared, never changed"""
    def make():
        keys = realise(batch.P, SCALES[scale])
        lattice_precondition(keys, SCALES[scale], batch.b)
        for row, route in zip(keys, batch.routes):
            assert route_rule(row, batch.K) == route, f"{batch.name}: the row is not built for route {route}"
        return keys, np.array([statement(row, batch.K) for row in keys])
    return cached(("select reference", id(batch), scale), make)


def check_lattice(be, batch, scales=tuple(SCALES)):
    routes = {}
    for scale in scales:
        keys, want = lattice_reference(batch, scale)
        got = be.run(0, keys, batch.K)
        direct = be.run(1, keys, batch.K)
        for r in range(len(keys)):
            what = f"NT {keys.shape[1]}, {batch.name}, row {r}, scale {scale}"
            assert got[r, 2] == batch.routes[r], f"{what}: route {got[r, 2]:.0f}, the case names {batch.routes[r]:.0f}"
            assert same_bits(got[r, :2], want[r]), f"{what}: {got[r, :2]} for {want[r]} ({(got[r, :2] - want[r]) / want[r, 1]} of the total)"
            assert direct[r, 2] == 2 and same_bits(direct[r, :2], want[r]), f"{what}, mode 1: {direct[r]} for {want[r]}"
        routes[scale] = got[:, 2]
    assert all(np.array_equal(v, batch.routes) for v in routes.values())


def case_routes(be, nt):
    for batch in batches_routes(nt):
        check_lattice(be, batch)


def case_general(be, nt):
    for batch in batches_general(nt):
        check_lattice(be, batch)


def case_positions(be, nt):
    for batch in batches_positions(nt):
        check_lattice(be, batch)


def case_every_k(be, nt):
    ks = served_k()
    assert (ks[128][0], ks[128][-1], ks[256][-1], ks[512][-1], ks[1024][0], ks[1024][-1]) == (22, 33, 65, 129, 129, 257)
    assert all(ks[n] == list(range(ks[n][0], ks[n][-1] + 1)) for n in NTS)
    for i, batch in enumerate(batches_k(nt)):
        check_lattice(be, batch, scales=(list(SCALES)[i % len(SCALES)],))


def case_real(be, nt):
    for name, K, rows in real_rows(nt):
        got, direct = be.run(0, rows, K), be.run(1, rows, K)
        for r, row in enumerate(rows):
            assert np.all(np.isfinite(row)) and not np.any(np.signbit(row))
            partial, total = statement(row, K, exact=True)
            n = int(np.count_nonzero(row))
            bound_p, bound_t = (n - K - 1) * Fraction(U) * partial, (n - 1) * Fraction(U) * total
            s = np.sort(row.ravel())
            gap = Fraction(float(s[-K])) - Fraction(float(s[-K - 1]))
            assert gap > 4 * bound_p, f"{name}, row {r}: the threshold gap {float(gap):.3e} could hide in the bound {float(bound_p):.3e}"
            route = route_rule(row, K)
            what = f"NT {nt}, {name}, row {r} (route {route})"
            assert got[r, 2] == route, f"{what}: route {got[r, 2]:.0f}"
            for out, mode in ((got[r], 0), (direct[r], 1)):
                ep, et = abs(Fraction(float(out[0])) - partial), abs(Fraction(float(out[1])) - total)
                print(f"{what}, mode {mode}: partial error / bound {float(ep / bound_p):.4f}, total {float(et / bound_t):.4f}")
                assert ep <= bound_p and et <= bound_t, what
            assert direct[r, 2] == 2


def case_rows_are_independent(be, nt):
    """a row alone, inside a batch and inside the permuted batch: the same bits"""
    K = served_k()[nt][-1]
    picked = [b for b in batches_routes(nt) + batches_general(nt) + batches_positions(nt) if b.K == K]
    P = np.concatenate([b.P[:2] for b in picked])
    routes = np.concatenate([b.routes[:2] for b in picked])
    assert set(routes) == {0.0, 1.0, 2.0}
    keys = realise(P, SCALES["2^-80"])
    perm = np.random.default_rng(nt).permutation(len(keys))
    for mode in (0, 1):
        whole = be.run(mode, keys, K)
        assert mode == 1 or np.array_equal(whole[:, 2], routes)
        assert same_bits(be.run(mode, keys[perm], K), whole[perm])
        for r in (0, len(keys) // 2, len(keys) - 1):
            assert same_bits(be.run(mode, keys[r:r + 1], K), whole[r:r + 1])


def case_refusals(be):
    """every refusal of the header: an error whose reason names the argument, and nothing written"""
    nt, K = 128, 22
    keys = realise(batches_routes(nt)[0].P[:2], SCALES["2^0"])
    d_keys, d_out = be.dev(keys), be.dev(np.full((2, 3), SENTINEL))
    ok = dict(mode=0, threads=nt, K=K, rows=2, keys_ptr=be.addr(d_keys), out_ptr=be.addr(d_out))
    assert be.call(**dict(ok, rows=0)) == 0 and np.all(be.host(d_out) == SENTINEL)          # no rows: nothing to do

    def refused(word, **change):
        assert be.call(**dict(ok, **change)) == 1, change
        assert word in be.error() and "probe_select" in be.error(), (change, be.error())
        assert np.all(be.host(d_out) == SENTINEL) and same_bits(be.host(d_keys), keys), change

    for bad in (0, 64, 192, 127, 129, 2048, -128):
        refused("threads", threads=bad)
    for bad in (0, -1, 10 * nt + 1):
        refused("K", K=bad)
    refused("K", K=10 * 128 + 1, threads=128)
    refused("mode", mode=2)
    refused("mode", mode=-1)
    refused("rows", rows=-1)
    refused("keys", keys_ptr=None)
    refused("out", out_ptr=None)
    assert be.call(**dict(ok, K=10 * nt)) == 0                                               # the largest K: everything excluded
    out = be.host(d_out)
    assert np.all(out[:, 0] == 0.0) and np.all(out[:, 1] > 0) and np.all(out[:, 2] == 2)


# ---- on the emulator ----------------------------------------------------------------------------------------------------------
def test_the_route_rule_on_rows_built_by_hand():
    """the rule itself, before anything is held to it: eight threads' worth of reasoning fits on a page"""
    nt = 128
    row = np.zeros((nt, SLOTS), dtype=np.int64)
    row[:, 0] = [key_of(FL + (t << 10)) for t in range(nt)]             # distinct bins: s0 = 7, bins 8 apart
    k = realise(row, 1023)
    assert route_rule(k, 5) == 0 and route_rule(k, nt) == 0 and route_rule(k, nt + 1) == 2
    row[7, 1] = row[9, 0] + (1 << 32)                                   # a second key in thread 9's bin
    k = realise(row, 1023)
    assert route_rule(k, nt - 9) == 1 and route_rule(k, nt - 8) == 1 and route_rule(k, nt - 10) == 0
    row[7, 1] = row[9, 0] + 1                                           # ... in its high word
    k = realise(row, 1023)
    assert route_rule(k, nt - 9) == 2 and route_rule(k, nt - 10) == 0
    row[7, 1] = 0
    row[:, 0] = key_of(FL, 3)
    assert route_rule(realise(row, 1023), 5) == 2                       # one high word


@pytest.mark.parametrize("nt", NTS)
def test_every_route_and_every_entry_of_the_general_routine(be, nt):
    case_routes(be, nt)


@pytest.mark.parametrize("nt", NTS)
def test_inside_the_general_routine(be, nt):
    case_general(be, nt)


@pytest.mark.parametrize("nt", NTS)
def test_where_the_threshold_and_the_top_key_live(be, nt):
    case_positions(be, nt)


@pytest.mark.parametrize("nt", NTS)
def test_every_served_k(be, nt):
    case_every_k(be, nt)


@pytest.mark.parametrize("nt", NTS)
def test_real_valued_rows_within_the_any_order_bound(be, nt):
    case_real(be, nt)


@pytest.mark.parametrize("nt", NTS)
def test_a_row_depends_on_nothing_but_the_row(be, nt):
    case_rows_are_independent(be, nt)


def test_refusals_write_nothing_and_name_the_argument(be):
    case_refusals(be)
