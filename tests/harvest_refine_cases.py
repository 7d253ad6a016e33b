"""Harvest's refinement stage alone (include/world_hip.h: world_hip_probe_harvest_refine -- hv_refine or hv_refine_frames on a
decimated signal and a candidate map the caller made up): the cases tests/test_harvest_refine_cpu.py runs on the host emulation
and tests/test_harvest_refine_gpu.py on the card, as functions of a backend.

The comparators.  R = the reference's own OverlapF0Candidates and RefineF0Candidates (oracle/_ref/libworld_ref_refine.so:
oracle/harvest_refine_ref.cpp includes the reference's harvest.cpp where it lies), recorded in tests/golden/harvest_refine.npz
(tests/golden/make_golden_harvest_refine.py); where both are present they agree bit for bit.  W = wo_harvest_refine of the WIDE
oracle: the reference's discrete path in double, every value in long double.  P = the same function of the double oracle, a
third statement: identical gates and 1e-10 relative to R.  expected() asserts all of that, then the case's reach.

The kernels do not compute what the reference computes (Goertzel recurrences against two FFTs; table or rotated windows;
DPP sums), so nothing here is bit for bit against R.  What is asserted of the code under test, H:
  gates      written 0 / non-0 per slot: H == R everywhere; W alone may differ on max(2, n / 50) slots (util.discrete_agreement)
  accuracy   refined F0 and score of the slots all three wrote, against W: util.assert_accurate (A = 4, c = 64 ulp, at the
             median, the 99th percentile and the maximum, R's own error the yardstick), over the slots of a GROUP and route --
             a quantile needs a sample, and the utterances here have a few dozen slots each
  footprint  outputs pre-filled with NaN: slots below 7 nc[u] of frames below nfb[u] hold numbers, everything else is still
             NaN; the parts of y and cand nobody may read hold values that would change the results
  identities route 1 == route 2 bit for bit wherever there is a table; a batch is its lone calls

Every utterance states what it was built to reach and expected() asserts it on the host from W's per-slot report (hw, first,
lgN, nh, the six idx, the gate) and from walk(), the kernel's cache rule restated: a case that stops reaching its branch fails.
Every non-empty slot of every case is also asserted to sit at least 1e-9 (relative) away from each of the gate's three
thresholds in W: no rounding-level ties, which nobody can hold.

Two things the window arithmetic makes impossible are not cases: blen = 2 hw + 1 is odd, so blen mod 8 is 1, 3, 5 or 7 and
blen is never a multiple of 32 (the cases stand at 31 | 33 and 63 | 65)."""
import collections
import ctypes as C
import math
import os

import numpy as np

import backends
import util
from backends import cached, same_bits
from oracle import loader as L

GOLDEN = os.path.join(util.GOLDEN, "harvest_refine.npz")
ORDER = (3, 2, 1, 0, 4, 5, 6)          # hv_refine_frames visits a track's slots in time order: frames f-3 .. f+3
UNREAD = 123.0                         # what the parts of cand nobody may read hold: a valid candidate, so a read would show
MARGIN = 1e-9


def hw_of(afs, f0):
    return int(1.5 * afs / f0 + 1.0)


def harmonic(afs, n, f0, seed, noise=1e-3, amps=(1.0, 0.6, 0.45, 0.3, 0.2, 0.15), start=0):
    """a harmonic sum at f0 (the partials up to the Nyquist frequency) with a little noise"""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + start) / afs
    y = noise * rng.standard_normal(n)
    for h, a in enumerate(amps):
        if f0 * (h + 1) <= afs / 2:
            y += a * np.sin(2 * np.pi * f0 * (h + 1) * t + 0.7 * h + 0.3)
    return y


def track(nf, f0, seed=0, jitter=0.0):
    rng = np.random.default_rng(seed)
    return f0 * (1.0 + jitter * rng.uniform(-1, 1, nf))


class U:
    """one utterance: the signal, the map cand [nf, nc], the rate and the gate's limits, and what it must reach"""

    def __init__(self, name, y, cand, afs=8000.0, f0_floor=40.0, f0_ceil=800.0, reach=None):
        self.name, self.afs, self.f0_floor, self.f0_ceil, self.reach = name, float(afs), float(f0_floor), float(f0_ceil), reach
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        cand = np.asarray(cand, dtype=np.float64)
        self.cand = np.ascontiguousarray(cand if cand.ndim == 2 else cand[:, None])
        self.nf, self.nc = self.cand.shape
        self.y.setflags(write=False)
        self.cand.setflags(write=False)

    @property
    def args(self):
        return dict(afs=self.afs, f0_floor=self.f0_floor, f0_ceil=self.f0_ceil)

    @property
    def table(self):
        return math.fmod(self.afs, 1000.0) == 0.0

    @property
    def routes(self):
        return (1, 2, 3) if self.table else (3,)


class Group:
    def __init__(self, name, utts, values=True, batch=False, maxc=None):
        self.name, self.utts, self.values, self.batch, self.maxc = name, utts, values, batch, maxc
        assert len({u.name for u in utts}) == len(utts)
        assert not batch or len({(u.afs, u.f0_floor, u.f0_ceil) for u in utts}) == 1

    @property
    def routes(self):
        return (1, 2, 3) if all(u.table for u in self.utts) else (3,)


# ---- the kernel's cache rule, restated -------------------------------------------------------------------------------------
def walk(report, nc):
    """hv_refine_frames keeps the window (hw, first) and, per harmonic, the bin of the slot it visited last -- across the slots
    of a track AND from a track into the next -- and reuses what is equal.  -> a Counter of what the visits of a map find:
    'rebuild', 'full' (window and every bin), 'partial' (window, some bins), 'window' (window, no bin), and the same with
    ' carried' (the first visit of a track j > 0) or ' over empty' (an empty slot lay between)"""
    ev = collections.Counter()
    for f in range(report.shape[0]):
        held = None
        for j in range(nc):
            visited, skipped = 0, False
            for m in ORDER:
                rep = report[f, j + nc * m]
                if rep[L.HR_GATE] == L.HR_EMPTY:
                    skipped = visited > 0
                    continue
                nh = rep[L.HR_NH]
                idx = tuple(int(rep[L.HR_IDX + h]) if h < nh else -1 for h in range(6))
                key = (int(rep[L.HR_HW]), int(rep[L.HR_FIRST]))
                if held and held[0] == key:
                    same = sum(1 for h in range(nh) if idx[h] == held[1][h])
                    kind = "full" if same == nh else "partial" if same else "window"
                    ev[kind] += 1
                    if visited == 0 and j > 0:
                        ev[kind + " carried"] += 1
                    if skipped:
                        ev[kind + " over empty"] += 1
                else:
                    ev["rebuild"] += 1
                held, visited, skipped = (key, idx), visited + 1, False
    return ev


def slots(w):
    """the reports of the non-empty slots [n, HR_WIDTH]"""
    rep = w["report"].reshape(-1, L.HR_WIDTH)
    return rep[rep[:, L.HR_GATE] != L.HR_EMPTY]


def residual(u, w):
    """r = first + hw - pos afs of every non-empty slot: what the rotation route turns a window by (0 on the table route)"""
    pos = (np.arange(u.nf) * 1.0 / 1000.0)[:, None] * u.afs
    rep = w["report"]
    r = rep[:, :, L.HR_FIRST] + rep[:, :, L.HR_HW] - pos
    return r[rep[:, :, L.HR_GATE] != L.HR_EMPTY]


def reaches(**want):
    """a reach function from conditions on the report: hw, blen, lgn, nh (sets that must ALL occur), gate (likewise),
    walk (kinds that must occur), and fn(u, w) for the rest"""
    def reach(u, w):
        s = slots(w)
        seen = dict(hw=set(s[:, L.HR_HW].tolist()), blen=set((2 * s[:, L.HR_HW] + 1).tolist()), lgn=set(s[:, L.HR_LGN].tolist()),
                    nh=set(s[:, L.HR_NH].tolist()), gate=set(s[:, L.HR_GATE].tolist()))
        for k in ("hw", "blen", "lgn", "nh", "gate"):
            if k in want:
                assert set(want[k]) <= seen[k], f"{u.name}: {k} {sorted(set(want[k]) - seen[k])} not reached (seen {sorted(seen[k])})"
        if "only_gate" in want:
            assert seen["gate"] == set(want["only_gate"]), f"{u.name}: gates {sorted(seen['gate'])}"
        if "walk" in want:
            ev = walk(w["report"], u.nc)
            for kind in want["walk"]:
                assert ev[kind] > 0, f"{u.name}: the walk never finds '{kind}' ({dict(ev)})"
        if "never" in want:
            ev = walk(w["report"], u.nc)
            for kind in want["never"]:
                assert ev[kind] == 0, f"{u.name}: the walk finds '{kind}' ({dict(ev)})"
        if "fn" in want:
            want["fn"](u, w)
    return reach


# ---- the comparators -------------------------------------------------------------------------------------------------------
def oracles():
    def make():
        return L.PortOracle(), L.WideOracle(), (L.RefRefine() if L.RefRefine.available() else None)
    return cached(("harvest refine oracles",), make)


def golden():
    return cached(("harvest refine golden",), lambda: dict(np.load(GOLDEN)))


def expected(group, u):
    """-> (r, w): R's refined and score [nf, 7 nc] and W's dict, after R == golden, P against R, the margins and the reach"""
    def make():
        port, wide, ref = oracles()
        what = f"{group.name}/{u.name}"
        g = golden()
        r = dict(refined=g[f"{what}/refined"], score=g[f"{what}/score"])
        assert r["refined"].shape == r["score"].shape == (u.nf, 7 * u.nc), f"{what}: the recorded shapes"
        if ref is not None:
            now = ref.harvest_refine(u.y, u.cand, **u.args)
            for k in ("refined", "score"):
                assert same_bits(now[k], r[k]), f"{what}: the reference's {k} is not the recorded one"
        w, p = wide.harvest_refine(u.y, u.cand, **u.args), port.harvest_refine(u.y, u.cand, **u.args)
        assert L.wide_is_wider(), "long double is no wider than double here: W is no yardstick"
        # the double oracle, a third statement: R's gates, 1e-10 relative (the project's Harvest tolerance)
        for k in ("refined", "score"):
            assert np.array_equal(p[k] != 0, r[k] != 0), f"{what}: the double oracle's gates are not the reference's ({k})"
            m = r[k] != 0
            assert util.max_rel(p[k][m], r[k][m]) <= 1e-10 if m.any() else True, f"{what}: the double oracle's {k} against the reference"
        assert np.array_equal(r["refined"] != 0, r["score"] != 0), what
        # the candidates' layout (OverlapF0Candidates): slot j + nc m is candidate j of frame f - m or f + m - 3
        empty = w["report"][:, :, L.HR_GATE] == L.HR_EMPTY
        for m in range(7):
            d = -m if m <= 3 else m - 3
            for f in range(u.nf):
                src = u.cand[f + d] if 0 <= f + d < u.nf else np.zeros(u.nc)
                assert np.array_equal(empty[f, m * u.nc:(m + 1) * u.nc], src == 0), f"{what}: slot layout, frame {f} m {m}"
        # no slot near a threshold: the gates can be held
        raw, live = w["raw"].reshape(-1, 2), ~empty.reshape(-1)
        if live.any():
            f0, sc = raw[live, 0], raw[live, 1]
            near = np.minimum(np.minimum(np.abs(f0 - u.f0_floor) / u.f0_floor, np.abs(f0 - u.f0_ceil) / u.f0_ceil), np.abs(sc - 2.5) / 2.5)
            assert near.min() >= MARGIN, f"{what}: a slot lies {near.min():.2e} (relative) from a threshold of the gate"
        n_differ = int(np.count_nonzero((w["refined"] != 0) != (r["refined"] != 0)))
        assert n_differ == 0, f"{what}: W and R gate {n_differ} slots differently although none is near a threshold"
        if u.reach:
            u.reach(u, w)
        for a in (r["refined"], r["score"], w["refined"], w["score"], w["report"], w["raw"]):
            a.setflags(write=False)
        return r, w
    return cached(("harvest refine expected", group.name, u.name), make)


# ---- the backend -----------------------------------------------------------------------------------------------------------
class Backend(backends.Backend):
    def call(self, utts, route, maxc=None, override=None):
        """the probe on utterances of one rate and gate -> (return code, the device arrays by name, the host copies of the
        inputs); `override` replaces arguments of the C call (refusals)"""
        n = len(utts)
        nfb, nc, y_len = [u.nf for u in utts], [u.nc for u in utts], [len(u.y) for u in utts]
        stride, y_stride = (max(nfb) + 7) & ~7, (max(y_len) + 7) & ~7
        maxc = maxc or 7 * max(1, max(nc))
        y, cand = np.full((n, y_stride), np.nan), np.full((n, stride, maxc), UNREAD)
        for i, u in enumerate(utts):
            y[i, :len(u.y)] = u.y
            cand[i, :u.nf, :u.nc] = u.cand
        keep = dict(y=y, cand=cand)
        d = {k: self.dev(v) for k, v in keep.items()}
        d["refined"], d["score"] = self.dev(np.full((n, stride, maxc), np.nan)), self.dev(np.full((n, stride, maxc), np.nan))
        ints = lambda v: (C.c_int * n)(*v)
        a = dict(n_utt=n, y_len=ints(y_len), nfb=ints(nfb), nc=ints(nc), afs=utts[0].afs, f0_floor=utts[0].f0_floor,
                 f0_ceil=utts[0].f0_ceil, maxc=maxc, fb_stride=stride, y_stride=y_stride, route=route)
        a.update({k: self.ptr(d[k]) for k in ("y", "cand", "refined", "score")})
        a.update(override or {})
        rc = self.lib.world_hip_probe_harvest_refine(self.ctx, *(a[k] for k in (
            "n_utt", "y_len", "nfb", "nc", "afs", "f0_floor", "f0_ceil", "maxc", "fb_stride", "y_stride", "route", "y", "cand", "refined", "score")))
        return rc, d, keep

    def run(self, utts, route, maxc=None):
        """-> per utterance dict(refined, score [nf, 7 nc]), after the footprint: numbers in the slots the stage owns, NaN
        everywhere else, the inputs as they were"""
        rc, d, keep = self.call(utts, route, maxc)
        assert rc == 0, self.error()
        h = {k: self.host(v) for k, v in d.items()}
        for k, v in keep.items():
            assert same_bits(h[k], v), f"the probe wrote into {k}"
        out = []
        for i, u in enumerate(utts):
            o = {}
            for k in ("refined", "score"):
                own = np.zeros(h[k].shape[1:], dtype=bool)
                own[:u.nf, :7 * u.nc] = True
                assert np.isfinite(h[k][i][own]).all(), f"{u.name} route {route}: {k} has slots the stage owns and did not write"
                assert np.isnan(h[k][i][~own]).all(), f"{u.name} route {route}: {k} written outside frames < nfb, slots < 7 nc"
                o[k] = np.array(h[k][i, :u.nf, :7 * u.nc])
            out.append(o)
        return out


def hold(be, group, route, outs, what, keys):
    """gates and accuracy of a group's outputs on one route against R and W, pooled over its utterances"""
    hs, rs, ws = ({k: [] for k in keys} for _ in range(3))
    for u, o in zip(group.utts, outs):
        r, w = expected(group, u)
        for k in keys:
            hs[k].append(o[k].ravel()), rs[k].append(r[k].ravel()), ws[k].append(w[k].ravel())
    for k in keys:
        h, r, w = (np.concatenate(v[k]) for v in (hs, rs, ws))
        tag = f"{what} route {route} {group.name} {k}"
        w_only = util.discrete_agreement(tag + " gate", h != 0, r != 0, w != 0)
        keep = np.flatnonzero((r != 0) & (w != 0))
        assert group.values is None or keep.size > 0, f"{tag}: no slot passes the gate"
        if keep.size:
            assert w_only.size == 0
            util.assert_accurate(tag, h[keep], r[keep], w[keep])


def run_group(be, g, route):
    return be.run(g.utts, route, g.maxc) if g.batch else [be.run([u], route, g.maxc)[0] for u in g.utts]


def case_group(be, name, what="harvest refine"):
    """every route of a group: footprint (run), gates of both outputs, accuracy of the refined F0, hv_refine == hv_refine_frames"""
    g = group(name)
    outs = {}
    for route in g.routes:
        outs[route] = run_group(be, g, route)
        for u, o in zip(g.utts, outs[route]):
            assert np.array_equal(o["refined"] != 0, o["score"] != 0), f"{name}/{u.name} route {route}: a slot with one of the two"
        hold(be, g, route, outs[route], what, ("refined",))
    if 1 in outs:
        for u, a, b in zip(g.utts, outs[1], outs[2]):
            for k in ("refined", "score"):
                assert same_bits(a[k], b[k]), f"{name}/{u.name}: hv_refine and hv_refine_frames differ in {k} at {np.argwhere(a[k] != b[k])[:8].tolist()}"
    return outs


def case_group_score(be, name, what="harvest refine"):
    """every route of a group: accuracy of the score"""
    g = group(name)
    for route in g.routes:
        hold(be, g, route, run_group(be, g, route), what, ("score",))


# ---- the groups ------------------------------------------------------------------------------------------------------------
def group_rates():
    """the table route at K = afs / 1000 = 6, 8, 10, 16; the rotation route at 7350, 11025 and 32000 / 3 Hz, where the residual r
    = first + hw - pos afs takes both signs and passes 0.4 in size (1/3 is all there is at 32000 / 3 Hz)"""
    def table(u, w):
        assert u.table and np.abs(residual(u, w)).max() < 1e-9, u.name

    def rotated(u, w):
        r = residual(u, w)
        most = 0.3 if u.name == "10667" else 0.4                     # (at 32000 / 3 Hz a millisecond is 10 2/3 samples: r is 0 or +-1/3)
        assert not u.table and r.min() < -most and r.max() > most and np.abs(r).max() <= 0.501, (u.name, r.min(), r.max())
    utts = []
    for afs in (6000.0, 8000.0, 10000.0, 16000.0, 7350.0, 11025.0, 32000.0 / 3.0):
        nf, n = 24, int(afs * 0.024) + 1
        c = np.zeros((nf, 2))
        c[:, 0] = track(nf, 182.0, seed=3, jitter=0.004)
        c[4:20, 1] = track(16, 182.0, seed=4, jitter=0.01)
        utts.append(U(f"{afs:.0f}", harmonic(afs, n, 182.0, seed=int(afs)), c, afs=afs, f0_floor=71.0,
                      reach=reaches(fn=table if math.fmod(afs, 1000.0) == 0 else rotated, gate=[L.HR_PASSED])))
    return Group("rates", utts)


def group_window_lengths():
    """hw at its maximum -- the candidate IS f0_floor -- with 1.5 afs / f0_floor whole (40 Hz at 8 kHz: hw 301, blen 603) and a
    hair to either side of whole (hw 300 | 301); blen on both sides of a power of two (255 | 257: lgN 9 | 10), of 32 (31 | 33)
    and 64 (63 | 65), blen mod 8 = 1, 3, 5, 7; the smallest windows (f0_ceil 2000 and 4000 at 8 kHz: blen 15 and 9)"""
    utts = []
    for name, fl, hw in (("floor 40", 40.0, 301), ("floor above", 40.0 * (1 + 1e-12), 300), ("floor below", 40.0 * (1 - 1e-12), 301)):
        assert hw_of(8000.0, fl) == hw
        c = np.zeros((40, 1))                                       # (frames 36 .. 39: the window's left half lies inside the signal)
        c[36:] = fl
        utts.append(U(name, harmonic(8000.0, 700, 42.0, seed=hw), c, f0_floor=fl, reach=reaches(hw=[hw], gate=[L.HR_PASSED])))
    for hw in (127, 128, 15, 16, 17, 18, 31, 32):
        f0 = 1.5 * 8000.0 / (hw - 0.5)
        assert hw_of(8000.0, f0) == hw
        lgn = 2 + int(math.log2(2 * hw + 1))
        utts.append(U(f"hw {hw}", harmonic(8000.0, 8 * 8 + 2 * hw, f0, seed=hw), np.full((8, 1), f0), f0_ceil=2000.0,
                      reach=reaches(hw=[hw], lgn=[lgn], gate=[L.HR_PASSED])))
    utts.append(U("ceil 2000", harmonic(8000.0, 80, 1950.0, seed=5), np.full((8, 1), 2000.0), f0_ceil=2000.0, reach=reaches(blen=[15], nh=[2])))
    utts.append(U("ceil 4000", harmonic(8000.0, 80, 3600.0, seed=6), np.full((8, 1), 3600.0), f0_ceil=4000.0, reach=reaches(blen=[9], nh=[1])))   # (4000 itself sits in the Nyquist bin: refined == f0_ceil, a tie)
    g = Group("window lengths", utts)
    assert {(2 * int(u.name[3:]) + 1) % 8 for u in utts if u.name.startswith("hw ")} == {1, 3, 5, 7}
    return g


def group_harmonics():
    """nh = 1 .. 6 with afs / 2 / f0 exactly whole at 800 and 1000 Hz; bins (h + 1) within 1e-9 of x.5 on both sides (the bin
    steps); (idx 8) mod N = 0, N / 4 and N / 2 (2 cos of the Goertzel angle = 2, 0, -2)"""
    utts = []
    for f0, nh in ((2500.0, 1), (1500.0, 2), (1100.0, 3), (1000.0, 4), (900.0, 4), (800.0, 5), (700.0, 5), (300.0, 6)):
        assert min(int(8000.0 / 2.0 / f0), 6) == nh
        utts.append(U(f"nh {nh} at {f0:.0f}", harmonic(8000.0, 160, f0, seed=int(f0)), np.full((8, 1), f0), f0_ceil=4000.0,
                      reach=reaches(nh=[nh], gate=[L.HR_PASSED])))

    def half_bin(side, bin_):
        def fn(u, w):
            s = slots(w)
            n = 1 << int(s[0, L.HR_LGN])
            x = u.cand[0, 0] * n / u.afs
            assert abs(x - 9.5) < 1e-9 and (x > 9.5) == (side > 0) and set(s[:, L.HR_IDX].tolist()) == {bin_}, (u.name, x)
        return fn
    for side, bin_ in ((+1, 10), (-1, 9)):
        f0 = 148.4375 * (1 + side * 2e-12)                           # hw 81, N 512: bins = 0.064 f0 = 9.5 -+
        utts.append(U(f"half bin {'above' if side > 0 else 'below'}", harmonic(8000.0, 260, 148.4375, seed=9), np.full((8, 1), f0),
                      reach=reaches(hw=[81], lgn=[9], fn=half_bin(side, bin_), gate=[L.HR_PASSED])))

    def angles(u, w):
        s = slots(w)
        n = 1 << int(s[0, L.HR_LGN])
        seen = {int(i) * 8 % n for i in s[0, L.HR_IDX:L.HR_IDX + 6]}
        assert n == 256 and {0, n // 4, n // 2} <= seen, (u.name, n, seen)
    utts.append(U("angles", harmonic(8000.0, 200, 250.0, seed=10), np.full((8, 1), 250.0), reach=reaches(nh=[6], fn=angles, gate=[L.HR_PASSED])))
    return Group("harmonics", utts)


def group_caches():
    """what hv_refine_frames keeps from one visited slot to the next (walk()): seven equal slots; the window kept and only some
    bins; a new window at every slot; a second track that starts where the first ended; an empty slot between two equal ones"""
    y = harmonic(8000.0, 340, 149.0, seed=11)
    nf = 16
    const = np.full((nf, 2), 149.0)
    a, b = 148.3, 149.0                                              # both hw 81; bins 9.49 / 9.54: harmonics 0, 2, 4 step
    assert hw_of(8000.0, a) == hw_of(8000.0, b) == 81
    alt = np.where(np.arange(nf)[:, None] % 2 == 0, a, b) * np.ones((1, 2))
    ramp = np.stack([140.0 + 2.5 * np.arange(nf), 183.1 - 2.5 * np.arange(nf)], axis=1)
    assert len({hw_of(8000.0, f) for f in ramp[:, 0]}) == nf
    gaps = const.copy()
    gaps[[3, 4, 8, 11], 0] = 0.0
    gaps[[2, 9, 10], 1] = 0.0
    lone = np.zeros((nf, 2))
    lone[6, 0] = lone[9, 1] = 149.0
    return Group("caches", [
        U("all equal", y, const, reach=reaches(walk=["full", "full carried"], never=["partial", "window"])),
        U("some bins", y, alt, reach=reaches(walk=["partial", "full", "partial carried"])),
        U("every slot", y, ramp, reach=reaches(walk=["rebuild"], never=["full", "partial", "window"])),
        U("gaps", y, gaps, reach=reaches(walk=["full over empty", "full carried"])),
        U("lone", y, lone, reach=reaches(walk=["rebuild"]))])


def group_edges():
    """1 to 9 frames, a candidate in every one (every slot whose source frame lies outside is the first or last frame's to
    empty); signals of 1, 2, blen - 1, blen, blen + 1 samples under the longest window (every sample clamped, one side
    clamped); no candidate slot at all (nothing written); a map of zeros"""
    utts = []
    for nf in (1, 2, 3, 4, 6, 7, 8, 9):
        c = np.stack([track(nf, 200.0, seed=nf, jitter=0.003), track(nf, 200.0, seed=nf + 50, jitter=0.01)], axis=1)
        utts.append(U(f"{nf} frames", harmonic(8000.0, 8 * nf + 130, 200.0, seed=20 + nf), c, reach=reaches(gate=[L.HR_PASSED])))
    for n in (1, 2, 602, 603, 604):
        utts.append(U(f"{n} samples", harmonic(8000.0, n, 40.0, seed=30 + n, noise=0.0) + 0.25, np.full((5, 1), 40.0), reach=reaches(hw=[301])))
    utts.append(U("no slots", harmonic(8000.0, 200, 200.0, seed=40), np.zeros((7, 0))))

    def nothing(u, w):
        assert slots(w).shape[0] == 0, u.name
    utts.append(U("all empty", harmonic(8000.0, 200, 200.0, seed=41), np.zeros((7, 2)), reach=nothing))
    return Group("edges", utts)


def group_gates():
    """the three ways the gate closes, each decided in W with a margin, and digital silence: power exactly 0 in every bin"""
    def silent(u, w):
        s = slots(w)
        assert s.shape[0] and np.array_equal(s[:, L.HR_ZERO_POWER], s[:, L.HR_NH]), u.name
    return Group("gates", [
        U("below floor", harmonic(8000.0, 300, 70.0, seed=50), np.full((8, 1), 72.0), f0_floor=71.0, reach=reaches(only_gate=[L.HR_FLOOR])),
        U("above ceil", harmonic(8000.0, 120, 900.0, seed=51), np.full((8, 1), 798.0), reach=reaches(gate=[L.HR_CEIL])),
        U("low score", harmonic(8000.0, 200, 500.0, seed=52, noise=1e-6, amps=(1.0,)), np.full((8, 1), 330.0), reach=reaches(gate=[L.HR_SCORE])),
        U("silence", np.zeros(200), np.full((8, 2), 200.0), reach=reaches(only_gate=[L.HR_FLOOR], fn=silent))], values=None)


def group_batches():
    """ragged nfb, nc and y_len in one call: the slot layout j + nc[u] m differs per utterance, the frame counts are no multiple
    of the four wavefronts of a workgroup, and rows are 28 slots wide where the widest utterance uses 21"""
    utts = []
    for i, (nf, nc, n, f0) in enumerate(((5, 1, 170, 210.0), (9, 3, 260, 150.0), (13, 0, 100, 100.0), (6, 2, 333, 95.0), (3, 3, 90, 400.0), (14, 2, 240, 120.0))):
        c = np.stack([track(nf, f0, seed=60 + 7 * i + j, jitter=0.004 * (j + 1)) for j in range(nc)], axis=1) if nc else np.zeros((nf, 0))
        if nc > 1:
            c[nf // 2, 1] = 0.0
        utts.append(U(f"utt {i}", harmonic(8000.0, n, f0, seed=70 + i), c))
    return Group("batches", utts, batch=True, maxc=28)


def group_wide():
    """15 candidates per frame, the default maxc = 105: tracks around three partials of one signal, some frames empty"""
    nf, nc = 12, 15
    c = np.zeros((nf, nc))
    for j in range(nc):
        c[:, j] = track(nf, (110.0, 220.0, 330.0)[j % 3], seed=80 + j, jitter=0.006)
        c[(j * 5) % nf, j] = 0.0
    return Group("wide", [U("15 candidates", harmonic(8000.0, 400, 110.0, seed=81), c)], maxc=105)


GROUPS = {"rates": group_rates, "window lengths": group_window_lengths, "harmonics": group_harmonics, "caches": group_caches,
          "edges": group_edges, "gates": group_gates, "batches": group_batches, "wide": group_wide}


def group(name):
    return cached(("harvest refine group", name), GROUPS[name])


# ---- identities that need no oracle ----------------------------------------------------------------------------------------
def case_batch_is_its_lone_calls(be):
    g = group("batches")
    for route in g.routes:
        for u, o in zip(g.utts, be.run(g.utts, route, g.maxc)):
            lone = be.run([u], route)[0]
            for k in ("refined", "score"):
                assert same_bits(o[k], lone[k]), f"{u.name} route {route}: {k} in the batch is not the lone call's"


def case_scaling(be):
    """The signal times 2^k.  Every recurrence, product and sum scales exactly, niv / pwv -- and with it the instantaneous
    frequencies and the score -- is unchanged bit for bit, but the refined F0 is num / (den + 1e-12) (FixF0's safeguard): den
    scales and the safeguard does not.  So: the score is the same bits for k = -30, 0, 30, 200 wherever the slot is written;
    k = 30 and k = 200 (the safeguard is below half an ulp of den) agree bit for bit in both outputs; at k = -200 den is far
    below the safeguard, the refined F0 is 0 to every digit and the gate closes every slot."""
    g = group("caches")
    for u in g.utts[:2] + group("rates").utts[4:5]:
        for route in u.routes:
            o = {k: be.run([U(u.name, u.y * 2.0 ** k, u.cand, **u.args)], route)[0] for k in (-200, -30, 0, 30, 200)}
            assert o[0]["score"].any(), u.name
            assert same_bits(o[30]["refined"], o[200]["refined"]) and same_bits(o[30]["score"], o[200]["score"]), (u.name, route)
            for k in (-30, 30):
                assert np.array_equal(o[k]["score"] != 0, o[0]["score"] != 0) and same_bits(o[k]["score"], o[0]["score"]), (u.name, route, k)
                assert util.max_rel(o[k]["refined"][o[0]["refined"] != 0], o[0]["refined"][o[0]["refined"] != 0]) < 1e-4
            assert not o[-200]["refined"].any() and not o[-200]["score"].any(), (u.name, route)


def case_delay(be):
    """on the table route a window is a row of the table wherever the frame lies: the signal delayed by K = afs / 1000 samples
    and every candidate moved one frame later give the same bits one frame later, wherever no window is clamped at an end"""
    for afs, f0 in ((8000.0, 230.0), (16000.0, 260.0)):
        k, nf, hw = int(afs / 1000.0), 20, hw_of(afs, f0 * 0.99)
        n = k * (nf + 2) + 2 * hw
        y = harmonic(afs, n, f0, seed=90)
        c = np.stack([track(nf, f0, seed=91, jitter=0.005), track(nf, f0, seed=92, jitter=0.009)], axis=1)
        later = np.concatenate([np.zeros((1, 2)), c])
        lo = (hw + 2 + k - 1) // k + 3                               # frames whose seven windows all lie inside both signals
        assert lo < nf - 4
        for route in (1, 2):
            a = be.run([U("a", y[k:], c, afs=afs, f0_floor=71.0)], route)[0]
            b = be.run([U("b", y, later, afs=afs, f0_floor=71.0)], route)[0]
            assert a["refined"][lo:nf - 3].all()
            for key in ("refined", "score"):
                assert same_bits(a[key][lo:nf - 3], b[key][lo + 1:nf - 2]), (afs, route, key)


def case_refusals(be):
    """a refusal names the argument and writes nothing"""
    g = group("caches")
    utts = g.utts[:1]
    u = utts[0]

    def refused(word, who=None, route=1, **override):
        rc, d, _ = be.call(who or utts, route, override=override)
        assert rc != 0 and word in be.error(), (word, override, rc, be.error())
        for k in ("refined", "score"):
            assert np.isnan(be.host(d[k])).all(), (word, k, "written by a refused call")
    refused("n_utt", n_utt=0)
    refused("y_len", y_len=None)
    refused("nfb", nfb=(C.c_int * 1)(0))
    refused("nc", nc=(C.c_int * 1)(-1))
    refused("nc", nc=(C.c_int * 1)(3))                                  # 21 slots in rows of 14
    refused("y_len", y_len=(C.c_int * 1)(0))
    refused("y_len", y_len=(C.c_int * 1)(len(u.y) + 9))                 # past y_stride
    refused("maxc", maxc=15)
    refused("maxc", maxc=0)
    refused("fb_stride", fb_stride=((u.nf + 7) & ~7) + 8)
    refused("afs", afs=float("nan"))
    refused("afs", afs=500.0)
    refused("f0_floor", f0_floor=0.0)
    refused("f0_floor", f0_ceil=30.0)
    refused("f0_floor", f0_floor=1.0)                                   # a window of 24 003 samples
    refused("route", route=4)
    refused("route", route=-1)
    refused("route", route=1, afs=11025.0)
    refused("route", route=2, afs=7350.0)
    for k in ("y", "cand", "refined", "score"):
        refused(k, **{k: None})
    for bad in (39.9, 801.0, -1.0, float("nan"), float("inf")):
        c = np.array(u.cand)
        c[5, 1] = bad
        refused("cand", who=[U("bad", u.y, c)])
    refused("cand", who=[U("bad", u.y, np.full((4, 1), 3500.0), afs=6000.0, f0_ceil=4000.0)])      # above afs / 2
    rc, d, _ = be.call(utts, 1)
    assert rc == 0, be.error()
    before = np.array(be.host(d["refined"]))
    rc, _, _ = be.call(utts, 1, override=dict(refined=be.ptr(d["refined"]), score=be.ptr(d["refined"])))
    assert rc != 0 and "overlaps" in be.error(), be.error()
    assert same_bits(be.host(d["refined"]), before)
