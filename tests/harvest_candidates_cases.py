"""Harvest's candidate stage alone (include/world_hip.h: world_hip_probe_harvest_candidates -- hv_compact_events,
hv_raw_candidates and hv_detect on zero-crossing lists the caller made up): the cases tests/test_harvest_candidates_cpu.py runs
on the host emulation and tests/test_harvest_candidates_gpu.py on the card, as functions of a backend.

The comparators.  R = the reference's own GetF0CandidateContour and DetectOfficialF0Candidates (oracle/_ref/
libworld_ref_candidates.so: oracle/harvest_candidates_ref.cpp includes the reference's harvest.cpp where it lies), O = the
oracle's restatement (world_oracle.c: wo_harvest_candidates), G = R's results recorded in tests/golden/harvest_candidates.npz
(tests/golden/make_golden_harvest_candidates.py: raw and cand of the golden-flagged groups, the CRC-32 of both for the rest).
expected() asserts R == O == G bit for bit wherever R is built (O == G elsewhere) and then the case's own reach.  Compaction
is held to its plain statement in numpy: the segments concatenated in order, cut at ev_cap.

Everything in the stage is + - x / and comparisons in the reference's operand order, and the library is built with
-ffp-contract=off: what is asserted of the code under test -- events, ev_count, raw over [nch][nfb[u]], cand below zcap, nc --
is asserted BIT FOR BIT, on the emulator and on the card; rows, slots and list entries the stage does not own keep the
sentinel.  No tolerance appears in this module.

Every case states what it was built to reach and asserts it on the host before the library is called -- from the oracle's
outputs and from the numpy restatement below of the documented rules (counts at the run ends, the staged range m per family,
the route, the exit the 32-lane search takes, the runs of a frame): a case that stops reaching its branch fails.  The probe
does not report the route (hv_raw_candidates is left exactly as it was); the restated rule names it.

The emulator runs the serial search (bandfilter.h: intervals_at_or_before, bracket and bisect): the groups "guess misses" and
"small lists" hold that there, and the 32-lane group search (intervals_at_or_before_group) is held by the GPU module alone.

Lists.  Edges are strictly increasing doubles in samples of the analysis rate, 8000 Hz unless a case says otherwise; frame f
sits at f / 1000 s, i.e. at sample 8 f.  A list whose candidates are to be SEEN is put into every band of a geometric ladder of
boundary F0s (ratio 1.2 < 1.1 / 0.9), so that every value passes some band's gate."""
import ctypes as C
import os
import zlib

import numpy as np

import backends
import util
from backends import cached, same_bits

GOLDEN = os.path.join(util.GOLDEN, "harvest_candidates.npz")
SENTINEL = backends.SENTINEL_F64
AFS = 8000.0
RUN = 256                    # harvest.hip: kRawRun, the frames of one workgroup of hv_raw_candidates
CAP = 288                    # bandfilter.h: kIntervalCap, the intervals a run stages per family
BATCH = 19                   # harvest.hip: hv_detect's kBatch


def maxc_of(nch):
    return int(nch / 10.0 + 0.5) * 7          # harvest.cpp:1179-1181


def zcap_of(nch):
    return min(maxc_of(nch), (nch + 10) // 11 + 1)      # harvest.hip: hv_detect's zero fill


def ladder(nch, lo):
    return lo * 1.2 ** np.arange(nch)


# ---- the documented rules, restated ---------------------------------------------------------------------------------------
def locs(e, afs=AFS):
    e = np.asarray(e, dtype=np.float64)
    return (e[:-1] + e[1:]) / 2.0 / afs


def frame_time(f):
    return f * 1 / 1000.0


def count_at(loc, t):
    """#{intervals whose location is <= t}: histc's >="""
    return int(np.searchsorted(loc, t, side="right"))


def staged_range(n_int, c_first, c_last):
    """bandfilter.h: interval_range_close -> (j_lo, m)"""
    k_first, k_last = min(max(c_first, 1), n_int - 1), min(max(c_last, 1), n_int - 1)
    return k_first - 1, k_last - (k_first - 1) + 1


def run_info(lists, nf, afs=AFS):
    """per run of RUN frames: dict(route = 0 zeroed by CheckEvent / 1 staged / 2 unstaged, c = [(c_first, c_last)] and
    m = [m] per family)"""
    n_int = [max(len(e) - 1, 0) for e in lists]
    out = []
    for f0 in range(0, nf, RUN):
        f1 = min(f0 + RUN, nf)
        if min(n_int) < 3:
            out.append(dict(route=0, c=[], m=[]))
            continue
        c = [(count_at(locs(e, afs), frame_time(f0)), count_at(locs(e, afs), frame_time(f1 - 1))) for e in lists]
        m = [staged_range(n, a, b)[1] for n, (a, b) in zip(n_int, c)]
        out.append(dict(route=1 if max(m) <= CAP else 2, c=c, m=m))
    return out


def group_search(loc, t):
    """bandfilter.h: intervals_at_or_before_group, lane by lane -> (count, the exits and clamps taken)"""
    n, tags = len(loc), []
    if n <= 0:
        return 0, ["empty"]
    if not loc[0] <= t:
        return 0, ["before first"]
    if loc[n - 1] <= t:
        return n, ["after last"]
    lo, hi = 0, n - 1
    ones_at = lambda idx: sum(1 for i in idx if loc[i] <= t)
    if hi - lo > 32:
        r = (t - loc[0]) / (loc[n - 1] - loc[0]) * (n - 1)
        g = 0 if r < 0.0 else (n - 1 if r > n - 1.0 else int(r))
        base = g - 15
        if base < lo + 1:
            base = lo + 1
            tags.append("base at lo + 1")
        if base > hi - 32:
            base = hi - 32
            tags.append("base at hi - 32")
        ones = ones_at(range(base, base + 32))
        if ones == 0:
            hi = base
            tags.append("window 0")
        elif ones == 32:
            lo = base + 31
            tags.append("window 32")
        else:
            tags.append("window 1" if ones == 1 else "window 31" if ones == 31 else "window mid")
            return base + ones, tags
    else:
        tags.append("no window")
    rounds = 0
    if hi - lo > 1024:
        tags.append("range above 1024")                        # (two strided rounds at the least)
    while hi - lo > 32:
        stride = (hi - lo + 31) // 32
        ones = ones_at(i for i in (lo + (s + 1) * stride for s in range(32)) if i < hi)
        lo, hi = lo + ones * stride, min(lo + (ones + 1) * stride, hi)
        rounds += 1
    if rounds:
        tags.append(f"strided {min(rounds, 2)}")
    left = hi - lo - 1
    tags.append("closing 0" if left == 0 else "closing 1" if left == 1 else "closing 31" if left == 31 else "closing mid")
    return lo + 1 + ones_at(range(lo + 1, hi)), tags


def search_exits(lists, nf):
    """the exits the eight end-point searches of every run take, and every count held to searchsorted"""
    tags = set()
    for e in lists:
        loc = locs(e)
        for f0 in range(0, nf, RUN):
            for f in (f0, min(f0 + RUN, nf) - 1):
                c, tg = group_search(loc, frame_time(f))
                assert c == count_at(loc, frame_time(f)), "the restated search miscounts"
                tags.update(tg)
    return tags


def interp1_at(e, t, strict=False):
    """interp1 of one family's interval F0s at t (matlabfunctions.cpp:136-176); strict: histc's >= taken as >"""
    loc, y = locs(e), AFS / np.diff(e)
    k = min(max(int(np.searchsorted(loc, t, side="left" if strict else "right")), 1), len(loc) - 1)
    return y[k - 1] + (t - loc[k - 1]) / (loc[k] - loc[k - 1]) * (y[k] - y[k - 1])


def sum_of_four(fams, t, strict=False):
    v = [interp1_at(e, t, strict) for e in fams]
    return (v[0] + v[1] + v[2] + v[3]) / 4.0


def frame_runs(col):
    """the voiced runs [(st, ed)] of one frame's raw candidates [nch], DetectOfficialF0CandidatesSub1's (bands 0 and nch - 1
    count as unvoiced)"""
    v = (np.asarray(col) > 0).astype(np.int8)
    v[0] = v[-1] = 0
    d = np.diff(v)
    return list(zip((np.flatnonzero(d == 1) + 1).tolist(), (np.flatnonzero(d == -1) + 1).tolist()))


def candidates_of(raw):
    """per frame the number of runs of at least ten bands"""
    return np.array([sum(1 for st, ed in frame_runs(raw[:, i]) if ed - st >= 10) for i in range(raw.shape[1])], dtype=np.int64)


# ---- cases ----------------------------------------------------------------------------------------------------------------
class U:
    """one utterance: nf frames at 1 ms; lists {band: four arrays of edges} (a band without an entry has four empty lists),
    or raw [nch, nf] for detection alone; reach(u, o): assertions on the oracle's outputs o"""

    def __init__(self, name, nf, lists=None, raw=None, reach=None):
        self.name, self.nf, self.lists, self.raw, self.reach = name, nf, lists, raw, reach
        for fams in (lists or {}).values():
            assert len(fams) == 4 and all(np.all(np.diff(e) > 0) for e in fams), name


class Group:
    """utterances that go through the probe in one call"""

    def __init__(self, name, band_f0, utts, f0_floor=40.0, f0_ceil=2000.0, afs=AFS, golden=False):
        self.name, self.band_f0, self.utts = name, np.asarray(band_f0, dtype=np.float64), list(utts)
        self.f0_floor, self.f0_ceil, self.afs, self.golden = f0_floor, f0_ceil, afs, golden
        self.nch, self.events = len(self.band_f0), self.utts[0].raw is None
        assert 12 <= self.nch <= 365 and len({u.name for u in self.utts}) == len(self.utts), name
        assert all(u.nf <= 2001 and (u.raw is None) == self.events for u in self.utts), name
        self.ev_cap = max([len(e) for u in self.utts for fams in (u.lists or {}).values() for e in fams] + [1]) + 3

    def packed(self, u):
        """edges [nch, 4, ev_cap] (what lies past a list's count is junk nobody may read) and counts [nch, 4]"""
        edges = np.full((self.nch, 4, self.ev_cap), 1e300)
        counts = np.zeros((self.nch, 4), dtype=np.int32)
        for band, fams in u.lists.items():
            for fam, e in enumerate(fams):
                edges[band, fam, :len(e)], counts[band, fam] = e, len(e)
        return edges, counts


def _fail(*why):
    raise AssertionError(why)


def periodic(P, start, n):
    return start + P * np.arange(n)


def quarter(P, start, n):
    """four families of n events of period P, a quarter period apart"""
    return [periodic(P, start + fam * P / 4.0, n) for fam in range(4)]


def from_periods(periods, start):
    return start + np.concatenate([[0.0], np.cumsum(periods)])


def glide(rng, span, p0, p1, start=0.0, walk=0.0):
    """edges over [start, start + span): periods going from p0 to p1 linearly, with a random walk of relative size `walk`"""
    n = int(2 * span / (p0 + p1)) + 2
    p = np.linspace(p0, p1, n)
    if walk:
        p = p * np.exp(np.cumsum(rng.uniform(-walk, walk, n)))
        p = np.clip(p, 5.0, 150.0)
    e = from_periods(p, start)
    return e[e < start + span + p1]


def families(rng, span, p0, p1, start=0.0, walk=0.0):
    return [glide(rng, span, p0, p1, start + rng.uniform(0, p0), walk) for _ in range(4)]


def everywhere(nch, fams):
    return {band: fams for band in range(nch)}


# ---- the comparators ------------------------------------------------------------------------------------------------------
def oracles():
    def make():
        from oracle import loader
        return loader.PortOracle(), (loader.RefCandidates() if loader.RefCandidates.available() else None)
    return cached(("harvest candidates oracles",), make)


def golden():
    return cached(("harvest candidates golden",), lambda: dict(np.load(GOLDEN)))


def digest(o):
    """the golden file's record of a large or random case: CRC-32 of raw's and cand's bytes, and nc"""
    return np.array([zlib.crc32(np.ascontiguousarray(o[k]).tobytes()) for k in ("raw", "cand")] + [o["nc"]], dtype=np.int64)


def compute(which, group, u):
    a = dict(afs=group.afs, f0_floor=group.f0_floor, f0_ceil=group.f0_ceil)
    if group.events:
        edges, counts = group.packed(u)
        return which.harvest_candidates(u.nf, group.band_f0, edges=edges, counts=counts, **a)
    return which.harvest_candidates(u.nf, group.band_f0, raw=u.raw, **a)


def expected(group):
    """per utterance the oracle's raw [nch, nf], cand [nf, maxc] and nc, after R == O == G and the case's own reach"""
    def make():
        port, ref = oracles()
        g = golden()
        out = []
        for u in group.utts:
            o = compute(port, group, u)
            what = f"{group.name}/{u.name}"
            if ref is not None:
                r = compute(ref, group, u)
                assert r["nc"] == o["nc"], f"{what}: the oracle's nc is not the reference's"
                for k in ("raw", "cand"):
                    assert same_bits(r[k], o[k]), f"{what}: the oracle's {k} is not the reference's"
            if group.golden:
                for k in ("raw", "cand"):
                    assert same_bits(g[f"{what}/{k}"], o[k]), f"{what}: the oracle's {k} is not the recorded reference's"
            else:
                assert np.array_equal(g[f"{what}/crc"], digest(o)), f"{what}: the oracle's results are not the recorded reference's"
            # the restated detection rule, on every case
            n = candidates_of(o["raw"])
            assert np.array_equal(n, np.count_nonzero(o["cand"], axis=1)) and o["nc"] == n.max(), f"{what}: runs per frame"
            assert not o["cand"][:, zcap_of(group.nch):].any(), f"{what}: a candidate beyond zcap"
            if u.reach:
                u.reach(u, o)
            o["raw"].setflags(write=False)
            o["cand"].setflags(write=False)
            out.append(o)
        return out
    return cached(("harvest candidates expected", group.name), make)


# ---- the backend ----------------------------------------------------------------------------------------------------------
class Backend(backends.Backend):
    def call(self, nfb, band_f0, seg_events=None, seg_count=None, raw=None, ev_cap=1, ev_group=40, stages=7, afs=AFS, f0_floor=40.0,
             f0_ceil=2000.0, override=None):
        """the probe -> (return code, the device arrays by name, the host copies of the inputs); seg_events [n, nch * 4, nseg,
        seg_cap]; `override` replaces arguments of the C call (refusals)"""
        n, nch, stride = len(nfb), len(band_f0), (max(nfb) + 7) & ~7
        maxc = maxc_of(nch)
        nseg, seg_cap = seg_events.shape[2:] if seg_events is not None else (1, ev_cap)
        d, keep = {}, {}
        if seg_events is not None:
            keep = dict(seg_events=np.array(seg_events, dtype=np.float64), seg_count=np.array(seg_count, dtype=np.int32))
            d.update({k: self.dev(v) for k, v in keep.items()})
            d["events"] = self.dev(np.full((n, nch * 4, ev_cap), SENTINEL))
            d["ev_count"] = self.dev(np.full((n, nch * 4), -7, dtype=np.int32))
        if raw is not None:
            keep["raw"] = np.array(raw, dtype=np.float64)
            assert keep["raw"].shape == (n, nch, stride)
            d["raw"] = self.dev(keep["raw"])
        else:
            d["raw"] = self.dev(np.full((n, nch, stride), SENTINEL))
        d["cand"] = self.dev(np.full((n, stride, maxc), SENTINEL))
        d["nc"] = self.dev(np.full(n, -7, dtype=np.int32))
        a = dict(n_utt=n, nfb=(C.c_int * n)(*nfb), afs=afs, f0_floor=f0_floor, f0_ceil=f0_ceil, nch=nch,
                 band_f0=(C.c_double * nch)(*[float(v) for v in band_f0]), maxc=maxc, fb_stride=stride, nseg=nseg, seg_cap=seg_cap,
                 ev_cap=ev_cap, ev_group=ev_group, stages=stages)
        a.update({k: self.ptr(d.get(k)) for k in ("seg_events", "seg_count", "events", "ev_count", "raw", "cand", "nc")})
        a.update(override or {})
        rc = self.lib.world_hip_probe_harvest_candidates(self.ctx, *(a[k] for k in (
            "n_utt", "nfb", "afs", "f0_floor", "f0_ceil", "nch", "band_f0", "maxc", "fb_stride", "nseg", "seg_cap", "ev_cap", "ev_group",
            "stages", "seg_events", "seg_count", "events", "ev_count", "raw", "cand", "nc")))
        return rc, d, keep

    def run(self, nfb, band_f0, **kw):
        """-> the host copies of every array; the inputs must be as they were"""
        rc, d, keep = self.call(nfb, band_f0, **kw)
        assert rc == 0, self.error()
        h = {k: self.host(v) for k, v in d.items()}
        for k, v in keep.items():
            assert same_bits(h[k], v) if v.dtype == np.float64 else np.array_equal(h[k], v), f"the probe wrote into {k}"
        return h

    def run_group(self, group, ev_group=40, only=None):
        """stages 2 and 4 (events) or 4 (raw given) on a group -> per utterance dict(raw [nch, nf], cand [nf, zcap], nc), after
        the checks of what the stage does not own"""
        utts = group.utts if only is None else [group.utts[i] for i in only]
        nfb = [u.nf for u in utts]
        n, nch, stride, zcap = len(utts), group.nch, (max(nfb) + 7) & ~7, zcap_of(group.nch)
        a = dict(afs=group.afs, f0_floor=group.f0_floor, f0_ceil=group.f0_ceil, ev_group=ev_group)
        if group.events:
            packed = [group.packed(u) for u in utts]
            h = self.run(nfb, group.band_f0, seg_events=np.stack([e for e, _ in packed]).reshape(n, nch * 4, 1, group.ev_cap),
                         seg_count=np.stack([c for _, c in packed]).reshape(n, nch * 4, 1), ev_cap=group.ev_cap, stages=6, **a)
            assert np.all(h["events"] == SENTINEL) and np.all(h["ev_count"] == -7), "one segment list: nothing to report"
        else:
            raw = np.full((n, nch, stride), 333.0)                    # frames past nfb are nobody's: never looked at
            for i, u in enumerate(utts):
                raw[i, :, :u.nf] = u.raw
            h = self.run(nfb, group.band_f0, raw=raw, stages=4, **a)
        out = []
        for i, u in enumerate(utts):
            what = f"{group.name}/{u.name}"
            assert np.all(h["raw"][i, :, u.nf:] == (SENTINEL if group.events else 333.0)), f"{what}: raw written past frame nfb"
            assert np.all(h["cand"][i, u.nf:] == SENTINEL), f"{what}: cand written past frame nfb"
            assert np.all(h["cand"][i, :, zcap:] == SENTINEL), f"{what}: cand written past slot zcap"
            out.append(dict(raw=h["raw"][i, :, :u.nf], cand=h["cand"][i, :u.nf, :zcap], nc=int(h["nc"][i])))
        return out


def hold(be, group, outs=None, want=None):
    want = expected(group) if want is None else want
    outs = be.run_group(group) if outs is None else outs
    zcap = zcap_of(group.nch)
    for u, o, w in zip(group.utts, outs, want):
        what = f"{group.name}/{u.name}"
        assert same_bits(o["raw"], w["raw"]), f"{what}: raw differs at (band, frame) {np.argwhere(o['raw'] != w['raw'])[:8].tolist()}"
        assert same_bits(o["cand"], w["cand"][:, :zcap]), f"{what}: cand differs at (frame, slot) {np.argwhere(o['cand'] != w['cand'][:, :zcap])[:8].tolist()}"
        assert o["nc"] == w["nc"], f"{what}: nc {o['nc']}, the reference's {w['nc']}"
    return outs


# ---- event -> raw candidate groups ----------------------------------------------------------------------------------------
def group_counts():
    """0, 1, 2, 3 events in one family (n_int 0, 0, 1, 2) zero the band, 4 (n_int = 3) is the smallest list that passes; each
    family takes its turn; and an utterance with every band zeroed"""
    nch, lists = 20, {}
    for fam in range(4):
        for i in range(5):
            fams = quarter(40.0, 100.0, 60)
            fams[fam] = fams[fam][10:10 + i]
            lists[fam * 5 + i] = fams

    def reach(u, o):
        for band in range(nch):
            passes = band % 5 == 4
            assert bool(o["raw"][band].any()) == passes, (band, "n_int = 3 passes, fewer zero the band")
            assert run_info(lists[band], u.nf)[0]["route"] == (1 if passes else 0)
        assert np.all(o["raw"][4::5] == 200.0)

    none = {band: [f[:3] for f in quarter(40.0, 100.0, 60)] for band in range(nch)}
    return Group("counts", np.full(nch, 200.0), [
        U("short family", 300, lists, reach=reach),
        U("all zeroed", 300, none, reach=lambda u, o: (not o["raw"].any() and o["nc"] == 0) or _fail("a band survived"))], golden=True)


def gate_side(c, factor, kept):
    """a double fb near c / factor: kept -- fb * factor == c exactly; not kept -- the nearest fb whose product lies beyond c
    (below it for the upper limit 1.1, above it for the lower limit 0.9: one unit in the last place of c where the products'
    spacing allows, the next product beyond otherwise)"""
    x = c / factor
    for _ in range(64):
        x = np.nextafter(x, -np.inf)
    near = [float(x)]
    for _ in range(128):
        near.append(float(np.nextafter(near[-1], np.inf)))
    if kept:
        hits = [v for v in near if v * factor == c]
        return hits[0] if hits else _fail("no boundary F0 whose product is", c, "take another period")
    return max(v for v in near if v * factor < c) if factor > 1 else min(v for v in near if v * factor > c)


PERIODS = (40.0, 36.5, 50.25, 20.0, 64.0, 9.5)


def group_constant():
    """uniform periods P, the four families a quarter period apart: every frame's candidate is afs / P exactly.  Per period four
    bands: c == fb * 1.1 and c == fb * 0.9 are kept, the nearest product outside each (gate_side) is dropped"""
    band_f0, lists = [], {}
    for i, P in enumerate(PERIODS):
        c = AFS / P
        band_f0 += [gate_side(c, 1.1, True), gate_side(c, 1.1, False), gate_side(c, 0.9, True), gate_side(c, 0.9, False)]
        for k in range(4):
            lists[4 * i + k] = quarter(P, 3.0, int(2500 / P))

    def reach(u, o):
        for i, P in enumerate(PERIODS):
            c = AFS / P
            assert band_f0[4 * i] * 1.1 == c and band_f0[4 * i + 1] * 1.1 < c and band_f0[4 * i + 2] * 0.9 == c and band_f0[4 * i + 3] * 0.9 > c
            for k, kept in enumerate((True, False, True, False)):
                assert np.all(o["raw"][4 * i + k] == (c if kept else 0.0)), (P, k)
    return Group("constant", band_f0, [U("six periods", 300, lists, reach=reach)], f0_floor=40.0, f0_ceil=2000.0, golden=True)


def group_limits(side):
    """c == f0_ceil and c == f0_floor are kept; one unit in the last place beyond, dropped"""
    c = AFS / 40.0
    floor, ceil, kept = dict(ceil=(40.0, c, True), ceil_out=(40.0, np.nextafter(c, -np.inf), False), floor=(c, 2000.0, True),
                             floor_out=(np.nextafter(c, np.inf), 2000.0, False))[side]

    def reach(u, o):
        assert np.all(o["raw"] == (c if kept else 0.0))
    return Group(f"limits {side}", np.full(12, 200.0), [U("P 40", 40, everywhere(12, quarter(40.0, 3.0, 20)), reach=reach)],
                 f0_floor=floor, f0_ceil=ceil, golden=True)


NCH_LADDER, LADDER_LO = 20, 45.0


def _seen(u, o):
    """the case's values are not all gated away: every frame of the utterance passes some band's gate"""
    assert np.all((o["raw"] > 0).any(axis=0)), (u.name, "frames without a surviving candidate", np.flatnonzero(~(o["raw"] > 0).any(axis=0))[:8])


def group_glide():
    """periods growing, shrinking and walking at random, so every rounding of interp1 matters; 1, 255, 256, 257, 600 and 2001
    frames: the run tail, and the workgroups with f_begin >= f_end beside the longest utterance"""
    rng = np.random.default_rng(11)
    utts = []
    for i, nf in enumerate((1, 255, 256, 257, 600, 2001)):
        span = 8.0 * nf + 400
        p0, p1, walk = ((14.0, 60.0, 0.0), (70.0, 12.0, 0.0), (30.0, 30.0, 0.03))[i % 3]
        fams = families(rng, span, p0, p1, start=-200.0, walk=walk)
        utts.append(U(f"{nf} frames", nf, everywhere(NCH_LADDER, fams), reach=_seen))
    return Group("glide", ladder(NCH_LADDER, LADDER_LO), utts)


def group_ends():
    """the first location after frame 300 and the last before frame nf - 400: both extrapolations of interp1, with a whole run
    left of every interval (counts 0, 0) and whole runs right of every interval (counts n_int, n_int); the same with n_int = 3"""
    rng = np.random.default_rng(12)
    nf = 1100
    long = [glide(rng, 8.0 * 400, 33.0, 35.0, 8.0 * 300 + rng.uniform(0, 30)) for _ in range(4)]
    short = [8.0 * 500 + np.array([0.0, 33.0, 66.0625, 99.1875]) + 7.0 * fam for fam in range(4)]

    def reach(fams):
        def check(u, o):
            info = run_info(fams, nf)
            n_int = [len(e) - 1 for e in fams]
            assert info[0]["c"] == [(0, 0)] * 4 and info[-1]["c"] == [(n, n) for n in n_int], info
            assert all(r["route"] == 1 for r in info)
            assert (o["raw"][:, :RUN] > 0).any() and (o["raw"][:, 4 * RUN:] > 0).any(), "the extrapolated ends are all gated away"
        return check
    return Group("ends", ladder(NCH_LADDER, LADDER_LO), [U("long", nf, everywhere(NCH_LADDER, long), reach=reach(long)),
                                                         U("n_int 3", nf, everywhere(NCH_LADDER, short), reach=reach(short))])


TIES_A, TIES_B = (0, 100, 255, 400, 511, 599), (256, 300, 512)     # (two adjacent frames cannot both tie in one list of ~36-sample periods)


def tied_list(rng, nf, frames, d, narrow=0.0):
    """a list with e[k] + e[k + 1] == 16 f for every f of `frames` (loc == t exactly), about 36 samples apart in between;
    narrow > 0: an interval of that width in front of every tied one"""
    anchors = [(-90.0, True)]
    for f in frames:
        anchors += ([(8.0 * f - d - narrow, False)] if narrow else []) + [(8.0 * f - d, False), (8.0 * f + d, True)]
    anchors.append((8.0 * nf + 90.0, False))
    e = []
    for (a, fill), (b, _) in zip(anchors[:-1], anchors[1:]):
        n = max(int(round((b - a) / (34.0 + rng.uniform(0, 5)))), 1) if fill else 1
        e += np.linspace(a, b, n, endpoint=False).tolist()
    return np.array(e + [anchors[-1][0]])


def group_ties():
    """a frame time equal to an interval location (histc's >=): at f_begin (0, 256, 512), at f_end - 1 (255, 511, 599) and
    mid-run; in one family (a second one takes the frames next to the first one's) and in all four"""
    rng = np.random.default_rng(13)
    nf = 600

    def reach(fams, tied):
        def check(u, o):
            for fam, frames in tied.items():
                e = fams[fam]
                for f in frames:
                    k = int(np.searchsorted(e, 8.0 * f, side="right")) - 1
                    assert e[k] + e[k + 1] == 16.0 * f and (e[k] + e[k + 1]) / 2.0 / AFS == frame_time(f), (fam, f)
            _seen(u, o)
        return check
    one = [tied_list(rng, nf, TIES_A, 17.25), tied_list(rng, nf, TIES_B, 18.5)] + [glide(rng, 8.0 * nf + 200, 36.0, 37.0, -100.0 + 9.0 * k) for k in range(2)]
    four_a = [tied_list(rng, nf, TIES_A, d) for d in (16.5, 18.0, 19.75, 15.125)]
    four_b = [tied_list(rng, nf, TIES_B, d) for d in (16.5, 18.0, 19.75, 15.125)]
    # A tie decides between two segments of interp1 that meet in the knot: the one that ends there gives y0 + 1.0 * (y1 - y0),
    # the one that starts there y1 itself.  The two differ only where y1 - y0 is inexact, and the frame's candidate only where
    # that survives the sum of the four families: a 2-sample interval (4000 Hz) in front of a wide tied one (113 Hz) loses
    # five bits of y1 in the difference.
    steep = [tied_list(rng, nf, TIES_A, 35.25, narrow=2.0)] + [glide(rng, 8.0 * nf + 200, 36.0, 37.0, -100.0 + 9.0 * k) for k in range(3)]

    def steep_reach(u, o):
        reach(steep, {0: TIES_A})(u, o)
        sums = [[sum_of_four(steep, frame_time(f), strict) for f in TIES_A] for strict in (False, True)]
        assert sum(a != b for a, b in zip(*sums)) >= 3, "histc's >= taken as > changes no candidate: the tie decides nothing"
    return Group("ties", ladder(NCH_LADDER, LADDER_LO), [
        U("steep", nf, everywhere(NCH_LADDER, steep), reach=steep_reach),
        U("one family", nf, everywhere(NCH_LADDER, one), reach=reach(one, {0: TIES_A, 1: TIES_B})),
        U("four families, run ends", nf, everywhere(NCH_LADDER, four_a), reach=reach(four_a, {fam: TIES_A for fam in range(4)})),
        U("four families, run starts", nf, everywhere(NCH_LADDER, four_b), reach=reach(four_b, {fam: TIES_B for fam in range(4)}))])


SMALL = (3, 8, 9, 31, 32, 33, 34, 64, 65)


def group_small_lists():
    """n_int = 3 .. 65: the serial search changes method at 9 intervals, the group search at 34"""
    rng = np.random.default_rng(14)
    utts = []
    for n in SMALL:
        nf = 300
        p = (8.0 * nf + 1200.0) / (n + 1)                      # the list spans the utterance and more either side, whatever its length
        fams = [from_periods(np.clip(p * np.exp(rng.uniform(-0.05, 0.05, n)), 4.0, None), -900.0 + rng.uniform(0, p / 4)) for _ in range(4)]

        def reach(u, o, fams=fams, n=n):
            assert all(len(e) - 1 == n for e in fams)
            tags = search_exits(fams, u.nf)
            assert ("no window" in tags) == (n <= 33) and any(t.startswith("window") for t in tags) == (n >= 34), (n, tags)
        utts.append(U(f"n_int {n}", nf, everywhere(24, fams), reach=reach))
    return Group("small lists", ladder(24, 12.0), utts, f0_floor=10.0, f0_ceil=2000.0)


MISS_EXITS = ("before first", "after last", "window 0", "window 32", "window 1", "window 31", "window mid", "base at lo + 1",
              "base at hi - 32", "strided 1", "strided 2", "range above 1024", "closing 0", "closing 1", "closing 31", "closing mid")


def miss_list(kind):
    """periods of about 2 and about 90 samples, no two neighbours alike: a count that is off by one picks another segment of
    interp1 and shows (between equal periods every segment gives the same value)"""
    rng = np.random.default_rng(sum(map(ord, kind)))
    dense = lambda n: 2.0 + rng.integers(-2, 3, n) / 16.0
    sparse = lambda n: 90.0 + rng.integers(-40, 41, n) / 8.0
    if kind == "dense first":
        p = [dense(1200), sparse(60)]
    elif kind == "sparse first":
        p = [sparse(60), dense(1200)]
    elif kind == "burst":
        p = [sparse(30), dense(1200), sparse(30)]
    else:                                                      # "long": hi - lo above 1024 behind the first window
        p = [dense(3800), sparse(100)]
    return np.concatenate(p)


def miss_candidates():
    """(kind, shift, nf, the exits of its searches) of every placement tried"""
    out = []
    for kind in ("dense first", "sparse first", "burst", "long"):
        p = miss_list(kind)
        nf = min(int(p.sum() / 8.0) + 60, 2001)
        for shift in np.arange(-16.0, 2048.0, 21.5):
            fams = [from_periods(p, shift + 0.5 * fam) for fam in range(4)]
            out.append((kind, float(shift), nf, search_exits(fams, nf)))
    return out


def group_guess_misses():
    """lists the proportional guess does not bracket -- 1200 intervals of 2 samples beside 60 of 90, the reverse, a dense burst
    in the middle, and 3900 intervals -- placed (a greedy cover over shifts of the list) so that the eight end-point searches
    take every exit of the documented search between them"""
    def make():
        cands, chosen, covered = miss_candidates(), [], set()
        while not covered >= set(MISS_EXITS):
            best = max(cands, key=lambda c: len((c[3] & set(MISS_EXITS)) - covered))
            gain = (best[3] & set(MISS_EXITS)) - covered
            assert gain, ("no placement reaches", sorted(set(MISS_EXITS) - covered))
            chosen.append(best)
            covered |= gain
        return chosen
    chosen = cached(("harvest candidates guess misses",), make)
    nch, utts = 24, []
    for kind, shift, nf, tags in chosen:
        fams = [from_periods(miss_list(kind), shift + 0.5 * fam) for fam in range(4)]
        utts.append(U(f"{kind} {shift}", nf, everywhere(nch, fams), reach=lambda u, o, fams=fams, tags=tags: (
            search_exits(fams, u.nf) == tags or _fail("exits moved"), _seen(u, o))))
    g = Group("guess misses", ladder(nch, 70.0), utts, f0_floor=40.0, f0_ceil=6000.0)
    g.exits = set().union(*(c[3] for c in chosen))
    assert g.exits >= set(MISS_EXITS), sorted(set(MISS_EXITS) - g.exits)
    return g


def cap_list(off):
    """40-sample periods, then periods of 7.125 samples give or take a quarter over samples 1900 .. 4300 (frames 256 .. 511 lie
    inside), then 40 again; no two dense neighbours alike, so that a count off by one shows"""
    rng = np.random.default_rng(16)
    dense = 7.125 + np.tile([0.25, -0.125, -0.25, 0.125], 85)[:337] + rng.integers(-1, 2, 337) / 32.0
    return from_periods(np.concatenate([[40.0] * 47, dense, [40.0] * 60]), 20.0 + off)


def cap_offset(want_m):
    """an offset of the list for which run 1 (frames 256 .. 511) touches exactly want_m intervals"""
    for off in np.arange(0.0, 7.125, 0.125):
        e = cap_list(off)
        a, b = count_at(locs(e), frame_time(RUN)), count_at(locs(e), frame_time(2 * RUN - 1))
        if staged_range(len(e) - 1, a, b)[1] == want_m:
            return float(off)
    _fail("no offset gives m =", want_m)


def group_cap_edge():
    """m == 288 in every family (staged) beside m == 289 in one family alone and in all four (unstaged); runs 0 and 2 of the same
    bands are staged"""
    def utt(name, ms):
        fams = [cap_list(cap_offset(m)) for m in ms]

        def reach(u, o):
            info = run_info(fams, u.nf)
            assert info[1]["m"] == list(ms) and info[1]["route"] == (1 if max(ms) <= CAP else 2), info[1]
            assert info[0]["route"] == info[2]["route"] == 1 and max(info[0]["m"] + info[2]["m"]) < CAP
            _seen(u, o)
        return U(name, 768, everywhere(NCH_LADDER, fams), reach=reach)
    return Group("cap edge", ladder(NCH_LADDER, LADDER_LO), [utt("288 everywhere", (288,) * 4), utt("289 in peaks", (288, 288, 289, 288)),
                                                             utt("289 everywhere", (289,) * 4)])


RAGGED = (1, 257, 600, 256, 2001)


def group_groups():
    """five utterances of 1, 257, 600, 256 and 2001 frames, each with lists of its own: walked in groups of 1, 2, 5 and 7"""
    rng = np.random.default_rng(15)
    utts = []
    for i, nf in enumerate(RAGGED):
        fams = families(rng, 8.0 * nf + 400, 20.0 + 9 * i, 48.0 - 5 * i, start=-200.0, walk=0.02)
        utts.append(U(f"utt {i}", nf, everywhere(NCH_LADDER, fams), reach=_seen))
    return Group("groups", ladder(NCH_LADDER, LADDER_LO), utts)


def group_random(call):
    """eight utterances of sixteen bands, every (band, utterance) with lists of its own of mixed density"""
    rng = np.random.default_rng(100 + call)
    nch, utts = 16, []
    band_f0 = ladder(nch, 50.0)
    for i in range(8):
        nf = int(rng.integers(60, 900))
        lists = {}
        for band in range(nch):
            if rng.uniform() < 0.1:
                lists[band] = [periodic(30.0, 5.0 * fam, int(rng.integers(0, 5))) for fam in range(4)]     # short or empty
                continue
            p = AFS / band_f0[band] * rng.uniform(0.8, 1.25)
            fams = []
            for _ in range(4):
                per = p * np.exp(np.cumsum(rng.uniform(-0.02, 0.02, int(8.0 * nf / p) + 8)))
                if rng.uniform() < 0.3:                        # a stretch of another density
                    a = int(rng.integers(0, len(per)))
                    per[a:a + int(rng.integers(1, 60))] *= rng.choice([0.25, 3.0])
                fams.append(from_periods(np.clip(per, 3.0, None), rng.uniform(-100.0, 50.0)))
            lists[band] = fams
        utts.append(U(f"utt {i}", nf, lists))
    return Group(f"random {call}", band_f0, utts, f0_floor=40.0, f0_ceil=1000.0)


# ---- detection: raw candidates given --------------------------------------------------------------------------------------
DETECT_NCH = (12, 19, 20, 38, 39, 57, 58, 152, 203)


def detect_map(nch, seed):
    """[nch, frames] raw candidates: a run of 9, 10 and 11 bands from every band it fits at (band 0 voiced in front of the run
    at band 1, the run reaching nch - 2 closed by the forced zero -- with band nch - 1 voiced or not), band nch - 1 alone, ten
    voiced and one unvoiced in turn, a denormal run, -0.0 between two runs, a frame of zeros; lattice and off-lattice values"""
    rng = np.random.default_rng(seed)
    cols = []

    def col():
        cols.append(np.zeros(nch))
        return cols[-1]
    lattice = lambda n: rng.integers(8 * 60, 8 * 2000, n) / 8.0
    for length in (9, 10, 11):
        for st in range(1, nch - length):                      # the run ends at st + length - 1 <= nch - 2
            c = col()
            c[st:st + length] = lattice(length) if (st + length) % 2 else rng.uniform(60.0, 2000.0, length)
            if st == 1:
                c[0] = 100.0
            if st + length == nch - 1:                         # closed by the forced zero alone; and the same with band nch - 1 unvoiced
                c[nch - 1] = 100.0
                col()[:] = c
                cols[-1][nch - 1] = 0.0
    col()[nch - 1] = 100.0
    col()
    c = col()                                                  # the most runs a frame holds
    c[:] = lattice(nch)
    c[0::11] = 0.0
    c = col()
    c[1:11] = 1e-310
    if nch >= 23:
        c = col()
        c[1:nch - 1] = lattice(nch - 2)
        c[11] = -0.0
    return np.stack(cols, axis=1)


def random_map(nch, frames, seed):
    rng = np.random.default_rng(seed)
    raw = np.zeros((nch, frames))
    for i in range(frames):
        j = 0
        while j < nch:
            n = int(rng.choice([1, 3, 9, 10, 11, 14, 25]))
            if rng.uniform() < 0.6:
                raw[j:j + n, i] = rng.uniform(60.0, 2000.0, min(n, nch - j))
            j += n
    return raw


def group_detect(nch):
    def reach(u, o):
        n = candidates_of(u.raw)
        most = (nch - 1) // 11
        assert n.max() == most == o["nc"] and most <= zcap_of(nch), (n.max(), most)
        lengths = {ed - st for i in range(u.nf) for st, ed in frame_runs(u.raw[:, i])}
        assert ({9, 10, 11} if nch > 12 else {9, 10}) <= lengths              # (twelve bands: 1 .. 10 is the longest run there is)
        if nch == 152:                                         # a run across every edge of the 19-band fetch batches
            for edge in range(BATCH, nch - 1, BATCH):
                assert any(st < edge < ed for i in range(u.nf) for st, ed in frame_runs(u.raw[:, i]) if ed - st >= 10), edge
    raw = detect_map(nch, nch)
    return Group(f"detect {nch}", ladder(nch, 60.0) if nch < 60 else np.linspace(60.0, 2000.0, nch),
                 [U("map", raw.shape[1], raw=raw, reach=reach)], f0_floor=60.0, f0_ceil=2000.0, golden=nch <= 20)


def group_detect_nc():
    """nc is the largest count over the frames of an utterance: none anywhere (the cleared start), in frame 0, in frame nf - 1,
    in a frame of the last partial workgroup"""
    nch, nf = 38, 300
    one, three = np.zeros(nch), np.zeros(nch)
    one[3:14] = 200.0
    three[1:11], three[12:23], three[24:36] = 100.0, 200.0, 300.0

    def utt(name, top, want):
        raw = np.zeros((nch, nf))
        if top is not None:
            raw[:, 40], raw[:, top] = one, three
        return U(name, nf, raw=raw, reach=lambda u, o: o["nc"] == want or _fail(name, o["nc"]))
    return Group("detect nc", ladder(nch, 60.0), [utt("none", None, 0), utt("frame 0", 0, 3), utt("last frame", nf - 1, 3),
                                                  utt("partial workgroup", 270, 3)], f0_floor=60.0, f0_ceil=2000.0, golden=False)


def group_detect_random():
    return Group("detect random", np.linspace(60.0, 2000.0, 152), [U("200 frames", 200, raw=random_map(152, 200, 7))], f0_floor=60.0,
                 f0_ceil=2000.0)


GROUPS = {"counts": group_counts, "constant": group_constant, "glide": group_glide, "ends": group_ends, "ties": group_ties,
          "small lists": group_small_lists, "guess misses": group_guess_misses, "cap edge": group_cap_edge, "groups": group_groups,
          "detect nc": group_detect_nc, "detect random": group_detect_random}
GROUPS.update({f"limits {s}": (lambda s=s: group_limits(s)) for s in ("ceil", "ceil_out", "floor", "floor_out")})
GROUPS.update({f"random {i}": (lambda i=i: group_random(i)) for i in range(2)})
GROUPS.update({f"detect {n}": (lambda n=n: group_detect(n)) for n in DETECT_NCH})


def group(name):
    return cached(("harvest candidates group", name), GROUPS[name])


def case_group(be, name):
    hold(be, group(name))


def case_groups_are_their_lone_calls(be, ev_group):
    """the five ragged utterances in groups of ev_group (ev_u0 = 0, ev_group, ...) equal their lone calls bit for bit"""
    g = group("groups")
    want = expected(g)
    outs = hold(be, g, be.run_group(g, ev_group=ev_group), want)
    for i in ((0, 4) if ev_group != 2 else range(len(g.utts))):
        lone = be.run_group(g, only=[i])[0]
        assert same_bits(lone["raw"], outs[i]["raw"]) and same_bits(lone["cand"], outs[i]["cand"]) and lone["nc"] == outs[i]["nc"], i


# ---- compaction -------------------------------------------------------------------------------------------------------------
def compaction_case(name):
    """-> (nseg, seg_cap, ev_cap, lengths [lists][nseg]) for the 48 lists of one utterance of 12 bands"""
    rng = np.random.default_rng(sum(map(ord, name)))
    lists = 48
    if name == "2 segments":
        menu = [[1, 0], [0, 1], [0, 0], [3, 3], [3, 0], [2, 1], [3, 2]]
        return 2, 3, 5, [menu[i % len(menu)] for i in range(lists)]                    # 3 + 3 > ev_cap = 5: cut; 3 + 2 == ev_cap
    if name == "3 segments":
        menu = [[0, 2, 4], [4, 0, 2], [4, 2, 0], [0, 0, 0], [0, 0, 1], [4, 4, 4], [0, 4, 0], [4, 4, 3]]
        return 3, 4, 11, [menu[i % len(menu)] for i in range(lists)]                   # 12 > ev_cap = 11; 11 == ev_cap
    nseg, seg_cap = int(name.split()[0]), 64
    totals = [1, 2047, 2048, 2049, 2100, 0, 777]                                       # ev_cap = 2049: one equal, one cut
    lengths = []
    for i in range(lists):
        total, l = totals[i % len(totals)], np.zeros(nseg, dtype=np.int64)
        full, rest = divmod(total, seg_cap)
        block = [seg_cap] * full + ([rest] if rest else [])
        if i % 4 == 0:                                                                 # a block in the middle: head and tail empty
            at = (nseg - len(block)) // 2
            l[at:at + len(block)] = block
        elif i % 4 == 1:                                                               # sprinkled over all segments, many of them empty
            left = total
            while left:
                s = int(rng.integers(0, nseg))
                n = min(int(rng.integers(1, seg_cap + 1)), seg_cap - l[s], left)
                l[s] += n
                left -= n
        elif i % 4 == 2:                                                               # packed at the tail: the last segments (past 256 where there are)
            l[nseg - len(block):] = block
        else:                                                                          # packed at the head
            l[:len(block)] = block
        lengths.append(l.tolist())
    return nseg, seg_cap, 2049, lengths


COMPACTIONS = ("2 segments", "3 segments", "256 segments", "257 segments", "300 segments")


def compaction_arrays(name):
    nseg, seg_cap, ev_cap, lengths = compaction_case(name)
    lists = len(lengths)
    seg_events, seg_count = np.full((1, lists, nseg, seg_cap), 1e300), np.zeros((1, lists, nseg), dtype=np.int32)
    want = []
    for i, ls in enumerate(lengths):
        whole = 0.5 + i / 64.0 + np.arange(sum(ls), dtype=np.float64)
        at = 0
        for s, n in enumerate(ls):
            seg_events[0, i, s, :n], seg_count[0, i, s] = whole[at:at + n], n
            at += n
        want.append(whole[:ev_cap])
    return seg_events, seg_count, ev_cap, want


def case_compaction(be, name):
    """stage 1 alone: every list is its segments concatenated in order, cut at ev_cap; what lies past ev_count is not touched"""
    nseg, seg_cap, ev_cap, lengths = compaction_case(name)
    seg_events, seg_count, ev_cap, want = compaction_arrays(name)
    # what the case was built to reach
    flat = [l for l in lengths]
    assert any(sum(l) == 0 for l in flat) and any(l[0] == 0 < sum(l) for l in flat) and any(l[-1] == 0 < sum(l) for l in flat)
    assert any(0 in l[1:-1] for l in flat if sum(l)) or nseg == 2
    assert any(max(l) == seg_cap for l in flat) and any(sum(l) == ev_cap for l in flat) and any(sum(l) > ev_cap for l in flat)
    if nseg > 3:
        assert {1, 2047, 2048, 2049} <= {sum(l) for l in flat} and (nseg > 256) == (name != "256 segments")
    h = be.run([10], np.full(12, 100.0), seg_events=seg_events, seg_count=seg_count, ev_cap=ev_cap, stages=1)
    for i, w in enumerate(want):
        assert h["ev_count"][0, i] == len(w), (name, i, int(h["ev_count"][0, i]), len(w))
        assert same_bits(h["events"][0, i, :len(w)], w), (name, i)
        assert np.all(h["events"][0, i, len(w):] == SENTINEL), (name, i, "written past ev_count")
    assert np.all(h["raw"] == SENTINEL) and np.all(h["cand"] == SENTINEL) and np.all(h["nc"] == -7), "stage 1 alone wrote more"


def case_compacted_lists_go_on(be):
    """lists cut into three segments, compacted, interpolated and detected equal the one-segment call on the whole lists; in two
    groups of utterances"""
    g = group("groups")
    utts = g.utts[1:4]
    want = expected(g)[1:4]
    nfb, nch = [u.nf for u in utts], g.nch
    packed = [g.packed(u) for u in utts]
    seg_cap = g.ev_cap
    seg_events, seg_count = np.full((len(utts), nch * 4, 3, seg_cap), 1e300), np.zeros((len(utts), nch * 4, 3), dtype=np.int32)
    for i, (edges, counts) in enumerate(packed):
        for l in range(nch * 4):
            e = edges.reshape(nch * 4, -1)[l, :counts.reshape(-1)[l]]
            n = len(e)
            cut = ([0, n // 5, n // 5, n], [0, 0, n // 2, n], [0, n // 3, n, n])[l % 3]     # an empty segment in the middle, at the head, at the tail
            for s in range(3):
                part = e[cut[s]:cut[s + 1]]
                seg_events[i, l, s, :len(part)], seg_count[i, l, s] = part, len(part)
    h = be.run(nfb, g.band_f0, seg_events=seg_events, seg_count=seg_count, ev_cap=g.ev_cap, ev_group=2, stages=7, afs=g.afs,
               f0_floor=g.f0_floor, f0_ceil=g.f0_ceil)
    zcap = zcap_of(nch)
    for i, (u, w) in enumerate(zip(utts, want)):
        edges, counts = packed[i]
        assert np.array_equal(h["ev_count"][i], counts.reshape(-1)), u.name
        for l in range(nch * 4):
            n = counts.reshape(-1)[l]
            assert same_bits(h["events"][i, l, :n], edges.reshape(nch * 4, -1)[l, :n]) and np.all(h["events"][i, l, n:] == SENTINEL)
        assert same_bits(h["raw"][i, :, :u.nf], w["raw"]) and same_bits(h["cand"][i, :u.nf, :zcap], w["cand"][:, :zcap]), u.name
        assert h["nc"][i] == w["nc"]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    """a refusal names the argument and writes nothing"""
    g = group("counts")
    utts = g.utts[:1]
    edges, counts = g.packed(utts[0])
    base = dict(seg_events=edges.reshape(1, g.nch * 4, 1, g.ev_cap), seg_count=counts.reshape(1, g.nch * 4, 1), ev_cap=g.ev_cap, stages=6)

    def refused(word, data=None, **override):
        rc, d, _ = be.call([utts[0].nf], g.band_f0, **{**base, **(data or {})}, override=override)
        assert rc != 0 and word in be.error(), (word, override, rc, be.error())
        for k in ("raw", "cand", "events"):
            assert np.all(be.host(d[k]) == SENTINEL), (word, k, "written by a refused call")
        assert np.all(be.host(d["nc"]) == -7) and np.all(be.host(d["ev_count"]) == -7)
    refused("nch", nch=11)
    refused("nch", nch=366)
    refused("band_f0", band_f0=(C.c_double * g.nch)(*([200.0] * (g.nch - 1) + [0.0])))
    refused("band_f0", band_f0=None)
    refused("ev_cap", ev_cap=0)
    refused("seg_cap", seg_cap=0)
    refused("seg_cap", seg_cap=g.ev_cap - 1)
    refused("nseg", nseg=0)
    refused("ev_group", ev_group=0)
    refused("stages", stages=8)
    refused("stages", stages=0)
    refused("stages", stages=2, nseg=2)
    refused("fb_stride", fb_stride=((utts[0].nf + 7) & ~7) + 8)
    refused("maxc", maxc=maxc_of(g.nch) + 7)
    refused("nfb", nfb=(C.c_int * 1)(0))
    for k in ("seg_events", "seg_count", "raw", "cand", "nc"):
        refused(k, **{k: None})
    refused("events", stages=7, nseg=2, events=None)
    over = counts.copy()
    over[3, 2] = g.ev_cap + 1
    refused("seg_count", data=dict(seg_count=over.reshape(1, g.nch * 4, 1)))
    rc, d, _ = be.call([utts[0].nf], g.band_f0, **base)
    assert rc == 0, be.error()
    before = np.array(be.host(d["raw"]))
    rc, _, _ = be.call([utts[0].nf], g.band_f0, **base, override=dict(raw=be.ptr(d["raw"]), cand=be.ptr(d["raw"])))
    assert rc != 0 and "overlaps" in be.error(), be.error()
    assert same_bits(be.host(d["raw"]), before)
