"""Harvest's contour stage alone (include/world_hip.h: world_hip_probe_harvest_contour -- hv_prune and launch_harvest_contour
on candidates the caller made up): the cases tests/test_harvest_contour_cpu.py runs on the host emulation and
tests/test_harvest_contour_gpu.py on the card, as functions of a backend.

The comparators.  R = the reference's own RemoveUnreliableCandidates / FixStep1 .. 4 / SmoothF0Contour (oracle/_ref/
libworld_ref_contour.so: oracle/harvest_contour_ref.cpp includes the reference's harvest.cpp where it lies), O = the oracle's
restatement (world_oracle.c: wo_harvest_contour), G = R's contours recorded in tests/golden/harvest_contour.npz
(tests/golden/make_golden_harvest_contour.py).  expected() asserts R == O == G bit for bit wherever R is built (O == G
elsewhere) and hands out O's, with O's branch counters (world_oracle.h: WO_HC_*).

The maps.  Unless a case says otherwise F0 values lie on a 1/8 Hz lattice and scores are multiples of 2^-10, so every sum, tie
and distance is exact in any order: a disagreement is logic, not rounding.  What a map is made of:
  track     the same F0 in one slot over consecutive frames.  FixStep1 drops the first frame of a run (no predecessor to
            extrapolate from), so a track on frames a .. b is the step-2 section a+1 .. b, and Extend's backward walk picks
            frame a up again from the candidates.
  fodder    candidates that Extend can follow but that never form a section themselves: every frame holds two values a few
            per cent apart whose scores alternate, so the base pick zigzags and FixStep1 drops every frame of it, while
            RemoveUnreliableCandidates keeps both (each has its like next door).
  ramp-in   v/2, v/2, 3v/4 in the three frames before a track of v: the line through v/2 and 3v/4 passes through v, so
            FixStep1 keeps the track's FIRST frame, and 3v/4 lies outside Extend's 18 %: a section of exactly the track.
Every case states what it was built to reach -- counters of O, sections of O's contours -- and hold() asserts that before
anything of the code under test is looked at: a case that stops reaching its branch fails.

What is asserted of the code under test (hold()): pruned candidates and scores, the step-2 and step-3 contours, step 4 outside
the bridged gaps, the frames at frame_period relative to basic_f0: bit for bit.  Step 4's bridged frames and the smoothed
contour: util.assert_f0_tight (1e-10).  The smoothed contour also, against the long-double oracle W fed the SAME step-4
contour (the backend's own), util.assert_accurate on the voiced frames of a batch.  The section table the last launch leaves:
the voiced runs of the backend's step-4 contour.  Rows past nfb[u] and frames past n_frames[u]: untouched."""
import ctypes as C
import os
import zlib

import numpy as np

import backends
import util
from backends import cached, same_bits

GOLDEN = os.path.join(util.GOLDEN, "harvest_contour.npz")
SENTINEL = backends.SENTINEL_F64
OUT_ROWS = ("step2", "step3", "step4", "basic_f0")
GOLDEN_KEYS = ("step2", "step3", "step4", "smooth")
TILE = 4096                  # harvest_contour.hip: kStepTile, the frames hc_step12 evaluates per trip (margin 6 either side)
MERGE_LDS_SECTIONS = 1024    # harvest_contour.hip: kMergeLdsSections
SMOOTH_LDS_FRAMES = 5228     # harvest_contour.hip: kSmoothLdsMax: a longer section is filtered out of HBM


# ---- maps -----------------------------------------------------------------------------------------------------------------
class U:
    """one utterance: nf frames at 1 ms, nc candidates per frame (7 nc slots)"""

    def __init__(self, name, nf, nc, reach=None, sections3=None, counters=None):
        self.name, self.nf, self.nc, self.nslot = name, nf, nc, 7 * nc
        self.cand, self.score = np.zeros((nf, 7 * nc)), np.zeros((nf, 7 * nc))
        self.reach = reach                 # callable(o): further assertions on the oracle's outputs
        self.sections3 = sections3         # the voiced sections the oracle's step-3 contour must have, [(first, last)]
        self.counters = dict(counters or {})   # {counter: the least the oracle must count}

    def put(self, f, slot, f0, sc=0.5):
        assert 0 <= f < self.nf and 0 <= slot < self.nslot and self.cand[f, slot] == 0, (self.name, f, slot)
        self.cand[f, slot], self.score[f, slot] = f0, sc
        return self

    def track(self, a, b, f0, slot=0, sc=0.5):
        """frames a .. b inclusive"""
        for f in range(a, b + 1):
            self.put(f, slot, f0, sc)
        return self

    def fodder(self, a, b, lo, hi, slots=(1, 2), holes=()):
        """frames a .. b inclusive but `holes`: lo and hi in the two slots, the top score alternating between them"""
        for f in range(a, b + 1):
            if f in holes:
                continue
            self.put(f, slots[0], lo, 0.25 if f % 2 else 0.125)
            self.put(f, slots[1], hi, 0.125 if f % 2 else 0.25)
        return self

    def exact(self, a, b, v, slot=0, sc=0.5):
        """a section of exactly frames a .. b of v (the ramp-in above); uses frames a-3 .. a-1 and slot + 1"""
        assert a >= 4 and v % 40 == 0
        self.put(a - 3, slot, v / 2, sc).put(a - 2, slot, v / 2, sc).put(a - 2, slot + 1, v * 31 / 40, sc / 2).put(a - 1, slot, 0.75 * v, sc)
        return self.track(a, b, v, slot, sc)

    def lattice(self):
        on = self.cand * 8
        return bool(np.all(on == np.round(on)) and np.all(self.score * 1024 == np.round(self.score * 1024)))


class Group:
    """utterances that go through the probe in one call"""

    def __init__(self, name, maxc, utts, frame_period=5.0, lattice=True, golden=True):
        self.name, self.maxc, self.utts, self.frame_period, self.golden = name, maxc, list(utts), frame_period, golden
        assert maxc % 7 == 0 and all(u.nslot <= maxc for u in self.utts), name
        assert len({u.name for u in self.utts}) == len(self.utts), name
        if lattice:
            assert all(u.lattice() for u in self.utts), name


def _fail(*why):
    raise AssertionError(why)


def runs(contour, force_ends=True):
    """[(first, last)] of the voiced runs, GetBoundaryList's (harvest.cpp:727-743: frames 0 and nf - 1 count as unvoiced)"""
    v = np.asarray(contour) > 0
    if force_ends and v.size:
        v = v.copy()
        v[0] = v[-1] = False
    d = np.diff(np.concatenate([[0], v.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


# ---- the comparators ------------------------------------------------------------------------------------------------------
def oracles():
    def make():
        from oracle import loader
        return loader.PortOracle(), loader.WideOracle(), (loader.RefContour() if loader.RefContour.available() else None)
    return cached(("harvest contour oracles",), make)


def golden():
    return cached(("harvest contour golden",), lambda: dict(np.load(GOLDEN)))


def digest(o):
    """the golden file's record of a large or random map: CRC-32 of each contour's bytes"""
    return np.array([zlib.crc32(np.ascontiguousarray(o[k]).tobytes()) for k in GOLDEN_KEYS], dtype=np.int64)


def expected(group):
    """per utterance the oracle's outputs (and counters), after R == O == G and after the case's own reach assertions"""
    def make():
        port, _, ref = oracles()
        g = golden()
        out = []
        for u in group.utts:
            o = port.harvest_contour(u.cand, u.score, group.frame_period)
            what = f"{group.name}/{u.name}"
            if ref is not None:
                r = ref.harvest_contour(u.cand, u.score)
                for k in r:
                    assert same_bits(r[k], o[k]), f"{what}: the oracle's {k} is not the reference's"
            if group.golden:
                for k in GOLDEN_KEYS:
                    assert same_bits(g[f"{what}/{k}"], o[k]), f"{what}: the oracle's {k} is not the recorded reference's"
            else:
                assert np.array_equal(g[f"{what}/crc"], digest(o)), f"{what}: the oracle's contours are not the recorded reference's"
            for name, least in u.counters.items():
                assert o["counters"][name] >= least, f"{what}: built to reach {name} >= {least}, the oracle counts {o['counters']}"
            if u.sections3 is not None:
                assert runs(o["step3"]) == list(u.sections3), f"{what}: step 3 sections {runs(o['step3'])}, built for {u.sections3}"
            if u.reach:
                u.reach(o)
            for a in o.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out.append(o)
        return out
    return cached(("harvest contour expected", group.name), make)


# ---- the backend ----------------------------------------------------------------------------------------------------------
class Backend(backends.Backend):
    exact_ties = True        # the emulator's one lane compares the distances themselves; the GPU's packed key: GpuBackend

    def shapes(self, group):
        nfb = [u.nf for u in group.utts]
        frames = [int((f - 1) / group.frame_period) + 1 for f in nfb]
        return nfb, frames, (max(nfb) + 7) & ~7, max(nfb) // 2 + 4, max(frames)

    def call(self, group, **change):
        """the probe on a group -> (return code, the device arrays by name); `change` overrides arguments (refusals)"""
        nfb, frames, stride, sec_cap, f_stride = self.shapes(group)
        n, maxc = len(group.utts), group.maxc
        cand, score = np.zeros((n, stride, maxc)), np.zeros((n, stride, maxc))
        for i, u in enumerate(group.utts):
            cand[i, :u.nf, :u.nslot], score[i, :u.nf, :u.nslot] = u.cand, u.score
            cand[i, :u.nf, u.nslot:] = score[i, :u.nf, u.nslot:] = 1.0     # slots past 7 nc are nobody's: never looked at
            cand[i, u.nf:], score[i, u.nf:] = 300.0, 1.0                      # nor are rows past nfb
        d = dict(cand=self.dev(cand), score=self.dev(score))
        for k, shape in (("pruned_cand", cand.shape), ("pruned_score", cand.shape), ("step2", (n, stride)), ("step3", (n, stride)),
                         ("step4", (n, stride)), ("basic_f0", (n, stride)), ("tpos", (n, f_stride)), ("f0", (n, f_stride))):
            d[k] = self.dev(np.full(shape, SENTINEL))
        d["sec_n"], d["sec"] = self.dev(np.full((n, 2), -7, dtype=np.int32)), self.dev(np.full((n, 6, sec_cap), -7, dtype=np.int32))
        a = dict(n_utt=n, nfb=(C.c_int * n)(*nfb), nc=(C.c_int * n)(*[u.nc for u in group.utts]), maxc=maxc, fb_stride=stride,
                 frame_period=group.frame_period, f_stride=f_stride, sec_cap=sec_cap, **{k: self.ptr(v) for k, v in d.items()})
        a.update(change)
        rc = self.lib.world_hip_probe_harvest_contour(
            self.ctx, a["n_utt"], a["nfb"], a["nc"], a["maxc"], a["fb_stride"], a["cand"], a["score"], a["frame_period"],
            a["f_stride"], a["pruned_cand"], a["pruned_score"], a["step2"], a["step3"], a["step4"], a["sec_cap"],
            a["sec_n"], a["sec"], a["basic_f0"], a["tpos"], a["f0"])
        return rc, d, (cand, score)

    def run(self, group):
        """-> per utterance {name: array}, trimmed to the utterance; what lies past it must be as it was"""
        rc, d, (cand, score) = self.call(group)
        assert rc == 0, self.error()
        h = {k: self.host(v) for k, v in d.items()}
        assert same_bits(h["cand"], cand) and same_bits(h["score"], score), "the probe wrote into its inputs"
        nfb, frames, *_ = self.shapes(group)
        out = []
        for i, u in enumerate(group.utts):
            what = f"{group.name}/{u.name}"
            o = {k: h[k][i, :u.nf] for k in OUT_ROWS}
            for k in OUT_ROWS + ("pruned_cand", "pruned_score"):
                assert np.all(h[k][i, u.nf:] == SENTINEL), f"{what}: {k} written past frame nfb"
            for k in ("tpos", "f0"):
                o[k] = h[k][i, :frames[i]]
                assert np.all(h[k][i, frames[i]:] == SENTINEL), f"{what}: {k} written past its last frame"
            for k in ("pruned_cand", "pruned_score"):
                o[k] = h[k][i, :u.nf, :u.nslot]
                if u.nc == 0:
                    assert np.all(h[k][i] == SENTINEL), f"{what}: {k} written for an utterance without candidates"
            o["sec_n"], o["sec"] = h["sec_n"][i], h["sec"][i]
            out.append(o)
        return out


def hold(be, group, outs=None, want=None):
    """the assertions of the module's docstring on one group"""
    want = expected(group) if want is None else want
    outs = be.run(group) if outs is None else outs
    port, wide, ref = oracles()
    acc_h, acc_r, acc_w = [], [], []
    for u, o, w in zip(group.utts, outs, want):
        what = f"{group.name}/{u.name}"
        for k in ("pruned_cand", "pruned_score", "step2", "step3"):
            assert same_bits(o[k], w[k]), f"{what}: {k} differs at {np.argwhere(o[k] != w[k])[:8].tolist()}"
        bridged = (w["step3"] == 0) & (w["step4"] > 0)
        assert np.array_equal(o["step4"] > 0, w["step4"] > 0), f"{what}: step 4 voicing"
        assert same_bits(o["step4"][~bridged], w["step4"][~bridged]), f"{what}: step 4 outside the bridged gaps"
        if bridged.any():
            util.assert_f0_tight(f"{what} step 4 bridges", o["step4"][bridged], w["step4"][bridged])
        # the section table the last launch leaves: the voiced runs of step 4 (the ends are not forced there: :1092-1094)
        secs = runs(o["step4"], force_ends=False)
        assert o["sec_n"][0] == len(secs), f"{what}: sec_n {o['sec_n']}, step 4 has {len(secs)} sections"
        assert list(zip(o["sec"][0, :len(secs)].tolist(), o["sec"][1, :len(secs)].tolist())) == secs, what
        # the smoother
        assert np.array_equal(o["basic_f0"] > 0, w["smooth"] > 0), f"{what}: voicing of the smoothed contour"
        if (w["smooth"] > 0).any():
            util.assert_f0_tight(f"{what} smooth", o["basic_f0"], w["smooth"])
            v = o["step4"] > 0
            acc_h.append(o["basic_f0"][v])
            acc_r.append((ref or port).smooth_f0(o["step4"])[v])
            acc_w.append(wide.smooth_f0(o["step4"])[v])
        else:
            assert np.all(o["basic_f0"] == 0)
        # the frames at frame_period
        assert same_bits(o["tpos"], w["tpos"]), f"{what}: tpos"
        src = np.minimum(u.nf - 1, np.floor(w["tpos"] * 1000.0 + 0.5).astype(np.int64))
        assert same_bits(o["f0"], o["basic_f0"][src]), f"{what}: f0 is not basic_f0 at the frames' nearest milliseconds"
    if acc_h:
        util.assert_accurate(f"harvest contour smooth {group.name} ({type(be).__name__})", np.concatenate(acc_h), np.concatenate(acc_r),
                             np.concatenate(acc_w))
    return outs


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _mask_reach(keep, drop):
    def reach(o):
        for f, s in keep:
            assert o["pruned_cand"][f, s] != 0, ("kept", f, s)
        for f, s in drop:
            assert o["pruned_cand"][f, s] == 0, ("pruned", f, s)
    return reach


def group_prune():
    """RemoveUnreliableCandidates: a like in the next frame only, the previous only, neither; the 5 % boundary and an ulp
    either side; frames 0 and nf - 1; no candidates at all (nc = 0); the base pick: first of equals across lanes, a frame
    whose scores are all 0"""
    up, down = float(np.nextafter(210.0, np.inf)), float(np.nextafter(210.0, -np.inf))
    u = U("neighbours", 120, 2, reach=_mask_reach(keep=[(10, 0), (11, 3), (30, 1), (31, 5), (50, 1), (51, 5), (41, 5), (0, 4), (119, 6)],
                                                  drop=[(20, 2), (40, 1), (60, 0), (62, 0)]))
    u.put(10, 0, 200).put(11, 3, 205)                 # next only / previous only
    u.put(20, 2, 200)                                 # neither
    u.put(30, 1, 200).put(31, 5, 210)                 # |200 - 210| / 200 == 0.05: kept
    u.put(40, 1, 200).put(41, 5, up)                  # an ulp beyond: 200 goes (210+ itself has 200 within 4.8 %)
    u.put(50, 1, 200).put(51, 5, down)
    u.put(60, 0, 200).put(62, 0, 200)                 # two frames away is not a neighbour
    u.put(0, 4, 200).put(119, 6, 200)                 # the ends are never pruned
    # the base pick inside tracks, where steps 1 and 2 pass it on: equal top scores on different values, the lowest slot's wins
    t = U("base pick", 80, 2, sections3=[(10, 30), (40, 70)])
    t.track(10, 30, 200, slot=9).track(10, 30, 300, slot=2)            # slot 2 first: 300
    t.track(40, 70, 240, slot=0).track(40, 70, 120, slot=13)
    t.reach = lambda o: (np.all(o["step2"][11:31] == 300) and np.all(o["step2"][41:71] == 240)) or _fail("base")
    z = U("all scores zero", 60, 1, reach=lambda o: runs(o["step2"]) == [(6, 19), (31, 50)] or _fail(runs(o["step2"])))
    z.track(5, 19, 200).track(20, 29, 200, sc=0.0).track(30, 50, 200)   # candidates all along, no score in the middle: no base there
    return Group("prune", 14, [u, t, z, U("no candidates", 37, 0, reach=lambda o: None)], lattice=False)


def group_prune_wide():
    """the base pick past 64 slots: equal top scores in slots one lane holds (64 apart) and in different lanes"""
    t = U("base pick wide", 90, 10, sections3=[(10, 30), (40, 70)])
    t.track(10, 30, 200, slot=69).track(10, 30, 300, slot=5)             # the same lane: 300
    t.track(40, 70, 240, slot=6).track(40, 70, 120, slot=69).track(40, 70, 480, slot=65)
    t.reach = lambda o: (np.all(o["step2"][11:31] == 300) and np.all(o["step2"][41:71] == 240)) or _fail("base")
    return Group("prune wide", 70, [t])


def group_step12():
    """FixStep1's 0.8 % against the extrapolation and against the previous frame, inside and outside; a[i-2] == 2 a[i-1];
    voiced frames 0 and 1; runs with end - start 5 and 6; a run that ends at nf - 2 and one that reaches nf - 1"""
    def at(f, v):
        return lambda o: (o["step2"][f] == v) or _fail((f, v, o["step2"][f - 3:f + 4]))

    def both(*fs):
        return lambda o: [f(o) for f in fs]
    us = []
    # previous == the one before: both quotients are (x - 250) / 250; 2 / 250 == 0.008 is not a jump, 2.125 / 250 is
    us.append(U("0.8% inside", 60, 1, reach=at(30, 252.0)).track(5, 29, 250).put(30, 0, 252).track(31, 55, 250))
    us.append(U("0.8% outside", 60, 1, reach=at(30, 0.0)).track(5, 29, 250).put(30, 0, 252.125).track(31, 55, 250))
    # 240, 250, x: the line says 260.  262 is within 0.8 % of it though 4.8 % from 250; 252 is within 0.8 % of 250 though 3 % from
    # the line; 252.125 is neither
    for name, x, keep in (("by the line", 262.0, True), ("by the previous", 252.0, True), ("by neither", 252.125, False)):
        u = U(f"0.8% {name}", 60, 1, reach=at(30, x if keep else 0.0))
        us.append(u.track(5, 27, 250).put(28, 0, 240).put(29, 0, 250).put(30, 0, x).track(31, 55, x))
    # 400, 200, 200: the line through 400 and 200 is 0 -- the reference divides by it: inf > 0.008, the previous frame decides
    us.append(U("line through zero", 60, 1, reach=both(at(30, 200.0), at(31, 200.0))).track(5, 28, 400).track(29, 55, 200))
    us.append(U("voiced frames 0 and 1", 40, 1, reach=both(at(0, 0.0), at(1, 0.0), at(2, 200.0))).track(0, 30, 200))
    # a track of n frames is a step-1 run of n - 1: end - start = n - 2
    us.append(U("run of 5", 40, 1, reach=lambda o: runs(o["step2"]) == [] or _fail()).track(10, 16, 200))
    us.append(U("run of 6", 40, 1, reach=lambda o: runs(o["step2"]) == [(11, 17)] or _fail()).track(10, 17, 200))
    us.append(U("ends at nf-2", 40, 1, reach=lambda o: runs(o["step2"]) == [(21, 38)] or _fail()).track(20, 38, 200))
    us.append(U("reaches nf-1", 40, 1, reach=both(at(39, 200.0), lambda o: runs(o["step2"]) == [(21, 38)] or _fail())).track(20, 39, 200))
    for nf in (1, 2, 3, 7):
        us.append(U(f"nfb {nf}", nf, 1).track(0, nf - 1, 200))
    return Group("step12", 7, us)


def group_tile_edge():
    """runs with end - start 5 (dropped) and 6 (kept) at every position across hc_step12's tile edge and its six-frame margin"""
    us = []
    for length, kept in ((7, False), (8, True)):
        for d in range(-9, 3):
            a = TILE + d
            u = U(f"track of {length} from tile{d:+d}", TILE + 40, 1)
            u.track(a, a + length - 1, 400)
            u.reach = (lambda a, n, kept: lambda o: runs(o["step2"]) == ([(a + 1, a + n - 1)] if kept else []) or _fail(runs(o["step2"])))(a, length, kept)
            us.append(u)
    return Group("tile edge", 7, us, golden=False)


STOPS = (0, 1, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96, 99, 100)


def _extend_utts(nc, tag):
    """Extend on one route (7 nc <= 64: a slot per lane, a ring of four; beyond: four slots per lane, a ring of two): a section
    of 200 Hz on frames 150 .. 170 with fodder on both sides that Extend follows, every step an exact tie between 2 Hz below
    and 2 Hz above the previous pick (the later slot wins, so the walk alternates 202, 200, ...).  After `stop` frames the
    fodder has a hole of four frames (the walk ends) or of three (it goes on to its reach of 100 frames, one more looked at)."""
    nslot = 7 * nc
    lane_pair = (3, 3 + 64) if nslot > 64 else None
    us = []
    for hole in (4, 3):
        for stop in STOPS:
            if hole == 3 and stop > 90:
                continue
            u = U(f"{tag} hole of {hole} after {stop}", 330, nc)
            sa, sb = (lane_pair if lane_pair and stop % 2 else (nslot - 6, nslot - 2))          # the same lane / two lanes
            u.track(150, 170, 200, slot=0, sc=0.75)
            for side in (+1, -1):
                origin = 170 if side > 0 else 150
                for k in range(1, 112):
                    f = origin + side * k
                    if stop < k <= stop + hole or not 0 < f < u.nf - 1:
                        continue
                    # the walk stands on 200 before odd steps, on 202 before even ones; the later slot holds what it must take
                    lo, hi = (198.0, 202.0) if k % 2 else (204.0, 200.0)
                    u.put(f, sa, lo, 0.25 if k % 4 < 2 else 0.0625).put(f, sb, hi, 0.125)
            reached = stop if hole == 4 else 101
            u.reach = (lambda reached, hole: lambda o: _reach_extend(o, reached, hole))(reached, hole)
            # (a hole that begins within four frames of the reach ends the walk by the reach, not by its fourth miss)
            u.counters = {"extend_tie": reached, "extend_stopped": 2 if hole == 4 and stop <= 96 else 0,
                          "extend_full_reach": 0 if hole == 4 else 2, "extend_hit_after_3": 0 if hole == 4 else 2}
            us.append(u)
    return us


def _reach_extend(o, reached, hole):
    assert runs(o["step2"]) == [(151, 170)], runs(o["step2"])
    v = np.flatnonzero(o["step3"] > 0)
    # (forwards the walk looks at 101 frames from the section's last; backwards at 101 from its first, the track's own one first)
    assert v.min() == 150 - min(reached, 100) and v.max() == 170 + reached, (v.min(), v.max(), reached)
    k = np.arange(1, min(reached, 20) + 1)
    k = k[o["step3"][170 + k] > 0]
    assert np.all(o["step3"][170 + k] == np.where(k % 2, 202.0, 200.0)), "the later slot did not win the ties"


def group_extend(nc):
    return Group(f"extend nslot {7 * nc}", 7 * nc, _extend_utts(nc, f"nslot {7 * nc}"), golden=False)


def group_extend_edges():
    """a candidate exactly at 18 % (100 -> 118 and 82) and an ulp outside; sections that start at frames 1 .. 3 and end at
    nf - 2, where `last` is clamped; both routes"""
    us = []
    for nc in (2, 14):
        for name, c, hit in (("118", 118.0, True), ("82", 82.0, True), ("118+", float(np.nextafter(118.0, np.inf)), False),
                             ("82-", float(np.nextafter(82.0, -np.inf)), False)):
            u = U(f"nslot {7 * nc} 100 to {name}", 120, nc, counters={"extend_at_range": 1} if hit else {})
            u.track(20, 60, 100, slot=1).put(61, 7 * nc - 1, c, 0.25).put(62, 7 * nc - 1, c, 0.25)
            u.reach = (lambda c, hit: lambda o: (o["pruned_cand"][61].max() == c and o["step3"][61] == (c if hit else 0.0))
                       or _fail((c, hit, o["step3"][58:64])))(c, hit)
            us.append(u)
        for a in (1, 2, 3):
            u = U(f"nslot {7 * nc} from frame {a} to nf-2", 60, nc, sections3=[(max(a - 1, 1), 58)])
            us.append(u.track(a - 1, 59, 200, slot=7 * nc - 3))
    return Group("extend edges", 98, us, lattice=False)


def group_extend_sub():
    """ExtendSub: 220 Hz with end - start exactly 10 (2200 / 220 < 10 is false: dropped) and 11; a dropped section with kept
    ones behind it (the swap-compaction); a section kept only by the mean carried over; every section dropped"""
    same = lambda o: same_bits(o["step3"], o["step2"]) or _fail("step 3 is not step 2")
    us = [U("220 Hz end-start 10", 60, 1, reach=same, counters={"rejected": 1, "sections": 1}).track(20, 30, 220),
          U("220 Hz end-start 11", 60, 1, sections3=[(20, 31)], counters={"kept": 1}).track(20, 31, 220),
          U("dropped then kept", 160, 1, sections3=[(40, 80), (100, 140)], counters={"rejected": 1, "compacted": 2})
          .track(10, 20, 220).track(40, 80, 220).track(100, 140, 330),
          # mean 220 carried: (220 + 11 * 200) / 11 = 220, 2200 / 220 = 10 < 11: kept.  On its own: 2200 / 200 = 11 < 11: dropped
          U("kept by the carried mean", 120, 1, sections3=[(10, 50), (70, 81)], counters={"kept": 2}).track(10, 50, 220).track(70, 81, 200),
          U("200 Hz end-start 11 alone", 120, 1, reach=same, counters={"rejected": 1, "sections": 1}).track(70, 81, 200),
          U("every section dropped", 120, 1, counters={"rejected": 3}, reach=lambda o: (same_bits(o["step3"], o["step2"]) and len(runs(o["step2"])) == 3)
            or _fail()).track(10, 19, 200).track(40, 49, 200).track(70, 79, 200)]
    return Group("extend sub", 7, us)


def group_merge():
    """MergeF0: disjoint; contained; overlaps decided either way and by equal scores; a later section whose backward walk starts
    before section 0's start (channel 0 is written first and met again at its sorted place)"""
    us = []
    # two sections 200 and 300 Hz, nine frames of fodder for both between them: the first walks forwards over it, the second back
    for name, sa, sb, counter in (("s1 > s2", 0.5, 0.25, "merge_s1_gt"), ("s1 == s2", 0.25, 0.25, "merge_s1_eq"), ("s1 < s2", 0.25, 0.5, "merge_s1_lt")):
        u = U(f"overlap {name}", 160, 2, counters={counter: 1})
        u.track(40, 80, 200, slot=0, sc=0.75).track(90, 130, 300, slot=0, sc=0.75)
        for f in range(81, 90):
            u.put(f, 1, 196.0 if f % 2 else 204.0, sa).put(f, 2, 296.0 if f % 2 else 304.0, sb)
            u.put(f, 3, 100.0 if f % 2 else 104.0, 0.875)              # the base pick there: a zigzag FixStep1 drops
        us.append(u)
    us.append(U("disjoint", 160, 2, counters={"merge_disjoint": 1}, sections3=[(40, 80), (100, 130)]).track(40, 80, 200).track(100, 130, 300))
    # 230 Hz for ten frames inside a long run of fodder around 200 that a 200 Hz section walks along: the short section's
    # walks follow the same fodder both ways and end where the long one's do
    u = U("contained", 260, 2, counters={"merge_contained": 1})
    u.track(40, 80, 200, slot=0, sc=0.75).fodder(81, 170, 196.0, 204.0, slots=(1, 2)).track(120, 135, 230, slot=3, sc=0.875)
    us.append(u)
    # section 0 (200 Hz, frames 120 ..) has nothing before it; section 1 (230 Hz, later) walks back over fodder that begins
    # before section 0: sorted by start it comes first, and channel 0 is merged again behind it
    u = U("out of order", 300, 2, counters={"merge_out_of_order": 1})
    u.track(120, 150, 100, slot=0, sc=0.75).fodder(60, 199, 226.0, 234.0, slots=(1, 2)).track(200, 240, 230, slot=3, sc=0.875)
    us.append(u)
    return Group("merge", 14, us)


def _many_sections(nf):
    """400 and 600 Hz in turns of eight frames: FixStep1 drops the first frame of every turn, seven voiced and one unvoiced
    frame over and over -- the most sections an utterance can hold -- and every section takes its first frame back"""
    u = U(f"{nf} frames of eight-frame turns", nf, 1)
    for k, a in enumerate(range(1, nf - 9, 8)):
        u.track(a, a + 7, 400.0 if k % 2 else 600.0, slot=k % 7)
    return u


def group_many_sections():
    big, small = _many_sections(9000), _many_sections(4000)
    big.counters = {"sections": MERGE_LDS_SECTIONS + 1, "merge_disjoint": MERGE_LDS_SECTIONS}
    big.reach = lambda o: o["counters"]["sections"] <= 9000 // 7 + 4 or _fail("beyond sec_cap")
    small.reach = lambda o: 400 < o["counters"]["sections"] <= MERGE_LDS_SECTIONS or _fail()
    return Group("many sections", 7, [big, small], golden=False)


def group_step4():
    """FixStep4: gaps of 8 (bridged) and 9 (not); three sections chained by short gaps; a gap next to the first and the last"""
    u = U("gaps", 400, 1, counters={"bridged": 4})
    u.track(10, 40, 200).track(49, 80, 260)            # frames 41 .. 48: 8
    u.track(90, 120, 200)                              # 81 .. 89: 9, left open
    u.track(150, 170, 300).track(174, 190, 380).track(192, 220, 290)      # a chain: 3 and 1 (values more than 18 % apart)
    u.track(300, 330, 300).track(339, 398, 200)        # the last section, reaching the end
    u.reach = lambda o: (np.all(o["step4"][41:49] > 0) and np.all(o["step4"][81:90] == 0) and np.all(o["step4"][150:221] > 0)
                         and runs(o["step3"])[0] == (10, 40)) or _fail(runs(o["step4"]))
    # Extend goes on over up to three misses and writes a frame wherever it hits: two hits and a miss, a hundred frames either
    # way, make step 3's contour 65 runs of two frames a frame apart -- more than the nf / 7 + 4 sections steps 2 and 4 can
    # leave -- and FixStep4 bridges every one of those gaps
    v = U("more runs in step 3 than sections anywhere else", 230, 1, counters={"bridged": 60})
    v.track(105, 125, 200, slot=0, sc=0.75)
    for side, origin in ((1, 125), (-1, 105)):
        for k in range(1, 101):
            if k % 3:
                v.put(origin + side * k, 1, 200.0, 0.25)
    v.reach = lambda o: (len(runs(o["step3"])) > 230 // 7 + 4 and runs(o["step4"]) == [(7, 223)]) or _fail(len(runs(o["step3"])), runs(o["step4"]))
    return Group("step4", 7, [u, v])


def group_smooth():
    """SmoothF0Contour: sections of exactly 7, 64, 65 and 1000 frames; sections that touch frame 1 and nf - 2"""
    u = U("7 64 65 1000", 1500, 1)
    u.exact(20, 26, 400).exact(60, 123, 240).exact(160, 224, 160).exact(300, 1299, 320)
    u.reach = lambda o: runs(o["step4"]) == [(20, 26), (60, 123), (160, 224), (300, 1299)] or _fail(runs(o["step4"]))
    # a varying contour, so that the filter has something to do
    w = U("glide", 900, 1)
    for f in range(0, 900):
        w.put(f, f % 7, np.round(8 * (200.0 + 40 * np.sin(f / 57.0) * f / 900.0)) / 8)
    w.reach = lambda o: runs(o["step4"], force_ends=False)[0][0] <= 1 and runs(o["step4"], force_ends=False)[-1][1] >= 898 or _fail(runs(o["step4"], False))
    return Group("smooth", 7, [u, w])


def group_smooth_hbm():
    """one section longer than the smoother's LDS holds"""
    n = SMOOTH_LDS_FRAMES + 80
    u = U("long section", n + 60, 1)
    for f in range(20, 20 + n):
        u.put(f, 0, 180.0 + np.round(8 * 30 * np.sin(f / 211.0)) / 8)
    u.reach = lambda o: max(b - a + 1 for a, b in runs(o["step4"])) > SMOOTH_LDS_FRAMES or _fail()
    return Group("smooth hbm", 7, [u], golden=False)


def random_map(seed, nf=500, nc=14):
    """10 .. 20 random-walk tracks with octave jumps, dropouts, random slots and shared scores"""
    rng = np.random.default_rng(seed)
    u = U(f"seed {seed}", nf, nc)
    for _ in range(int(rng.integers(10, 21))):
        a = int(rng.integers(0, nf - 20))
        b = min(nf - 1, a + int(rng.integers(8, 260)))
        f = float(rng.integers(100 * 8, 380 * 8))
        slot = int(rng.integers(0, u.nslot))
        sc = float(rng.integers(1, 9)) / 8
        for i in range(a, b + 1):
            f += float(rng.integers(-6, 7))
            r = rng.random()
            if r < 0.04:
                continue                                                      # a dropout
            if r < 0.06:
                f = f * 2 if f < 300 * 8 else f / 2                            # an octave jump
            if r > 0.9:
                slot = int(rng.integers(0, u.nslot))
            if r > 0.97:
                sc = float(rng.integers(1, 9)) / 8
            v = min(max(np.round(f), 72 * 8), 790 * 8) / 8
            if u.cand[i, slot] == 0:
                u.put(i, slot, v, sc)
    return u


RANDOM_MAPS, RANDOM_CALLS = 240, 4


def group_random(call):
    per = RANDOM_MAPS // RANDOM_CALLS
    return Group(f"random {call}", 98, [random_map(1000 + call * per + i) for i in range(per)], golden=False)


def group_ragged(frame_period=5.0):
    """nc = 0, 2 and 14 side by side, 3 to several thousand frames"""
    us = [U("3 frames", 3, 2).track(0, 2, 200, slot=3), U("no candidates", 911, 0), random_map(77, nf=2600, nc=14), _many_sections(700),
          random_map(78, nf=333, nc=2), U("1 frame", 1, 14).put(0, 97, 300.0)]
    for u in us:
        u.name = f"ragged {u.name}"
    return Group(f"ragged {frame_period}", 98, us, frame_period=frame_period, golden=False)


GROUPS = {
    "prune": group_prune, "prune wide": group_prune_wide, "step12": group_step12, "tile edge": group_tile_edge,
    "extend 14": lambda: group_extend(2), "extend 70": lambda: group_extend(10), "extend 98": lambda: group_extend(14),
    "extend 161": lambda: group_extend(23), "extend 252": lambda: group_extend(36), "extend edges": group_extend_edges,
    "extend sub": group_extend_sub, "merge": group_merge, "many sections": group_many_sections, "step4": group_step4,
    "smooth": group_smooth, "smooth hbm": group_smooth_hbm,
    "ragged 1.0": lambda: group_ragged(1.0), "ragged 2.5": lambda: group_ragged(2.5), "ragged 5.0": lambda: group_ragged(5.0),
    **{f"random {c}": (lambda c: lambda: group_random(c))(c) for c in range(RANDOM_CALLS)},
}


def group(name):
    return cached(("harvest contour group", name), GROUPS[name])


def case_group(be, name):
    return hold(be, group(name))


# ---- the declared near-tie band -------------------------------------------------------------------------------------------
# Distances from the previous pick are differences of doubles within 18 % of it, so they are multiples of 4 units of their
# own last place (8 above the pick's binade): 1, 255 and 257 units apart do not exist.  The cases are the nearest that do --
# 4, 100, 252 (inside the band), 256 and 260 (outside) -- and one pair 8 units apart that straddles a multiple of 256.
NEAR_TIES = ((4, "4"), (100, "100"), (252, "252"), (256, "256"), (260, "260"), (-8, "straddle"))


def near_tie_utts():
    """cur = 256 Hz; frame 61 holds 296 (40 Hz above) in an EARLIER slot and 216 - k 2^-45 (40 Hz + k units of the distance's last
    place below) in a later one, both again in frame 62 so that neither is pruned.  k = -8: 296 - 2^-44 * ... the nearer one
    straddles: the distances 40 - 8 units and 40 are 8 units apart and differ above the low byte."""
    unit = 2.0 ** -47                                                  # the last place of a distance in [32, 64)
    us = []
    for k, name in NEAR_TIES:
        for nc in (2, 14):
            hi, lo = (296.0, 216.0 - k * unit) if k > 0 else (296.0 + k * unit, 216.0)
            d_hi, d_lo = abs(256.0 - hi), abs(256.0 - lo)
            assert d_hi < d_lo and (d_lo - d_hi) == abs(k) * unit
            u = U(f"near tie {name} nslot {7 * nc}", 120, nc)
            u.track(20, 60, 256.0, slot=1).put(61, 3, hi, 0.25).put(62, 3, hi, 0.25).put(61, 7 * nc - 2, lo, 0.25).put(62, 7 * nc - 2, lo, 0.25)
            u.near = (hi, lo, d_hi, d_lo)
            us.append(u)
    return us


def kernel_rule(cur, row):
    """Extend's nearest candidate as the kernel states it: the distances with their low 8 mantissa bits cleared, the later
    slot among equals"""
    d = np.abs(cur - row)
    key = d.view(np.int64) & ~np.int64(0xFF)
    key[row == 0] = np.iinfo(np.int64).max
    best = int(np.flatnonzero(key == key.min()).max())
    return row[best]


GROUPS["near ties"] = lambda: Group("near ties", 98, near_tie_utts(), lattice=False)
SPECIAL = ("near ties",)            # held by a case of their own, not by case_group


def case_near_ties(be):
    g = group("near ties")
    want = expected(g)
    outs = be.run(g)
    differing = 0
    for u, o, w in zip(g.utts, outs, want):
        hi, lo, d_hi, d_lo = u.near
        assert w["step3"][61] == hi and w["step3"][62] == hi, "the reference takes the nearer"
        rule = kernel_rule(256.0, w["pruned_cand"][61])
        pick = hi if be.exact_ties else rule
        assert o["step3"][61] == pick and o["step3"][62] == pick, (u.name, o["step3"][61], pick)
        if pick != hi:
            differing += 1
            assert abs(d_lo - d_hi) / d_hi < 2.0 ** -44, u.name
            w = dict(w, **{k: np.array(w[k]) for k in ("step3", "step4", "smooth")})
            for k in ("step3", "step4"):
                w[k][61:63] = lo
            w["smooth"] = oracles()[0].smooth_f0(w["step4"])
        hold(be, Group("near ties one", 98, [u], lattice=False), outs=[o], want=[w])
    if be.exact_ties:
        assert differing == 0
    else:
        assert differing == 2 * 3, differing       # 4, 100, 252 on both routes: the band, and nothing else


# ---- batch and shape ------------------------------------------------------------------------------------------------------
def case_ragged_is_its_lone_calls(be):
    g = group("ragged 5.0")
    outs = be.run(g)
    for u, o in zip(g.utts, outs):
        lone = be.run(Group(f"lone {u.name}", g.maxc, [u], lattice=False))[0]
        for k in OUT_ROWS + ("pruned_cand", "pruned_score", "tpos", "f0"):
            assert same_bits(lone[k], o[k]), (u.name, k)
        assert lone["sec_n"][0] == o["sec_n"][0]


def case_lone_job_shapes(be, set_hint):
    """a lone job with and without the shared-device hint (256 or 1024 threads for the one-workgroup kernels): the same bits"""
    for name in ("many sections", "merge", "smooth"):
        g = group(name)
        for u in g.utts[:2]:
            one = Group(f"lone {u.name}", g.maxc, [u], lattice=False)
            set_hint(0)
            a = be.run(one)[0]
            set_hint(1)
            try:
                b = be.run(one)[0]
            finally:
                set_hint(0)
            for k in OUT_ROWS + ("pruned_cand", "pruned_score", "tpos", "f0"):
                assert same_bits(a[k], b[k]), (u.name, k)
            hold(be, one, outs=[a], want=[expected(g)[g.utts.index(u)]])


# ---- refusals -------------------------------------------------------------------------------------------------------------
def case_refusals(be):
    g = group("extend sub")
    rc, d, _ = be.call(g)
    assert rc == 0
    n = len(g.utts)

    def refused(word, **change):
        rc, d, _ = be.call(g, **change)
        assert rc == 1, change
        assert word in be.error() and "probe_harvest_contour" in be.error(), (change, be.error())
        for k in OUT_ROWS + ("pruned_cand", "pruned_score", "tpos", "f0"):
            assert np.all(be.host(d[k]) == SENTINEL), (change, k)
        assert np.all(be.host(d["sec"]) == -7) and np.all(be.host(d["sec_n"]) == -7)

    for k in ("cand", "score", "pruned_cand", "pruned_score", "step2", "step3", "step4", "sec_n", "sec", "basic_f0", "tpos", "f0"):
        refused(k, **{k: None})
    refused("nfb", nfb=None)
    refused("nc", nc=None)
    refused("nc", nc=(C.c_int * n)(*([1] * (n - 1) + [2])))             # 14 slots in a frame of 7
    refused("nc", nc=(C.c_int * n)(*([1] * (n - 1) + [-1])))
    for bad in (259, 266, 0, 8, -7):
        refused("maxc", maxc=bad)
    refused("nfb", nfb=(C.c_int * n)(*([60] * (n - 1) + [0])))
    refused("n_utt", n_utt=0)
    refused("frame_period", frame_period=0.0)
    refused("fb_stride", fb_stride=8)
    refused("sec_cap", sec_cap=3)
    refused("f_stride", f_stride=2)
