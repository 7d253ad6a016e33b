"""Harvest's candidate stage alone on the MI355X (include/world_hip.h: world_hip_probe_harvest_candidates): the cases of
tests/harvest_candidates_cases.py through the shipped library -- the 32-lane group search of hv_raw_candidates' eight end points
(intervals_at_or_before_group: the emulation of tests/test_harvest_candidates_cpu.py replaces it by the serial search, so every
exit the "guess misses" and "small lists" groups are built for is held HERE alone), the staged and the unstaged route, the block
scan and flat copy of hv_compact_events, hv_detect's batched fetches and its atomicMax -- then the Python layer."""
import numpy as np
import pytest

import harvest_candidates_cases as cases
from backends import OnGpu, gpu_backend, wh  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cases.Backend):
    pass


be = gpu_backend(GpuBackend)


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group(be, name):
    cases.case_group(be, name)


@pytest.mark.parametrize("ev_group", (1, 2, 5, 7))
def test_groups_of_utterances_are_their_lone_calls(be, ev_group):
    cases.case_groups_are_their_lone_calls(be, ev_group)


@pytest.mark.parametrize("name", cases.COMPACTIONS)
def test_compaction(be, name):
    cases.case_compaction(be, name)


def test_compacted_lists_go_on_through_the_stages(be):
    cases.case_compacted_lists_go_on(be)


def test_refusals_write_nothing_and_name_the_argument(be):
    cases.case_refusals(be)


def test_the_stage_by_its_launches(wh, be):
    """wh.profile's kernel names: one segment list runs hv_raw_candidates once per group of utterances and hv_detect once,
    nothing else; several segment lists add hv_compact_events per group"""
    g = cases.group("groups")
    prof = wh.profile(lambda: be.run_group(g, ev_group=2))
    assert sorted(prof) == ["hv_detect", "hv_raw_candidates"], sorted(prof)
    assert len(prof["hv_raw_candidates"]) == 3 and len(prof["hv_detect"]) == 1, prof
    prof = wh.profile(lambda: cases.case_compacted_lists_go_on(be))
    assert sorted(prof) == ["hv_compact_events", "hv_detect", "hv_raw_candidates"] and len(prof["hv_compact_events"]) == 2, prof


def test_probe_harvest_candidates_of_the_python_layer(wh):
    import torch
    g = cases.group("counts")
    want = cases.expected(g)
    packed = [g.packed(u) for u in g.utts]
    n, nfb = len(g.utts), [u.nf for u in g.utts]
    ev = torch.from_numpy(np.stack([e for e, _ in packed]).reshape(n, g.nch * 4, 1, g.ev_cap)).cuda()
    cnt = torch.from_numpy(np.stack([c for _, c in packed]).reshape(n, g.nch * 4, 1)).cuda()
    out = wh.probe_harvest_candidates(nfb, g.band_f0, ev, cnt, afs=g.afs, f0_floor=g.f0_floor, f0_ceil=g.f0_ceil, stages=6)
    zcap = cases.zcap_of(g.nch)
    for i, (u, w) in enumerate(zip(g.utts, want)):
        assert cases.same_bits(out["raw"][i, :, :u.nf].cpu().numpy(), w["raw"])
        assert cases.same_bits(out["cand"][i, :u.nf, :zcap].cpu().numpy(), w["cand"][:, :zcap]) and int(out["nc"][i]) == w["nc"]
        assert torch.isnan(out["raw"][i, :, u.nf:]).all() and torch.isnan(out["cand"][i, :, zcap:]).all()
    d = g = cases.group("detect 38")
    raw = torch.zeros((1, d.nch, (d.utts[0].nf + 7) & ~7), dtype=torch.float64)
    raw[0, :, :d.utts[0].nf] = torch.from_numpy(np.array(d.utts[0].raw))
    out = wh.probe_harvest_candidates([d.utts[0].nf], d.band_f0, raw=raw.cuda(), stages=4, f0_floor=60.0, f0_ceil=2000.0)
    assert int(out["nc"][0]) == cases.expected(d)[0]["nc"]
    with pytest.raises(RuntimeError, match="stages"):
        wh.probe_harvest_candidates([d.utts[0].nf], d.band_f0, raw=raw.cuda(), stages=8)
