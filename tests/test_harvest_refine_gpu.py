"""Harvest's refinement stage alone on the MI355X (include/world_hip.h: world_hip_probe_harvest_refine): the cases of
tests/harvest_refine_cases.py through the shipped library -- the eight sample phases of a recurrence in neighbouring lanes and
their DPP sums (oct_sum), the harmonic sums across rows (row_pair_sum, half_pair_sum), the readlane set-up of a track, the
wave-uniform loops and the `more` step of hv_refine exist only here (the emulation of tests/test_harvest_refine_cpu.py walks the
phases in one lane) -- then the identities that need no oracle, the launches and the Python layer."""
import numpy as np
import pytest

import harvest_refine_cases as cases
from backends import OnGpu, gpu_backend, same_bits, wh  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cases.Backend):
    pass


be = gpu_backend(GpuBackend)


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group(be, name):
    cases.case_group(be, name, what="harvest refine gpu")


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group_score_accuracy(be, name):
    cases.case_group_score(be, name, what="harvest refine gpu")


def test_a_batch_is_its_lone_calls(be):
    cases.case_batch_is_its_lone_calls(be)


def test_scaling_the_signal_by_powers_of_two(be):
    cases.case_scaling(be)


def test_a_delay_of_one_frame_on_the_table_route(be):
    cases.case_delay(be)


def test_refusals_write_nothing_and_name_the_argument(be):
    cases.case_refusals(be)


def test_route_0_is_the_route_the_profile_names_and_one_launch(wh, be, monkeypatch):
    """wh.profile's kernel names: every route is exactly one launch of its kernel and nothing else; route 0 is hv_refine where
    there is a table and hv_refine_frames by rotation elsewhere -- the same bits as the route named -- and follows
    WORLD_HIP_REFINE_FRAMES and WORLD_HIP_REFINE_ROTATE as a Harvest call does"""
    monkeypatch.delenv("WORLD_HIP_REFINE_FRAMES", raising=False)
    monkeypatch.delenv("WORLD_HIP_REFINE_ROTATE", raising=False)
    g = cases.group("rates")
    by_name = {u.name: u for u in g.utts}

    def one(u, route):
        out = []
        prof = wh.profile(lambda: out.append(be.run([u], route)[0]))
        assert len(prof) == 1 and len(next(iter(prof.values()))) == 1, prof
        return next(iter(prof)), out[0]

    def same(a, b):
        return same_bits(a["refined"], b["refined"]) and same_bits(a["score"], b["score"])
    u = by_name["8000"]
    named = {route: one(u, route) for route in (0, 1, 2, 3)}
    assert [named[r][0] for r in (0, 1, 2, 3)] == ["hv_refine", "hv_refine", "hv_refine_frames", "hv_refine_frames"], named
    assert same(named[0][1], named[1][1])
    v = by_name["11025"]
    k0, o0 = one(v, 0)
    k3, o3 = one(v, 3)
    assert k0 == k3 == "hv_refine_frames" and same(o0, o3)
    monkeypatch.setenv("WORLD_HIP_REFINE_FRAMES", "1")
    k, o = one(u, 0)
    assert k == "hv_refine_frames" and same(o, named[2][1])
    monkeypatch.setenv("WORLD_HIP_REFINE_ROTATE", "1")
    k, o = one(u, 0)
    assert k == "hv_refine_frames" and same(o, named[3][1])


def test_probe_harvest_refine_of_the_python_layer(wh):
    import torch
    g = cases.group("batches")
    n = len(g.utts)
    nfb, nc, y_len = [u.nf for u in g.utts], [u.nc for u in g.utts], [len(u.y) for u in g.utts]
    y = torch.zeros((n, (max(y_len) + 7) & ~7), dtype=torch.float64)
    cand = torch.zeros((n, (max(nfb) + 7) & ~7, 21), dtype=torch.float64)
    for i, u in enumerate(g.utts):
        y[i, :len(u.y)] = torch.from_numpy(np.array(u.y))
        cand[i, :u.nf, :u.nc] = torch.from_numpy(np.array(u.cand))
    u0 = g.utts[0]
    refined, score = wh.probe_harvest_refine(y.cuda(), y_len, cand.cuda(), nfb, nc, route=1, **u0.args)
    be = GpuBackend(wh)
    for i, (u, o) in enumerate(zip(g.utts, be.run(g.utts, 1, g.maxc))):
        assert same_bits(refined[i, :u.nf, :7 * u.nc].cpu().numpy(), o["refined"]) and same_bits(score[i, :u.nf, :7 * u.nc].cpu().numpy(), o["score"])
        assert torch.isnan(refined[i, u.nf:]).all() and torch.isnan(score[i, :, 7 * u.nc:]).all()
    with pytest.raises(RuntimeError, match="route"):
        wh.probe_harvest_refine(y.cuda(), y_len, cand.cuda(), nfb, nc, route=4, **u0.args)
