"""Harvest's contour stage alone on the MI355X (include/world_hip.h: world_hip_probe_harvest_contour): the cases of
tests/harvest_contour_cases.py through the shipped library -- hv_prune's base pick by readlane, hc_extend's packed (distance,
slot) key on both of its routes, its two walking wavefronts and ring of row buffers, hc_merge in LDS and out of HBM, hc_smooth in
LDS and out of HBM: the spellings the one-lane emulation of tests/test_harvest_contour_cpu.py replaces -- then the Python layer."""
import numpy as np
import pytest

import harvest_contour_cases as cases
from backends import OnGpu, gpu_backend, wh  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cases.Backend):
    exact_ties = False       # Extend's packed key: distances equal after clearing their low 8 mantissa bits are equally near


be = gpu_backend(GpuBackend)
GENERIC = [name for name in cases.GROUPS if name not in cases.SPECIAL]


@pytest.mark.parametrize("name", GENERIC)
def test_group(be, name):
    cases.case_group(be, name)


def test_the_near_tie_band(be):
    cases.case_near_ties(be)


def test_a_ragged_batch_is_its_lone_calls(be):
    cases.case_ragged_is_its_lone_calls(be)


def test_lone_job_with_and_without_the_shared_device_hint(be):
    cases.case_lone_job_shapes(be, lambda hint: be.lib.world_hip_set_hint(be.ctx, hint))


def test_refusals_write_nothing_and_name_the_argument(be):
    cases.case_refusals(be)


def test_the_routes_by_their_launch_shapes(wh, be):
    """wh.profile's kernel names: the back half is hv_prune and the five contour launches, nothing else; the one-utterance
    shapes of hc_step12_sections and hc_merge (1024 threads) and the batch's (256) give the same bits (the case above), and
    the maps built for the wide tracking route, the HBM merge and the HBM smoother have more slots, sections and frames than
    the narrow routes hold (asserted on the host: the kernels choose by those numbers alone)"""
    g = cases.group("extend 70")
    prof = wh.profile(lambda: be.run(g))
    assert sorted(prof) == sorted(("hv_prune", "hc_step12_sections", "hc_extend", "hc_merge", "hc_smooth", "hc_output")), sorted(prof)
    assert all(len(ms) == 1 for ms in prof.values()), prof
    assert all(u.nslot > 64 for u in g.utts) and all(u.nslot <= 64 for u in cases.group("extend 14").utts)
    many = cases.expected(cases.group("many sections"))
    assert many[0]["counters"]["sections"] > cases.MERGE_LDS_SECTIONS >= many[1]["counters"]["sections"]
    long = cases.expected(cases.group("smooth hbm"))[0]
    assert max(b - a + 1 for a, b in cases.runs(long["step4"])) > cases.SMOOTH_LDS_FRAMES


def test_probe_harvest_contour_of_the_python_layer(wh, be):
    import torch
    g = cases.group("merge")
    want = cases.expected(g)
    nfb, frames, stride, sec_cap, f_stride = be.shapes(g)
    cand, score = np.zeros((len(g.utts), stride, g.maxc)), np.zeros((len(g.utts), stride, g.maxc))
    for i, u in enumerate(g.utts):
        cand[i, :u.nf, :u.nslot], score[i, :u.nf, :u.nslot] = u.cand, u.score
    out = wh.probe_harvest_contour(torch.from_numpy(cand).cuda(), torch.from_numpy(score).cuda(), nfb, [u.nc for u in g.utts], g.frame_period)
    assert out["n_frames"] == frames and out["sec"].shape == (len(g.utts), 6, sec_cap)
    for i, (u, w) in enumerate(zip(g.utts, want)):
        for k in ("step2", "step3", "step4"):
            assert cases.same_bits(out[k][i, :u.nf].cpu().numpy(), w[k]), (u.name, k)
        assert torch.isnan(out["step2"][i, u.nf:]).all()
        assert cases.same_bits(out["tpos"][i, :frames[i]].cpu().numpy(), w["tpos"])
    with pytest.raises(RuntimeError, match="nc"):
        wh.probe_harvest_contour(torch.from_numpy(cand).cuda(), torch.from_numpy(score).cuda(), nfb, [3] * len(g.utts), g.frame_period)
