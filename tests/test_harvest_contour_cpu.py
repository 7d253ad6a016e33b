"""Harvest's contour stage alone on the host emulation (include/world_hip.h: world_hip_probe_harvest_contour): the cases of
tests/harvest_contour_cases.py -- its docstring says what a map is made of and what is asserted -- through tests/emu, and the
comparators held to each other: the reference's own functions (oracle/_ref, where built), the oracle's restatement and the
reference's recorded contours (tests/golden/harvest_contour.npz) agree bit for bit on every map before anything is held to
them.  tests/test_harvest_contour_gpu.py runs the same cases on the card: the emulation walks one lane, so the base pick's
readlane, Extend's packed (distance, slot) key and the two walking wavefronts have their shipped spelling only there."""
import numpy as np
import pytest

import harvest_contour_cases as cases
from backends import cpu_backend, lib  # noqa: F401 (lib: a fixture)

be = cpu_backend(cases.Backend)
GENERIC = [name for name in cases.GROUPS if name not in cases.SPECIAL]


def set_hint_of(be):
    return lambda hint: be.lib.world_hip_set_hint(be.ctx, hint)


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_reference_oracle_and_golden_agree_and_the_map_reaches_its_branch(name):
    """(no backend: expected() asserts R == O == G bit for bit on every contour of every utterance, then the case's reach)"""
    want = cases.expected(cases.group(name))
    assert len(want) == len(cases.group(name).utts)


def test_the_wide_oracle_follows_the_same_discrete_path():
    """the long-double yardstick of the smoother is fed the same step-4 contour: its own agrees with the oracle's bit for bit
    (steps 1 .. 4 are not wo_real arithmetic), and its smoothed contour within a few ulp"""
    port, wide, _ = cases.oracles()
    g = cases.group("smooth")
    for u, o in zip(g.utts, cases.expected(g)):
        w = wide.harvest_contour(u.cand, u.score, g.frame_period)
        assert cases.same_bits(w["step4"], o["step4"])
        v = o["smooth"] > 0
        assert v.any() and np.max(np.abs(w["smooth"][v] - o["smooth"][v]) / o["smooth"][v]) < 1e-12
        assert cases.same_bits(port.smooth_f0(o["step4"]), o["smooth"])


def test_every_listed_branch_is_reached_by_a_case_built_for_it():
    """the counters the groups below add up to: no branch of steps 3 and 4 is left to the random sweep"""
    total = {}
    for name in GENERIC:
        if name.startswith(("random", "ragged")):
            continue
        for o in cases.expected(cases.group(name)):
            for k, v in o["counters"].items():
                total[k] = total.get(k, 0) + v
    assert all(total[k] > 0 for k in total), total


@pytest.mark.parametrize("name", GENERIC)
def test_group(be, name):
    cases.case_group(be, name)


def test_the_near_tie_band(be):
    cases.case_near_ties(be)


def test_a_ragged_batch_is_its_lone_calls(be):
    cases.case_ragged_is_its_lone_calls(be)


def test_lone_job_with_and_without_the_shared_device_hint(be):
    cases.case_lone_job_shapes(be, set_hint_of(be))


def test_refusals_write_nothing_and_name_the_argument(be):
    cases.case_refusals(be)
