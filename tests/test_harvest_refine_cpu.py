"""Harvest's refinement stage alone on the host emulation (include/world_hip.h: world_hip_probe_harvest_refine): the cases of
tests/harvest_refine_cases.py -- its docstring says what a case is made of and what is asserted -- through tests/emu, and the
comparators held to each other: the reference's own functions (oracle/_ref, where built) against their recorded results
(tests/golden/harvest_refine.npz) bit for bit, the double oracle against the reference at 1e-10 with identical gates, the
wide oracle's gates and every case's reach.  tests/test_harvest_refine_gpu.py runs the same cases on the card: the emulation
walks the eight sample phases and the 64 window lanes in ONE lane, so the DPP sums, the readlane set-up, the wave-uniform
loops and the lanes' own LDS traffic have their shipped spelling only there."""
import pytest

import harvest_refine_cases as cases
from backends import cpu_backend, lib  # noqa: F401 (lib: a fixture)

be = cpu_backend(cases.Backend)


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_comparators_agree_and_the_case_reaches_its_branch(name):
    """(no backend: expected() asserts R == golden bit for bit, P against R, W's margins and gates, then the case's reach)"""
    g = cases.group(name)
    for u in g.utts:
        cases.expected(g, u)


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group(be, name):
    cases.case_group(be, name, what="harvest refine emu")


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group_score_accuracy(be, name):
    """(held by the emulation's eight sample phases and 64 window lanes: with ONE phase over the whole window, and a rotated
    window built by one rotation per sample, the score -- a cancellation -- missed this bound in four groups by up to 31563 ulp
    against e_R 3497)"""
    cases.case_group_score(be, name, what="harvest refine emu")


def test_a_batch_is_its_lone_calls(be):
    cases.case_batch_is_its_lone_calls(be)


def test_scaling_the_signal_by_powers_of_two(be):
    cases.case_scaling(be)


def test_a_delay_of_one_frame_on_the_table_route(be):
    cases.case_delay(be)


def test_refusals_write_nothing_and_name_the_argument(be):
    cases.case_refusals(be)
