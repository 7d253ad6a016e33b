"""Harvest's candidate stage alone on the host emulation (include/world_hip.h: world_hip_probe_harvest_candidates): the cases of
tests/harvest_candidates_cases.py -- its docstring says what a list is made of and what is asserted -- through tests/emu, and
the comparators held to each other: the reference's own functions (oracle/_ref, where built), the oracle's restatement and the
reference's recorded results (tests/golden/harvest_candidates.npz) agree bit for bit on every case before anything is held to
them.  tests/test_harvest_candidates_gpu.py runs the same cases on the card: the emulation walks one lane and searches the
lists serially (bracket and bisect), so the 32-lane group search, the ballots two searches share in a wavefront, the scan of
hv_compact_events and its eight loads in flight have their shipped spelling only there."""
import numpy as np
import pytest

import harvest_candidates_cases as cases
from backends import cpu_backend, lib  # noqa: F401 (lib: a fixture)

be = cpu_backend(cases.Backend)


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_reference_oracle_and_golden_agree_and_the_case_reaches_its_branch(name):
    """(no backend: expected() asserts R == O == G bit for bit on raw, cand and nc of every utterance, then the case's reach)"""
    g = cases.group(name)
    assert len(cases.expected(g)) == len(g.utts)


def test_the_reference_finds_the_made_up_edges_in_a_signal():
    """ZeroCrossingEngine itself on a piecewise-linear signal whose falling crossings are the made-up edges (dyadic values, so
    its fine edges are exact) returns the intervals the two restated lines of oracle/harvest_candidates_ref.cpp give"""
    _, ref = cases.oracles()
    if ref is None:
        pytest.skip("the reference is not built here")
    edges = np.array([10.25, 50.5, 90.75, 131.5, 180.25, 200.5, 260.125])
    n = 300
    s = np.ones(n)
    for e in edges:      # the engine's fine edge of a fall from s[i] > 0 to s[i + 1] <= 0 is (i + 1) + s[i] / (s[i] - s[i + 1])
        i, f = int(e) - 1, e - int(e)
        s[i], s[i + 1] = f, f - 1.0                            # (a difference of exactly 1: the quotient is f)
        s[i + 2:i + 6] = -1.0
    loc, val = ref.zero_crossing_engine(s, cases.AFS)
    assert cases.same_bits(loc, cases.locs(edges)) and cases.same_bits(val, cases.AFS / np.diff(edges))


def test_the_guess_misses_take_every_exit_of_the_group_search():
    g = cases.group("guess misses")
    assert g.exits >= set(cases.MISS_EXITS), sorted(set(cases.MISS_EXITS) - g.exits)


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
