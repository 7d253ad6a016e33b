"""Fixtures of Harvest's refinement stage on made-up candidate maps: tests/golden/harvest_refine.npz.

Run on a CPU machine where oracle/_ref/libworld_ref_refine.so exists (oracle/Makefile builds it: oracle/harvest_refine_ref.cpp
includes the unmodified reference's harvest.cpp where it lies and calls OverlapF0Candidates and RefineF0Candidates):

    python tests/golden/make_golden_harvest_refine.py

The inputs are not stored: tests/harvest_refine_cases.py regenerates every signal and map from its definition.  For every
utterance of every group the file holds what THE REFERENCE returned: "<group>/<utterance>/refined" and "/score", [nf, 7 nc].
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import harvest_refine_cases as cases  # noqa: E402
from oracle import loader  # noqa: E402


def main():
    ref = loader.RefRefine()
    out = {}
    for name in cases.GROUPS:
        g = cases.group(name)
        for u in g.utts:
            r = ref.harvest_refine(u.y, u.cand, **u.args)
            out[f"{g.name}/{u.name}/refined"], out[f"{g.name}/{u.name}/score"] = r["refined"], r["score"]
    np.savez_compressed(cases.GOLDEN, **out)
    print(f"{cases.GOLDEN}: {len(out)} arrays, {os.path.getsize(cases.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
