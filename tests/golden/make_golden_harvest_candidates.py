"""Fixtures of Harvest's candidate stage on made-up zero-crossing lists: tests/golden/harvest_candidates.npz.

Run on a CPU machine where oracle/_ref/libworld_ref_candidates.so exists (oracle/Makefile builds it: oracle/harvest_candidates_ref.cpp
includes the unmodified reference's harvest.cpp where it lies and calls GetF0CandidateContour and DetectOfficialF0Candidates):

    python tests/golden/make_golden_harvest_candidates.py

The inputs are not stored: tests/harvest_candidates_cases.py regenerates every list and map from its definition.  For every
utterance of every group the file holds what THE REFERENCE returned: "<group>/<utterance>/raw" [nch, nf] and "/cand" [nf, maxc]
-- or, for the groups of long or random cases (Group.golden false), "<group>/<utterance>/crc": the CRC-32 of both arrays' bytes
and the number of candidates.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import harvest_candidates_cases as cases  # noqa: E402
from oracle import loader  # noqa: E402


def main():
    ref = loader.RefCandidates()
    out = {}
    for name in cases.GROUPS:
        g = cases.group(name)
        for u in g.utts:
            r = cases.compute(ref, g, u)
            if g.golden:
                out[f"{g.name}/{u.name}/raw"], out[f"{g.name}/{u.name}/cand"] = r["raw"], r["cand"]
            else:
                out[f"{g.name}/{u.name}/crc"] = cases.digest(r)
    np.savez_compressed(cases.GOLDEN, **out)
    print(f"{cases.GOLDEN}: {len(out)} arrays, {os.path.getsize(cases.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
