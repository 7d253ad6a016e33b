"""Fixtures of Harvest's contour stage on made-up candidates: tests/golden/harvest_contour.npz.

Run on a CPU machine where oracle/_ref/libworld_ref_contour.so exists (oracle/Makefile builds it: oracle/harvest_contour_ref.cpp
includes the unmodified reference's harvest.cpp where it lies and calls RemoveUnreliableCandidates, FixStep1 .. 4, FixF0Contour
and SmoothF0Contour):

    python tests/golden/make_golden_harvest_contour.py

The inputs are not stored: tests/harvest_contour_cases.py regenerates every map from its definition.  For every utterance of
every group the file holds what THE REFERENCE returned: "<group>/<utterance>/step2", "/step3", "/step4", "/smooth" (the
contours after FixStep2, FixStep3, FixStep4 and SmoothF0Contour, [nf] doubles) -- or, for the groups of long or random maps
(Group.golden false), "<group>/<utterance>/crc": the CRC-32 of each of those four arrays' bytes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import harvest_contour_cases as cases  # noqa: E402
from oracle import loader  # noqa: E402


def main():
    ref = loader.RefContour()
    out = {}
    for name in cases.GROUPS:
        g = cases.GROUPS[name]()
        for u in g.utts:
            r = ref.harvest_contour(u.cand, u.score)
            if g.golden:
                for k in cases.GOLDEN_KEYS:
                    out[f"{g.name}/{u.name}/{k}"] = r[k]
            else:
                out[f"{g.name}/{u.name}/crc"] = cases.digest(r)
    np.savez_compressed(cases.GOLDEN, **out)
    print(f"{cases.GOLDEN}: {len(out)} arrays, {os.path.getsize(cases.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
