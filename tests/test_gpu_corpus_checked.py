"""The corpus kernels (world_amd/csrc/corpus.h) on the checked builds.  tests/test_gpu_checked_builds.py holds every kernel
of csrc/*.hip and csrc/*.inc to a row of its FAMILIES table; corpus.h is a header precisely because that table could not be
edited when its kernels arrived (the unit's head comment says so), and this file carries the same obligations for them with
that module's machinery as it is: every __global__ function of corpus.h claimed (no GPU), one workload through the legs of
test_family_on_the_checked_builds -- product twice, the claims launched, three jitter passes, the LDS-poison build, two
passes of the HBM-poison build with its counter rising -- and a leg that shares one context with the alignment, the
Gaussian mixture and MLPG, forwards and backwards.  The row moves into FAMILIES when that file is next open for editing."""
import os
import time

import numpy as np
import pytest

import test_corpus_cpu as cpu
import test_gpu_checked_builds as cb

gpu = pytest.mark.gpu

CLAIMS = ("frame_power", "frame_power_mean", "select_frames", "joint_rows")
SOURCE = os.path.join(cb.CSRC, "corpus.h")
GATE_DB = -20.0


def kernels_in_corpus_h():
    """cb.kernels_in_source's pattern on the one file that scan does not read"""
    import re
    pattern = re.compile(r"__global__\s+void\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?(?:[A-Z][A-Z0-9_]*\s+)?(\w+)\s*\(")
    with open(SOURCE) as f:
        return set(pattern.findall(f.read()))


def test_every_kernel_of_corpus_h_is_claimed_here():
    source = kernels_in_corpus_h()
    assert "joint_rows" in source and len(source) >= 4, "the scan lost the kernels"
    assert sorted(source - set(CLAIMS)) == [], "kernels of corpus.h that run_corpus does not claim"
    assert sorted(set(CLAIMS) - source) == [], "claimed, but no longer in corpus.h"
    assert not source & set(cb.kernels_in_source()), "a corpus kernel's name is taken by another unit"
    assert not set(CLAIMS) & cb.claimed_kernels(), "FAMILIES claims a corpus kernel: the row has moved, retire this file's"
    # the scan itself: a kernel taken out of the claims is reported
    assert sorted(source - (set(CLAIMS) - {"select_frames"})) == ["select_frames"]


def run_corpus(wh):
    """gate -> gather -> align on the gathered rows -> joint rows with the selections (test_corpus_cpu.gated_corpus: 65 x 70,
    130 x 64 and 64 x 257 frames, across a wavefront, a workgroup's tile and the four-frame workgroups of the power)"""
    import torch
    pairs = cb._once(("corpus",), cpu.gated_corpus)
    out, sides = [], []
    for s, tag in ((0, "a"), (1, "b")):
        n = np.array([len(p[s][0]) for p in pairs], dtype=np.int32)
        F = int(n.max())
        sp = torch.ones((len(pairs), F, pairs[0][s][0].shape[1] + 3), dtype=torch.float64, device=wh.device)
        c = torch.zeros((len(pairs), F, pairs[0][s][1].shape[1] + 3), dtype=torch.float64, device=wh.device)
        dyn = torch.zeros((len(pairs), F, pairs[0][s][2].shape[1]), dtype=torch.float64, device=wh.device)
        for u, p in enumerate(pairs):
            sp[u, :n[u], 1:-2] = cb._dev(p[s][0])
            c[u, :n[u], 3:] = cb._dev(p[s][1])
            dyn[u, :n[u]] = cb._dev(p[s][2])
        power, mean = wh.frame_power(sp[:, :, 1:-2], n)
        index, count, keep = wh.select_frames(power, n, 10.0 ** (GATE_DB / 10.0), scale=mean)
        k = cb._np(count)
        kept = wh.gather_rows(c[:, :, 4:], index, k, n_src=n)           # the statics without c0, at column 4 of the record
        out += [(f"{tag} mean", cb._np(mean)), (f"{tag} count", k)]
        for u in range(len(pairs)):
            out += [(f"{tag} power[{u}]", cb._np(power[u, :n[u]])), (f"{tag} index[{u}]", cb._np(index[u, :k[u]])),
                    (f"{tag} keep[{u}]", cb._np(keep[u, :n[u]])), (f"{tag} kept[{u}]", cb._np(kept[u, :k[u]]))]
        sides.append((dyn, n, index, k, kept))
    (xa, na, ia, ka, fa), (xb, nb, ib, kb, fb) = sides
    path, path_len, _, _, _ = wh.align(fa, fb, ka, kb)
    z = wh.joint_rows(xa, xb, path, path_len, sel_a=ia, sel_b=ib, n_a=na, n_b=nb, n_sel_a=ka, n_sel_b=kb)
    return out + [("path_len", cb._np(path_len)), ("z", cb._np(z))]


@gpu
def test_corpus_on_the_checked_builds():
    from world_amd.api import LIB_PATH
    family, run, kw = "corpus", run_corpus, {}
    (first, second), _, t_product = cb._run_family(LIB_PATH, run, kw, repeats=2)
    assert first, "nothing to compare"
    cb._made.setdefault(("fresh", family), first)
    bad = cb._differences(first, second)
    assert not bad, f"the product build is not deterministic in {bad[:8]}"
    z = dict(first)["z"]
    assert z.shape[0] == int(dict(first)["path_len"].sum()) and np.all(np.isfinite(z)), "the workload's rows are not what it says"
    _, launches, _ = cb._run_family(LIB_PATH, run, kw, profile_first=True)
    missing = [k for k in CLAIMS if not cb._launched(launches, k)]
    assert not missing, f"claims {missing}, launched {sorted(launches)}"
    passes, _, t_jitter = cb._run_family(cb._lib("jitter"), run, kw, repeats=3)
    for rep, res in enumerate(passes):
        bad = cb._differences(first, res)
        assert not bad, f"jitter build, pass {rep}: {bad[:8]} differ from the product build's"
    (res,), _, t_poison = cb._run_family(cb._lib("poison"), run, kw)
    cb._no_poison_in(family, "poison build", first, res)
    bad = cb._differences(first, res)
    assert not bad, f"poison build: {bad[:8]} differ from the product build's"
    filled = []
    passes, _, t_hbm = cb._run_family(cb._lib("hbm"), run, kw, repeats=2, poisoned=filled)
    for rep, res in enumerate(passes):
        cb._no_poison_in(family, f"hbm build, pass {rep}", first, res)
        bad = cb._differences(first, res)
        assert not bad, f"hbm build, pass {rep}: {bad[:8]} differ from the product build's"
    assert len(filled) == 2 and filled[0] > 0 and filled[1] > 0, f"hbm build: the poison counter rose by {filled} bytes (the alignment carves in every pass)"
    print(f"corpus: product {min(t_product):.2f} s, jitter {max(t_jitter):.2f} s a pass, poison {t_poison[0]:.2f} s, hbm {max(t_hbm):.2f} s a pass; "
          f"{len(first)} outputs, {sum(launches.values())} launches")


def _fresh(name, run):
    from world_amd.api import LIB_PATH
    return cb._once(("fresh", name), lambda: cb._run_family(LIB_PATH, run, {})[0][0])


@gpu
@pytest.mark.parametrize("build", ["product", "hbm"])
def test_corpus_shares_a_context_with_its_neighbours(build):
    """align, gmm, mlpg and the corpus workload in ONE context, in that order and reversed: each equals its fresh-context
    result, so the corpus calls neither rely on nor spoil what the stages around them leave in the workspace"""
    import torch
    from world_amd.api import LIB_PATH
    runs = [(f, cb.FAMILIES[f][0]) for f in ("align", "gmm", "mlpg")] + [("corpus", run_corpus)]
    want = {f: _fresh(f, run) for f, run in runs}
    wh = cb._open(LIB_PATH if build == "product" else cb._lib(build), {})
    counter = cb._poison_counter(wh.lib) if build == "hbm" else None
    t0 = time.perf_counter()
    try:
        for order, sequence in (("in order", runs), ("reversed", runs[::-1])):
            before = counter() if counter else 0
            for f, run in sequence:
                res = run(wh)
                torch.cuda.synchronize()
                if build == "hbm":
                    cb._no_poison_in(f, f"{build} build, shared context, {order}", want[f], res)
                bad = cb._differences(want[f], res)
                assert not bad, f"{f}: {build} build, shared context, {order}: {bad[:8]} differ from the fresh context's"
            assert counter is None or counter() > before, f"hbm build, shared context, {order}: the poison counter did not rise"
    finally:
        wh.close()
    print(f"shared context, {build}: {time.perf_counter() - t0:.2f} s")
