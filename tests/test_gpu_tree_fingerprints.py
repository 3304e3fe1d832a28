"""Every tree of the GPU builders, bit for bit against a recording (tests/golden/tree_fingerprints.json, written by
scripts/tree_fingerprints.py twice, with equal results, at commit 4b0219c, before the builders' files were touched:
DESIGN.md 3.30).  Per case -- the soups of bvh_brute.LADDER, every hostile class, bvh_brute's non-finite scene
and its chain of the walk's depth, the 64-light Cornell box -- and per tree setting of bvh_brute.TREES the
SHA-256 of Scene.bvh_tree(), of Scene.wide_tree() (or "none") and the rs_scene_walk_info status equal the recording,
and one rebuild() gives the first build's fingerprint again.  The builders are deterministic (kernel boundaries order
every hand-off, ties go to the smaller index, min / max atomics only), so the recording holds on every run."""
import json
import os

import numpy as np
import pytest

import bvh_brute as B
from gpu_harness import bits
from restir_amd.renderer import Renderer
from scripts import tree_fingerprints as TF

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_fingerprints.json")))
CASES = TF.cases()


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(8, 8)
    yield r
    r.close()


def test_recording_covers_the_cases():
    assert TF.TREES == B.TREES
    for name, want in (("nonfinite", B.nonfinite_scene()), ("depth8", B.depth8_scene())):
        assert np.array_equal(bits(CASES[name]().positions), bits(want.positions)), f"{name}: the recorder's scene is not bvh_brute's"
    assert set(GOLDEN) == set(CASES)
    assert all(set(v) == set(TF.TREES) for v in GOLDEN.values())


@pytest.mark.parametrize("case", list(CASES))
def test_tree_fingerprints(case, renderer, monkeypatch):
    for k in ("RESTIR_BVH", "RESTIR_WIDE"):
        monkeypatch.setenv(k, "")            # registered for restoring: case_fingerprints sets them per tree
    got = TF.case_fingerprints(renderer, CASES[case]())
    for tree, fp in got.items():
        assert fp["first"] == GOLDEN[case][tree], f"{case} on {tree}: the tree differs from the recording"
        assert fp["rebuilt"] == fp["first"], f"{case} on {tree}: rebuild() gave another tree"
