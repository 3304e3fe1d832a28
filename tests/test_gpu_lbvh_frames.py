"""RESTIR_BVH=lbvh (include/restir_c.h: the Karras LBVH, kept for comparison) in frames.  build_bvh_lbvh is a pipeline
of its own (k_karras, k_refit_level, k_emit, k_leaf_tris: leaves of at most 4 triangles, its own preorder numbering)
that no other test selects.  With the variable set, and once more with RESTIR_WIDE=off in addition (then every walk
follows the LBVH's skip pointers):

  * the C2-like and C3-like sequences of tests/test_gpu_skip_walks.py equal the default builder's frames, reservoirs,
    G-buffer and ray counts, and the oracle's frames, bit for bit (closest hits and shadow rays do not depend on the
    tree);
  * the update / refit / rebuild plan keeps a structurally valid tree at every step, frames equal a fresh scene's,
    and a rebuild under the variable builds an LBVH again.

Every run asserts that the tree it rendered with is an LBVH: leaves of at most 4 triangles (the default builder's SAH
collapse goes to 8) and node words that differ from the default builder's.
"""
import numpy as np
import pytest

import bvh_brute as B
from restir_amd import params as P
from restir_amd import scenes

import gpu_harness as GH
import skip_walk_cases as S
from skip_walk_cases import oracle_frames, scns  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu

WIDE = {"wide": None, "skip": "off"}


@pytest.mark.parametrize("walk", GH.WALKS)
@pytest.mark.parametrize("wide", list(WIDE))
@pytest.mark.parametrize("which", ["c2", "c3"])
def test_lbvh_frames_equal_default_builder_and_oracle(scns, oracle_frames, which, wide, walk, monkeypatch):  # noqa: F811
    sc, (W, H) = scns[which], S.SIZE[which]
    prms = S.base_prms()
    lb = S.sequence(monkeypatch, sc, W, H, walk, WIDE[wide], prms, bvh="lbvh")
    ref = S.sequence(monkeypatch, sc, W, H, walk, None, prms)
    S.same_runs(lb, ref, f"lbvh {which} {wide} {walk}")
    for f, (a, b) in enumerate(zip(lb.frames, oracle_frames[which])):
        assert np.array_equal(a, b), f"lbvh {which} {wide} {walk} frame {f}: {int((a != b).any(-1).sum())} px differ from the oracle"


@pytest.mark.parametrize("wide", list(WIDE))
@pytest.mark.parametrize("which", ["c2", "c3"])
def test_lbvh_update_refit_rebuild(scns, which, wide, monkeypatch):  # noqa: F811
    sc, (W, H) = scns[which], S.SIZE[which]
    prm = P.c3_params(m_area=8)
    g, gs = S.load(monkeypatch, W, H, sc, "lane", WIDE[wide], bvh="lbvh")      # (asserts an LBVH was built)
    f_ = GH.pinned_renderer(W, H, "lane")
    n0, p0 = gs.bvh_tree()
    status = gs.walk_info()["status"]
    plan = [(0, 0.05, False), (40, 0.05, True), (90, 0.4, False), (130, 0.4, True)]
    for f, (t, amp, with_normals) in enumerate(plan):
        pos = scenes.moving_light_positions(sc, t, 240, amplitude=amp)
        gs.update_positions(pos, sc.normals if with_normals else None)
        if f == 3:
            gs.rebuild()
        nodes, prims = gs.bvh_tree()
        assert B.check_bvh_tree(nodes, prims, pos, 4)["max_leaf"] <= 4, f"step {f}: not an LBVH"
        assert gs.walk_info()["status"] == status
        fresh = f_.load_scene(scenes.Scene(pos, sc.normals, sc.tri_material, sc.materials, sc.camera))
        fn, fp = fresh.bvh_tree()
        if f < 3:           # a refit keeps the topology: skips, leaf words and the triangle order
            assert np.array_equal(nodes.view(np.int32)[:, [3, 7]], n0.view(np.int32)[:, [3, 7]]) and np.array_equal(prims, p0)
        else:               # a rebuild under the variable is a fresh LBVH build
            assert np.array_equal(nodes.view(np.uint32), fn.view(np.uint32)) and np.array_equal(prims, fp)
        cam = scenes.orbit_camera(sc.camera, f, 240, 0.3)
        a = g.produce_restir(gs, cam, prm, f).copy()
        GH.assert_walked(g, "lane")
        b = f_.produce_restir(fresh, cam, prm, f).copy()
        assert np.array_equal(a, b), f"frame {f}: refit != fresh ({int((a != b).any(-1).sum())} px)"
        fresh.close()
    gs.close()
    g.close()
    f_.close()
