"""The sequences of tests/test_gpu_skip_walks.py (frames without the 8-wide tree) and tests/test_gpu_lbvh_frames.py (the
same under RESTIR_BVH=lbvh): the two scenes, a loader that asserts the tree state it loaded, one frame per parameter
block with the walk and split state asserted after every frame, and the run-against-run comparison.  TEST
INFRASTRUCTURE ONLY; the module-scoped fixtures are imported by both test modules.
"""
import numpy as np
import pytest

import bvh_brute as B
import gpu_harness as GH
import oracle_lib as O
from restir_amd import params as P
from restir_amd import scenes

SIZE = {"c2": (64, 48), "c3": (64, 40)}          # 40 rows: a partial 16-row tile


@pytest.fixture(scope="module")
def scns():
    return {"c2": scenes.cornell_many_lights(256), "c3": scenes.sponza_like(target_tris=30_000, n_lamps=128)}


def base_prms(m_area=8):
    return [P.c3_params(m_area=m_area)] * 3 + [P.c3_params(m_area=m_area, do_visibility_pass=1)]


@pytest.fixture(scope="module")
def oracle_frames(scns):
    """the oracle's frames of the base sequence, once per scene"""
    return {which: GH.oracle_frames(sc, O.OracleScene(sc), *SIZE[which], base_prms()).frames for which, sc in scns.items()}


def load(monkeypatch, W, H, sc, walk, wide, split="off", sort=None, status="live", bvh=None):
    """a renderer and the scene loaded with (wide = None) or without (wide = "off") the 8-wide tree, by the default
    builder or (bvh = "lbvh") the Karras LBVH; the state is asserted"""
    GH.set_env(monkeypatch, RESTIR_WIDE=wide, RESTIR_BVH=bvh, RESTIR_SORT=sort, RESTIR_SORT_SPATIAL=sort,
               RESTIR_SORT_TEMPORAL=sort)
    g = GH.pinned_renderer(W, H, walk, split)
    gs = g.load_scene(sc)
    info = gs.walk_info()
    if wide == "off":
        assert info["status"] == "off" and info["wide_nodes"] == 0 and gs.wide_tree() is None, info
    else:
        assert info["status"] == status and (info["wide_nodes"] > 0) == (status == "live"), info
    if bvh == "lbvh":       # a valid tree with the LBVH's leaf maximum whose words are not the default builder's
        nodes, prims = gs.bvh_tree()
        B.check_bvh_tree(nodes, prims, sc.positions, 4)
        monkeypatch.delenv("RESTIR_BVH")
        ref = g.load_scene(sc)
        monkeypatch.setenv("RESTIR_BVH", "lbvh")
        rn, _ = ref.bvh_tree()
        ref.close()
        assert rn.shape != nodes.shape or not np.array_equal(rn.view(np.uint32), nodes.view(np.uint32)), \
            "RESTIR_BVH=lbvh built the default builder's tree"
    return g, gs


def sequence(monkeypatch, sc, W, H, walk, wide, prms, split="off", sort=None, bvh=None):
    """one frame per entry of prms (frame index = position, orbiting camera): frames, ray counts, final reservoirs
    and G-buffer"""
    g, gs = load(monkeypatch, W, H, sc, walk, wide, split, sort, bvh=bvh)
    out = GH.render_frames(g, gs, sc, prms, walk, split, every_frame=True, gbuffer=True)
    gs.close()
    g.close()
    return out


def same_runs(a, b, what):
    for f, (x, y) in enumerate(zip(a.frames, b.frames)):
        GH.assert_equal_finite(x, y, f"{what} frame {f}")
    assert a.rays == b.rays, f"{what}: rays {a.rays} vs {b.rays}"
    assert GH.same(a.res, b.res), f"{what}: reservoirs differ"
    assert GH.same(a.gb, b.gb), f"{what}: G-buffer differs"
