"""Hostile geometry and rays on every tree the GPU can build: {PLOC (default), RESTIR_BVH=lbvh} x {8-wide tree live,
RESTIR_WIDE=off}.  Scenes and rays are those of tests/bvh_brute.py (flat grids near, far from and close to the origin,
slivers of aspect 1e2 .. 1e6, a mixed-scale soup, coincident duplicates, zero-area triangles, a soup at 1e20, and a
ladder of triangle counts around the builders' block sizes); the reference is brute force in float32, which the
oracle's two trees equal on these very inputs (tests/test_hostile_geometry_oracle.py, CPU).

Per tree and class:
  * the structural checker (bvh_brute.check_bvh_tree) on Scene.bvh_tree(): preorder skips, leaf words that tile the
    triangle slots, leaf maximum 8 (PLOC) / 4 (LBVH), exact box containment;
  * two builds of the same positions, and a rebuild(), give the identical tree (the builders are deterministic);
  * closest hits of the lockstep and the per-lane walk: prim and the bits of t equal brute force on rays through mesh
    vertices, edge midpoints and centroids, straight down onto grid vertices and inside the plane of the grid -- no
    exclusion, no tolerance (closest hits do not depend on the tree);
  * any-hit of both walks equals brute force on interior-aimed and axis-parallel rays, except the rays that
    bvh_brute.ambiguous() / reference_unsound() flag from the geometry and the reference alone (at most 2 %, asserted
    before any GPU result is read).

No any-hit assertion is made on the vertex / edge / axis-at-vertex rays: an any-hit walk's box test has no margin, a
ray lying exactly in a box face gives 0 * inf = NaN in the slab test and the box is culled -- the known, accepted
residue of DESIGN 3.14.

Every case asserts the tree state it ran under (rs_scene_walk_info: "off" and no wide nodes, or consistent with
wide_tree(); the LBVH by its leaf maximum and by differing from the default builder's tree), so a silent fallback to
the path the rest of the suite covers fails here.
"""
import functools

import numpy as np
import pytest

import bvh_brute as B
from gpu_harness import bits, set_env
from restir_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.02        # a condition on the inputs, not a tolerance on the result
# classes whose 8-wide tree must be live when it is not switched off.  The soup at 1e20 and the 300 coincident
# triangles over the grid load as RS_WIDE_TOO_DEEP today (no collapse within the walk's 8 levels): their per-lane walks
# take the skip pointers, with the same answers -- a fallback that costs speed only, so it is reported, not required
WIDE_LIVE = set(B.CLASS_NAMES) - {"huge", "dups"}


def _setenv(monkeypatch, tree):
    bvh, wide = B.TREES[tree]
    set_env(monkeypatch, RESTIR_BVH=bvh, RESTIR_WIDE=wide)
    return bvh, wide


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the class, its rays and their brute-force answers: computed once, shared by the four trees, never written to"""
    cls = B.hostile_class(name)
    o, d = B.closest_rays(cls)
    tb, pb = B.brute_closest(cls.positions, o, d, cls.tnear, 3.0e38)
    ao, ad, atn, atf = B.anyhit_rays(cls)
    skip = B.ambiguous(cls.positions, ao, ad, atn, atf) | B.reference_unsound(cls.positions, ao, ad, atn, atf)
    aref = B.brute_any(cls.positions, ao, ad, atn, atf)
    for a in (o, d, tb, pb, ao, ad, atn, atf, skip, aref):
        a.setflags(write=False)
    return cls, (o, d, tb, pb), (ao, ad, atn, atf, skip, aref)


@functools.lru_cache(maxsize=None)
def _ladder_reference(n):
    cls = B.ladder_class(n)
    o, d = B.closest_rays(cls, n=512)
    tb, pb = B.brute_closest(cls.positions, o, d, cls.tnear, 3.0e38)
    return cls, o, d, tb, pb


def _assert_tree_state(gs, bvh, wide, n_tris, must_be_live):
    """the scene's walk state is the one the case asked for; returns the checked binary tree"""
    info = gs.walk_info()
    wt = gs.wide_tree()
    assert (wt is None) == (info["wide_nodes"] == 0) == (info["status"] != "live"), info
    if wide == "off":
        assert info == {"wide_nodes": 0, "wide_depth": -1, "status": "off"}, info
    else:
        assert info["status"] != "off", info
        if must_be_live:
            assert info["status"] == "live" and info["wide_nodes"] > 0, info
    nodes, prims = gs.bvh_tree()
    assert nodes.shape[0] == gs.n_nodes and prims.shape[0] == n_tris == gs.n_tris
    return nodes, prims, info


def _assert_lbvh_differs(monkeypatch, g, sc, nodes, n_tris):
    """the tree under RESTIR_BVH=lbvh is not the default builder's (from 64 triangles on the two cannot coincide: the
    PLOC collapse of a 64-triangle scene into leaves of at most 4 would be by chance)"""
    if n_tris < 64:
        return
    monkeypatch.delenv("RESTIR_BVH")
    ref = g.load_scene(sc)
    monkeypatch.setenv("RESTIR_BVH", "lbvh")
    rn, _ = ref.bvh_tree()
    ref.close()
    assert rn.shape != nodes.shape or not np.array_equal(bits(rn), bits(nodes)), "RESTIR_BVH=lbvh built the default tree"


@pytest.mark.parametrize("name", B.CLASS_NAMES)
@pytest.mark.parametrize("tree", list(B.TREES))
def test_hostile_class(tree, name, monkeypatch):
    cls, (o, d, tb, pb), (ao, ad, atn, atf, skip, aref) = _reference(name)
    share = float(skip.mean())
    assert share <= AMBIGUOUS_CAP, f"{name}: {100 * share:.2f} % of the any-hit rays are ambiguous: change the inputs"
    assert (pb >= 0).mean() >= cls.hits
    bvh, wide = _setenv(monkeypatch, tree)
    leaf_max = 4 if bvh else 8
    sc = B.scene_from_positions(cls.positions)
    g = Renderer(8, 8)
    gs, gs2 = g.load_scene(sc), g.load_scene(sc)
    nodes, prims, info = _assert_tree_state(gs, bvh, wide, cls.n_tris, name in WIDE_LIVE)
    stats = B.check_bvh_tree(nodes, prims, cls.positions, leaf_max)
    if bvh:
        _assert_lbvh_differs(monkeypatch, g, sc, nodes, cls.n_tris)
    # determinism: a second build, and a rebuild under the same variables, give the same words
    n2, p2 = gs2.bvh_tree()
    assert gs2.n_nodes == gs.n_nodes and np.array_equal(bits(n2), bits(nodes)) and np.array_equal(p2, prims)
    gs2.rebuild()
    n2, p2 = gs2.bvh_tree()
    assert gs2.n_nodes == gs.n_nodes and np.array_equal(bits(n2), bits(nodes)) and np.array_equal(p2, prims)
    assert gs2.walk_info() == info
    gs2.close()
    print(f"[hostile] {name} on {tree}: {stats}, wide {info['status']}, closest hits {100 * (pb >= 0).mean():.1f} %, "
          f"occluded {100 * aref.mean():.1f} %, excluded {100 * share:.2f} %")
    for lockstep in (True, False):
        t, prim = g.debug_trace(gs, o, d, float(cls.tnear), 3.0e38, any_hit=False, lockstep=lockstep)
        bad = np.flatnonzero((prim != pb) | (bits(t) != bits(tb)))
        assert bad.size == 0, (f"{name} on {tree}, lockstep={lockstep}: {bad.size} of {len(o)} closest rays differ from "
                               f"brute force, first {bad[:5]}: prim {prim[bad[:5]]} vs {pb[bad[:5]]}")
        if hasattr(cls, "never_hit"):
            assert not np.isin(prim, cls.never_hit).any()
        _, anyg = g.debug_trace(gs, ao, ad, atn, atf, any_hit=True, lockstep=lockstep)
        bad = np.flatnonzero(((anyg != 0) != aref) & ~skip)
        assert bad.size == 0, (f"{name} on {tree}, lockstep={lockstep}: {bad.size} unambiguous any-hit rays differ from "
                               f"brute force, first {bad[:5]}")
    gs.close()
    g.close()


@pytest.mark.parametrize("tree", list(B.TREES))
def test_size_ladder(tree, monkeypatch):
    """Soups of 1 .. 4097 triangles: around the leaf maximum (8, 9), PLOC's search radius (16, 17, 18, 33) and block
    (255, 256, 257, 512, 513) and beyond.  For n <= 3 without a wide tree the status is whatever rs_scene_walk_info
    reports; only its consistency with bvh_tree() and wide_tree() is asserted."""
    bvh, wide = _setenv(monkeypatch, tree)
    g = Renderer(8, 8)
    for n in B.LADDER:
        cls, o, d, tb, pb = _ladder_reference(n)
        sc = B.scene_from_positions(cls.positions)
        gs = g.load_scene(sc)
        nodes, prims, info = _assert_tree_state(gs, bvh, wide, n, False)
        B.check_bvh_tree(nodes, prims, cls.positions, 4 if bvh else 8)
        if bvh:
            _assert_lbvh_differs(monkeypatch, g, sc, nodes, n)
        for lockstep in (True, False):
            t, prim = g.debug_trace(gs, o, d, float(cls.tnear), 3.0e38, any_hit=False, lockstep=lockstep)
            bad = np.flatnonzero((prim != pb) | (bits(t) != bits(tb)))
            assert bad.size == 0, f"n={n} on {tree}, lockstep={lockstep}: {bad.size} closest rays differ, first {bad[:5]}"
        gs.close()
    g.close()
