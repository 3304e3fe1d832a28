"""CPU: the oracle's two trees (the binary stack walk and the 8-wide walk of oracle/restir_oracle.c) against brute
force on the hostile scene and ray classes of tests/bvh_brute.py -- the very inputs tests/test_gpu_hostile_geometry.py
gives the GPU's four trees.  It establishes that the demand made of the GPU is fair: closest hits equal brute force in
prim and in the bits of t on every class, rays through vertices, along shared edges and inside the plane of a flat
mesh included; any-hit equals brute force on every ray that neither bvh_brute.ambiguous() nor
bvh_brute.reference_unsound() flags (the second: float32 Moller-Trumbore's own t on a sliver of aspect 1e6 is off by
up to a factor of 2, see there; it flags 25 of the 2048 rays on needles_1e6 and none on any other class -- with other
seeds 21 to 29 there and at most 1 on needles_1e4).  Both masks come from the geometry and the reference alone, and
together they must stay within 2 %.

No any-hit assertion is made on the vertex / edge / axis-at-vertex rays: an any-hit walk's box test has no margin,
a ray lying exactly in a box face gives 0 * inf = NaN in the slab test and the box is culled -- the accepted residue
of DESIGN 3.14.
"""
import numpy as np
import pytest

import bvh_brute as B
import oracle_lib as O
from gpu_harness import bits

AMBIGUOUS_CAP = 0.02        # a condition on the inputs, not a tolerance on the result


@pytest.fixture(scope="module", params=B.CLASS_NAMES)
def case(request):
    cls = B.hostile_class(request.param)
    o, d = B.closest_rays(cls)
    ref = B.brute_closest(cls.positions, o, d, cls.tnear, 3.0e38)
    ao, ad, atn, atf = B.anyhit_rays(cls)
    amb = B.ambiguous(cls.positions, ao, ad, atn, atf) | B.reference_unsound(cls.positions, ao, ad, atn, atf)
    aref = B.brute_any(cls.positions, ao, ad, atn, atf)
    return cls, (o, d, ref), (ao, ad, atn, atf, amb, aref)


@pytest.mark.parametrize("wide", [False, True], ids=["binary", "wide"])
def test_oracle_equals_brute_force(case, wide):
    cls, (o, d, (tb, pb)), (ao, ad, atn, atf, amb, aref) = case
    assert len(o) <= 2048 and len(ao) <= 2048 and cls.n_tris <= 4096
    share = float(amb.mean())
    assert share <= AMBIGUOUS_CAP, f"{cls.name}: {100 * share:.2f} % of the any-hit rays are ambiguous: change the inputs"
    assert (pb >= 0).mean() >= cls.hits, f"{cls.name}: only {100 * (pb >= 0).mean():.1f} % of the closest rays hit"
    if hasattr(cls, "never_hit"):
        assert not np.isin(pb, cls.never_hit).any()
    os_ = O.OracleScene(B.scene_from_positions(cls.positions), wide=wide)
    if cls.name != "huge":                      # the oracle may decline an 8-wide tree over 1e20 boxes
        assert os_.wide == wide
    t, prim = os_.trace_closest(o, d, float(cls.tnear), 3.0e38)
    bad = np.flatnonzero((prim != pb) | (bits(t) != bits(tb)))
    assert bad.size == 0, f"{cls.name}: {bad.size} closest rays differ from brute force, first {bad[:5]}"
    anyh = os_.trace_any(ao, ad, atn, atf).astype(bool)
    bad = np.flatnonzero((anyh != aref) & ~amb)
    print(f"[hostile] {cls.name} wide={wide}: hits {100 * (pb >= 0).mean():.1f} %, any-hit occluded "
          f"{100 * aref.mean():.1f} %, ambiguous {100 * share:.2f} %")
    assert bad.size == 0, f"{cls.name}: {bad.size} unambiguous any-hit rays differ from brute force, first {bad[:5]}"


@pytest.mark.parametrize("n", B.LADDER)
def test_oracle_size_ladder(n):
    cls = B.ladder_class(n)
    o, d = B.closest_rays(cls, n=512)
    tb, pb = B.brute_closest(cls.positions, o, d, cls.tnear, 3.0e38)
    for wide in (False, True):
        t, prim = O.OracleScene(B.scene_from_positions(cls.positions), wide=wide).trace_closest(o, d, float(cls.tnear), 3.0e38)
        assert np.array_equal(prim, pb) and np.array_equal(bits(t), bits(tb)), (n, wide)


def test_checker_catches_broken_trees():
    """the structural checker on a hand-made tree, and on the same tree with one skip, one box and one leaf word off"""
    pos = B.soup(6, 7).astype(np.float32)
    tri = pos.reshape(-1, 3, 3)
    lo, hi = tri.min(1), tri.max(1)

    def box(ids):
        return lo[ids].min(0), hi[ids].max(0)

    def node(b, skip, leaf):
        n = np.zeros(8, np.float32)
        n[0:3], n[4:7] = b
        n.view(np.int32)[3], n.view(np.int32)[7] = skip, leaf
        return n
    prims = np.array([3, 0, 5, 1, 2, 4], np.int32)
    # root(0) -> [leaf(1): slots 0..1] [inner(2) -> leaf(3): slots 2..4, leaf(4): slot 5]
    good = np.stack([node(box(prims), 5, -1), node(box(prims[0:2]), 2, (0 << 3) | 1), node(box(prims[2:6]), 5, -1),
                     node(box(prims[2:5]), 4, (2 << 3) | 2), node(box(prims[5:6]), 5, (5 << 3) | 0)])
    assert B.check_bvh_tree(good, prims, pos, 8) == {"nodes": 5, "leaves": 3, "max_leaf": 3}
    with pytest.raises(AssertionError):
        B.check_bvh_tree(good, prims, pos, 2)                      # a leaf above the builder's maximum
    for what in ("skip", "box", "leafword", "prims"):
        bad, p = good.copy(), prims.copy()
        if what == "skip":
            bad.view(np.int32)[2, 3] -= 1
        elif what == "box":
            bad[3, 4] = np.nextafter(bad[3, 4], np.float32(-np.inf))
        elif what == "leafword":
            bad.view(np.int32)[4, 7] = (4 << 3) | 0
        else:
            p[1] = p[0]
        with pytest.raises(AssertionError):
            B.check_bvh_tree(bad, p, pos, 8)
