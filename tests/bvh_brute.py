"""Test infrastructure (numpy only): a brute-force reference for the BVH ray queries, the structural checker of the
binary skip-pointer tree (Scene.bvh_tree(), rs_debug_bvh_tree) and the seeded hostile scene / ray generators that
tests/test_hostile_geometry_oracle.py (CPU, the oracle's two trees) and tests/test_gpu_hostile_geometry.py (GPU, both
builders with and without the 8-wide tree) share.

brute_closest / brute_any are Moller-Trumbore over every triangle in float32, in the operation order of rs_scene.h
tri_test (dot products summed as (x + y) + z; the edges formed as v1 - v0, v2 - v0 in float32 as the builders store
them), ties to the smaller t and then the smaller triangle index -- so a walk that visits every box the accepted
triangle lies in returns these very bits, whatever the tree.

ambiguous() is computed in float64 from the geometry alone and flags the rays whose any-hit answer float32 rounding
may decide: the hit point within delta (barycentric) of an edge, or t within delta (relative) of an end of the
segment.  The any-hit tests drop those rays and assert the rest.
"""
import numpy as np

F = np.float32
T_MISS = F(-1.0)


# ---------------------------------------------------------------------------------------------- brute force
def _dot(a, b):
    m = a * b
    return (m[..., 0] + m[..., 1]) + m[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0],
                     x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], -1)


def _per_ray(x, n, dtype):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype), (n,)))


def _mt(positions, o, d, dtype):
    """(det, u, v, t), each (rays, triangles), in `dtype`"""
    P = np.asarray(positions, np.float32).reshape(-1, 9).astype(dtype)
    v0 = P[:, 0:3]
    e1, e2 = P[:, 3:6] - v0, P[:, 6:9] - v0
    o = np.asarray(o, np.float32).astype(dtype)[:, None, :]
    d = np.asarray(d, np.float32).astype(dtype)[:, None, :]
    dd = np.broadcast_to(d, (d.shape[0], e2.shape[0], 3))
    p = _cross(dd, e2[None])
    det = _dot(e1[None], p)
    inv = dtype(1.0) / det
    sv = o - v0[None]
    u = _dot(sv, p) * inv
    q = _cross(sv, e1[None])
    v = _dot(dd, q) * inv
    t = _dot(e2[None], q) * inv
    return det, u, v, t


def _accept(positions, o, d, tn, tf):
    det, u, v, t = _mt(positions, o, d, np.float32)
    one, zero = F(1.0), F(0.0)
    ok = (det != zero) & (u >= zero) & (u <= one) & (v >= zero) & (u + v <= one) & (t >= tn[:, None]) & (t <= tf[:, None])
    return ok, t


def _chunks(n_rays, n_tris):
    step = max(1, (1 << 20) // max(1, n_tris))
    return [(a, min(n_rays, a + step)) for a in range(0, n_rays, step)]


def brute_closest(positions, o, d, tnear, tfar):
    """(t float32, prim int32) per ray; misses are (-1, -1) as Renderer.debug_trace and the oracle report them"""
    n = len(o)
    tn, tf = _per_ray(tnear, n, np.float32), _per_ray(tfar, n, np.float32)
    ts, prims = np.full(n, T_MISS, np.float32), np.full(n, -1, np.int32)
    nt = np.asarray(positions).reshape(-1, 9).shape[0]
    with np.errstate(all="ignore"):
        for a, b in _chunks(n, nt):
            ok, t = _accept(positions, o[a:b], d[a:b], tn[a:b], tf[a:b])
            tm = np.where(ok, t, F(np.inf))
            best = tm.min(axis=1)
            first = (tm == best[:, None]).argmax(axis=1)        # the smallest index among the equal smallest t
            hit = ok.any(axis=1)
            ts[a:b] = np.where(hit, best, T_MISS)
            prims[a:b] = np.where(hit, first, -1)
    return ts, prims


def brute_any(positions, o, d, tnear, tfar):
    """bool per ray: some triangle passes the same acceptance test within [tnear, tfar]"""
    n = len(o)
    tn, tf = _per_ray(tnear, n, np.float32), _per_ray(tfar, n, np.float32)
    out = np.zeros(n, bool)
    nt = np.asarray(positions).reshape(-1, 9).shape[0]
    with np.errstate(all="ignore"):
        for a, b in _chunks(n, nt):
            out[a:b] = _accept(positions, o[a:b], d[a:b], tn[a:b], tf[a:b])[0].any(axis=1)
    return out


def ambiguous(positions, o, d, tnear, tfar, delta=1e-3):
    """bool per ray, float64, from the geometry alone: some triangle is hit within delta of one of its edges (t within
    the segment widened by delta, relative), or hit inside or within delta of its edges with t within delta (relative)
    of tnear or tfar, or has a non-finite determinant."""
    n = len(o)
    tn, tf = _per_ray(tnear, n, np.float64), _per_ray(tfar, n, np.float64)
    out = np.zeros(n, bool)
    nt = np.asarray(positions).reshape(-1, 9).shape[0]
    with np.errstate(all="ignore"):
        for a, b in _chunks(n, 2 * nt):
            det, u, v, t = _mt(positions, o[a:b], d[a:b], np.float64)
            m = np.minimum(np.minimum(u, v), 1.0 - u - v)
            lo, hi = tn[a:b, None], tf[a:b, None]
            near_edge = (np.abs(m) <= delta) & (t >= lo - delta * np.abs(lo)) & (t <= hi + delta * np.abs(hi))
            near_end = (m >= -delta) & ((np.abs(t - lo) <= delta * np.abs(lo)) | (np.abs(t - hi) <= delta * np.abs(hi)))
            out[a:b] = (near_edge | near_end | ~np.isfinite(det)).any(axis=1)
    return out


def reference_unsound(positions, o, d, tnear, tfar, delta=1e-3):
    """bool per ray: brute_any says hit, but of no accepted triangle does the float32 hit point o + t d lie in the
    triangle's own box (inflated by delta t |d| and 8 float32 ulp of the coordinates per axis).

    Why the any-hit tests drop these rays as well: a walk tests a subset of the triangles with brute force's very
    arithmetic, so it can only differ from brute_any by culling a box that holds an accepted triangle -- and a
    conservative box test cannot cull a box that the segment [tnear, tfar] enters, which it does when the accepted hit
    point lies inside the triangle's box.  On a sliver the float32 determinant keeps few bits (relative error about
    2^-24 x aspect: at aspect 1e6 the accepted t was seen off by a factor of 2), the accepted "hit" is then nowhere
    near the triangle, and whether a walk reports it depends on the tree.  Brute force is no reference for those rays;
    the closest-hit walks find them all the same (tfar is open there), and that is asserted without exclusion."""
    n = len(o)
    tn, tf = _per_ray(tnear, n, np.float32), _per_ray(tfar, n, np.float32)
    tri = np.asarray(positions, np.float32).reshape(-1, 3, 3).astype(np.float64)
    tlo, thi = tri.min(axis=1), tri.max(axis=1)
    o64, d64 = np.asarray(o, np.float32).astype(np.float64), np.asarray(d, np.float32).astype(np.float64)
    out = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for a, b in _chunks(n, 4 * len(tri)):
            ok, t = _accept(positions, o[a:b], d[a:b], tn[a:b], tf[a:b])
            t = t.astype(np.float64)[:, :, None]
            p = o64[a:b, None, :] + t * d64[a:b, None, :]
            slack = delta * np.abs(t * d64[a:b, None, :]) + 8 * 2.0 ** -24 * (np.abs(o64[a:b, None, :]) + np.abs(p))
            inside = ((p >= tlo[None] - slack) & (p <= thi[None] + slack)).all(axis=2)
            out[a:b] = ok.any(axis=1) & ~(ok & inside).any(axis=1)
    return out


# ---------------------------------------------------------------------------------------------- tree checker
def check_bvh_tree(nodes, prims, positions, leaf_max):
    """Asserts that (nodes (N, 8) float32, prims) -- Scene.bvh_tree() -- is a valid skip-pointer tree over `positions`
    (the positions last given to the scene): preorder skips, two children per interior node, leaf words that tile the
    triangle slots, prims a permutation, and exact (<=, no tolerance) containment of every triangle's float32 box in
    its leaf's box and of both child boxes in every interior box.  Triangles with a non-finite coordinate are exempt
    from containment, as in test_gpu_wide._check_conservative."""
    nodes = np.ascontiguousarray(nodes, np.float32)
    pos = np.asarray(positions, np.float32).reshape(-1, 9)
    N, n_tris = nodes.shape[0], pos.shape[0]
    assert N >= 1 and nodes.shape[1] == 8 and prims.shape == (n_tris,), (nodes.shape, prims.shape, n_tris)
    words = nodes.view(np.int32)
    skip, leaf = words[:, 3].astype(np.int64), words[:, 7].astype(np.int64)
    m = np.arange(N, dtype=np.int64)
    assert skip[0] == N, f"node 0 is not the root: skip {skip[0]} of {N} nodes"
    bad = np.flatnonzero(~((m < skip) & (skip <= N)))
    assert bad.size == 0, f"skip out of (m, n_nodes] at nodes {bad[:5]}: {skip[bad[:5]]}"
    inner = np.flatnonzero(leaf < 0)
    assert (leaf[inner] == -1).all()
    assert (inner + 1 < skip[inner]).all(), "an interior node without room for a child"
    c1 = inner + 1
    c2 = skip[c1]
    bad = inner[~((c2 > inner) & (c2 < skip[inner]))]
    assert bad.size == 0, f"second child outside (m, skip(m)) at nodes {bad[:5]}"
    bad = inner[skip[c2] != skip[inner]]
    assert bad.size == 0, f"second child's skip != the parent's at nodes {bad[:5]}"
    lv = np.flatnonzero(leaf >= 0)
    assert (skip[lv] == lv + 1).all(), "a leaf whose skip is not the next node"
    first, cnt = leaf[lv] >> 3, (leaf[lv] & 7) + 1
    assert cnt.max() <= leaf_max, f"leaf of {cnt.max()} triangles > {leaf_max}"
    order = np.argsort(first, kind="stable")
    ends = first[order] + cnt[order]
    assert first[order][0] == 0 and ends[-1] == n_tris and (first[order][1:] == ends[:-1]).all(), \
        "the leaf words do not tile [0, n_tris)"
    assert np.array_equal(np.sort(prims), np.arange(n_tris)), "prims is not a permutation"
    # containment
    tri = pos.reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        tlo, thi = tri.min(axis=1), tri.max(axis=1)
    owed = np.isfinite(tri).all(axis=(1, 2))
    lo, hi = nodes[:, 0:3], nodes[:, 4:7]
    slot_leaf = np.empty(n_tris, np.int64)
    for l, f, c in zip(lv, first, cnt):
        slot_leaf[f:f + c] = l
    t = prims.astype(np.int64)
    ok = ((lo[slot_leaf] <= tlo[t]) & (hi[slot_leaf] >= thi[t])).all(axis=1) | ~owed[t]
    assert ok.all(), f"{int((~ok).sum())} triangles stick out of their leaf box, first slot {np.flatnonzero(~ok)[:5]}"
    for c in (c1, c2):
        ok = ((lo[inner] <= lo[c]) & (hi[inner] >= hi[c])).all(axis=1)
        assert ok.all(), f"{int((~ok).sum())} interior boxes do not contain a child, first {inner[~ok][:5]}"
    return {"nodes": N, "leaves": int(lv.size), "max_leaf": int(cnt.max())}


# ---------------------------------------------------------------------------------------------- scenes
class HostileClass:
    """positions (T, 9) float32; scale = the unit of ray distances (tnear = 0.01 scale, miss tfar 2 / 5 scale);
    dist = sigma of the ray origins around their targets; grid = (z, lattice vertices) for the grid classes;
    hits = the least share of hostile closest rays that must hit something (the test is not vacuous)"""
    def __init__(self, name, positions, scale=1.0, dist=None, grid=None, hits=0.5):
        self.name, self.positions = name, np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
        self.scale, self.dist, self.grid, self.hits = float(scale), float(dist if dist is not None else scale), grid, hits
        self.tnear = F(0.01 * scale)

    @property
    def n_tris(self):
        return self.positions.shape[0]


def grid_positions(n=32, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """n x n quads, two triangles each, in z = 0 over [-1, 1]^2 (float64: scaled and moved before rounding)"""
    x = -1.0 + 2.0 * np.arange(n + 1) / n
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i, j = i.ravel(), j.ravel()
    z = np.zeros_like(i, np.float64)
    p00, p10 = np.stack([x[i], x[j], z], 1), np.stack([x[i + 1], x[j], z], 1)
    p01, p11 = np.stack([x[i], x[j + 1], z], 1), np.stack([x[i + 1], x[j + 1], z], 1)
    t = np.stack([np.concatenate([p00, p10, p11], 1), np.concatenate([p00, p11, p01], 1)], 1).reshape(-1, 3, 3)
    return (t * scale + np.asarray(offset, np.float64)).reshape(-1, 9)


def soup(n, seed, spread=(4.0, 2.0, 1.5), sigma=0.05):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)) * np.asarray(spread)
    return (c + rng.normal(scale=sigma, size=(n, 3, 3))).reshape(n, 9)


def _needles(aspect, seed, n=1024):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(a, rng.normal(size=(n, 3)))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    c = rng.uniform(-1, 1, (n, 3))
    return np.concatenate([c - a, c + a, c + b / aspect], 1)


def _mixed_soup(seed, n=3000):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10, 10, (n, 1, 3))
    s = 10.0 ** rng.uniform(-4, 1, (n, 1, 1))
    return (c + rng.normal(size=(n, 3, 3)) * s).reshape(n, 9)


def _dups(seed):
    g = grid_positions()
    t = g[1000].reshape(3, 3) + np.array([0.0, 0.0, 0.5])
    return np.concatenate([g, np.tile(t.reshape(1, 9), (300, 1))])


def _zero_area(seed):
    rng = np.random.default_rng(seed)
    g = grid_positions()
    pt = np.concatenate([rng.uniform(-1, 1, (100, 2)), rng.uniform(-0.5, 0.5, (100, 1))], 1)
    points = np.tile(pt, (1, 3))                                        # three equal points
    a = np.concatenate([rng.uniform(-1, 1, (100, 2)), rng.uniform(-0.5, 0.5, (100, 1))], 1).astype(np.float32)
    # exactly collinear in float32, along an axis or a diagonal of the plane: a, a + e, a + 2 e with a + e and
    # a + 2 e formed in float32 from power-of-two steps, so that e2 = 2 e1 exactly and the determinant is exactly 0
    e = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, -1, 0]], np.float32)[rng.integers(0, 4, 100)] * F(0.125)
    a = np.round(a * 1024) / 1024                                       # multiples of 2^-10: every sum below is exact
    lines = np.concatenate([a, a + e, a + 2 * e], 1).astype(np.float64)
    extra = np.concatenate([points, lines])
    out = np.concatenate([g, extra])
    where = rng.permutation(len(out))                                   # mixed in, not appended
    return out[where], np.flatnonzero(where >= len(g))


LADDER = (1, 2, 3, 8, 9, 16, 17, 18, 33, 255, 256, 257, 512, 513, 1025, 4097)
CLASS_NAMES = ("grid", "grid_far", "grid_tiny", "needles_1e2", "needles_1e4", "needles_1e6", "mixed_soup", "dups",
               "zero_area", "huge")


def _lattice(n=32, scale=1.0, offset=(0.0, 0.0, 0.0)):
    x = -1.0 + 2.0 * np.arange(n + 1) / n
    X, Y = np.meshgrid(x, x, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1) * scale + np.asarray(offset, np.float64)


def hostile_class(name):
    far = (4096.0, -4096.0, 2048.0)
    if name == "grid":
        return HostileClass(name, grid_positions(), grid=_lattice())
    if name == "grid_far":
        return HostileClass(name, grid_positions(offset=far), grid=_lattice(offset=far))
    if name == "grid_tiny":
        return HostileClass(name, grid_positions(scale=1e-3), scale=1e-3, grid=_lattice(scale=1e-3))
    if name.startswith("needles_"):
        asp = float(name.split("_")[1])
        return HostileClass(name, _needles(asp, 21), hits=0.2 if asp <= 1e4 else 0.0)
    if name == "mixed_soup":
        return HostileClass(name, _mixed_soup(22), dist=3.0, hits=0.3)
    if name == "dups":
        return HostileClass(name, _dups(23), grid=_lattice())
    if name == "zero_area":
        pos, zero = _zero_area(24)
        c = HostileClass(name, pos, grid=_lattice())
        c.never_hit = zero
        return c
    if name == "huge":
        # Moller-Trumbore's t needs a product of three lengths: at 1e20 it overflows float32 for every ray, so no ray
        # hits anything -- by brute force and by every walk alike.  The class is about the builder (the merged areas
        # overflow float32) and about walks over boxes of this size.
        return HostileClass(name, soup(500, 25) * 1e20, scale=1e20, hits=0.0)
    raise KeyError(name)


def ladder_class(n):
    return HostileClass(f"ladder_{n}", soup(n, 100 + n), hits=0.0)


# ---------------------------------------------------------------------------------------------- rays
def _aim(rng, targets, dist):
    """origins = target + N(0, dist) rounded to float32, directions normalised in float64 from the rounded origin"""
    o = (targets + rng.normal(size=targets.shape) * dist).astype(np.float32)
    d = targets - o.astype(np.float64)
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(nrm > 0, d / np.where(nrm > 0, nrm, 1.0), np.array([0.0, 0.0, 1.0]))
    return o, d.astype(np.float32)


def closest_rays(cls, seed=1, n=2048):
    """Hostile closest-hit rays: aimed at mesh vertices, edge midpoints and centroids; on the grid classes also
    axis-down rays from exactly above lattice vertices and rays inside the plane of the grid."""
    rng = np.random.default_rng(seed)
    tri = cls.positions.reshape(-1, 3, 3).astype(np.float64)
    n_aim = n - 512 if cls.grid is not None else n
    which = rng.integers(0, len(tri), n_aim)
    kind = rng.integers(0, 3, n_aim)
    k = rng.integers(0, 3, n_aim)
    vert = tri[which, k]
    mid = 0.5 * (tri[which, k] + tri[which, (k + 1) % 3])
    cen = tri[which].mean(axis=1)
    tgt = np.where((kind == 0)[:, None], vert, np.where((kind == 1)[:, None], mid, cen))
    o, d = _aim(rng, tgt, cls.dist)
    if cls.grid is not None:
        lat = cls.grid
        v = lat[rng.integers(0, len(lat), 256)]
        od = v + np.array([0.0, 0.0, 1.0]) * cls.scale * rng.uniform(0.25, 2.0, (256, 1))
        od = od.astype(np.float32)
        od[:, :2] = v[:, :2].astype(np.float32)                          # exactly above the (rounded) vertex
        dd = np.tile(np.array([0, 0, -1], np.float32), (256, 1))
        v = lat[rng.integers(0, len(lat), 256)]
        lo = lat.min(axis=0)
        op = np.stack([np.full(256, lo[0] - 0.5 * cls.scale), v[:, 1] + rng.integers(0, 2, 256) * 0.01 * cls.scale,
                       v[:, 2]], 1).astype(np.float32)                   # in the plane; half of them along an edge row
        dp = np.tile(np.array([1, 0, 0], np.float32), (256, 1))
        o, d = np.concatenate([o, od, op]), np.concatenate([d, dd, dp])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def anyhit_rays(cls, seed=2, n=1024, n_axis=1024):
    """(o, d, tnear, tfar): n rays aimed at interior points (every barycentric >= 0.05; every fifth direction random)
    and n_axis axis-parallel rays (d.x = 0, or d = (0, 0, -1)) from random origins.  tfar = 0.99 t of the brute-force
    closest hit, 1.01 t on every third ray; misses get 2 and 5 scene units."""
    rng = np.random.default_rng(seed)
    tri = cls.positions.reshape(-1, 3, 3).astype(np.float64)
    fin = np.flatnonzero(np.isfinite(tri).all(axis=(1, 2)))
    which = fin[rng.integers(0, len(fin), n)]
    b = 0.05 + 0.85 * rng.dirichlet((1.0, 1.0, 1.0), n)
    tgt = np.einsum("nk,nkc->nc", b, tri[which])
    o, d = _aim(rng, tgt, cls.dist)
    r = rng.normal(size=(len(d[::5]), 3))
    d[::5] = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)
    pts = tri[fin].reshape(-1, 3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    pad = 0.25 * cls.scale
    oa = rng.uniform(lo - pad, hi + pad + np.array([0, 0, cls.scale]), (n_axis, 3)).astype(np.float32)
    da = rng.normal(size=(n_axis, 3))
    da[:, 0] = 0.0
    da /= np.linalg.norm(da, axis=1, keepdims=True)
    da[::2] = np.array([0.0, 0.0, -1.0])
    o, d = np.concatenate([o, oa]), np.concatenate([d, da.astype(np.float32)])
    tn = np.full(len(o), cls.tnear, np.float32)
    t, prim = brute_closest(cls.positions, o, d, tn, F(3.0e38))
    hit = prim >= 0
    third = (np.arange(len(o)) % 3) == 0
    tf = np.where(hit, t * np.where(third, F(1.01), F(0.99)), np.where(third, F(5.0 * cls.scale), F(2.0 * cls.scale)))
    return np.ascontiguousarray(o), np.ascontiguousarray(d), tn, tf.astype(np.float32)


def scene_from_positions(pos):
    """a scenes.Scene of the Cornell material 0 over (T, 9) positions"""
    from restir_amd import scenes
    base = scenes.cornell_box(8)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    n = pos.shape[0]
    nrm = np.tile(np.array([0, 0, 1] * 3, np.float32), (n, 1))
    return scenes.Scene(pos, nrm, np.zeros(n, np.uint32), base.materials[:1], base.camera)


# ---------------------------------------------------------------------------------------------- the trees and their cases
# tree setting -> (RESTIR_BVH, RESTIR_WIDE): {PLOC (default), the Karras LBVH} x {8-wide tree live, switched off}
TREES = {"ploc_wide": (None, None), "ploc_skip": (None, "off"), "lbvh_wide": ("lbvh", None), "lbvh_skip": ("lbvh", "off")}


def soup32(n, seed, dup=0):
    """tests/test_gpu_wide.py's soup, in float32 throughout; the first `dup` triangles coincide"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)).astype(np.float32) * np.array([4, 2, 1.5], np.float32)
    p = (c + rng.normal(scale=0.05, size=(n, 3, 3)).astype(np.float32)).reshape(n, 9)
    if dup:
        p[:dup] = p[0]                   # coincident triangles: every centroid equal in a > 256-triangle node
    return p


def chain(n, ratio):
    """n triangles side by side along x, each `ratio` x the size of the previous: a binned / swept SAH split peels
    off the largest triangle at every level, so the source tree is a chain of depth n - 1 (the SAH-optimal 8-wide
    collapse of 100 such triangles needs exactly 8 levels; of 110, more than the walk's group stack holds)"""
    pos, x = [], 0.0
    for i in range(n):
        sz = ratio ** i
        pos.append([x, 0.0, 0.0, x + sz, 0.0, 0.0, x, sz, 0.0])
        x += sz
    return np.array(pos, np.float32)


def nonfinite_scene():
    """a soup with one NaN and one infinite coordinate: the scene loads without a wide tree"""
    p = soup32(800, 5)
    p[17, 4] = np.nan
    p[401, 0] = np.inf
    return scene_from_positions(p)


def depth8_scene():
    """a chain whose wide tree has exactly the walk's stack depth"""
    return scene_from_positions(chain(100, 1.5))


def wide_lib():
    """tests/cpp/wide_harness.cpp (rs_wide.h on the host), built on first use"""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "wide_harness.cpp")
    hdr = os.path.join(root, "restir-embree_amd", "csrc", "rs_wide.h")
    so = os.path.join(root, "oracle", "_build", "libwide_harness.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    L = ctypes.CDLL(so)
    L.wide_check.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int,
                             ctypes.c_int]
    L.wide_query.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return L
