"""Fingerprints of every tree the GPU builders produce, for bit-identity checks across a change of the builders'
host code (tests/test_gpu_tree_fingerprints.py compares against tests/golden/tree_fingerprints.json).

Per case and tree setting (tests/bvh_brute.py TREES: {PLOC, RESTIR_BVH=lbvh} x {8-wide tree,
RESTIR_WIDE=off}) it records the SHA-256 of Scene.bvh_tree() (nodes and prims bytes), of Scene.wide_tree() (words,
prims and depth; "none" without a wide tree) and the rs_scene_walk_info status.  Cases: the soups of
bvh_brute.LADDER (1 .. 4097 triangles: the builders' n == 1 branches, the leaf maxima, PLOC's radius, the workgroup
size, kSmall, and one size above the wide builder's kChunk), every bvh_brute.CLASS_NAMES class, a
non-finite scene and a chain of exactly the walk's depth (bvh_brute.nonfinite_scene / depth8_scene), and the 64-light Cornell box.

    python scripts/tree_fingerprints.py --out tests/golden/tree_fingerprints.json     # record (at the parent commit)
    python scripts/tree_fingerprints.py --check tests/golden/tree_fingerprints.json   # compare, exit 1 on a difference
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "restir-embree_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TREES = {"ploc_wide": (None, None), "ploc_skip": (None, "off"), "lbvh_wide": ("lbvh", None), "lbvh_skip": ("lbvh", "off")}


# The recorder is run at a parent commit too (see above), so beyond the generators that tests/bvh_brute.py has had
# since the recording was made it carries its own statement of the two remaining scenes;
# tests/test_gpu_tree_fingerprints.py holds them equal, bit for bit, to bvh_brute.nonfinite_scene / depth8_scene.
def _nonfinite_positions():
    """a float32 soup of 800 triangles (seed 5) with one NaN and one infinite coordinate"""
    rng = np.random.default_rng(5)
    c = rng.uniform(-1, 1, (800, 1, 3)).astype(np.float32) * np.array([4, 2, 1.5], np.float32)
    p = (c + rng.normal(scale=0.05, size=(800, 3, 3)).astype(np.float32)).reshape(800, 9)
    p[17, 4] = np.nan
    p[401, 0] = np.inf
    return p


def _depth8_positions():
    """100 triangles side by side along x, each 1.5 x the previous: a wide tree of exactly the walk's stack depth"""
    pos, x = [], 0.0
    for i in range(100):
        sz = 1.5 ** i
        pos.append([x, 0.0, 0.0, x + sz, 0.0, 0.0, x, sz, 0.0])
        x += sz
    return np.array(pos, np.float32)


def cases():
    """name -> callable returning the scenes.Scene (built lazily: the generators are numpy only)"""
    import bvh_brute as B
    from restir_amd import scenes
    out = {}
    for n in B.LADDER:
        out[f"ladder_{n}"] = lambda n=n: B.scene_from_positions(B.ladder_class(n).positions)
    for name in B.CLASS_NAMES:
        out[name] = lambda name=name: B.scene_from_positions(B.hostile_class(name).positions)
    out["nonfinite"] = lambda: B.scene_from_positions(_nonfinite_positions())
    out["depth8"] = lambda: B.scene_from_positions(_depth8_positions())
    out["cornell_64"] = lambda: scenes.cornell_many_lights(64)
    return out


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def fingerprint(gs):
    """{"bvh", "wide", "status"} of a loaded scene"""
    nodes, prims = gs.bvh_tree()
    wt = gs.wide_tree()
    wide = "none" if wt is None else _sha(wt[0], wt[1], np.int32(wt[2]))
    return {"bvh": _sha(nodes, prims), "wide": wide, "status": str(gs.walk_info()["status"])}


def set_tree_env(tree):
    """the builders read both variables at every build"""
    for k, v in zip(("RESTIR_BVH", "RESTIR_WIDE"), TREES[tree]):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def case_fingerprints(renderer, scene):
    """{tree: {"first": fingerprint of the first build, "rebuilt": fingerprint after one rebuild()}}; leaves
    RESTIR_BVH / RESTIR_WIDE at the last setting (the caller restores them)"""
    out = {}
    for tree in TREES:
        set_tree_env(tree)
        gs = renderer.load_scene(scene)
        first = fingerprint(gs)
        gs.rebuild()
        out[tree] = {"first": first, "rebuilt": fingerprint(gs)}
        gs.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="write the fingerprints of the first builds here (JSON)")
    ap.add_argument("--check", help="compare with this recording; exit 1 when a case differs")
    a = ap.parse_args()
    from restir_amd.renderer import Renderer
    r = Renderer(8, 8)
    got, unstable = {}, []
    for name, make in cases().items():
        fp = case_fingerprints(r, make())
        got[name] = {t: v["first"] for t, v in fp.items()}
        unstable += [f"{name}/{t}" for t, v in fp.items() if v["first"] != v["rebuilt"]]
        print(name, json.dumps(got[name]), flush=True)
    r.close()
    if unstable:
        print("rebuild() changed the tree:", ", ".join(unstable))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    bad = []
    if a.check:
        want = json.load(open(a.check))
        bad = [k for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
        print(f"{len(got) - len(bad)} of {len(got)} cases equal {a.check}" + (f"; differ: {bad}" if bad else ""))
    sys.exit(1 if bad or unstable else 0)


if __name__ == "__main__":
    main()
