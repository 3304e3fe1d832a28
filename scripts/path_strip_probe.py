"""Times the ground truths' row sets (rs_render_ground_truth_rows) with the library's device events, by
scripts/path_probe.py's method: 1920x1080, max_bounces 5, C2 and C3, one warm-up launch, then the median of --repeats
launches (frame index varied).

  python scripts/path_strip_probe.py --entries [--tree DIR] [--out FILE]
      the full-frame entries rs_render_path and rs_render_path_unbiased at --spp (8).  --tree DIR takes the package
      and its library from another checkout's restir-embree_amd (a build of the parent commit), so that a job script
      can alternate processes of the two builds in one session and compare; every process writes its own file.

  python scripts/path_strip_probe.py [--world 8] [--out profiles/path_strips.json]
      one rank's share of a `world`-rank ground truth, every share timed alone on this one GPU: the interleaved
      phases {16, world, p} against `world` contiguous equal bands of whole strips, {16 ceil(strips / world), world,
      p}.  Per assignment: every share's ms, max, mean, max / mean, and the sum over the shares divided by the
      full-frame launch's ms.  A one-GPU compute floor of the slowest rank, not a scaling result: no gather, no
      second device.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def workload(name):
    from restir_amd import params as P, scenes
    if name == "C2":
        return scenes.cornell_many_lights(1024), P.metric_params()
    return scenes.sponza_like(), P.c3_params()


def timed(g, gs, sc, prm, a, unbiased, rows=None):
    """(median ms, min, max, rays of frame 0) of --repeats launches after one warm-up"""
    kw = dict(max_bounces=a.bounces, copy_out=False, timed=True, unbiased=unbiased)
    if rows is not None:
        kw["rows"] = rows
    ms, rays = [], 0
    for f in range(-1, a.repeats):
        g.render_path(gs, sc.camera, prm, max(f, 0), a.spp, **kw)
        if f >= 0:
            ms.append(float(g.last_times.shade_ms))
        if f == 0:
            rays = int(g.last_times.rays)
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "rays": rays}


def entries(a, Renderer):
    res = {}
    for name in a.configs.split(","):
        sc, prm = workload(name)
        g = Renderer(a.width, a.height)
        gs = g.load_scene(sc)
        res[name] = {est: timed(g, gs, sc, prm, a, est == "unbiased") for est in ("reference", "unbiased")}
        print(name, res[name], flush=True)
        gs.close()
        g.close()
    return res


def shares(a, Renderer):
    n_strips = (a.height + 15) // 16
    band = 16 * ((n_strips + a.world - 1) // a.world)
    res = {}
    for name in a.configs.split(","):
        sc, prm = workload(name)
        g = Renderer(a.width, a.height)
        gs = g.load_scene(sc)
        rows = {}
        for est in ("reference", "unbiased"):
            full = timed(g, gs, sc, prm, a, est == "unbiased")
            row = {"full_frame": full}
            for label, strip in (("interleaved", 16), ("contiguous", band)):
                t = [timed(g, gs, sc, prm, a, est == "unbiased", (strip, a.world, p)) for p in range(a.world)]
                ms = [v["ms"] for v in t]
                assert sum(v["rays"] for v in t) == full["rays"], (name, est, label)
                row[label] = {"strip_rows": strip, "ms": ms, "rays": [v["rays"] for v in t], "max_ms": max(ms),
                              "mean_ms": round(statistics.mean(ms), 4),
                              "max_over_mean": round(max(ms) / statistics.mean(ms), 4),
                              "sum_over_full_frame": round(sum(ms) / full["ms"], 4)}
            rows[est] = row
            print(name, est, row, flush=True)
        res[name] = rows
        gs.close()
        g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--entries", action="store_true")
    ap.add_argument("--tree", default=os.path.join(ROOT, "restir-embree_amd"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from restir_amd.renderer import Renderer
    res = {"width": a.width, "height": a.height, "max_bounces": a.bounces, "spp": a.spp, "repeats": a.repeats,
           "timer": "rs_pass_times.shade_ms (device events around the launch), one warm-up launch, median"}
    if a.entries:
        res["tree"] = os.path.relpath(os.path.abspath(a.tree), ROOT)
        res["configs"] = entries(a, Renderer)
    else:
        res["world"] = a.world
        res["note"] = "every share timed alone on one GPU: a compute floor of the slowest rank, not a scaling result"
        res["configs"] = shares(a, Renderer)
    out = a.out or os.path.join(ROOT, "profiles", "path_strips_entries.json" if a.entries else "path_strips.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
