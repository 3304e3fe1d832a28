"""Times the NEE path tracer (rs_render_path, csrc/rs_path.h) with the library's device events.

C2 and C3 at 1920x1080, max_bounces 5, 1 and 8 samples per pixel: one warm-up launch, then the median of
--repeats launches (frame index varied, so the paths are different ones of the same distribution).  Writes
profiles/path_probe.json: ms per launch, rays, Mrays/s and ms(spp 8) / (8 ms(spp 1)) -- what the refill of
finished lanes with the next sample buys, since one sample per pixel leaves nothing to refill with -- and,
next to them, the path oracle's wall time for frame 0 on --threads host threads.

  python scripts/path_probe.py [--out profiles/path_probe.json]

--unbiased: the unbiased estimator (rs_render_path_unbiased, k_path<T, kEstUnbiased>) beside the reference's on the
same four configs instead -- after a warm-up of both, --repeats pairs of launches alternating between the two kernels
in one session, the median of each.  Writes profiles/path_probe_unbiased.json: ms per launch, rays and Mrays/s of
both, and unbiased / reference in ms and in rays.

  python scripts/path_probe.py --unbiased [--out profiles/path_probe_unbiased.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "restir-embree_amd"), os.path.join(ROOT, "tests")]

import oracle_lib as O  # noqa: E402
import path_oracle as PO  # noqa: E402
from restir_amd import params as P, scenes  # noqa: E402
from restir_amd.renderer import Renderer  # noqa: E402


def workload(name):
    if name == "C2":
        return scenes.cornell_many_lights(1024), P.metric_params()
    return scenes.sponza_like(), P.c3_params()


def _row(ms, rays):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "rays_frame0": rays, "mrays_per_s": round(rays / (ms[0] * 1e3), 1)}


def compare(a):
    """the reference's estimator and the unbiased one, alternating"""
    W, H = a.width, a.height
    res = {"width": W, "height": H, "max_bounces": a.bounces, "repeats": a.repeats,
           "timer": "rs_pass_times.shade_ms (device events around the launch)",
           "protocol": "one warm-up launch of each kernel, then reference and unbiased launches alternating", "configs": {}}
    for name in a.configs.split(","):
        sc, prm = workload(name)
        g = Renderer(W, H)
        gs = g.load_scene(sc)
        rows = {}
        for spp in map(int, a.spp.split(",")):
            ms, rays = {False: [], True: []}, {}
            for f in range(-1, a.repeats):                      # -1: the warm-up pair
                for unbiased in (False, True):
                    g.render_path(gs, sc.camera, prm, max(f, 0), spp, max_bounces=a.bounces, copy_out=False, timed=True,
                                  unbiased=unbiased)
                    if f >= 0:
                        ms[unbiased].append(float(g.last_times.shade_ms))
                    if f == 0:
                        rays[unbiased] = int(g.last_times.rays)
            row = {"reference": _row(ms[False], rays[False]), "unbiased": _row(ms[True], rays[True])}
            row["ms_unbiased_over_reference"] = round(row["unbiased"]["ms"] / row["reference"]["ms"], 4)
            row["rays_unbiased_over_reference"] = round(rays[True] / rays[False], 4)
            rows[f"spp{spp}"] = row
            print(name, spp, row, flush=True)
        res["configs"][name] = rows
        gs.close()                      # a scene goes before its context
        g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--spp", default="1,8")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--unbiased", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "path_probe_unbiased.json" if a.unbiased else "path_probe.json")
    if a.unbiased:
        return write(a.out, compare(a))
    W, H = a.width, a.height
    res = {"width": W, "height": H, "max_bounces": a.bounces, "repeats": a.repeats, "oracle_threads": a.threads,
           "timer": "rs_pass_times.shade_ms (device events around the launch)", "configs": {}}
    for name in a.configs.split(","):
        sc, prm = workload(name)
        g = Renderer(W, H)
        gs = g.load_scene(sc)
        o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
        rows = {}
        for spp in map(int, a.spp.split(",")):
            g.render_path(gs, sc.camera, prm, 0, spp, max_bounces=a.bounces, copy_out=False, timed=True)   # warm-up
            ms, rays = [], 0
            for f in range(a.repeats):
                g.render_path(gs, sc.camera, prm, f, spp, max_bounces=a.bounces, copy_out=False, timed=True)
                ms.append(float(g.last_times.shade_ms))
                rays = int(g.last_times.rays) if f == 0 else rays
            med = statistics.median(ms)
            row = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "rays_frame0": rays,
                   "mrays_per_s": round(rays / (ms[0] * 1e3), 1)}
            if not a.no_oracle:
                with O.num_threads(a.threads):
                    t0 = time.perf_counter()
                    PO.render_path(o, os_, sc.camera, prm, 0, spp, max_bounces=a.bounces)
                    row["oracle_s"] = round(time.perf_counter() - t0, 3)
                    row["oracle_rays"] = o.rays
            rows[f"spp{spp}"] = row
            print(name, spp, row, flush=True)
        if "spp1" in rows and "spp8" in rows:
            rows["spp8_over_8_spp1"] = round(rows["spp8"]["ms"] / (8.0 * rows["spp1"]["ms"]), 4)
        res["configs"][name] = rows
        gs.close()                      # a scene goes before its context
        g.close()
    write(a.out, res)


def write(out, res):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
