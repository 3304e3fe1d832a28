"""Times the NEE path tracer (rs_render_path, csrc/rs_path.h) with the library's device events.

C2 and C3 at 1920x1080, max_bounces 5, 1 and 8 samples per pixel: one warm-up launch, then the median of
--repeats launches (frame index varied, so the paths are different ones of the same distribution).  Writes
profiles/path_probe.json: ms per launch, rays, Mrays/s and ms(spp 8) / (8 ms(spp 1)) -- what the refill of
finished lanes with the next sample buys, since one sample per pixel leaves nothing to refill with -- and,
next to them, the path oracle's wall time for frame 0 on --threads host threads.

  python scripts/path_probe.py [--out profiles/path_probe.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_probe.json"))
    a = ap.parse_args()
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
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
