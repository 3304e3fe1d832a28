"""Closed-form references and recorded bounds of the unbiased path tracer (rs_render_path_unbiased; checker
tests/cpp/path_oracle.c).  TEST INFRASTRUCTURE ONLY.

Scenes, references, measure(), the seeds and the caps are closed_form's.  This module adds what the new estimator
needs of its own: its estimator table, the quad under a uniform background (a closed form that exercises the
continuation sample, which the furnace does not), and the MEASURED figures of the checker with the bound function
over them.

Bounds, by closed_form's rule: nothing is compared against the code under test.  SE is the standard deviation of the
per-seed sum ratios over the 24 MEASURE_SEEDS, measured on the checker, divided by sqrt(len(SEEDS)); the sum-ratio
bound is 4 SE and may not exceed SUM_CAP; the per-pixel bounds are PIXEL_MARGIN x the checker's median and 99th
percentile on the image averaged over SEEDS.  No row is a quirk: every region must equal the light.
"""
from __future__ import annotations

import functools

import numpy as np

import closed_form as CF
from closed_form import MEASURE_SEEDS, PIXEL_MARGIN, SEEDS, SUM_CAP, measure  # noqa: F401
from restir_amd import params as P
from restir_amd import scenes

# name -> keyword arguments of render_path; "unbiased" is the direct-light ground truth (calc_gi off)
ESTIMATORS = {"unbiased": dict(calc_gi=False), "unbiased_m1": dict(max_bounces=1), "unbiased_m5": dict(max_bounces=5)}
SPP = {"open": 256, "blocked": 256, "furnace_steep": 512, "furnace_grazing": 512, "furnace_types_steep": 512,
       "furnace_types_grazing": 512}
DIRECT_SCENES = ("open", "blocked", *CF.FURNACE_SCENES)

# ---------------------------------------------------------------- the quad under a uniform background
QUAD_KD, QUAD_KS, QUAD_BG = (0.4, 0.3, 0.2), (0.3, 0.2, 0.3), (1.0, 2.0, 0.5)
QUAD_EXPONENTS = (1, 8, 500)
QUAD_W, QUAD_H, QUAD_SPP = 16, 12, 256
QUAD_BOUNCES = (1, 5)
QUAD_CAMERA = scenes.Camera(eye=(0.0, -2.0, 1.0), at=(0.0, 0.0, 0.0), fov_y=40.0)


@functools.lru_cache(maxsize=None)
def quad_scene(n):
    """One 10 x 10 Phong quad at z = 0 and no emitter: with use_skybox = 0 every direction of the upper hemisphere
    brings bg_color, so the radiance leaving the quad is the furnace value (kd + ks) bg for every view and exponent,
    and all of it arrives through the BRDF sample's ray missing the scene."""
    b = scenes._Builder()
    m = b.material(scenes.Material(kd=QUAD_KD, ks=QUAD_KS, shininess=float(n), type=scenes.PHONG))
    b.quad([-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0], m)
    return CF._finish(b, QUAD_CAMERA, f"quad_n{n}", QUAD_W, QUAD_H)


def quad_reference(cf, g):
    """closed_form.Reference of a quad scene for its G-buffer g: (kd + ks) bg on every pixel that hits the quad"""
    g = np.asarray(g, np.float64)
    mask = g[..., 16] > 0
    img = np.zeros(mask.shape)
    img[mask] = CF.furnace_expected(g[mask][:, 6:9], g[mask][:, 9:12], QUAD_BG, g[mask][:, 17]).sum(-1)
    return CF.Reference(mask, img, {"quad": mask.copy()}, None, g[mask][:, 0:3], g[mask][:, 3:6])


def get_scene(name):
    return quad_scene(int(name[6:])) if name.startswith("quad_n") else CF.get_scene(name)


def samples_for(scene):
    return QUAD_SPP if scene.startswith("quad_n") else SPP[scene]


def frame_params(scene, seed):
    if scene.startswith("quad_n"):
        return P.default_params(seed=seed, use_skybox=0, bg_color=QUAD_BG)
    return P.default_params(seed=seed)


# ---------------------------------------------------------------- the recorded checker figures and the bounds from them
# "scene/estimator/region": (ratio: mean over SEEDS, sd: over MEASURE_SEEDS, per-pixel median, p99) -- the checker's
# (tests/cpp/path_oracle.c) figures at samples_for(scene) samples per pixel
MEASURED = {
    "open/unbiased/all": (1.0005, 0.00117, 0.0083, 0.0397),
    "blocked/unbiased/lit": (1.0019, 0.00211, 0.0084, 0.0394),
    "blocked/unbiased/penumbra": (0.9972, 0.00481, 0.0191, 0.4072),
    "furnace_steep/unbiased/lambert": (1.0009, 0.00089, 0.0039, 0.0143),
    "furnace_steep/unbiased/phong_n1": (0.9992, 0.00107, 0.0052, 0.0217),
    "furnace_steep/unbiased/phong_n8": (0.9999, 0.00122, 0.0056, 0.0198),
    "furnace_steep/unbiased/spec_n64": (1.0000, 0.00023, 0.0018, 0.0058),
    "furnace_steep/unbiased/phong_n500": (0.9988, 0.00095, 0.0048, 0.0159),
    "furnace_grazing/unbiased/lambert": (0.9999, 0.00099, 0.0042, 0.0139),
    "furnace_grazing/unbiased/phong_n1": (0.9997, 0.00230, 0.0086, 0.0343),
    "furnace_grazing/unbiased/phong_n8": (0.9996, 0.00182, 0.0091, 0.0412),
    "furnace_grazing/unbiased/spec_n64": (0.9990, 0.00261, 0.0109, 0.0412),
    "furnace_grazing/unbiased/phong_n500": (1.0003, 0.00172, 0.0068, 0.0220),
    "furnace_types_steep/unbiased/lambert": (1.0009, 0.00089, 0.0039, 0.0143),
    "furnace_types_steep/unbiased/normal": (0.9996, 0.00091, 0.0037, 0.0162),
    "furnace_types_steep/unbiased/mirror": (1.0002, 0.00059, 0.0035, 0.0146),
    "furnace_types_steep/unbiased/dielectric": (1.0005, 0.00082, 0.0050, 0.0190),
    "furnace_types_steep/unbiased/transparent": (0.9993, 0.00088, 0.0035, 0.0132),
    "furnace_types_grazing/unbiased/lambert": (0.9999, 0.00099, 0.0042, 0.0139),
    "furnace_types_grazing/unbiased/normal": (0.9996, 0.00108, 0.0044, 0.0132),
    "furnace_types_grazing/unbiased/mirror": (1.0000, 0.00085, 0.0043, 0.0121),
    "furnace_types_grazing/unbiased/dielectric": (1.0001, 0.00239, 0.0096, 0.0311),
    "furnace_types_grazing/unbiased/transparent": (1.0002, 0.00109, 0.0044, 0.0126),
    "quad_n1/unbiased_m1/quad": (1.0000, 0.00206, 0.0094, 0.0307),
    "quad_n1/unbiased_m5/quad": (1.0000, 0.00206, 0.0094, 0.0307),
    "quad_n8/unbiased_m1/quad": (1.0001, 0.00169, 0.0073, 0.0302),
    "quad_n8/unbiased_m5/quad": (1.0001, 0.00169, 0.0073, 0.0302),
    "quad_n500/unbiased_m1/quad": (0.9998, 0.00038, 0.0014, 0.0075),
    "quad_n500/unbiased_m5/quad": (0.9998, 0.00038, 0.0014, 0.0075),
}


def bounds(scene, estimator, region):
    """(SE of the mean over SEEDS, sum-ratio bound 4 SE, per-pixel median bound, per-pixel p99 bound)"""
    _, sd, median, p99 = MEASURED[f"{scene}/{estimator}/{region}"]
    se = sd / np.sqrt(len(SEEDS))
    return se, 4.0 * se, PIXEL_MARGIN * median, PIXEL_MARGIN * p99


def check(scene, estimator, result, say=print):
    """Assert one measure() result against the bounds; prints every figure before it asserts.  No quirk rows."""
    failures = []
    for region, r in result.items():
        if region == "umbra":
            say(f"[closed-form] {scene}/{estimator}/umbra: level {r['level']:.3g} over {r['pixels']} pixels")
            if not r["level"] <= CF.UMBRA_BOUND:
                failures.append(f"umbra level {r['level']:.3g} > {CF.UMBRA_BOUND}")
            continue
        se, sum_bound, med_bound, p99_bound = bounds(scene, estimator, region)
        ratio = float(np.mean(r["ratios"]))
        say(f"[closed-form] {scene}/{estimator}/{region}: ratio {ratio:.4f} (SE {se:.4f}, bound {sum_bound:.4f}) "
            f"per-pixel median {r['median']:.4f} (<= {med_bound:.4f}) p99 {r['p99']:.4f} (<= {p99_bound:.4f}) "
            f"over {r['pixels']} pixels")
        assert sum_bound <= SUM_CAP, (scene, estimator, region, sum_bound)
        if not abs(ratio - 1.0) <= sum_bound:
            failures.append(f"{region}: sum ratio {ratio:.4f} off by more than {sum_bound:.4f}")
        if not r["median"] <= med_bound:
            failures.append(f"{region}: per-pixel median {r['median']:.4f} > {med_bound:.4f}")
        if not r["p99"] <= p99_bound:
            failures.append(f"{region}: per-pixel p99 {r['p99']:.4f} > {p99_bound:.4f}")
    assert not failures, f"{scene}/{estimator}: " + "; ".join(failures)
