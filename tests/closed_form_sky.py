"""Closed-form references, sky textures and recorded bounds of the sky-light path tracer (rs_render_path_sky; checker
tests/cpp/sky_oracle.c).  TEST INFRASTRUCTURE ONLY.

Scenes, measure(), the seeds and the caps are closed_form's and closed_form_unbiased's.  This module adds the skies, a
Lambert quad under a sky with a sun (expected radiance by Gauss-Legendre quadrature of the bilinear radiance function,
restated here in numpy float64 from its definition), the Phong quads under a uniform sky and under bg_color, a sealed
room, a numpy restatement of the integer sampling tables (restir-embree_amd/csrc/rs_sky.h), and the MEASURED figures
of the checker with the bound function over them.

Bounds, by closed_form's rule: nothing is compared against the code under test.  SE is the standard deviation of the
per-seed sum ratios over the 24 MEASURE_SEEDS, measured on the checker, divided by sqrt(len(SEEDS)); the sum-ratio
bound is 4 SE and may not exceed SUM_CAP; the per-pixel bounds are PIXEL_MARGIN x the checker's median and 99th
percentile on the image averaged over SEEDS.
"""
from __future__ import annotations

import functools

import numpy as np

import closed_form as CF
import closed_form_unbiased as CU
import oracle_lib as O
from closed_form import MEASURE_SEEDS, PIXEL_MARGIN, SEEDS, SUM_CAP, measure  # noqa: F401
from restir_amd import params as P
from restir_amd import scenes

# name -> keyword arguments of render_path(unbiased=True, sky_light=True)
ESTIMATORS = {"sky_nogi": dict(calc_gi=False), "sky_m0": dict(max_bounces=0), "sky_m1": dict(max_bounces=1),
              "sky_m5": dict(max_bounces=5)}
SUN_ESTIMATORS = ("sky_nogi", "sky_m0", "sky_m5")       # one expectation: the scene is convex
SPP = 256
W, H = CU.QUAD_W, CU.QUAD_H

# ---------------------------------------------------------------- skies
SKY_W, SKY_H = 32, 16
SKY_DIM, SKY_SUN = (0.10, 0.12, 0.15), (4000.0, 3500.0, 2500.0)
SUN_ROWS, SUN_COLS = (3, 4), (20, 21)                   # texel row y is the polar angle y / 16 * 180 deg: 33.75 and 45


def sun_sky():
    """32 x 16 float RGB: dim everywhere, a 2 x 2 block of texels at about 40 degrees from the zenith 4000 times brighter"""
    t = np.empty((SKY_H, SKY_W, 3), np.float32)
    t[...] = SKY_DIM
    t[SUN_ROWS[0]:SUN_ROWS[1] + 1, SUN_COLS[0]:SUN_COLS[1] + 1] = SKY_SUN
    return scenes.Texture(t)


def zenith_sky():
    """the sun at the zenith: the two top texel rows; nothing from below the horizon (texel row 8 is the horizon: the
    lookup reaches zero there), so that a roof's underside sees no sky past the quad's edge"""
    t = np.empty((SKY_H, SKY_W, 3), np.float32)
    t[...] = SKY_DIM
    t[0:2] = SKY_SUN
    t[SKY_H // 2:] = 0.0
    return scenes.Texture(t)


def bright_sky():
    """32 x 16 float RGB, every texel within a factor of three of every other: every cell's integer weight is above
    4000, so a sample's position inside its cell is fine-grained.  (Under sun_sky the dim cells weigh 2: their
    samples land on two columns per cell, among them directions that lie in a coordinate plane exactly.)"""
    return scenes.Texture((1.0 + 2.0 * np.random.default_rng(8).random((SKY_H, SKY_W, 3))).astype(np.float32))


def uniform_sky(rgb=CU.QUAD_BG):
    t = np.empty((4, 8, 3), np.float32)
    t[...] = rgb
    return scenes.Texture(t)


# sizes of the table tests: 63 / 64 / 65 cross the wave of the device's scan, 257 and 1025 its workgroup chunk
TABLE_SIZES = ((1, 1), (1, 5), (5, 1), (63, 3), (64, 2), (65, 2), (257, 3), (1025, 2))
TABLE_FORMATS = ("f32_rgb", "u8_rgb", "u8_1")


def table_sky(w, h, fmt, seed=11):
    rng = np.random.default_rng(seed + 1000 * w + h)
    if fmt == "f32_rgb":
        return scenes.Texture((rng.random((h, w, 3)) ** 4 * 50.0).astype(np.float32))
    if fmt == "u8_rgb":
        return scenes.Texture(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return scenes.Texture(rng.integers(0, 256, (h, w, 1), dtype=np.uint8))


def black_sky():
    return scenes.Texture(np.zeros((4, 8, 3), np.float32))


def hostile_sky():
    """a NaN texel and a negative texel among ordinary ones"""
    t = (np.random.default_rng(3).random((6, 9, 3)) * 3.0).astype(np.float32)
    t[2, 4] = np.nan
    t[4, 1] = -5.0
    return scenes.Texture(t)


# ---------------------------------------------------------------- the tables, restated (rs_sky.h)
def _texels(tex):
    """(h, w, 3) float32: what the lookup's texel read returns for every texel, byte order and the 1-channel
    three-byte read included (rows padded to 4 bytes, zeros behind the last row)"""
    a = np.asarray(tex.data)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.dtype != np.uint8:
        return a[..., :3].astype(np.float32)
    if a.shape[2] >= 3:
        return a[..., :3].astype(np.float32) / np.float32(255.0)
    h, w = a.shape[:2]
    pitch = (w + 3) & ~3
    buf = np.zeros(pitch * h + 16, np.uint8)
    for y in range(h):
        buf[y * pitch:y * pitch + w] = a[y, :, 0]
    off = (np.arange(h)[:, None] * pitch + np.arange(w)[None, :])
    return np.stack([buf[off + 2], buf[off + 1], buf[off]], -1).astype(np.float32) / np.float32(255.0)


def numpy_tables(tex):
    """(row_cdf (h, w) uint32, marginal (h,) uint64)"""
    t = _texels(tex)
    h, w = t.shape[:2]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (t[..., 0] + t[..., 1]) + t[..., 2]
        i1, j1 = np.minimum(np.arange(w) + 1, w - 1), np.minimum(np.arange(h) + 1, h - 1)
        total = (s + s[:, i1]) + (s[j1, :] + s[j1][:, i1])
        sin_row = O.libm_f1("sinf", np.float32(np.pi) * (np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h))
        wgt = np.where(total > 0, total, np.float32(0.0)) * sin_row[:, None]
        wgt = np.where(wgt > 0, wgt, np.float32(0.0)).astype(np.float32)
        r = wgt / wgt.max() * np.float32(65535.0)
        r = np.minimum(np.where(r >= 0, r, np.float32(0.0)), np.float32(65535.0))
        q = np.where(wgt > 0, r.astype(np.uint32) + np.uint32(1), np.uint32(0)).astype(np.uint32)
    cdf = np.cumsum(q, axis=1, dtype=np.uint32)
    return cdf, np.cumsum(cdf[:, -1].astype(np.uint64), dtype=np.uint64)


# ---------------------------------------------------------------- the radiance function and its cosine integral
def sky_radiance(tex, px, py):
    """The bilinear lookup's definition in float64: texel (x, y) is the value at texel coordinates (x, y), edges clamped"""
    t = np.asarray(tex.data, np.float64)
    h, w = t.shape[:2]
    fx, fy = np.floor(px), np.floor(py)
    tx, ty = (px - fx)[..., None], (py - fy)[..., None]
    x0, x1 = np.clip(fx, 0, w - 1).astype(int), np.clip(fx + 1, 0, w - 1).astype(int)
    y0, y1 = np.clip(fy, 0, h - 1).astype(int), np.clip(fy + 1, 0, h - 1).astype(int)
    a = t[y0, x0] * (1 - tx) + t[y0, x1] * tx
    b = t[y1, x0] * (1 - tx) + t[y1, x1] * tx
    return a * (1 - ty) + b * ty


def sky_irradiance(tex, order=8):
    """(3,) the integral of L cos(theta) over the hemisphere around +z, Gauss-Legendre of `order` points per axis on
    every cell of texel-coordinate space: theta = py / h pi, phi = (px / w - 1/2) 2 pi, d omega = sin(theta) d theta d phi"""
    h, w = np.asarray(tex.data).shape[:2]
    assert h % 2 == 0                                      # the horizon is a cell boundary
    x, wt = np.polynomial.legendre.leggauss(order)
    x, wt = 0.5 * (x + 1.0), 0.5 * wt
    px = (np.arange(w)[:, None] + x[None, :]).reshape(-1)
    py = (np.arange(h // 2)[:, None] + x[None, :]).reshape(-1)
    wx, wy = np.tile(wt, w), np.tile(wt, h // 2)
    PX, PY = np.meshgrid(px, py)
    theta = PY / h * np.pi
    f = sky_radiance(tex, PX, PY) * (np.cos(theta) * np.sin(theta))[..., None]
    return (f * (wy[:, None] * wx[None, :])[..., None]).sum((0, 1)) * (np.pi / h) * (2 * np.pi / w)


# ---------------------------------------------------------------- scenes
SUN_KD = CU.QUAD_KD


def _quad(b, m):
    b.quad([-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0], m)


@functools.lru_cache(maxsize=None)
def get_scene(name):
    """sun_quad: the 10 x 10 Lambert quad at z = 0 under sun_sky; sealed_room: the same under a 1000 x 1000 opaque roof at
    z = 3, sun at the zenith; skyquad_n<N>: closed_form_unbiased's Phong quad under a uniform sky of QUAD_BG; bgquad_n<N>:
    the same with use_skybox = 0 and bg_color = QUAD_BG"""
    b = scenes._Builder()
    if name in ("sun_quad", "sealed_room"):
        _quad(b, b.material(scenes.Material(kd=SUN_KD, type=scenes.LAMBERT)))
        if name == "sealed_room":
            r = b.material(scenes.Material(kd=(0.5, 0.5, 0.5), type=scenes.LAMBERT))
            b.quad([-500, -500, 3], [-500, 500, 3], [500, 500, 3], [500, -500, 3], r)
        sky = sun_sky() if name == "sun_quad" else zenith_sky()
    else:
        kind, n = name.split("_n")
        _quad(b, b.material(scenes.Material(kd=CU.QUAD_KD, ks=CU.QUAD_KS, shininess=float(n), type=scenes.PHONG)))
        sky = uniform_sky() if kind == "skyquad" else None
    cf = CF._finish(b, CU.QUAD_CAMERA, name, W, H)
    cf.scene.sky = sky
    return cf


ROOM_HALF, ROOM_Z = 500.0, 3.0
# the projected solid angle the roof leaves open as seen from the quad's nearest edge: pi sin^2 of the gap's elevation
ROOM_GAP = float(np.pi * np.sin(np.arctan(ROOM_Z / (ROOM_HALF - 5.0))) ** 2)


def frame_params(scene, seed):
    if scene.startswith("bgquad"):
        return P.default_params(seed=seed, use_skybox=0, bg_color=CU.QUAD_BG)
    return P.default_params(seed=seed, use_skybox=1)


def sun_expected(order=8):
    """(3,) radiance leaving the Lambert quad under sun_sky: kd / pi times the sky's cosine integral"""
    return np.asarray(SUN_KD) / np.pi * sky_irradiance(sun_sky(), order)


def reference(cf, g):
    """closed_form.Reference for the G-buffer g: sun_quad -- sun_expected on every pixel of the quad; the Phong quads --
    closed_form_unbiased.quad_reference, (kd + ks) bg"""
    if cf.name != "sun_quad":
        return CU.quad_reference(cf, g)
    g = np.asarray(g, np.float64)
    mask = g[..., 16] > 0
    img = np.zeros(mask.shape)
    img[mask] = sun_expected().sum()
    return CF.Reference(mask, img, {"quad": mask.copy()}, None, g[mask][:, 0:3], g[mask][:, 3:6])


# ---------------------------------------------------------------- the recorded checker figures and the bounds from them
# "scene/estimator/region": (ratio: mean over SEEDS, sd: over MEASURE_SEEDS, per-pixel median, p99) -- the checker's
# (tests/cpp/sky_oracle.c) figures at SPP samples per pixel
MEASURED = {
    "sun_quad/sky_nogi/quad": (1.0011, 0.00220, 0.0130, 0.0462),
    "sun_quad/sky_m0/quad": (1.0011, 0.00220, 0.0130, 0.0462),
    "sun_quad/sky_m5/quad": (1.0011, 0.00220, 0.0130, 0.0462),
    "skyquad_n1/sky_m1/quad": (1.0003, 0.00273, 0.0103, 0.0433),
    "skyquad_n8/sky_m1/quad": (1.0010, 0.00325, 0.0092, 0.0418),
    "skyquad_n500/sky_m1/quad": (1.0007, 0.00168, 0.0068, 0.0287),
    "bgquad_n1/sky_nogi/quad": (1.0000, 0.00206, 0.0094, 0.0307),
    "bgquad_n8/sky_nogi/quad": (1.0001, 0.00169, 0.0073, 0.0302),
    "bgquad_n500/sky_nogi/quad": (0.9998, 0.00038, 0.0014, 0.0075),
}

# Per-pixel variance over the 24 MEASURE_SEEDS on sun_quad at VARIANCE_SPP samples per pixel, summed over the quad's
# pixels: or_render_path_unbiased (max_bounces = 1: there the same expectation) over or_render_path_sky (calc_gi = 0),
# as measured on the checker
VARIANCE_SPP = 16
VARIANCE_RATIO = 71.65


def variance_ratio(render_sky, render_unbiased, mask):
    """render_*(seed) -> (H, W, 3); the ratio above"""
    a = np.stack([render_sky(s).astype(np.float64).sum(-1) for s in MEASURE_SEEDS])
    b = np.stack([render_unbiased(s).astype(np.float64).sum(-1) for s in MEASURE_SEEDS])
    return float(b.var(axis=0, ddof=1)[mask].sum() / a.var(axis=0, ddof=1)[mask].sum())


def bounds(scene, estimator, region):
    """(SE of the mean over SEEDS, sum-ratio bound 4 SE, per-pixel median bound, per-pixel p99 bound)"""
    _, sd, median, p99 = MEASURED[f"{scene}/{estimator}/{region}"]
    se = sd / np.sqrt(len(SEEDS))
    return se, 4.0 * se, PIXEL_MARGIN * median, PIXEL_MARGIN * p99


def check(scene, estimator, result, say=print):
    """Assert one measure() result against the bounds; prints every figure before it asserts."""
    failures = []
    for region, r in result.items():
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
