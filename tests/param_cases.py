"""The frame-parameter sweep: one table of cases shared by tests/test_param_cases_oracle.py (the CPU oracle: every
case changes the frame, every frame is finite) and tests/test_gpu_param_sweep.py (the HIP renderer against the
oracle, element for element, in every pass form).  TEST INFRASTRUCTURE ONLY.

rs_frame_params has twenty fields; each case moves ONE of them away from BASE -- to the ends of its documented range,
to a value at which the code takes another path (a halo of 0, 1, 12 and 20 rows; a threshold that is NaN), or to a
value that folds into nothing if a pass kept the default as a constant.  BASE has temporal reuse, the visibility pass,
two spatial passes and reject_dissimilar on, so every field is read by some pass.

  CASES     name -> the fields it changes (frames of SIZE, FRAMES frames on material_cases.camera's orbit)
  SMALL     name -> ((W, H), fields): frames smaller than any neighbour offset
  AGREE     name -> (fields, the case it must equal): parameters that differ and must not change a bit
  scene(), params(case), size(case), oracle(case)
"""
from __future__ import annotations

import functools

import gpu_harness as GH
from material_cases import camera  # noqa: F401  (the sweep's frames ride the materials' orbit)
from restir_amd import params as P
from restir_amd import scenes

NAN, INF = float("nan"), float("inf")
SIZE, FRAMES = (64, 48), 3
BASE = dict(m_area=6, do_temporal=1, do_spatial=1, spatial_neighbors=4, spatial_passes=2, reject_dissimilar=1,
            do_visibility_pass=1)
MIN_CHANGED = 0.05            # the effect guard: the share of the last frame's pixels a case must change
BG = (0.1, 2.0, 7.5)

COMBINED = dict(confidence_cap=3, spatial_radius=150.0, min_normal_similarity=-1.0, max_depth_difference=0.05,
                tnear_offset=0.1, tfar_offset=0.0, normal_offset=0.05)

CASES = {
    # confidence_cap: k_initial, the temporal pass and spatial_store apply it; capped history is what a frame inherits
    "cap_0": dict(confidence_cap=0),
    "cap_1": dict(confidence_cap=1),
    "cap_3": dict(confidence_cap=3),
    "cap_max": dict(confidence_cap=P.MAX_CONFIDENCE_CAP),        # the largest accepted: nothing is ever capped
    # spatial_radius: neighbour offsets up to floor(sqrt(radius)) pixels; the halo rows of a tile are that many
    "radius_0": dict(spatial_radius=0.0),                        # every neighbour is the pixel itself
    "radius_0.99": dict(spatial_radius=0.99),                    # halo 0 with the spatial pass on
    "radius_1": dict(spatial_radius=1.0),                        # halo 1
    "radius_150": dict(spatial_radius=150.0),                    # halo 12
    "radius_400": dict(spatial_radius=400.0),                    # halo 20
    "radius_1e6": dict(spatial_radius=1.0e6),                    # up to 1000 px on a 64-px frame: all clamped
    "radius_max": dict(spatial_radius=P.MAX_SPATIAL_RADIUS),     # the largest accepted: offsets up to 2^28 px
    # the similarity thresholds of reject_dissimilar; a comparison with NaN is false, so a NaN threshold rejects
    # nothing (normal) or, for the depth, nothing either: dr < NaN and dr > NaN are both false
    "normal_sim_-1": dict(min_normal_similarity=-1.0),
    "normal_sim_1": dict(min_normal_similarity=1.0),
    "normal_sim_nan": dict(min_normal_similarity=NAN),
    "depth_diff_0": dict(max_depth_difference=0.0),
    "depth_diff_0.02": dict(max_depth_difference=0.02),
    "depth_diff_0.05": dict(max_depth_difference=0.05),
    "depth_diff_2": dict(max_depth_difference=2.0),
    "depth_diff_inf": dict(max_depth_difference=INF),
    "depth_diff_nan": dict(max_depth_difference=NAN),
    # the ray offsets: every shadow and BRDF ray of every pass form
    "tnear_0": dict(tnear_offset=0.0),
    "tnear_0.1": dict(tnear_offset=0.1),
    "tfar_0": dict(tfar_offset=0.0),                             # the shadow ray reaches the emitter itself
    "normal_off_0": dict(normal_offset=0.0),
    "normal_off_0.05": dict(normal_offset=0.05),
    "seed_0": dict(seed=0),
    "seed_ffffffff": dict(seed=0xFFFFFFFF),
    "bg_color": dict(bg_color=BG),                               # the miss pixels alone: reservoirs unchanged
    # the counts at their ends
    "area_0": dict(m_area=0),
    "brdf_0": dict(m_brdf=0),
    "brdf_3": dict(m_brdf=3),
    "nbr_0": dict(spatial_neighbors=0),
    "nbr_64": dict(spatial_neighbors=64),
    "passes_0": dict(spatial_passes=0),
    "passes_3": dict(spatial_passes=3),
    "combined": COMBINED,
}
SMALL = {
    "small_1x1": ((1, 1), dict(spatial_radius=400.0, confidence_cap=1)),
    "small_7x3": ((7, 3), dict(spatial_radius=400.0, confidence_cap=1)),
}
# Cases whose point is agreement: name -> (fields, the case whose run they must equal; None is BASE at their size).
# A negative depth window rejects every neighbour (hd = -0.5: dr < 1 - hd or dr > 1 + hd holds for every dr).  The
# one pixel of the 1 x 1 frame looks past the box (a miss carries bg_color as its emission) and its reservoir is
# empty under any parameters: that case is about a launch of one pixel whose every neighbour offset is clamped onto
# it, not about a value.
AGREE = {"depth_diff_-1": (dict(max_depth_difference=-1.0), "nbr_0"), "small_1x1": (SMALL["small_1x1"][1], None)}

ALL = (*CASES, *SMALL, "depth_diff_-1")
CONF_MAX = {"cap_0": 0, "cap_1": 1, "cap_3": 3, "cap_max": 94983}      # the largest final confidence, by the oracle
HALO = {"radius_0": 0, "radius_0.99": 0, "radius_1": 1, "radius_150": 12, "radius_400": 20}

# the cases of each pass form of tests/test_gpu_param_sweep.py (the single context runs ALL)
OFFSETS = ("tnear_0", "tnear_0.1", "tfar_0", "normal_off_0", "normal_off_0.05")
SORTED = (*OFFSETS, "cap_1", "radius_0", "radius_150", "radius_400")
SPLIT_AHEAD = ("cap_1", "radius_400", "tnear_0")
TILES = ("radius_0", "radius_0.99", "radius_1", "radius_150", "radius_400", "cap_1")
MGPU = ("radius_150", "radius_400")
TILE_SIZE = (64, 64)          # bands of 21 rows or more with 2 and 3 ranks: a 20-row halo fits

# the ground truths read the offsets, the seed and the background only
GT_SIZE, GT_SPP, GT_BOUNCES = (32, 24), 2, 3
GT_FIELDS = dict(tnear_offset=0.1, normal_offset=0.05, seed=0xFFFFFFFF, bg_color=BG)


@functools.lru_cache(maxsize=None)
def scene():
    return scenes.cornell_many_lights(128)


def fields(case):
    if case is None:
        return {}
    if case in SMALL:
        return SMALL[case][1]
    if case in AGREE:
        return AGREE[case][0]
    return CASES[case]


def params(case=None, **kw):
    """BASE with the case's fields (None: BASE itself), then kw"""
    return P.default_params(**{**BASE, **fields(case), **kw})


def size(case=None):
    return SMALL[case][0] if case in SMALL else SIZE


def changed_fields(case):
    """the names of the fields in which params(case) differs from params()"""
    a, b = params(case), params()
    out = []
    for name, _ in P.FrameParams._fields_:
        x, y = getattr(a, name), getattr(b, name)
        x, y = (tuple(x), tuple(y)) if name == "bg_color" else (x, y)
        if x != y and not (x != x and y != y):
            out.append(name)
    return out


@functools.lru_cache(maxsize=None)
def oracle(case=None, wh=None):
    """the oracle's run of `case` (None: BASE) at its own size, or at wh"""
    return GH.oracle_restir(scene(), params(case), wh or size(case), FRAMES, camera)


GT_KINDS = ("mis", "path", "unbiased")
GT_FRAMES = 2


def ground_truth(kind, render, prm, f):
    """frame f of one ground truth; render is a Renderer (with its scene handle bound) or the oracle's stand-in below"""
    if kind == "mis":
        return render.render_direct_mis(scene().camera, prm, f, GT_SPP)
    return render.render_path(scene().camera, prm, f, GT_SPP, max_bounces=GT_BOUNCES, unbiased=kind == "unbiased")


class _OracleTruths:
    def __init__(self):
        import oracle_lib as O
        self.o, self.os = O.OracleRenderer(*GT_SIZE), O.OracleScene(scene())

    def render_direct_mis(self, cam, prm, f, spp):
        return self.o.render_direct_mis(self.os, cam, prm, f, spp)

    def render_path(self, cam, prm, f, spp, **kw):
        import path_oracle as PO
        return PO.render_path(self.o, self.os, cam, prm, f, spp, **kw)


@functools.lru_cache(maxsize=None)
def oracle_truths(moved=True):
    """kind -> GT_FRAMES frames of the CPU checkers, with GT_FIELDS moved or at the defaults"""
    o, prm = _OracleTruths(), P.default_params(**(GT_FIELDS if moved else {}))
    out = {k: [ground_truth(k, o, prm, f) for f in range(GT_FRAMES)] for k in GT_KINDS}
    for frames in out.values():
        for a in frames:
            a.setflags(write=False)
    return out


def changed_share(a, b):
    """the share of pixels in which two frames differ"""
    return float((a != b).any(-1).mean())
