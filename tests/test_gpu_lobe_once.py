"""GPU tests: the Phong lobe's power taken once per direction (rs_device.h lobe_pow) -- the pdf's pow(max(0, d), n)
and the BRDF's pow(max(d, 0), n) of one area candidate are one rs_powf_sel where the two bases are the same bits,
and the BRDF keeps a power of its own where they are not (d NaN or -0).

One room holds every case: its floor and back wall are 0.1 m patches that cycle through PATCHES, so every 8 x 8
wave tile on them mixes Lambert and Phong pixels and the shininess edges -- odd integers (1, 3, 65: the sign of a
negative base), even ones (2, 64), a non-integer (12.5), 0, a negative one (-3), +inf, ks = 0 on a Phong type (the
pdf skips the lobe, the BRDF does not) and a Phong patch of shininess 3 whose vertex normals are zero: its shading
normal is 0 * inf = NaN, so is the mirror direction, and d is NaN for every light direction.  (Such a pixel's
cosine is NaN too, so its L is NaN whatever the power: the case shows that the own-power path runs and leaves
the frame and the reservoirs as the oracle has them, not that a wrong power would be seen.  A d of -0 needs all
three products of the dot to be -0 -- an axis-parallel light direction; no rendered candidate has one.)

Every initial-pass kernel that evaluates the pair renders the room with and without a BRDF candidate and with
the shadow rays in the pass or in a visibility pass, at 64 x 48 and at 72 x 40 (a partial tile in x and in y);
frames are compared with np.array_equal, G-buffers and reservoirs too, NaN matching NaN (material_cases.same).
"""
import functools

import numpy as np
import pytest

import material_cases as M
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.scenes import LAMBERT, PHONG, Material

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (72, 40))
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
M_AREA = 17          # five batches of three and the peeled batch of two; two chunks of the sorted passes

_KD, _KS = (0.4, 0.4, 0.45), (0.3, 0.3, 0.25)
NAN_PATCH = 11
PATCHES = (
    Material(kd=_KD, ks=_KS, shininess=1.0, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=3.0, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=65.0, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=2.0, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=64.0, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=12.5, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=0.0, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=-3.0, type=PHONG),
    Material(kd=_KD, ks=_KS, shininess=float("inf"), type=PHONG),
    Material(kd=_KD, ks=(0.0, 0.0, 0.0), shininess=16.0, type=PHONG),     # omp = 0
    Material(kd=(0.73, 0.73, 0.73), type=LAMBERT),
    Material(kd=_KD, ks=_KS, shininess=3.0, type=PHONG),                  # NAN_PATCH: zero vertex normals
)

# kernel -> (walks, candidate split, environment read when the renderer is created)
KERNELS = {
    "pixel_lockstep": ("lockstep", "off", {"RESTIR_SORT": "off"}),
    "pixel_lane": ("lane", "off", {"RESTIR_SORT": "off"}),
    "split": ("lockstep", "on", {"RESTIR_SORT": "off"}),
    "sorted": ("lane", "off", {"RESTIR_SORT": "on", "RESTIR_PERSIST_SORTED": "off"}),
    "sorted_persistent": ("lane", "off", {"RESTIR_SORT": "on", "RESTIR_PERSIST_SORTED": "on"}),
}
CONFIGS = [(b, v) for b in (0, 1) for v in (0, 1)]          # (m_brdf, do_visibility_pass)


@functools.lru_cache(maxsize=None)
def patch_room():
    """material_cases.room's shell, boxes and lights with the floor and the back wall in 20 x 20 patches"""
    b = scenes._Builder()
    pm = [b.material(m) for m in PATCHES]
    wall = b.material(Material(kd=(0.7, 0.7, 0.7), type=LAMBERT))
    n, s = 20, 0.1
    for i in range(n):
        for j in range(n):
            k = (i + 5 * j) % len(PATCHES)
            u0, u1, v0, v1 = -1 + s * i, -1 + s * (i + 1), s * j, s * (j + 1)
            b.quad([u0, v0 - 1, 0], [u1, v0 - 1, 0], [u1, v1 - 1, 0], [u0, v1 - 1, 0], pm[k],
                   normal=[0, 0, 0] if k == NAN_PATCH else [0, 0, 1])
            b.quad([u0, 1, 2 * v0], [u1, 1, 2 * v0], [u1, 1, 2 * v1], [u0, 1, 2 * v1], pm[k],
                   normal=[0, 0, 0] if k == NAN_PATCH else [0, -1, 0])
    b.quad([-1, -1, 2], [-1, 1, 2], [1, 1, 2], [1, -1, 2], wall, normal=[0, 0, -1])
    b.quad([-1, -1, 0], [-1, 1, 0], [-1, 1, 2], [-1, -1, 2], wall, normal=[1, 0, 0])
    b.quad([1, 1, 0], [1, -1, 0], [1, -1, 2], [1, 1, 2], wall, normal=[-1, 0, 0])
    b.box([-0.65, 0.0, 0.0], [-0.05, 0.6, 1.2], b.material(PATCHES[4]), rot_z=0.3)
    b.box([0.05, -0.55, 0.0], [0.65, 0.05, 0.6], wall, rot_z=-0.3)
    la, lb = b.material(M.LIGHT_A), b.material(M.LIGHT_B)
    h, z = 0.09, 1.98
    for cx, cy in ((-0.5, -0.4), (0.5, -0.4), (-0.5, 0.5), (0.5, 0.5)):
        b.quad([cx - h, cy - h, z], [cx - h, cy + h, z], [cx + h, cy + h, z], [cx + h, cy - h, z], la, normal=[0, 0, -1])
    b.quad([-h, -h, z], [-h, h, z], [h, h, z], [h, -h, z], lb, normal=[0, 0, -1])
    return b.build(scenes.CORNELL_CAMERA, "patch_room")


def params(m_brdf, vis):
    return P.default_params(m_area=M_AREA, m_brdf=m_brdf, do_visibility_pass=vis)


@functools.lru_cache(maxsize=None)
def oracle(m_brdf, vis, size):
    return M.oracle_restir(patch_room(), params(m_brdf, vis), size, 1)


def _f32(x):
    return np.asarray(x, np.float32)


def _dot(a, b):
    t = a * b
    return (t[..., 0] + t[..., 1]) + t[..., 2]            # glm compute_dot


def _normalize(a):
    return a * (np.float32(1.0) / np.sqrt(_dot(a, a)))[..., None]


@functools.lru_cache(maxsize=None)
def lobe_bases(size):
    """The two bases of the first frame's area candidates, restated in float32 from the oracle's G-buffer for the
    direction to a light's first vertex (make_frame's wr; phong_pdf's and eval_brdf's gmax).  Returns, per pixel:
    whether the pass draws candidates there, the bits of max(0, d) and of max(d, 0), shininess and type."""
    sc = patch_room()
    g = oracle(0, 0, size).gbuffer
    pos, nrm, le = g[..., 0:3], g[..., 3:6], g[..., 12:15]
    cam = _f32(M.camera(sc, 0).eye)
    emitter = int(np.nonzero(sc.emissive_mask())[0][0])
    light = _f32(sc.positions[emitter][0:3])
    with np.errstate(all="ignore"):
        wo = _normalize(pos - cam)
        refl = wo - (nrm * _dot(nrm, wo)[..., None]) * np.float32(2.0)        # glm reflect
        wr = _normalize(refl)
        d = _dot(_normalize(light - pos), wr)
        base_pdf = np.where(np.float32(0.0) < d, d, np.float32(0.0))          # gmax(0, d)
        base_brdf = np.where(d < np.float32(0.0), np.float32(0.0), d)         # gmax(d, 0)
    alive = (g[..., 16] > 0) & ~(le > 0).any(-1)
    return (alive, np.ascontiguousarray(base_pdf).view(np.uint32), np.ascontiguousarray(base_brdf).view(np.uint32),
            g[..., M.SHIN_COL], g[..., M.TYPE_COL])


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_room_reaches_the_own_power_and_mixes_tiles(size):
    """What the comparison relies on, established on the host: candidates whose two bases differ in bits on a lobe of
    odd-integer shininess (the BRDF's own power), every shininess case on screen, and 8 x 8 wave tiles that hold
    Lambert and Phong pixels together."""
    alive, bp, bb, shin, typ = lobe_bases(size)
    phong = alive & (typ == PHONG)
    own = phong & (bp != bb) & (shin == 3.0)
    print(f"[lobe once] {size}: {int(own.sum())} pixels with differing bases (NaN against +0) at shininess 3, "
          f"{int((phong & (bp == bb)).sum())} Phong pixels with one base")
    assert own.sum() >= 8 and (phong & (bp == bb)).sum() >= 200
    for m in PATCHES[:10]:
        s = np.float32(m.shininess)
        assert (phong & (shin == s)).sum() >= 8, f"shininess {m.shininess} covers too few pixels"
    H, W = alive.shape
    mixed = sum(1 for y in range(0, H, 8) for x in range(0, W, 8)
                if (alive & (typ == LAMBERT))[y:y + 8, x:x + 8].any() and phong[y:y + 8, x:x + 8].any()
                and own[y:y + 8, x:x + 8].any())
    assert mixed >= 2, "no wave tile with Lambert, Phong and differing-base pixels together"


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_lobe_once_matches_oracle(kernel, size, monkeypatch):
    traversal, split, env = KERNELS[kernel]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for m_brdf, vis in CONFIGS:
        got = M.gpu_restir(patch_room(), params(m_brdf, vis), size, 1, traversal, split)
        M.assert_same_render(got, oracle(m_brdf, vis, size), f"{kernel} m_brdf={m_brdf} vis={vis}")
