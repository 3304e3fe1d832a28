"""GPU tests of the NEE path tracer (rs_render_path, restir-embree_amd/csrc/rs_path.h) against its checker
(tests/cpp/path_oracle.c or_render_path, pinned by tests/test_path_oracle.py) on the same seeds, and of its
contract: GI off is rs_render_direct_mis bit for bit, the ReSTIR history is untouched, the integrating sphere's
closed form, the ray count, the error cases, and the C++ tool's --path frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from gpu_harness import assert_close
import path_oracle as PO
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.renderer import Renderer, RestirError, camera_desc, decode_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "restir-embree_amd", "restir_render")

# scene, params, W, H, spp, max_bounces, russian_roulette settings
CASES = {
    "c1": (lambda: scenes.cornell_box(8), lambda: P.default_params(), 64, 48, 4, 5, (True,)),
    # 36 rows leave a partial tile row; Phong vertices
    "phong": (lambda: scenes.sponza_like(target_tris=30_000, n_lamps=128), lambda: P.c3_params(), 64, 36, 2, 5, (True,)),
    # roulette live past bounce 5; lanes outside the 50x38 image sit in the refill loop from the start
    "rr": (lambda: scenes.cornell_box(8), lambda: P.default_params(), 50, 38, 3, 8, (True, False)),
    # maps at bounce vertices, sky on misses
    "textured": (lambda: scenes.textured_cornell(), lambda: P.default_params(use_skybox=1), 64, 48, 2, 3, (True,)),
}


@pytest.mark.parametrize("which", list(CASES))
def test_path_matches_oracle(which):
    """Two frames per case, traversal pinned to lockstep and to lane: the two kinds are equal bit for bit and
    the frame is within the project's frame bound of or_render_path."""
    fn, prm_fn, W, H, spp, mb, rrs = CASES[which]
    sc, prm = fn(), prm_fn()
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    out = {}
    for mode in ("lockstep", "lane"):
        g = Renderer(W, H)
        g.set_traversal(mode)
        gs = g.load_scene(sc)
        for rr in rrs:
            out[mode, rr] = [g.render_path(gs, sc.camera, prm, f, spp, max_bounces=mb, russian_roulette=rr,
                                           timed=True).copy() for f in range(2)]
            assert g.last_times.rays >= W * H
    for rr in rrs:
        for f in range(2):
            assert np.array_equal(out["lockstep", rr][f], out["lane", rr][f])
            ref = PO.render_path(o, os_, sc.camera, prm, f, spp, max_bounces=mb, russian_roulette=rr)
            assert_close(out["lane", rr][f], ref, f"{which} rr={int(rr)} frame {f}", tag="path")
    if len(rrs) > 1:
        differ = (out["lane", True][0] != out["lane", False][0]).any(axis=-1).mean()
        print(f"[path] {which}: roulette changes {100 * differ:.1f} % of the pixels")
        assert differ > 0


@pytest.mark.parametrize("which", ["c1", "phong"])
def test_gi_off_equals_direct_mis(which):
    fn, prm_fn, W, H, spp, _, _ = CASES[which]
    sc, prm = fn(), prm_fn()
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    for f in range(2):
        want = g.render_direct_mis(gs, sc.camera, prm, f, spp).copy()
        for mb in (0, 5, 15):                   # 15: the 128 KiB record array
            assert np.array_equal(g.render_path(gs, sc.camera, prm, f, spp, max_bounces=mb, calc_gi=False), want), (f, mb)
    assert want.max() > 0


@pytest.mark.parametrize("m", [0, 1, 3])
def test_integrating_sphere_closed_form(m):
    """tests/test_path_oracle.py's scene and bound on the GPU: kd Le f sum_{j<=m} (kd (1 - f))^j within 1 %."""
    sc, f = PO.integrating_sphere()
    g = Renderer(PO.SPHERE_W, PO.SPHERE_H)
    gs = g.load_scene(sc)
    prm = P.default_params(use_skybox=0)
    got = PO.sphere_measure(lambda fr: g.render_path(gs, sc.camera, prm, fr, 64, max_bounces=m).copy())
    want = PO.sphere_expected(f, m)
    print(f"[path] sphere m={m}: measured {got:.6f} expected {want:.6f} ({100 * (got / want - 1):+.3f} %)")
    assert abs(got / want - 1.0) <= 0.01


def test_path_leaves_restir_history_untouched():
    """A path launch between ReSTIR frames 0 and 1 (temporal on) leaves both equal to a run without it."""
    sc = scenes.cornell_many_lights(1024)
    W, H = 96, 54
    prm_t = P.c3_params(m_area=8)
    ref, g = Renderer(W, H), Renderer(W, H)
    rs, gs = ref.load_scene(sc), g.load_scene(sc)
    a0 = ref.produce_restir(rs, sc.camera, prm_t, 0).copy()
    a1 = ref.produce_restir(rs, sc.camera, prm_t, 1).copy()
    b0 = g.produce_restir(gs, sc.camera, prm_t, 0).copy()
    p = g.render_path(gs, sc.camera, prm_t, 7, 3).copy()
    b1 = g.produce_restir(gs, sc.camera, prm_t, 1).copy()
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    assert np.isfinite(p).all() and not np.array_equal(p, b0)


def test_ray_count():
    sc = scenes.cornell_box(8)
    W, H = 64, 48
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    rays = {}
    for gi in (False, True):
        g.render_path(gs, sc.camera, P.default_params(), 0, 2, calc_gi=gi, timed=True)
        rays[gi] = int(g.last_times.rays)
        assert g.last_times.primary_rays == W * H and g.last_times.total_ms > 0
    assert rays[False] >= W * H and rays[True] > rays[False]


def test_invalid_arguments_raise():
    sc = scenes.cornell_box(8)
    W, H = 16, 16
    g, other = Renderer(W, H), Renderer(W, H)
    gs, os_ = g.load_scene(sc), other.load_scene(sc)
    prm = P.default_params()
    g.render_path(gs, sc.camera, prm, 0, 1)                                 # the valid call
    for kw in (dict(spp=0), dict(spp=65537), dict(max_bounces=-1), dict(max_bounces=16)):
        with pytest.raises(RestirError):
            g.render_path(gs, sc.camera, prm, 0, **kw)
    with pytest.raises(RestirError):
        g.render_path(os_, sc.camera, prm, 0, 1)                             # a scene of another context
    with pytest.raises(RestirError):
        g.render_path(gs, sc.camera, P.default_params(use_skybox=1), 0, 1)   # no sky: RS_E_UNSUPPORTED
    cam, pp = camera_desc(sc.camera), P.PathParams()
    args = [g.h, gs.h, ctypes.byref(cam), ctypes.byref(prm), ctypes.byref(pp)]
    for i in range(5):                                                       # each null argument
        a = list(args)
        a[i] = None
        with pytest.raises(RestirError):
            g._check(g.lib.rs_render_path(*a, 0, 1, None, None))
    g.tile_begin(gs, sc.camera, prm, 0, 0, H, 0, 0)
    with pytest.raises(RestirError):
        g.render_path(gs, sc.camera, prm, 0, 1)                              # a tile frame in flight
    g.tile_temporal()
    g.tile_finish()
    g.render_path(gs, sc.camera, prm, 0, 1)


def test_cpp_tool_path_frames(tmp_path):
    """restir_render --path (restir::Renderer::produceStandard): the PFM of the last of two frames equals the
    Python binding's second frame for the same scene file, camera and parameters bit for bit."""
    assert os.path.exists(TOOL), "build restir-embree_amd (make) first"
    sc = scenes.cornell_box(8)
    obj, out = tmp_path / "c1.obj", tmp_path / "f.pfm"
    scenes.write_obj(sc, str(obj))
    c = sc.camera
    W, H = 64, 48
    p = subprocess.run([TOOL, "--obj", str(obj), "--w", str(W), "--h", str(H), "--eye", *map(str, c.eye), "--at",
                        *map(str, c.at), "--fov", str(c.fov_y), "--path", "2", "--bounces", "3", "--frames", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("path tracer 2 spp, 3 bounces") == 2
    img = decode_image(out)
    g = Renderer(W, H)
    gs = g.load_scene(str(obj))
    want = g.render_path(gs, c, P.default_params(), 1, 2, max_bounces=3)
    assert img.shape == want.shape and want.max() > 0
    assert np.array_equal(img, want)
