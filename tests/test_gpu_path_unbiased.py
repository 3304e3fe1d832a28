"""GPU tests of the unbiased path tracer (rs_render_path_unbiased, restir-embree_amd/csrc/rs_path.h): bit for bit
against its checker (tests/cpp/path_oracle.c or_render_path_unbiased, pinned to the light by tests/test_path_unbiased_oracle.py)
on the same seeds, ray count included; against the closed forms directly, never reading the checker; ReSTIR against
this new truth on the Phong furnace; and the contract of rs_render_path -- errors, untouched ReSTIR history, the C++
tool's --path --unbiased frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import closed_form as CF
import closed_form_unbiased as CU
import oracle_lib as O
from gpu_harness import assert_close
import path_oracle as PO
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.renderer import Renderer, RestirError, camera_desc, decode_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "restir-embree_amd", "restir_render")


def _quad_prm():
    return CU.frame_params("quad_n8", 123)


# scene, params, W, H, spp, max_bounces, render_path keywords per run.  The shapes of tests/test_gpu_path.py.
CASES = {
    "c1": (lambda: scenes.cornell_box(8), P.default_params, 64, 48, 4, 5, ({},)),
    # 36 rows leave a partial tile row; Phong vertices
    "phong": (lambda: scenes.sponza_like(target_tris=30_000, n_lamps=128), P.c3_params, 64, 36, 2, 5, ({},)),
    # roulette live past bounce 5; lanes outside the 50x38 image sit in the refill loop from the start
    "rr": (lambda: scenes.cornell_box(8), P.default_params, 50, 38, 3, 8,
           (dict(russian_roulette=True), dict(russian_roulette=False))),
    "spp1": (lambda: scenes.cornell_box(8), P.default_params, 64, 48, 1, 5, ({},)),      # nothing to refill from
    "m0": (lambda: scenes.cornell_box(8), P.default_params, 64, 48, 2, 0, ({},)),        # the BRDF ray sees emitters only
    "m15": (lambda: scenes.cornell_box(8), P.default_params, 50, 38, 2, 15, ({},)),      # 128 KiB of records
    "gi0": (lambda: scenes.cornell_box(8), P.default_params, 64, 48, 2, 5, (dict(calc_gi=False),)),
    "di0": (lambda: scenes.cornell_box(8), P.default_params, 64, 48, 2, 5, (dict(calc_di=False),)),
    # no emitters: the light part's uniform early-out; everything arrives from the background
    "quad": (lambda: CU.quad_scene(8).scene, _quad_prm, CU.QUAD_W, CU.QUAD_H, 4, 5, ({},)),
}


@pytest.mark.parametrize("which", list(CASES))
def test_unbiased_path_equals_checker(which):
    """Two frames per case, traversal pinned to lockstep and to lane: the two kinds and or_render_path_unbiased are
    equal bit for bit, and times.rays is the checker's count."""
    fn, prm_fn, W, H, spp, mb, runs = CASES[which]
    sc, prm = fn(), prm_fn()
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    out, rays = {}, {}
    for mode in ("lockstep", "lane"):
        g = Renderer(W, H)
        g.set_traversal(mode)
        gs = g.load_scene(sc)
        for i, kw in enumerate(runs):
            for f in range(2):
                out[mode, i, f] = g.render_path(gs, sc.camera, prm, f, spp, max_bounces=mb, timed=True, unbiased=True,
                                                **kw).copy()
                rays[mode, i, f] = int(g.last_times.rays)
                assert g.last_times.primary_rays == W * H
    for i, kw in enumerate(runs):
        for f in range(2):
            assert np.array_equal(out["lockstep", i, f], out["lane", i, f])
            ref = PO.render_path(o, os_, sc.camera, prm, f, spp, max_bounces=mb, unbiased=True, **kw)
            n_diff = int((out["lane", i, f] != ref).any(axis=-1).sum())
            print(f"[unbiased] {which} {kw} frame {f}: {n_diff} of {W * H} pixels not bit-identical, rays "
                  f"{rays['lane', i, f]} (checker {o.rays})")
            assert np.isfinite(ref).all() and ref.max() > 0 and len(np.unique(ref)) > 2
            assert np.array_equal(out["lane", i, f], ref)
            assert rays["lane", i, f] == rays["lockstep", i, f] == o.rays
    if len(runs) > 1:
        differ = (out["lane", 0, 0] != out["lane", 1, 0]).any(axis=-1).mean()
        print(f"[unbiased] {which}: roulette changes {100 * differ:.1f} % of the pixels")
        assert differ > 0


def test_sky_and_maps_match_checker():
    """textured_cornell with the sky on: maps at the bounce vertices and on emitters, the sky on misses.  The sky
    lookup's atan2f / acosf are the device library's, so this case is held to tests/test_gpu_path.py's frame bound
    for the same scene and not to equality."""
    sc, prm, W, H = scenes.textured_cornell(), P.default_params(use_skybox=1), 64, 48
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    for f in range(2):
        gpu = g.render_path(gs, sc.camera, prm, f, 2, max_bounces=3, unbiased=True).copy()
        ref = PO.render_path(o, os_, sc.camera, prm, f, 2, max_bounces=3, unbiased=True)
        assert_close(gpu, ref, f"textured frame {f}", tag="unbiased")


# ---------------------------------------------------------------- closed forms, never reading the checker
class GpuBackend:
    """closed_form's backend over Renderer: the unbiased estimators of closed_form_unbiased and, for the comparison
    with ReSTIR, closed_form's own ReSTIR estimators (frames accumulated on the device)"""

    def __init__(self):
        self._scenes = {}

    def _pair(self, cf):
        if cf.name not in self._scenes:
            g = Renderer(cf.width, cf.height)
            self._scenes[cf.name] = (g, g.load_scene(cf.scene))
        return self._scenes[cf.name]

    def gbuffer(self, cf):
        g, gs = self._pair(cf)
        g.reset_history()
        g.produce_restir(gs, cf.camera, P.default_params(), 0)
        return g.gbuffer()

    def mean_image(self, cf, estimator, seed, n):
        g, gs = self._pair(cf)
        if estimator in CU.ESTIMATORS:
            return g.render_path(gs, cf.camera, CU.frame_params(cf.name, seed), 0, n, unbiased=True,
                                 **CU.ESTIMATORS[estimator]).astype(np.float64)
        kind, kw = CF.ESTIMATORS[estimator]
        assert kind == "restir"
        prm = P.default_params(seed=seed, **kw)
        g.reset_history()
        g.post_reset()
        for f in range(n):
            g.produce_restir(gs, cf.camera, prm, f, copy_out=False, timed=False)
            g.post_frame(accumulate=True, tonemap=False, gamma_correct=False, stats=False)
        return g.display_rgba()[..., :3].astype(np.float64)


_backend, _refs, _results = GpuBackend(), {}, {}


def _reference(name):
    if name not in _refs:
        cf = CU.get_scene(name)
        g = _backend.gbuffer(cf)
        _refs[name] = CU.quad_reference(cf, g) if name.startswith("quad_n") else CF.reference(cf, g)
    return _refs[name]


def _measure(scene, estimator, frames):
    if (scene, estimator) not in _results:
        _results[scene, estimator] = CU.measure(_backend, CU.get_scene(scene), _reference(scene), estimator, frames=frames)
    return _results[scene, estimator]


@pytest.mark.parametrize("scene", CF.FURNACE_SCENES)
def test_furnace_closed_form(scene):
    """render_direct_mis(unbiased=True) routes to the same launch; every strip (kd + ks) Le, no quirk rows"""
    CU.check(scene, "unbiased", _measure(scene, "unbiased", CU.samples_for(scene)))
    cf = CU.get_scene(scene)
    g, gs = _backend._pair(cf)
    a = g.render_direct_mis(gs, cf.camera, CU.frame_params(scene, CU.SEEDS[0]), 0, 8, unbiased=True).copy()
    assert np.array_equal(a, _backend.mean_image(cf, "unbiased", CU.SEEDS[0], 8)) and a.max() > 0


@pytest.mark.parametrize("m", CU.QUAD_BOUNCES)
@pytest.mark.parametrize("n", CU.QUAD_EXPONENTS)
def test_quad_closed_form(n, m):
    scene, est = f"quad_n{n}", f"unbiased_m{m}"
    CU.check(scene, est, _measure(scene, est, CU.QUAD_SPP))


@pytest.mark.parametrize("m", [1, 6, 12])
def test_integrating_sphere_closed_form(m):
    sc, f = PO.integrating_sphere()
    g = Renderer(PO.SPHERE_W, PO.SPHERE_H)
    gs = g.load_scene(sc)
    prm = P.default_params(use_skybox=0)
    got = PO.sphere_measure(lambda fr: g.render_path(gs, sc.camera, prm, fr, 64, max_bounces=m, unbiased=True).copy())
    want = PO.sphere_expected(f, m)
    print(f"[unbiased] sphere m={m}: measured {got:.6f} expected {want:.6f} ({100 * (got / want - 1):+.3f} %)")
    assert abs(got / want - 1.0) <= 0.01


def test_restir_agrees_with_the_unbiased_truth():
    """furnace_steep: ReSTIR (pairwise weights, temporal reuse, 256 frames per seed) and the unbiased 512-spp image
    agree per strip within the sum of their two recorded 4 SE bounds -- the kd-and-ks strips included, where the
    reference's estimators sit at 0.59 to 0.98 of ReSTIR."""
    scene = "furnace_steep"
    truth = _measure(scene, "unbiased", CU.samples_for(scene))
    restir = CF.measure(_backend, CU.get_scene(scene), _reference(scene), "pairwise_T1")
    failures = []
    for strip in CF.STRIPS:
        a, b = float(np.mean(restir[strip]["ratios"])), float(np.mean(truth[strip]["ratios"]))
        bound = CF.bounds(scene, "pairwise_T1", strip)[1] + CU.bounds(scene, "unbiased", strip)[1]
        print(f"[unbiased] {scene}/{strip}: ReSTIR {a:.4f} unbiased {b:.4f} difference {a - b:+.4f} (bound {bound:.4f})")
        if not abs(a - b) <= bound:
            failures.append(strip)
    assert not failures, failures


# ---------------------------------------------------------------- contract
def test_leaves_restir_history_untouched():
    sc = scenes.cornell_many_lights(1024)
    W, H = 96, 54
    prm_t = P.c3_params(m_area=8)
    ref, g = Renderer(W, H), Renderer(W, H)
    rs, gs = ref.load_scene(sc), g.load_scene(sc)
    a0 = ref.produce_restir(rs, sc.camera, prm_t, 0).copy()
    a1 = ref.produce_restir(rs, sc.camera, prm_t, 1).copy()
    b0 = g.produce_restir(gs, sc.camera, prm_t, 0).copy()
    p = g.render_path(gs, sc.camera, prm_t, 7, 3, unbiased=True).copy()
    b1 = g.produce_restir(gs, sc.camera, prm_t, 1).copy()
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    assert np.isfinite(p).all() and not np.array_equal(p, b0)
    assert not np.array_equal(p, g.render_path(gs, sc.camera, prm_t, 7, 3))          # and it is another estimator


def test_invalid_arguments_raise():
    sc = scenes.cornell_box(8)
    W, H = 16, 16
    g, other = Renderer(W, H), Renderer(W, H)
    gs, os_ = g.load_scene(sc), other.load_scene(sc)
    prm = P.default_params()
    g.render_path(gs, sc.camera, prm, 0, 1, unbiased=True)                                 # the valid call
    for kw in (dict(spp=0), dict(spp=65537), dict(max_bounces=-1), dict(max_bounces=16)):
        with pytest.raises(RestirError):
            g.render_path(gs, sc.camera, prm, 0, unbiased=True, **kw)
    with pytest.raises(RestirError):
        g.render_path(os_, sc.camera, prm, 0, 1, unbiased=True)                            # a scene of another context
    with pytest.raises(RestirError):
        g.render_path(gs, sc.camera, P.default_params(use_skybox=1), 0, 1, unbiased=True)  # no sky: RS_E_UNSUPPORTED
    cam, pp = camera_desc(sc.camera), P.PathParams()
    args = [g.h, gs.h, ctypes.byref(cam), ctypes.byref(prm), ctypes.byref(pp)]
    for i in range(5):                                                                     # each null argument
        a = list(args)
        a[i] = None
        with pytest.raises(RestirError):
            g._check(g.lib.rs_render_path_unbiased(*a, 0, 1, None, None))
    g.tile_begin(gs, sc.camera, prm, 0, 0, H, 0, 0)
    with pytest.raises(RestirError):
        g.render_path(gs, sc.camera, prm, 0, 1, unbiased=True)                             # a tile frame in flight
    g.tile_temporal()
    g.tile_finish()
    g.render_path(gs, sc.camera, prm, 0, 1, unbiased=True)


def test_cpp_tool_unbiased_frames(tmp_path):
    """restir_render --path 4 --unbiased (restir::Renderer::unbiasedEstimator): the PFM of the last of two frames is
    the binding's second frame bit for bit; --unbiased without --path is refused."""
    assert os.path.exists(TOOL), "build restir-embree_amd (make) first"
    sc = scenes.cornell_box(8)
    obj, out = tmp_path / "c1.obj", tmp_path / "f.pfm"
    scenes.write_obj(sc, str(obj))
    c = sc.camera
    W, H = 64, 48
    base = [TOOL, "--obj", str(obj), "--w", str(W), "--h", str(H), "--eye", *map(str, c.eye), "--at", *map(str, c.at),
            "--fov", str(c.fov_y), "--bounces", "3", "--frames", "2", "--out", str(out)]
    p = subprocess.run([*base, "--path", "4", "--unbiased"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("unbiased path tracer 4 spp, 3 bounces") == 2
    img = decode_image(out)
    g = Renderer(W, H)
    gs = g.load_scene(str(obj))
    want = g.render_path(gs, c, P.default_params(), 1, 4, max_bounces=3, unbiased=True).copy()
    assert img.shape == want.shape and want.max() > 0
    assert np.array_equal(img, want)
    assert not np.array_equal(img, g.render_path(gs, c, P.default_params(), 1, 4, max_bounces=3))
    p = subprocess.run([*base, "--unbiased"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--unbiased" in p.stderr
