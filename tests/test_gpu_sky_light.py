"""GPU tests of the sky-light path tracer (rs_render_path_sky, restir-embree_amd/csrc/rs_path.h kEstUnbiasedSky) and of
the sky's sampling tables (csrc/rs_sky.h, rs_sky_build.hip): the tables equal the checker's (tests/cpp/sky_oracle.c)
exactly; frames against the checker on the same seeds, ray count included; the closed forms of
tests/closed_form_sky.py directly, never reading the checker; the variance ratio; the contract of rs_render_path; row
sets, two local ranks and the C++ tool's --sky --sky-light frames."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import closed_form_sky as CS
import closed_form_unbiased as CU
import oracle_lib as O
from gpu_harness import assert_close
import sky_oracle as SO
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.mgpu import MultiGpuFrame
from restir_amd.renderer import (GT_PATH_UNBIASED_SKY, RS_E_INVALID, RS_E_UNSUPPORTED, Renderer, RestirError, RowSet,
                                 camera_desc, decode_image)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "restir-embree_amd", "restir_render")


def _with_sky(sc, tex):
    return dataclasses.replace(sc, sky=tex)


# ---------------------------------------------------------------- tables
@pytest.fixture(scope="module")
def table_renderer():
    g = Renderer(16, 16)
    return g, g.load_scene(CS.get_scene("bgquad_n1").scene)


@pytest.mark.parametrize("fmt", CS.TABLE_FORMATS)
@pytest.mark.parametrize("size", CS.TABLE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tables_equal_the_checker(table_renderer, size, fmt):
    """63 / 64 / 65 cross the scan's wave, 257 and 1025 the workgroup's chunk; every texel format"""
    g, gs = table_renderer
    tex = CS.table_sky(*size, fmt)
    gs.set_sky(tex)
    cdf, marg = gs.sky_tables()
    want_cdf, want_marg = SO.sky_tables(O.OracleScene(_with_sky(CS.get_scene("bgquad_n1").scene, tex)))
    assert cdf.shape == want_cdf.shape and want_marg[-1] > 0
    assert np.array_equal(cdf, want_cdf) and np.array_equal(marg, want_marg)


def test_tables_follow_the_sky(table_renderer):
    """the cache is dropped by set_sky; a sky without light and one with hostile texels"""
    g, gs = table_renderer
    seen = []
    for tex in (CS.sun_sky(), CS.black_sky(), CS.hostile_sky(), CS.sun_sky()):
        gs.set_sky(tex)
        cdf, marg = gs.sky_tables()
        again = gs.sky_tables()
        want_cdf, want_marg = SO.sky_tables(O.OracleScene(_with_sky(CS.get_scene("bgquad_n1").scene, tex)))
        assert np.array_equal(cdf, want_cdf) and np.array_equal(marg, want_marg)
        assert np.array_equal(again[0], cdf) and np.array_equal(again[1], marg)
        seen.append(int(marg[-1]))
    assert seen[0] == seen[3] > 0 and seen[1] == 0 and seen[2] not in (0, seen[0])


# ---------------------------------------------------------------- frames against the checker
def _closed_cornell():
    """cornell_box and its camera inside a closed cube of the box's wall material: no ray ever misses, the camera's
    included, but for sky shadow rays that start within tnear of a cube edge -- on the device and in the checker alike.
    Under bright_sky: sun_sky's dim cells put their samples on two columns per cell, some of them directions that lie
    in a coordinate plane to the last bit, and a shadow ray that runs along a wall of the cube two ulp outside it is
    a hit for the device's walk and a miss for the checker's (measured: 2 such rays in 200 000, one pixel each)."""
    sc = scenes.cornell_box(8)
    b = scenes._Builder()
    lo, hi = [-30.0, -30.0, -30.0], [30.0, 30.0, 30.0]
    c = [[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])]
    for f in ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)):
        b.quad(*[c[k] for k in f], 0)
    pos, nrm = np.concatenate(b.pos), np.concatenate(b.nrm)
    return dataclasses.replace(
        sc, positions=np.ascontiguousarray(np.concatenate([sc.positions.reshape(-1, 9), pos.reshape(-1, 9)])),
        normals=np.ascontiguousarray(np.concatenate([sc.normals.reshape(-1, 9), nrm.reshape(-1, 9)])),
        tri_material=np.ascontiguousarray(np.concatenate([sc.tri_material, np.zeros(len(pos.reshape(-1, 9)), sc.tri_material.dtype)])),
        sky=CS.bright_sky(), name="closed_cornell")


FRAME_CASES = {
    # scene, W, H, spp, max_bounces, exact
    "textured": (lambda: scenes.textured_cornell(), 64, 48, 2, 3, False),
    "sun_quad": (lambda: CS.get_scene("sun_quad").scene, CS.W, CS.H, 4, 5, False),
    "closed": (_closed_cornell, 64, 48, 2, 3, True),
}


@pytest.mark.parametrize("which", list(FRAME_CASES))
def test_frames_against_the_checker(which):
    """Two frames, traversal pinned to lockstep and to lane: the two kinds are bit-identical, times.rays is the checker's
    count, and the frame is the checker's within the bound of frames that pass through the device's atan2f / acosf --
    a one-ulp difference there can also move a miss direction into the neighbouring cell.  Without any miss after the
    camera vertex the frame is the checker's bit for bit."""
    fn, W, H, spp, mb, exact = FRAME_CASES[which]
    sc, prm = fn(), P.default_params(use_skybox=1)
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    out, rays = {}, {}
    for mode in ("lockstep", "lane"):
        g = Renderer(W, H)
        g.set_traversal(mode)
        gs = g.load_scene(sc)
        for f in range(2):
            out[mode, f] = g.render_path(gs, sc.camera, prm, f, spp, max_bounces=mb, timed=True, unbiased=True,
                                         sky_light=True).copy()
            rays[mode, f] = int(g.last_times.rays)
            assert g.last_times.primary_rays == W * H
    for f in range(2):
        gpu = out["lane", f]
        assert np.array_equal(out["lockstep", f], gpu)
        ref = SO.render_path_sky(o, os_, sc.camera, prm, f, spp, max_bounces=mb)
        assert np.isfinite(gpu).all() and np.isfinite(ref).all() and ref.max() > 0
        print(f"[sky] {which} frame {f}: rays {rays['lane', f]} (checker {o.rays})")
        assert rays["lane", f] == rays["lockstep", f] == o.rays
        if exact:
            assert np.array_equal(gpu, ref)
        else:
            assert_close(gpu, ref, f"{which} frame {f}", tag="sky")


# ---------------------------------------------------------------- closed forms, never reading the checker
class GpuBackend:
    """closed_form's backend over Renderer.render_path(unbiased=True, sky_light=True)"""

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
        return g.render_path(gs, cf.camera, CS.frame_params(cf.name, seed), 0, n, unbiased=True, sky_light=True,
                             **CS.ESTIMATORS[estimator]).astype(np.float64)


_backend, _refs = GpuBackend(), {}


def _reference(name):
    if name not in _refs:
        cf = CS.get_scene(name)
        _refs[name] = CS.reference(cf, _backend.gbuffer(cf))
    return _refs[name]


def _check(scene, estimator):
    CS.check(scene, estimator, CS.measure(_backend, CS.get_scene(scene), _reference(scene), estimator, frames=CS.SPP))


@pytest.mark.parametrize("estimator", CS.SUN_ESTIMATORS)
def test_sun_sky_closed_form(estimator):
    _check("sun_quad", estimator)


@pytest.mark.parametrize("n", CU.QUAD_EXPONENTS)
def test_uniform_sky_closed_form(n):
    _check(f"skyquad_n{n}", "sky_m1")


@pytest.mark.parametrize("n", CU.QUAD_EXPONENTS)
def test_background_with_gi_off_closed_form(n):
    """bg_color with calc_gi = 0: the furnace value, where rs_render_path_unbiased is black"""
    scene = f"bgquad_n{n}"
    _check(scene, "sky_nogi")
    cf, ref = CS.get_scene(scene), _reference(scene)
    g, gs = _backend._pair(cf)
    old = g.render_path(gs, cf.camera, CS.frame_params(scene, CS.SEEDS[0]), 0, 4, calc_gi=False, unbiased=True)
    assert (old[ref.mask] == 0).all()


def test_variance_ratio():
    """at least half the checker's recorded ratio: the same seeds give nearly the same images, and the half covers the
    few pixels the frame bound lets differ"""
    cf, ref = CS.get_scene("sun_quad"), _reference("sun_quad")
    g, gs = _backend._pair(cf)
    ratio = CS.variance_ratio(
        lambda s: g.render_path(gs, cf.camera, CS.frame_params(cf.name, s), 0, CS.VARIANCE_SPP, calc_gi=False,
                                unbiased=True, sky_light=True).copy(),
        lambda s: g.render_path(gs, cf.camera, CS.frame_params(cf.name, s), 0, CS.VARIANCE_SPP, max_bounces=1,
                                unbiased=True).copy(), ref.mask)
    print(f"[sky] variance ratio {ratio:.2f} (the checker's {CS.VARIANCE_RATIO})")
    assert ratio >= 0.5 * CS.VARIANCE_RATIO


# ---------------------------------------------------------------- contract
def test_direct_entry_and_untouched_history():
    sc = _with_sky(scenes.cornell_many_lights(1024), CS.sun_sky())
    W, H = 96, 54
    prm_t, prm = P.c3_params(m_area=8), P.c3_params(m_area=8, use_skybox=1)
    ref, g = Renderer(W, H), Renderer(W, H)
    rs, gs = ref.load_scene(sc), g.load_scene(sc)
    a0 = ref.produce_restir(rs, sc.camera, prm_t, 0).copy()
    a1 = ref.produce_restir(rs, sc.camera, prm_t, 1).copy()
    b0 = g.produce_restir(gs, sc.camera, prm_t, 0).copy()
    p = g.render_path(gs, sc.camera, prm, 7, 3, calc_gi=False, unbiased=True, sky_light=True).copy()
    d = g.render_direct_mis(gs, sc.camera, prm, 7, 3, unbiased=True, sky_light=True).copy()
    b1 = g.produce_restir(gs, sc.camera, prm_t, 1).copy()
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    assert np.isfinite(p).all() and np.array_equal(p, d)
    assert not np.array_equal(p, g.render_path(gs, sc.camera, prm, 7, 3, calc_gi=False, unbiased=True))
    with pytest.raises(ValueError):
        g.render_path(gs, sc.camera, prm, 7, 3, sky_light=True)
    with pytest.raises(ValueError):
        g.render_direct_mis(gs, sc.camera, prm, 7, 3, sky_light=True)


def _code(fn):
    """the RS_E_* code of the error fn raises.  Only the message is kept: an exception info bound in this frame would
    tie fn's renderer and scene into a reference cycle, and the cycle collector finalises a renderer and its scene in
    any order."""
    try:
        fn()
    except RestirError as e:
        msg = str(e)
    else:
        pytest.fail("no RestirError")
    return int(msg.split("librestir_amd error ")[1].split(":")[0])


def test_invalid_arguments_raise():
    sc = _with_sky(scenes.cornell_box(8), CS.sun_sky())
    W, H = 16, 16
    g, other = Renderer(W, H), Renderer(W, H)
    gs, os_ = g.load_scene(sc), other.load_scene(sc)
    prm = P.default_params(use_skybox=1)
    kw = dict(unbiased=True, sky_light=True)
    g.render_path(gs, sc.camera, prm, 0, 1, **kw)                                          # the valid call
    for bad in (dict(spp=0), dict(spp=65537), dict(max_bounces=-1), dict(max_bounces=16)):
        assert _code(lambda: g.render_path(gs, sc.camera, prm, 0, **bad, **kw)) == RS_E_INVALID
    assert _code(lambda: g.render_path(os_, sc.camera, prm, 0, 1, **kw)) == RS_E_INVALID   # a scene of another context
    cam, pp = camera_desc(sc.camera), P.PathParams()
    args = [g.h, gs.h, ctypes.byref(cam), ctypes.byref(prm), ctypes.byref(pp)]
    for i in range(5):                                                                     # each null argument
        a = list(args)
        a[i] = None
        assert _code(lambda: g._check(g.lib.rs_render_path_sky(*a, 0, 1, None, None))) == RS_E_INVALID
    g.tile_begin(gs, sc.camera, prm, 0, 0, H, 0, 0)
    assert _code(lambda: g.render_path(gs, sc.camera, prm, 0, 1, **kw)) == RS_E_INVALID    # a tile frame in flight
    g.tile_temporal()
    g.tile_finish()
    g.render_path(gs, sc.camera, prm, 0, 1, **kw)
    gs.set_sky(None)
    assert _code(lambda: g.render_path(gs, sc.camera, prm, 0, 1, **kw)) == RS_E_UNSUPPORTED     # use_skybox without a sky
    g.render_path(gs, sc.camera, P.default_params(), 0, 1, **kw)                           # bg_color needs none
    gs.set_sky(scenes.Texture(np.full((1, 32769, 1), 200, np.uint8)))
    assert _code(lambda: g.render_path(gs, sc.camera, prm, 0, 1, **kw)) == RS_E_UNSUPPORTED     # wider than the tables take
    assert _code(gs.sky_tables) == RS_E_UNSUPPORTED
    g.render_path(gs, sc.camera, prm, 0, 1, unbiased=True)                                 # from the new entry only
    gs.set_sky(scenes.Texture(np.full((1, 32768, 1), 200, np.uint8)))
    g.render_path(gs, sc.camera, prm, 0, 1, **kw)


def test_black_sky_equals_the_unbiased_entry():
    """a sky without light: no sky sample, no extra draw -- with max_bounces = 0 and calc_gi = 0 the two entries are
    defined the same"""
    sc = _with_sky(scenes.cornell_box(8), CS.black_sky())
    W, H = 64, 48
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    prm = P.default_params(use_skybox=1)
    a = g.render_path(gs, sc.camera, prm, 0, 4, max_bounces=0, calc_gi=False, unbiased=True, sky_light=True, timed=True).copy()
    rays = int(g.last_times.rays)
    b = g.render_path(gs, sc.camera, prm, 0, 4, max_bounces=0, calc_gi=False, unbiased=True, timed=True).copy()
    assert np.isfinite(a).all() and a.max() > 0 and np.array_equal(a, b) and rays == int(g.last_times.rays)


# ---------------------------------------------------------------- row sets, ranks, the tool
def test_row_sets_assemble_the_full_frame():
    sc, prm, W, H = scenes.textured_cornell(), P.default_params(use_skybox=1), 64, 40
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    kw = dict(max_bounces=3, unbiased=True, sky_light=True)
    full = g.render_path(gs, sc.camera, prm, 1, 2, timed=True, **kw).copy()
    full_rays = int(g.last_times.rays)
    for stride in (1, 2, 3):
        img, rays = np.full_like(full, np.nan), 0
        for phase in range(stride):
            part = g.render_path(gs, sc.camera, prm, 1, 2, rows=(16, stride, phase), timed=True, **kw)
            own = (np.arange(H) // 16) % stride == phase
            img[own] = part[own]
            rays += int(g.last_times.rays)
        assert np.array_equal(img, full) and rays == full_rays, stride
    cam, pp, rs = camera_desc(sc.camera), P.PathParams(), RowSet(16, 1, 0)
    assert g.lib.rs_render_ground_truth_rows(g.h, gs.h, ctypes.byref(cam), ctypes.byref(prm), GT_PATH_UNBIASED_SKY,
                                             ctypes.byref(pp), 1, 1, ctypes.byref(rs), None, None) == 0
    for unknown in (3, GT_PATH_UNBIASED_SKY + 1):            # 3 stays no estimator (tests/test_gpu_gt_rows.py)
        assert g.lib.rs_render_ground_truth_rows(g.h, gs.h, ctypes.byref(cam), ctypes.byref(prm), unknown,
                                                 ctypes.byref(pp), 1, 1, ctypes.byref(rs), None, None) == RS_E_INVALID


def test_two_local_ranks_gather_one_contexts_frame():
    sc, prm, W, H = scenes.textured_cornell(), P.default_params(use_skybox=1), 72, 40
    one = Renderer(W, H)
    ones = one.load_scene(sc)
    kw = dict(max_bounces=3, unbiased=True, sky_light=True)
    want = one.render_path(ones, sc.camera, prm, 1, 2, **kw).copy()
    rs = [Renderer(W, H) for _ in range(2)]
    ss = [r.load_scene(sc) for r in rs]
    m = MultiGpuFrame(rs)
    got = m.render_path(ss, sc.camera, prm, 1, 2, copy_out=True, **kw)
    assert np.array_equal(got, want) and want.max() > 0
    direct = m.render_direct_mis(ss, sc.camera, prm, 1, 2, unbiased=True, sky_light=True, copy_out=True)
    assert np.array_equal(direct, one.render_direct_mis(ones, sc.camera, prm, 1, 2, unbiased=True, sky_light=True))
    with pytest.raises(ValueError):
        m.render_path(ss, sc.camera, prm, 1, 2, sky_light=True)
    m.close()


def _write_pfm(path, img):
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(img[::-1], "<f4").tobytes())


def test_cpp_tool_sky_light_frames(tmp_path):
    """restir_render --sky f.pfm --path 4 --unbiased --sky-light (restir::Renderer::LoadSky, skyLight): the PFM of the
    last of two frames is the binding's second frame bit for bit; --sky-light without --unbiased is refused."""
    assert os.path.exists(TOOL), "build restir-embree_amd (make) first"
    sc = scenes.cornell_box(8)
    obj, out, sky = tmp_path / "c1.obj", tmp_path / "f.pfm", tmp_path / "sky.pfm"
    scenes.write_obj(sc, str(obj))
    _write_pfm(sky, np.asarray(CS.sun_sky().data))
    c = sc.camera
    W, H = 64, 48
    base = [TOOL, "--obj", str(obj), "--w", str(W), "--h", str(H), "--eye", *map(str, c.eye), "--at", *map(str, c.at),
            "--fov", str(c.fov_y), "--bounces", "3", "--frames", "2", "--out", str(out), "--sky", str(sky), "--path", "4"]
    p = subprocess.run([*base, "--unbiased", "--sky-light"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    img = decode_image(out)
    g = Renderer(W, H)
    gs = g.load_scene(str(obj))
    gs.load_sky(str(sky))
    assert np.array_equal(gs.sky_tables()[0], SO.sky_tables(O.OracleScene(_with_sky(sc, CS.sun_sky())))[0])
    prm = P.default_params(use_skybox=1)
    want = g.render_path(gs, c, prm, 1, 4, max_bounces=3, unbiased=True, sky_light=True).copy()
    assert img.shape == want.shape and want.max() > 0
    assert np.array_equal(img, want)
    assert not np.array_equal(img, g.render_path(gs, c, prm, 1, 4, max_bounces=3, unbiased=True))
    p = subprocess.run([*base, "--sky-light"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--sky-light" in p.stderr
