"""CPU tests: the checker of the unbiased path tracer (tests/cpp/path_oracle.c or_render_path_unbiased, which
tests/test_gpu_path_unbiased.py holds rs_render_path_unbiased against bit for bit) against lighting known in closed
form: the Phong furnaces and the occluder scenes of tests/closed_form.py with no quirk rows, a quad under a uniform
background (the continuation sample), and the integrating sphere at every bounce limit, roulette included.  Bounds:
closed_form_unbiased.py's docstring; the recorded figures: DESIGN.md section 5."""
import numpy as np
import pytest

import closed_form as CF
import closed_form_unbiased as CU
import oracle_lib as O
import path_oracle as PO
from restir_amd import params as P
from restir_amd import scenes


class OracleBackend:
    """closed_form's backend over the unbiased checker"""

    def __init__(self):
        self._scenes = {}

    def _pair(self, cf):
        if cf.name not in self._scenes:
            self._scenes[cf.name] = (O.OracleRenderer(cf.width, cf.height), O.OracleScene(cf.scene))
        return self._scenes[cf.name]

    def gbuffer(self, cf):
        o, os_ = self._pair(cf)
        o.reset_history()
        o.render(os_, cf.camera, P.default_params(), 0)
        return o.gbuffer()

    def mean_image(self, cf, estimator, seed, n):
        o, os_ = self._pair(cf)
        return PO.render_path(o, os_, cf.camera, CU.frame_params(cf.name, seed), 0, n, unbiased=True,
                              **CU.ESTIMATORS[estimator]).astype(np.float64)


@pytest.fixture(scope="module")
def backend():
    return OracleBackend()


_refs = {}


def reference(backend, name):
    if name not in _refs:
        cf = CU.get_scene(name)
        g = backend.gbuffer(cf)
        _refs[name] = CU.quad_reference(cf, g) if name.startswith("quad_n") else CF.reference(cf, g)
    return _refs[name]


@pytest.mark.parametrize("scene", CU.DIRECT_SCENES)
def test_direct_light_against_closed_form(backend, scene):
    """GI off: every furnace strip is (kd + ks) Le within its bound -- the kd-and-ks strips and the DIELECTRIC strip
    included, which the reference's estimators leave at 0.59 to 0.98 -- and `open` / `blocked` are the polygon formula
    and the quadrature, umbra dark."""
    cf, ref = CU.get_scene(scene), reference(backend, scene)
    CU.check(scene, "unbiased", CU.measure(backend, cf, ref, "unbiased", frames=CU.samples_for(scene)))


@pytest.mark.parametrize("m", CU.QUAD_BOUNCES)
@pytest.mark.parametrize("n", CU.QUAD_EXPONENTS)
def test_quad_under_uniform_background(backend, n, m):
    """GI on: every pixel on the quad is (kd + ks) bg, all of it brought by the continuation sample.  The reference's
    estimator on the same input is darker than 0.85 at n = 1 and n = 8 (measured 0.613 and 0.784): the failure this
    estimator removes."""
    scene, est = f"quad_n{n}", f"unbiased_m{m}"
    cf, ref = CU.get_scene(scene), reference(backend, scene)
    assert ref.mask.sum() >= 150
    CU.check(scene, est, CU.measure(backend, cf, ref, est, frames=CU.QUAD_SPP))
    if n in (1, 8):
        o, os_ = backend._pair(cf)
        img = PO.render_path(o, os_, cf.camera, CU.frame_params(scene, CU.SEEDS[0]), 0, CU.QUAD_SPP, max_bounces=m)
        ratio = float(img.astype(np.float64).sum(-1)[ref.mask].sum() / ref.image[ref.mask].sum())
        print(f"[closed-form] {scene}: the reference's estimator at m={m}: ratio {ratio:.4f}")
        assert ratio < 0.85


@pytest.fixture(scope="module")
def sphere():
    sc, f = PO.integrating_sphere()
    return sc, f, O.OracleRenderer(PO.SPHERE_W, PO.SPHERE_H), O.OracleScene(sc)


_sphere_got = {}


def _sphere(sphere, m, unbiased=True):
    sc, f, o, os_ = sphere
    if (unbiased, m) not in _sphere_got:
        prm = P.default_params(use_skybox=0)
        _sphere_got[unbiased, m] = PO.sphere_measure(
            lambda fr: PO.render_path(o, os_, sc.camera, prm, fr, 64, max_bounces=m, unbiased=unbiased))
    return _sphere_got[unbiased, m]


@pytest.mark.parametrize("m", [0, 1, 3, 6, 12])
def test_integrating_sphere_closed_form(sphere, m):
    """kd Le f sum_{j<=m} (kd (1 - f))^j within tests/test_path_oracle.py's 1 %, roulette on: live at m = 6 and 12,
    where it now divides the direct part of the vertices past bounce 5 too."""
    got, want = _sphere(sphere, m), PO.sphere_expected(sphere[1], m)
    print(f"m={m}: measured {got:.6f} expected {want:.6f} ({100 * (got / want - 1):+.3f} %)")
    assert abs(got / want - 1.0) <= 0.01


def test_roulette_no_longer_darkens_the_sphere(sphere):
    """m = 12: the reference's estimator divides only the indirect part by the survival probability, so it is lower."""
    ref, got = _sphere(sphere, 12, unbiased=False), _sphere(sphere, 12)
    print(f"m=12: the reference's estimator {ref:.6f}, unbiased {got:.6f}")
    assert ref < got


PARITY_SMALLEST = (lambda: scenes.cornell_box(8), 64, 48, 1, 5)      # tests/test_gpu_path_unbiased.py "spp1"


def test_plumbing():
    fn, W, H, spp, mb = PARITY_SMALLEST
    sc, prm = fn(), P.default_params()
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    a = PO.render_path(o, os_, sc.camera, prm, 0, spp, max_bounces=mb, unbiased=True)
    rays = o.rays
    assert np.array_equal(a, PO.render_path(o, os_, sc.camera, prm, 0, spp, max_bounces=mb, unbiased=True)) and o.rays == rays
    assert not np.array_equal(a, PO.render_path(o, os_, sc.camera, prm, 1, spp, max_bounces=mb, unbiased=True))
    PO.render_path(o, os_, sc.camera, prm, 0, spp, max_bounces=mb)
    print(f"rays: unbiased {rays}, the reference's estimator {o.rays} ({rays / o.rays:.3f})")
    assert W * H < rays < o.rays
    # neither strategy: black on surfaces, emitters and the background as seen, primary rays only
    black = PO.render_path(o, os_, sc.camera, prm, 0, spp, max_bounces=mb, calc_di=False, calc_gi=False, unbiased=True)
    assert o.rays == W * H
    o.render(os_, sc.camera, prm, 0)
    g = o.gbuffer()
    surface = (g[..., 16] > 0) & (g[..., 12:15].sum(-1) == 0)
    assert surface.sum() > 0.5 * W * H and (black[surface] == 0).all() and a[surface].max() > 0
