"""CPU tests of the path-tracer checker itself (tests/cpp/path_oracle.c or_render_path, the restatement of
NEEPathIntegrator::integrateImpl2 that tests/test_gpu_path.py holds rs_render_path against): it degenerates to
the direct-MIS oracle bit for bit when global illumination is off or the bounce limit is zero, and in an
integrating sphere it reproduces the closed form of every bounce limit."""
import numpy as np
import pytest

import oracle_lib as O
import path_oracle as PO
from restir_amd import params as P
from restir_amd import scenes

CASES = {"c1": (lambda: scenes.cornell_box(8), P.default_params, 64, 48, 4),
         "phong": (lambda: scenes.sponza_like(target_tris=30_000, n_lamps=128), P.c3_params, 64, 36, 2)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    fn, prm, W, H, spp = CASES[request.param]
    sc = fn()
    return sc, prm(), O.OracleRenderer(W, H), O.OracleScene(sc), spp


def test_gi_off_equals_direct_mis_oracle(case):
    sc, prm, o, os_, spp = case
    ref = o.render_direct_mis(os_, sc.camera, prm, 0, spp)
    rays = o.rays
    for mb in (0, 5, 15):
        assert np.array_equal(PO.render_path(o, os_, sc.camera, prm, 0, spp, max_bounces=mb, calc_gi=False), ref), mb
        assert o.rays == rays
    assert ref.max() > 0


def test_zero_bounces_equals_direct_mis_oracle(case):
    sc, prm, o, os_, _ = case
    for frame in (0, 1):
        ref = o.render_direct_mis(os_, sc.camera, prm, frame, 1)
        assert np.array_equal(PO.render_path(o, os_, sc.camera, prm, frame, 1, max_bounces=0, calc_gi=True), ref)


@pytest.fixture(scope="module")
def sphere():
    sc, f = PO.integrating_sphere()
    return sc, f, O.OracleRenderer(PO.SPHERE_W, PO.SPHERE_H), O.OracleScene(sc)


def test_integrating_sphere_scene(sphere):
    sc, f, _, _ = sphere
    assert sc.n_tris == 1280 and int(sc.emissive_mask().sum()) == 62
    assert abs(f - 0.04907) < 5e-5


@pytest.mark.parametrize("m", [0, 1, 2, 3, 6])
def test_integrating_sphere_closed_form(sphere, m):
    """kd Le f sum_{j<=m} (kd (1 - f))^j within 1 %: the steps from m to m + 1 are 47, 15, 6 and 2.9 % for
    m = 0..3, so an off-by-one in the bounce limit or a double-counted emitter fails; m = 6 has Russian
    roulette live.  (Monte Carlo error of the mean about 0.03 %, tessellation about 0.1 %.)"""
    sc, f, o, os_ = sphere
    prm = P.default_params(use_skybox=0)
    got = PO.sphere_measure(lambda fr: PO.render_path(o, os_, sc.camera, prm, fr, 64, max_bounces=m))
    want = PO.sphere_expected(f, m)
    print(f"m={m}: measured {got:.6f} expected {want:.6f} ({100 * (got / want - 1):+.3f} %)")
    assert abs(got / want - 1.0) <= 0.01
