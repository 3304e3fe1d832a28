"""CPU tests: every estimator of the oracle (oracle/restir_oracle.c, tests/cpp/path_oracle.c) against lighting known in
closed form (tests/closed_form.py): Lambert's polygon formula on an unoccluded scene, a float64 quadrature with
brute-force visibility on the same scene with a blocker, and the Phong furnace (kd + ks) Le.  The parity tests prove
the kernels equal the oracle; these prove the oracle (and, in tests/test_gpu_closed_form.py, the kernels) equal the
light.  Bounds and their origin: closed_form.py's docstring; the recorded figures: DESIGN.md section 5."""
import numpy as np
import pytest

import closed_form as CF
import oracle_lib as O
import path_oracle as PO
from restir_amd import params as P


class OracleBackend:
    """closed_form's backend over the CPU oracle"""

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
        kind, kw = CF.ESTIMATORS[estimator]
        o, os_ = self._pair(cf)
        if kind == "mis":
            return o.render_direct_mis(os_, cf.camera, P.default_params(seed=seed), 0, spp=n).astype(np.float64)
        if kind == "path":
            return PO.render_path(o, os_, cf.camera, P.default_params(seed=seed), 0, n, calc_gi=False).astype(np.float64)
        prm = P.default_params(seed=seed, **kw)
        o.reset_history()
        acc = np.zeros((cf.height, cf.width, 3))
        for f in range(n):
            acc += o.render(os_, cf.camera, prm, f)
        return acc / n


@pytest.fixture(scope="module")
def backend():
    return OracleBackend()


_refs = {}


def _reference(backend, name):
    if name not in _refs:
        cf = CF.get_scene(name)
        _refs[name] = CF.reference(cf, backend.gbuffer(cf))
    return _refs[name]


@pytest.mark.parametrize("name", ["open", "blocked", *CF.FURNACE_SCENES])
def test_scene_is_valid(backend, name):
    """closed_form.validate: no emitter behind another, none below a receiver's horizon, none with a shading normal
    off its plane; the regions the assertions sum over are populated (every furnace strip covers >= 100 pixels)."""
    cf, ref = CF.get_scene(name), _reference(backend, name)
    counts = CF.validate(cf, ref.x, ref.n)
    print(f"[closed-form] {name}: {counts}; pixels per region { {k: int(v.sum()) for k, v in ref.regions.items()} }"
          + (f"; umbra {int(ref.umbra.sum())}" if ref.umbra is not None else ""))
    assert all(v == 0 for v in counts.values()), counts
    assert all(v.sum() >= 100 for v in ref.regions.values())
    assert ref.mask.sum() > 0.4 * cf.width * cf.height or name.startswith("furnace")
    if ref.umbra is not None:
        assert ref.umbra.sum() >= 4


def test_validate_catches_the_two_scene_mistakes(backend):
    """A bent emitter shading normal and an emitter hanging in front of another are both counted."""
    cf, ref = CF.get_scene("open"), _reference(backend, "open")
    e = int(np.nonzero(cf.emissive)[0][0])
    bent = CF.CFScene(**{**vars(cf), "shading_normals": cf.shading_normals.copy()})
    bent.shading_normals[e] = [0.1, 0.0, -0.995]
    assert CF.validate(bent, ref.x, ref.n)["emitters_with_bent_shading_normal"] == 1
    hung = CF.CFScene(**{**vars(cf), "tris": cf.tris.copy()})
    hung.tris[e] = hung.tris[e] * [2.0, 2.0, 1.0] - [0.0, 0.0, 0.3]            # a larger emitter 0.3 below the others
    assert CF.validate(hung, ref.x, ref.n)["segments_crossing_another_emitter"] > 0
    low = CF.CFScene(**{**vars(cf), "tris": cf.tris.copy()})
    low.tris[e, 0, 2] = -0.5
    assert CF.validate(low, ref.x, ref.n)["emitter_vertices_below_a_horizon"] > 0


def test_quadrature_agrees_with_polygon_formula(backend):
    """On open_scene the two references are the same integral: the quadrature is pinned by Lambert's formula before
    it is trusted with the blocker.  Also the quadrature's visibility finds nothing in the way there."""
    cf, ref = CF.get_scene("open"), _reference(backend, "open")
    rel = np.abs(ref.quadrature[ref.mask] - ref.image[ref.mask]) / ref.image[ref.mask]
    print(f"[closed-form] quadrature vs polygon formula over {ref.mask.sum()} pixels: max {rel.max():.3g} "
          f"median {np.median(rel):.3g}")
    assert rel.max() <= CF.QUAD_VS_POLYGON
    g = backend.gbuffer(cf).astype(np.float64)
    _, vis = CF.quadrature_radiance(cf, ref.x[::7], ref.n[::7], g[ref.mask][::7, 6:9])
    assert (vis == 1.0).all()


def test_polygon_formula_known_values():
    """Lambert's formula against an elementary answer: a regular 720-gon of radius 0.5 one unit overhead is a disc to
    within (pi / 720)^2, and a disc of half angle alpha irradiates the point below it with pi sin^2(alpha).  Tilting
    the receiver by beta (disc still above its horizon) multiplies that by cos(beta)."""
    k = 720
    a = 2 * np.pi * np.arange(k) / k
    disc = np.stack([0.5 * np.cos(a), 0.5 * np.sin(a), np.ones(k)], -1)
    want = np.pi * 0.25 / 1.25                                                # tan(alpha) = 0.5
    n = np.array([[0, 0, 1.0], [np.sin(0.3), 0, np.cos(0.3)]])
    got = CF.polygon_irradiance(np.zeros((2, 3)), n, disc)
    assert abs(got[0] / want - 1) < 1e-4 and abs(got[1] / (want * np.cos(0.3)) - 1) < 1e-4
    assert np.allclose(CF.polygon_irradiance(np.zeros((2, 3)), n, disc[::-1]), got, rtol=1e-12)      # either winding


CASES = [(s, e) for s in ("open", "blocked") for e in CF.ESTIMATORS] + \
        [(s, e) for s in CF.FURNACE_SCENES for e in CF.FURNACE_ESTIMATORS]


@pytest.mark.parametrize("scene,estimator", CASES, ids=[f"{s}-{e}" for s, e in CASES])
def test_estimator_against_closed_form(backend, scene, estimator):
    """Sum ratio per region within 4 SE (<= 2 %), per-pixel median and p99 within 1.5 x the recorded ones, umbra dark;
    the two reference quirks asserted as quirks.  The same seed twice gives the same image."""
    cf, ref = CF.get_scene(scene), _reference(backend, scene)
    CF.check(scene, estimator, CF.measure(backend, cf, ref, estimator))
    n = 4 if CF.ESTIMATORS[estimator][0] == "restir" else 8
    assert np.array_equal(backend.mean_image(cf, estimator, CF.SEEDS[0], n), backend.mean_image(cf, estimator, CF.SEEDS[0], n))


@pytest.mark.parametrize("scene", ["furnace_types_steep", "furnace_types_grazing"])
@pytest.mark.parametrize("estimator", ["mis", "path_nogi"])
def test_dielectric_strip_is_phong_to_mis_and_path(backend, scene, estimator):
    """The kd + ks darkness of the DIELECTRIC strip is Phong's quirk and nothing else: with that strip typed PHONG the
    image is the same bit for bit (and the quirk itself is bracketed by test_estimator_against_closed_form)."""
    a = backend.mean_image(CF.get_scene(scene), estimator, CF.SEEDS[0], 8)
    b = backend.mean_image(CF.get_scene(scene + "_swapped"), estimator, CF.SEEDS[0], 8)
    assert np.array_equal(a, b) and a.max() > 0
    assert CF.is_quirk(scene, estimator, "dielectric") and not CF.is_quirk(scene, estimator, "normal")
