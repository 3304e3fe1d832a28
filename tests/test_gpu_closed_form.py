"""GPU tests: every estimator of the HIP renderer (produce_restir, render_direct_mis, render_path) against lighting
known in closed form -- the cases, references, masks and bounds of tests/test_closed_form_oracle.py, taken from
tests/closed_form.py, on Renderer.  Nothing here reads the CPU oracle: the bounds are closed_form's constants and the
G-buffer fed to the references is the renderer's own."""
import time

import numpy as np
import pytest

import closed_form as CF
from restir_amd import params as P
from restir_amd.renderer import Renderer

pytestmark = pytest.mark.gpu


class GpuBackend:
    """closed_form's backend over Renderer; frames accumulate on the device (rs_post_frame), one read-back per seed"""

    def __init__(self, traversal=None):
        self.traversal = traversal
        self._scenes = {}

    def _pair(self, cf):
        if cf.name not in self._scenes:
            g = Renderer(cf.width, cf.height)
            if self.traversal:
                g.set_traversal(self.traversal)
            self._scenes[cf.name] = (g, g.load_scene(cf.scene))
        return self._scenes[cf.name]

    def gbuffer(self, cf):
        g, gs = self._pair(cf)
        g.reset_history()
        g.produce_restir(gs, cf.camera, P.default_params(), 0)
        return g.gbuffer()

    def mean_image(self, cf, estimator, seed, n):
        kind, kw = CF.ESTIMATORS[estimator]
        g, gs = self._pair(cf)
        if kind == "mis":
            return g.render_direct_mis(gs, cf.camera, P.default_params(seed=seed), 0, n).astype(np.float64)
        if kind == "path":
            return g.render_path(gs, cf.camera, P.default_params(seed=seed), 0, n, calc_gi=False).astype(np.float64)
        prm = P.default_params(seed=seed, **kw)
        g.reset_history()
        g.post_reset()
        for f in range(n):
            g.produce_restir(gs, cf.camera, prm, f, copy_out=False, timed=False)
            g.post_frame(accumulate=True, tonemap=False, gamma_correct=False, stats=False)
        return g.display_rgba()[..., :3].astype(np.float64)          # display = accumulator (no tonemap, no gamma)


_backends, _refs = {}, {}


def _backend(traversal=None):
    if traversal not in _backends:
        _backends[traversal] = GpuBackend(traversal)
    return _backends[traversal]


def _reference(name):
    if name not in _refs:
        cf = CF.get_scene(name)
        _refs[name] = CF.reference(cf, _backend().gbuffer(cf))
    return _refs[name]


@pytest.mark.parametrize("name", ["open", "blocked", *CF.FURNACE_SCENES])
def test_scene_is_valid_at_the_gpu_gbuffer(name):
    cf, ref = CF.get_scene(name), _reference(name)
    counts = CF.validate(cf, ref.x, ref.n)
    assert all(v == 0 for v in counts.values()), counts
    assert all(v.sum() >= 100 for v in ref.regions.values())
    if ref.umbra is not None:
        assert ref.umbra.sum() >= 4
    if ref.quadrature is not None:
        rel = np.abs(ref.quadrature[ref.mask] - ref.image[ref.mask]) / ref.image[ref.mask]
        assert rel.max() <= CF.QUAD_VS_POLYGON


CASES = [(s, e) for s in ("open", "blocked") for e in CF.ESTIMATORS] + \
        [(s, e) for s in CF.FURNACE_SCENES for e in CF.FURNACE_ESTIMATORS]


def _run(scene, estimator, traversal=None):
    cf, ref = CF.get_scene(scene), _reference(scene)
    b = _backend(traversal)
    t = time.perf_counter()
    result = CF.measure(b, cf, ref, estimator)
    print(f"[closed-form] {scene}/{estimator} ({traversal or 'auto'}): {time.perf_counter() - t:.2f} s")
    CF.check(scene, estimator, result)
    n = 4 if CF.ESTIMATORS[estimator][0] == "restir" else 8
    assert np.array_equal(b.mean_image(cf, estimator, CF.SEEDS[0], n), b.mean_image(cf, estimator, CF.SEEDS[0], n))


@pytest.mark.parametrize("scene,estimator", CASES, ids=[f"{s}-{e}" for s, e in CASES])
def test_estimator_against_closed_form(scene, estimator):
    """Default traversal.  Sum ratio per region within 4 SE of the oracle's scatter (<= 2 %), per-pixel median and p99
    within 1.5 x the recorded ones, umbra dark, the reference's two quirks asserted as quirks, same seed same image."""
    _run(scene, estimator)


@pytest.mark.parametrize("traversal", ["lane", "lockstep"])
def test_blocked_scene_under_pinned_traversal(traversal):
    """The shadow edge under each walk kind: spatial + temporal reuse with pairwise weights."""
    _run("blocked", "pairwise_T1", traversal)


@pytest.mark.parametrize("scene", ["furnace_types_steep", "furnace_types_grazing"])
@pytest.mark.parametrize("estimator", ["mis", "path_nogi"])
def test_dielectric_strip_is_phong_to_mis_and_path(scene, estimator):
    """tests/test_closed_form_oracle.py's check on the renderer: the DIELECTRIC strip typed PHONG, the same image"""
    b = _backend()
    x = b.mean_image(CF.get_scene(scene), estimator, CF.SEEDS[0], 8)
    y = b.mean_image(CF.get_scene(scene + "_swapped"), estimator, CF.SEEDS[0], 8)
    assert np.array_equal(x, y) and x.max() > 0
