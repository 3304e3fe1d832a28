"""GPU tests of the ground truths over a row set (rs_render_ground_truth_rows, Renderer.render_path(rows=...)):
the strips of all phases assemble the full-frame entry's frame bit for bit, a phase writes its own rows and no other,
and its ray counts are its launch's.  72 x 52: a partial tile column, strips of 16, 16, 16 and 4 rows."""
import ctypes

import numpy as np
import pytest

from restir_amd import params as P
from restir_amd import scenes
from restir_amd.renderer import Renderer, RestirError, RowSet

pytestmark = pytest.mark.gpu

W, H = 72, 52
ESTIMATORS = ["mis", "path", "unbiased"]
# 9 levels of vertex records are 72 KiB of dynamic LDS: past what a launch may ask for unannounced
CASES = {"cornell": dict(spp=3, max_bounces=8), "sponza": dict(spp=2, max_bounces=5)}


def _scene(which):
    return scenes.cornell_box(8) if which == "cornell" else scenes.sponza_like(target_tris=30_000, n_lamps=128)


def _render(r, s, cam, prm, est, frame, case, rows=None):
    """One launch; (copy of the framebuffer, rays, primary rays)."""
    if est == "mis":
        img = r.render_direct_mis(s, cam, prm, frame, case["spp"], timed=True, rows=rows)
    else:
        img = r.render_path(s, cam, prm, frame, case["spp"], max_bounces=case["max_bounces"], timed=True,
                            unbiased=est == "unbiased", rows=rows)
    return img.copy(), int(r.last_times.rays), int(r.last_times.primary_rays)


class _Ctx:
    def __init__(self, which, traversal=None, height=H):
        self.sc, self.prm, self.case = _scene(which), P.default_params(), CASES[which]
        self.r = Renderer(W, height)
        if traversal:
            self.r.set_traversal(traversal)
        self.s = self.r.load_scene(self.sc)
        self._full = {}

    def full(self, est, frame):
        """The existing full-frame entry's frame and counts, rendered once."""
        if (est, frame) not in self._full:
            self._full[est, frame] = _render(self.r, self.s, self.sc.camera, self.prm, est, frame, self.case)
        return self._full[est, frame]

    def render(self, est, frame, rows=None):
        return _render(self.r, self.s, self.sc.camera, self.prm, est, frame, self.case, rows)


@pytest.fixture(scope="module", params=list(CASES))
def ctx(request):
    return _Ctx(request.param)


def _check_phases(c, est, strip, stride):
    height = c.r.H
    f0, _, _ = c.full(est, 0)
    f1, rays1, prim1 = c.full(est, 1)
    assert prim1 == W * height and not np.array_equal(f0, f1)
    cur, _, _ = c.render(est, 0)                              # the framebuffer holds full frame 0 again
    assert np.array_equal(cur, f0)
    y = np.arange(height)
    rays = prim = 0
    for p in range(stride):
        own = (y // strip) % stride == p
        img, r, pr = c.render(est, 1, rows=(strip, stride, p))
        assert np.array_equal(img[own], f1[own]), f"{est} {strip}/{stride}/{p}: own rows differ from the full frame"
        assert np.array_equal(img[~own], cur[~own]), f"{est} {strip}/{stride}/{p}: a row outside the set changed"
        assert pr == int(own.sum()) * W
        cur, rays, prim = img, rays + r, prim + pr
    assert np.array_equal(cur, f1)
    assert rays == rays1 and prim == W * height


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("est", ESTIMATORS)
def test_phases_assemble_the_full_frame(ctx, est, world):
    _check_phases(ctx, est, 16, world)


@pytest.mark.parametrize("est", ESTIMATORS)
def test_identity_set_and_wider_strips(ctx, est):
    """{16, 1, 0} is the existing entry; strips of 32 rows (two tile rows each, the last one 20 rows) assemble too."""
    f1, rays1, prim1 = ctx.full(est, 1)
    ctx.render(est, 0)
    img, rays, prim = ctx.render(est, 1, rows=(16, 1, 0))
    assert np.array_equal(img, f1) and (rays, prim) == (rays1, prim1)
    _check_phases(ctx, est, 32, 2)


@pytest.mark.parametrize("traversal", ["lane", "lockstep"])
def test_phases_with_a_fixed_traversal(traversal):
    _check_phases(_Ctx("cornell", traversal), "path", 16, 3)


def test_empty_phase_and_invalid_sets():
    c = _Ctx("cornell", height=40)                            # 3 strips: phase 3 of 4 owns none
    f0, _, _ = c.render("path", 0)
    img, rays, prim = c.render("path", 1, rows=(16, 4, 3))
    assert (rays, prim) == (0, 0) and np.array_equal(img, f0)
    for est in ESTIMATORS:
        for bad in [(0, 2, 0), (-16, 2, 0), (8, 2, 0), (24, 2, 0), (16, 0, 0), (16, -1, 0), (16, 2, 2), (16, 2, -1)]:
            with pytest.raises(RestirError):
                c.render(est, 1, rows=bad)
    # the error code itself, an unknown estimator and a path estimator without its parameters
    from restir_amd.params import PathParams
    from restir_amd.renderer import camera_desc
    cam, pp, rs = camera_desc(c.sc.camera), PathParams(5, True, True, True), RowSet(16, 2, 0)

    def call(est, path, rows):
        return c.r.lib.rs_render_ground_truth_rows(c.r.h, c.s.h, ctypes.byref(cam), ctypes.byref(c.prm), est, path, 1, 1,
                                                   rows, None, None)
    RS_E_INVALID = -1
    assert call(1, ctypes.byref(pp), ctypes.byref(rs)) == 0
    assert call(3, ctypes.byref(pp), ctypes.byref(rs)) == RS_E_INVALID
    assert call(-1, ctypes.byref(pp), ctypes.byref(rs)) == RS_E_INVALID
    assert call(1, None, ctypes.byref(rs)) == RS_E_INVALID
    assert call(2, None, ctypes.byref(rs)) == RS_E_INVALID
    assert call(0, None, ctypes.byref(rs)) == 0
    assert call(1, ctypes.byref(pp), None) == RS_E_INVALID
    for bad in [(8, 2, 0), (16, 0, 0), (16, 2, 2)]:
        assert call(1, ctypes.byref(pp), ctypes.byref(RowSet(*bad))) == RS_E_INVALID
    # the two accepted calls wrote strips 0 and 2; the rejected ones nothing
    assert np.array_equal(c.render("path", 1, rows=(16, 4, 3))[0][16:32], f0[16:32])
