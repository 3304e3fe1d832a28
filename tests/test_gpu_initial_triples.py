"""The one-thread-per-pixel initial pass of the lockstep kinds (rs_passes.h initial_ris, area_batch_px) walks three area
candidates' shadow rays together, and the first BRDF candidate's shadow ray rides in the last area batch's walk when
that batch has a free slot (m_area % 3 != 0, m_brdf >= 1, rays traced in the pass).  The reservoir updates keep their
candidate order and RNG slots, so no value may change: frames, reservoirs and ray counts of the lockstep kernel
against the per-lane walks (one candidate per walk), frames and reservoirs against the oracle, all with
np.array_equal.  (The oracle's ray counter is not the kernels': on the first case it reads 5292 where both walk kinds
of this tree and of its parent count 4163, so ray counts are compared between the walk kinds, as
tests/test_gpu_lockstep_step.py does.)

m_area: 1, 2 (a single peeled batch), 3, 6 (full batches only), 4, 5, 7 (full batches and a last batch of one or two),
31, 32, 33 (C2's counts); m_brdf 0 (no rider), 1 (the rider only), 2 (the rider, then a walk of its own).  70 x 41
leaves clamped lanes in the edge tiles.  Both light-table sources (RESTIR_LIGHT_LDS: the LDS kernel makes a batch's
picks when it needs them, the global-table kernel a batch ahead).  The walks are pinned and the candidate-split pass
is off, and both are asserted after every frame, as tests/test_gpu_light_lds.py does.

A renderer per (shape, scene, walk kind, table source) is made once and renders every candidate count: no pass here
keeps history between frames, and the switch is read when a context is created.
"""
import pytest

import gpu_harness as GH
import oracle_lib as O
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.distributed import GpuTileBackend

pytestmark = pytest.mark.gpu

M_AREA = [1, 2, 3, 4, 5, 6, 7, 31, 32, 33]
M_BRDF = [0, 1, 2]
SHAPES = [(70, 41), (64, 48)]
SCENES = ["many_lights", "box"]
FRAME = 1                                   # one frame per case, a step along the orbit


class _World:
    """scenes, oracle scenes and renderers, each made on first use and kept for the module"""

    def __init__(self):
        self.made = {"many_lights": lambda: scenes.cornell_many_lights(64), "box": lambda: scenes.cornell_box(8),
                     "blocker": lambda: GH.with_ceiling_blocker(scenes.cornell_many_lights(1024), "c2_blocker")}
        self.sc, self.osc, self.gpu, self.orc = {}, {}, {}, {}

    def scene(self, which):
        if which not in self.sc:
            self.sc[which] = self.made[which]()
            self.osc[which] = O.OracleScene(self.sc[which])
        return self.sc[which], self.osc[which]

    def renderer(self, which, W, H, walk, lds):
        key = (which, W, H, walk, lds)
        if key not in self.gpu:
            with pytest.MonkeyPatch.context() as mp:
                GH.set_env(mp, RESTIR_LIGHT_LDS=lds)
                g = GH.pinned_renderer(W, H, walk)
            self.gpu[key] = (g, g.load_scene(self.scene(which)[0]))
        return self.gpu[key]

    def oracle(self, W, H):
        if (W, H) not in self.orc:
            self.orc[(W, H)] = O.OracleRenderer(W, H)
        return self.orc[(W, H)]

    def close(self):
        for g, gs in self.gpu.values():
            gs.close()
            g.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _gpu(world, which, W, H, prm, walk, lds="auto"):
    """(frame, reservoirs, rays) of one frame with the walks pinned to `walk`"""
    g, gs = world.renderer(which, W, H, walk, lds)
    frame = g.produce_restir(gs, GH.orbit_cam(world.scene(which)[0], FRAME), prm, FRAME).copy()
    rays = int(g.last_times.rays)
    GH.assert_walked(g, walk)
    return frame, g.reservoirs().copy(), rays


def _oracle(world, which, W, H, prm):
    sc, osc = world.scene(which)
    o = world.oracle(W, H)
    frame = o.render(osc, GH.orbit_cam(sc, FRAME), prm, FRAME)
    return frame, o.reservoirs(), o.rays


def _check(world, which, W, H, prm, what, tables=("auto", "off")):
    fb, rb, nb = _gpu(world, which, W, H, prm, "lane")
    fo, ro, no = _oracle(world, which, W, H, prm)
    for lds in tables:
        fa, ra, na = _gpu(world, which, W, H, prm, "lockstep", lds)
        w = f"{what}, RESTIR_LIGHT_LDS={lds}"
        GH.assert_equal_finite(fa, fb, f"{w}: frame, lockstep vs per-lane")
        GH.assert_equal_finite(fa, fo, f"{w}: frame, lockstep vs oracle")
        GH.assert_equal_finite(ra, rb, f"{w}: reservoirs, lockstep vs per-lane")
        GH.assert_equal_finite(ra, ro, f"{w}: reservoirs, lockstep vs oracle")
        assert na == nb and na > 0, f"{w}: {na} rays in lockstep, {nb} per lane"


@pytest.mark.parametrize("m_brdf", M_BRDF)
@pytest.mark.parametrize("m_area", M_AREA)
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("which", SCENES)
def test_initial_pass(world, which, W, H, m_area, m_brdf):
    _check(world, which, W, H, P.default_params(m_area=m_area, m_brdf=m_brdf), f"{which} {W}x{H} ({m_area}, {m_brdf})")


@pytest.mark.parametrize("m_area,m_brdf", [(2, 1), (4, 1), (6, 2), (32, 1)])
@pytest.mark.parametrize("which", SCENES)
def test_visibility_pass(world, which, m_area, m_brdf):
    """do_visibility_pass: the initial pass traces no shadow ray (no rider either: the BRDF candidate is drawn after
    the area candidates), the visibility pass walks one ray per lane"""
    prm = P.default_params(m_area=m_area, m_brdf=m_brdf, do_visibility_pass=1)
    _check(world, which, 70, 41, prm, f"{which} visibility pass ({m_area}, {m_brdf})")


@pytest.mark.parametrize("m_area,m_brdf", [(4, 1), (32, 1), (33, 2), (5, 0)])
def test_reduce_path(world, m_area, m_brdf):
    """C2 under a quad that hides the ceiling lights (tests/test_gpu_lockstep_walks.py): every ceiling-bound shadow
    ray ends at its first leaf while the wall-bound rays of the wave go on -- the walk's cross-lane minimum"""
    _check(world, "blocker", 70, 41, P.default_params(m_area=m_area, m_brdf=m_brdf), f"blocker ({m_area}, {m_brdf})")


@pytest.mark.parametrize("m_area,m_brdf", [(4, 1), (32, 1), (33, 2)])
def test_band(world, m_area, m_brdf):
    """rows 13..30 of the 70 x 41 frame through the tile stages (y0 and y1 inside the frame and off the 8-px tile
    grid): the band's rows, their reservoirs and the ray count against the per-lane walks, and the rows against the
    oracle's full frame (every pixel of this pass stands alone)"""
    W, H, y0, y1 = 70, 41, 13, 31
    prm = P.default_params(m_area=m_area, m_brdf=m_brdf)
    sc, _ = world.scene("many_lights")
    out = {}
    for walk in ("lockstep", "lane"):
        g, gs = world.renderer("many_lights", W, H, walk, "auto")
        be = GpuTileBackend(g)
        be.begin(gs, GH.orbit_cam(sc, FRAME), prm, FRAME, y0, y1, 0, 0)
        be.temporal()
        band = be.finish(timed=True).cpu().numpy().reshape(-1, W, 3).copy()
        GH.assert_walked(g, walk)
        out[walk] = band, g.reservoirs()[y0:y1].copy(), int(g.last_times.rays)
    fo, ro, _ = _oracle(world, "many_lights", W, H, prm)
    what = f"band ({m_area}, {m_brdf})"
    GH.assert_equal_finite(out["lockstep"][0], out["lane"][0], f"{what}: rows, lockstep vs per-lane")
    GH.assert_equal_finite(out["lockstep"][0], fo[y0:y1], f"{what}: rows, lockstep vs oracle")
    GH.assert_equal_finite(out["lockstep"][1], out["lane"][1], f"{what}: reservoirs, lockstep vs per-lane")
    GH.assert_equal_finite(out["lockstep"][1], ro[y0:y1], f"{what}: reservoirs, lockstep vs oracle")
    assert out["lockstep"][2] == out["lane"][2] and out["lockstep"][2] > 0, f"{what}: rays {out['lockstep'][2]} vs {out['lane'][2]}"
