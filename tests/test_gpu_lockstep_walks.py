"""The lockstep walks (rs_scene.h occluded_wave_multi / occluded_wave / closest_wave) take the wave's next node from
the skip order (rs_lockstep.h lockstep_next) instead of a cross-lane minimum; only a leaf step on which every ray on
the node ended still reduces.  The answers must not change: direct ray queries against the per-lane walks and the
oracle, and whole frames and reservoirs against the per-lane walks, all on the raw values.

Scenes: C2 (cornell_many_lights) and C2 with one large quad 5 mm under the ceiling lights -- every ceiling-bound
shadow ray ends at its first leaf while the wall-bound rays of the same wave go on, which is the reduce path; a
one-triangle scene (the root is a leaf, skip = n_nodes); rays whose tfar lies below every box (no node entered).
The frames pin the walk kind and switch the candidate-split pass off, and assert both after rendering, as
tests/test_gpu_light_lds.py does: AUTO runs frames this small through k_gbuffer_initial_split.
"""
import numpy as np
import pytest

import gpu_harness as GH
import oracle_lib as O
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

N_RAYS = 4096 + 37          # a partial last wave


def _with_blocker():
    return GH.with_ceiling_blocker(scenes.cornell_many_lights(1024), "c2_blocker")


def _one_triangle():
    tri = np.array([[-1, -1, 0, 1, -1, 0, 0, 1, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), 3)[None]
    return scenes.Scene(tri, nrm, np.zeros(1, np.uint32), [scenes.Material(kd=(0.5, 0.5, 0.5))], scenes.CORNELL_CAMERA)


def _shadow_rays(sc, rng):
    """Shadow rays as the initial pass shoots them: from points in the lower box towards emitter centroids, tfar just
    short of the emitter; ceiling and wall emitters mixed inside every wave."""
    em = sc.positions[sc.emissive_mask()].reshape(-1, 3, 3).mean(1)
    wall = em[np.abs(em[:, 1] - 0.985) < 1e-3]
    ceil = em[em[:, 2] > 1.9]
    assert len(wall) == 32 and len(ceil) == 2016
    to_wall = rng.random(N_RAYS) < 0.3
    tgt = np.where(to_wall[:, None], wall[rng.integers(0, len(wall), N_RAYS)], ceil[rng.integers(0, len(ceil), N_RAYS)])
    o = np.stack([rng.uniform(-0.95, 0.95, N_RAYS), rng.uniform(-0.95, 0.9, N_RAYS), rng.uniform(0.02, 1.5, N_RAYS)], 1)
    o = o.astype(np.float32)
    d = (tgt - o).astype(np.float32)
    dist = np.linalg.norm(d, axis=1).astype(np.float32)
    d /= dist[:, None]
    return o, d, (dist * np.float32(0.999)).astype(np.float32), to_wall


def _check_queries(sc, o, d, tnear, tfar_any, tfar_closest=3.0e38):
    """closest and any-hit: lockstep == per-lane == oracle; returns (prim, any) of the lockstep walks"""
    g = Renderer(8, 8)
    gs = g.load_scene(sc)
    os_ = O.OracleScene(sc)
    n = o.shape[0]
    tn = np.full(n, tnear, np.float32)
    tr, pr = os_.trace_closest(o, d, tnear, tfar_closest)
    anyr = os_.trace_any(o, d, tn, tfar_any)
    out = {}
    for lockstep in (True, False):
        t, prim = g.debug_trace(gs, o, d, tnear, tfar_closest, any_hit=False, lockstep=lockstep)
        _, anyg = g.debug_trace(gs, o, d, tn, tfar_any, any_hit=True, lockstep=lockstep)
        out[lockstep] = (t, prim, anyg)
        assert np.array_equal(prim, pr), f"closest prim vs oracle (lockstep={lockstep})"
        assert np.array_equal(GH.bits(t), GH.bits(tr)), f"closest t vs oracle (lockstep={lockstep})"
        assert np.array_equal(anyg, anyr), f"any-hit vs oracle (lockstep={lockstep})"
    for a, b in zip(out[True], out[False]):
        assert np.array_equal(a, b), "lockstep vs per-lane"
    gs.close()
    g.close()
    return out[True][1], out[True][2]


@pytest.mark.parametrize("blocker", [True, False], ids=["c2_blocker", "c2"])
def test_shadow_and_primary_queries(blocker):
    sc = _with_blocker() if blocker else scenes.cornell_many_lights(1024)
    o, d, tf, to_wall = _shadow_rays(sc, np.random.default_rng(5))
    _, occ = _check_queries(sc, o, d, 0.01, tf)
    if blocker:    # the quad stops every ceiling-bound ray; wall-bound rays of the same waves mostly go on to the end
        assert occ[~to_wall].all() and (occ[to_wall] == 0).sum() > 200


@pytest.mark.parametrize("hitting", [True, False], ids=["all_hit", "none_hit"])
def test_root_is_a_leaf(hitting):
    rng = np.random.default_rng(6)
    b = rng.dirichlet([1, 1, 1], N_RAYS) * 0.98 + 0.005          # strictly inside the triangle
    v = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float64)
    o = (b @ v + np.array([0, 0, 1.0])).astype(np.float32)
    d = np.tile(np.array([0, 0, -1 if hitting else 1], np.float32), (N_RAYS, 1))
    prim, occ = _check_queries(_one_triangle(), o, d, 0.0, np.full(N_RAYS, 3.0e38, np.float32))
    assert (prim == (0 if hitting else -1)).all() and (occ != 0).all() == hitting and (occ != 0).any() == hitting


def test_no_node_entered():
    """Rays that start 9 m in front of the box with tfar = 1: the root's box test fails for every ray."""
    sc = scenes.cornell_many_lights(1024)
    rng = np.random.default_rng(7)
    o = np.stack([rng.uniform(-0.5, 0.5, N_RAYS), np.full(N_RAYS, -10.0), rng.uniform(0.5, 1.5, N_RAYS)], 1).astype(np.float32)
    d = np.tile(np.array([0, 1, 0], np.float32), (N_RAYS, 1))
    prim, occ = _check_queries(sc, o, d, 0.01, np.full(N_RAYS, 1.0, np.float32), tfar_closest=1.0)
    assert (prim == -1).all() and (occ == 0).all()


def _frames(sc, W, H, prm, walk, n_frames=3):
    """n_frames frames with two frames in flight and the reservoirs after the last one, walks pinned to `walk`"""
    import torch
    from restir_amd.distributed import _CudaBuf
    torch.cuda.set_stream(torch.cuda.Stream())        # the clones below are ordered on the frames' stream
    g = GH.pinned_renderer(W, H, walk, run_ahead=2, stream=torch.cuda.current_stream().cuda_stream)
    gs = g.load_scene(sc)
    frames = []
    for f in range(n_frames):
        g.produce_restir(gs, GH.orbit_cam(sc, f), prm, f, copy_out=False, timed=False)
        frames.append(torch.as_tensor(_CudaBuf(g.frame_device_ptr(), W * H * 12, "<f4", 4), device="cuda").clone())
    GH.assert_walked(g, walk)
    out = [t.cpu().numpy().reshape(H, W, 3) for t in frames], g.reservoirs()
    gs.close()
    g.close()
    return out


@pytest.fixture(scope="module")
def frame_scenes():
    return {"c2_blocker": _with_blocker(), "c2": scenes.cornell_many_lights(1024)}


@pytest.mark.parametrize("m_area", [32, 3])                   # 3: the last candidate pair has one inactive ray
@pytest.mark.parametrize("W,H", [(50, 38), (64, 48)])
@pytest.mark.parametrize("which", ["c2_blocker", "c2"])
def test_frames_and_reservoirs_equal_per_lane(frame_scenes, which, W, H, m_area):
    sc = frame_scenes[which]
    prm = P.metric_params(m_area=m_area)                      # spatial k = 4
    assert prm.do_spatial == 1 and prm.spatial_neighbors == 4
    fa, ra = _frames(sc, W, H, prm, "lockstep")
    fb, rb = _frames(sc, W, H, prm, "lane")
    for f, (a, b) in enumerate(zip(fa, fb)):
        assert np.isfinite(a).all()
        GH.assert_same_bits(a, b, f"frame {f}, lockstep vs per-lane walks")
    GH.assert_same_bits(ra, rb, "reservoirs, lockstep vs per-lane walks")
