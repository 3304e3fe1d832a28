"""The spatial pass's batches (rs_passes.h k_spatial, CONSTANT MIS): at the metric point (canon_vis) list position 0 --
the pixel's own sample, known unoccluded -- is evaluated without a walk and the neighbours fill whole pairs (1,2),
(3,4), ...; after a visibility pass the first spatial pass traces it and the pairing stays (0,1), (2,3), ...
No value may change: frames, reservoirs and the ray counter of the lockstep kernels against the per-lane walks, and
frames and reservoirs against the oracle, all with np.array_equal.

k: 1 (one ray after the canonical), 2 and 4 (full last pair), 3 and 5 (half-full last pair), 8, 16 (the last list
cached in LDS), 17 (list_px re-derives the list from the RNG slots); 4 and 8 are the boundaries a selection loop that
gathers its neighbours four at a time would have (measured and not kept, DESIGN 3.20 -- the cases stay for whoever
tries again).  reject_dissimilar and the five spatial_mis modes run the selection loop every mode shares.
Scenes: C2's generator with 64 lights, and with 0.2 m lights, where many drawn neighbours are emissive pixels and are
skipped.  Frames of 50 x 38 (no multiple of the 8 x 8 wave tile) and 64 x 64; two frames per case.  Frames this small
launch k_spatial<T, CM, 1>; the band case drives the same kernel through the tile stages.  The walk kind is pinned and
asserted after the frames, as tests/test_gpu_lockstep_step.py does.
"""
import pytest

import gpu_harness as GH
import oracle_lib as O
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.distributed import GpuTileBackend, band_rows, halo_rows

pytestmark = pytest.mark.gpu

N_FRAMES = 2
KS = [1, 2, 3, 4, 5, 8, 16, 17]
SHAPES = [("c2", 50, 38), ("big_lights", 64, 64)]


@pytest.fixture(scope="module")
def world():
    """name -> (scene, its oracle scene), built once"""
    sc = {"c2": scenes.cornell_many_lights(64), "big_lights": scenes.cornell_many_lights(64, size=0.2)}
    return {k: (v, O.OracleScene(v)) for k, v in sc.items()}


def _prm(**kw):
    """the metric point with three area candidates (the initial pass is not what these cases are about)"""
    return P.metric_params(m_area=3, m_brdf=1, **kw)


def _check(world, which, W, H, prm, what):
    """-> (rays of the lockstep kernels, rays of the oracle)"""
    sc, osc = world[which]
    return GH.check_walks_against_oracle(sc, osc, W, H, prm, what, N_FRAMES)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("which,W,H", SHAPES)
def test_neighbour_counts(world, which, W, H, k):
    _check(world, which, W, H, _prm(spatial_neighbors=k), f"{which} {W}x{H} k={k}")


@pytest.mark.parametrize("k", [3, 4])
def test_canonical_traced_then_known(world, k):
    """after a visibility pass the first spatial pass traces list position 0 (pairs (0,1), (2,3), ...), the second
    knows it unoccluded (0 alone, then (1,2), ...): both pairings in one frame"""
    prm = _prm(spatial_neighbors=k, do_visibility_pass=1, spatial_passes=2)
    _check(world, "c2", 50, 38, prm, f"visibility pass + 2 spatial passes, k={k}")


def test_reject_dissimilar(world):
    """reject_dissimilar reads the neighbours' normals and depths in the selection loop.  The orbit camera sees the
    box's corners and the blocks' edges, so the normal and depth tests reject neighbours there: the oracle traces a
    different number of rays with the flag than without (28312 and 24039 over the two frames; asserted below)."""
    n = {}
    for rej in (0, 1):
        na, no = _check(world, "c2", 50, 38, _prm(spatial_neighbors=5, reject_dissimilar=rej), f"reject_dissimilar={rej}")
        n[rej] = no
    assert n[0] != n[1], f"no neighbour was rejected: {n[0]} oracle rays either way"


@pytest.mark.parametrize("mis", sorted(P.MIS_NAMES))
def test_mis_modes(world, mis):
    """every spatial_mis mode runs the selection loop; only CONSTANT has the paired evaluation"""
    _check(world, "big_lights", 50, 38, _prm(spatial_neighbors=3, spatial_mis=mis), f"spatial_mis={mis}")


def test_full_size_launch(world):
    """1280 x 544: 10 880 waves, past the 2 x 5 120 resident waves of a 256-CU device below which a lockstep launch
    takes the small-launch register budget -- the instantiation k_spatial<T, CM, 0> of a 1080p frame.  Lockstep
    against per-lane only (the oracle would take seconds at this size)."""
    sc, _ = world["c2"]
    prm = _prm(spatial_neighbors=4)
    a = GH.gpu_frames(sc, 1280, 544, [prm] * N_FRAMES, "lockstep")
    b = GH.gpu_frames(sc, 1280, 544, [prm] * N_FRAMES, "lane")
    for f in range(N_FRAMES):
        GH.assert_equal_finite(a.frames[f], b.frames[f], f"frame {f}, lockstep vs per-lane")
    GH.assert_equal_finite(a.res, b.res, "reservoirs, lockstep vs per-lane")
    na, nb = sum(a.rays), sum(b.rays)
    assert na == nb and na > 0, f"{na} rays in lockstep, {nb} per lane"


def test_band(world):
    """two bands of a 64 x 64 frame through the tile stages (k_spatial<T, CM, 1> on 32 rows + halo), both pairings:
    each band equals the same rows of the full frame"""
    import torch
    sc, _ = world["c2"]
    W, H, n_ranks = 64, 64, 2
    prm = _prm(spatial_neighbors=4, do_visibility_pass=1, spatial_passes=2)
    full = GH.gpu_frames(sc, W, H, [prm] * N_FRAMES, "lockstep").frames
    torch.cuda.set_stream(torch.cuda.Stream())
    st = torch.cuda.current_stream().cuda_stream
    rs = [GH.pinned_renderer(W, H, "lockstep", stream=st) for _ in range(n_ranks)]
    bes = [GpuTileBackend(r) for r in rs]
    hs = [be.load_scene(sc) for be in bes]
    h = halo_rows(prm)
    for f in range(N_FRAMES):
        for r, be in enumerate(bes):
            y0, y1 = band_rows(H, r, n_ranks)
            be.begin(hs[r], GH.orbit_cam(sc, f), prm, f, y0, y1, h, h)
        for be in bes:
            be.temporal()
        for p in range(prm.spatial_passes):
            torch.cuda.synchronize()
            bes[1].halo_tensor(0).copy_(bes[0].halo_tensor(3))
            bes[0].halo_tensor(1).copy_(bes[1].halo_tensor(2))
            torch.cuda.synchronize()
            for be in bes:
                be.spatial(p)
        for r, be in enumerate(bes):
            y0, y1 = band_rows(H, r, n_ranks)
            band = be.finish().cpu().numpy().reshape(-1, W, 3)
            GH.assert_equal_finite(band, full[f][y0:y1], f"frame {f}, rows {y0}..{y1}")
    for r in rs:
        assert r.traversal()[1] == 0, "a band did not walk as pinned"
