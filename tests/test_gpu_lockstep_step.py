"""The lockstep walks' step (rs_scene.h occluded_wave_multi / occluded_wave / closest_wave) branches on the leaf flag
first, and on an interior node each ray tests the box and moves its cursor inside its own region (lockstep_enter).
No value may change: frames, reservoirs and the ray counter of the lockstep kernels against the per-lane walks, and
frames and reservoirs against the oracle, all with np.array_equal.

(m_area, m_brdf): with two area candidates per walk the last batch is full (2, 32), half full (1, 3) or absent (0);
the BRDF candidate (a one-ray walk of its own) is absent, single or double.
Scenes: C2's generator with 64 lights, the same under a quad that hides the ceiling lights (every ceiling-bound shadow
ray ends in its first leaf), and with 0.2 m lights, where the BRDF candidate's ray exists in most lanes (a cosine
direction rarely lands on a 0.02 m quad).  The walk kind is pinned and the candidate-split pass switched off, and both
are asserted after the frames, as tests/test_gpu_light_lds.py does.
"""
import pytest

import oracle_lib as O
from gpu_harness import check_walks_against_oracle, with_ceiling_blocker
from restir_amd import params as P
from restir_amd import scenes

pytestmark = pytest.mark.gpu

N_FRAMES = 2
PAIRS = [(1, 1), (2, 1), (3, 1), (32, 1), (2, 0), (0, 1), (2, 2)]
SHAPES = [("c2", 64, 64), ("c2", 50, 38), ("blocker", 50, 38), ("big_lights", 50, 38)]


@pytest.fixture(scope="module")
def world():
    """name -> (scene, its oracle scene), built once"""
    sc = {"c2": scenes.cornell_many_lights(64), "big_lights": scenes.cornell_many_lights(64, size=0.2)}
    sc["blocker"] = with_ceiling_blocker(sc["c2"], "c2_64_blocker")
    return {k: (v, O.OracleScene(v)) for k, v in sc.items()}


def _check(world, which, W, H, prm, what):
    sc, osc = world[which]
    check_walks_against_oracle(sc, osc, W, H, prm, what, N_FRAMES)


@pytest.mark.parametrize("m_area,m_brdf", PAIRS)
@pytest.mark.parametrize("which,W,H", SHAPES)
def test_initial_pass(world, which, W, H, m_area, m_brdf):
    _check(world, which, W, H, P.default_params(m_area=m_area, m_brdf=m_brdf), f"{which} {W}x{H} ({m_area}, {m_brdf})")


@pytest.mark.parametrize("which", ["c2", "big_lights"])
def test_visibility_pass(world, which):
    """do_visibility_pass: the initial pass traces no shadow ray, the visibility pass walks one ray per lane"""
    _check(world, which, 50, 38, P.default_params(m_area=2, m_brdf=1, do_visibility_pass=1), f"{which} visibility pass")


@pytest.mark.parametrize("which", ["blocker", "big_lights"])
def test_spatial_reuse(world, which):
    """k = 4 neighbours: k_spatial pairs its shadow rays through the same walk"""
    prm = P.metric_params(m_area=3, m_brdf=1)
    assert prm.do_spatial == 1 and prm.spatial_neighbors == 4
    _check(world, which, 50, 38, prm, f"{which} spatial")
