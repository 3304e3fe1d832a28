"""Frames without the 8-wide tree.  with_trav (csrc/restir_capi.hip) instantiates every pass kernel for the walk kind
with and without TRAV_WIDE; the rest of the suite renders only scenes whose 8-wide tree is live, so Kind<TRAV_LANE> and
Kind<TRAV_LOCKSTEP> -- what runs under RESTIR_WIDE=off and, automatically, for a scene with a non-finite vertex or a
tree deeper than the walk's stack -- never rendered a frame under test.  Here they do: closest_lane_from /
occluded_lane_from inside the ReSTIR passes, the lockstep kernels' per-lane BRDF rays on the skip pointers, the
`else` arms of the sorted initial / temporal / spatial passes for T = TRAV_LANE, k_path and the MIS ground truth
without a wide tree, and k_scene_update with no wide refit to do.

The reference of every case is the same run with the wide tree live: frames, reservoirs, G-buffer and the ray count
equal bit for bit (closest hits and shadow rays do not depend on the tree).  The first sequence of each
scene is compared with the oracle as well.  Every run asserts the tree state it was loaded with (rs_scene_walk_info)
and, after rendering, the walk kind and the initial pass's split state, so a silent fallback to the covered path
fails the test.
"""
import numpy as np
import pytest

import bvh_brute as B
import gpu_harness as GH
import skip_walk_cases as S
from restir_amd import params as P
from restir_amd import scenes
from gpu_harness import KIND, WALKS
from skip_walk_cases import SIZE, oracle_frames, scns  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu

def _both(monkeypatch, sc, W, H, walk, prms, what, **kw):
    off = S.sequence(monkeypatch, sc, W, H, walk, "off", prms, **kw)
    live = S.sequence(monkeypatch, sc, W, H, walk, None, prms, **kw)
    S.same_runs(off, live, what)
    return off


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("which", ["c2", "c3"])
def test_temporal_spatial_visibility(scns, oracle_frames, which, walk, monkeypatch):
    """three temporal + spatial frames, then a visibility-pass frame; also against the oracle, bit for bit"""
    sc, (W, H) = scns[which], SIZE[which]
    off = _both(monkeypatch, sc, W, H, walk, S.base_prms(), f"{which} {walk}")
    for f, (a, b) in enumerate(zip(off.frames, oracle_frames[which])):
        assert np.array_equal(a, b), f"{which} {walk} frame {f}: {int((a != b).any(-1).sum())} px differ from the oracle"


@pytest.mark.parametrize("m_area", [8, 37])                  # 37: the last chunk of candidates is partial
def test_sorted_passes_lane(scns, m_area, monkeypatch):
    """RESTIR_SORT, RESTIR_SORT_SPATIAL and RESTIR_SORT_TEMPORAL on with per-lane walks and no wide tree: the three
    `else` arms of `if constexpr (trav_lane(T) && trav_wide(T))` in rs_passes.h"""
    sc, (W, H) = scns["c3"], SIZE["c3"]
    srt = _both(monkeypatch, sc, W, H, "lane", S.base_prms(m_area), f"sorted a{m_area}", sort="on")
    plain = S.sequence(monkeypatch, sc, W, H, "lane", "off", S.base_prms(m_area), sort="off")
    S.same_runs(srt, plain, f"sorted vs per-candidate a{m_area}")


@pytest.mark.parametrize("walk", WALKS)
def test_two_brdf_candidates(scns, walk, monkeypatch):
    """m_brdf = 2: the BRDF rays that the lockstep kernels, too, walk per lane -- here on the skip pointers"""
    sc, (W, H) = scns["c3"], SIZE["c3"]
    _both(monkeypatch, sc, W, H, walk, [P.c3_params(m_area=8, m_brdf=2)] * 3, f"m_brdf=2 {walk}")


@pytest.mark.parametrize("which", ["c2", "c3"])
def test_initial_split_lockstep(scns, which, monkeypatch):
    sc, (W, H) = scns[which], SIZE[which]
    _both(monkeypatch, sc, W, H, "lockstep", [P.c3_params(m_area=8)] * 3, f"split {which}", split="on")


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("mis", ["balance", "pairwise"])
def test_spatial_mis_two_passes(scns, mis, walk, monkeypatch):
    sc, (W, H) = scns["c2"], SIZE["c2"]
    prm = P.c3_params(m_area=8, spatial_mis=mis, spatial_passes=2)
    assert prm.spatial_mis != P.CONSTANT
    _both(monkeypatch, sc, W, H, walk, [prm] * 3, f"{mis} {walk}")


@pytest.mark.parametrize("walk", WALKS)
def test_ground_truths(scns, walk, monkeypatch):
    """render_direct_mis (spp 2) and render_path (spp 2, 3 bounces): k_path and the MIS integrator on the skip
    pointers equal the wide-tree launches bit for bit, rays included"""
    sc, (W, H) = scns["c3"], SIZE["c3"]
    prm = P.c3_params()
    out = {}
    for wide in ("off", None):
        g, gs = S.load(monkeypatch, W, H, sc, walk, wide)
        fr = []
        for f in range(2):
            fr.append((g.render_direct_mis(gs, GH.orbit_cam(sc, f), prm, f, 2, timed=True).copy(), int(g.last_times.rays)))
            assert g.traversal()[1] == KIND[walk]
            fr.append((g.render_path(gs, GH.orbit_cam(sc, f), prm, f, 2, max_bounces=3, timed=True).copy(), int(g.last_times.rays)))
            assert g.traversal()[1] == KIND[walk]
        out[wide] = fr
        gs.close()
        g.close()
    for i, ((a, ra), (b, rb)) in enumerate(zip(out["off"], out[None])):
        what = f"{'path' if i % 2 else 'direct MIS'} frame {i // 2} {walk}"
        assert np.isfinite(a).all() and ra >= W * H, what
        assert np.array_equal(a, b), f"{what}: {int((a != b).any(-1).sum())} px differ from the wide-tree launch"
        assert ra == rb, what
    assert not np.array_equal(out["off"][0][0], out["off"][1][0])        # indirect light is in the path frames


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("which", ["c2", "c3"])
def test_update_positions_binary_refit_alone(scns, which, walk, monkeypatch):
    """The plan of test_gpu_parity.test_update_positions_refit_matches_fresh_scene with RESTIR_WIDE=off: the binary
    refit with nothing for the wide refit to do.  Frames equal a fresh scene's, and the refit tree passes the
    structural checker after the amplitude-0.4 motion and again after rs_scene_rebuild."""
    sc, (W, H) = scns[which], SIZE[which]
    prm = P.c3_params(m_area=8)
    g, gs = S.load(monkeypatch, W, H, sc, walk, "off")
    f_ = GH.pinned_renderer(W, H, walk)
    plan = [(0, 0.05, False), (40, 0.05, True), (90, 0.4, False), (130, 0.4, True)]
    n0, p0 = gs.bvh_tree()
    B.check_bvh_tree(n0, p0, sc.positions, 8)
    for f, (t, amp, with_normals) in enumerate(plan):
        pos = scenes.moving_light_positions(sc, t, 240, amplitude=amp)
        gs.update_positions(pos, sc.normals if with_normals else None)
        if f == 3:
            gs.rebuild()
        # (a pipelined update once swapped the reason away with the tree copies: "off" read "too_deep" after it)
        assert gs.walk_info() == {"wide_nodes": 0, "wide_depth": -1, "status": "off"}, f"after update {f}"
        cam = scenes.orbit_camera(sc.camera, f, 240, 0.3)
        a = g.produce_restir(gs, cam, prm, f).copy()
        GH.assert_walked(g, walk)
        fresh = f_.load_scene(scenes.Scene(pos, sc.normals, sc.tri_material, sc.materials, sc.camera))
        assert fresh.walk_info()["status"] == "off"
        b = f_.produce_restir(fresh, cam, prm, f).copy()
        assert np.array_equal(a, b), f"frame {f}: refit != fresh ({int((a != b).any(-1).sum())} px)"
        if f >= 2:
            nodes, prims = gs.bvh_tree()
            B.check_bvh_tree(nodes, prims, pos, 8)
            if f == 2:      # a refit keeps the topology: skips, leaf words and the triangle order
                assert np.array_equal(nodes.view(np.int32)[:, [3, 7]], n0.view(np.int32)[:, [3, 7]]) and np.array_equal(prims, p0)
            else:           # a rebuild is a fresh build
                fn, fp = fresh.bvh_tree()
                assert np.array_equal(nodes.view(np.uint32), fn.view(np.uint32)) and np.array_equal(prims, fp)
            assert gs.walk_info()["status"] == "off"
        fresh.close()
    gs.close()
    g.close()
    f_.close()


def _with_extra_triangle(sc, tri):
    mat = int(np.flatnonzero(~sc.emissive_mask())[0])
    nrm = np.tile(np.array([0, 0, 1], np.float32), 3)[None]
    return scenes.Scene(np.concatenate([sc.positions, np.asarray(tri, np.float32).reshape(1, 9)]),
                        np.concatenate([sc.normals, nrm]),
                        np.concatenate([sc.tri_material, np.array([sc.tri_material[mat]], np.uint32)]),
                        sc.materials, sc.camera)


def test_nonfinite_vertex_falls_back_in_frames(scns, monkeypatch):
    """The automatic fallback: the Cornell scene plus one triangle with a NaN coordinate loads without a wide tree
    (RS_WIDE_NONFINITE).  Its frames are finite, equal between lockstep and per-lane walks, and equal the frames of
    the scene with that triangle replaced by a zero-area triangle at the origin -- neither can be hit."""
    sc, (W, H) = scns["c2"], SIZE["c2"]
    nan_sc = _with_extra_triangle(sc, [0.1, 0.2, 0.3, np.nan, 0.1, 0.5, 0.4, 0.3, 0.9])
    zero_sc = _with_extra_triangle(sc, np.zeros(9))
    prms = S.base_prms()
    out = {}
    for walk in WALKS:
        g, gs = S.load(monkeypatch, W, H, nan_sc, walk, None, status="nonfinite")
        out[walk] = [g.produce_restir(gs, GH.orbit_cam(sc, f), prm, f).copy() for f, prm in enumerate(prms)]
        GH.assert_walked(g, walk)
        gs.close()
        g.close()
    g, gs = S.load(monkeypatch, W, H, zero_sc, "lane", None)
    ref = [g.produce_restir(gs, GH.orbit_cam(sc, f), prm, f).copy() for f, prm in enumerate(prms)]
    gs.close()
    g.close()
    for f in range(len(prms)):
        assert np.isfinite(out["lane"][f]).all()
        assert np.array_equal(out["lane"][f], out["lockstep"][f]), f"frame {f}: lockstep != per-lane"
        assert np.array_equal(out["lane"][f], ref[f]), f"frame {f}: NaN triangle != zero-area triangle"
