"""GPU parity tests: the HIP path (through the C ABI, librestir_amd.so) against the oracle on the
same seeded inputs.

Tolerances:
  * BVH queries: bit-exact (same Moller-Trumbore arithmetic, same tie rule) -- hit prim and t.
  * G-buffer: bit-exact (round 6: the transcendentals come from one shared sequence, csrc/rs_libm.h).
  * frame: per-pixel relative L2 <= 1e-4 on >= 99.5 % of pixels and mean relative L2 <= 1e-4 for the older
    tests (written when ocml and glibc differed in the last ulp and a reservoir selection could flip); the
    frames here are bit-identical since round 6, and the newer tests assert that (the residue measured at the
    BASELINE sizes is in tests/test_gpu_workloads.py).
"""
import os
import tempfile

import numpy as np
import pytest

import oracle_lib as O
from gpu_harness import assert_close, orbit_cam
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.renderer import Renderer, RestirError

pytestmark = pytest.mark.gpu

def _pair(sc, W, H, prm, frames=1, cam=None):
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    o = O.OracleRenderer(W, H)
    os_ = O.OracleScene(sc)
    out = []
    for f in range(frames):
        c = cam(f) if cam else sc.camera
        a = g.produce_restir(gs, c, prm, f).copy()
        b = o.render(os_, c, prm, f)
        out.append((a, b))
    return g, o, out


# ---------------------------------------------------------------- BVH build + traversal
@pytest.mark.parametrize("scene_fn", [lambda: scenes.cornell_box(8), lambda: scenes.cornell_many_lights(1024),
                                      lambda: scenes.sponza_like(target_tris=40_000, n_lamps=256)])
def test_bvh_queries_bit_exact(scene_fn):
    sc = scene_fn()
    g = Renderer(8, 8)
    gs = g.load_scene(sc)
    assert gs.n_tris == sc.n_tris and gs.n_emissive == int(sc.emissive_mask().sum())
    os_ = O.OracleScene(sc)
    rng = np.random.default_rng(11)
    n = 20000
    lo = sc.positions.reshape(-1, 3).min(0)
    hi = sc.positions.reshape(-1, 3).max(0)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:100, 0] = 0.0                      # axis-parallel rays (inf reciprocals)
    d[100:200, 1] = 0.0
    tr, pr = os_.trace_closest(o, d, 0.01, 3.0e38)
    tf = np.where(tr > 0, tr * np.float32(0.999), np.float32(2.0)).astype(np.float32)
    tf[::3] = np.where(tr[::3] > 0, tr[::3] * np.float32(1.001), np.float32(5.0))
    anyr = os_.trace_any(o, d, np.full(n, 0.01, np.float32), tf)
    for lockstep in (True, False):          # wave-coherent traversal used by the passes, and per-lane
        t, prim = g.debug_trace(gs, o, d, 0.01, 3.0e38, any_hit=False, lockstep=lockstep)
        assert np.array_equal(prim, pr)
        assert np.array_equal(t, tr)
        _, anyg = g.debug_trace(gs, o, d, np.full(n, 0.01, np.float32), tf, any_hit=True, lockstep=lockstep)
        assert np.array_equal(anyg, anyr)


def test_bvh_degenerate_scenes():
    # one triangle, and two coplanar overlapping triangles (tie rule: smaller index wins)
    tri = np.array([[-1, -1, 0, 1, -1, 0, 0, 1, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), 3)[None]
    for k in (1, 2, 5):
        sc = scenes.Scene(np.repeat(tri, k, 0), np.repeat(nrm, k, 0), np.zeros(k, np.uint32),
                          [scenes.Material(kd=(0.5, 0.5, 0.5))], scenes.CORNELL_CAMERA)
        g = Renderer(4, 4)
        gs = g.load_scene(sc)
        o = np.array([[0, -0.2, 1], [0.9, 0.9, 1], [0, 0, -1]], np.float32)
        d = np.array([[0, 0, -1], [0, 0, -1], [0, 0, 1]], np.float32)
        for lockstep in (True, False):
            t, prim = g.debug_trace(gs, o, d, 0.0, 3e38, any_hit=False, lockstep=lockstep)
            assert list(prim) == [0, -1, 0] and t[0] == 1.0 and t[2] == 1.0


# ---------------------------------------------------------------- per-pass state
def test_gbuffer_matches_oracle():
    sc = scenes.cornell_box(8)
    g, o, _ = _pair(sc, 96, 80, P.default_params())
    a, b = g.gbuffer(), o.gbuffer()
    assert np.array_equal(a, b)                # 1/I_M included (shared rs_libm.h lgammaf / expf / powf)


def test_initial_reservoirs_match_oracle():
    sc = scenes.cornell_many_lights(256)
    g, o, frames = _pair(sc, 80, 64, P.default_params(m_area=8))
    ra, rb = g.reservoirs(), o.reservoirs()
    same_sample = np.all(ra[..., 0:9] == rb[..., 0:9], axis=-1)
    assert same_sample.mean() >= 0.995
    assert np.array_equal(ra[..., 11], rb[..., 11])          # confidence (capped)
    assert_close(*frames[0], "C2-like initial")


# ---------------------------------------------------------------- frames
def test_frame_c1_reference_defaults():
    sc = scenes.cornell_box(8)
    _, _, frames = _pair(sc, 128, 128, P.default_params())
    assert_close(*frames[0], "C1")


def test_frame_c2_metric_point():
    sc = scenes.cornell_many_lights(1024)
    _, _, frames = _pair(sc, 192, 108, P.metric_params())
    assert_close(*frames[0], "C2 metric")


@pytest.mark.parametrize("mis", ["constant", "debias_contrib", "debias_z", "balance", "pairwise"])
def test_spatial_mis_modes(mis):
    sc = scenes.cornell_box(8)
    prm = P.default_params(m_area=4, do_spatial=1, spatial_neighbors=3, spatial_passes=2, spatial_mis=mis)
    _, _, frames = _pair(sc, 64, 48, prm)
    assert_close(*frames[0], mis)


@pytest.mark.parametrize("mis", ["constant", "debias_contrib", "debias_z", "balance", "pairwise"])
def test_canonical_visibility_with_visibility_pass(mis):
    """F.canon_vis (restir_capi.hip): the spatial pass skips the canonical sample's ray when that sample is known
    unoccluded from the pixel -- never after a visibility pass on the first spatial pass, always on the second.
    Visibility pass + temporal + two spatial passes in every MIS mode over a moving camera: frames and
    reservoirs bit-identical to the oracle, which traces every such ray."""
    sc = scenes.cornell_many_lights(128)
    prm = P.default_params(m_area=6, do_visibility_pass=1, do_temporal=1, do_spatial=1, spatial_neighbors=4,
                           spatial_passes=2, spatial_mis=mis)
    cam = lambda f: scenes.orbit_camera(sc.camera, f, 24, 0.3)
    g, o, frames = _pair(sc, 64, 48, prm, frames=3, cam=cam)
    for i, (a, b) in enumerate(frames):
        assert np.array_equal(a, b), f"{mis} frame {i}: {int(np.any(a != b, -1).sum())} px differ"
    assert np.array_equal(g.reservoirs(), o.reservoirs())


def test_temporal_spatial_sequence_moving_camera():
    sc = scenes.cornell_box(8)
    prm = P.default_params(m_area=4, do_spatial=1, spatial_neighbors=4, do_temporal=1)
    cam = lambda f: scenes.orbit_camera(sc.camera, f, 24, 0.3)
    _, _, frames = _pair(sc, 96, 72, prm, frames=4, cam=cam)
    for i, (a, b) in enumerate(frames):
        assert_close(a, b, f"temporal frame {i}")


def test_visibility_pass_and_reject_dissimilar():
    sc = scenes.cornell_many_lights(128)
    prm = P.default_params(m_area=6, do_visibility_pass=1, do_spatial=1, spatial_neighbors=4, reject_dissimilar=1)
    _, _, frames = _pair(sc, 80, 60, prm, frames=2)
    for a, b in frames:
        assert_close(a, b, "visibility+reject")


def test_phong_scene_c3_small():
    sc = scenes.sponza_like(target_tris=30_000, n_lamps=128)
    prm = P.c3_params(m_area=8)
    cam = lambda f: scenes.orbit_camera(sc.camera, f, 240, 0.3)
    _, _, frames = _pair(sc, 96, 54, prm, frames=2, cam=cam)
    for a, b in frames:
        assert_close(a, b, "sponza-like")


@pytest.mark.parametrize("which", ["c2", "c3"])
def test_traversal_kinds_bit_identical(which):
    """LOCKSTEP, LANE and AUTO (which alternates the kinds over its first six frames) render
    bit-identical frames, matching the oracle; AUTO has settled on a kind after six frames, and its
    later frames dispatch the tile rows in the measured cost order (ragged last tile row included)."""
    if which == "c2":
        sc, prm, W, H = scenes.cornell_many_lights(1024), P.metric_params(), 64, 48
        cam = lambda f: sc.camera
    else:
        sc, prm, W, H = scenes.sponza_like(target_tris=30_000, n_lamps=128), P.c3_params(m_area=8), 64, 40
        cam = lambda f: scenes.orbit_camera(sc.camera, f, 240, 0.3)
    n_frames = 9
    frames = {}
    for mode in ("lockstep", "lane", "auto"):
        g = Renderer(W, H)
        g.set_traversal(mode)
        gs = g.load_scene(sc)
        frames[mode] = [g.produce_restir(gs, cam(f), prm, f).copy() for f in range(n_frames)]
        if mode == "auto":
            m, last, choice = g.traversal(gs)
            assert m == -1 and choice in (0, 1) and last == choice
    for f in range(n_frames):
        assert np.array_equal(frames["lockstep"][f], frames["lane"][f]), f"frame {f}: lockstep != lane"
        assert np.array_equal(frames["lockstep"][f], frames["auto"][f]), f"frame {f}: lockstep != auto"
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    for f in range(2):
        assert_close(frames["lane"][f], o.render(os_, cam(f), prm, f), f"{which} frame {f}")


@pytest.mark.parametrize("which", ["c2", "c3", "brdf2", "odd"])
def test_initial_split_bit_identical(which):
    """The candidate-split initial pass (a pixel's candidates over 4 waves, LDS weight exchange) renders
    frames bit-identical to the one-thread-per-pixel pass for both traversal kinds, incl. B=2 BRDF
    candidates, no area candidates, odd candidate counts and a ragged image; AUTO picks split for a
    small launch with lockstep walks."""
    W, H = 64, 40
    cam = lambda f: sc.camera
    if which == "c2":
        sc, prm = scenes.cornell_many_lights(1024), P.metric_params()
    elif which == "c3":
        sc, prm = scenes.sponza_like(target_tris=30_000, n_lamps=128), P.c3_params(m_area=7)
        cam = lambda f: scenes.orbit_camera(sc.camera, f, 240, 0.3)
    elif which == "brdf2":
        sc, prm = scenes.cornell_box(8), P.default_params(m_area=5, m_brdf=2, do_temporal=1, do_spatial=1)
    else:
        sc, prm, W, H = scenes.cornell_box(8), P.default_params(m_area=0, m_brdf=1), 45, 27
    out = {}
    for trav in ("lockstep", "lane"):
        for split in ("off", "on", "auto"):
            g = Renderer(W, H)
            g.set_traversal(trav)
            g.set_initial_split(split)
            gs = g.load_scene(sc)
            out[trav, split] = [g.produce_restir(gs, cam(f), prm, f).copy() for f in range(3)]
            if split == "auto":                  # small launch: split for lockstep walks only
                assert g.initial_split() == (-1, trav == "lockstep")
            elif split == "on":
                assert g.initial_split() == (1, True)
    ref = out["lockstep", "off"]
    for k, v in out.items():
        for f in range(3):
            assert np.array_equal(ref[f], v[f]), f"{which} {k} frame {f}"
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    assert_close(out["lane", "on"][0], o.render(os_, cam(0), prm, 0), f"{which} split vs oracle")


@pytest.mark.parametrize("which", ["c2", "c3", "c5", "c5mix", "fused"])
def test_run_ahead_bit_identical(which):
    """Frame pipelining (initial pass of frame f+1 on the side stream, overlapping frame f's later
    passes) renders the same frames as strictly sequential frames, with temporal reuse, moving
    geometry (rs_scene_update_positions between frames) and a fused-shade configuration.  The traversal
    kind is pinned: AUTO's first six frames are tuning frames, which run alone on the context's stream;
    pinned, every frame after the first runs on its lane beside the frames before it, and frames are
    only cloned on the frames' stream (no host sync between frames), so the overlap really happens."""
    W, H = 96, 64
    upd = None
    cam = lambda f: orbit_cam(sc, f)
    if which == "c2":
        sc, prm = scenes.cornell_many_lights(1024), P.metric_params()
    elif which == "c3":
        sc, prm = scenes.sponza_like(target_tris=30_000, n_lamps=128), P.c3_params(m_area=6)
    elif which == "c5":
        sc, prm = scenes.cornell_many_lights(256), P.c3_params(m_area=6)
        upd = lambda f: (scenes.moving_light_positions(sc, f, 48), None)
    elif which == "c5mix":
        # pipelined updates (the second scene copy), frames without an update, and in-place updates
        # with normals (which drain the pipeline) in one sequence
        sc, prm = scenes.cornell_many_lights(256), P.c3_params(m_area=6)
        upd = lambda f: (None if f % 4 == 2 else scenes.moving_light_positions(sc, f, 48),
                         sc.normals if f % 4 == 3 else None)
    else:
        sc, prm = scenes.cornell_box(8), P.default_params(m_area=4)
    import torch
    from restir_amd.distributed import _CudaBuf
    torch.cuda.set_stream(torch.cuda.Stream())       # the clones below are ordered on the frames' stream
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    n_frames = 10 if which == "c5mix" else 6
    for ra in (0, 1, 2):
        g = Renderer(W, H, stream=st)
        g.set_traversal("lane" if which == "c3" else "lockstep")
        g.set_run_ahead(ra)
        gs = g.load_scene(sc)
        frames = []
        for f in range(n_frames):
            if upd:
                pos, nrm = upd(f)
                if pos is not None:
                    gs.update_positions(pos, nrm)
            g.produce_restir(gs, cam(f), prm, f, copy_out=False, timed=False)
            frames.append(torch.as_tensor(_CudaBuf(g.frame_device_ptr(), W * H * 12, "<f4", 4), device="cuda").clone())
        out[ra] = [t.cpu().numpy().reshape(H, W, 3) for t in frames]
    for f in range(n_frames):
        for ra in (1, 2):
            assert np.array_equal(out[0][f], out[ra][f]), f"{which} depth {ra} frame {f}"
    if which not in ("c5", "c5mix"):
        o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
        for f in range(2):
            assert_close(out[2][f], o.render(os_, cam(f), prm, f), f"{which} run-ahead frame {f}")


def test_run_ahead_sequencing_bit_identical():
    """The host sequencing no other test crosses, in one run: traversal left on AUTO (six tuning frames on the
    context's stream with their row-cost recording, then the tile-row order) with frames in flight, the depth changed
    2 -> 0 -> 1 -> 2 between frames, pipelined position updates on most frames, one in-place update with normals, and
    a ground-truth render (lane 0, the context's stream) between two ReSTIR frames.  Every ReSTIR frame equals, bit
    for bit, the same calls on a renderer pinned to lockstep walks at depth 0 (both walk kinds give identical frames:
    test_traversal_kinds_bit_identical; the row order only changes dispatch order)."""
    import torch
    from restir_amd.distributed import _CudaBuf
    W, H, n_frames = 96, 64, 12
    sc, prm = scenes.cornell_many_lights(256), P.c3_params(m_area=6)
    assert prm.do_temporal and prm.do_spatial
    cam = lambda f: orbit_cam(sc, f)
    depth_at = {0: 2, 6: 0, 8: 1, 10: 2}
    torch.cuda.set_stream(torch.cuda.Stream())       # the clones below are ordered on the frames' stream
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for run in ("lockstep0", "sequenced"):
        g = Renderer(W, H, stream=st)
        if run == "lockstep0":
            g.set_traversal("lockstep")
            g.set_run_ahead(0)
        gs = g.load_scene(sc)
        frames = []
        for f in range(n_frames):
            if run == "sequenced" and f in depth_at:
                g.set_run_ahead(depth_at[f])
            if f == 5:
                g.render_direct_mis(gs, cam(f), prm, f, spp=1, copy_out=False)
            if f == 7:
                gs.update_positions(scenes.moving_light_positions(sc, f, 48), sc.normals)   # in place, with normals
            elif f not in (0, 3):
                gs.update_positions(scenes.moving_light_positions(sc, f, 48), None)         # pipelined at depth > 0
            g.produce_restir(gs, cam(f), prm, f, copy_out=False, timed=False)
            frames.append(torch.as_tensor(_CudaBuf(g.frame_device_ptr(), W * H * 12, "<f4", 4), device="cuda").clone())
        out[run] = [t.cpu().numpy().reshape(H, W, 3) for t in frames]
        if run == "sequenced":
            assert g.traversal(gs)[2] in (0, 1),"the six tuning frames did not settle the scene's traversal kind"
    for f in range(n_frames):
        assert np.isfinite(out["sequenced"][f]).all() and out["sequenced"][f].any()
        assert np.array_equal(out["lockstep0"][f], out["sequenced"][f]), f"frame {f}"


def test_spatial_reuse_variance_matches_oracle():
    """SURVEY.md §8(c) / north star: spatial-reuse variance -- per-pixel variance over 64 frame indices
    (static camera, temporal off, metric point), averaged over non-emissive pixels -- within [0.95, 1.05]
    of the oracle's."""
    sc = scenes.cornell_many_lights(256)
    W, H, N = 64, 40, 64
    prm = P.metric_params()
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    gpu = np.stack([g.produce_restir(gs, sc.camera, prm, f).copy() for f in range(N)]).astype(np.float64)
    ref = np.stack([o.render(os_, sc.camera, prm, f) for f in range(N)]).astype(np.float64)
    emissive = g.gbuffer()[..., 12:15].max(-1) > 0
    v_gpu = gpu.mean(-1).var(0)[~emissive].mean()
    v_ref = ref.mean(-1).var(0)[~emissive].mean()
    assert 0.95 <= v_gpu / v_ref <= 1.05, (v_gpu, v_ref)


def test_c5_moving_lights_match_oracle():
    """C5 extension: lights moved each frame with rs_scene_update_positions (light CDF + BVH rebuilt)
    under an orbiting camera with temporal + spatial reuse; the oracle renders each frame from a fresh
    scene with the same positions."""
    sc = scenes.cornell_many_lights(256)
    prm = P.c3_params(m_area=8)
    W, H = 64, 48
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    o = O.OracleRenderer(W, H)
    n_before = gs.n_nodes
    for f in range(3):
        pos = scenes.moving_light_positions(sc, 20 * f, 240)
        gs.update_positions(pos)
        cam = scenes.orbit_camera(sc.camera, f, 240, 0.3)
        a = g.produce_restir(gs, cam, prm, f).copy()
        moved = scenes.Scene(pos, sc.normals, sc.tri_material, sc.materials, sc.camera)
        b = o.render(O.OracleScene(moved), cam, prm, f)
        assert_close(a, b, f"C5 frame {f}")
    assert gs.n_nodes > 0 and abs(gs.n_nodes - n_before) < n_before
    with pytest.raises(ValueError):
        gs.update_positions(np.zeros((3, 9), np.float32))


@pytest.mark.parametrize("which", ["c2", "c3"])
def test_update_positions_refit_matches_fresh_scene(which):
    """rs_scene_update_positions (device light CDF + in-place BVH refit, no host sync) renders frames
    bit-identical to a freshly created scene with the same positions -- including a large motion
    (amplitude 0.4: refit boxes grow, answers must not change), the normals path, and an explicit
    rs_scene_rebuild.  BVH queries of the refit tree are bit-identical to a fresh tree's."""
    if which == "c2":
        sc, prm, W, H = scenes.cornell_many_lights(256), P.c3_params(m_area=8), 64, 48
    else:
        sc, prm, W, H = scenes.sponza_like(target_tris=30_000, n_lamps=128), P.c3_params(m_area=8), 64, 40
    g, f_ = Renderer(W, H), Renderer(W, H)
    gs = g.load_scene(sc)
    plan = [(0, 0.05, False), (40, 0.05, True), (90, 0.4, False), (130, 0.4, True)]
    for f, (t, amp, with_normals) in enumerate(plan):
        pos = scenes.moving_light_positions(sc, t, 240, amplitude=amp)
        gs.update_positions(pos, sc.normals if with_normals else None)
        if f == 3:
            gs.rebuild()
        cam = scenes.orbit_camera(sc.camera, f, 240, 0.3)
        a = g.produce_restir(gs, cam, prm, f).copy()
        fresh = f_.load_scene(scenes.Scene(pos, sc.normals, sc.tri_material, sc.materials, sc.camera))
        b = f_.produce_restir(fresh, cam, prm, f).copy()
        assert np.array_equal(a, b), f"frame {f}: refit != fresh ({np.abs(a - b).max()})"
        if f == 2:
            rng = np.random.default_rng(5)
            lo, hi = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
            o = rng.uniform(lo, hi, (4000, 3)).astype(np.float32)
            d = rng.normal(size=(4000, 3)).astype(np.float32)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            for lockstep in (True, False):
                ta, pa = g.debug_trace(gs, o, d, 0.01, 3.0e38, any_hit=False, lockstep=lockstep)
                tb, pb = f_.debug_trace(fresh, o, d, 0.01, 3.0e38, any_hit=False, lockstep=lockstep)
                assert np.array_equal(pa, pb) and np.array_equal(ta, tb)
        fresh.close()


@pytest.mark.parametrize("which", ["c1", "phong"])
def test_direct_mis_matches_oracle(which):
    """§8f-3 MIS direct-light ground truth (rs_render_direct_mis) against or_render_direct_mis on the
    same seeds (frame tolerance: 1/I_M and powf are ocml vs glibc); the two traversal kinds give
    bit-identical frames."""
    if which == "c1":
        sc, prm, W, H, spp = scenes.cornell_box(8), P.default_params(), 64, 48, 4
    else:
        sc, prm, W, H, spp = scenes.sponza_like(target_tris=30_000, n_lamps=128), P.c3_params(), 64, 36, 2
    o, os_ = O.OracleRenderer(W, H), O.OracleScene(sc)
    out = {}
    for mode in ("lockstep", "lane"):
        g = Renderer(W, H)
        g.set_traversal(mode)
        gs = g.load_scene(sc)
        out[mode] = [g.render_direct_mis(gs, sc.camera, prm, f, spp, timed=True).copy() for f in range(2)]
        assert g.last_times.rays >= W * H
    for f in range(2):
        assert np.array_equal(out["lockstep"][f], out["lane"][f])
        assert_close(out["lane"][f], o.render_direct_mis(os_, sc.camera, prm, f, spp), f"MIS {which} frame {f}")


def test_direct_mis_leaves_restir_history_and_converges():
    """A ground-truth launch between two ReSTIR frames does not change the second (temporal) frame;
    ReSTIR's RIS (initial pass, unbiased) accumulated with rs_post_frame converges to the MIS image on
    the C2 scene (surfaces facing the emitters' back faces excluded, see tests/test_oracle.py)."""
    sc = scenes.cornell_many_lights(1024)
    W, H = 96, 54
    prm_t = P.c3_params(m_area=8)
    ref, g = Renderer(W, H), Renderer(W, H)
    rs, gs = ref.load_scene(sc), g.load_scene(sc)
    a0 = ref.produce_restir(rs, sc.camera, prm_t, 0).copy()
    a1 = ref.produce_restir(rs, sc.camera, prm_t, 1).copy()
    b0 = g.produce_restir(gs, sc.camera, prm_t, 0).copy()
    g.render_direct_mis(gs, sc.camera, prm_t, 7, 3)
    b1 = g.produce_restir(gs, sc.camera, prm_t, 1).copy()
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)

    prm = P.metric_params(do_spatial=0)
    gt = g.render_direct_mis(gs, sc.camera, prm, 0, 512).astype(np.float64)
    g.post_reset()
    n = 64
    for f in range(n):
        g.produce_restir(gs, sc.camera, prm, f, copy_out=False)
        _, st = g.post_frame(accumulate=True, tonemap=False, gamma_correct=False, stats=(f == n - 1))
    assert st.acc_frames_used == n - 1           # accFrameCtr the last frame was blended with
    acc = g.display_rgba()[..., :3].astype(np.float64)          # display = accumulator (no tonemap/gamma)
    gb = g.gbuffer()
    mask = (gb[..., 12:15].sum(-1) == 0) & (gb[..., 5] > -0.5) & (gt.sum(-1) > 0)
    assert mask.sum() > 0.4 * W * H
    ratio = acc.sum(-1)[mask].sum() / gt.sum(-1)[mask].sum()
    assert abs(ratio - 1.0) <= 0.02, ratio


def test_post_frame_matches_oracle():
    """rs_post_frame (accumulate + ACES + sRGB + mean/variance) against the oracle's post restatement
    applied to the GPU's own frames: accumulator bit-exact, display within powf ulps, stats 1e-9."""
    sc = scenes.cornell_box(8)
    prm = P.default_params(m_area=4, do_spatial=1, do_temporal=1)
    W, H = 64, 48
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    post = O.OraclePost(W, H)
    for f in range(4):
        frame = g.produce_restir(gs, sc.camera, prm, f).copy()
        _, st = g.post_frame(accumulate=True, tonemap=False, gamma_correct=False)
        disp = g.display_rgba()
        ref_disp, ref = post.apply(frame, accumulate=True, tonemap=False, gamma_correct=False)
        assert st.acc_frames_used == ref["acc_frames_used"] == f
        np.testing.assert_array_equal(disp, ref_disp)                     # display == accumulator
        assert abs(st.mean - ref["mean"]) <= 1e-9 * abs(ref["mean"]) + 1e-12
        assert abs(st.variance - ref["variance"]) <= 1e-9 * abs(ref["variance"]) + 1e-12
    frame = g.produce_restir(gs, sc.camera, prm, 4).copy()
    _, st = g.post_frame(accumulate=True)                                 # tonemap + gamma (defaults)
    ref_disp, ref = post.apply(frame, accumulate=True)
    np.testing.assert_allclose(g.display_rgba(), ref_disp, rtol=0, atol=2e-6)
    g.post_reset()
    _, st = g.post_frame(accumulate=False)
    assert st.acc_frames_used == 0


def test_export_png_and_sidecar(tmp_path):
    """SimpleGuiDX11::exportImage (pg/simpleguidx11.cpp:607-650): the display buffer as RGBA8 with
    (uint8)(v * 255) truncation, and the sidecar's fields (params, mean/variance, camera)."""
    from PIL import Image
    sc, prm = scenes.cornell_box(8), P.default_params(m_area=4, do_spatial=1, spatial_passes=2)
    g = Renderer(48, 32)
    gs = g.load_scene(sc)
    for f in range(3):
        g.produce_restir(gs, sc.camera, prm, f)
        _, st = g.post_frame(accumulate=True)
    disp = g.display_rgba()
    p = tmp_path / "shot.png"
    g.export_png(p, render_time_s=1.25)
    got = np.asarray(Image.open(p))
    want = (disp * np.float32(255.0)).astype(np.uint8)
    assert got.shape == (32, 48, 4) and np.array_equal(got, want)
    txt = open(str(p) + ".txt").read()
    assert f"Image name: {p}" in txt and "Area samples: 4" in txt and "BRDF samples: 1" in txt
    assert "Spatial reuse: True" in txt and "\tPass count: 2" in txt and "Temporal reuse: False" in txt
    assert "Render time: 1.25 s" in txt and "Iteration count: 3" in txt
    mean = float(txt.split("Image mean: ")[1].split()[0])
    assert abs(mean - st.mean) <= 1e-5 * abs(st.mean)
    e = sc.camera.eye
    assert f"Camera position: vec3({e[0]:f}, {e[1]:f}, {e[2]:f})" in txt


def test_timing_totals_match_per_frame_times():
    """rs_get_timing_totals (no per-frame sync) sums the same rays as per-frame timed readback and
    counts every frame, across more frames than the event ring holds."""
    sc, prm = scenes.cornell_many_lights(1024), P.metric_params()
    W, H, n = 64, 48, 70
    a = Renderer(W, H)
    ga = a.load_scene(sc)
    a.set_traversal("lockstep")
    per_frame = 0
    for f in range(n):
        a.produce_restir(ga, sc.camera, prm, f, copy_out=False, timed=True)
        per_frame += int(a.last_times.rays)
    b = Renderer(W, H)
    gb = b.load_scene(sc)
    b.set_traversal("lockstep")
    b.produce_restir(gb, sc.camera, prm, 0, copy_out=False, timed=False)
    _, k = b.timing_totals(reset=True)
    assert k == 1
    for f in range(n):
        b.produce_restir(gb, sc.camera, prm, f, copy_out=False, timed=False)
    tot, k = b.timing_totals()
    assert k == n and int(tot.rays) == per_frame and tot.primary_rays == n * W * H
    assert 0.0 < tot.gbuffer_initial_ms <= tot.total_ms
    tot_a, k_a = a.timing_totals()
    assert k_a == n and int(tot_a.rays) == per_frame


# ---------------------------------------------------------------- edge cases + API behaviour
@pytest.mark.parametrize("wh", [(1, 1), (17, 9), (3, 64)])
def test_odd_sizes(wh):
    sc = scenes.cornell_box(8)
    prm = P.default_params(m_area=3, do_spatial=1, spatial_neighbors=2, do_temporal=1)
    _, _, frames = _pair(sc, wh[0], wh[1], prm, frames=2)
    for a, b in frames:
        assert_close(a, b, f"size {wh}")


def test_no_emitters():
    sc = scenes.cornell_box(8)
    keep = ~sc.emissive_mask()
    sc2 = scenes.Scene(sc.positions[keep], sc.normals[keep], sc.tri_material[keep], sc.materials, sc.camera)
    _, _, frames = _pair(sc2, 32, 32, P.metric_params())
    assert np.array_equal(frames[0][0], frames[0][1])


def test_deterministic_and_reset_history():
    sc = scenes.cornell_box(8)
    prm = P.default_params(m_area=4, do_spatial=1, do_temporal=1)
    g = Renderer(48, 48)
    gs = g.load_scene(sc)
    a0 = g.produce_restir(gs, sc.camera, prm, 0).copy()
    a1 = g.produce_restir(gs, sc.camera, prm, 1).copy()
    g.reset_history()
    b0 = g.produce_restir(gs, sc.camera, prm, 0).copy()
    b1 = g.produce_restir(gs, sc.camera, prm, 1).copy()
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)


def test_invalid_arguments_raise():
    sc = scenes.cornell_box(8)
    g = Renderer(8, 8)
    gs = g.load_scene(sc)
    with pytest.raises(RestirError):
        g.produce_restir(gs, sc.camera, P.default_params(use_skybox=1), 0)
    with pytest.raises(RestirError):
        g.produce_restir(gs, sc.camera, P.default_params(do_spatial=1, spatial_neighbors=65), 0)
    with pytest.raises(RestirError):
        g.load_scene("/nonexistent/file.obj")


def test_obj_loader_matches_array_scene():
    """rs_scene_load_obj (MTL Pc/Kd/Ks/Ke/Ns conventions of pg/ModelLoader.cpp:41-153) yields the same
    frame as the equivalent in-memory scene."""
    sc = scenes.cornell_box(8)
    with tempfile.TemporaryDirectory() as d:
        mtl = os.path.join(d, "s.mtl")
        obj = os.path.join(d, "s.obj")
        with open(mtl, "w") as f:
            for i, m in enumerate(sc.materials):
                # write sRGB-compressed Kd/Ks so the loader's expansion recovers the linear values
                def comp(v):
                    v = np.float32(v)
                    return 0.0 if v <= 0 else (v * 12.92 if v <= 0.0031308 else 1.055 * v ** (1 / 2.4) - 0.055)
                f.write(f"newmtl m{i}\nPc {m.type}\nKd {' '.join(f'{comp(c):.9g}' for c in m.kd)}\n"
                        f"Ks {' '.join(f'{comp(c):.9g}' for c in m.ks)}\nKe {' '.join(f'{c:.9g}' for c in m.le)}\n"
                        f"Ns {m.shininess:.9g}\n")
        with open(obj, "w") as f:
            f.write("mtllib s.mtl\n")
            for t in range(sc.n_tris):
                p, n = sc.positions[t].reshape(3, 3), sc.normals[t].reshape(3, 3)
                for v in p:
                    f.write(f"v {v[0]:.9g} {v[1]:.9g} {v[2]:.9g}\n")
                for v in n:
                    f.write(f"vn {v[0]:.9g} {v[1]:.9g} {v[2]:.9g}\n")
            cur = -1
            for t in range(sc.n_tris):
                if sc.tri_material[t] != cur:
                    cur = sc.tri_material[t]
                    f.write(f"usemtl m{cur}\n")
                b = 3 * t + 1
                f.write(f"f {b}//{b} {b + 1}//{b + 1} {b + 2}//{b + 2}\n")
        g = Renderer(48, 48)
        gs_obj = g.load_scene(obj)
        assert gs_obj.n_tris == sc.n_tris and gs_obj.n_emissive == int(sc.emissive_mask().sum())
        a = g.produce_restir(gs_obj, sc.camera, P.default_params(), 0).copy()
    g2 = Renderer(48, 48)
    b = g2.produce_restir(g2.load_scene(sc), sc.camera, P.default_params(), 0)
    assert_close(a, b, "obj loader")


def test_debug_reprojection_matches_oracle():
    """debugReprojection (pg/ReSTIRIntegrator.cpp:30, :647-689) on a moving camera with temporal + spatial
    reuse: the rejection colours land in the G-buffer emission bit-exactly where the oracle puts them (all
    four kinds occur), and the frames -- shaded from the painted G-buffer -- agree within tolerance.  A
    partial tile refuses the flag (its marks can land on any pixel)."""
    sc = scenes.sponza_like(target_tris=20_000, n_lamps=64)
    prm, prm0 = P.c3_params(m_area=6, debug_reprojection=1), P.c3_params(m_area=6)
    W, H = 96, 64
    cams = [scenes.orbit_camera(sc.camera, 3 * f, 48, 0.6) for f in range(4)]
    g, o, g0 = Renderer(W, H), O.OracleRenderer(W, H), Renderer(W, H)
    gs, os_, gs0 = g.load_scene(sc), O.OracleScene(sc), g0.load_scene(sc)
    colours = {(100.0, 100.0, 0.0), (0.0, 100.0, 0.0), (100.0, 0.0, 100.0), (0.0, 0.0, 100.0)}
    seen = set()
    for f, c in enumerate(cams):
        a = g.produce_restir(gs, c, prm, f).copy()
        b = o.render(os_, c, prm, f)
        le_g, le_o = g.gbuffer()[..., 12:15], o.gbuffer()[..., 12:15]
        assert np.array_equal(le_g, le_o), f"frame {f}: {int(np.any(le_g != le_o, -1).sum())} G emissions differ"
        seen |= {tuple(map(float, v)) for v in le_g.reshape(-1, 3)} & colours
        assert_close(a, b, f"debug_reprojection frame {f}")
        a0 = g0.produce_restir(gs0, c, prm0, f).copy()
        if f > 0:
            assert not np.array_equal(a, a0)          # the flag changes the picture
    assert seen == colours, seen
    with pytest.raises(RestirError):
        g.tile_begin(gs, cams[0], prm, 0, 0, H // 2, 8, 5)


def test_wide_tree_live_on_c3():
    """The C3 scene's 8-wide tree (host SAH tree, SAH-optimal collapse with the depth bound, rs_wide.h) must be
    built and walked: a tree deeper than the walk's stack would silently fall back to the skip-pointer walks
    (same results, 2x slower).  Checks that the wide walk runs (mode 6/7 returns -1 without a wide tree), never
    overflows its stack, and keeps random rays well below a pathological fetch count."""
    sc = scenes.by_name("C3")
    g = Renderer(8, 8)
    gs = g.load_scene(sc)
    rng = np.random.default_rng(5)
    n = 20000
    lo = sc.positions.reshape(-1, 3).min(0)
    hi = sc.positions.reshape(-1, 3).max(0)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for any_hit in (False, True):
        fetches, tris, lost = g.debug_trace(gs, o, d, 0.01, 3.0e38, any_hit=any_hit, wide_stats=True)
        # without a wide tree the debug modes return -1 (0xffff in both 16-bit fields)
        assert ((fetches > 0) & (fetches != 0xFFFF)).all(), "no 8-wide tree on the C3 scene (skip-pointer fallback)"
        assert (lost == 0).all()
        assert fetches.mean() < 100.0       # a broken tree (e.g. boxes opened for every ray) walks far more


@pytest.mark.parametrize("W,H", [(64, 40), (1920, 1080)])
def test_persistent_sorted_pass_bit_identical(W, H, monkeypatch):
    """The sorted initial pass by persistent waves (rs_passes.h k_gbuffer_initial_sorted_pq, RESTIR_PERSIST_SORTED:
    every wave pulls 8x8 tiles from a per-launch counter) renders the one-launch kernel's frames bit for bit --
    at 1080p each resident wave walks several tiles; the ray totals agree too (per-wave counts stored once)."""
    sc = scenes.sponza_like(target_tris=30_000, n_lamps=128)
    prm = P.c3_params(m_area=32)
    cam = lambda f: scenes.orbit_camera(sc.camera, f, 240, 0.3)   # noqa: E731
    out = {}
    for mode in ("on", "off"):
        monkeypatch.setenv("RESTIR_PERSIST_SORTED", mode)
        g = Renderer(W, H)
        g.set_traversal("lane")
        gs = g.load_scene(sc)
        fr = [g.produce_restir(gs, cam(f), prm, f, timed=True).copy() for f in range(3)]
        out[mode] = (fr, int(g.last_times.rays), g.reservoirs().copy())
        if mode == "on" and (W, H) == (1920, 1080):
            # the hand-off buffers are per resident wave of the persistent launch, not per tile of the frame
            # (round 5: ~0.67 GB per lane at 1080p): <= 0.2 GB over every lane
            hb = g.handoff_bytes()
            print(f"[handoff] 1080p persistent sorted pass: {hb / 1e6:.1f} MB")
            assert 0 < hb <= 200e6, hb
        gs.close()
        g.close()
    for f, (a, b) in enumerate(zip(out["on"][0], out["off"][0])):
        assert np.array_equal(a, b), f"frame {f}: persistent sorted pass != one-launch"
    assert out["on"][1] == out["off"][1]
    assert np.array_equal(out["on"][2], out["off"][2])


@pytest.mark.parametrize("which", ["c3", "c3_a37", "c2_lane", "c2_lockstep"])
def test_sorted_initial_pass_bit_identical(which, monkeypatch):
    """The wave-sorted initial, temporal and spatial passes (rs_passes.h k_gbuffer_initial_sorted, k_temporal<T |
    TEMPORAL_SORT>, k_spatial_sorted: per 8x8 tile the shadow rays are counting-sorted by octant x light bucket /
    target cell and traced in that order) render the frames of the per-candidate kernels bit for bit
    (RESTIR_SORT=off, RESTIR_SORT_SPATIAL=off, RESTIR_SORT_TEMPORAL=off), incl. a
    candidate count that is not a multiple of the chunk, a visibility-pass frame (no shadow rays in the initial
    pass), and both walk kinds on the metric scene."""
    trav = "lockstep" if which == "c2_lockstep" else "lane"
    if which.startswith("c2"):
        sc, prm, W, H = scenes.cornell_many_lights(1024), P.metric_params(), 64, 48
    else:
        sc, W, H = scenes.sponza_like(target_tris=30_000, n_lamps=128), 64, 40
        prm = P.c3_params(m_area=37 if which == "c3_a37" else 32)
    cam = lambda f: scenes.orbit_camera(sc.camera, f, 240, 0.3)
    out = {}
    for sort in ("on", "off"):
        monkeypatch.setenv("RESTIR_SORT", sort)
        monkeypatch.setenv("RESTIR_SORT_SPATIAL", sort)
        monkeypatch.setenv("RESTIR_SORT_TEMPORAL", sort)
        g = Renderer(W, H)
        g.set_traversal(trav)
        gs = g.load_scene(sc)
        fr = [g.produce_restir(gs, cam(f), prm, f, timed=True).copy() for f in range(3)]
        rays = int(g.last_times.rays)
        vis = P.c3_params(m_area=8, do_visibility_pass=1)
        fr.append(g.produce_restir(gs, cam(3), vis, 3).copy())
        out[sort] = (fr, rays, g.reservoirs().copy())
    for f, (a, b) in enumerate(zip(out["on"][0], out["off"][0])):
        assert np.array_equal(a, b), f"{which} frame {f}: sorted != per-candidate"
    assert out["on"][1] == out["off"][1]                # the same rays traced
    assert np.array_equal(out["on"][2], out["off"][2])
