"""The one-thread-per-pixel initial pass with the light tables in LDS (rs_passes.h LIGHT_LDS, restir_capi.hip
use_light_lds) against the same pass reading them from global memory (RESTIR_LIGHT_LDS=off).

The LDS copy holds the same CDF and guide values and light_index makes the same comparisons on them, so every
frame and every reservoir must be bit-identical: the comparisons below are on the raw 32-bit words.  The switch is
read when a context is created, so every renderer is made after the environment is set.  The walks are pinned to
lockstep: AUTO's first frames alternate the walk kind to time it, and per-lane frames take the sorted pass, which
keeps the global tables.  The candidate-split pass is switched off for the same reason (_pinned), and every renderer
asserts after its frames that the one-thread-per-pixel lockstep kernel is what ran.
"""
import numpy as np
import pytest

import gpu_harness as GH
import oracle_lib as O
from restir_amd import params as P
from restir_amd import scenes

pytestmark = pytest.mark.gpu

def _pinned(monkeypatch, mode, W, H, **kw):
    """A renderer created under RESTIR_LIGHT_LDS=mode for the launch the variant belongs to: lockstep walks, and the
    candidate-split pass off -- AUTO runs these small frames (less than one round of the device's waves) through
    k_gbuffer_initial_split, which keeps the global tables."""
    GH.set_env(monkeypatch, RESTIR_LIGHT_LDS=mode)
    return GH.pinned_renderer(W, H, "lockstep", **kw)


def _render(monkeypatch, mode, sc, W, H, prm, frames=1):
    """(frames, reservoirs after the last frame, emissive triangles) of a renderer created under RESTIR_LIGHT_LDS=mode"""
    g = _pinned(monkeypatch, mode, W, H)
    gs = g.load_scene(sc)
    out = [g.produce_restir(gs, sc.camera, prm, f).copy() for f in range(frames)]
    GH.assert_walked(g, "lockstep")      # else the LDS kernel was not launched
    res = g.reservoirs()
    n = gs.n_emissive
    gs.close()
    g.close()
    return out, res, n


def _off_vs_auto(monkeypatch, sc, W, H, prm, what, frames=1):
    a, ra, n = _render(monkeypatch, "off", sc, W, H, prm, frames)
    b, rb, _ = _render(monkeypatch, "auto", sc, W, H, prm, frames)
    for f in range(frames):
        GH.assert_same_bits(a[f], b[f], f"{what} frame {f}")
    GH.assert_same_bits(ra, rb, f"{what} reservoirs")
    return b, n


def _light_scene(tris):
    """The Cornell shell with the given emissive triangles ((T, 9) positions, facing down) of one material."""
    b = scenes._Builder()
    scenes._cornell_shell(b)
    tris = np.asarray(tris, np.float32).reshape(-1, 9)
    if len(tris):
        light = b.material(scenes.Material(le=(17.0, 12.0, 4.0), type=scenes.LAMBERT))
        b.tris(tris, np.tile(np.array([0, 0, -1], np.float32), (len(tris), 3)), light)
    return b.build(scenes.CORNELL_CAMERA, "light_lds")


@pytest.mark.parametrize("which", ["initial", "metric"])
def test_table_full_to_capacity(monkeypatch, which):
    """2048 emissive triangles: every word of the LDS CDF is a table entry, and guide entries reach 2047."""
    sc = scenes.cornell_many_lights(1024)
    prm = P.default_params(m_area=32, m_brdf=1) if which == "initial" else P.metric_params()
    frames, n = _off_vs_auto(monkeypatch, sc, 64, 64, prm, which)
    assert n == 2048
    ref = O.OracleRenderer(64, 64).render(O.OracleScene(sc), sc.camera, prm, 0)
    GH.assert_close(frames[0], ref, f"{which} vs oracle")


def test_just_over_capacity(monkeypatch):
    """2050 emissive triangles do not fit the LDS arrays: the launch rule must fall back to the global-table kernel
    (the LDS kernel would copy and search only the first 2048 entries).  The context does not report which kernel
    it launched, so the check is that the frames equal the switched-off renderer's."""
    sc = scenes.cornell_many_lights(1025)
    _, n = _off_vs_auto(monkeypatch, sc, 64, 64, P.metric_params(), "1025 lights")
    assert n == 2050


@pytest.mark.parametrize("which", ["one_quad", "zero_area", "no_lights"])
def test_degenerate_tables(monkeypatch, which):
    z = 1.98
    a = [-0.3, -0.3, z, -0.3, 0.3, z, 0.3, 0.3, z]
    c = [-0.3, -0.3, z, 0.3, 0.3, z, 0.3, -0.3, z]
    if which == "one_quad":          # 2 CDF entries: most guide entries are equal
        sc, n_want = _light_scene([a, c]), 2
    elif which == "zero_area":       # a zero-area triangle between two others: equal adjacent CDF entries (ties)
        sc, n_want = _light_scene([a, [0.5, 0.5, z] * 3, c]), 3
    else:                            # no emitter: the wave-uniform exit of the candidate loops
        sc, n_want = _light_scene([]), 0
    _, n = _off_vs_auto(monkeypatch, sc, 64, 64, P.default_params(m_area=8, m_brdf=1), which)
    assert n == n_want


def test_partial_tile_frame(monkeypatch):
    """50x38 is no multiple of the 16x16 workgroup tile: lanes clamped into the image take part in the copy and
    the barrier, and store nothing."""
    sc = scenes.cornell_many_lights(300)         # 600 entries: a partly filled table with a padded tail
    _off_vs_auto(monkeypatch, sc, 50, 38, P.metric_params(), "50x38")


def test_moving_lights_run_ahead(monkeypatch):
    """C5's pipelined updates: the lights move before every frame with two frames in flight, so a frame's
    workgroups copy the tables of the scene copy that frame was enqueued with while the next update writes the
    other one."""
    import torch
    from restir_amd.distributed import _CudaBuf
    W, H, n_frames = 64, 64, 4
    sc, prm = scenes.cornell_many_lights(256), P.c3_params(m_area=8)
    torch.cuda.set_stream(torch.cuda.Stream())       # the clones below are ordered on the frames' stream
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for mode in ("off", "auto"):
        g = _pinned(monkeypatch, mode, W, H, run_ahead=2, stream=st)
        gs = g.load_scene(sc)
        frames = []
        for f in range(n_frames):
            gs.update_positions(scenes.moving_light_positions(sc, f, 48))
            g.produce_restir(gs, GH.orbit_cam(sc, f), prm, f, copy_out=False, timed=False)
            frames.append(torch.as_tensor(_CudaBuf(g.frame_device_ptr(), W * H * 12, "<f4", 4), device="cuda").clone())
        GH.assert_walked(g, "lockstep")      # else the LDS kernel was not launched
        out[mode] = [t.cpu().numpy().reshape(H, W, 3) for t in frames], g.reservoirs()
        gs.close()
        g.close()
    for f in range(n_frames):
        GH.assert_same_bits(out["off"][0][f], out["auto"][0][f], f"moving lights frame {f}")
    GH.assert_same_bits(out["off"][1], out["auto"][1], "moving lights reservoirs")
