"""The frame harness of the GPU tests: the comparisons, the pinned renders and the shared scenes that every
tests/test_gpu_*.py used to carry a copy of.  TEST INFRASTRUCTURE ONLY.  Imports without a GPU (collection on a
CPU-only machine); a Renderer is created inside functions only.

Three kinds of comparison, and a call site keeps the kind it has:
  assert_close         the project's frame bound: >= PIX_FRAC of the pixels within PIX_TOL (relative L2) and the mean
                       relative L2 <= MEAN_TOL -- for frames that pass through the device's own libm
  assert_equal_finite  a is finite, then np.array_equal(a, b): -0.0 equals +0.0
  assert_same_bits     the 32-bit words are equal: -0.0 differs from +0.0, a NaN equals the same NaN
  assert_same_render   frames by np.array_equal; G-buffer and reservoirs element by element with NaN equal to NaN

Pinned renders: AUTO times the walk kinds on its first frames and runs small frames through the candidate-split
pass, so a test of one kernel pins the walk kind and the split (pinned_renderer) and asserts afterwards that this is
what ran (assert_walked).  gpu_frames / oracle_frames render a sequence on the orbit camera of the walk tests;
check_walks_against_oracle is the lockstep == per-lane == oracle comparison.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from restir_amd import scenes

# ---------------------------------------------------------------- comparisons
PIX_TOL, PIX_FRAC, MEAN_TOL = 1e-4, 0.995, 1e-4          # the project's frame bound
TYPE_COL = 17                                            # the G-buffer's material-type column


def frame_stats(gpu, ref):
    """(share of pixels within PIX_TOL, mean, max) of the per-pixel relative L2 error"""
    diff = np.linalg.norm(gpu.astype(np.float64) - ref, axis=-1)
    rel = diff / np.maximum(np.linalg.norm(ref.astype(np.float64), axis=-1), 1e-3)
    return float((rel <= PIX_TOL).mean()), float(rel.mean()), float(rel.max())


def assert_close(gpu, ref, what, tag=None):
    """gpu is finite and within the frame bound of ref; with a tag the statistics are printed (-s)"""
    assert np.isfinite(gpu).all(), what
    frac, mean, mx = frame_stats(gpu, ref)
    if tag:
        print(f"[{tag}] {what}: {int((gpu != ref).any(axis=-1).sum())} of {gpu.shape[0] * gpu.shape[1]} pixels not "
              f"bit-identical, frac_ok={frac:.5f} mean_rel={mean:.3g} max_rel={mx:.3g}", flush=True)
    assert frac >= PIX_FRAC and mean <= MEAN_TOL, f"{what}: frac_ok={frac:.5f} mean_rel={mean:.3g} max_rel={mx:.3g}"


def bits(a):
    """float32 viewed as uint32 (a float16 array as uint16)"""
    if np.asarray(a).dtype == np.float16:
        return np.ascontiguousarray(a).view(np.uint16)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(a, b, what):
    """the words of a and b are equal; the message counts the pixels / rows (last axis folded) that are not"""
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, what
    d = a != b
    if d.ndim > 1:
        d = d.any(-1)
    assert not d.any(), f"{what}: {int(d.sum())} of {d.size} differ, first at {np.argwhere(d)[:4].tolist()}"


def assert_equal_finite(a, b, what):
    assert np.isfinite(a).all(), what
    assert np.array_equal(a, b), f"{what}: {int(np.any(a != b, -1).sum())} px differ"


class Render:
    """frames (list of (H, W, 3)), the G-buffer and the reservoirs after the last frame; read-only"""

    def __init__(self, frames, gbuffer, reservoirs):
        self.frames, self.gbuffer, self.reservoirs = frames, gbuffer, reservoirs
        for a in (*frames, gbuffer, reservoirs):
            a.setflags(write=False)


def run_restir(renderer, handle, sc, n_frames, frame_fn, camera):
    """n_frames over camera(sc, f) on either renderer; frame_fn(handle, camera, f) renders one frame"""
    renderer.reset_history()
    frames = [np.array(frame_fn(handle, camera(sc, f), f), copy=True) for f in range(n_frames)]
    return Render(frames, np.array(renderer.gbuffer(), copy=True), np.array(renderer.reservoirs(), copy=True))


def oracle_restir(sc, prm, size, n_frames, camera):
    import oracle_lib as O
    o, os_ = O.OracleRenderer(*size), O.OracleScene(sc)
    return run_restir(o, os_, sc, n_frames, lambda h, c, f: o.render(h, c, prm, f), camera)


def gpu_restir(sc, prm, size, n_frames, traversal=None, split=None, *, camera):
    from restir_amd.renderer import Renderer
    g = Renderer(*size)
    if traversal:
        g.set_traversal(traversal)
    if split:
        g.set_initial_split(split)
    gs = g.load_scene(sc)
    return run_restir(g, gs, sc, n_frames, lambda h, c, f: g.produce_restir(h, c, prm, f), camera)


def same(a, b):
    """every element equal, or NaN on both sides"""
    return np.array_equal(a, b, equal_nan=True)


def _differ(a, b):
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def assert_same_render(a, b, what, type_column=True):
    """frames, G-buffer (without the type column if asked) and reservoirs equal element by element; the message
    names every part that is not"""
    bad = []
    for f, (x, y) in enumerate(zip(a.frames, b.frames)):
        if not np.array_equal(x, y):
            bad.append(f"frame {f}: {int(np.any(x != y, -1).sum())} pixels")
    ga, gb = a.gbuffer, b.gbuffer
    if not type_column:
        keep = [c for c in range(ga.shape[-1]) if c != TYPE_COL]
        ga, gb = ga[..., keep], gb[..., keep]
    if not same(ga, gb):
        d = _differ(ga, gb)
        bad.append(f"G-buffer: columns {sorted(set(np.nonzero(d)[-1].tolist()))} on {int(d.any(-1).sum())} pixels")
    if not same(a.reservoirs, b.reservoirs):
        d = _differ(a.reservoirs, b.reservoirs)
        bad.append(f"reservoirs: columns {sorted(set(np.nonzero(d)[-1].tolist()))} on {int(d.any(-1).sum())} pixels")
    assert not bad, f"{what}: " + "; ".join(bad)


# ---------------------------------------------------------------- pinned renders
KIND = {"lockstep": 0, "lane": 1}                        # TRAV_LOCKSTEP, TRAV_LANE: what Renderer.traversal() reports
WALKS = ["lane", "lockstep"]


def orbit_cam(sc, f):
    """the walk tests' orbit: 48 steps, radius 0.2"""
    return scenes.orbit_camera(sc.camera, f, 48, 0.2)


def set_env(monkeypatch, **variables):
    """set each variable under monkeypatch; None deletes it"""
    for k, v in variables.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def pinned_renderer(W, H, walk, split="off", run_ahead=None, stream=None):
    from restir_amd.renderer import Renderer
    g = Renderer(W, H, stream=stream)
    g.set_traversal(walk)
    g.set_initial_split(split)
    if run_ahead is not None:
        g.set_run_ahead(run_ahead)
    return g


def assert_walked(g, walk, split="off"):
    """the last frame walked as pinned, and its initial pass ran candidate-split exactly when pinned on"""
    assert g.traversal()[1] == KIND[walk], "the last frame did not walk as pinned"
    assert g.initial_split()[1] is (split == "on"), "the last frame's initial pass: split state not as pinned"


Frames = namedtuple("Frames", "frames res rays gb")      # rays: one count per frame; gb: None unless asked for


def render_frames(g, gs, sc, prms, walk, split="off", every_frame=False, gbuffer=False, camera=orbit_cam):
    """frame f of prms[f] on camera(sc, f) with a pinned renderer and its scene handle; assert_walked after every
    frame or after the last"""
    frames, rays = [], []
    for f, prm in enumerate(prms):
        frames.append(g.produce_restir(gs, camera(sc, f), prm, f).copy())
        rays.append(int(g.last_times.rays))
        if every_frame:
            assert_walked(g, walk, split)
    if not every_frame:
        assert_walked(g, walk, split)
    return Frames(frames, g.reservoirs(), rays, g.gbuffer() if gbuffer else None)


def gpu_frames(sc, W, H, prms, walk, split="off", **kw):
    """render_frames on a renderer and a scene handle of its own, both closed afterwards"""
    g = pinned_renderer(W, H, walk, split)
    gs = g.load_scene(sc)
    out = render_frames(g, gs, sc, prms, walk, split, **kw)
    gs.close()
    g.close()
    return out


def oracle_frames(sc, osc, W, H, prms, gbuffer=False, camera=orbit_cam):
    import oracle_lib as O
    o = O.OracleRenderer(W, H)
    frames, rays = [], []
    for f, prm in enumerate(prms):
        frames.append(o.render(osc, camera(sc, f), prm, f))
        rays.append(o.rays)
    return Frames(frames, o.reservoirs(), rays, o.gbuffer() if gbuffer else None)


def check_walks_against_oracle(sc, osc, W, H, prm, what, n_frames):
    """n_frames of prm: frames and reservoirs of the lockstep kernels equal the per-lane walks' and the oracle's, the
    ray counts of the two walk kinds are equal -> (rays of the lockstep kernels, rays of the oracle)"""
    prms = [prm] * n_frames
    a = gpu_frames(sc, W, H, prms, "lockstep")
    b = gpu_frames(sc, W, H, prms, "lane")
    o = oracle_frames(sc, osc, W, H, prms)
    for f in range(n_frames):
        assert_equal_finite(a.frames[f], b.frames[f], f"{what} frame {f}, lockstep vs per-lane")
        assert_equal_finite(a.frames[f], o.frames[f], f"{what} frame {f}, lockstep vs oracle")
    assert_equal_finite(a.res, b.res, f"{what} reservoirs, lockstep vs per-lane")
    assert_equal_finite(a.res, o.res, f"{what} reservoirs, lockstep vs oracle")
    na, nb = sum(a.rays), sum(b.rays)
    assert na == nb and na > 0, f"{what}: {na} rays in lockstep, {nb} per lane"
    return na, sum(o.rays)


def with_ceiling_blocker(sc, name):
    """sc with a quad under the ceiling lights (z = 1.98, +-0.97), facing down, of one more white material: every
    ceiling-bound shadow ray ends in its first leaf while the wall-bound rays of the same wave go on"""
    z = 1.98
    p = np.array([[-0.97, -0.97, z, -0.97, 0.97, z, 0.97, 0.97, z],
                  [-0.97, -0.97, z, 0.97, 0.97, z, 0.97, -0.97, z]], np.float32)
    n = np.tile(np.array([0, 0, -1], np.float32), (2, 3))
    mats = list(sc.materials) + [scenes.Material(kd=(0.73, 0.73, 0.73), type=scenes.LAMBERT, shininess=1.0)]
    return scenes.Scene(positions=np.concatenate([sc.positions, p]), normals=np.concatenate([sc.normals, n]),
                        tri_material=np.concatenate([sc.tri_material, np.full(2, len(mats) - 1, np.uint32)]),
                        materials=mats, camera=sc.camera, name=name)


# ---------------------------------------------------------------- tiles
def emulate_tiles(sc, W, H, prm, n_ranks, cams, margin):
    """the frames of n_ranks contexts on one device playing n_ranks ranks: every band through the tile stages, the halo
    rows moved device to device through the tensor views the RCCL exchange uses"""
    import torch
    from restir_amd.distributed import GpuTileBackend, band_rows, halo_rows
    from restir_amd.renderer import Renderer
    torch.cuda.set_stream(torch.cuda.Stream())      # a real (non-null) stream shared with the contexts
    st = torch.cuda.current_stream().cuda_stream
    bes = [GpuTileBackend(Renderer(W, H, stream=st)) for _ in range(n_ranks)]
    hs = [be.load_scene(sc) for be in bes]
    h = halo_rows(prm)
    out = []
    for f, cam in enumerate(cams):
        for r, be in enumerate(bes):
            y0, y1 = band_rows(H, r, n_ranks)
            be.begin(hs[r], cam, prm, f, y0, y1, max(margin, h), h)
        for be in bes:
            be.temporal()
        if prm.do_spatial:
            for p in range(prm.spatial_passes):
                torch.cuda.synchronize()
                for r, be in enumerate(bes):
                    if h == 0:                      # a radius below 1: no neighbour leaves its pixel, no halo rows
                        assert all(be.halo_tensor(i) is None for i in range(4))
                        continue
                    if r > 0:
                        be.halo_tensor(0).copy_(bes[r - 1].halo_tensor(3))
                    if r < n_ranks - 1:
                        be.halo_tensor(1).copy_(bes[r + 1].halo_tensor(2))
                torch.cuda.synchronize()
                for be in bes:
                    be.spatial(p)
        bands = [be.finish().cpu().numpy().reshape(-1, W, 3) for be in bes]
        out.append(np.concatenate(bands, 0))
    return out
