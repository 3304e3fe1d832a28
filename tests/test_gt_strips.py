"""CPU tests of the multi-rank ground truths' orchestration: the strip rule and the strip gather plan of
restir-embree_amd/csrc/rs_mgpu_core.h (tests/cpp/mgpu_strips_harness.cpp) against restir_amd.distributed.strip_rows_of,
and TiledRenderer.render_path / render_direct_mis over gloo with the path oracle as every rank's renderer: the frame
gathered on rank 0 equals the oracle's full frame bit for bit."""
import ctypes
import os
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mgpu_strips_harness.cpp")

HEIGHTS = [1, 15, 16, 17, 36, 40, 52, 1080, 2160]
WORLDS = list(range(1, 9))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("strips") / "libmgpu_strips_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.strips_of.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    L.strip_plan_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong),
                                   ctypes.c_char_p, ctypes.c_int]
    return L


def _native_strips(L, H, world, r):
    cap = H // 16 + 2
    buf = (ctypes.c_int32 * (2 * cap))()
    n = L.strips_of(H, world, r, buf, cap)
    assert 0 <= n <= cap
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


@pytest.mark.parametrize("H", HEIGHTS)
def test_strip_rule_covers_every_row_once_and_matches_python(harness, H):
    from restir_amd.distributed import strip_rows_of
    for world in WORLDS:
        owner = np.full(H, -1)
        for r in range(world):
            strips = _native_strips(harness, H, world, r)
            assert strips == strip_rows_of(H, r, world), (H, world, r)
            assert strips == sorted(strips)
            for a, b in strips:
                assert 0 <= a < b <= H and a % 16 == 0 and b - a <= 16 and (a // 16) % world == r
                assert (owner[a:b] == -1).all(), (H, world, r, a, b)
                owner[a:b] = r
        assert (owner >= 0).all(), (H, world)


@pytest.mark.parametrize("H", HEIGHTS)
def test_strip_gather_plans(harness, H):
    from restir_amd.distributed import strip_rows_of
    row_bytes = 40 * 12
    for world in WORLDS:
        recv0 = ctypes.c_ulonglong()
        msg = ctypes.create_string_buffer(512)
        rc = harness.strip_plan_check(world, H, row_bytes, ctypes.byref(recv0), msg, 512)
        assert msg.value == b"" and rc == 0, (H, world, rc, msg.value)
        own0 = sum(b - a for a, b in strip_rows_of(H, 0, world))
        assert recv0.value == (H - own0) * row_bytes, (H, world)


def test_strip_loads(harness):
    """The row counts behind the design: 8 ranks at 1080 rows hold between 128 and 144 rows, and with more ranks than
    strips (40 rows: 3 strips) the ranks beyond own nothing."""
    rows = [sum(b - a for a, b in _native_strips(harness, 1080, 8, r)) for r in range(8)]
    assert max(rows) == 144 and min(rows) == 128 and sum(rows) == 1080, rows
    rows = [sum(b - a for a, b in _native_strips(harness, 2160, 8, r)) for r in range(8)]
    assert max(rows) == 272 and min(rows) == 256, rows
    assert [_native_strips(harness, 40, 4, r) for r in range(4)] == [[(0, 16)], [(16, 32)], [(32, 40)], []]
    assert [len(_native_strips(harness, 40, 8, r)) for r in range(8)] == [1, 1, 1, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------- gloo orchestration
W, H, SPP, BOUNCES, FRAMES = 40, 36, 2, 3, (0, 1)
KINDS = ["path", "unbiased", "mis"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_frame(orend, oscene, camera, params, frame_index, spp, path_kwargs):
    import path_oracle
    if path_kwargs is None:                        # the direct-light ground truth: the recursion with GI off
        return path_oracle.render_path(orend, oscene, camera, params, frame_index, spp, calc_gi=False)
    return path_oracle.render_path(orend, oscene, camera, params, frame_index, spp, **path_kwargs)


class OracleStripBackend:
    """Every rank renders the oracle's full frame and hands back only its rows: every row outside the set is NaN,
    so a strip sent from or received at the wrong place cannot go unnoticed."""

    def __init__(self, W, H):
        import oracle_lib as O
        self.W, self.H = W, H
        self.r = O.OracleRenderer(W, H)

    def run_ahead_lanes(self):
        return 1

    def load_scene(self, scene):
        import oracle_lib as O
        return O.OracleScene(scene)

    def render_ground_truth_rows(self, scene, camera, params, frame_index, spp, path_kwargs, rows):
        import torch
        strip, stride, phase = rows
        img = _oracle_frame(self.r, scene, camera, params, frame_index, spp, path_kwargs).copy()
        y = np.arange(self.H)
        img[(y // strip) % stride != phase] = np.nan
        return torch.from_numpy(img.reshape(-1))


def _render(tr, s, cam, prm, kind, f):
    if kind == "mis":
        return tr.render_direct_mis(s, cam, prm, f, spp=SPP)
    return tr.render_path(s, cam, prm, f, spp=SPP, max_bounces=BOUNCES, unbiased=kind == "unbiased")


def _worker(rank, world, port, out_path):
    import sys
    sys.path[:0] = [os.path.join(ROOT, "restir-embree_amd"), os.path.join(ROOT, "tests")]
    import torch.distributed as dist
    import oracle_lib as O
    from restir_amd import params as P, scenes
    from restir_amd.distributed import TiledRenderer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    O.lib().or_set_num_threads(2)
    sc, prm = scenes.cornell_box(8), P.default_params()
    tr = TiledRenderer(W, H, rank, world, backend=OracleStripBackend(W, H))
    s = tr.load_scene(sc)
    frames = []
    for kind in KINDS:
        for f in FRAMES:
            fr = _render(tr, s, sc.camera, prm, kind, f)
            if rank == 0:
                frames.append(fr.numpy().copy())
            else:
                assert fr is None
    if rank == 0:
        np.save(out_path, np.stack(frames))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def oracle_full_frames():
    import oracle_lib as O
    from restir_amd import params as P, scenes
    sc, prm = scenes.cornell_box(8), P.default_params()
    r, s = O.OracleRenderer(W, H), O.OracleScene(sc)
    kw = {"path": dict(max_bounces=BOUNCES, russian_roulette=True, calc_di=True, calc_gi=True, unbiased=False),
          "unbiased": dict(max_bounces=BOUNCES, russian_roulette=True, calc_di=True, calc_gi=True, unbiased=True),
          "mis": None}
    return np.stack([_oracle_frame(r, s, sc.camera, prm, f, SPP, kw[kind]) for kind in KINDS for f in FRAMES])


@pytest.mark.parametrize("world", [2, 3])
def test_tiled_ground_truths_match_full_frame(world, tmp_path, oracle_full_frames):
    """40 x 36: strips of 16, 16 and 4 rows.  World 2 gives rank 0 two strips around rank 1's; world 3 one each."""
    out = str(tmp_path / "frames.npy")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    got = np.load(out)
    ref = oracle_full_frames
    assert got.shape == ref.shape and np.isfinite(ref).all()
    assert len({ref[i].tobytes() for i in range(len(ref))}) == len(ref)     # six different frames
    for i, (kind, f) in enumerate((k, f) for k in KINDS for f in FRAMES):
        bad = int(np.any(got[i] != ref[i], -1).sum())
        assert np.array_equal(got[i], ref[i]), f"world {world} {kind} frame {f}: {bad} pixels differ"
