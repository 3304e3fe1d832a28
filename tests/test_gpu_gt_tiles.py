"""GPU test of TiledRenderer.render_path / render_direct_mis over GpuTileBackend: three real processes (one HIP context
each on the same GPU), every rank rendering its strips through Renderer.render_path(rows=...), the strips gathered over
gloo (staged through host memory, as tests/test_gpu_tiles.py does: RCCL refuses two ranks on one device).  The frame
on rank 0 equals one Renderer's bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 72, 52, 2, 3
KINDS = ["path", "unbiased", "mis"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _render(r, s, cam, prm, kind, f):
    if kind == "mis":
        return r.render_direct_mis(s, cam, prm, f, spp=SPP)
    return r.render_path(s, cam, prm, f, spp=SPP, max_bounces=BOUNCES, unbiased=kind == "unbiased")


def _gpu_worker(rank, world, port, out_path):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "restir-embree_amd"), os.path.join(root, "tests")]
    import torch
    import torch.distributed as dist
    from restir_amd import params as P, scenes
    from restir_amd.distributed import TiledRenderer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    sc, prm = scenes.cornell_many_lights(64), P.default_params()
    tr = TiledRenderer(W, H, rank, world, device=0)
    s = tr.load_scene(sc)
    frames = []
    for f, kind in enumerate(KINDS):
        fr = _render(tr, s, sc.camera, prm, kind, f)
        if rank == 0:
            frames.append(fr.cpu().numpy().copy())
    if rank == 0:
        np.save(out_path, np.stack(frames))
    dist.barrier()
    dist.destroy_process_group()


def test_multiprocess_ground_truth_strips_on_gpu(tmp_path):
    from restir_amd import params as P, scenes
    from restir_amd.renderer import Renderer
    world = 3
    out = str(tmp_path / "frames.npy")
    mp.spawn(_gpu_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    got = np.load(out)
    sc, prm = scenes.cornell_many_lights(64), P.default_params()
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    for f, kind in enumerate(KINDS):
        ref = _render(g, gs, sc.camera, prm, kind, f).copy()
        bad = int(np.any(got[f] != ref, -1).sum())
        assert np.array_equal(got[f], ref), f"{kind}: {bad} pixels differ"
