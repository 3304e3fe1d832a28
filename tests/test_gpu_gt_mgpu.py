"""GPU tests of the ground truths across ranks (rs_mgpu_render_ground_truth, MultiGpuFrame.render_path /
render_direct_mis): every rank renders its interleaved 16-row strips, the strips gathered on rank 0 equal one
context's frame bit for bit, and rs_post_frame there accumulates all rows.

On the one-GPU test box the ranks are contexts of one process (device copies); the RCCL branch runs against the
stand-in librccl with the ranks as threads (tests/cpp/mgpu_gt_rccl_driver.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

from restir_amd import params as P
from restir_amd import scenes
from restir_amd.distributed import strip_rows_of
from restir_amd.mgpu import MultiGpuFrame
from restir_amd.renderer import Renderer, RestirError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 72
ESTIMATORS = ["mis", "path", "unbiased"]
CASES = {"cornell": dict(spp=3, max_bounces=8), "sponza": dict(spp=2, max_bounces=5)}
MAX_WORLD = 4


def _scene(which):
    return scenes.cornell_box(8) if which == "cornell" else scenes.sponza_like(target_tris=30_000, n_lamps=128)


def _ground_truth(r, s, cam, prm, est, frame, case, **kw):
    """Renderer or MultiGpuFrame: the same three calls"""
    if est == "mis":
        return r.render_direct_mis(s, cam, prm, frame, case["spp"], **kw)
    return r.render_path(s, cam, prm, frame, case["spp"], max_bounces=case["max_bounces"], unbiased=est == "unbiased", **kw)


def _renderers(sc, H, n):
    rs = [Renderer(W, H) for _ in range(n)]
    for r in rs:
        r.set_traversal("lockstep")               # ReSTIR frames on the run-ahead lanes (no AUTO tuning frames)
    return rs, [r.load_scene(sc) for r in rs]


@pytest.mark.parametrize("H", [52, 40])
@pytest.mark.parametrize("which", list(CASES))
def test_local_ranks_gather_one_contexts_frame(which, H):
    """World 2, 3 and 4 over the same contexts (4 ranks at 40 rows: a rank without rows).  Around the ground truths a
    ReSTIR frame before and one after still equal one context's frames 0 and 1: history and bands are untouched."""
    sc, case = _scene(which), CASES[which]
    gt_prm, prm = P.default_params(), P.metric_params(m_area=4)
    cam = sc.camera
    (one,), (ones,) = _renderers(sc, H, 1)
    ref = {est: _ground_truth(one, ones, cam, gt_prm, est, 1, case).copy() for est in ESTIMATORS}
    assert len({v.tobytes() for v in ref.values()}) == 3
    restir = [one.produce_restir(ones, cam, prm, f).copy() for f in range(2)]
    rs, ss = _renderers(sc, H, MAX_WORLD)
    for world in (2, 3, 4):
        m = MultiGpuFrame(rs[:world])
        m.reset_history()
        bands = m.bands()
        img = m.render(ss[:world], cam, prm, 0, copy_out=True)
        assert np.array_equal(img, restir[0]), f"world {world}: the ReSTIR frame before"
        foreign = (H - sum(b - a for a, b in strip_rows_of(H, 0, world))) * W * 12
        for est in ESTIMATORS:
            before = m.stats()["gather_bytes"]
            img = _ground_truth(m, ss[:world], cam, gt_prm, est, 1, case, copy_out=True)
            bad = int(np.any(img != ref[est], -1).sum())
            assert np.array_equal(img, ref[est]), f"{which} H {H} world {world} {est}: {bad} pixels differ"
            assert m.stats()["gather_bytes"] - before == foreign
        assert m.bands() == bands
        img = m.render(ss[:world], cam, prm, 1, copy_out=True)
        assert np.array_equal(img, restir[1]), f"world {world}: the ReSTIR frame after"
        m.close()


def test_post_frame_on_a_gathered_ground_truth():
    """Three accumulated launches on 3 ranks: rank 0's accumulator statistics are one context's; a context that holds
    only its own strips refuses."""
    H, world, case = 52, 3, CASES["cornell"]
    sc, prm = scenes.cornell_box(8), P.default_params()
    (one,), (ones,) = _renderers(sc, H, 1)
    rs, ss = _renderers(sc, H, world)
    m = MultiGpuFrame(rs)
    m.render(ss, sc.camera, P.metric_params(m_area=4), 0)     # bands first: rank 0's last ReSTIR frame is 17 rows
    for f in range(3):
        _ground_truth(one, ones, sc.camera, prm, "path", f, case, copy_out=False)
        _, want = one.post_frame(accumulate=True)
        _ground_truth(m, ss, sc.camera, prm, "path", f, case)
        _, got = rs[0].post_frame(accumulate=True)
        assert got.pixels == want.pixels == W * H
        assert (got.sum, got.sqr_sum, got.acc_frames_used) == (want.sum, want.sqr_sum, want.acc_frames_used), f
        assert want.acc_frames_used == f and want.sum > 0
    with pytest.raises(RestirError, match="not gathered"):
        rs[1].post_frame(accumulate=True)
    _ground_truth(m, ss, sc.camera, prm, "path", 3, case, gather=False)
    with pytest.raises(RestirError, match="not gathered"):
        rs[0].post_frame(accumulate=True)
    rs[0].render_path(ss[0], sc.camera, prm, 3, rows=(16, 2, 1), copy_out=False)
    with pytest.raises(RestirError, match="not gathered"):
        rs[0].post_frame()
    # a full-frame entry and a ReSTIR band behave as before
    rs[0].render_path(ss[0], sc.camera, prm, 3, copy_out=False)
    rs[0].post_frame()
    one.render_path(ones, sc.camera, prm, 3, rows=(16, 1, 0), copy_out=False)
    assert one.post_frame()[1].pixels == W * H
    m.render(ss, sc.camera, P.metric_params(m_area=4), 1)
    (a, b) = m.bands()[1]
    assert rs[1].post_frame()[1].pixels == (b - a) * W
    m.close()


def _write_scene(tmp_path, sc):
    obj = tmp_path / "scene.obj"
    scenes.write_obj(sc, str(obj))
    c = sc.camera
    return str(obj), [*map(str, c.eye), *map(str, c.at), str(c.fov_y)]


@pytest.fixture(scope="module")
def gt_rccl_driver(tmp_path_factory):
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    assert os.path.exists(os.path.join(build, "librestir_rcclstub.so")), \
        "build it first: make -C tests/cpp (run by __graft_entry__.build())"
    exe = str(tmp_path_factory.mktemp("gt_rccl") / "mgpu_gt_rccl_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mgpu_gt_rccl_driver.cpp"),
                           "-L" + build, "-lrestir_rcclstub", "-Wl,-rpath," + build, "-pthread"])
    return exe


@pytest.mark.parametrize("world", [2, 4])
def test_rccl_branch_threads_on_one_gpu(tmp_path, gt_rccl_driver, world):
    """72 x 52 (strips of 16, 16, 16 and 4 rows): with 2 ranks rank 1 sends two strips, the second short -- the
    stand-in pairs them with rank 0's receives in issue order and counts unequal sizes."""
    obj, cam = _write_scene(tmp_path, scenes.cornell_many_lights(64))
    frames = 2
    cmd = [gt_rccl_driver, obj, str(W), "52", str(world), str(frames), "2", "3", *cam]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    r = json.loads(line[-1])
    print(f"[rccl-stub] {r}")
    assert r["bad_frames"] == 0 and r["mismatches"] == 0 and r["unpaired"] == 0 and r["pairs"] > 0, (r, p.stderr[-2000:])
    assert p.returncode == 0 and r["rank_errors"] == 0
    foreign = sum(b - a for q in range(1, world) for a, b in strip_rows_of(52, q, world))
    assert r["pairs"] == 2 * frames * sum(len(strip_rows_of(52, q, world)) for q in range(1, world))
    assert r["bytes"] == r["gather_bytes"] == 2 * frames * foreign * W * 12


@pytest.mark.parametrize("unbiased", [False, True])
def test_restir_render_ranks_path_compare(tmp_path, unbiased):
    exe = os.path.join(ROOT, "restir-embree_amd", "restir_render")
    assert os.path.exists(exe), "build it first (__graft_entry__.build())"
    obj, cam = _write_scene(tmp_path, scenes.cornell_many_lights(64))
    cmd = [exe, "--obj", obj, "--w", str(W), "--h", "52", "--frames", "2", "--ranks", "3", "--path", "2", "--bounces", "3",
           "--compare", "--eye", *cam[0:3], "--at", *cam[3:6], "--fov", cam[6]] + (["--unbiased"] if unbiased else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and line, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    r = json.loads(line[-1])
    assert r["ranks"] == 3 and r["compared"] is True and r["bit_identical"] is True, r
