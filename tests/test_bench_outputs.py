"""bench.py's plain run and its options: --full is off by default and gates everything beyond the headline
figure, --dump-outputs writes the last timed step's framebuffer (float32, bounded, a fixed sample when larger)
and two runs with the same arguments give the same arrays."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_flags_default_to_a_plain_run():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_float_arrays(tmp_path):
    frame = np.arange(48 * 64 * 3, dtype=np.float32).reshape(48, 64, 3)
    acc = np.linspace(0.0, 1.0, 11)                    # float64 stays float64
    d = tmp_path / "out" / "nested"
    bench.dump_outputs(str(d), {"frame": frame, "acc": acc})
    assert sorted(os.listdir(d)) == ["acc.npy", "frame.npy"]
    got = np.load(d / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)
    assert np.load(d / "acc.npy").dtype == np.float64


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4000)
    a = np.random.default_rng(3).random((50, 40, 3)).astype(np.float32)     # 24000 B > 4000 B
    bench.dump_outputs(str(tmp_path / "a"), {"frame": a})
    bench.dump_outputs(str(tmp_path / "b"), {"frame": a})
    ga, gb = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "b" / "frame.npy")
    assert ga.dtype == np.float32 and ga.shape == (1000,) and ga.nbytes <= 4000
    assert np.array_equal(ga, gb)
    assert np.isin(ga, a).all() and len(np.unique(ga)) > 900                 # elements of `a`, not a constant


@pytest.mark.gpu
def test_plain_run_dumps_the_last_frame_reproducibly(tmp_path, capsys):
    """Two plain runs at 64x48 (C2's scene and parameters, 2 timed steps after 1 warm-up step): the line carries
    the headline fields and nothing that takes a run of its own, frame.npy is the (H, W, 3) float32 framebuffer of
    frame index warmup + steps - 1, bit-identical between the runs and equal to that frame rendered directly."""
    import torch
    from restir_amd import Renderer
    W, H = 64, 48
    prev = torch.cuda.current_stream()
    frames, lines = [], []
    try:
        for tag in ("a", "b"):
            capsys.readouterr()
            bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--width", str(W), "--height", str(H),
                        "--dump-outputs", str(tmp_path / tag)])
            lines.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1]))
            assert os.listdir(tmp_path / tag) == ["frame.npy"]
            frames.append(np.load(tmp_path / tag / "frame.npy"))
    finally:
        torch.cuda.set_stream(prev)
    for line in lines:
        assert line["metric"] == bench.METRIC and line["unit"] == "frames/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["steps"] == 2 and line["warmup"] == 1
        ms = line["ms_per_step"]
        # both are rounded to 4 decimals: ms_per_step is off by <= 5e-5 ms, i.e. by 5e-5 / ms relative
        assert ms > 0 and line["value"] == pytest.approx(1e3 / ms, rel=1e-4 / ms + 1e-6)
        assert line["cpu_baseline"] is None
        assert not {"configs", "kernel_roofline", "limiter", "full_record"} & set(line)
    a, b = frames
    assert a.dtype == np.float32 and a.shape == (H, W, 3) and np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, b)
    sc, prm, _, _ = bench.workload("C2")
    r = Renderer(W, H, device=0)
    gs = r.load_scene(sc)
    want = r.produce_restir(gs, sc.camera, prm, 2).copy()
    gs.close()
    r.close()
    # the two walk kinds the library tunes between agree on every closest hit; an any-hit ray in ~1e9 may differ
    assert (a == want).all(axis=-1).mean() >= 0.999
