"""GPU tests: every frame parameter away from its default, on every pass form, against the CPU oracle -- the three
frames, the final reservoirs and the final G-buffer element for element (np.array_equal; no tolerance).  The cases
and the oracle's runs come from tests/param_cases.py; that each case changes the frame is asserted on the oracle
alone in tests/test_param_cases_oracle.py.

Forms, each asserting the state it ran in: one context with lockstep and with per-lane walks (the whole table); the
wave-sorted passes pinned on and off; the candidate-split initial pass; run-ahead 2; tiles of 2 and 3 contexts with
halos of 0, 1, 12 and 20 rows; MultiGpuFrame over local contexts, its halo bytes and its refusal of a band thinner
than the halo; the three ground truths.  One renderer and scene handle per form, shared by the cases.

The ranges of spatial_radius and confidence_cap (restir_c.h): every value outside them is rejected before anything is
launched, by rs_render_frame, rs_tile_begin and rs_mgpu_render_frame, and the history is as if the call had not been
made.
"""
import numpy as np
import pytest

import gpu_harness as GH
import param_cases as C
from restir_amd import params as P
from restir_amd.distributed import halo_rows
from restir_amd.mgpu import MultiGpuFrame
from restir_amd.renderer import Renderer, RestirError

pytestmark = pytest.mark.gpu

WALKS = ("lockstep", "lane")
NAN, INF = float("nan"), float("inf")
ABOVE = float(np.nextafter(np.float32(P.MAX_SPATIAL_RADIUS), np.float32(INF)))
REJECTED = [("spatial_radius", v) for v in (NAN, -1.0, -1e-30, -INF, INF, 1e20, ABOVE)] + \
           [("confidence_cap", v) for v in (P.MAX_CONFIDENCE_CAP + 1, 2**31 - 1)]


@pytest.fixture(scope="module")
def oracle_runs():
    """the oracle's run of every case, once"""
    return {case: C.oracle(case) for case in (None, *C.ALL)}


@pytest.fixture(scope="module")
def forms():
    """get(monkeypatch, size, walk, split, sort, ahead) -> (renderer, scene handle): one per form, made on first use
    (the sorted passes are chosen from the environment when the context is created) and closed at the end"""
    cache, streams = {}, []

    def get(monkeypatch, size, walk, split="off", sort=None, ahead=None):
        key = (size, walk, split, sort, ahead)
        if key not in cache:
            GH.set_env(monkeypatch, RESTIR_SORT=sort, RESTIR_SORT_SPATIAL=sort, RESTIR_SORT_TEMPORAL=sort)
            stream = None
            if ahead is not None:            # frames read on the device: a stream torch orders its clones on
                import torch
                streams.append(torch.cuda.Stream())
                stream = streams[-1].cuda_stream
            g = GH.pinned_renderer(*size, walk, split, run_ahead=ahead, stream=stream)
            gs = g.load_scene(C.scene())
            assert gs.walk_info()["status"] == "live"
            cache[key] = (g, gs)
        return cache[key]

    yield get
    for g, gs in cache.values():
        gs.close()
        g.close()


def _run(form, prm, walk, split="off"):
    """FRAMES frames of prm on the orbit; every frame walked and split as pinned"""
    g, gs = form

    def frame(h, cam, f):
        out = g.produce_restir(h, cam, prm, f)
        GH.assert_walked(g, walk, split)
        return out
    return GH.run_restir(g, gs, C.scene(), C.FRAMES, frame, C.camera)


# ---------------------------------------------------------------- 1. one context, the whole table
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", C.ALL)
def test_case_matches_oracle(case, walk, forms, oracle_runs, monkeypatch):
    got = _run(forms(monkeypatch, C.size(case), walk), C.params(case), walk)
    GH.assert_same_render(got, oracle_runs[case], f"{case} {walk}")
    if case in C.CONF_MAX:
        assert got.reservoirs[..., 11].max() == C.CONF_MAX[case]


@pytest.mark.parametrize("walk", WALKS)
def test_base_matches_oracle(walk, forms, oracle_runs, monkeypatch):
    GH.assert_same_render(_run(forms(monkeypatch, C.SIZE, walk), C.params(), walk), oracle_runs[None], f"base {walk}")


# ---------------------------------------------------------------- 2. the sorted passes pinned on and off
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", C.SORTED)
def test_sorted_passes_on_and_off(case, walk, forms, oracle_runs, monkeypatch):
    """RESTIR_SORT, RESTIR_SORT_SPATIAL and RESTIR_SORT_TEMPORAL all on and all off (BASE has CONSTANT weights and
    four neighbours, which the sorted spatial pass takes): equal to each other and to the oracle"""
    runs = {s: _run(forms(monkeypatch, C.SIZE, walk, sort=s), C.params(case), walk) for s in ("on", "off")}
    GH.assert_same_render(runs["on"], runs["off"], f"{case} {walk} sorted on vs off")
    GH.assert_same_render(runs["on"], oracle_runs[case], f"{case} {walk} sorted")


# ---------------------------------------------------------------- 3. the split initial pass and run-ahead
@pytest.mark.parametrize("case", C.SPLIT_AHEAD)
def test_initial_split(case, forms, oracle_runs, monkeypatch):
    got = _run(forms(monkeypatch, C.SIZE, "lockstep", split="on"), C.params(case), "lockstep", split="on")
    GH.assert_same_render(got, oracle_runs[case], f"{case} split")


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", C.SPLIT_AHEAD)
def test_run_ahead(case, walk, forms, oracle_runs, monkeypatch):
    """Run-ahead 2: three frames enqueued back to back with no host synchronisation between them, each cloned from
    the framebuffer on the frames' stream"""
    import torch
    from restir_amd.distributed import _CudaBuf
    g, gs = forms(monkeypatch, C.SIZE, walk, ahead=2)
    (w, h), prm, sc = C.SIZE, C.params(case), C.scene()
    g.reset_history()
    stream = torch.cuda.ExternalStream(g.stream)
    clones = []
    with torch.cuda.stream(stream):
        for f in range(C.FRAMES):
            g.produce_restir(gs, C.camera(sc, f), prm, f, copy_out=False, timed=False)
            clones.append(torch.as_tensor(_CudaBuf(g.frame_device_ptr(), w * h * 12, "<f4", 4), device="cuda").clone())
        frames = [c.cpu().numpy().reshape(h, w, 3) for c in clones]      # on the clones' stream: the copy waits for them
    GH.assert_walked(g, walk)
    got = GH.Render(frames, g.gbuffer().copy(), g.reservoirs().copy())
    GH.assert_same_render(got, oracle_runs[case], f"{case} {walk} run-ahead 2")


# ---------------------------------------------------------------- 4. tiles and MultiGpuFrame
def _cams():
    return [C.camera(C.scene(), f) for f in range(C.FRAMES)]


@pytest.fixture(scope="module")
def full_frames(forms):
    """the single context's frames of the tile cases at TILE_SIZE, equal to the oracle's"""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        form = forms(mp, C.TILE_SIZE, "lockstep")
        for case in C.TILES:
            got = _run(form, C.params(case), "lockstep")
            GH.assert_same_render(got, C.oracle(case, C.TILE_SIZE), f"{case} at {C.TILE_SIZE}")
            out[case] = got.frames
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("case", C.TILES)
def test_tiles_with_each_halo(case, n_ranks, full_frames):
    """Bands of 32 and of 21 or 22 rows with halos of 0, 0, 1, 12 and 20 rows, margin = the halo"""
    w, h = C.TILE_SIZE
    prm = C.params(case)
    if case in C.HALO:
        assert halo_rows(prm) == C.HALO[case]
    tiles = GH.emulate_tiles(C.scene(), w, h, prm, n_ranks, _cams(), margin=0)
    for f, (a, b) in enumerate(zip(tiles, full_frames[case])):
        assert np.array_equal(a, b), f"{case} {n_ranks} ranks frame {f}: {int((a != b).any(-1).sum())} px differ"


def _mgpu(world):
    w, h = C.TILE_SIZE
    rs = [Renderer(w, h) for _ in range(world)]
    for r in rs:
        r.set_traversal("lockstep")               # frames on the run-ahead lanes (no AUTO tuning frames)
    ss = [r.load_scene(C.scene()) for r in rs]
    return rs, ss, MultiGpuFrame(rs)


def test_mgpu_halos_of_12_and_20_rows(full_frames):
    """MultiGpuFrame over two local contexts: frames equal the single context's, the halo bytes are the plan's --
    per exchange and direction rows x W x 48 B (rs_mgpu.hip halo_bytes), one exchange per spatial pass -- and a
    rejected parameter between two frames leaves the bands' history alone"""
    (w, h), world = C.TILE_SIZE, 2
    rs, ss, m = _mgpu(world)
    cams = _cams()
    for case in C.MGPU:
        prm = C.params(case)
        m.reset_history()
        m.stats(reset=True)
        for f, cam in enumerate(cams):
            for field, v in REJECTED:
                with pytest.raises(RestirError, match=field):
                    m.render(ss, cam, C.params(case, **{field: v}), f, copy_out=True)
            img = m.render(ss, cam, prm, f, copy_out=True)
            ref = full_frames[case][f]
            assert np.array_equal(img, ref), f"{case} frame {f}: {int((img != ref).any(-1).sum())} px differ"
        st = m.stats()
        want = C.FRAMES * prm.spatial_passes * 2 * (world - 1) * C.HALO[case] * w * 48
        assert st["frames"] == C.FRAMES and st["halo_bytes_sent"] == st["halo_bytes_recv"] == want, (case, st, want)
    m.close()


def test_mgpu_band_thinner_than_halo():
    """Four bands of 16 rows: a 20-row halo is refused loudly, a 12-row halo renders"""
    rs, ss, m = _mgpu(4)
    cam = _cams()[0]
    assert m.bands() == [(0, 16), (16, 32), (32, 48), (48, 64)]
    with pytest.raises(RestirError, match="band is thinner than the spatial halo"):
        m.render(ss, cam, C.params("radius_400"), 0, copy_out=True)
    img = m.render(ss, cam, C.params("radius_150"), 0, copy_out=True)
    want = C.oracle("radius_150", C.TILE_SIZE).frames[0]
    assert np.array_equal(img, want), f"{int((img != want).any(-1).sum())} px differ"
    m.close()


# ---------------------------------------------------------------- 5. the ground truths
class _GpuTruths:
    def __init__(self, walk):
        self.g = Renderer(*C.GT_SIZE)
        self.g.set_traversal(walk)
        self.gs = self.g.load_scene(C.scene())
        self.walk = walk

    def render_direct_mis(self, cam, prm, f, spp):
        out = self.g.render_direct_mis(self.gs, cam, prm, f, spp).copy()
        assert self.g.traversal()[1] == GH.KIND[self.walk]
        return out

    def render_path(self, cam, prm, f, spp, **kw):
        out = self.g.render_path(self.gs, cam, prm, f, spp, **kw).copy()
        assert self.g.traversal()[1] == GH.KIND[self.walk]
        return out


def test_ground_truths_with_moved_offsets():
    """render_direct_mis, render_path and render_path(unbiased=True) with tnear_offset, normal_offset, the seed and
    the background away from their defaults: the walk kinds bit-identical, the frame within the project's frame
    bound of its CPU checker (tests/test_gpu_path.py, tests/test_gpu_path_unbiased.py)"""
    prm = P.default_params(**C.GT_FIELDS)
    want = C.oracle_truths(True)
    gpu = {walk: _GpuTruths(walk) for walk in WALKS}
    for kind in C.GT_KINDS:
        for f in range(C.GT_FRAMES):
            a, b = (C.ground_truth(kind, gpu[walk], prm, f) for walk in WALKS)
            assert np.array_equal(a, b), f"{kind} frame {f}: lockstep != lane"
            GH.assert_close(a, want[kind][f], f"{kind} frame {f} with moved offsets", tag="path")
            assert (a == np.asarray(C.BG, np.float32)).all(-1).any()


# ---------------------------------------------------------------- 6. the ranges
def test_out_of_range_radius_and_cap_are_rejected(forms, oracle_runs, monkeypatch):
    """Each value raises RestirError with a message naming its field, from rs_render_frame and from rs_tile_begin,
    between the frames of a temporal sequence: the sequence still equals the oracle's, so the history -- reservoirs,
    G-buffers, the frame count -- is untouched and no tile frame was left in flight."""
    g, gs = forms(monkeypatch, C.SIZE, "lockstep")
    w, h = C.SIZE

    def frame(handle, cam, f):
        for field, v in REJECTED:
            bad = C.params(**{field: v})
            with pytest.raises(RestirError, match=field):
                g.produce_restir(handle, cam, bad, f)
            with pytest.raises(RestirError, match=field):
                g.tile_begin(handle, cam, bad, f, 0, h, 0, 0)
        return g.produce_restir(handle, cam, C.params(), f)
    GH.assert_same_render(GH.run_restir(g, gs, C.scene(), C.FRAMES, frame, C.camera), oracle_runs[None], "base with rejected calls")
    # a radius is checked whether or not a spatial pass reads it
    with pytest.raises(RestirError, match="spatial_radius"):
        g.produce_restir(gs, C.scene().camera, P.default_params(spatial_radius=NAN), 0)


def test_frame_sides_beyond_2_to_30_are_rejected():
    """the frame side the radius bound is derived for (restir_c.h RS_MAX_SPATIAL_RADIUS)"""
    for size in ((2**30 + 1, 1), (1, 2**30 + 1)):
        with pytest.raises(RestirError, match="2\\^30"):
            Renderer(*size)
