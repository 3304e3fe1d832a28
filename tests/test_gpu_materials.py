"""GPU tests: the seven material types and the extreme material values, end to end on the HIP renderer against the
CPU oracle -- frames, the whole G-buffer (1/I_M included) and the reservoirs element for element.  Scenes, cases and
the oracle's renders come from tests/material_cases.py; what they rely on is asserted on the oracle alone in
tests/test_materials_oracle.py."""
import numpy as np
import pytest

import material_cases as M
from gpu_harness import assert_close
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

SIZE_IDS = [f"{w}x{h}" for w, h in M.SIZES]


# ---------------------------------------------------------------- 1. the type matrix
@pytest.mark.parametrize("size", M.SIZES, ids=SIZE_IDS)
def test_zoo_shows_every_type_on_the_gpu(size):
    px = M.type_pixels(M.gpu_restir(M.zoo(), M.config("a3b2"), size, 1).gbuffer)
    assert set(px) == set(M.ALL_TYPES) and min(px.values()) >= M.MIN_PIXELS, px


@pytest.mark.parametrize("size", M.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("cfg", list(M.INITIAL))
def test_initial_pass_matches_oracle(cfg, size):
    """The initial pass alone, with and without area candidates, under both walk kinds and both layouts of the pass"""
    want = M.oracle_zoo(cfg, size)
    for traversal in ("lockstep", "lane"):
        for split in ("off", "on"):
            got = M.gpu_restir(M.zoo(), M.config(cfg), size, M.ZOO_FRAMES, traversal, split)
            M.assert_same_render(got, want, f"{cfg} {traversal} split {split}")


@pytest.mark.parametrize("size", M.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("cfg", list(M.REUSE))
def test_reuse_passes_match_oracle(cfg, size):
    """Temporal reuse, the visibility pass and two spatial passes in every spatial_mis mode, and with
    reject_dissimilar"""
    M.assert_same_render(M.gpu_restir(M.zoo(), M.config(cfg), size, M.ZOO_FRAMES), M.oracle_zoo(cfg, size), cfg)


def _gpu_truth(kind, sc, size, traversal=None):
    g = Renderer(*size)
    if traversal:
        g.set_traversal(traversal)
    gs = g.load_scene(sc)
    if kind == "mis":
        return [g.render_direct_mis(gs, sc.camera, P.default_params(), f, M.MIS_SPP).copy() for f in range(2)]
    return [g.render_path(gs, sc.camera, P.default_params(), f, M.PATH_SPP, max_bounces=M.PATH_BOUNCES).copy()
            for f in range(2)]


@pytest.mark.parametrize("size", M.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("kind", ["mis", "path"])
def test_mis_and_path_match_oracle(kind, size):
    """render_direct_mis (4 spp) and render_path (2 spp, 3 bounces, GI on) as test_direct_mis_matches_oracle and
    test_path_matches_oracle compare them: the walk kinds bit-identical, the frame within the project's frame bound"""
    sc = M.zoo()
    out = {t: _gpu_truth(kind, sc, size, t) for t in ("lockstep", "lane")}
    want = (M.oracle_mis if kind == "mis" else M.oracle_path)(sc, size)
    for f in range(2):
        assert np.array_equal(out["lockstep"][f], out["lane"][f])
        assert_close(out["lane"][f], want[f], f"{kind} zoo frame {f}", tag="materials")


@pytest.mark.parametrize("m_brdf,classes", [(2, M.CLASSES), (0, M.CLASSES_NO_BRDF)], ids=["brdf2", "brdf0"])
def test_restir_type_classes_on_the_gpu(m_brdf, classes):
    """No oracle: re-typing every material inside its class leaves frames and reservoirs bit-identical and the
    G-buffer too apart from its type column; a re-typing across a class boundary changes the frame."""
    sc, prm, size = M.zoo(), M.reuse_params(m_brdf=m_brdf), M.SIZES[1]
    base = M.gpu_restir(sc, prm, size, M.ZOO_FRAMES)
    moved = M.gpu_restir(M.retyped(sc, M.rotation(classes)), prm, size, M.ZOO_FRAMES)
    M.assert_same_render(base, moved, f"m_brdf={m_brdf} rotation", type_column=False)
    assert not np.array_equal(base.gbuffer[..., M.TYPE_COL], moved.gbuffer[..., M.TYPE_COL])
    for a, b in M.CROSSINGS[m_brdf]:
        crossed = M.gpu_restir(M.retyped(sc, {a: b}), prm, size, M.ZOO_FRAMES)
        assert np.any(crossed.frames[-1] != base.frames[-1]), f"type {a} -> {b} changed nothing"


@pytest.mark.parametrize("kind", ["mis", "path"])
def test_mis_and_path_type_classes_on_the_gpu(kind):
    sc, size = M.zoo(), M.SIZES[1]
    base = _gpu_truth(kind, sc, size)
    moved = _gpu_truth(kind, M.retyped(sc, M.rotation(M.CLASSES_MIS)), size)
    for f in range(2):
        assert np.array_equal(base[f], moved[f]), f"{kind} frame {f}"
    for a, b in ((scenes.MIRROR, scenes.PHONG), (scenes.DIELECTRIC, scenes.NORMAL)):
        assert np.any(_gpu_truth(kind, M.retyped(sc, {a: b}), size)[0] != base[0]), f"type {a} -> {b} changed nothing"


def test_obj_without_pc_and_ns_loads_as_type_normal(tmp_path):
    """An ordinary MTL -- Kd, a non-zero Ks, Ke on the emitters, neither Pc nor Ns -- loads as type NORMAL with
    shininess 0 and renders the frames of the array scene with those values and sRGB-expanded Kd and Ks, bit for bit."""
    want_sc = M.obj_default_scene()
    obj = tmp_path / "default.obj"
    M.write_default_obj(want_sc, str(obj))
    assert "Pc" not in (tmp_path / "default.mtl").read_text() and "Ns" not in (tmp_path / "default.mtl").read_text()
    prm, size = M.edge_params(), M.SIZES[1]
    g = Renderer(*size)
    gs = g.load_scene(str(obj))
    assert gs.n_tris == want_sc.n_tris and gs.n_emissive == int(want_sc.emissive_mask().sum())
    got = M.run_restir(g, gs, want_sc, M.EDGE_FRAMES, lambda h, c, f: g.produce_restir(h, c, prm, f))
    hit = got.gbuffer[..., 16] > 0
    assert (got.gbuffer[hit][:, M.TYPE_COL] == scenes.NORMAL).all() and (got.gbuffer[hit][:, M.SHIN_COL] == 0).all()
    assert got.gbuffer[hit][:, 9:12].max() > 0
    M.assert_same_render(got, M.gpu_restir(want_sc, prm, size, M.EDGE_FRAMES), "obj default vs array scene")
    M.assert_same_render(got, M.oracle_restir(want_sc, prm, size, M.EDGE_FRAMES), "obj default vs oracle")


# ---------------------------------------------------------------- 2. value edges
@pytest.mark.parametrize("case", list(M.EDGES))
def test_value_edge_matches_oracle(case):
    """One property of the LAMBERT, PHONG and MIRROR walls, or of one emitter, at an extreme value: temporal + spatial
    reuse with pairwise weights and two BRDF candidates, two frames at 50 x 38."""
    got = M.gpu_restir(M.edge_scene(case), M.edge_params(), M.EDGE_SIZE, M.EDGE_FRAMES)
    M.assert_same_render(got, M.oracle_edge(case), case)


def test_unmodified_edge_room_matches_oracle():
    M.assert_same_render(M.gpu_restir(M.edge_scene(), M.edge_params(), M.EDGE_SIZE, M.EDGE_FRAMES), M.oracle_edge(None),
                         "edge room")


@pytest.mark.parametrize("which", list(M.ROUGH_MAPS))
def test_roughness_map_edge_matches_oracle(which):
    """Shininess = 2 / r^2 - 2 per pixel from a roughness map: +inf from texels of 0, 0 from texels of 1 (255), negative
    from float texels above 1"""
    got = M.gpu_restir(M.rough_scene(which), M.edge_params(), M.EDGE_SIZE, M.EDGE_FRAMES)
    M.assert_same_render(got, M.oracle_rough(which), which)


SORTED_CASES = ("shin_neg_ks0", "shin_neg_ks", "shin_inf", "kd0_ks0", "le_1e30", "float_1p5_and_0")


@pytest.mark.parametrize("traversal", ["lane", "lockstep"])
@pytest.mark.parametrize("case", SORTED_CASES)
def test_value_edge_under_the_sorted_passes(case, traversal, monkeypatch):
    """The wave-sorted initial, temporal and spatial passes (RESTIR_SORT*, as test_sorted_initial_pass_bit_identical
    selects them) keep an unlit candidate's weight as a flag, 0 or NaN: the edges whose weights are NaN or infinite"""
    for k in ("RESTIR_SORT", "RESTIR_SORT_SPATIAL", "RESTIR_SORT_TEMPORAL"):
        monkeypatch.setenv(k, "on")
    rough = case in M.ROUGH_MAPS
    sc = M.rough_scene(case) if rough else M.edge_scene(case)
    got = M.gpu_restir(sc, M.edge_params(), M.EDGE_SIZE, M.EDGE_FRAMES, traversal)
    M.assert_same_render(got, M.oracle_rough(case) if rough else M.oracle_edge(case), f"{case} sorted {traversal}")
