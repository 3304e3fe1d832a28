"""GPU tests of the scene's light tables (rs_debug_light_tables): the emitter records, the light CDF and its guide
table, which one device builder (restir_capi.hip light_table) writes at scene creation, at every
rs_scene_update_positions and at rs_scene_rebuild.

Everything is compared bit for bit: cdf, pick and area with the oracle's tables (OracleScene.cdf(), the reference's
TriangleCDF restated), the remaining fields with a float32 numpy restatement of them (IEEE single divisions and
products of the oracle's values; np.cumsum in float32 is the sequential sum the reference forms), the positions,
normals and emission with the scene's inputs.

The emitter counts reach every path of the builder: 1 and 2 (near-minimal), 16 (a multiple of the 4-wide step),
2050 (a tail of 2), 8198 (one full 8192-element chunk, then a chunk of one 4-wide step and a tail of 2) and 0 (the
zero placeholders; the kernel does not run)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_harness import assert_close, assert_same_bits, bits
from restir_amd import params as P
from restir_amd import scenes
from restir_amd.renderer import Renderer

pytestmark = pytest.mark.gpu

K_CDF_GUIDE = 1024


def _with(sc, **kw):
    f = dict(positions=sc.positions, normals=sc.normals, tri_material=sc.tri_material, materials=sc.materials,
             camera=sc.camera)
    f.update(kw)
    return scenes.Scene(**f)


def _single_emitter():
    sc = scenes.cornell_box(1)
    keep = np.ones(sc.n_tris, bool)
    keep[np.flatnonzero(sc.emissive_mask())[1:]] = False
    return _with(sc, positions=sc.positions[keep], normals=sc.normals[keep], tri_material=sc.tri_material[keep])


def _no_emitter():
    sc = scenes.cornell_box(1)
    return _with(sc, materials=[scenes.Material(**{**vars(m), "le": (0.0, 0.0, 0.0)}) for m in sc.materials])


def _bent_normals():
    """cornell_many_lights(8) with the three vertex normals of one emissive triangle made different."""
    sc = scenes.cornell_many_lights(8)
    t = np.flatnonzero(sc.emissive_mask())[5]
    nrm = np.array(sc.normals, np.float32, copy=True)
    for v, d in enumerate(([0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1])):
        n = nrm[t, 3 * v:3 * v + 3].astype(np.float64) + d
        nrm[t, 3 * v:3 * v + 3] = (n / np.linalg.norm(n)).astype(np.float32)
    return _with(sc, normals=nrm)


SCENES = {
    "lights_2": lambda: scenes.cornell_many_lights(1),
    "lights_16": lambda: scenes.cornell_many_lights(8),
    "lights_2050": lambda: scenes.cornell_many_lights(1025),
    "lights_8198": lambda: scenes.cornell_many_lights(4099),
    "single": _single_emitter,
    "bent_normals": _bent_normals,
}
N_EMIS = {"lights_2": 2, "lights_16": 16, "lights_2050": 2050, "lights_8198": 8198, "single": 1, "bent_normals": 16}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


def _assert_tables(gs, sc, what):
    """The scene's current tables against the oracle's for `sc` (the inputs the tables were built from)."""
    em, cdf, guide = gs.debug_light_tables()
    emis = np.flatnonzero(sc.emissive_mask())
    ne = emis.size
    assert em.shape[0] == cdf.shape[0] == gs.n_emissive == ne, what
    os_ = O.OracleScene(sc)
    assert os_.n_emissive == ne
    o_cdf, o_pick, o_area = os_.cdf()
    assert (o_area > 0).all() and (np.diff(o_cdf) > 0).all(), what      # what the scenes here promise
    assert_same_bits(cdf, o_cdf, f"{what}: cdf")
    assert_same_bits(em[:, 4, 3], o_pick, f"{what}: pick")
    assert_same_bits(em[:, 6, 0], o_area, f"{what}: area")
    # the remaining fields, in float32 like the reference
    total = np.cumsum(o_area, dtype=np.float32)[-1]
    inv_area = np.float32(1.0) / o_area
    pdf_brdf = (o_area / total) * inv_area
    pos, nrm = (np.ascontiguousarray(a, np.float32).reshape(-1, 3, 3)[emis] for a in (sc.positions, sc.normals))
    nb = bits(nrm)
    flat = (nb[:, 0] == nb[:, 1]).all(axis=1) & (nb[:, 0] == nb[:, 2]).all(axis=1)
    pdf_area = o_pick * inv_area
    assert_same_bits(em[:, 6, 1], inv_area, f"{what}: inv_area")
    assert_same_bits(em[:, 0, 3], np.where(flat, pdf_area, -pdf_area), f"{what}: signed pdf_area")
    assert_same_bits(em[:, 5, 3], pdf_brdf, f"{what}: pdf_brdf")
    j = np.arange(K_CDF_GUIDE + 1, dtype=np.float32) / np.float32(K_CDF_GUIDE)
    assert np.array_equal(guide, np.searchsorted(cdf, j, "left")), f"{what}: guide"
    # the inputs, carried over
    le = sc.material_arrays()[0][:, 6:9][np.asarray(sc.tri_material)[emis]]
    assert_same_bits(em[:, 0:3, 0:3], pos, f"{what}: positions")
    assert_same_bits(em[:, 1:4, 3], nrm[:, 0], f"{what}: n0")
    assert_same_bits(em[:, 4, 0:3], nrm[:, 1], f"{what}: n1")
    assert_same_bits(em[:, 5, 0:3], nrm[:, 2], f"{what}: n2")
    assert_same_bits(em[:, 3, 0:3], le, f"{what}: emission")
    assert not bits(em[:, 6, 2:]).any() and not bits(em[:, 7]).any(), f"{what}: padding"
    return flat


@pytest.mark.parametrize("name", list(SCENES))
def test_fresh_scene_tables_match_oracle(name):
    sc = _scene(name)
    g = Renderer(32, 24)
    gs = g.load_scene(sc)
    assert gs.n_emissive == N_EMIS[name]
    flat = _assert_tables(gs, sc, name)
    assert int((~flat).sum()) == (1 if name == "bent_normals" else 0)
    gs.close()
    g.close()


def test_scene_without_emitters_keeps_zero_tables():
    sc = _no_emitter()
    g = Renderer(32, 24)
    gs = g.load_scene(sc)
    em, cdf, guide = gs.debug_light_tables()
    assert gs.n_emissive == 0 and em.shape[0] == 0 and cdf.shape[0] == 0
    assert not guide.any()
    img = g.produce_restir(gs, sc.camera, P.c3_params(m_area=8), 0)
    assert np.isfinite(img).all()
    gs.rebuild()
    assert not gs.debug_light_tables()[2].any()
    gs.close()
    g.close()


@pytest.mark.parametrize("name", ["lights_2050", "lights_8198"])
def test_tables_after_updates_match_oracle(name):
    """The same assertions against a fresh oracle scene of the moved positions: after an in-place update (with
    normals), after a pipelined update with a frame in flight, and after a rebuild."""
    sc = _scene(name)
    g = Renderer(32, 24)
    gs = g.load_scene(sc)
    prm = P.c3_params(m_area=8)
    g.set_run_ahead(0)
    for t, normals in ((20, None), (40, sc.normals)):
        pos = scenes.moving_light_positions(sc, t, 240, amplitude=0.05)
        gs.update_positions(pos, normals)
        _assert_tables(gs, _with(sc, positions=pos), f"{name}: in place, t = {t}")
    g.set_run_ahead(2)
    g.produce_restir(gs, sc.camera, prm, 0, copy_out=False, timed=False)
    pos = scenes.moving_light_positions(sc, 90, 240, amplitude=0.4)
    gs.update_positions(pos)
    _assert_tables(gs, _with(sc, positions=pos), f"{name}: pipelined")
    gs.rebuild()
    _assert_tables(gs, _with(sc, positions=pos), f"{name}: rebuild")
    g.synchronize()
    gs.close()
    g.close()


def test_frame_of_chunked_table_matches_oracle():
    """One frame whose area candidates come from the 8198-emitter tables (the second chunk included)."""
    sc, prm, W, H = _scene("lights_8198"), P.c3_params(m_area=8), 32, 24
    g = Renderer(W, H)
    gs = g.load_scene(sc)
    a = g.produce_restir(gs, sc.camera, prm, 0).copy()
    b = O.OracleRenderer(W, H).render(O.OracleScene(sc), sc.camera, prm, 0)
    assert_close(a, b, "8198 emitters")
    gs.close()
    g.close()
