"""CPU tests: what tests/test_gpu_materials.py relies on, asserted on the oracle alone -- the zoo shows every material
type, the type classes are the oracle's (ReSTIR with and without BRDF candidates, MIS, path), every value edge
changes the frame and leaves it comparable, and the roughness maps give the shininess values they are meant to."""
import numpy as np
import pytest

import material_cases as M
from restir_amd import scenes

SIZE = (50, 38)


def test_zoo_shows_every_type():
    for size in M.SIZES:
        px = M.type_pixels(M.oracle_zoo("pairwise", size).gbuffer)
        print(f"[materials] zoo {size[0]}x{size[1]}: pixels per type {px}")
        assert set(px) == set(M.ALL_TYPES)
        assert min(px.values()) >= M.MIN_PIXELS
    sc = M.zoo()
    non_lambert = [m for m in sc.materials if m.type != scenes.LAMBERT and not any(m.le)]
    assert len(non_lambert) == 6 and all(max(m.ks) > 0 for m in non_lambert)
    assert len({m.shininess for m in non_lambert}) == 6
    assert sorted(m.type for m in non_lambert if m.type in (scenes.PHONG, scenes.DIELECTRIC)) == [2, 4]


def _restir(sc, m_brdf):
    return M.oracle_restir(sc, M.reuse_params(m_brdf=m_brdf), SIZE, M.ZOO_FRAMES)


@pytest.mark.parametrize("m_brdf,classes", [(2, M.CLASSES), (0, M.CLASSES_NO_BRDF)], ids=["brdf2", "brdf0"])
def test_restir_type_classes(m_brdf, classes):
    """Re-typing every material inside its class changes nothing but the G-buffer's type column; moving one wall
    across each class boundary changes the frame."""
    sc = M.zoo()
    base = _restir(sc, m_brdf)
    rot = M.rotation(classes)
    assert sum(rot[t] != t for t in M.ALL_TYPES) == sum(len(c) for c in classes if len(c) > 1)
    moved = _restir(M.retyped(sc, rot), m_brdf)
    M.assert_same_render(base, moved, f"m_brdf={m_brdf} rotation", type_column=False)
    assert not np.array_equal(base.gbuffer[..., M.TYPE_COL], moved.gbuffer[..., M.TYPE_COL])
    for a, b in M.CROSSINGS[m_brdf]:
        crossed = _restir(M.retyped(sc, {a: b}), m_brdf)
        n = int(np.any(crossed.frames[-1] != base.frames[-1], -1).sum())
        print(f"[materials] m_brdf={m_brdf}: type {a} -> {b} changes {n} pixels")
        assert n > 0


@pytest.mark.parametrize("kind", ["mis", "path"])
def test_mis_and_path_type_classes(kind):
    render = M.oracle_mis if kind == "mis" else M.oracle_path
    sc = M.zoo()
    base = render(sc, SIZE)
    moved = render(M.retyped(sc, M.rotation(M.CLASSES_MIS)), SIZE)
    for f, (a, b) in enumerate(zip(base, moved)):
        assert np.array_equal(a, b), f"{kind} frame {f}"
    crossed = render(M.retyped(sc, {scenes.MIRROR: scenes.PHONG}), SIZE)
    assert int(np.any(crossed[0] != base[0], -1).sum()) > 0
    crossed = render(M.retyped(sc, {scenes.DIELECTRIC: scenes.NORMAL}), SIZE)
    assert int(np.any(crossed[0] != base[0], -1).sum()) > 0


@pytest.mark.parametrize("case", list(M.EDGES))
def test_value_edge_is_not_vacuous(case):
    """Each edge changes the oracle's frame.  The one exception is pinned as such: an emitter's reflectance is never
    evaluated (evaluateF returns 0 on a pixel whose Le is positive), so a Phong-typed emitter changes the G-buffer --
    kd, ks, type and a 1/I_M on the emitter's pixels -- and not the frame."""
    base, edge = M.oracle_edge(None), M.oracle_edge(case)
    changed = [int(np.any(a != b, -1).sum()) for a, b in zip(edge.frames, base.frames)]
    black = int((edge.frames[-1].sum(-1) == 0).sum()) - int((base.frames[-1].sum(-1) == 0).sum())
    inf = int(np.isinf(edge.frames[-1]).any(-1).sum())
    print(f"[materials] {case}: pixels changed per frame {changed}, black pixels {black:+d}, infinite pixels {inf}, "
          f"NaN reservoirs {int(np.isnan(edge.reservoirs).any(-1).sum())}")
    assert not any(np.isnan(f).any() for f in edge.frames)           # Integrator::sanitize
    if case == "emitter_phong":
        assert changed == [0, 0]
        g0, g1 = base.gbuffer, edge.gbuffer
        on = g1[..., M.TYPE_COL] != g0[..., M.TYPE_COL]
        assert on.sum() > 0 and (g1[on][:, M.IM_COL] > 0).all() and (g0[on][:, M.IM_COL] == 0).all()
        return
    assert min(changed) > 0
    if case == "le_1e30":
        assert inf > 0                 # p-hat = length(L) squares 1e30: the frame holds +inf, which compares as a number
    else:
        assert inf == 0


def test_negative_shininess_blackens_diffuse_pixels():
    """The oracle's behaviour that the kernels must reproduce: with shininess -0.5 and ks = 0 the pdf's lobe term is
    a * pow(0, -0.5) * 0 = inf * 0 = NaN wherever the light direction is at or behind the mirror direction's horizon;
    the pixel's weight sum becomes NaN and the sanitised pixel is black.  The same with shininess +inf (a = inf) and
    NaN."""
    base = M.oracle_edge(None)
    for case in ("shin_neg_ks0", "shin_inf", "shin_nan"):
        edge = M.oracle_edge(case)
        g = edge.gbuffer
        no_lobe = (g[..., 16] > 0) & (g[..., 9:12].max(-1) == 0) & (g[..., 12:15].sum(-1) == 0) & \
                  (g[..., M.SHIN_COL] != base.gbuffer[..., M.SHIN_COL])            # the edited walls where ks = 0
        black = no_lobe & (edge.frames[-1].sum(-1) == 0) & (base.frames[-1].sum(-1) > 0)
        print(f"[materials] {case}: {int(black.sum())} of {int(no_lobe.sum())} edited pixels without a lobe are black")
        assert black.sum() > 0


@pytest.mark.parametrize("which", list(M.ROUGH_MAPS))
def test_roughness_map_gives_the_edge_shininess(which):
    base, edge = M.oracle_rough(None), M.oracle_rough(which)
    g = edge.gbuffer
    phong = g[..., M.TYPE_COL] == scenes.PHONG
    shin = g[..., M.SHIN_COL]
    count = {"inf": int((np.isinf(shin) & phong).sum()), "negative": int(((shin < 0) & phong).sum()),
             "zero": int(((shin == 0) & phong).sum())}
    print(f"[materials] {which}: Phong pixels with shininess {count}")
    want = {"u8_zero_blocks": ("inf",), "u8_255": ("zero",), "float_1p5_and_0": ("negative", "inf")}[which]
    assert all(count[k] > 0 for k in want)
    assert min(int(np.any(a != b, -1).sum()) for a, b in zip(edge.frames, base.frames)) > 0
    assert all(np.isfinite(f).all() for f in edge.frames)
    tex = M.ROUGH_MAPS[which]()
    if which == "u8_zero_blocks":                                     # a block of at least 3 x 3 zero texels
        z = tex[..., 0] == 0
        assert any(z[y:y + 3, x:x + 3].all() for y in range(z.shape[0] - 2) for x in range(z.shape[1] - 2))
    elif which == "u8_255":
        assert tex.dtype == np.uint8 and (tex == 255).any()
    else:
        assert tex.dtype == np.float32 and tex.shape[2] == 3 and (tex == 1.5).any() and (tex == 0).any()


def test_obj_default_scene_is_type_normal_shininess_zero():
    sc = M.obj_default_scene()
    assert all(m.type == scenes.NORMAL and m.shininess == 0.0 for m in sc.materials)
    assert M.srgb_expand(0.5) == pytest.approx(0.21404114, rel=1e-6) and M.srgb_expand(0.02) == pytest.approx(0.02 / 12.92)
    frame = M.oracle_restir(sc, M.edge_params(), SIZE, 1).frames[0]
    assert np.isfinite(frame).all() and frame.max() > 0
