"""CPU tests of tests/gpu_harness.py: about ten GPU modules compare through its helpers, so each helper is shown to
fail when it should.  Synthetic arrays only -- no renderer, no oracle."""
import os

import numpy as np
import pytest

import gpu_harness as GH
from restir_amd import scenes


def _image(h=8, w=8, seed=0):
    return np.random.default_rng(seed).uniform(0.5, 2.0, (h, w, 3)).astype(np.float32)


def _next_up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


# ---------------------------------------------------------------- assert_equal_finite
def test_equal_finite_passes_on_equal_arrays_and_signed_zeros():
    a = _image()
    GH.assert_equal_finite(a, a.copy(), "equal")
    z = np.zeros((8, 8, 3), np.float32)
    GH.assert_equal_finite(-z, z, "-0.0 vs +0.0")


def test_equal_finite_raises_on_one_pixel():
    a, b = _image(), _image()
    b[3, 5, 1] = _next_up(b[3, 5, 1])
    with pytest.raises(AssertionError, match="1 px differ"):
        GH.assert_equal_finite(a, b, "one pixel")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_equal_finite_raises_on_nonfinite_even_if_identical(bad):
    a = _image()
    a[0, 0, 0] = bad
    with pytest.raises(AssertionError):
        GH.assert_equal_finite(a, a.copy(), "non-finite")


# ---------------------------------------------------------------- assert_same_bits
def test_same_bits_passes_on_identical_arrays():
    a = _image()
    GH.assert_same_bits(a, a.copy(), "identical")
    n = a.copy()
    n[2, 2, 2] = np.nan                                   # the same NaN word on both sides
    GH.assert_same_bits(n, n.copy(), "identical NaN")


def test_same_bits_raises_on_signed_zeros():
    z = np.zeros((8, 8, 3), np.float32)
    with pytest.raises(AssertionError):
        GH.assert_same_bits(-z, z, "-0.0 vs +0.0")


def test_same_bits_raises_on_one_ulp_and_counts_one():
    a, b = _image(), _image()
    b[6, 1, 2] = _next_up(b[6, 1, 2])
    with pytest.raises(AssertionError, match=r"one ulp: 1 of 64 differ, first at \[\[6, 1\]\]"):
        GH.assert_same_bits(a, b, "one ulp")
    with pytest.raises(AssertionError, match="1 of 8 differ"):          # rows of a table
        GH.assert_same_bits(a[6], b[6], "one row")
    with pytest.raises(AssertionError, match="1 of 3 differ"):          # a 1-D column
        GH.assert_same_bits(a[6, 1], b[6, 1], "one entry")


def test_bits_views_float32_and_float16():
    assert GH.bits(np.array([1.0, -0.0], np.float32)).tolist() == [0x3F800000, 0x80000000]
    assert GH.bits(np.array([1.0, -0.0], np.float16)).tolist() == [0x3C00, 0x8000]
    assert GH.bits(np.array([1.0], np.float64)).dtype == np.uint32     # converted to float32 first


# ---------------------------------------------------------------- assert_close
def _off_by(ref, pixels, rel):
    """ref with the given pixels scaled by (1 + rel): a relative L2 error of rel in each"""
    out = ref.copy()
    for y, x in pixels:
        out[y, x] *= np.float32(1.0 + rel)
    return out


def test_frame_stats():
    ref = _image()
    frac, mean, mx = GH.frame_stats(_off_by(ref, [(1, 1)], 1.0), ref)
    assert frac == 63 / 64 and mean == pytest.approx(1 / 64) and mx == pytest.approx(1.0)
    # the denominator floor: a black reference pixel is measured against 1e-3
    black = np.zeros((8, 8, 3), np.float32)
    got = black.copy()
    got[0, 0] = (1e-4, 0.0, 0.0)
    assert GH.frame_stats(got, black)[2] == pytest.approx(0.1, rel=1e-5)


def test_close_passes_on_identical_and_when_every_pixel_is_within_tolerance():
    ref = _image()
    GH.assert_close(ref.copy(), ref, "identical")
    assert int(np.ceil(GH.PIX_FRAC * 64)) == 64           # at 8 x 8 the share bound asks for every pixel
    GH.assert_close(_off_by(ref, [(y, x) for y in range(8) for x in range(8)], 0.5e-4), ref, "64 of 64 within PIX_TOL")


def test_close_raises_on_one_bad_pixel_of_64():
    ref = _image()
    with pytest.raises(AssertionError, match="frac_ok=0.98438"):        # 63 / 64 < PIX_FRAC
        GH.assert_close(_off_by(ref, [(4, 4)], 1.0), ref, "one of 64")


def test_close_raises_on_nan():
    ref = _image()
    gpu = ref.copy()
    gpu[0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        GH.assert_close(gpu, ref, "NaN")


def test_close_both_arms_at_16x16():
    """one bad pixel of 256 has the share 0.9961 >= PIX_FRAC, so the mean decides: 256 x MEAN_TOL in that pixel"""
    ref = _image(16, 16)
    assert 255 / 256 >= GH.PIX_FRAC
    GH.assert_close(_off_by(ref, [(9, 3)], 0.9 * 256 * GH.MEAN_TOL), ref, "mean below MEAN_TOL")
    with pytest.raises(AssertionError, match="frac_ok=0.99609"):
        GH.assert_close(_off_by(ref, [(9, 3)], 1.1 * 256 * GH.MEAN_TOL), ref, "mean above MEAN_TOL")
    with pytest.raises(AssertionError):                                 # two bad pixels: the share arm, 254 / 256
        GH.assert_close(_off_by(ref, [(9, 3), (0, 0)], 2e-4), ref, "share below PIX_FRAC")


def test_close_prints_with_a_tag(capsys):
    ref = _image()
    GH.assert_close(ref.copy(), ref, "quiet")
    assert capsys.readouterr().out == ""
    GH.assert_close(ref.copy(), ref, "loud", tag="t")
    assert capsys.readouterr().out.startswith("[t] loud: 0 of 64 pixels not bit-identical")


# ---------------------------------------------------------------- assert_same_render
def _render(seed=1):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0, 1, (8, 8, 19)).astype(np.float32)
    g[..., GH.TYPE_COL] = 2.0
    g[0, 0, 15] = np.nan                                  # a NaN shininess, equal to itself here
    return GH.Render([_image(seed=seed), _image(seed=seed + 1)], g, rng.uniform(0, 1, (8, 8, 12)).astype(np.float32))


def _changed(r, frames=None, gbuffer=None, reservoirs=None):
    f = [a.copy() for a in r.frames]
    g, s = r.gbuffer.copy(), r.reservoirs.copy()
    for part, at in ((f[1] if frames else None, frames), (g, gbuffer), (s, reservoirs)):
        if at is not None:
            part[at] += np.float32(1.0)
    return GH.Render(f, g, s)


def test_same_render():
    a = _render()
    GH.assert_same_render(a, _render(), "equal, NaN on both sides")
    with pytest.raises(AssertionError, match=r"^frames: frame 1: 1 pixels$"):
        GH.assert_same_render(a, _changed(a, frames=(2, 3, 0)), "frames")
    with pytest.raises(AssertionError, match=r"^res: reservoirs: columns \[11\] on 1 pixels$"):
        GH.assert_same_render(a, _changed(a, reservoirs=(7, 7, 11)), "res")
    with pytest.raises(AssertionError, match=r"^gb: G-buffer: columns \[18\] on 1 pixels$"):
        GH.assert_same_render(a, _changed(a, gbuffer=(5, 0, 18)), "gb")
    one_sided = a.gbuffer.copy()
    one_sided[0, 0, 15] = 4.0                             # a NaN on one side only
    with pytest.raises(AssertionError, match=r"columns \[15\] on 1 pixels"):
        GH.assert_same_render(a, GH.Render(a.frames, one_sided, a.reservoirs), "NaN")


def test_same_render_type_column():
    a = _render()
    b = _changed(a, gbuffer=(slice(None), slice(None), GH.TYPE_COL))
    with pytest.raises(AssertionError, match=rf"columns \[{GH.TYPE_COL}\] on 64 pixels"):
        GH.assert_same_render(a, b, "types", type_column=True)
    GH.assert_same_render(a, b, "types", type_column=False)
    with pytest.raises(AssertionError):                                 # the other columns still count
        GH.assert_same_render(a, _changed(b, gbuffer=(5, 0, 18)), "types", type_column=False)


def test_render_is_read_only():
    with pytest.raises(ValueError):
        _render().frames[0][0, 0, 0] = 1.0


# ---------------------------------------------------------------- set_env
def test_set_env_sets_deletes_and_restores():
    os.environ["RESTIR_HARNESS_A"] = "before"
    os.environ.pop("RESTIR_HARNESS_B", None)
    try:
        with pytest.MonkeyPatch.context() as mp:
            GH.set_env(mp, RESTIR_HARNESS_A=None, RESTIR_HARNESS_B="on", RESTIR_HARNESS_C=None)
            assert "RESTIR_HARNESS_A" not in os.environ and "RESTIR_HARNESS_C" not in os.environ
            assert os.environ["RESTIR_HARNESS_B"] == "on"
            GH.set_env(mp, RESTIR_HARNESS_A="during")
            assert os.environ["RESTIR_HARNESS_A"] == "during"
        assert os.environ["RESTIR_HARNESS_A"] == "before" and "RESTIR_HARNESS_B" not in os.environ
    finally:
        del os.environ["RESTIR_HARNESS_A"]


# ---------------------------------------------------------------- with_ceiling_blocker
def test_ceiling_blocker_adds_two_triangles_and_one_material():
    sc = scenes.cornell_many_lights(64)
    out = GH.with_ceiling_blocker(sc, "blocked")
    n = sc.n_tris
    assert out.n_tris == n + 2 and len(out.materials) == len(sc.materials) + 1 and out.name == "blocked"
    assert np.array_equal(out.positions[:n], sc.positions) and np.array_equal(out.normals[:n], sc.normals)
    assert np.array_equal(out.tri_material[:n], sc.tri_material)
    assert list(out.materials[:-1]) == list(sc.materials)
    quad = np.asarray(out.positions[n:], np.float32).reshape(2, 3, 3)
    assert (quad[..., 2] == np.float32(1.98)).all() and (np.abs(quad[..., :2]) == np.float32(0.97)).all()
    assert (np.asarray(out.normals[n:]).reshape(2, 3, 3) == [0, 0, -1]).all()
    assert (out.tri_material[n:] == len(sc.materials)).all()
    new = out.materials[-1]
    assert new.type == scenes.LAMBERT and tuple(new.kd) == (0.73, 0.73, 0.73) and not any(new.le)


def test_orbit_cam_is_the_walk_tests_orbit():
    sc = scenes.cornell_many_lights(64)
    a, b = GH.orbit_cam(sc, 5), scenes.orbit_camera(sc.camera, 5, 48, 0.2)
    assert np.array_equal(np.asarray(a.as_array()), np.asarray(b.as_array()))
