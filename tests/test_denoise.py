"""CPU tests of the denoiser's host side: the tensor-archive format, the C ABI's
host-only weight check (topology, error messages), and properties of the fp32 reference
(oracle/denoise_ref.py) the GPU tests compare against.  No device work."""
import struct

import numpy as np
import pytest

from restir_amd import tza
from restir_amd.denoise import check_weights
from restir_amd.renderer import RestirError

import denoise_cases as C  # the hostile images and the float64 definitions, shared with the GPU tests
import denoise_ref as ref  # oracle/ (test infrastructure)


@pytest.fixture(scope="module")
def weights():
    return tza.random_unet_weights(seed=3)


@pytest.mark.parametrize("dtype", ["f", "h"])
def test_tza_round_trip(weights, dtype):
    blob = tza.write_tza(weights, dtype)
    back = tza.read_tza(blob)
    assert list(back) == list(weights)
    for k, v in weights.items():
        want = v if dtype == "f" else v.astype(np.float16).astype(np.float32)
        np.testing.assert_array_equal(back[k], want)


def test_check_weights_reports_topology(weights):
    info = check_weights(tza.write_tza(weights))
    shapes = tza.unet_shapes(9)
    assert info.input_channels == 9
    assert list(info.channels) == [shapes[n][0] for n in ref.LAYERS]
    params = sum(o * i * 9 + o for o, i in shapes.values())
    assert info.parameters == params
    # MAC per padded input pixel: a layer at pooling level l runs on 1/4^l of the pixels
    levels = [0, 0, 1, 2, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0]
    mac = sum(shapes[n][0] * shapes[n][1] * 9 / 4 ** lv for n, lv in zip(ref.LAYERS, levels))
    assert info.mac_per_pixel == pytest.approx(mac)
    assert 1.0e5 < mac < 1.5e5


def test_check_weights_other_input_sets():
    for ic in (3, 6):
        assert check_weights(tza.write_tza(tza.random_unet_weights(seed=1, ic=ic))).input_channels == ic


def test_check_weights_rejects_malformed(weights):
    blob = tza.write_tza(weights)
    with pytest.raises(RestirError, match="magic"):
        check_weights(b"\x00\x00" + blob[2:])
    with pytest.raises(RestirError, match="version"):
        check_weights(blob[:2] + b"\x03" + blob[3:])
    with pytest.raises(RestirError):
        check_weights(blob[:40])
    w = dict(weights)
    del w["dec_conv2b.bias"]
    with pytest.raises(RestirError, match="dec_conv2b.bias"):
        check_weights(tza.write_tza(w))
    w = dict(weights)
    w["dec_conv3a.weight"] = w["dec_conv3a.weight"][:, :100]
    with pytest.raises(RestirError, match="dec_conv3a"):
        check_weights(tza.write_tza(w))
    w = dict(weights)
    w["dec_conv0.weight"] = np.zeros((4, 32, 3, 3), np.float32)
    w["dec_conv0.bias"] = np.zeros(4, np.float32)
    with pytest.raises(RestirError, match="dec_conv0"):
        check_weights(tza.write_tza(w))
    # a table entry pointing past the end of the blob
    magic, major, minor, toff = struct.unpack_from("<HBBQ", blob, 0)
    bad = bytearray(blob)
    struct.pack_into("<Q", bad, 4, len(blob) + 100)
    with pytest.raises(RestirError, match="table"):
        check_weights(bytes(bad))


def test_pu_transfer_round_trip():
    y = np.concatenate([np.geomspace(1e-8, 65504, 2000), [0.0, ref.PU_Y0, ref.PU_Y1]]).astype(np.float32)
    x = ref.pu_forward(y)
    assert np.all(np.diff(x[:2000]) > 0)                              # monotone
    np.testing.assert_allclose(ref.pu_inverse(x), y, rtol=2e-5, atol=1e-12)
    assert float(ref.pu_forward(np.float32(65504.0)) * ref.NORM_SCALE) == pytest.approx(1.0, abs=1e-6)


def test_autoexposure_constant_and_bins():
    img = np.full((40, 50, 3), 2.0, np.float32)
    assert float(ref.autoexposure(img)) == pytest.approx(0.18 / 2.0, rel=1e-6)
    dark = np.zeros((40, 50, 3), np.float32)
    assert float(ref.autoexposure(dark)) == 1.0                        # every bin below eps
    half = img.copy()
    half[:, :25] = 0.0                                                 # bins at zero are skipped
    assert float(ref.autoexposure(half)) == pytest.approx(0.18 / 2.0, rel=1e-6)


def _class_image(cls, H, W):
    """Colour of one of the three image classes of the scale tests (hostile: +Inf planted at every size)."""
    if cls == "black":
        return np.zeros((H, W, 3), np.float32)
    make = C.benign_images if cls == "benign" else C.hostile_images
    return make(H, W, seed=H * 100 + W)[0]


@pytest.mark.parametrize("cls", ["benign", "hostile", "black"])
@pytest.mark.parametrize("H,W", C.AE_SHAPES)
def test_autoexposure_matches_definition(H, W, cls):
    """ref.autoexposure against the float64 definition (denoise_cases.autoexposure64), rel 1e-6: the reference takes
    a pixel's luminance in float32 (3 roundings of 6e-8) and sums a bin in float64.

    Its log2 sum is float32 too: a bin holding 1e30 or +Inf (FLT_MAX once sanitised) has log2 L of 90 to 127,
    where float32 values are spaced 7.6e-6, and 0.18 / 2**(s / n) carries ln 2 times the error of s / n -- summed
    plainly that costs 1.7e-6 to 4.8e-6 on four of the hostile images.  The reference therefore takes the exponent of
    a bin mean >= 2**32 out exactly (frexp) before the float32 log2; measured now: hostile <= 9.7e-8, benign <= 7.3e-8,
    black exactly 1.  The parent's reference returns 1.0, 6e-12 or 0.0 on the seven hostile images."""
    color = _class_image(cls, H, W)
    with np.errstate(all="ignore"):
        got = float(ref.autoexposure(color))
    want = C.autoexposure64(color)
    print(f"{H}x{W} {cls}: reference {got!r}, float64 definition {want!r}, rel {abs(got - want) / want:.2e}")
    if cls == "black":
        assert got == 1.0 and want == 1.0
    else:
        assert got > 0.0 and np.isfinite(got)
        assert abs(got - want) <= 1e-6 * want, (got, want)       # float32 luminance, float64 bin sums


@pytest.mark.parametrize("H,W", C.AE_SHAPES)
def test_autoexposure_of_sanitised_is_bit_identical(H, W):
    color, albedo, normal = C.hostile_images(H, W, seed=5)
    with np.errstate(all="ignore"):
        a = ref.autoexposure(color)
    b = ref.autoexposure(C.sanitised(color, albedo, normal)[0])
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), (a, b)


def _autoexposure_plain(color):
    """The reference's arithmetic without its range reduction: float32 luminance, float64 bin sums, a float32 mean,
    float32 log2 values summed in float32, float32 power and quotient."""
    c = np.asarray(color, np.float32)
    lum = (np.float32(0.212671) * c[..., 0] + np.float32(0.715160) * c[..., 1] + np.float32(0.072169) * c[..., 2])
    s, n = np.float32(0.0), 0
    for y0, y1, x0, x1 in C.bins(*c.shape[:2]):
        L = np.float32(lum[y0:y1, x0:x1].astype(np.float64).sum()) / np.float32((y1 - y0) * (x1 - x0))
        if L > np.float32(1e-8):
            s += np.float32(np.log2(np.float64(L)))
            n += 1
    return np.float32(0.18) / np.float32(2.0 ** (s / n)) if n else np.float32(1.0)


@pytest.mark.parametrize("gain", [1e-6, 1.0, 1e8])
def test_autoexposure_keeps_its_bits_below_the_range_reduction(gain):
    """On finite, non-negative images whose bin means stay below 2**32 neither the sanitisation nor the range
    reduction takes part: the scale is, bit for bit, the plain float32 arithmetic's."""
    for seed, (H, W) in enumerate(C.AE_SHAPES + C.LAYER_SHAPES + ((40, 50),)):
        color = C.benign_images(H, W, seed)[0] * np.float32(gain)
        if seed % 2:
            color[: H // 2] = 0.0
        assert float(C.autoexposure64(color)) * float(gain) < 1e3          # bin means of order `gain`
        assert ref.autoexposure(color).tobytes() == _autoexposure_plain(color).tobytes(), (H, W, gain)


def test_autoexposure_bin_of_flt_max_does_not_overflow():
    """Several FLT_MAX pixels in one bin are legal input: the bin's mean is FLT_MAX, not inf."""
    img = np.full((16, 32, 3), 1.0, np.float32)
    img[:, :16] = C.FLT_MAX                                           # bin 0: 256 pixels at FLT_MAX; bin 1: 1.0
    got = float(ref.autoexposure(img))
    want = C.autoexposure64(img)
    exact = 0.18 / 2.0 ** 64                                          # geometric mean of 2**128 and 1
    assert abs(want - exact) <= 1e-6 * exact and abs(got - want) <= 1e-6 * want, (got, want, exact)


@pytest.mark.parametrize("H,W", C.LAYER_SHAPES + ((47, 33),))
def test_hostile_plan_plants_every_value(H, W):
    """The case module itself: at the sizes used end to end every listed value reaches a pixel, +Inf stays in one
    bin, the constant bins are constant, and the auto-exposure is in range (the condition on the inputs)."""
    color, albedo, normal = C.hostile_images(H, W, seed=1, scale=0.8)
    plan = C.hostile_plan(H, W, 0.8)
    for im, values in ((0, C.color_values(0.8)), (1, C.ALBEDO_VALUES), (2, C.NORMAL_VALUES)):
        planted = {repr(p[3]) for p in plan if p[2] == im}
        assert planted >= {repr(v) for v, _ in values}, (im, planted)
    ys, xs = np.nonzero(np.isposinf(color).any(-1))
    assert len(ys) == 1
    B = C.bins(H, W)
    for b, v in C.constant_bins(H, W).items():
        y0, y1, x0, x1 = B[b]
        assert (color[y0:y1, x0:x1] == np.float32(v)).all()
    assert sorted(C.constant_bins(H, W).values()) == sorted(C.BIN_VALUES)
    C.assert_scale_in_range(color)
    rows, cols = {p[0] for p in plan}, {p[1] for p in plan}
    assert {0, H - 1} <= rows and {0, W - 1} <= cols                  # the padding boundary is planted


@pytest.mark.parametrize("H,W", C.LAYER_SHAPES)
def test_preprocess_at_planted_pixels(H, W):
    scale = np.float32(0.8)
    color, albedo, normal = C.hostile_images(H, W, seed=2, scale=0.8)
    with np.errstate(all="ignore"):
        x = ref.preprocess(color, albedo, normal, scale, 9)
    assert np.isfinite(x).all() and x.min() >= 0.0 and x.max() <= 1.0
    assert not x[:, H:].any() and not x[:, :, W:].any()               # the padding
    top = float(ref.pu_forward(np.float32(65504.0)) * ref.NORM_SCALE)
    const = C.constant_bins(H, W)
    checked = 0
    for y, x_, im, val, exp in C.hostile_plan(H, W, 0.8):
        for k in range(3):
            if exp[k] is None:
                continue
            want = top if (im == 0 and exp[k] == 1.0) else exp[k]
            assert float(x[3 * im + k, y, x_]) == want, (y, x_, im, k, val, float(x[3 * im + k, y, x_]), want)
            checked += 1
    assert checked >= 3 * 30
    B = C.bins(H, W)
    for b, v in const.items():                                        # the constant bins: PU of the scaled constant
        y0, y1, x0, x1 = B[b]
        want = ref.pu_forward(np.float32(v) * scale) * ref.NORM_SCALE
        assert (x[0:3, y0:y1, x0:x1] == want).all()


@pytest.mark.parametrize("scale", [0.8, None])
def test_denoise_of_sanitised_is_bit_identical(weights, scale):
    H, W = 33, 21
    color, albedo, normal = C.hostile_images(H, W, seed=3, scale=scale or 1.0)
    C.assert_scale_in_range(color)
    with np.errstate(all="ignore"):
        a, ya, sa = ref.denoise(color, albedo, normal, weights, input_scale=scale, quantize=True,
                                return_network_output=True)
    b, yb, sb = ref.denoise(*C.sanitised(color, albedo, normal), weights, input_scale=scale, quantize=True,
                            return_network_output=True)
    assert np.float32(sa).tobytes() == np.float32(sb).tobytes()
    assert np.isfinite(a).all() and (a >= 0).all() and a.max() > 0.0
    assert ya.tobytes() == yb.tobytes() and a.tobytes() == b.tobytes()


def test_reference_shapes_and_quantised_close(weights):
    rng = np.random.default_rng(0)
    H, W = 21, 35
    color = rng.lognormal(0.0, 1.0, (H, W, 3)).astype(np.float32)
    albedo = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    n = rng.standard_normal((H, W, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    a = ref.denoise(color, albedo, n, weights)
    b = ref.denoise(color, albedo, n, weights, quantize=True)
    assert a.shape == (H, W, 3) and np.isfinite(a).all() and (a >= 0).all()
    rel = np.abs(a - b).sum() / np.abs(a).sum()
    assert rel < 2e-2, rel
