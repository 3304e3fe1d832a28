"""The denoiser (csrc/rs_denoise.hip) on the inputs real frames hold and tests/test_gpu_denoise.py never draws:
exact zeros, NaN, +-Inf, negative colour, colour past the half-float range, albedo and normals outside their
intervals, zero normals, whole black bins, portrait sizes -- tests/denoise_cases.py plants them at the image corners,
on the padding boundary, on both sides of a bin boundary and inside.

What is pinned:
  * the auto-exposure against its float64 definition (rel 1e-4: float32 luminance, log2 and sums on the GPU), over
    one-bin, exactly-256-pixel, uneven and many-bin sizes, for benign, hostile and black images;
  * the sanitisation is invisible: an image and its sanitised copy give the same bits in the scale, in all 16 dumped
    tensors and in the output -- one +Inf channel used to take the scale to 0 and the whole frame to black;
  * the network input per element, the planted pixels exactly; every tensor finite; every layer against float64 with
    test_gpu_denoise.py's bound (its body, shared); end to end against the reference;
  * no state survives a change of size; the frame path (accumulator and G-buffer at their own strides) equals the
    image path bit for bit; a rejected call leaves the denoiser working.
An end-to-end case first asserts the condition on its INPUT (denoise_cases.assert_scale_in_range) before any GPU
result is read.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from restir_amd import Renderer, metric_params, scenes, tza  # noqa: E402
from restir_amd.denoise import DenoiseParams, Denoiser  # noqa: E402
from restir_amd.renderer import RS_E_INVALID, RS_E_UNSUPPORTED, RS_OK  # noqa: E402

import denoise_cases as C  # noqa: E402
import denoise_ref as ref  # noqa: E402  (oracle/, test infrastructure)
from gpu_harness import bits  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    r = Renderer(64, 48)
    w = tza.random_unet_weights(seed=7)
    d = Denoiser(r, w)
    yield r, d, w
    d.close()
    r.close()


def _run_all(d, images, scale=None):
    """(output, scale, the 16 dumped tensors with their borders and channel padding) of one execute."""
    out = C.run(d, *images, scale=scale)
    return out, np.float32(d.scale()), [d.dump(i)[0] for i in range(16)]


def _assert_same(a, b, what):
    (oa, sa, ta), (ob, sb, tb) = a, b
    assert sa.tobytes() == sb.tobytes(), (what, sa, sb)
    for i in range(16):
        assert ta[i].shape == tb[i].shape and np.array_equal(bits(ta[i]), bits(tb[i])), f"{what}: tensor {i}"
    assert np.array_equal(bits(oa), bits(ob)), f"{what}: output"


def _class_image(cls, H, W):
    """One of the three image classes of the scale test (hostile: +Inf planted at every size)."""
    if cls == "benign":
        return C.benign_images(H, W, seed=H * 100 + W)
    color, albedo, normal = C.hostile_images(H, W, seed=H * 100 + W)
    return (np.zeros_like(color) if cls == "black" else color), albedo, normal


@pytest.mark.parametrize("cls", ["benign", "hostile", "black"])
@pytest.mark.parametrize("H,W", C.AE_SHAPES)
def test_scale_matches_definition(ctx, H, W, cls):
    r, d, w = ctx
    images = _class_image(cls, H, W)
    want = C.autoexposure64(images[0])
    C.run(d, *images)                                       # input_scale unset: auto-exposure
    got = d.scale()
    print(f"{H}x{W} {cls}: scale {got!r}, float64 definition {want!r}, rel {abs(got - want) / want:.2e}")
    if cls == "black":
        assert want == 1.0 and got == 1.0
    else:
        # float32 bin sums: test_autoexposure_matches_reference's bound (not pytest.approx: its absolute 1e-12 would
        # pass any scale this small)
        assert abs(got - want) <= 1e-4 * want, (H, W, got, want)


@pytest.mark.parametrize("scale", [0.8, None], ids=["scale0.8", "auto"])
@pytest.mark.parametrize("H,W", [(33, 21), (47, 33)])
def test_sanitisation_is_invisible(ctx, H, W, scale):
    r, d, w = ctx
    images = C.hostile_images(H, W, seed=H + W, scale=scale or 1.0)
    clean = C.sanitised(*images)
    assert any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(images, clean))
    s64 = C.assert_scale_in_range(images[0])
    a = _run_all(d, images, scale)
    b = _run_all(d, clean, scale)
    _assert_same(a, b, f"{H}x{W} hostile against sanitised")
    if scale is None:
        assert abs(float(a[1]) - s64) <= 1e-4 * s64, (float(a[1]), s64)
    assert a[0].max() > 0.0                                # not the black frame of a zero scale


@pytest.mark.parametrize("H,W", [(33, 21), (47, 33)])
def test_network_input(ctx, H, W):
    r, d, w = ctx
    scale = 0.8
    color, albedo, normal = C.hostile_images(H, W, seed=7 * H, scale=scale)
    C.run(d, color, albedo, normal, scale=scale)
    a, real = d.dump(0)
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    assert a.shape == (Hp + 2, Wp + 2, 16) and real == 9
    got = a[1:-1, 1:-1, :9].astype(np.float64).transpose(2, 0, 1)
    with np.errstate(all="ignore"):
        want = ref.preprocess(color, albedo, normal, np.float32(scale), 9).astype(np.float16)
    ulp = np.abs(np.spacing(want)).astype(np.float64)      # of each element
    diff = np.abs(got - want.astype(np.float64))
    assert np.isfinite(a).all()
    assert (diff <= ulp).all(), float((diff / ulp).max())
    checked = 0
    for y, x, im, val, exp in C.hostile_plan(H, W, scale):
        for k in range(3):
            if exp[k] is not None:
                assert got[3 * im + k, y, x] == exp[k], (y, x, im, k, val, got[3 * im + k, y, x])
                checked += 1
    assert checked >= 90
    B = C.bins(H, W)
    (y0, y1, x0, x1), = [B[b] for b, v in C.constant_bins(H, W).items() if v == 0.0]
    assert not got[0:3, y0:y1, x0:x1].any()               # the black bin
    assert not got[:, H:].any() and not got[:, :, W:].any(), "padding region"
    assert not a[0].any() and not a[-1].any() and not a[:, 0].any() and not a[:, -1].any(), "border"
    assert not a[..., 9:].any(), "channel padding"


def test_finite_everywhere(ctx):
    r, d, w = ctx
    for scale in (0.8, None):
        images = C.hostile_images(47, 33, seed=11, scale=scale or 1.0)
        C.assert_scale_in_range(images[0])
        out, s, tensors = _run_all(d, images, scale)
        assert np.isfinite(s) and s > 0
        for i, t in enumerate(tensors):
            assert np.isfinite(t).all(), f"tensor {i}"
        assert np.isfinite(out).all() and (out >= 0).all() and out.max() > 0


@pytest.mark.parametrize("H,W,fill", [pytest.param(H, W, fill, id=f"{H}-{W}" + ("-fill" + fill if fill else ""))
                                      for H, W in C.LAYER_SHAPES for fill in (None, "1")])
def test_every_layer_matches_float64_hostile(ctx, monkeypatch, H, W, fill):
    """test_gpu_denoise.py's per-convolution bound (1 float16 ulp + 3e-5 x magnitude, at most 2 % of the elements
    different) on hostile portrait images."""
    r, d, w = ctx
    got, dumps = C.check_every_layer(r, d, w, monkeypatch, C.hostile_images(H, W, seed=31 + H, scale=0.9), fill)
    for i, (a, real) in enumerate(dumps):
        assert np.isfinite(a).all(), f"tensor {i}"
    assert np.isfinite(got).all() and (got >= 0).all()


def test_end_to_end_hostile(ctx):
    r, d, w = ctx
    color, albedo, normal = C.hostile_images(47, 33, seed=5)
    C.assert_scale_in_range(color)
    with np.errstate(all="ignore"):
        want = ref.denoise(color, albedo, normal, w, quantize=True)
        s = ref.autoexposure(color)
    got = C.run(d, color, albedo, normal)
    assert np.isfinite(got).all() and (got >= 0).all() and got.max() > 0
    m, x = C.pu_err(got, want, s)
    print(f"hostile 47x33, auto-exposure {float(s):.3e}: PU-domain |err| mean {m:.2e} max {x:.2e}")
    assert m <= 1e-3 and x <= 2e-2, (m, x)


def test_no_stale_state_across_sizes(ctx):
    """One denoiser over 83x37, 1x1, 33x21, 83x37: every output and tensor (zero borders and channel padding included)
    is what a fresh denoiser gives for that size."""
    r, _, w = ctx
    d = Denoiser(r, w)
    runs = []
    try:
        for H, W in ((83, 37), (1, 1), (33, 21), (83, 37)):
            images = C.hostile_images(H, W, seed=3, scale=0.8, inf=False)
            for scale in (0.8, None):
                if scale is None:
                    C.assert_scale_in_range(images[0])
                got = _run_all(d, images, scale)
                fresh = Denoiser(r, w)
                try:
                    want = _run_all(fresh, images, scale)
                finally:
                    fresh.close()
                _assert_same(got, want, f"{H}x{W} scale {scale}: reused against fresh")
                runs.append(got)
    finally:
        d.close()
    _assert_same(runs[0], runs[6], "83x37, first against last")
    _assert_same(runs[1], runs[7], "83x37 auto-exposure, first against last")


def test_frame_path_equals_image_path():
    """rs_denoise_frame reads the accumulator (3 floats per pixel) and the G-buffer's kd and normal (4 floats per
    pixel) in place; execute() reads contiguous copies of the same values: the same bits.  r.gbuffer() copies the
    G-buffer's floats unconverted (rs_dump_gbuffer) and post_frame(accumulate=False) makes the accumulator the frame,
    so the values fed in are the same and no tolerance applies.  This frame's misses and lights carry a zero normal
    and a zero albedo; it has no black bin (the hostile images have)."""
    W, H = 50, 38
    r = Renderer(W, H)
    sc = scenes.cornell_many_lights(64)
    s = r.load_scene(sc)
    d = Denoiser(r, tza.random_unet_weights(seed=21))
    try:
        frame = r.produce_restir(s, sc.camera, metric_params(m_area=8), 0).copy()
        r.post_frame(accumulate=False, stats=False)          # accumulator = the frame
        C.assert_scale_in_range(frame)
        out = d.frame_output().copy()
        a = (out, np.float32(d.scale()), [d.dump(i)[0] for i in range(16)])
        g = r.gbuffer()
        normal, kd = np.ascontiguousarray(g[..., 3:6]), np.ascontiguousarray(g[..., 6:9])
        assert np.isfinite(frame).all() and (normal == 0).all(-1).any() and (kd == 0).all(-1).any()
        b = _run_all(d, (frame, kd, normal))
        _assert_same(a, b, "frame path against image path")
        s64 = C.autoexposure64(frame)
        assert abs(float(a[1]) - s64) <= 1e-4 * s64, (float(a[1]), s64)
    finally:
        d.close()
        s.close()
        r.close()


def test_loud_errors_leave_the_denoiser_working(ctx):
    """The C ABI's rejections (ctypes: the wrapper always sends hdr = 1 and its own sizes), each followed by a 16x16
    execute that gives the bits it gave before."""
    r, d, w = ctx
    lib = d.lib
    images = C.benign_images(16, 16, seed=4)
    before = _run_all(d, images, 0.8)
    want = ref.denoise(*images, w, input_scale=0.8, quantize=True)
    m, x = C.pu_err(before[0], want, 0.8)
    assert m <= 1e-3 and x <= 2e-2, (m, x)

    dev = [torch.from_numpy(a).cuda() for a in images]
    out = torch.empty_like(dev[0])
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731

    def call(color, albedo, normal, W, H, hdr=1):
        prm = DenoiseParams(0.8, hdr)
        return lib.rs_denoiser_execute(d.h, p(color), p(albedo), p(normal), p(out), W, H, ctypes.byref(prm))

    cases = [("normal=None", lambda: call(dev[0], dev[1], None, 16, 16), RS_E_INVALID, "normal"),
             ("albedo=None", lambda: call(dev[0], None, dev[2], 16, 16), RS_E_INVALID, "albedo"),
             ("hdr=0", lambda: call(dev[0], dev[1], dev[2], 16, 16, hdr=0), RS_E_UNSUPPORTED, "hdr"),
             ("width 0", lambda: call(dev[0], dev[1], dev[2], 0, 16), RS_E_INVALID, "empty"),
             ("height 0", lambda: call(dev[0], dev[1], dev[2], 16, 0), RS_E_INVALID, "empty")]
    for name, f, code, word in cases:
        rc = f()
        assert rc == code and rc != RS_OK, (name, rc)
        assert word in lib.rs_last_error(r.h).decode(), (name, lib.rs_last_error(r.h).decode())
        _assert_same(_run_all(d, images, 0.8), before, f"after {name}")
