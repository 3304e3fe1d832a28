"""The denoiser's hostile inputs: images, shapes and float64 definitions shared by tests/test_denoise.py (the CPU
reference, oracle/denoise_ref.py) and tests/test_gpu_denoise_inputs.py (csrc/rs_denoise.hip).  TEST
INFRASTRUCTURE ONLY; the images and definitions import nothing from denoise_ref, so a mistake there is not repeated here
(the GPU tests' shared steps at the end do use it: they compare against it).

Real frames are not lognormal: a Cornell frame is mostly exact zeros, a primary miss carries a zero normal, and a
bad material can put Inf or NaN into a pixel's radiance.  What the denoiser promises for them:
  * colour is read as NaN -> 0, then clamped to [0, FLT_MAX] -- by the auto-exposure and (after the scale, to
    65504) by the input transform; albedo as NaN -> 0, [0, 1]; normal as NaN -> 0, [-1, 1];
  * so an image and its `sanitised` copy give the same bits everywhere (scale, every tensor, output).

  benign_images(H, W, seed)       lognormal colour, uniform albedo, unit normals (what the older tests draw)
  hostile_plan(H, W, scale, inf)  the planted pixels: (y, x, image, values, expected network input or None)
  hostile_images(H, W, seed, ..)  benign_images with the plan applied and, from four bins on, three constant bins
  sanitised(color, albedo, normal)
  autoexposure64(color)           the auto-exposure from its definition, in float64
  assert_scale_in_range(color)    the condition on an end-to-end case (see there)
  run, pu_err, check_every_layer  one execute on the GPU, the PU-domain error, the per-convolution comparison
"""
from __future__ import annotations

import math

import numpy as np

NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)

# one bin of fewer than 256 pixels, one of exactly 256, uneven bins of 8 and 9 rows / columns, 6 and 9 bins
AE_SHAPES = ((1, 1), (15, 15), (16, 16), (17, 16), (16, 17), (33, 21), (47, 33))
# portrait, neither side a multiple of 16
LAYER_SHAPES = ((33, 21), (83, 37))

# the constant bins of an image with at least four bins: exact zeros, below the 1e-8 threshold, above it
BIN_VALUES = (0.0, 1e-9, 1e-7)
SCALE_RANGE = (1e-30, 1e30)


def benign_images(H, W, seed=0):
    rng = np.random.default_rng(seed)
    color = rng.lognormal(-0.5, 1.2, (H, W, 3)).astype(np.float32)
    albedo = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    n = rng.standard_normal((H, W, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return color, albedo, n


def bins(H, W):
    """[(y0, y1, x0, x1)] of the ceil(H/16) x ceil(W/16) auto-exposure bins, row-major."""
    nbh, nbw = -(-H // 16), -(-W // 16)
    return [(i * H // nbh, (i + 1) * H // nbh, j * W // nbw, (j + 1) * W // nbw)
            for i in range(nbh) for j in range(nbw)]


def _bin_of(H, W, y, x):
    for b, (y0, y1, x0, x1) in enumerate(bins(H, W)):
        if y0 <= y < y1 and x0 <= x < x1:
            return b
    raise AssertionError((y, x))


def constant_bins(H, W):
    """{bin index: constant colour} from four bins on: the three bins holding the fewest planted pixels (the first
    such in row-major order), so that the colour values keep enough pixels of their own."""
    nb = len(bins(H, W))
    if nb < 4:
        return {}
    load = [0] * nb
    for y, x in positions(H, W):
        load[_bin_of(H, W, y, x)] += 1
    return dict(zip(sorted(sorted(range(nb), key=lambda b: load[b])[:3]), BIN_VALUES))


def positions(H, W):
    """The planted pixels in a fixed order, without repeats: the four corners, the last row and the last column (the
    padding boundary), both sides of the first bin boundary in each direction, one interior pixel."""
    nbh, nbw = -(-H // 16), -(-W // 16)
    yb, xb = (H // nbh if nbh > 1 else H // 2), (W // nbw if nbw > 1 else W // 2)    # bin 1 starts here
    p = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    p += [(H - 1, W // 4), (H - 1, W // 2), (H - 1, 3 * W // 4)]
    p += [(H // 4, W - 1), (H // 2, W - 1), (3 * H // 4, W - 1)]
    p += [(yb - 1, W // 3), (yb, W // 3), (H // 3, xb - 1), (H // 3, xb)]
    p += [(H // 2 + 1, W // 2 + 1)]
    out = []
    for y, x in p:
        q = (min(max(y, 0), H - 1), min(max(x, 0), W - 1))
        if q not in out:
            out.append(q)
    return out


def color_values(scale, inf=True):
    """(planted colour, expected network input): per channel None = left as it is / not a closed form.  1.0 stands for
    pu_forward(65504) * NORM_SCALE, which is 1 in float16."""
    big = 70000.0 / scale                      # above the half-float range once scaled
    v = [((NAN, None, None), (0.0, None, None)),
         ((NAN, NAN, NAN), (0.0, 0.0, 0.0)),
         ((None, INF, None), (None, 1.0, None)),
         ((-INF, -INF, -INF), (0.0, 0.0, 0.0)),
         ((-3.0, -3.0, -3.0), (0.0, 0.0, 0.0)),
         ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
         ((1e-40, 1e-40, 1e-40), (None, None, None)),          # a float32 subnormal: tiny, not a closed form
         ((1e30, 1e30, 1e30), (1.0, 1.0, 1.0)),
         ((big, big, big), (1.0, 1.0, 1.0))]
    return v if inf else v[:2] + v[3:]


ALBEDO_VALUES = [((NAN, NAN, NAN), (0.0, 0.0, 0.0)), ((INF, INF, INF), (1.0, 1.0, 1.0)),
                 ((-INF, -INF, -INF), (0.0, 0.0, 0.0)), ((-0.5, -0.5, -0.5), (0.0, 0.0, 0.0)),
                 ((1.5, 1.5, 1.5), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                 ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0)), ((NAN, 0.25, None), (0.0, 0.25, None))]
NORMAL_VALUES = [((NAN, NAN, NAN), (0.5, 0.5, 0.5)), ((INF, INF, INF), (1.0, 1.0, 1.0)),
                 ((-INF, -INF, -INF), (0.0, 0.0, 0.0)), ((5.0, 5.0, 5.0), (1.0, 1.0, 1.0)),
                 ((-5.0, -5.0, -5.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5)),      # a primary miss
                 ((0.5, -2.0, 1.0), (0.75, 0.0, 1.0))]                                           # not unit length


def hostile_plan(H, W, scale=1.0, inf=True):
    """[(y, x, image, values, expected)]: image 0 colour / 1 albedo / 2 normal; `values` three floats or None (channel
    untouched); `expected` the network input of that pixel's three channels, None where no closed form is claimed.
    Colour goes only to pixels outside the constant bins, the single +Inf (one channel) to one pixel, so to one bin;
    the values cycle over the positions, so from 9 free positions on every value is planted."""
    const = constant_bins(H, W)
    pos = positions(H, W)
    plan = []
    cv, seen_inf = color_values(scale, inf), False
    free = [p for p in pos if _bin_of(H, W, *p) not in const]
    for i, (y, x) in enumerate(free):
        val, exp = cv[i % len(cv)]
        if INF in val:
            if seen_inf:
                val, exp = cv[4]
            seen_inf = True
        plan.append((y, x, 0, val, exp))
    for i, (y, x) in enumerate(pos):
        plan.append((y, x, 1) + ALBEDO_VALUES[i % len(ALBEDO_VALUES)])
        plan.append((y, x, 2) + NORMAL_VALUES[(i + 3) % len(NORMAL_VALUES)])     # another phase than the albedo's
    return plan


def hostile_images(H, W, seed=0, scale=1.0, inf=True):
    """benign_images(H, W, seed) with hostile_plan's values planted and constant_bins' bins filled (colour only).
    `scale`: the input scale the images are meant for (70000 / scale is planted).  inf=False plants no +Inf in the
    colour: on a small image it alone takes the auto-exposure below SCALE_RANGE."""
    color, albedo, normal = benign_images(H, W, seed)
    imgs = (color, albedo, normal)
    B = bins(H, W)
    for b, v in constant_bins(H, W).items():
        y0, y1, x0, x1 = B[b]
        color[y0:y1, x0:x1] = np.float32(v)
    for y, x, im, val, _ in hostile_plan(H, W, scale, inf):
        for k in range(3):
            if val[k] is not None:
                imgs[im][y, x, k] = np.float32(val[k])
    return color, albedo, normal


def sanitised(color, albedo, normal):
    """The images the denoiser is defined to read: colour NaN -> 0, negative -> 0, +Inf -> FLT_MAX, -Inf -> 0; albedo
    NaN -> 0, [0, 1]; normal NaN -> 0, [-1, 1]."""
    def s(a, lo, hi):
        a = np.asarray(a, np.float32)
        a = np.where(np.isnan(a), np.float32(0.0), a)
        return np.clip(a, np.float32(lo), np.float32(hi)).astype(np.float32)
    return s(color, 0.0, FLT_MAX), s(albedo, 0.0, 1.0), s(normal, -1.0, 1.0)


def autoexposure64(color) -> float:
    """The auto-exposure by its definition, in float64: the colour sanitised per channel (NaN -> 0, then clamped to
    [0, FLT_MAX]); ceil(H/16) x ceil(W/16) bins, bin b spanning [b*H/n, (b+1)*H/n) in integer arithmetic; each bin's
    mean luminance; bins with a mean <= 1e-8 skipped; 0.18 / 2**(mean of the others' log2), or 1 with none left."""
    c = np.asarray(color).astype(np.float64)
    c = np.clip(np.where(np.isnan(c), 0.0, c), 0.0, FLT_MAX)
    lum = 0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2]
    logs = []
    for y0, y1, x0, x1 in bins(*c.shape[:2]):
        m = float(lum[y0:y1, x0:x1].sum()) / ((y1 - y0) * (x1 - x0))
        if m > 1e-8:
            logs.append(math.log2(m))
    return 0.18 / 2.0 ** (sum(logs) / len(logs)) if logs else 1.0


def assert_scale_in_range(color) -> float:
    """A condition on the INPUT of an end-to-end case, not a tolerance on a result: its auto-exposure lies in
    SCALE_RANGE.  Below FLT_MAX's reciprocal times 65504 (1.9e-34) the scaled FLT_MAX no longer reaches the half-float
    clamp, so +Inf and its sanitised copy would part ways, and the output transform's 1 / scale leaves float32."""
    s = autoexposure64(color)
    assert SCALE_RANGE[0] <= s <= SCALE_RANGE[1], s
    return s


# ---------------------------------------------------------------- the GPU tests' shared steps (these do read denoise_ref)
def pu_err(got, want, scale=1.0):
    """(mean, max) |error| in the network-output (PU) domain of two denoised images."""
    import denoise_ref as ref
    to_x = lambda y: ref.pu_forward(np.float32(scale) * y) * ref.NORM_SCALE   # noqa: E731
    e = np.abs(to_x(got) - to_x(want))
    return float(e.mean()), float(e.max())


def run(d, color, albedo, normal, scale=None):
    """one Denoiser.execute on device copies of the images; the output as a numpy array"""
    import torch
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    out = d.execute(dev(color), dev(albedo), dev(normal), input_scale=scale)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_every_layer(r, d, w, monkeypatch, images, fill):
    """The per-convolution comparison of tests/test_gpu_denoise.py's docstring on `images` at the input scale 0.9 (benign
    images there, hostile ones in tests/test_gpu_denoise_inputs.py).  Returns the output and the dumped tensors."""
    import denoise_ref as ref
    from restir_amd.denoise import Denoiser
    color, albedo, normal = images
    H, W = color.shape[:2]
    if fill is not None:
        monkeypatch.setenv("RESTIR_DN_FILL", fill)
        d = Denoiser(r, w)
    try:
        got = run(d, color, albedo, normal, scale=0.9)
        dumps = [d.dump(i) for i in range(16)]
    finally:
        if fill is not None:
            d.close()
    t = {}
    for i, (a, real) in enumerate(dumps):
        assert not a[0].any() and not a[-1].any() and not a[:, 0].any() and not a[:, -1].any(), f"tensor {i}: border"
        assert not a[..., real:].any(), f"tensor {i}: channel padding"
        t[i] = a[1:-1, 1:-1, :real].astype(np.float64).transpose(2, 0, 1)
    # the network input tensor: the reference's preprocessing rounded to float16
    want_in = ref.preprocess(color, albedo, normal, np.float32(0.9), 9).astype(np.float16).astype(np.float64)
    assert np.abs(t[0] - want_in).max() <= np.abs(np.spacing(want_in.astype(np.float16))).max()
    for name, srcs, post, dst in ref.NET:
        y = ref.layer64(w, name, [(t[s], up) for s, up in srcs], post)
        if dst is None:        # dec_conv0 + output transform, float32 on the GPU
            want = ref.postprocess(y.astype(np.float32), np.float32(0.9), H, W)
            np.testing.assert_allclose(got, want, rtol=2e-4, atol=1e-6, err_msg=name)
            continue
        y16 = y.astype(np.float16)
        g16 = t[dst].astype(np.float16)
        assert g16.shape == y16.shape, name
        ulp = np.spacing(np.abs(y16)).astype(np.float64)
        mag = ref.layer64(w, name, [(t[s], up) for s, up in srcs], post, magnitude=True)
        bound = ulp * 1.0001 + 3e-5 * mag
        diff = np.abs(g16.astype(np.float64) - y16.astype(np.float64))
        off = diff > 0
        print(f"{name}: {off.mean() * 100:.3f} % of {diff.size} elements differ, max {float((diff / bound).max()):.3f} of the bound")
        assert (diff <= bound).all(), (name, float((diff / bound).max()))
        assert off.mean() <= 0.02, (name, float(off.mean()))
    return got, dumps
