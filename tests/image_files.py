"""Radiance RGBE files written from numpy, for the decoder tests (tests/test_image_io.py) and the sky of
tests/test_gpu_textures.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def rgbe_encode(img):
    """float32 (H, W, 3) -> RGBE bytes (Ward's float2rgbe) and the floats a decoder must return."""
    v = img.max(-1).astype(np.float64)
    m, e = np.frexp(v)
    scale = np.where(v > 1e-32, m * 256.0 / np.where(v > 0, v, 1), 0.0)
    rgb = np.clip(np.floor(img * scale[..., None]), 0, 255).astype(np.uint8)
    ex = np.where(v > 1e-32, e + 128, 0).astype(np.uint8)
    rgbe = np.concatenate([rgb, ex[..., None]], -1)
    f = np.where(rgbe[..., 3:4] > 0, np.ldexp(1.0, rgbe[..., 3:4].astype(np.int32) - 136), 0.0)
    dec = (rgbe[..., :3].astype(np.float64) * f).astype(np.float32)
    return rgbe, dec


def _rle_channel(a):
    out, i, n = bytearray(), 0, len(a)
    while i < n:
        j = i
        while j < n and j - i < 127 and a[j] == a[i]:
            j += 1
        if j - i >= 3:
            out += bytes([128 + (j - i), a[i]])
            i = j
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and a[j] == a[j + 1] == a[j + 2]):
            j += 1
        out += bytes([j - i]) + bytes(a[i:j])
        i = j
    return out


def write_hdr(path, rgbe, rle):
    H, W, _ = rgbe.shape
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n")
        f.write(f"-Y {H} +X {W}\n".encode())
        for y in range(H):
            if rle:
                f.write(bytes([2, 2, W >> 8, W & 255]))
                for c in range(4):
                    f.write(_rle_channel(rgbe[y, :, c].tolist()))
            else:
                f.write(rgbe[y].tobytes())
