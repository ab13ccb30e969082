"""Reference of jh_blit's conversion (include/jello_hip.h, DESIGN.md "Surface blit"), written from the rule alone: numpy and
binary64 pow, nothing shared with the threshold table or the kernel.

    p = c * a in f32; v = clamp(p, 0, 1) with NaN -> 0; unorm u8 = rint_f32(v * 255); sRGB colour u8 = rint_f64(255 enc(v));
    alpha = rint_f32(clamp(a) * 255) in every format; BGRA swaps bytes 0 and 2.
"""
import numpy as np

RGBA8_UNORM, BGRA8_UNORM, RGBA8_SRGB, BGRA8_SRGB = range(4)
FORMATS = (RGBA8_UNORM, BGRA8_UNORM, RGBA8_SRGB, BGRA8_SRGB)


def clamp01(p):
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(p > 0, p, np.float32(0))
        return np.where(v < 1, v, np.float32(1)).astype(np.float32)


def unorm8(v):
    return np.rint(np.asarray(v, np.float32) * np.float32(255.0)).astype(np.uint8)


def srgb8(v):
    d = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d <= 0.0031308, 12.92 * d, 1.055 * np.power(d, 1.0 / 2.4) - 0.055)
    return np.rint(255.0 * e).astype(np.uint8)


def convert_f32(c, a, fmt):
    """Colour channels c (..., 3) and alpha a (...) as f32 (widened f16) -> (..., 4) uint8 in the surface's byte order."""
    c = np.asarray(c, np.float32)
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = clamp01(c * a[..., None])
    col = srgb8(p) if fmt in (RGBA8_SRGB, BGRA8_SRGB) else unorm8(p)
    out = np.empty(p.shape[:-1] + (4,), np.uint8)
    out[..., :3] = col
    out[..., 3] = unorm8(clamp01(a))
    if fmt in (BGRA8_UNORM, BGRA8_SRGB):
        out[..., [0, 2]] = out[..., [2, 0]]
    return out


def convert(image_f16_bits, fmt):
    """An RGBA16F image as f16 bit patterns (H, W, 4) uint16 -> the (H, W, 4) uint8 surface."""
    f = np.asarray(image_f16_bits, np.uint16).view(np.float16).astype(np.float32)
    return convert_f32(f[..., :3], f[..., 3], fmt)
