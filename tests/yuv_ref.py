"""Reference of jh_blit_yuv's conversion (include/jello_hip.h "YUV blit"), written from the rule alone: numpy
for the pixels, fractions.Fraction for the coefficient tables.  Nothing is shared with tools/gen_yuv_table.py, the committed
header or the kernel; the R'G'B' codes come from surface_ref.convert.

    codes   (R, G, B) = bytes 0..2 of the blit's RGBA8_UNORM (transfer NONE) or RGBA8_SRGB (transfer SRGB) pixel
    Y       = clamp8(o + floor((M[0] . (R, G, B) + 2^15) / 2^16))
    Cb, Cr  = clamp8(128 + floor((M[1 or 2] . S + 2^17) / 2^18)), S = the code sums of x in {2cx, min(2cx+1, w-1)},
              y in {2cy, min(2cy+1, h-1)}
    tables  rne(exact * 2^16), green adjusted: Y row sums to rne(scale * 2^16), chroma rows to 0
"""
from fractions import Fraction

import numpy as np

import surface_ref

NV12, I420 = 0, 1
BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
NONE, SRGB = 0, 1
LAYOUTS, MATRICES, RANGES, TRANSFERS = (NV12, I420), (BT601, BT709), (LIMITED, FULL), (NONE, SRGB)

_K = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000))}


def _rne(q):
    """round-half-even of a Fraction, spelled out."""
    n, d = q.numerator, q.denominator
    fl = n // d
    rem2 = 2 * (n - fl * d)
    if rem2 > d or (rem2 == d and fl % 2):
        fl += 1
    return fl


def exact_matrix(matrix, rng):
    """(3 x 3 Fractions, offset): the real-valued formula Y = o + row0 . rgb, Cb = 128 + row1 . rgb, Cr = 128 + row2 . rgb."""
    kr, kb = _K[matrix]
    kg = 1 - kr - kb
    sy, sc, off = (Fraction(219, 255), Fraction(224, 255), 16) if rng == LIMITED else (Fraction(1), Fraction(1), 0)
    rows = [[sy * kr, sy * kg, sy * kb],
            [-sc * kr / (2 * (1 - kb)), -sc * kg / (2 * (1 - kb)), sc / 2],
            [sc / 2, -sc * kg / (2 * (1 - kr)), -sc * kb / (2 * (1 - kr))]]
    return rows, off


def table(matrix, rng):
    """(3 x 3 ints in 16.16, offset)."""
    rows, off = exact_matrix(matrix, rng)
    sy = Fraction(219, 255) if rng == LIMITED else Fraction(1)
    m = [[_rne(c * 65536) for c in row] for row in rows]
    for row, want in zip(m, (_rne(sy * 65536), 0, 0)):
        row[1] += want - sum(row)
    return m, off


def clamp8(v):
    return np.clip(v, 0, 255)


def luma(codes, matrix, rng, clamp=True):
    """(..., 3) codes -> Y (int64)."""
    m, off = table(matrix, rng)
    c = np.asarray(codes).astype(np.int64)
    y = off + ((m[0][0] * c[..., 0] + m[0][1] * c[..., 1] + m[0][2] * c[..., 2] + (1 << 15)) >> 16)
    return clamp8(y) if clamp else y


def chroma_of_sums(sums, matrix, rng, clamp=True):
    """(..., 3) sums of four codes -> (Cb, Cr) (int64)."""
    m, _ = table(matrix, rng)
    s = np.asarray(sums).astype(np.int64)
    out = []
    for row in (m[1], m[2]):
        v = 128 + ((row[0] * s[..., 0] + row[1] * s[..., 1] + row[2] * s[..., 2] + (1 << 17)) >> 18)
        out.append(clamp8(v) if clamp else v)
    return out[0], out[1]


def chroma_sums(codes):
    """(H, W, 3) codes -> (ceil(H/2), ceil(W/2), 3) sums over x in {2cx, min(2cx+1, W-1)}, y in {2cy, min(2cy+1, H-1)}."""
    c = np.asarray(codes).astype(np.int64)
    h, w = c.shape[:2]
    ys0 = np.arange(0, h, 2)
    ys1 = np.minimum(ys0 + 1, h - 1)
    xs0 = np.arange(0, w, 2)
    xs1 = np.minimum(xs0 + 1, w - 1)
    return c[ys0][:, xs0] + c[ys0][:, xs1] + c[ys1][:, xs0] + c[ys1][:, xs1]


def from_codes(codes, matrix, rng):
    """(H, W, 3) uint8 R'G'B' codes -> (Y (H, W), Cb, Cr (ceil(H/2), ceil(W/2))) uint8."""
    y = luma(codes, matrix, rng).astype(np.uint8)
    cb, cr = chroma_of_sums(chroma_sums(codes), matrix, rng)
    return y, cb.astype(np.uint8), cr.astype(np.uint8)


def codes_of(image_f16_bits, transfer):
    fmt = surface_ref.RGBA8_SRGB if transfer == SRGB else surface_ref.RGBA8_UNORM
    return surface_ref.convert(image_f16_bits, fmt)[..., :3]


def convert(image_f16_bits, layout, matrix, rng, transfer):
    """An RGBA16F image as f16 bit patterns (H, W, 4) uint16 -> the planes as uint8 arrays: NV12 (Y (H, W), CbCr (ceil(H/2),
    ceil(W/2), 2)); I420 (Y, Cb, Cr)."""
    y, cb, cr = from_codes(codes_of(image_f16_bits, transfer), matrix, rng)
    if layout == NV12:
        return y, np.stack([cb, cr], axis=-1)
    return y, cb, cr
