"""The load rule of DESIGN.md 5.21 in numpy, written from the rule alone: the reference jh_load_surface and jh_load_yuv are compared
with byte for byte.  int64 for the codes, fractions.Fraction for the coefficient tables, numpy's float16 (round to nearest even) for
the texels; nothing of include/jello_load.h, the generated headers or the generators is used.  The store rule is morph_ref.store's.

  texel   U(c) = the binary32 nearest to c / 255; L(c) = the sRGB decode of c / 255 in binary64, rounded once to binary32 (the table of
          the fine kernel, by its definition).  Colour = L under an sRGB format or transfer, else U; alpha = U(a).
          STRAIGHT f16(colour), f16(U(a));  PREMULTIPLIED the store rule on (colour, U(a));  OPAQUE alpha 1.0;  BGRA swaps bytes 0, 2.
  chroma  cx0 = x >> 1, cx1 = clamp(cx0 + (x odd ? 1 : -1), 0, ceil(w / 2) - 1), the same in y;
          REPLICATE S = 16 C[cy0][cx0];  BILINEAR S = 9 C[cy0][cx0] + 3 C[cy0][cx1] + 3 C[cy1][cx0] + C[cy1][cx1]
  codes   Y' = Y - o, u = S_cb - 2048, v = S_cr - 2048:  R = clamp8((16 Ky Y' + Krv v + 2^19) >> 20), G with Kgu u + Kgv v, B with Kbu u
  tables  rne(exact * 2^16) of 255/219 or 1, 2 (1 - Kr) s, -2 Kb (1 - Kb) / Kg s, -2 Kr (1 - Kr) / Kg s, 2 (1 - Kb) s, s = 255/224 or 1

The keyword arguments named `variant` build the WRONG variants the battery has to tell from the rule (tests/test_load_spec.py):
bias (the rounding constant), truncate (the tables), clamp_first, swap_weights, cosited, mirror_edge, reciprocal (U as c * (1 / 255)),
decode_after (premultiplied sRGB decoded after the division)."""
from fractions import Fraction

import numpy as np

import morph_ref

RGBA8_UNORM, BGRA8_UNORM, RGBA8_SRGB, BGRA8_SRGB = range(4)
FORMATS = (RGBA8_UNORM, BGRA8_UNORM, RGBA8_SRGB, BGRA8_SRGB)
STRAIGHT, PREMULTIPLIED, OPAQUE = 0, 1, 2
ALPHAS = (STRAIGHT, PREMULTIPLIED, OPAQUE)
NV12, I420 = 0, 1
BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
NONE, SRGB = 0, 1
REPLICATE, BILINEAR = 0, 1
LAYOUTS, MATRICES, RANGES, TRANSFERS, CHROMAS = (NV12, I420), (BT601, BT709), (LIMITED, FULL), (NONE, SRGB), (REPLICATE, BILINEAR)
F = np.float32

_K = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000))}


def _rne(q):
    """round-half-even of a Fraction, spelled out."""
    n, d = q.numerator, q.denominator
    fl = n // d
    rem2 = 2 * (n - fl * d)
    if rem2 > d or (rem2 == d and fl % 2):
        fl += 1
    return fl


def exact_coefficients(matrix, rng):
    """([Ky, Krv, Kgu, Kgv, Kbu] as Fractions, offset): the real-valued inverse matrix on (Y - o, Cb - 128, Cr - 128)."""
    kr, kb = _K[matrix]
    kg = 1 - kr - kb
    sy, s, off = (Fraction(255, 219), Fraction(255, 224), 16) if rng == LIMITED else (Fraction(1), Fraction(1), 0)
    return [sy, 2 * (1 - kr) * s, -2 * kb * (1 - kb) / kg * s, -2 * kr * (1 - kr) / kg * s, 2 * (1 - kb) * s], off


def table(matrix, rng, truncate=False):
    """([Ky, Krv, Kgu, Kgv, Kbu] in 16.16, offset)."""
    k, off = exact_coefficients(matrix, rng)
    if truncate:  # (a wrong variant: towards zero)
        return [int(c * 65536) for c in k], off
    return [_rne(c * 65536) for c in k], off


def unorm_table(reciprocal=False):
    """U: float32 [256]."""
    c = np.arange(256, dtype=F)
    if reciprocal:  # (a wrong variant)
        return (c * (F(1.0) / F(255.0))).astype(F)
    return (c / F(255.0)).astype(F)  # (the IEEE quotient is the binary32 nearest to c / 255: test_load_spec checks it with Fractions)


def srgb_decode(x):
    """The sRGB decode of binary64 values, in binary64."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.where(x <= 0.04045, x / 12.92, np.power((x + 0.055) / 1.055, 2.4))


def linear_table():
    """L: float32 [256]."""
    return srgb_decode(np.arange(256, dtype=np.float64) / 255.0).astype(F)


def texels(pixels, fmt=None, alpha=STRAIGHT, transfer=None, reciprocal=False, decode_after=False):
    """(..., 4) uint8 pixels -- in the byte order of the surface format `fmt`, or RGBA codes under `transfer` -> (..., 4) uint16 f16
    bit patterns."""
    if (fmt is None) == (transfer is None):
        raise ValueError("one of fmt and transfer")
    if alpha not in ALPHAS or (fmt is not None and fmt not in FORMATS) or (transfer is not None and transfer not in TRANSFERS):
        raise ValueError("unknown format, transfer or alpha")
    px = np.asarray(pixels, np.uint8)
    srgb = transfer == SRGB if fmt is None else fmt in (RGBA8_SRGB, BGRA8_SRGB)
    if fmt in (BGRA8_UNORM, BGRA8_SRGB):
        px = px[..., [2, 1, 0, 3]]
    U = unorm_table(reciprocal)
    colour = (linear_table() if srgb else U)[px[..., :3]]
    a = U[px[..., 3]]
    if alpha == PREMULTIPLIED:
        if decode_after and srgb:  # (a wrong variant: the code un-premultiplied first, then decoded)
            with np.errstate(all="ignore"):
                a_inv = F(1.0) / np.maximum(a, F(1e-6))
                colour = srgb_decode((U[px[..., :3]] * a_inv[..., None]).astype(np.float64)).astype(F)
                return np.concatenate([colour, a[..., None]], axis=-1).astype(np.float16).view(np.uint16)
        return morph_ref.store(np.concatenate([colour, a[..., None]], axis=-1).astype(F), False)
    if alpha == OPAQUE:
        a = np.ones_like(a)
    return np.concatenate([colour, a[..., None]], axis=-1).astype(F).astype(np.float16).view(np.uint16)


def _other(n_luma, n_chroma, mirror_edge=False):
    """(c0, c1) per luma position of an axis: the sample that covers it and the one it blends with."""
    x = np.arange(n_luma, dtype=np.int64)
    c0 = x >> 1
    c1 = c0 + np.where(x & 1, 1, -1)
    if mirror_edge:  # (a wrong variant: the sample beyond the edge mirrored instead of repeated)
        c1 = np.where(c1 < 0, np.minimum(1, n_chroma - 1), np.where(c1 >= n_chroma, np.maximum(n_chroma - 2, 0), c1))
    return c0, np.clip(c1, 0, n_chroma - 1)


def chroma_sums(plane, w, h, chroma, swap_weights=False, cosited=False, mirror_edge=False):
    """(ceil(h/2), ceil(w/2)) codes -> (h, w) int64 sums S."""
    c = np.asarray(plane).astype(np.int64)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    assert c.shape == (ch, cw)
    if chroma not in CHROMAS:
        raise ValueError("unknown chroma filter")
    cx0, cx1 = _other(w, cw, mirror_edge=mirror_edge)
    cy0, cy1 = _other(h, ch, mirror_edge=mirror_edge)
    if chroma == REPLICATE:
        return 16 * c[cy0][:, cx0]
    if cosited:  # (a wrong variant: MPEG-2 siting in x -- an even texel sits on its sample, an odd one halfway to the next)
        x = np.arange(w)
        nx = np.minimum(cx0 + 1, cw - 1)
        wy0, wy1 = (1, 3) if swap_weights else (3, 1)
        top = np.where(x & 1, 2 * c[cy0][:, cx0] + 2 * c[cy0][:, nx], 4 * c[cy0][:, cx0])
        bot = np.where(x & 1, 2 * c[cy1][:, cx0] + 2 * c[cy1][:, nx], 4 * c[cy1][:, cx0])
        return wy0 * top + wy1 * bot
    w0, w1 = (1, 3) if swap_weights else (3, 1)  # (swapped: a wrong variant)
    return w0 * w0 * c[cy0][:, cx0] + w0 * w1 * c[cy0][:, cx1] + w1 * w0 * c[cy1][:, cx0] + w1 * w1 * c[cy1][:, cx1]


def codes(y, s_cb, s_cr, matrix, rng, bias=1 << 19, truncate=False, clamp_first=False, clamp8=True):
    """Luma codes and chroma sums of one shape -> (..., 3) int64 R'G'B' codes; clamp8=False: the rule's shifted sums before clamp8 acts."""
    if matrix not in MATRICES or rng not in RANGES:
        raise ValueError("unknown matrix or range")
    k, off = table(matrix, rng, truncate)
    yy = np.asarray(y).astype(np.int64) - off
    if clamp_first:  # (a wrong variant: Y' clamped at 0 before the products and the shift, not the shifted sum to [0, 255] after them.
        yy = np.maximum(yy, 0)  # Clamping the SUM to [0, 255 << 20] before the shift is no variant: it gives the rule's codes.)
    u, v = np.asarray(s_cb).astype(np.int64) - 2048, np.asarray(s_cr).astype(np.int64) - 2048
    luma = 16 * k[0] * yy
    sums = (luma + k[1] * v, luma + k[2] * u + k[3] * v, luma + k[4] * u)
    shifted = np.stack([(s + bias) >> 20 for s in sums], axis=-1)
    return np.clip(shifted, 0, 255) if clamp8 else shifted


def exact_codes(y, cb, cr, matrix, rng):
    """The real-valued inverse matrix on codes (not sums), clamped to [0, 255]: (..., 3) float64."""
    k, off = exact_coefficients(matrix, rng)
    k = [float(c) for c in k]
    yy = np.asarray(y, np.float64) - off
    u, v = np.asarray(cb, np.float64) - 128.0, np.asarray(cr, np.float64) - 128.0
    return np.clip(np.stack([k[0] * yy + k[1] * v, k[0] * yy + k[2] * u + k[3] * v, k[0] * yy + k[4] * u], axis=-1), 0.0, 255.0)


def split_planes(planes, layout):
    """(Y, Cb, Cr) from the planes as jh_blit_yuv lays them out: NV12 (Y, CbCr (ch, cw, 2)); I420 (Y, Cb, Cr)."""
    if layout == NV12:
        y, c = planes
        c = np.asarray(c)
        c = c.reshape(c.shape[0], -1, 2)
        return np.asarray(y), c[..., 0], c[..., 1]
    return tuple(np.asarray(p) for p in planes)


def yuv_codes(planes, layout, matrix, rng, chroma, **variant):
    """The (h, w, 3) int64 R'G'B' codes of a frame."""
    y, cb, cr = split_planes(planes, layout)
    h, w = y.shape
    cv = {k: v for k, v in variant.items() if k in ("swap_weights", "cosited", "mirror_edge")}
    kv = {k: v for k, v in variant.items() if k in ("bias", "truncate", "clamp_first", "clamp8")}
    return codes(y, chroma_sums(cb, w, h, chroma, **cv), chroma_sums(cr, w, h, chroma, **cv), matrix, rng, **kv)


def _into(dst, frame_bits, rect):
    """dst -- (H, W, 4) uint16 bits, or (H, W): a never-written image -- with frame_bits in the rectangle rect (None: the whole image)."""
    out = np.zeros(tuple(dst) + (4,), np.uint16) if isinstance(dst, tuple) else np.array(dst, np.uint16)
    H, W = out.shape[:2]
    x, y, w, h = (0, 0, W, H) if rect is None or (rect[2] == 0 and rect[3] == 0) else rect
    if (w == 0) != (h == 0) or x + w > W or y + h > H:
        raise ValueError("the rectangle is outside the image or empty in one dimension")
    if frame_bits.shape[:2] != (h, w):
        raise ValueError("the frame has the rectangle's size")
    out[y:y + h, x:x + w] = frame_bits
    return out


def load_surface(dst, pixels, fmt, alpha=STRAIGHT, rect=None, **variant):
    """What dst holds after jh_load_surface of the (h, w, 4) uint8 frame `pixels`."""
    return _into(dst, texels(pixels, fmt=fmt, alpha=alpha, **variant), rect)


def load_yuv(dst, planes, layout=NV12, matrix=BT709, rng=LIMITED, transfer=NONE, chroma=BILINEAR, rect=None, **variant):
    """What dst holds after jh_load_yuv of the frame in `planes`."""
    if layout not in LAYOUTS:
        raise ValueError("unknown layout")
    rgb = yuv_codes(planes, layout, matrix, rng, chroma, **variant).astype(np.uint8)
    px = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    return _into(dst, texels(px, transfer=transfer, alpha=STRAIGHT), rect)
