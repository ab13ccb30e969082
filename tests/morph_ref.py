"""The morphology rule of DESIGN.md 5.11 in numpy, written from the rule alone: the reference jh_morphology is compared with byte for
byte.  The 2-D window is taken directly, by shifted views of the padded image -- no separable shortcut, no prefix or suffix trick.

  operand   the f16 texel widened to binary32 (c, a); p = (c a, a), each product exact -- or with STRAIGHT p = (c, a) as stored.
            A source that was never written: all zero, transparent black.
  window    output (X, Y) of the rectangle takes the image positions [X - rx, X + rx] x [Y - ry, Y + ry].  The IMAGE is the edge,
            not the rectangle.  Outside the image: ZERO: +0.0f in all four channels takes part; CLAMP: the position does not.
  order     per channel: any NaN in the window gives a NaN; otherwise DILATE is the greatest, ERODE the least operand in IEEE
            totalOrder (-0 below +0).  As integer keys k = bits ^ ((int32)bits >> 31 & 0x7fffffff), compared as signed.
  store     STRAIGHT: f16(V), exact.  Default: a_inv = 1.0f / max(V.a, 1e-6f); f16(V.rgb a_inv + 0.0f), f16(V.a + 0.0f)  (maxNum)

(A radius larger than the image is walked as the image's extent: the positions beyond that are all outside the image, where every
position is the same operand, and one of them is already in the window.)

The keyword arguments of `morph` after `dst_bits` build the six near misses the battery has to tell from the rule
(tests/test_morph_spec.py): a NaN ignored instead of sticky, -0 and +0 taken for equal, the window clipped to the rectangle instead
of the image, ZERO's padding left out, straight operands where premultiplied ones are asked for, a window of [-r, r)."""
import numpy as np

import image_ref
from image_ref import fmax, same_bits  # noqa: F401 (part of this module's interface: equal f16 bit patterns, a NaN equal to any NaN)

ERODE, DILATE = 0, 1
ZERO, CLAMP = 0, 1
STRAIGHT = 1
MAX_RADIUS = 255
INT_MIN, INT_MAX = -2**31, 2**31 - 1


def key(values, op, nan_sticky=True, signed_zero=True):
    """The int32 order keys of a float32 array under the operator."""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32).copy()
    if not signed_zero:  # (a near miss: -0 is read as +0)
        bits[bits == 0x80000000] = 0
    signed = bits.view(np.int32)
    k = signed ^ ((signed >> 31) & 0x7FFFFFFF)
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    winner, neutral = (INT_MAX, INT_MIN) if op == DILATE else (INT_MIN, INT_MAX)
    return np.where(nan, np.int32(winner if nan_sticky else neutral), k).astype(np.int32)  # (a near miss: a NaN never wins)


def unkey(k):
    """The float32 values of keys (of an extreme: a NaN)."""
    k = np.ascontiguousarray(k, np.int32)
    return (k ^ ((k >> 31) & 0x7FFFFFFF)).view(np.uint32).view(np.float32)


def _radii(radius):
    rx, ry = radius if isinstance(radius, (tuple, list)) else (radius, radius)
    return int(rx), int(ry)


def resolve(shape, rect):
    return image_ref.resolve(shape, rect, "the rectangle is not inside the image or is empty in one dimension", texels=True)


def legal(op, radius, edge, flags, shape, rect):
    rx, ry = _radii(radius)
    if op not in (ERODE, DILATE) or edge not in (ZERO, CLAMP) or flags & ~STRAIGHT:
        raise ValueError("unknown op, edge or flag bit")
    if not (0 <= rx <= MAX_RADIUS and 0 <= ry <= MAX_RADIUS):
        raise ValueError("a radius above 255")
    return (rx, ry) + resolve(shape, rect)


def window_extremum(p, op, rx, ry, edge, x, y, rw, rh, nan_sticky=True, signed_zero=True, zero_pad=True, closed_window=True):
    """(rh, rw, 4) float32: the rule's V for the rectangle, out of the operands p (H, W, 4) float32 of the whole image."""
    h, w = p.shape[:2]
    k = key(p, op, nan_sticky, signed_zero)
    neutral = INT_MIN if op == DILATE else INT_MAX
    pad = 0 if (edge == ZERO and zero_pad) else neutral  # key(+0.0f) = 0; CLAMP: the position does not take part
    ex, ey = min(rx, w), min(ry, h)
    padded = np.full((h + 2 * ey, w + 2 * ex, 4), pad, np.int32)
    padded[ey:ey + h, ex:ex + w] = k
    pick = np.maximum if op == DILATE else np.minimum
    acc = np.full((rh, rw, 4), neutral, np.int32)
    def span(e):  # (a near miss: the window [-r, r); radius 0 still reads the centre)
        return range(-e, e + 1) if closed_window or e == 0 else range(-e, e)

    for dy in span(ey):
        for dx in span(ex):
            pick(acc, padded[ey + y + dy:ey + y + dy + rh, ex + x + dx:ex + x + dx + rw], out=acc)
    return unkey(acc)  # (with nan_sticky=False a window of NaNs alone leaves the neutral key, a NaN)


def store(v, straight):
    """(…, 4) float32 -> uint16 f16 bit patterns, as the rule stores."""
    with np.errstate(all="ignore"):
        if straight:
            texels = v
        else:
            zero = np.float32(0.0)
            a_inv = np.float32(1.0) / fmax(v[..., 3], np.float32(1e-6))
            texels = np.concatenate([v[..., :3] * a_inv[..., None] + zero, v[..., 3:] + zero], axis=-1)
        return texels.astype(np.float32).astype(np.float16).view(np.uint16)


def operands(src_bits, straight):
    return image_ref.operands(src_bits, not straight)


def morph(src_bits, op, radius, edge=ZERO, flags=0, rect=None, dst_bits=None, nan_sticky=True, signed_zero=True, window_image=True,
          zero_pad=True, premultiply=True, closed_window=True):
    """The image jh_morphology leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero);
    dst_bits: what dst held (None: a never-written dst, transparent black).  radius: a scalar or (rx, ry); rect: (x, y, width,
    height), None or 0 x 0: the whole image.  Returns (H, W, 4) uint16."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    rx, ry, x, y, rw, rh = legal(op, radius, edge, flags, src_bits.shape, rect)
    out = np.zeros_like(src_bits) if dst_bits is None else np.array(dst_bits, np.uint16)
    straight = bool(flags & STRAIGHT)
    p = operands(src_bits, straight or not premultiply)  # (a near miss: the premultiply skipped, the store kept)
    variant = dict(nan_sticky=nan_sticky, signed_zero=signed_zero, zero_pad=zero_pad, closed_window=closed_window)
    if window_image:
        v = window_extremum(p, op, rx, ry, edge, x, y, rw, rh, **variant)
    else:  # (a near miss: the rectangle is taken for the image)
        v = window_extremum(p[y:y + rh, x:x + rw], op, rx, ry, edge, 0, 0, rw, rh, **variant)
    out[y:y + rh, x:x + rw] = store(v, straight)
    return out
