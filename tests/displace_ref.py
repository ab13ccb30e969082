"""The displacement rule (include/jello_hip.h "Displace") in numpy, written from the rule alone: what jh_displace has to
produce, bit for bit.  Positions are int64 (exact), sums binary32 with the rule's fmaf; the plan, the taps, the index rules and the
cubic weights are tests/warp_ref.py's helpers, the offset is written out here, independently of include/jello_displace.h.

  offset(scale, bits)   D, int64: the displacement in 2^-32 texel that f16 map values give under a binary32 scale
  positions(...)        (U, V), the displaced source positions of the destination rectangle's texels
  displace(...)         the image jh_displace leaves in dst
  direct(...)           the definition the rule rounds: bilinear / Catmull-Rom sampling in binary64 at the SAME integer positions

offset() and displace() take keyword switches that build near misses of the rule (tests/test_displace_spec.py asserts that the battery
of tests/displace_cases.py tells each of them from the rule): t_after=True (scale m - scale 0.5: the half subtracted after the product),
trunc=True (truncation instead of rint), ties_away=True (a half rounded away from zero), clamp=False (no clamp at 2^22 -- held at 2^29
only to stay inside int64), nan_zero=False (a NaN product goes through a max/min clamp and comes out as -2^22), map_premultiplied=True
(the map's colour channels times its alpha), swap_channels=True, frac_unshifted=True (the fraction taken from the displaced position
before the half-texel shift), map_at_source=True (the map read at the texel the plan's position falls into, not at the destination
texel)."""
import numpy as np

import warp_ref
from image_ref import fmaf32, fmax, operands, same_bits  # noqa: F401 (same_bits is part of this module's interface)
from warp_ref import BICUBIC, BILINEAR, CLAMP, EDGES, FILTERS, MIRROR, NEAREST, REPEAT, STRAIGHT, ZERO  # noqa: F401

R, G, B, A = 0, 1, 2, 3
CHANNELS = (R, G, B, A)
CHANNEL_NAMES = "rgba"
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
MAX_OFFSET = float(1 << 22)
F = np.float32


def offset(scale, bits, t_after=False, trunc=False, ties_away=False, clamp=True, nan_zero=True):
    """D = rint(clamp(scale (m - 0.5)) 2^32), int64, for the f16 bit patterns `bits` (any shape) under the binary32 `scale`."""
    with np.errstate(all="ignore"):
        m = np.asarray(bits, np.uint16).view(np.float16).astype(F)
        s = F(scale)
        if t_after:
            d = ((s * m).astype(F) - F(s * F(0.5))).astype(F)
        else:
            t = (m - F(0.5)).astype(F)  # exact: at most 24 significant bits
            d = (s * t).astype(F)       # one binary32 product
        nan = np.isnan(d)
        lim = MAX_OFFSET if clamp else float(1 << 29)
        d = np.where(nan, F(0.0) if nan_zero else F(-MAX_OFFSET), np.clip(d, F(-lim), F(lim)))
        scaled = d.astype(np.float64) * 4294967296.0  # exact
        if ties_away:
            return np.where(np.abs(scaled - np.trunc(scaled)) == 0.5, np.trunc(scaled) + np.sign(scaled), np.rint(scaled)).astype(np.int64)
        return (np.trunc(scaled) if trunc else np.rint(scaled)).astype(np.int64)  # (np.rint: ties to even)


def _map_values(map_bits, channel, premultiplied):
    if not premultiplied or channel == A:
        return map_bits[..., channel]
    with np.errstate(all="ignore"):
        v = map_bits.view(np.float16).astype(F)
        return (v[..., channel] * v[..., A]).astype(np.float16).view(np.uint16)


def positions(map_bits, pl, dst_rect, scale, x_channel, y_channel, swap_channels=False, map_premultiplied=False, map_at_source=False, **offset_variant):
    """(U, V) int64 arrays (dh, dw): the plan's positions of the destination rectangle's texels plus the map's offsets."""
    U0, V0 = warp_ref.positions(pl, dst_rect)
    dx, dy, dw, dh = dst_rect
    if map_at_source:
        H, W = map_bits.shape[:2]
        at = map_bits[np.clip(V0 >> 32, 0, H - 1), np.clip(U0 >> 32, 0, W - 1)]
    else:
        at = map_bits[dy:dy + dh, dx:dx + dw]
    if swap_channels:
        x_channel, y_channel = y_channel, x_channel
    sx, sy = scale if isinstance(scale, (tuple, list)) else (scale, scale)
    return (U0 + offset(sx, _map_values(at, x_channel, map_premultiplied), **offset_variant),
            V0 + offset(sy, _map_values(at, y_channel, map_premultiplied), **offset_variant))


def _taps(filt, U, frac_unshifted):
    taps = warp_ref.axis_taps(filt, U)
    if not frac_unshifted or filt == NEAREST:
        return taps
    return [(i, w) for (i, _), (_, w) in zip(taps, warp_ref.axis_taps(filt, U + (1 << 31)))]  # (the wrong variant: the weights of the unshifted position)


def _arguments(src_bits, map_bits, dst_shape, scale, x_channel, y_channel, matrix, filt, edge, flags, src_rect, dst_rect):
    if filt not in FILTERS or edge not in EDGES or flags & ~STRAIGHT:
        raise ValueError("unknown filter, edge or flag bits")
    if x_channel not in CHANNELS or y_channel not in CHANNELS:
        raise ValueError("a channel outside 0..3")
    if not all(np.isfinite(F(s)) for s in (scale if isinstance(scale, (tuple, list)) else (scale,))):
        raise ValueError("a scale is not finite")
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    shape = tuple(dst_shape[:2])
    map_bits = np.zeros(shape + (4,), np.uint16) if map_bits is None else np.ascontiguousarray(map_bits, np.uint16)  # (never written: 0)
    if map_bits.shape[:2] != shape:
        raise ValueError("the map's size is not the destination's")
    srect, drect = warp_ref.rects(src_bits.shape, shape, src_rect, dst_rect)
    return src_bits, map_bits, srect, drect, warp_ref.plan(matrix)


def displace(src_bits, map_bits, dst_shape, scale, x_channel=R, y_channel=G, matrix=IDENTITY, filt=BILINEAR, edge=ZERO, flags=0, src_rect=None,
             dst_rect=None, dst_bits=None, frac_unshifted=False, **variant):
    """The image jh_displace leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero); map_bits:
    the map, of dst's size (None: never written); dst_shape = (height, width) of dst; dst_bits: what dst held (None: a never-written
    dst, transparent black; the map itself where the map is dst).  Rectangles are (x, y, width, height), None: the whole image.  scale:
    one number or (x, y).  Returns (height, width, 4) uint16."""
    src_bits, map_bits, (sx, sy, sw, sh), drect, pl = _arguments(src_bits, map_bits, dst_shape, scale, x_channel, y_channel, matrix, filt, edge, flags,
                                                                 src_rect, dst_rect)
    out = np.zeros(map_bits.shape, np.uint16) if dst_bits is None else np.array(dst_bits, np.uint16)
    dx, dy, dw, dh = drect
    if dw == 0 or dh == 0:
        return out
    U, V = positions(map_bits, pl, drect, scale, x_channel, y_channel, **variant)
    straight = bool(flags & STRAIGHT)
    p = operands(src_bits[sy:sy + sh, sx:sx + sw], not straight, F)
    with np.errstate(all="ignore"):
        ix = [(warp_ref.index(edge, i, sw), w[..., None]) for i, w in _taps(filt, U, frac_unshifted)]
        iy = [(warp_ref.index(edge, j, sh), w[..., None]) for j, w in _taps(filt, V, frac_unshifted)]

        def operand(i, j):
            if sw == 0 or sh == 0:
                return np.zeros((dh, dw, 4), F)
            live = (i >= 0) & (j >= 0)
            return np.where(live[..., None], p[np.maximum(j, 0), np.maximum(i, 0)], F(0.0)).astype(F)

        zero4 = np.zeros((dh, dw, 4), F)
        acc = zero4
        for j, wy in iy:  # rows, then columns
            h = zero4
            for i, wx in ix:
                h = fmaf32(wx, operand(i, j), h)
            acc = fmaf32(wy, h, acc)
        if straight:
            texels = acc
        else:
            zero = F(0.0)
            a_inv = F(1.0) / fmax(acc[..., 3], F(1e-6))
            texels = np.concatenate([acc[..., :3] * a_inv[..., None] + zero, acc[..., 3:] + zero], axis=-1)
        out[dy:dy + dh, dx:dx + dw] = texels.astype(F).astype(np.float16).view(np.uint16)
    return out


def _weights64(filt, U):
    """The taps of one axis in binary64 at the int64 positions U, with the whole 32-bit fraction: [(index int64, weight float64)]."""
    if filt == NEAREST:
        return [(U >> 32, np.ones(U.shape))]
    u = U - (1 << 31)
    i0, f = u >> 32, (u & 0xFFFFFFFF).astype(np.float64) / 4294967296.0  # exact: 32 bits
    if filt == BILINEAR:
        return [(i0, 1.0 - f), (i0 + 1, f)]
    return [(i0 - 1 + k, w) for k, w in enumerate(warp_ref._cubic64(f))]


def direct(src_bits, map_bits, dst_shape, scale, x_channel=R, y_channel=G, matrix=IDENTITY, filt=BILINEAR, edge=ZERO, flags=0, src_rect=None,
           dst_rect=None):
    """The definition the rule rounds, at the rule's own integer positions: bilinear or Catmull-Rom sampling (NEAREST: the texel whose
    cell holds the position) in binary64 with the un-truncated fraction, before the store -- ((dh, dw, 4) float64 of the destination
    rectangle, premultiplied unless STRAIGHT; (U, V) int64).  Taking the positions from the rule leaves no texel out near a boundary."""
    src_bits, map_bits, (sx, sy, sw, sh), drect, pl = _arguments(src_bits, map_bits, dst_shape, scale, x_channel, y_channel, matrix, filt, edge, flags,
                                                                 src_rect, dst_rect)
    U, V = positions(map_bits, pl, drect, scale, x_channel, y_channel)
    p = operands(src_bits[sy:sy + sh, sx:sx + sw], not flags & STRAIGHT, np.float64)
    acc = np.zeros(U.shape + (4,))
    for j, wy in _weights64(filt, V):
        jj = warp_ref.index(edge, j, sh)
        for i, wx in _weights64(filt, U):
            ii = warp_ref.index(edge, i, sw)
            live = (ii >= 0) & (jj >= 0)
            acc += (wx * wy)[..., None] * np.where(live[..., None], p[np.maximum(jj, 0), np.maximum(ii, 0)], 0.0)
    return acc, (U, V)
