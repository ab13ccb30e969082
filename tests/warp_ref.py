"""The warp rule (include/jello_hip.h "Warp") in numpy, written from the rule alone: what jh_warp has to produce, bit
for bit.  Positions are int64 (exact), sums binary32 with the rule's fmaf (image_ref.fmaf32).

  plan(matrix)      the six integers P, Q, R, S, T, W (ValueError for an illegal matrix)
  bounds(...)       the rectangle of jh_warp_bounds
  warp(...)         the image jh_warp leaves in dst
  direct(...)       the definition the rule rounds: bilinear / Catmull-Rom sampling in binary64 at the binary64 inverse

warp() takes keyword switches that build near misses of the rule (tests/test_warp_spec.py asserts that the battery of
tests/warp_cases.py tells each of them from the rule): floor=False (the index by truncation toward zero), frac_round=True (the
fraction rounded to 16 bits instead of truncated), coef_bits=16 (the plan's coefficients at 2^-16), rows_first=False, fused=False
(multiply, round, add), mirror_2n=False (MIRROR with period 2 n - 2: the edge texel not repeated), edge_rect=False (the image is the
edge, not the rectangle), premultiply=False."""
import math

import numpy as np

import image_ref
from image_ref import fmaf32, fmax, mul_add32, same_bits  # noqa: F401 (same_bits is part of this module's interface)

NEAREST, BILINEAR, BICUBIC = 0, 1, 2
FILTERS = (NEAREST, BILINEAR, BICUBIC)
FILTER_NAMES = {NEAREST: "nearest", BILINEAR: "bilinear", BICUBIC: "bicubic"}
ZERO, CLAMP, REPEAT, MIRROR = 0, 1, 2, 3
EDGES = (ZERO, CLAMP, REPEAT, MIRROR)
EDGE_NAMES = {ZERO: "zero", CLAMP: "clamp", REPEAT: "repeat", MIRROR: "mirror"}
STRAIGHT = 1
MAX_SIDE = 32768
MAX_SCALE, MAX_OFFSET = 64.0, float(1 << 22)
GROW = {NEAREST: 0.5, BILINEAR: 1.0, BICUBIC: 2.0}


def inverse(matrix):
    """(p, q, r, s, t, w) in binary64, every product and quotient rounded once (Python floats: nothing is contracted).  ValueError
    naming the condition for an illegal matrix."""
    m = [float(v) for v in matrix]
    if len(m) != 6:
        raise ValueError("six entries")
    a, b, c, d, e, f = m
    if not all(math.isfinite(v) for v in m):
        raise ValueError("a matrix entry is not finite")
    det = a * d - b * c
    if not math.isfinite(det):
        raise ValueError("the determinant is not finite")
    if det == 0.0:
        raise ValueError("the determinant is 0")

    def div(x):  # (a quotient beyond binary64 is an Inf in C; Python raises instead)
        try:
            return x / det
        except OverflowError:
            return math.copysign(math.inf, x) * math.copysign(1.0, det)

    inv = (div(d), div(-c), div(c * f - d * e), div(-b), div(a), div(b * e - a * f))
    if not all(abs(inv[i]) <= MAX_SCALE for i in (0, 1, 3, 4)):
        raise ValueError("an inverse coefficient above 64")
    if not all(abs(inv[i]) <= MAX_OFFSET for i in (2, 5)):
        raise ValueError("an inverse offset above 2^22")
    return inv


def plan(matrix, coef_bits=32):
    """P, Q, R, S, T, W.  coef_bits=16: a wrong variant, the coefficients rounded at 2^-16 texel."""
    inv = inverse(matrix)
    drop = 32 - coef_bits
    out = []
    for i, v in enumerate(inv):
        bits = coef_bits if i % 3 == 2 else coef_bits - 1
        out.append(int(round(v * float(1 << bits))) << drop)  # (round: half to even, exact on a float; the scaling is exact)
    return tuple(out)


def bounds(matrix, src_size, filt, dst_size):
    """jh_warp_bounds: (x, y, width, height), (0, 0, 0, 0) when empty."""
    inverse(matrix)
    a, b, c, d, e, f = [float(v) for v in matrix]
    g = GROW[filt]
    lo, hi = [math.inf, math.inf], [-math.inf, -math.inf]
    for y in (-g, float(src_size[1]) + g):
        for x in (-g, float(src_size[0]) + g):
            for k, v in enumerate(((a * x + c * y) + e, (b * x + d * y) + f)):
                if v != v:
                    lo[k], hi[k] = -math.inf, math.inf
                lo[k], hi[k] = min(lo[k], v), max(hi[k], v)
    first, count = [], []
    for k in range(2):
        x0 = lo[k] if math.isinf(lo[k]) else math.floor(lo[k]) - 1
        x1 = hi[k] if math.isinf(hi[k]) else math.ceil(hi[k]) + 1
        x0, x1 = max(x0, 0), min(x1, dst_size[k])
        if not x1 > x0:
            return (0, 0, 0, 0)
        first.append(int(x0))
        count.append(int(x1 - x0))
    return (first[0], first[1], count[0], count[1])


def index(edge, i, n, mirror_2n=True):
    """The index in [0, n) a tap i reads, -1 where it reads +0 (ZERO outside); i an int64 array."""
    if mirror_2n or edge != MIRROR:
        return image_ref.index(edge, i, n)
    i = np.asarray(i, np.int64)
    if n == 1:  # (the wrong variant: period 2 n - 2)
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def cubic_weights(f):
    """w0 .. w3 of the rule at the float32 fraction(s) f."""
    f = np.asarray(f, np.float32)
    h = np.float32
    with np.errstate(all="ignore"):
        w0 = (fmaf32(fmaf32(h(-0.5), f, h(1.0)), f, h(-0.5)) * f).astype(np.float32)
        w1 = fmaf32((fmaf32(h(1.5), f, h(-2.5)) * f).astype(np.float32), f, h(1.0))
        w2 = (fmaf32(fmaf32(h(-1.5), f, h(2.0)), f, h(0.5)) * f).astype(np.float32)
        w3 = ((fmaf32(h(0.5), f, h(-0.5)) * f).astype(np.float32) * f).astype(np.float32)
    return [w0, w1, w2, w3]


def axis_taps(filt, U, floor=True, frac_round=False):
    """The taps of one axis at the int64 positions U: a list of (index array int64, weight array float32), ascending."""
    U = np.asarray(U, np.int64)

    def shift32(v):
        return v >> 32 if floor else np.where(v >= 0, v >> 32, -((-v) >> 32))  # (the wrong variant truncates toward zero)

    if filt == NEAREST:
        return [(shift32(U), np.ones(U.shape, np.float32))]
    u = U - (1 << 31)
    if frac_round:
        u = u + (1 << 15)
    i0 = shift32(u)
    f = (((u >> 16) & 0xFFFF).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)
    if filt == BILINEAR:
        return [(i0, (np.float32(1.0) - f).astype(np.float32)), (i0 + 1, f)]
    return [(i0 - 1 + k, w) for k, w in enumerate(cubic_weights(f))]


def rects(src_shape, dst_shape, src_rect, dst_rect):
    """((sx, sy, sw, sh), (dx, dy, dw, dh)) resolved; ValueError for what the rule refuses."""
    out = []
    for (h, w), r in ((src_shape[:2], src_rect), (dst_shape[:2], dst_rect)):
        if w > MAX_SIDE or h > MAX_SIDE:
            raise ValueError("an image side above 32768")
        out.append(image_ref.resolve((h, w), r, "a rectangle is outside its image or empty in one dimension"))
    return tuple(out)


def positions(pl, dst_rect):
    """(U, V) int64 arrays (dh, dw) of the destination rectangle's texels."""
    P, Q, R, S, T, W = pl
    dx, dy, dw, dh = dst_rect
    X2 = 2 * (dx + np.arange(dw, dtype=np.int64)) + 1
    Y2 = 2 * (dy + np.arange(dh, dtype=np.int64)) + 1
    return P * X2[None, :] + Q * Y2[:, None] + R, S * X2[None, :] + T * Y2[:, None] + W


def warp(src_bits, dst_shape, matrix, filt=BILINEAR, edge=ZERO, flags=0, src_rect=None, dst_rect=None, dst_bits=None, floor=True,
         frac_round=False, coef_bits=32, rows_first=True, fused=True, mirror_2n=True, edge_rect=True, premultiply=True):
    """The image jh_warp leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero).  dst_shape =
    (height, width) of dst; dst_bits: what dst held (None: a never-written dst, transparent black).  Rectangles are (x, y, width,
    height), None: the whole image.  Returns (height, width, 4) uint16."""
    if filt not in FILTERS or edge not in EDGES or flags & ~STRAIGHT:
        raise ValueError("unknown filter, edge or flag bits")
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    out = np.zeros(tuple(dst_shape[:2]) + (4,), np.uint16) if dst_bits is None else np.array(dst_bits, np.uint16)
    (sx, sy, sw, sh), drect = rects(src_bits.shape, out.shape, src_rect, dst_rect)
    pl = plan(matrix, coef_bits)
    dx, dy, dw, dh = drect
    if dw == 0 or dh == 0:
        return out
    U, V = positions(pl, drect)
    tx, ty = axis_taps(filt, U, floor, frac_round), axis_taps(filt, V, floor, frac_round)
    step = fmaf32 if fused else mul_add32
    straight = bool(flags & STRAIGHT)
    with np.errstate(all="ignore"):
        if edge_rect:
            p, ox, oy, nx, ny = src_bits[sy:sy + sh, sx:sx + sw], 0, 0, sw, sh
        else:  # (a wrong variant: tap indices resolved against the image)
            p, ox, oy, ny, nx = src_bits, sx, sy, src_bits.shape[0], src_bits.shape[1]
        p = p.view(np.float16).astype(np.float32)
        if not straight and premultiply:
            p = np.concatenate([p[..., :3] * p[..., 3:], p[..., 3:]], axis=-1).astype(np.float32)
        ix = [(index(edge, i + ox, nx, mirror_2n), w[..., None]) for i, w in tx]
        iy = [(index(edge, j + oy, ny, mirror_2n), w[..., None]) for j, w in ty]

        def operand(i, j):
            if nx == 0 or ny == 0:
                return np.zeros((dh, dw, 4), np.float32)
            live = (i >= 0) & (j >= 0)
            return np.where(live[..., None], p[np.maximum(j, 0), np.maximum(i, 0)], np.float32(0.0)).astype(np.float32)

        zero4 = np.zeros((dh, dw, 4), np.float32)
        acc = zero4
        if rows_first:
            for j, wy in iy:
                h = zero4
                for i, wx in ix:
                    h = step(wx, operand(i, j), h)
                acc = step(wy, h, acc)
        else:  # (a wrong variant)
            for i, wx in ix:
                g = zero4
                for j, wy in iy:
                    g = step(wy, operand(i, j), g)
                acc = step(wx, g, acc)
        if straight:
            texels = acc
        else:
            zero = np.float32(0.0)
            a_inv = np.float32(1.0) / fmax(acc[..., 3], np.float32(1e-6))
            texels = np.concatenate([acc[..., :3] * a_inv[..., None] + zero, acc[..., 3:] + zero], axis=-1)
        out[dy:dy + dh, dx:dx + dw] = texels.astype(np.float32).astype(np.float16).view(np.uint16)
    return out


def _cubic64(f):
    return [((-0.5 * f + 1.0) * f - 0.5) * f, (1.5 * f - 2.5) * f * f + 1.0, ((-1.5 * f + 2.0) * f + 0.5) * f, (0.5 * f - 0.5) * f * f]


def direct(src_bits, dst_shape, matrix, filt, edge=ZERO, flags=0, src_rect=None, dst_rect=None):
    """The definition the rule rounds: bilinear or Catmull-Rom sampling (NEAREST: the texel whose cell holds the position) in
    binary64 at the binary64 inverse position, before the store -- ((dh, dw, 4) float64 of the destination rectangle, premultiplied
    unless STRAIGHT; (u, v) float64 positions)."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    (sx, sy, sw, sh), (dx, dy, dw, dh) = rects(src_bits.shape, tuple(dst_shape[:2]), src_rect, dst_rect)
    ip, iq, ir, is_, it, iw = inverse(matrix)
    xs, ys = (dx + np.arange(dw) + 0.5)[None, :], (dy + np.arange(dh) + 0.5)[:, None]
    u, v = ip * xs + iq * ys + ir, is_ * xs + it * ys + iw
    p = src_bits[sy:sy + sh, sx:sx + sw].view(np.float16).astype(np.float64)
    if not flags & STRAIGHT:
        p = np.concatenate([p[..., :3] * p[..., 3:], p[..., 3:]], axis=-1)

    def taps(c):
        if filt == NEAREST:
            return [(np.floor(c).astype(np.int64), np.ones_like(c))]
        i0 = np.floor(c - 0.5)
        f = c - 0.5 - i0
        i0 = i0.astype(np.int64)
        if filt == BILINEAR:
            return [(i0, 1.0 - f), (i0 + 1, f)]
        return [(i0 - 1 + k, w) for k, w in enumerate(_cubic64(f))]

    acc = np.zeros((dh, dw, 4))
    for j, wy in taps(v):
        jj = index(edge, j, sh)
        for i, wx in taps(u):
            ii = index(edge, i, sw)
            live = (ii >= 0) & (jj >= 0)
            acc += (wx * wy)[..., None] * np.where(live[..., None], p[np.maximum(jj, 0), np.maximum(ii, 0)], 0.0)
    return acc, (u, v)
