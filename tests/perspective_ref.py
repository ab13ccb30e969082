"""The perspective rule (include/jello_hip.h "Perspective") in numpy, written from the rule alone: what jh_perspective
has to produce, bit for bit.  The plan is Python floats (binary64, one rounding per operation, nothing contracted); the position is
numpy float64 with every operation one numpy operation, so IEEE gives the same bits; the taps, the index rules and the cubic weights
are tests/warp_ref.py's helpers, the sums binary32 with the rule's fmaf (image_ref.fmaf32).  The adjugate and the position formula
are written out here, independently of include/jello_perspective.h.

  adjugate(matrix)      (adj[9] row-major, det) (ValueError for an illegal matrix)
  plan(matrix)          the nine doubles G
  positions(G, rect)    (U, V, void): int64 positions and the void mask of a destination rectangle's texels
  bounds(...)           the rectangle of jh_perspective_bounds
  perspective(...)      the image jh_perspective leaves in dst

plan(), positions() and perspective() take keyword switches that build near misses of the rule (tests/test_perspective_spec.py asserts
that the battery of tests/perspective_cases.py tells each of the first eight from the rule, and that the ninth is the rule): fused=True
(an fma in the numerator: fma(G0, x', G1 y') + G2), divide=True (n / den instead of n (1 / den)), den_ge=True (den >= 0 as the front
test), centre0=True (texel centres at +0), trunc=True (truncation instead of rint), clamp=False (no clamp at 2^22 -- held at 2^29 only
to stay inside int64), void_clamp=True (a void texel reads position (0, 0) under CLAMP instead of storing zero), row_major=True (the
matrix read row by row), norm_divide=True (G = adj / 2^k, a division, in place of the ldexp)."""
import math
from fractions import Fraction

import numpy as np

import warp_ref
from image_ref import fmaf32, fmax, operands, same_bits  # noqa: F401 (same_bits is part of this module's interface)
from warp_ref import BICUBIC, BILINEAR, CLAMP, EDGES, FILTERS, GROW, MAX_SIDE, MIRROR, NEAREST, REPEAT, STRAIGHT, ZERO  # noqa: F401

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
MAX_POSITION = float(1 << 22)


def affine(m6):
    a, b, c, d, e, f = (float(v) for v in m6)
    return (a, b, 0.0, c, d, 0.0, e, f, 1.0)


def adjugate(matrix, row_major=False):
    """(adj, det): the nine two-product differences, row-major, and det = ((a adj00) + (c adj10)) + (e adj20)."""
    m = [float(v) for v in matrix]
    if len(m) != 9:
        raise ValueError("nine entries")
    if not all(math.isfinite(v) for v in m):
        raise ValueError("a matrix entry is not finite")
    if row_major:  # (a wrong variant)
        a, c, e, b, d, f, p, q, s = m
    else:
        a, b, p, c, d, q, e, f, s = m
    adj = (d * s - f * q, e * q - c * s, c * f - e * d,
           f * p - b * s, a * s - e * p, e * b - a * f,
           b * q - d * p, c * p - a * q, a * d - c * b)
    if not all(math.isfinite(v) for v in adj):
        raise ValueError("an adjugate entry is not finite")
    det = ((a * adj[0]) + (c * adj[3])) + (e * adj[6])
    if not math.isfinite(det):
        raise ValueError("the determinant is not finite")
    if det == 0.0:
        raise ValueError("the determinant is 0")
    return adj, det


def plan(matrix, row_major=False, norm_divide=False):
    """G: adj scaled by 2^-k, 2^(k-1) < max |adj| <= 2^k, negated when det < 0."""
    adj, det = adjugate(matrix, row_major)
    top = max(abs(v) for v in adj)
    mant, k = math.frexp(top)  # top = mant 2^k, 1/2 <= mant < 1
    if mant == 0.5:
        k -= 1
    if norm_divide:
        g = [v / (2.0 ** k) for v in adj]
    else:
        g = [math.ldexp(v, -k) for v in adj]
    return tuple(-v if det < 0.0 else v for v in g)


def positions(G, dst_rect, fused=False, divide=False, den_ge=False, centre0=False, trunc=False, clamp=True):
    """(U, V, void): int64 arrays (dh, dw) of the destination rectangle's texels (0 where void) and the bool mask of the void ones."""
    dx, dy, dw, dh = dst_rect
    half = 0.0 if centre0 else 0.5
    xp = (np.arange(dx, dx + dw, dtype=np.float64) + half)[None, :]
    yp = (np.arange(dy, dy + dh, dtype=np.float64) + half)[:, None]
    G = [np.float64(g) for g in G]

    def three(g0, g1, g2):
        if fused:
            return _fma64(g0, xp, g1 * yp) + g2
        return ((g0 * xp) + (g1 * yp)) + g2

    with np.errstate(all="ignore"):
        nu, nv, den = three(*G[0:3]), three(*G[3:6]), three(*G[6:9])
        nu, nv, den = np.broadcast_arrays(nu, nv, den)
        if divide:
            u, v = nu / den, nv / den
        else:
            q = np.float64(1.0) / den
            u, v = nu * q, nv * q
        void = ~(den >= 0.0 if den_ge else den > 0.0) | np.isnan(u) | np.isnan(v)
        lim = MAX_POSITION if clamp else float(1 << 29)
        out = []
        for c in (u, v):
            c = np.where(void, 0.0, np.clip(c, -lim, lim))
            scaled = c * 4294967296.0  # exact
            out.append((np.trunc(scaled) if trunc else np.rint(scaled)).astype(np.int64))  # (np.rint: ties to even)
    return out[0], out[1], void


def _fma64(a, x, b):
    """fma(a, x, b) in binary64, exactly, elementwise (through exact rationals: slow, for the near miss only)."""
    x, b = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(b, np.float64))
    out = np.empty(x.shape, np.float64)
    for i in np.ndindex(x.shape):
        if not (math.isfinite(a) and math.isfinite(x[i]) and math.isfinite(b[i])):
            out[i] = float(a) * x[i] + b[i]
        else:
            out[i] = float(Fraction(float(a)) * Fraction(float(x[i])) + Fraction(float(b[i])))
    return out


def bounds(matrix, src_size, filt, dst_size):
    """jh_perspective_bounds: (x, y, width, height), (0, 0, 0, 0) when empty, the whole destination when a corner has w <= 0."""
    adjugate(matrix)
    a, b, p, c, d, q, e, f, s = [float(v) for v in matrix]
    g = GROW[filt]
    lo, hi = [math.inf, math.inf], [-math.inf, -math.inf]
    whole = False

    def div(n, w):
        try:
            return n / w
        except OverflowError:
            return math.copysign(math.inf, n)

    for y in (-g, float(src_size[1]) + g):
        for x in (-g, float(src_size[0]) + g):
            xw, yw, w = ((a * x) + (c * y)) + e, ((b * x) + (d * y)) + f, ((p * x) + (q * y)) + s
            if not w > 0.0:
                whole = True
                continue
            for k, v in enumerate((div(xw, w), div(yw, w))):
                if v != v:
                    lo[k], hi[k] = -math.inf, math.inf
                lo[k], hi[k] = min(lo[k], v), max(hi[k], v)
    if whole:
        lo, hi = [-math.inf, -math.inf], [math.inf, math.inf]
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


def perspective(src_bits, dst_shape, matrix, filt=BILINEAR, edge=ZERO, flags=0, src_rect=None, dst_rect=None, dst_bits=None, row_major=False,
                norm_divide=False, void_clamp=False, **position_variant):
    """The image jh_perspective leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero).
    dst_shape = (height, width) of dst; dst_bits: what dst held (None: a never-written dst, transparent black).  Rectangles are (x,
    y, width, height), None: the whole image.  Returns (height, width, 4) uint16."""
    if filt not in FILTERS or edge not in EDGES or flags & ~STRAIGHT:
        raise ValueError("unknown filter, edge or flag bits")
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    out = np.zeros(tuple(dst_shape[:2]) + (4,), np.uint16) if dst_bits is None else np.array(dst_bits, np.uint16)
    (sx, sy, sw, sh), drect = warp_ref.rects(src_bits.shape, out.shape, src_rect, dst_rect)
    G = plan(matrix, row_major, norm_divide)
    dx, dy, dw, dh = drect
    if dw == 0 or dh == 0:
        return out
    U, V, void = positions(G, drect, **position_variant)
    straight = bool(flags & STRAIGHT)
    p = operands(src_bits[sy:sy + sh, sx:sx + sw], not straight, np.float32)
    with np.errstate(all="ignore"):
        def resolve(i, n):
            if not void_clamp:  # (the wrong variant: a void texel reads position (0, 0) under CLAMP)
                return warp_ref.index(edge, i, n)
            return np.where(void, warp_ref.index(CLAMP, i, n), warp_ref.index(edge, i, n))

        ix = [(resolve(i, sw), w[..., None]) for i, w in warp_ref.axis_taps(filt, U)]
        iy = [(resolve(j, sh), w[..., None]) for j, w in warp_ref.axis_taps(filt, V)]

        def operand(i, j):
            if sw == 0 or sh == 0:
                return np.zeros((dh, dw, 4), np.float32)
            live = (i >= 0) & (j >= 0)
            return np.where(live[..., None], p[np.maximum(j, 0), np.maximum(i, 0)], np.float32(0.0)).astype(np.float32)

        zero4 = np.zeros((dh, dw, 4), np.float32)
        acc = zero4
        for j, wy in iy:  # rows, then columns
            h = zero4
            for i, wx in ix:
                h = fmaf32(wx, operand(i, j), h)
            acc = fmaf32(wy, h, acc)
        if straight:
            texels = acc
        else:
            zero = np.float32(0.0)
            a_inv = np.float32(1.0) / fmax(acc[..., 3], np.float32(1e-6))
            texels = np.concatenate([acc[..., :3] * a_inv[..., None] + zero, acc[..., 3:] + zero], axis=-1)
        bits = texels.astype(np.float32).astype(np.float16).view(np.uint16)
        if not void_clamp:
            bits = np.where(void[..., None], np.uint16(0), bits)  # a void texel: four +0.0
        out[dy:dy + dh, dx:dx + dw] = bits
    return out
