"""numpy reference of jh_shadow, written from DESIGN.md 5.18 ("Shadow rule") and include/jello_hip.h ("Shadow"), not from
include/jello_shadow.h: the plan in binary64 (Python floats), the position in int64, then every binary32 operation of the coverage
one numpy operation on float32 arrays (the exact fmaf and minNum / maxNum of tests/image_ref.py), the store and the OVER blend by
tests/composite_ref.py.  `restate` is the same rule in binary64 with math.erf in place of the approximant -- what the accuracy
conditions are stated on -- and `exact` the convolution itself by a dense row integration.  The keyword variants are deliberately
wrong rules, for tests/test_shadow_spec.py's sensitivity test."""
import math

import numpy as np

import composite_ref
import warp_ref
from image_ref import fmaf32, fmax, fmin, resolve

F = np.float32
OVER, INVERT = 1, 2
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
K = 4                       # the cap window reaches K sigma to either side of a texel's row
SIGMA_FLOOR = 2.0 ** -8     # a smaller sigma is taken as this: the point-sampled shape
SIGMA_MAX = 2.0 ** 16
BOX_MAX = 2.0 ** 22         # |box coordinate|, the radius
MAX_EXTENT = 1 << 23        # image sides
BOUNDS_GROW = 3.625         # jh_shadow_bounds: the box grown by this many sigma (Phi(-3.625) = 1.45e-4 < 2^-12 = 2.44e-4)
ERF_LIMIT = 4.0             # |z| is clamped here: the approximant is 1.0f from there on
# Abramowitz & Stegun 7.1.28: erf z = 1 - (1 + a1 z + ... + a6 z^6)^-16, |error| <= 3e-7; the coefficients as binary32
ERF_A = tuple(F(v) for v in (0.0705230784, 0.0422820123, 0.0092705272, 0.0001520143, 0.0002765672, 0.0000430638))
# N, the sub-intervals of a cap, from rho = r / sigma (binary64): the first row whose bound is not below rho
N_STEPS = ((0.5, 4), (1.5, 8), (math.inf, 16))
DEFAULTS = dict(box=(0.0, 0.0, 0.0, 0.0), radius=0.0, sigma=1.0, color=(0.0, 0.0, 0.0, 1.0), matrix=IDENTITY, flags=0)


def steps(rho):
    for bound, n in N_STEPS:
        if rho <= bound:
            return n
    raise ValueError("rho is a NaN")


def erf32(z, fused=True):
    """The approximant G(z) on float32 arrays: x = minNum(|z|, 4); u = x (a1 + x (a2 + ... x a6)) by five fmaf and a product, which is
    p - 1; four times s = s (2 + s), which is p^2 - 1 of the last, so s = p^16 - 1; e = 1 - 1 / (1 + s); the sign of z."""
    z = np.asarray(z, F)
    fma = fmaf32 if fused else (lambda w, v, acc: (w * v + acc).astype(F))
    with np.errstate(all="ignore"):
        x = fmin(np.abs(z), F(ERF_LIMIT))
        q = np.broadcast_to(ERF_A[5], x.shape)
        for c in ERF_A[4::-1]:
            q = fma(x, q, c)
        s = x * q
        for _ in range(4):
            s = s * (F(2.0) + s)
        e = F(1.0) - F(1.0) / (F(1.0) + s)
        return np.copysign(e, z).astype(F)


_erf64 = np.vectorize(math.erf, otypes=[np.float64])


def legal(box, radius, sigma, matrix, flags=0, dst_size=None):
    """Nothing for a legal descriptor, ValueError naming the condition otherwise (the rectangle apart)."""
    x0, y0, x1, y1 = (float(F(v)) for v in box)
    radius, sigma = float(F(radius)), float(F(sigma))
    if not all(math.isfinite(v) for v in (x0, y0, x1, y1)):
        raise ValueError("the box is not finite")
    if not (x1 >= x0 and y1 >= y0):
        raise ValueError("the box has x1 < x0 or y1 < y0")
    if max(abs(x0), abs(y0), abs(x1), abs(y1)) > BOX_MAX:
        raise ValueError("a box coordinate above 2^22")
    if not (math.isfinite(radius) and radius >= 0.0):
        raise ValueError("the radius is negative or not finite")
    if not (math.isfinite(sigma) and 0.0 <= sigma <= SIGMA_MAX):
        raise ValueError("sigma is outside [0, 2^16] or not finite")
    if flags & ~(OVER | INVERT):
        raise ValueError("unknown flag bits")
    if dst_size is not None and (dst_size[0] > MAX_EXTENT or dst_size[1] > MAX_EXTENT):
        raise ValueError("an image extent above 2^23")
    warp_ref.inverse(matrix)


def plan(box, radius, sigma, matrix=IDENTITY, flags=0, floor_sigma=True, clamp_radius=True, k=K):
    """The plan: dict(m = (P, Q, R, S, T, W), centre = (Cx, Cy) int, a, b, radius, core, straight, sigma, inv_s, window float32, n, k).
    `floor_sigma`, `clamp_radius`, `k`: wrong variants."""
    legal(box, radius, sigma, matrix, flags)
    x0, y0, x1, y1 = (float(F(v)) for v in box)
    radius, sigma = float(F(radius)), float(F(sigma))
    cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
    a, b = (x1 - x0) * 0.5, (y1 - y0) * 0.5
    r = min(radius, a, b) if clamp_radius else radius
    sig = max(sigma, SIGMA_FLOOR) if floor_sigma else max(sigma, 2.0 ** -40)
    return dict(m=warp_ref.plan(matrix), centre=(int(round(cx * 4294967296.0)), int(round(cy * 4294967296.0))), a=F(a), b=F(b), radius=F(r),
                core=F(a - r), straight=F(b - r), sigma=F(sig), inv_s=F(1.0 / (sig * 1.4142135623730951)), window=F(k * sig), n=steps(r / sig), k=k)


def positions(pl, rect, centre_half=True):
    """(dU, dV): the int64 positions of the rectangle's texel centres relative to the box centre, 2^-32 shape units."""
    if centre_half:
        U, V = warp_ref.positions(pl["m"], rect)
    else:  # (a wrong variant: the texel's corner)
        P, Q, R, S, T, W = pl["m"]
        X2, Y2 = 2 * (rect[0] + np.arange(rect[2], dtype=np.int64)), 2 * (rect[1] + np.arange(rect[3], dtype=np.int64))
        U, V = P * X2[None, :] + Q * Y2[:, None] + R, S * X2[None, :] + T * Y2[:, None] + W
    return U - pl["centre"][0], V - pl["centre"][1]


def to_f32(d):
    """An int64 position as binary32: (float)(int32)(d >> 32) + (float)((uint32)d >> 8) 2^-24, the sum rounded once."""
    hi = (d >> 32).astype(np.int32).astype(F)
    lo = ((d & 0xFFFFFFFF) >> 8).astype(F) * F(2.0 ** -24)
    return (hi + lo).astype(F)


def coverage(pl, x, y, T=F, midpoint=True, fused=True):
    """S at the positions (x, y) relative to the centre, arrays of dtype T: float32 is the rule, float64 its restatement with
    math.erf.  `midpoint` False: the half-width at a sub-interval's far end."""
    x, y = np.asarray(x, T), np.asarray(y, T)
    a, r, core, straight, inv_s, window = (T(pl[k]) for k in ("a", "radius", "core", "straight", "inv_s", "window"))
    if T is F:
        G, fma, lo_, hi_ = (lambda z: erf32(z, fused)), (fmaf32 if fused else (lambda u, v, w: (u * v + w).astype(F))), fmax, fmin
    else:
        G, fma, lo_, hi_ = _erf64, (lambda u, v, w: u * v + w), np.fmax, np.fmin

    def band(p, w):
        return G((p + w) * inv_s) - G((p - w) * inv_s)

    with np.errstate(all="ignore"):
        acc = band(y, straight) * band(x, a)
        acc = np.broadcast_to(acc, np.broadcast(x, y).shape).astype(T)
        if r > 0:
            n = pl["n"]
            for sign in (1, -1):
                q = (y if sign > 0 else -y) - straight
                lo, hi = lo_(q - window, T(0.0)), hi_(q + window, r)
                live = hi > lo
                if not live.any():
                    continue
                t0, t1 = T(1.0) - np.sqrt(T(1.0) - lo / r), T(1.0) - np.sqrt(T(1.0) - hi / r)
                dt = (t1 - t0) * T(1.0 / n)
                m_prev, g_prev = lo, G((lo - q) * inv_s)
                for i in range(1, n + 1):
                    if i < n:
                        t = fma(T(i), dt, t0)
                        m = hi_(lo_((r * t) * (T(2.0) - t), m_prev), hi)
                    else:
                        m = hi
                    g = G((m - q) * inv_s)
                    mm = T(0.5) * (m_prev + m) if midpoint else m
                    w = core + np.sqrt((r - mm) * (r + mm))
                    acc = np.where(live, fma(g - g_prev, band(x, w), acc), acc).astype(T)
                    m_prev, g_prev = m, g
        return hi_(T(0.25) * acc, T(1.0)).astype(T)


def store_bits(color, s):
    """The texel STORE writes for the coverage s (after INVERT): colour x s, one product per channel, through the store rule."""
    with np.errstate(all="ignore"):
        c = np.array(color, F)
        p = (c[None, None, :] * np.asarray(s, F)[..., None]).astype(F)
        a_inv = F(1.0) / fmax(p[..., 3], composite_ref.STORE_FLOOR)
        out = np.concatenate([p[..., :3] * a_inv[..., None] + F(0.0), p[..., 3:] + F(0.0)], axis=-1)
        return out.astype(np.float16).view(np.uint16)


def shadow(shape, rect=None, dst_bits=None, box=(0.0, 0.0, 0.0, 0.0), radius=0.0, sigma=1.0, color=(0.0, 0.0, 0.0, 1.0), matrix=IDENTITY, flags=0,
           centre_half=True, midpoint=True, floor_sigma=True, clamp_radius=True, k=K, fused=True, src_over=True):
    """The image jh_shadow leaves: shape = (H, W), dst_bits what dst held (None: never written, transparent black)."""
    H, W = shape
    legal(box, radius, sigma, matrix, flags, (W, H))
    out = np.zeros((H, W, 4), np.uint16) if dst_bits is None else np.array(dst_bits, np.uint16)
    x0, y0, w, h = resolve((H, W), rect)
    pl = plan(box, radius, sigma, matrix, flags, floor_sigma, clamp_radius, k)
    if w == 0 or h == 0:
        return out
    dU, dV = positions(pl, (x0, y0, w, h), centre_half)
    s = coverage(pl, to_f32(dU), to_f32(dV), F, midpoint, fused)
    if flags & INVERT:
        s = (F(1.0) - s).astype(F)
    bits = store_bits(color, s)
    if flags & OVER:
        prior = out[y0:y0 + h, x0:x0 + w]
        bits = composite_ref.texels(bits, prior) if src_over else composite_ref.texels(prior, bits)  # (wrong: the shadow under dst)
    out[y0:y0 + h, x0:x0 + w] = bits
    return out


def restate(pl, rect):
    """The binary64 restatement at the rectangle's texels: the same plan scalars and int64 positions, S in binary64 with math.erf."""
    dU, dV = positions(pl, rect)
    return coverage(pl, dU.astype(np.float64) / 4294967296.0, dV.astype(np.float64) / 4294967296.0, np.float64)


def exact(a, b, r, sigma, x, y, rows=6000):
    """The Gaussian convolution of the rounded rectangle's indicator at (x, y) (floats), binary64: the straight band in closed form,
    each cap by `rows` uniform rows, each the exact mass of its rows times the exact chord term at its middle."""
    s = 1.0 / (sigma * math.sqrt(2.0))
    E = math.erf

    def band(p, w):
        return E((p + w) * s) - E((p - w) * s)

    total = band(y, b - r) * band(x, a)
    if r > 0:
        m = np.linspace(0.0, r, rows + 1)
        mid = 0.5 * (m[:-1] + m[1:])
        w = (a - r) + np.sqrt(np.maximum(r * r - mid * mid, 0.0))
        bx = _erf64((x + w) * s) - _erf64((x - w) * s)
        for sign in (1.0, -1.0):
            q = sign * y - (b - r)
            g = _erf64((m - q) * s)
            total += float(np.sum((g[1:] - g[:-1]) * bx))
    return 0.25 * total


def bounds(box, radius, sigma, matrix, dst_size):
    """jh_shadow_bounds: (x, y, width, height) of dst outside which S < 2^-12; (0, 0, 0, 0) when nothing is left."""
    legal(box, radius, sigma, matrix, 0, dst_size)
    x0, y0, x1, y1 = (float(F(v)) for v in box)
    g = BOUNDS_GROW * max(float(F(sigma)), SIGMA_FLOOR)
    if not (x1 > x0 and y1 > y0):
        return (0, 0, 0, 0)
    a, b, c, d, e, f = [float(v) for v in matrix]
    lo, hi = [math.inf, math.inf], [-math.inf, -math.inf]
    for py in (y0 - g, y1 + g):
        for px in (x0 - g, x1 + g):
            for k, v in enumerate(((a * px + c * py) + e, (b * px + d * py) + f)):
                if v != v:
                    lo[k], hi[k] = -math.inf, math.inf
                lo[k], hi[k] = min(lo[k], v), max(hi[k], v)
    first, count = [], []
    for k in range(2):
        p0 = lo[k] if math.isinf(lo[k]) else math.floor(lo[k]) - 1
        p1 = hi[k] if math.isinf(hi[k]) else math.ceil(hi[k]) + 1
        p0, p1 = max(p0, 0), min(p1, dst_size[k])
        if not p1 > p0:
            return (0, 0, 0, 0)
        first.append(int(p0))
        count.append(int(p1 - p0))
    return (first[0], first[1], count[0], count[1])
