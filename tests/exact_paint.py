"""What a pixel is painted with, from the definitions, in numpy float64: gradient ramps, the linear / two-point
conical / sweep gradient parameter, the extend modes, the bilinear image sample, and fine's composite and store.  The
reference of tests/test_paint_spec.py (on the oracle) and tests/test_gpu_paint.py (on the HIP image); it reads neither
oracle/ nor tests/fine_by_hand.py.

The rules, with the reference shader's lines:

* The sampling point of pixel (x, y) is its TOP-LEFT CORNER (x, y), not its centre: fine.wgsl:895 builds
  `xy = vec2(f32(global_id.x * PIXELS_PER_THREAD), f32(global_id.y))` without an offset, and the gradient and image
  commands evaluate at `vec2(xy.x + f32(i), xy.y)` (fine.wgsl:980-982, 1002-1003, 1039-1040, 1071-1072).
* A gradient pixel is painted with the f16 ramp texel at index round(extend(t) * 511) (fine.wgsl:983, 1027, 1061;
  extend_mode: fine.wgsl:800-812).  The texel is rounded to f16 BEFORE fine's un-premultiplying store
  (fine.wgsl:1092-1102) divides by alpha: the division amplifies the texel's rounding, so the order is part of the rule.
* t of a radial gradient is the canvas / PDF two-point conical definition: the largest t with r(t) >= 0 and
  |p - c(t)| = r(t); where there is none the pixel is not painted.
* An image is sampled at the inverse transform (u, v) of the pixel corner from the texels (floor u, ceil u) x (floor v,
  ceil v); a texel outside the image is transparent black; there is no sample where u >= width or v >= height
  (fine.wgsl:1072-1084).  So the image fades over one texel on its left and top side and on its right and bottom side
  alike (ceil u = width is outside), and is cut at u = width where it has already faded out.

Every function takes `defect`: the name of one near miss of the rule (DEFECTS), for the sensitivity tests.

The device evaluates t in f32, so a gradient gives for each pixel the SET of ramp indices reachable within t +- delta
(`index_candidates`), including both ends where a wrap or fold lies inside that interval; a pixel is right if it equals
the pixel rule for one index of the set within the store's bound (`check_image`)."""
import math

import numpy as np

NUM_SAMPLES = 512
U = 2.0 ** -24          # the unit of every f32 rounding count
GRADIENT_EPSILON = 2.0 ** -12   # draw_leaf.wgsl:151

DEFECTS = ("centre", "index512", "floor_index", "reflect_as_repeat", "no_swapped_flip", "no_t_sign", "ramp_linear_light",
           "ramp_not_premultiplied", "counts_by_floor", "unpremul_before_f16", "image_texel_centres",
           "image_interp_before_premul", "alpha_as_srgb")

PAD, REPEAT, REFLECT = 0, 1, 2


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def srgb_encode(l):
    l = np.asarray(l, np.float64)
    return np.where(l <= 0.0031308, 12.92 * l, 1.055 * np.power(np.maximum(l, 0.0), 1.0 / 2.4) - 0.055)


def srgb_decode(s):
    """IEC 61966-2-1."""
    s = np.asarray(s, np.float64)
    return np.where(s <= 0.04045, s / 12.92, np.power((np.maximum(s, 0.0) + 0.055) / 1.055, 2.4))


def round_half_away(x):
    return math.floor(abs(x) + 0.5) * (1 if x >= 0 else -1)


def to_f16(a):
    """A ramp texel's way from float64 to f16, as the host stores it: RTNE to f32, then to the nearest f16 with TIES AWAY
    FROM ZERO (the reference's gfx/color.go:11-25 converts with jmath.Float16bits, which drops the f32's low 12 bits and
    adds half an f16 ULP; make_ramp's premul16 does the same).  An f32 that is an exact f16 tie comes about through
    the first rounding, about once in 2^13 texels; RTNE would send it to the even neighbour.  Below 2^-14 the f16 is
    subnormal and the conversion's f32 product with 2^-112 rounds once more, RTNE, to a multiple of 2^-37."""
    x = np.abs(f32(a))
    m, e = np.frexp(x)
    xt = np.ldexp(np.floor(m * 4096.0), e - 12)                 # the f32 without its low 12 mantissa bits
    ulp = np.ldexp(1.0, e - 11)
    normal = np.floor(xt / ulp + 0.5) * ulp
    tiny = np.floor(np.rint(xt * 2.0 ** 37) * 2.0 ** -13 + 0.5) * 2.0 ** -24
    h = np.where(xt >= 2.0 ** -14, normal, tiny)
    return (np.sign(np.asarray(a, np.float64)) * np.minimum(h, 65504.0)).astype(np.float16)


# ---- ramp ------------------------------------------------------------------------------------------------------------
def segment_counts(offsets, defect=None):
    """Samples per segment of the stops (after the stop at 0 is prepended): the rule above make_ramp."""
    offs = [float(np.float32(o)) for o in offsets]
    if offs[0] != 0.0:
        offs = [0.0] + offs
    counts, remaining = [], NUM_SAMPLES
    for i in range(1, len(offs)):
        if i == len(offs) - 1:
            n = remaining
        else:
            frac = float(np.float32(offs[i]) - np.float32(offs[i - 1]))     # an f32 difference
            x = float(np.float32(NUM_SAMPLES) * np.float32(frac))
            n = math.floor(x) if defect == "counts_by_floor" else round_half_away(x)
            n = min(remaining, n)
        remaining -= n
        counts.append(n)
    return counts


def ramp(stops, defect=None):
    """stops: [(offset, (r, g, b, a))], linear-light un-premultiplied colours.  Returns (512 x 4 float64 premultiplied,
    its f16 rounding)."""
    stops = [(float(np.float32(o)), tuple(float(v) for v in c)) for o, c in stops]
    if stops[0][0] != 0.0:
        stops = [(0.0, stops[0][1])] + stops
    counts = segment_counts([o for o, _ in stops], defect)
    rows = []
    for i, n in enumerate(counts):
        c0, c1 = np.array(stops[i][1]), np.array(stops[i + 1][1])
        if n == 0:
            continue
        t = np.ones(1) if n == 1 else np.arange(n) / (n - 1.0)
        t = t[:, None]
        if n == 1:
            rgb, a = np.broadcast_to(c1[:3], (1, 3)), np.full((1, 1), c1[3])
        elif defect == "ramp_linear_light":
            rgb, a = c0[:3] + (c1[:3] - c0[:3]) * t, c0[3] + (c1[3] - c0[3]) * t
        else:
            e0, e1 = srgb_encode(c0[:3]), srgb_encode(c1[:3])
            rgb, a = srgb_decode(e0 + (e1 - e0) * t), c0[3] + (c1[3] - c0[3]) * t
        rows.append(np.concatenate([rgb if defect == "ramp_not_premultiplied" else rgb * a, a], axis=1))
    out = np.concatenate(rows, axis=0)
    assert out.shape == (NUM_SAMPLES, 4)
    return out, to_f16(out)


# ---- gradient parameters ---------------------------------------------------------------------------------------------
def affine_mul(m, n):
    """m after n; (a, b, c, d, e, f): x' = a x + c y + e, y' = b x + d y + f."""
    a, b, c, d, e, f = m
    A, B, C, D, E, F = n
    return (a * A + c * B, b * A + d * B, a * C + c * D, b * C + d * D, a * E + c * F + e, b * E + d * F + f)


def affine_inverse_apply(m, x, y):
    a, b, c, d, e, f = m
    det = a * d - b * c
    return ((x - e) * d - (y - f) * c) / det, (-(x - e) * b + (y - f) * a) / det


def affine_cond(m):
    a, b, c, d = m[:4]
    s = np.linalg.svd(np.array([[a, c], [b, d]]), compute_uv=False)
    return float(s[0] / s[1])


def pixel_grid(width, height, defect=None):
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    off = 0.5 if defect == "centre" else 0.0
    return xs + off, ys + off


def linear_t(x, y, p0, p1):
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    return ((x - p0[0]) * dx + (y - p0[1]) * dy) / (dx * dx + dy * dy)


def radial_t(x, y, c0, r0, c1, r1, defect=None):
    """The largest t with r(t) >= 0 and |p - c(t)| = r(t), c(t) = c0 + t (c1 - c0), r(t) = r0 + t (r1 - r0); NaN where
    there is none."""
    pdx, pdy = x - c0[0], y - c0[1]
    cdx, cdy = c1[0] - c0[0], c1[1] - c0[1]
    dr = r1 - r0
    a = cdx * cdx + cdy * cdy - dr * dr
    b = pdx * cdx + pdy * cdy + r0 * dr
    c = pdx * pdx + pdy * pdy - r0 * r0
    with np.errstate(invalid="ignore", divide="ignore"):
        if abs(a) <= 1e-12 * (cdx * cdx + cdy * cdy + dr * dr):     # one root: a t^2 - 2 b t + c = 0 with a = 0
            t = np.where(b != 0, c / (2.0 * b), np.nan)
            t = np.where(r0 + t * dr >= 0, t, np.nan)
        else:
            disc = b * b - a * c
            sq = np.sqrt(np.maximum(disc, 0.0))
            t_hi, t_lo = (b + sq) / a, (b - sq) / a
            if a < 0:
                t_hi, t_lo = t_lo, t_hi
            t = np.where(r0 + t_hi * dr >= 0, t_hi, t_lo)
            t = np.where((disc < 0) | (r0 + t * dr < 0), np.nan, t)
    if defect == "no_swapped_flip" and r1 == 0:
        t = 1.0 - t
    if defect == "no_t_sign" and r0 > r1 > 0:
        t = 2.0 * r0 / (r0 - r1) - t
    return t


def sweep_turns(x, y, centre):
    """The angle of p - centre from +x towards +y, in turns, in [0, 1)."""
    phi = np.arctan2(y - centre[1], x - centre[0]) / (2.0 * math.pi)
    return np.where(phi < 0, phi + 1.0, phi)


def extend(t, mode, defect=None):
    if mode == PAD:
        return np.clip(t, 0.0, 1.0)
    if mode == REPEAT or defect == "reflect_as_repeat":
        return t - np.floor(t)
    return np.abs(t - 2.0 * np.round(0.5 * t))


def sweep_polynomial_distance(n=1 << 16):
    """max over s in [0, 1] of |P(s) - atan(s) / 2 pi| for the shader's four-term polynomial (fine.wgsl:1054), in
    turns: a property of the rule, measured on a dense grid."""
    s = np.linspace(0.0, 1.0, n + 1)
    q = s * s
    p = s * (0.15912117063999176 + q * (-5.185396969318390e-2 + q * (2.476101927459240e-2 + q * (-7.0547382347285748e-3))))
    return float(np.abs(p - np.arctan(s) / (2.0 * math.pi)).max())


def ramp_index(e, defect=None):
    if defect == "index512":
        return np.clip(np.round(e * 512.0), 0, 511).astype(np.int64)
    if defect == "floor_index":
        return np.clip(np.floor(e * 511.0), 0, 511).astype(np.int64)
    return np.clip(np.floor(e * 511.0 + 0.5), 0, 511).astype(np.int64)


K_SAMPLES = 9
N_CAND = 2 * (K_SAMPLES + 3) + 2


def index_candidates(t, delta, mode, defect=None, wrap_unit=None):
    """(H, W, K) ramp indices reachable within t +- delta.  The interval is sampled densely enough that two samples are
    at most half a ramp step apart where delta * 511 <= 2, each sample is rounded both ways on a tie, and an integer t
    inside the interval (a wrap of Repeat, a fold of Reflect) is a sample of its own: for Repeat with both ends.
    wrap_unit = (t0, scale): t = (phi - t0) * scale of a sweep, whose phi wraps at whole turns before it is scaled."""
    f = np.linspace(-1.0, 1.0, K_SAMPLES)
    tau = t[..., None] + delta[..., None] * f
    if wrap_unit is not None:
        t0, scale = wrap_unit
        phi = tau / scale + t0
        k = np.round(phi)
        seam = np.abs(phi - k)[..., K_SAMPLES // 2] <= np.abs(delta / scale)
        lo = (phi - np.floor(phi) - t0) * scale
        ends = np.stack([(0.0 - t0) * scale + 0 * t, (1.0 - t0) * scale + 0 * t], axis=-1)
        tau = np.concatenate([lo, np.where(seam[..., None], ends, lo[..., :2])], axis=-1)
    else:
        tau = np.concatenate([tau, tau[..., :2]], axis=-1)      # (every kind: one K for all draws of a case)
    n = np.round(t)
    inside = np.abs(t - n) <= delta
    tau = np.concatenate([tau, np.where(inside, n, t)[..., None]], axis=-1)
    e = extend(tau, mode, defect)
    if defect in ("index512", "floor_index"):
        cand = [ramp_index(e, defect)]
    else:
        cand = [np.clip(np.floor(e * 511.0 + 0.5), 0, 511).astype(np.int64), np.clip(np.ceil(e * 511.0 - 0.5), 0, 511).astype(np.int64)]
    wraps = inside & (mode == REPEAT or (mode == REFLECT and defect == "reflect_as_repeat"))
    cand.append(np.where(wraps, 0, cand[0][..., -1])[..., None])        # (every mode: one K for all draws of a case)
    cand.append(np.where(wraps, 511, cand[0][..., -1])[..., None])
    if len(cand) == 3:
        cand.insert(1, cand[0])
    return np.concatenate(cand, axis=-1)


# ---- image -----------------------------------------------------------------------------------------------------------
def decode_texels(rgba8, srgb=True, defect=None):
    """(h, w, 4) uint8 -> float64 un-premultiplied linear colour."""
    v = np.asarray(rgba8, np.float64) / 255.0
    out = v.copy()
    if srgb:
        out[..., :3] = srgb_decode(v[..., :3])
        if defect == "alpha_as_srgb":
            out[..., 3] = srgb_decode(v[..., 3])
    return out


def image_sample(u, v, rgba8, srgb=True, defect=None):
    """Premultiplied float64 sample (..., 4) at texel coordinates (u, v), and the mask of points that have a sample."""
    tex = decode_texels(rgba8, srgb, defect)
    h, w = tex.shape[:2]
    if defect == "image_texel_centres":
        u, v = u - 0.5, v - 0.5
    pre = tex.copy()
    if defect != "image_interp_before_premul":
        pre[..., :3] *= pre[..., 3:4]

    def texel(tx, ty):
        ok = (tx >= 0) & (ty >= 0) & (tx < w) & (ty < h)
        t = pre[np.clip(ty, 0, h - 1).astype(np.int64), np.clip(tx, 0, w - 1).astype(np.int64)]
        return np.where(ok[..., None], t, 0.0)
    fu, fv, cu, cv = np.floor(u), np.floor(v), np.ceil(u), np.ceil(v)
    fru, frv = (u - fu)[..., None], (v - fv)[..., None]
    a, b, c, d = texel(fu, fv), texel(fu, cv), texel(cu, fv), texel(cu, cv)
    ab = a * (1 - frv) + b * frv
    cd = c * (1 - frv) + d * frv
    fg = ab * (1 - fru) + cd * fru
    if defect == "image_interp_before_premul":
        fg = np.concatenate([fg[..., :3] * fg[..., 3:4], fg[..., 3:4]], axis=-1)
    return fg, (u < w) & (v < h)


# ---- pixel -----------------------------------------------------------------------------------------------------------
def over(bg, fg, area):
    fgi = fg * area
    return bg * (1.0 - fgi[..., 3:4]) + fgi


def store(c):
    """fine's un-premultiplying store (fine.wgsl:1092-1102), before the f16 rounding."""
    a = c[..., 3:4]
    return np.concatenate([c[..., :3] / np.maximum(a, 1e-6), a], axis=-1)


def f16_half_ulp(v):
    v = np.maximum(np.abs(v), 2.0 ** -14)
    return 0.5 * 2.0 ** (np.floor(np.log2(v)) - 10)


# roundings of the composite, in units of 2^-24 (see the table in tests/test_gpu_paint.py)
C_OVER_RESULT = 3.0     # fg * area, bg * k, their sum: each relative to a term that is at most the result
C_OVER_BG = 3.0         # fg.a * area and 1 - that (absolute, <= 1 each) scale the base; the host's f32 premultiply of it
C_DIV = 2.0             # 1 / max(a, 1e-6) and the product with it
C_LAYER = 3.0           # a layer's rgba * area * alpha (two products) and blend's bg * (1 - a) + src, per term as above


def store_bound(premul, base, fg_err=0.0, area_err=0.0, fg=None, layers=0):
    """Bound of |stored - store(premul)| per channel: half an f16 ULP of the value, the f32 roundings of `over` and of
    the division (C_* above), and what an error of the paint (fg_err, per channel) or of the area (area_err) adds."""
    c, a = premul[..., :3], premul[..., 3:4]
    err = U * ((C_OVER_RESULT + layers * C_LAYER) * premul + (C_OVER_BG + layers * C_LAYER) * base)
    err = err + fg_err
    if fg is not None:
        err = err + area_err[..., None] * (fg + base * fg[..., 3:4])
    ea, ec = err[..., 3:4], err[..., :3]
    am = np.maximum(a, 1e-6)
    v = c / am
    ev = ec / am + v * ea / am + C_DIV * U * v
    out = np.concatenate([ev, ea], axis=-1)
    return out + f16_half_ulp(np.concatenate([v, a], axis=-1))


# ---- delta of t: counted f32 roundings, in units of 2^-24 * the largest intermediate (table in test_gpu_paint.py) -----
C_LIN = 24.0        # draw_leaf: two transformed points (4 each), their difference (1), dot (3), 1 / dot (1), the product
                    # (1), line_c (3); fine: two products and two sums, the product with the lane's pixel and its sum (6)
C_EXT = 4.0         # extend (a product, round / floor, a difference), the product with 511
C_RAD_P = 40.0      # as a displacement of the pixel: inverse transform (4 per coefficient, 7 per translation),
                    # two_point_to_unit_line (the same again), two matrix products (3 + 5 each), the scale (1), fine's
                    # two products and two sums per coordinate (4)
C_RAD_T = 20.0      # on t itself: focal_x (2), cf (4), its length (4), radius (1), 1 / radius (1), fine's squares, sum,
                    # root, product, difference (6), focal_x + t_sign * t (2)
C_SWEEP_P = 16.0    # inverse of transform * translation (4 + 7), fine's two products and two sums (4), |x|, |y| exact
C_SWEEP_PHI = 12.0  # in turns: the quotient (1), s (1), four Horner steps (8), the two folds that subtract (2)
C_SWEEP_T = 6.0     # (phi - t0) * scale (2), 1 / (t1 - t0) (2), t0 and t1 as stored f32 (2)
C_IMG_UV = 12.0     # inverse transform (4 + 4), fine's two products and two sums (4)
C_IMG_MIX = 12.0    # alpha / 255, the table's rounding, premultiply (3); two mixes of 1 - t, two products, a sum (8); 1 spare
MAX_STEPS = 2.0     # a pixel whose delta * 511 exceeds this many ramp steps is left out
FD = 2.0 ** -10     # step of the float64 derivative of t, and the width of the valid / invalid boundary band


class Paint:
    """What one draw may paint each pixel with: cand (H, W, K, 4) premultiplied paints, err (H, W, 4) bound of the
    paint's own error (images), state (H, W): 1 painted, 0 not painted, 2 either; skip (H, W): left out."""
    def __init__(self, cand, err, state, skip):
        self.cand, self.err, self.state, self.skip = cand, err, state, skip


def _brush_grid(width, height, transform, defect):
    x, y = pixel_grid(width, height, defect)
    if transform is not None:
        x, y = affine_inverse_apply(transform, x, y)
    return x, y


def _max_coordinate(width, height, transform, points):
    m = float(max(width, height, 16))
    for px, py in points:
        if transform is not None:
            a, b, c, d, e, f = transform
            px, py = a * px + c * py + e, b * px + d * py + f
        m = max(m, abs(px), abs(py))
    return m


def gradient_paint(g, width, height, defect=None):
    """g: a gradient draw of tests/paint_cases.py (kind, geometry, stops, extend, transform: the f32 product of path
    and brush transform, or None)."""
    T = None if g.transform is None else tuple(f32(g.transform))
    x, y = _brush_grid(width, height, T, defect)
    scale = 1.0 if T is None else math.sqrt(abs(T[0] * T[3] - T[1] * T[2]))
    cond = 1.0 if T is None else affine_cond(T)
    wrap = None
    with np.errstate(invalid="ignore", divide="ignore"):
        if g.kind == "linear":
            p0, p1 = f32(g.p0), f32(g.p1)
            t = linear_t(x, y, p0, p1)
            M = _max_coordinate(width, height, T, [p0, p1])
            d = scale * math.hypot(p1[0] - p0[0], p1[1] - p0[1])
            delta = U * C_LIN * (M / d) * (1.0 + np.abs(t))
            state = np.ones(t.shape, np.int8)
        elif g.kind == "radial":
            c0, c1, r0, r1 = f32(g.p0), f32(g.p1), float(f32(g.r0)), float(f32(g.r1))
            fn = lambda xx, yy: radial_t(xx, yy, c0, r0, c1, r1, defect)
            t = fn(x, y)
            h = FD / scale
            nb = [fn(x + h, y), fn(x - h, y), fn(x, y + h), fn(x, y - h)]
            # |dt / d(device pixel)|, by the 1-norm: brush-space central differences, stretched by the transform
            if T is None:
                gx, gy = (nb[0] - nb[1]) / (2 * h), (nb[2] - nb[3]) / (2 * h)
                grad = np.abs(gx) + np.abs(gy)
            else:
                grad = (np.abs(nb[0] - nb[1]) + np.abs(nb[2] - nb[3])) / (2 * h) * cond / scale
            M = _max_coordinate(width, height, T, [c0, c1]) + scale * max(r0, r1)
            eps_p = U * C_RAD_P * M * cond
            amp, fx = 1.0, 0.0
            a0, a1, q0, q1 = r0, r1, c0, c1
            # the strip threshold (draw_leaf.wgsl:164): within it r1 is read as r0.  The battery sits on it exactly
            # (r0 = r1) or far from it, so the term is 0; a case in between would need it
            assert r0 == r1 or abs(r0 - r1) > 64 * GRADIENT_EPSILON, "radii within the strip threshold but not equal"
            if abs(r0 - r1) > GRADIENT_EPSILON:
                if a1 == 0.0:
                    a0, a1, q0, q1 = a1, a0, q1, q0
                fx = a0 / (a0 - a1)
                cf = (1 - fx) * q0 + fx * q1
                dist = math.hypot(*(cf - q1))
                if dist > 0:
                    R = a1 / dist
                    # the focal-on-circle threshold (draw_leaf.wgsl:201): within it the radius is read as 1; as above
                    assert R == 1.0 or abs(R - 1.0) > 64 * GRADIENT_EPSILON, "radius within the focal-on-circle threshold but not 1"
                    if abs(R - 1.0) > GRADIENT_EPSILON:
                        amp = max(1.0, max(R * R, 1.0) / abs(R * R - 1.0))
            delta = eps_p * grad + U * C_RAD_T * amp * (np.abs(t) + abs(fx) + 1.0)
            if c0[0] == c1[0] and c0[1] == c1[1]:
                # the shifted centre of a concentric gradient (draw_leaf.wgsl:178-181): c0 moves by (eps, eps), c(t) by
                # (1 - t) of that, which is a displacement of the pixel
                delta = delta + GRADIENT_EPSILON * scale * grad * np.maximum(1.0, np.abs(1.0 - t))
            valid = np.isfinite(t)
            nvalid = sum(np.isfinite(n).astype(np.int64) for n in nb)
            state = np.where(valid & (nvalid == 4), 1, np.where(~valid & (nvalid == 0), 0, 2)).astype(np.int8)
            delta = np.where(np.isfinite(delta), delta, np.inf)
            t = np.where(valid, t, 0.0)
        elif g.kind == "sweep":
            c = f32(g.p0)
            t0, t1 = g.t0 / (2.0 * math.pi), g.t1 / (2.0 * math.pi)
            phi = sweep_turns(x, y, c)
            s = 1.0 / (t1 - t0)
            t = (phi - t0) * s
            r_dev = scale * np.hypot(x - c[0], y - c[1])
            M = _max_coordinate(width, height, T, [c])
            dphi = sweep_polynomial_distance() + U * C_SWEEP_PHI + U * C_SWEEP_P * M * cond * math.sqrt(2.0) / (2.0 * math.pi * r_dev)
            delta = dphi * abs(s) + U * C_SWEEP_T * (1.0 + np.abs(t) + max(abs(t0), abs(t1)) * abs(s))
            delta = np.where(r_dev > 0, delta, np.inf)
            state = np.ones(t.shape, np.int8)
            wrap = (t0, s)
        else:
            raise ValueError(g.kind)
        delta = delta + U * C_EXT * (1.0 + np.abs(t))
    delta = np.where(state == 0, 0.0, delta)
    skip = ~(delta * 511.0 <= MAX_STEPS)
    delta = np.where(skip, 0.0, delta)
    idx = index_candidates(t, delta, g.extend, defect, wrap)
    r64, r16 = ramp(g.stops, defect)
    table = r64 if defect == "unpremul_before_f16" else r16.astype(np.float64)
    return Paint(table[idx], np.zeros(t.shape + (4,)), state, skip)


def image_paint(g, width, height, defect=None):
    T = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0) if g.transform is None else tuple(f32(g.transform))
    x, y = pixel_grid(width, height, defect)
    u, v = affine_inverse_apply(T, x, y)
    a, b, c, d, e, f = T
    det = a * d - b * c
    M = float(max(width, height, abs(e), abs(f), 16))
    eu = U * C_IMG_UV * (abs(d) + abs(c)) / abs(det) * M * (abs(a * d) + abs(b * c)) / abs(det)
    ev = U * C_IMG_UV * (abs(b) + abs(a)) / abs(det) * M * (abs(a * d) + abs(b * c)) / abs(det)
    h, w = g.pixels.shape[:2]
    fg, has = image_sample(u, v, g.pixels, g.srgb, defect)
    err = np.zeros_like(fg)
    for du in (-eu, 0.0, eu):
        for dv in (-ev, 0.0, ev):
            uu = np.where((np.abs(u - np.round(u)) <= eu) & (du == 0.0), np.round(u), u + du)
            vv = np.where((np.abs(v - np.round(v)) <= ev) & (dv == 0.0), np.round(v), v + dv)
            err = np.maximum(err, np.abs(image_sample(uu, vv, g.pixels, g.srgb, defect)[0] - fg))
    err = err + U * C_IMG_MIX
    # at the cut, within the bound of u or v, both readings of u < width and v < height are allowed
    near_cut = ((np.abs(u - w) <= eu) & (v < h + ev)) | ((np.abs(v - h) <= ev) & (u < w + eu))
    state = np.where(near_cut, 2, np.where(has, 1, 0)).astype(np.int8)
    return Paint(fg[..., None, :], err, state, np.zeros(u.shape, bool))


def expected(case, defect=None):
    """Per pixel of the case: (want (H, W, K, 4) stored values, bound (H, W, K, 4), state (H, W), skip (H, W),
    painted (H, W): a draw covers the pixel)."""
    W, H = case.width, case.height
    base = np.array(case.base, np.float64)
    base = np.concatenate([f32(base[:3] * base[3]), f32(base[3:])])   # the host premultiplies in f32
    layers = 0 if case.layer_alpha is None else 1
    want = bound = None
    state = np.zeros((H, W), np.int8)
    skip = np.zeros((H, W), bool)
    painted = np.zeros((H, W), bool)
    plain = store(np.broadcast_to(base, (H, W, 4)))
    for dr in case.draws:
        p = image_paint(dr, W, H, defect) if dr.kind == "image" else gradient_paint(dr, W, H, defect)
        area, area_err = case.area(dr)
        if p.cand.shape[2] == 1:
            p.cand = np.repeat(p.cand, N_CAND, axis=2)
        K = p.cand.shape[2]
        if want is None:
            want = np.repeat(plain[:, :, None, :], K, axis=2).copy()
            bound = np.repeat(store_bound(np.broadcast_to(base, (H, W, 4)), base)[:, :, None, :], K, axis=2).copy()
        assert K == want.shape[2], "draws of one case have the same number of candidates"
        on = area > 0
        a4 = area[:, :, None, None]
        if layers:
            src = over(0.0, p.cand, a4) * float(np.float32(case.layer_alpha))
            pm = base * (1.0 - src[..., 3:4]) + src
            fgs = p.cand * float(np.float32(case.layer_alpha))
        else:
            pm = over(base, p.cand, a4)
            fgs = p.cand
        b = store_bound(pm, base, (p.err * area[..., None])[:, :, None, :], area_err[:, :, None], fgs, layers)
        want[on], bound[on] = store(pm)[on], b[on]
        state[on], skip[on], painted[on] = p.state[on], p.skip[on], True
    return want, bound, state, skip, painted, plain


def check_image(case, img, defect=None):
    """img: (H, W, 4) float64 of the stored f16 values.  Returns a dict: bad (H, W) pixels out of bound, share: the
    largest error as a share of its bound over the checked pixels, left_out: share of the painted pixels that are
    left out as ill-conditioned or boundary."""
    want, bound, state, skip, painted, plain = expected(case, defect)
    H, W = case.height, case.width
    pb = _premul_base(case)
    plain_bound = store_bound(pb, pb[0, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio_k = (np.abs(img[:, :, None, :] - want) / bound).max(axis=-1)      # (H, W, K)
        ratio_paint = ratio_k.min(axis=-1)
        ratio_plain = (np.abs(img - plain) / plain_bound).max(axis=-1)
    ratio = np.where(state == 1, ratio_paint, np.where(state == 0, ratio_plain, np.minimum(ratio_paint, ratio_plain)))
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    checked = ~skip
    bad = checked & (ratio > 1.0)
    # left out: not checked at all (ill-conditioned), or on a boundary where painted and untouched are both allowed and
    # are not the same value anyway (an image has faded to nothing where it is cut)
    differ = (np.abs(want[:, :, 0, :] - plain) > bound[:, :, 0, :] + plain_bound).any(axis=-1)
    left_mask = painted & (state != 0) & (skip | ((state == 2) & differ))
    n_painted = max(int((painted & (state != 0)).sum()), 1)
    return {"bad": bad, "share": float(ratio[checked].max()) if checked.any() else 0.0, "left_out": int(left_mask.sum()) / n_painted,
            "ratio": ratio, "left_out_mask": left_mask}


def _premul_base(case):
    base = np.array(case.base, np.float64)
    base = np.concatenate([f32(base[:3] * base[3]), f32(base[3:])])
    return np.broadcast_to(base, (case.height, case.width, 4)).copy()
