"""The image calls' side of the Python glue: the enums and constants of include/jello_hip.h, the descriptor builders that
``Engine``'s methods pass to the C ABI, and the context-free queries (include/jello_queries.h) -- the taps, tables, plans, bounds,
weights and offsets that need no GPU, from the library (jh_<name>) or from its host twin (jl_<name>).
"""
import ctypes
import enum

import numpy as np

from . import _lib
from ._lib import CBlurDesc, CColorDesc, CCompositeDesc, CConvolveDesc, CDisplaceDesc, CDistanceDesc, CDistPlan, CLightingDesc, CLightPlan, CLoadSurfaceDesc, CLoadYuvDesc, CLut3dDesc, CMorphDesc, CPerspectiveDesc, CResampleDesc, CShadowDesc, CShadowPlan, CStatsDesc, CStatsPlan, CStatsRecord, CTurbPlan, CTurbulenceDesc, CWarpDesc


def _query(name, twin=False):
    """The query `name` of the library (jh_<name>), or of its host twin (jl_<name>)."""
    L = _lib.load_host()
    return getattr(L, "jl_" + name) if twin else getattr(L.hip, "jh_" + name)


class BlurEdge(enum.IntEnum):
    """jh_blur_edge: what a tap outside the image reads -- nothing (ZERO), or the nearest texel of the image (CLAMP)."""
    ZERO = 0
    CLAMP = 1


BLUR_MAX_SIGMA = 64.0


def blur_taps(sigma):
    """jh_blur_taps: (weights, R) of one axis of the blur rule -- the 2R + 1 float32 taps w[-R..R] of `sigma` and
    R = ceil(3 sigma).  No GPU needed.  ValueError for a sigma that is negative, above 64 or NaN."""
    f = _query("blur_taps")
    sigma = float(np.float32(sigma))
    r = ctypes.c_uint32(0)
    if f(sigma, None, ctypes.byref(r)) != 0:
        raise ValueError("blur_taps: sigma is negative, above 64 or NaN")
    w = np.empty(2 * r.value + 1, dtype=np.float32)
    f(sigma, w.ctypes.data, None)
    return w, r.value


def _rect(rect):  # (x, y, width, height) as a descriptor takes it: four ints, 0 x 0 -- the whole image -- for None
    x, y, w, h = (0, 0, 0, 0) if rect is None else rect
    return int(x), int(y), int(w), int(h)


def _blur_desc(sigma, edge, rect):
    sx, sy = sigma if isinstance(sigma, (tuple, list)) else (sigma, sigma)
    return CBlurDesc(float(sx), float(sy), int(edge), *_rect(rect))


COMPOSITE_TINT = 1  # JH_COMPOSITE_TINT


def _composite_desc(mix, compose, opacity, tint, src_rect, offset):
    d = CCompositeDesc(int(mix), int(compose), float(opacity), 0 if tint is None else COMPOSITE_TINT)
    if tint is not None:
        d.tint[:] = [float(v) for v in tint]
    d.sx, d.sy, d.sw, d.sh = _rect(src_rect)
    d.dx, d.dy = int(offset[0]), int(offset[1])
    return d


class ResampleFilter(enum.IntEnum):
    """jh_resample_filter: the kernel of jh_resample, by its support at 1:1 -- 0.5, 1, 2 and 3 texels."""
    BOX = 0
    TRIANGLE = 1
    CATMULL_ROM = 2
    LANCZOS3 = 3


RESAMPLE_STRAIGHT = 1  # JH_RESAMPLE_STRAIGHT
RESAMPLE_MAX_TAPS = 96  # JH_RESAMPLE_MAX_TAPS


def resample_taps(filter, n_in, n_out):
    """jh_resample_taps for every output index of one axis of the resample rule, n_in source texels onto n_out: a
    list of (first, weights) -- the window's first source index and its float32 taps.  No GPU needed.  ValueError for an unknown
    filter or sizes outside 1 <= n_in <= 16 n_out."""
    f = _query("resample_taps")
    out = []
    w = np.empty(RESAMPLE_MAX_TAPS, dtype=np.float32)
    first, count = ctypes.c_uint32(0), ctypes.c_uint32(0)
    for i in range(max(int(n_out), 1)):
        if f(int(filter), int(n_in), int(n_out), i, w.ctypes.data, ctypes.byref(first), ctypes.byref(count)) != 0:
            raise ValueError("resample_taps: unknown filter, or sizes outside 1 <= n_in <= 16 n_out")
        out.append((first.value, w[:count.value].copy()))
    return out


def _resample_desc(filter, src_rect, dst_rect, premultiplied):
    return CResampleDesc(int(filter), 0 if premultiplied else RESAMPLE_STRAIGHT, *_rect(src_rect), *_rect(dst_rect))


class MorphOp(enum.IntEnum):
    """jh_morph_op: the least (ERODE) or the greatest (DILATE) operand of the window."""
    ERODE = 0
    DILATE = 1


class MorphEdge(enum.IntEnum):
    """jh_morph_edge: a position outside the image takes part as transparent black (ZERO) or not at all (CLAMP)."""
    ZERO = 0
    CLAMP = 1


MORPH_STRAIGHT = 1  # JH_MORPH_STRAIGHT
MORPH_MAX_RADIUS = 255  # JH_MORPH_MAX_RADIUS


def _morph_desc(op, radius, edge, rect, premultiplied):
    rx, ry = radius if isinstance(radius, (tuple, list)) else (radius, radius)
    if not (0 <= int(rx) <= MORPH_MAX_RADIUS and 0 <= int(ry) <= MORPH_MAX_RADIUS):
        raise ValueError("jh_morphology: a radius above 255 or below 0")
    return CMorphDesc(int(op), int(edge), 0 if premultiplied else MORPH_STRAIGHT, int(rx), int(ry), *_rect(rect))


class WarpFilter(enum.IntEnum):
    """jh_warp_filter: the taps of jh_warp -- 1, 2 x 2 and 4 x 4 (Catmull-Rom) source texels."""
    NEAREST = 0
    BILINEAR = 1
    BICUBIC = 2


class WarpEdge(enum.IntEnum):
    """jh_warp_edge: what a tap outside the source rectangle reads -- transparent black, the nearest texel, the rectangle tiled, the
    rectangle tiled with every other copy flipped."""
    ZERO = 0
    CLAMP = 1
    REPEAT = 2
    MIRROR = 3


WARP_STRAIGHT = 1  # JH_WARP_STRAIGHT
WARP_MAX_SIDE = 32768  # JH_WARP_MAX_SIDE


def _matrix6(matrix):
    m = [float(v) for v in matrix]
    if len(m) != 6:
        raise ValueError("jh_warp: the matrix has 6 entries (a, b, c, d, e, f)")
    return (ctypes.c_double * 6)(*m)


def warp_plan(matrix, twin=False):
    """jh_warp_plan (twin: jl_warp_plan, the host twin): the six integers (P, Q, R, S, T, W) of the warp rule for
    `matrix` = (a, b, c, d, e, f), source rectangle -> destination image.  No GPU needed.  ValueError for an illegal matrix."""
    plan = (ctypes.c_int64 * 6)()
    if _query("warp_plan", twin)(_matrix6(matrix), plan) != 0:
        raise ValueError("jh_warp: illegal matrix (an entry not finite, a determinant that is 0 or not finite, an inverse coefficient "
                         "above 64 or an inverse offset above 2^22)")
    return tuple(int(v) for v in plan)


def warp_bounds(matrix, src_size, filter, dst_size, twin=False):
    """jh_warp_bounds (twin: jl_warp_bounds): the rectangle (x, y, width, height) of a destination of `dst_size` = (width, height)
    outside which a warp of a source rectangle of `src_size` under WarpEdge.ZERO is transparent black; (0, 0, 0, 0) when nothing is
    left.  No GPU needed.  ValueError for an illegal matrix, an unknown filter or a side above 32768."""
    rect = (ctypes.c_uint32 * 4)()
    if _query("warp_bounds", twin)(_matrix6(matrix), int(src_size[0]), int(src_size[1]), int(filter), int(dst_size[0]), int(dst_size[1]), rect) != 0:
        raise ValueError("jh_warp: illegal matrix, unknown filter or a side above 32768")
    return tuple(int(v) for v in rect)


def _warp_family_desc(ctype, matrix, straight, filter, edge, src_rect, dst_rect, premultiplied):
    """What jh_warp_desc, jh_displace_desc and jh_perspective_desc share: the matrix (in the descriptor's layout), filter, edge, the
    call's `straight` flag and the two rectangles."""
    d = ctype()
    d.matrix[:] = list(matrix)
    d.filter, d.edge, d.flags = int(filter), int(edge), 0 if premultiplied else straight
    d.src_x, d.src_y, d.src_width, d.src_height = _rect(src_rect)
    d.dst_x, d.dst_y, d.dst_width, d.dst_height = _rect(dst_rect)
    return d


def _warp_desc(matrix, filter, edge, src_rect, dst_rect, premultiplied):
    return _warp_family_desc(CWarpDesc, _matrix6(matrix), WARP_STRAIGHT, filter, edge, src_rect, dst_rect, premultiplied)


class ConvolveEdge(enum.IntEnum):
    """jh_convolve_edge: what a tap outside the image reads -- feConvolveMatrix's edgeMode none, duplicate and wrap,
    and the image mirrored; WarpEdge's values."""
    ZERO = 0
    CLAMP = 1
    REPEAT = 2
    MIRROR = 3


class ConvolveMode(enum.IntEnum):
    """jh_convolve_mode: the operand of jh_convolve -- colour times alpha (what feConvolveMatrix is defined on), the four channels as
    stored, or the colour channels as stored with the source's alpha copied (preserveAlpha)."""
    PREMULTIPLIED = 0
    STRAIGHT = 1
    PRESERVE_ALPHA = 2


CONVOLVE_MAX_ORDER = 15  # JH_CONVOLVE_MAX_ORDER
CONVOLVE_MAX_TAPS = 225  # JH_CONVOLVE_MAX_TAPS


def _order2(order, what="order"):
    ox, oy = order if isinstance(order, (tuple, list)) else (order, order)
    if int(ox) != ox or int(oy) != oy or int(ox) < 0 or int(oy) < 0:
        raise ValueError("jh_convolve: the %s is a non-negative integer or a pair of them" % what)
    return int(ox), int(oy)


def convolve_weights(order, kernel_matrix, divisor=0.0, twin=False):
    """jh_convolve_weights (twin: jl_convolve_weights, the host twin): the float32 weights (order_y, order_x) jh_convolve applies for
    feConvolveMatrix's `kernel_matrix` (order_x * order_y values, row-major) and `divisor` (0: the sum of the matrix, or 1 if that is
    0) -- flipped by 180 degrees and divided.  `order` is a scalar or (order_x, order_y).  No GPU needed.  ValueError
    for an order outside 1..15, a non-finite input or a weight that does not come out finite."""
    ox, oy = _order2(order)
    km = [float(v) for v in np.asarray(kernel_matrix, np.float64).ravel()]
    if not (1 <= ox <= CONVOLVE_MAX_ORDER and 1 <= oy <= CONVOLVE_MAX_ORDER) or len(km) != ox * oy:
        raise ValueError("jh_convolve: an order outside 1..15, or a kernelMatrix that does not have order_x * order_y entries")
    w = (ctypes.c_float * (ox * oy))()
    if _query("convolve_weights", twin)(ox, oy, (ctypes.c_double * len(km))(*km), float(divisor), w) != 0:
        raise ValueError("jh_convolve: illegal kernelMatrix or divisor (an entry not finite, or a weight that does not come out finite)")
    return np.array(w, np.float32).reshape(oy, ox)


def _convolve_desc(weights, order, target, edge, mode, bias, rect):
    w = np.asarray(weights, np.float32)
    if order is None:
        if w.ndim != 2:
            raise ValueError("jh_convolve: weights without an order are a two-dimensional array (order_y, order_x)")
        order = (w.shape[1], w.shape[0])
    ox, oy = _order2(order)
    w = w.ravel()
    if not (1 <= ox <= CONVOLVE_MAX_ORDER and 1 <= oy <= CONVOLVE_MAX_ORDER):
        raise ValueError("jh_convolve: an order outside 1..15")
    if w.size != ox * oy:
        raise ValueError("jh_convolve: %d weights for an order of %d x %d" % (w.size, ox, oy))
    tx, ty = (ox // 2, oy // 2) if target is None else _order2(target, "target")
    d = CConvolveDesc(ox, oy, tx, ty, int(edge), int(mode), float(bias), *_rect(rect))
    d.weights[:ox * oy] = [float(v) for v in w]
    return d


class LightKind(enum.IntEnum):
    """jh_lighting_kind: feDiffuseLighting or feSpecularLighting."""
    DIFFUSE = 0
    SPECULAR = 1


class LightSource(enum.IntEnum):
    """jh_light_source: feDistantLight, fePointLight, feSpotLight."""
    DISTANT = 0
    POINT = 1
    SPOT = 2


LIGHTING_TABLE_ENTRIES = 4097  # JH_LIGHTING_TABLE_ENTRIES
LIGHTING_TABLE_SPEC, LIGHTING_TABLE_SPOT = 1, 2  # jh_lighting_tables' `which`


def _vec3(v, what):
    v = tuple(float(c) for c in v)
    if len(v) != 3:
        raise ValueError("jh_lighting: %s has three components" % what)
    return v


def _lighting_desc(kind=LightKind.DIFFUSE, light=LightSource.DISTANT, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0),
                   direction=(0.0, 0.0, 1.0), position=(0.0, 0.0, 0.0), points_at=(0.0, 0.0, 0.0), spot_exponent=1.0, cone_cos=-1.0, rect=None):
    """jh_lighting_desc.  What the rule refuses is left for the call to refuse."""
    d = CLightingDesc()
    d.kind, d.light = int(kind), int(light)
    d.surface_scale, d.constant, d.specular_exponent, d.spot_exponent = float(surface_scale), float(constant), float(specular_exponent), float(spot_exponent)
    d.color[:] = _vec3(color, "color")
    d.x, d.y, d.width, d.height = _rect(rect)
    d.direction[:] = _vec3(direction, "direction")
    d.position[:] = _vec3(position, "position")
    d.points_at[:] = _vec3(points_at, "points_at")
    d.cone_cos = float(cone_cos)
    return d


def lighting_plan(twin=False, **keywords):
    """jh_lighting_plan (twin: jl_lighting_plan, the host twin): the plan of the lighting rule for the keywords of
    Engine.lighting -- dict(s=float32 (2, 3) indexed [span - 1][wsum - 2], ldir, p, sdir = float32 (3,), cone = float32).  No GPU needed.
    ValueError for a descriptor the rule refuses."""
    d, plan = _lighting_desc(**keywords), CLightPlan()
    if _query("lighting_plan", twin)(ctypes.byref(d), ctypes.byref(plan)) != 0:
        raise ValueError("jh_lighting: illegal descriptor")
    return dict(s=np.array(plan.s, np.float32).reshape(2, 3), ldir=np.array(plan.ldir, np.float32), p=np.array(plan.p, np.float32),
                sdir=np.array(plan.sdir, np.float32), cone=np.float32(plan.cone))


def lighting_tables(twin=False, **keywords):
    """jh_lighting_tables (twin: jl_lighting_tables): (spec, spot, which) -- the power tables the keywords of Engine.lighting need, float32
    [4097] each or None where the exponent is 1 or is not in use, and the bit mask.  No GPU needed.  ValueError as lighting_plan."""
    d = _lighting_desc(**keywords)
    spec, spot = np.zeros(LIGHTING_TABLE_ENTRIES, np.float32), np.zeros(LIGHTING_TABLE_ENTRIES, np.float32)
    which = ctypes.c_uint32(0)
    if _query("lighting_tables", twin)(ctypes.byref(d), spec.ctypes.data, spot.ctypes.data, ctypes.byref(which)) != 0:
        raise ValueError("jh_lighting: illegal descriptor")
    w = which.value
    return (spec if w & LIGHTING_TABLE_SPEC else None, spot if w & LIGHTING_TABLE_SPOT else None, w)


class TurbulenceKind(enum.IntEnum):
    """jh_turbulence_kind: feTurbulence's type."""
    FRACTAL_NOISE = 0
    TURBULENCE = 1


TURBULENCE_MAX_OCTAVES = 16  # JH_TURBULENCE_MAX_OCTAVES


def _pair(v, what):
    v = (v, v) if isinstance(v, (int, float)) else tuple(v)
    if len(v) != 2:
        raise ValueError("jh_turbulence: %s has two components" % what)
    return float(v[0]), float(v[1])


def _turbulence_desc(base_frequency=0.0, octaves=1, seed=0, kind=TurbulenceKind.TURBULENCE, stitch_tile=None, origin=(0.0, 0.0), rect=None):
    """jh_turbulence_desc.  What the rule refuses is left for the call to refuse."""
    d = CTurbulenceDesc()
    d.kind, d.octaves, d.seed, d.stitch = int(kind), int(octaves), int(seed), 0 if stitch_tile is None else 1
    d.x, d.y, d.width, d.height = _rect(rect)
    d.base_frequency[:] = _pair(base_frequency, "base_frequency")
    if stitch_tile is not None:
        tile = tuple(float(c) for c in stitch_tile)
        if len(tile) != 4:
            raise ValueError("jh_turbulence: stitch_tile has four components (x, y, width, height)")
        d.tile[:] = tile
    d.origin[:] = _pair(origin, "origin")
    return d


def turbulence_plan(twin=False, **keywords):
    """jh_turbulence_plan (twin: jl_turbulence_plan, the host twin): the plan of the turbulence rule for the keywords of
    Engine.turbulence -- dict(frequency=float64 (2,), step, start = int64 (2,), wrap, width = int32 (2,), max_extent = uint32 (2,), key,
    stitched).  No GPU needed.  ValueError for a descriptor the rule refuses."""
    d, plan = _turbulence_desc(**keywords), CTurbPlan()
    if _query("turbulence_plan", twin)(ctypes.byref(d), ctypes.byref(plan)) != 0:
        raise ValueError("jh_turbulence: illegal descriptor")
    return dict(frequency=np.array(plan.frequency, np.float64), step=np.array(plan.step, np.int64), start=np.array(plan.start, np.int64),
                wrap=np.array(plan.wrap, np.int32), width=np.array(plan.width, np.int32), max_extent=np.array(plan.max_extent, np.uint32),
                key=int(plan.key), stitched=int(plan.stitched))


def turbulence_tables(twin=False, **keywords):
    """jh_turbulence_tables (twin: jl_turbulence_tables): (selector, gradients) -- P, uint8 [256], and G, float32 [4][256][2], of the seed
    among the keywords of Engine.turbulence.  No GPU needed.  ValueError as turbulence_plan."""
    d = _turbulence_desc(**keywords)
    selector, gradients = np.zeros(256, np.uint8), np.zeros((4, 256, 2), np.float32)
    if _query("turbulence_tables", twin)(ctypes.byref(d), selector.ctypes.data, gradients.ctypes.data) != 0:
        raise ValueError("jh_turbulence: illegal descriptor")
    return selector, gradients


class DisplaceChannel(enum.IntEnum):
    """jh_displace_channel: the channel of the map that moves an axis -- feDisplacementMap's xChannelSelector and
    yChannelSelector."""
    R = 0
    G = 1
    B = 2
    A = 3


DISPLACE_STRAIGHT = 1  # JH_DISPLACE_STRAIGHT
AFFINE_IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)  # (a, b, c, d, e, f)


def displace_offset(scale, bits, twin=False):
    """jh_displace_offset (twin: jl_displace_offset, the host twin): D, the displacement in units of 2^-32 texel that the map value
    with the f16 bit pattern `bits` gives under the binary32 `scale`, by the rule of DESIGN.md 5.17: rint(clamp(scale (m - 0.5)) 2^32), a
    NaN product counting as 0.  No GPU needed."""
    out = ctypes.c_int64(0)
    if _query("displace_offset", twin)(float(np.float32(scale)), int(bits) & 0xFFFF, ctypes.byref(out)) != 0:
        raise ValueError("jh_displace: null argument")
    return int(out.value)


def _displace_desc(scale, x_channel, y_channel, matrix, filter, edge, src_rect, dst_rect, premultiplied):
    d = _warp_family_desc(CDisplaceDesc, _matrix6(matrix), DISPLACE_STRAIGHT, filter, edge, src_rect, dst_rect, premultiplied)
    sx, sy = scale if isinstance(scale, (tuple, list)) else (scale, scale)
    d.scale_x, d.scale_y = float(np.float32(sx)), float(np.float32(sy))
    d.x_channel, d.y_channel = int(x_channel), int(y_channel)
    return d


class ShadowFlags(enum.IntFlag):
    """jh_shadow's flags: OVER lays the shadow over what dst holds (Normal + SrcOver, in place), INVERT takes the
    coverage 1 - S -- the raw material of CSS inset shadows."""
    NONE = 0
    OVER = 1
    INVERT = 2


SHADOW_MAX_EXTENT = 1 << 23  # JSHADOW_MAX_EXTENT


def _shadow_desc(box, radius, sigma, color, matrix=None, rect=None, over=False, invert=False):
    """jh_shadow_desc.  What the rule refuses is left for the call to refuse."""
    d = CShadowDesc()
    d.matrix[:] = list(_matrix6(AFFINE_IDENTITY if matrix is None else matrix))
    d.x, d.y, d.width, d.height = _rect(rect)
    d.flags = int((ShadowFlags.OVER if over else 0) | (ShadowFlags.INVERT if invert else 0))
    d.radius, d.sigma = float(np.float32(radius)), float(np.float32(sigma))
    box, color = [float(np.float32(v)) for v in box], [float(np.float32(v)) for v in color]
    if len(box) != 4 or len(color) != 4:
        raise ValueError("jh_shadow: the box has four entries (x0, y0, x1, y1) and the color four (r, g, b, a, premultiplied)")
    d.box[:], d.color[:] = box, color
    return d


def shadow_plan(box, radius, sigma, matrix=None, twin=False):
    """jh_shadow_plan (twin: jl_shadow_plan, the host twin): the plan of the shadow rule -- dict(m = the six integers of
    the matrix, centre = int64 (2,), a, b, radius (clamped to the smaller half side), core, straight, sigma (floored at 2^-8), inv_s =
    1 / (sigma sqrt 2), window = K sigma as float32, n, k).  No GPU needed.  ValueError for a descriptor the rule refuses."""
    with np.errstate(over="ignore"):
        d, plan = _shadow_desc(box, radius, sigma, (0.0, 0.0, 0.0, 1.0), matrix), CShadowPlan()
    if _query("shadow_plan", twin)(ctypes.byref(d), ctypes.byref(plan)) != 0:
        raise ValueError("jh_shadow: illegal descriptor")
    out = dict(m=tuple(int(v) for v in plan.m), centre=np.array(plan.centre, np.int64), n=int(plan.n), k=int(plan.k))
    out.update({name: np.float32(getattr(plan, name)) for name in ("a", "b", "radius", "core", "straight", "sigma", "inv_s", "window")})
    return out


def shadow_bounds(box, radius, sigma, dst_size, matrix=None, twin=False):
    """jh_shadow_bounds (twin: jl_shadow_bounds): the rectangle (x, y, width, height) of a destination of `dst_size` = (width, height)
    outside which the shadow's coverage S is below 2^-12; (0, 0, 0, 0) when nothing is left.  It is what `rect` of Engine.shadow is
    restricted to: a 300 x 200 card in a 4096^2 frame costs a launch over the card's shadow, not over the frame.  No GPU needed.
    ValueError for a descriptor the rule refuses or a side above 2^23."""
    with np.errstate(over="ignore"):
        d = _shadow_desc(box, radius, sigma, (0.0, 0.0, 0.0, 1.0), matrix)
    rect = (ctypes.c_uint32 * 4)()
    if not (0 <= int(dst_size[0]) < 1 << 32 and 0 <= int(dst_size[1]) < 1 << 32) or \
            _query("shadow_bounds", twin)(ctypes.byref(d), int(dst_size[0]), int(dst_size[1]), rect) != 0:
        raise ValueError("jh_shadow: illegal descriptor or an image extent above 2^23")
    return tuple(int(v) for v in rect)


def box_shadow_geometry(box, radius, offset, spread):
    """CSS box-shadow's arithmetic on a border box (x0, y0, x1, y1) with corner radius `radius`: the offset shifts the box, the
    spread grows it on every side (a negative one shrinks it, to nothing at most: the sides meet at the middle) and grows the radius
    where there is one (a sharp corner stays sharp; never below 0).  Returns (box, radius) of the shape that is blurred."""
    x0, y0, x1, y1 = (float(v) for v in box)
    ox, oy = (float(v) for v in offset)
    s, r = float(spread), float(radius)
    x0, y0, x1, y1 = x0 + ox - s, y0 + oy - s, x1 + ox + s, y1 + oy + s
    if x1 < x0:
        x0 = x1 = 0.5 * (x0 + x1)
    if y1 < y0:
        y0 = y1 = 0.5 * (y0 + y1)
    return (x0, y0, x1, y1), (max(r + s, 0.0) if r > 0.0 else 0.0)


PERSPECTIVE_STRAIGHT = 1  # JH_PERSPECTIVE_STRAIGHT
PROJECTIVE_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)  # (a, b, p, c, d, q, e, f, s)


def _matrix9(matrix):
    m = [float(v) for v in matrix]
    if len(m) != 9:
        raise ValueError("jh_perspective: the matrix has 9 entries (a, b, p, c, d, q, e, f, s)")
    return (ctypes.c_double * 9)(*m)


def perspective_plan(matrix, twin=False):
    """jh_perspective_plan (twin: jl_perspective_plan, the host twin): the nine doubles G of the perspective rule for
    `matrix` = (a, b, p, c, d, q, e, f, s), source rectangle -> destination image: the adjugate scaled by a power of two so that
    every |G| <= 1, negated when the determinant is negative.  No GPU needed.  ValueError for an illegal matrix."""
    plan = (ctypes.c_double * 9)()
    if _query("perspective_plan", twin)(_matrix9(matrix), plan) != 0:
        raise ValueError("jh_perspective: illegal matrix (an entry or an adjugate entry not finite, a determinant that is 0 or not finite)")
    return tuple(float(v) for v in plan)


def perspective_bounds(matrix, src_size, filter, dst_size, twin=False):
    """jh_perspective_bounds (twin: jl_perspective_bounds): the rectangle (x, y, width, height) of a destination of `dst_size` =
    (width, height) outside which jh_perspective of a source rectangle of `src_size` under WarpEdge.ZERO is transparent black -- the
    whole destination when the rectangle reaches w <= 0; (0, 0, 0, 0) when nothing is left.  No GPU needed.  ValueError for an illegal
    matrix, an unknown filter or a side above 32768."""
    rect = (ctypes.c_uint32 * 4)()
    if _query("perspective_bounds", twin)(_matrix9(matrix), int(src_size[0]), int(src_size[1]), int(filter), int(dst_size[0]), int(dst_size[1]), rect) != 0:
        raise ValueError("jh_perspective: illegal matrix, unknown filter or a side above 32768")
    return tuple(int(v) for v in rect)


def _perspective_desc(matrix, filter, edge, src_rect, dst_rect, premultiplied):
    return _warp_family_desc(CPerspectiveDesc, _matrix9(matrix), PERSPECTIVE_STRAIGHT, filter, edge, src_rect, dst_rect, premultiplied)


class DistanceWhich(enum.IntEnum):
    """jh_distance_which: the distance to the nearest seed (OUTER), to the nearest non-seed (INNER), or the signed distance to the
    texel edge between the two classes, negative inside (SIGNED) -- DESIGN.md 5.20."""
    OUTER = 0
    INNER = 1
    SIGNED = 2


class DistanceEdge(enum.IntEnum):
    """jh_distance_edge: every position outside the image is a non-seed (ZERO: an inner distance ends at the image's border), or no
    position outside the image exists (CLAMP)."""
    ZERO = 0
    CLAMP = 1


class DistanceFlags(enum.IntFlag):
    """jh_distance's flags: STRAIGHT stores f16(color v) as it is -- data images, masks, SDF textures -- instead of by the store rule."""
    NONE = 0
    STRAIGHT = 1


DISTANCE_MAX_RADIUS = 255  # JH_DISTANCE_MAX_RADIUS


def _distance_desc(channel=3, threshold=0.5, which=DistanceWhich.OUTER, edge=DistanceEdge.ZERO, max_distance=1, scale=1.0, offset=0.0,
                   color=(1.0, 1.0, 1.0, 1.0), rect=None, straight=False):
    """jh_distance_desc.  What the rule refuses is left for the call to refuse, except a max_distance that does not fit the field."""
    if int(max_distance) != max_distance or not 0 <= int(max_distance) < 1 << 32:
        raise ValueError("jh_distance: max_distance is an integer in [1, 255]")
    with np.errstate(over="ignore"):
        color = [float(np.float32(v)) for v in color]
        if len(color) != 4:
            raise ValueError("jh_distance: the color has four entries (r, g, b, a, premultiplied)")
        d = CDistanceDesc(int(channel), float(np.float32(threshold)), int(which), int(edge), int(max_distance), float(np.float32(scale)),
                          float(np.float32(offset)))
    d.color[:] = color
    d.flags = int(DistanceFlags.STRAIGHT if straight else DistanceFlags.NONE)
    d.x, d.y, d.width, d.height = _rect(rect)
    return d


def distance_plan(image_size, twin=False, **keywords):
    """jh_distance_plan (twin: jl_distance_plan, the host twin): what Engine.distance with these keywords does on an image of
    `image_size` = (width, height) -- dict(rect = the resolved (x, y, width, height), radius, cap = (radius + 1)^2, planes,
    plane_columns, plane_rows, scratch_bytes).  It says which eager call has to precede a capture: one whose scratch_bytes are no
    less.  No GPU needed.  ValueError for a descriptor the rule refuses or a rectangle the image refuses."""
    d, plan = _distance_desc(**keywords), CDistPlan()
    if not (0 <= int(image_size[0]) < 1 << 32 and 0 <= int(image_size[1]) < 1 << 32) or \
            _query("distance_plan", twin)(ctypes.byref(d), int(image_size[0]), int(image_size[1]), ctypes.byref(plan)) != 0:
        raise ValueError("jh_distance: illegal descriptor or rectangle")
    return dict(rect=(plan.x, plan.y, plan.width, plan.height), radius=plan.radius, cap=plan.cap, planes=plan.planes,
                plane_columns=plan.plane_columns, plane_rows=plan.plane_rows, scratch_bytes=int(plan.scratch_bytes))


class StatsWhat(enum.IntFlag):
    """The parts of jh_stats's record (JH_STATS_BOUNDS | JH_STATS_EXTREMES | JH_STATS_HISTOGRAM); a part not asked for is zeros."""
    BOUNDS = 1
    EXTREMES = 2
    HISTOGRAM = 4
    ALL = 7


class StatsPopulation(enum.IntEnum):
    """jh_stats_population: the texels the extremes and the histogram are taken over -- every texel of the rectangle (ALL) or the
    content texels only (CONTENT: a layer on a transparent background, whose bin 0 would otherwise hold the background)."""
    ALL = 0
    CONTENT = 1


class StatsTransfer(enum.IntEnum):
    """jh_stats_transfer: the histogram's code for R, G, B -- round-half-even of 255 clamp(v) (LINEAR) or jh_blit's sRGB code (SRGB);
    alpha is always LINEAR."""
    LINEAR = 0
    SRGB = 1


STATS_MAX_TEXELS = 1 << 31  # JH_STATS_MAX_TEXELS
STATS_MAX_PARTIALS = 1024  # JH_STATS_MAX_PARTIALS
STATS_RECORD_BYTES = ctypes.sizeof(CStatsRecord)


def _stats_desc(what=StatsWhat.ALL, channel=3, threshold=2.0 ** -24, population=StatsPopulation.ALL, transfer=StatsTransfer.LINEAR, rect=None):
    """jh_stats_desc.  What the rule refuses is left for the call to refuse, except a `what` that does not fit the field.  The default
    threshold is the smallest positive f16: content is what is not transparent."""
    if int(what) != what or not 0 <= int(what) < 1 << 32:
        raise ValueError("jh_stats: what is a subset of StatsWhat")
    with np.errstate(over="ignore"):
        d = CStatsDesc(int(what), int(channel), float(np.float32(threshold)), int(population), int(transfer))
    d.x, d.y, d.width, d.height = _rect(rect)
    return d


def stats_plan(image_size, twin=False, **keywords):
    """jh_stats_plan (twin: jl_stats_plan, the host twin): what Engine.stats with these keywords does on an image of `image_size` =
    (width, height) -- dict(rect = the resolved (x, y, width, height), launches, record_bytes, scratch_bytes).  The scratch is the
    same for every image with texels: one eager call makes every later one capturable.  No GPU needed.  ValueError for a descriptor
    the rule refuses or a rectangle the image refuses."""
    d, plan = _stats_desc(**keywords), CStatsPlan()
    if not (0 <= int(image_size[0]) < 1 << 32 and 0 <= int(image_size[1]) < 1 << 32) or \
            _query("stats_plan", twin)(ctypes.byref(d), int(image_size[0]), int(image_size[1]), ctypes.byref(plan)) != 0:
        raise ValueError("jh_stats: illegal descriptor or rectangle")
    return dict(rect=(plan.x, plan.y, plan.width, plan.height), launches=plan.launches, record_bytes=int(plan.record_bytes),
                scratch_bytes=int(plan.scratch_bytes))


def stats_codes(f16_bits, transfer=StatsTransfer.LINEAR, twin=False):
    """jh_stats_codes (twin: jl_stats_codes): the histogram code (uint8, the shape of the input) of every f16 bit pattern of `f16_bits`
    under `transfer`, as a colour channel's.  No GPU needed.  ValueError for an unknown transfer."""
    bits = np.ascontiguousarray(f16_bits, np.uint16)
    codes = np.empty(bits.shape, np.uint8)
    if _query("stats_codes", twin)(int(transfer), bits.size, bits.ctypes.data, codes.ctypes.data) != 0:
        raise ValueError("jh_stats: unknown transfer")
    return codes


class LoadAlpha(enum.IntEnum):
    """jh_load_alpha: what byte 3 of a loaded surface pixel is -- straight alpha beside straight colour, the alpha
    the colour has been multiplied by (what blit() writes), or nothing (BGRX: the texel is opaque)."""
    STRAIGHT = 0
    PREMULTIPLIED = 1
    OPAQUE = 2


class ChromaFilter(enum.IntEnum):
    """jh_chroma_filter: how load_yuv reads the half-resolution chroma planes -- the sample that covers the texel (REPLICATE, the
    adjoint of blit_yuv's box), or the 9 / 3 / 3 / 1 blend of the four nearest, centre-sited, the edge sample repeated (BILINEAR)."""
    REPLICATE = 0
    BILINEAR = 1


LOAD_TRANSFER = 4  # jh_load_texel's format_or_transfer: 4 + a YuvTransfer names RGBA codes under that transfer


def _load_surface_desc(fmt, alpha, src, pitch, rect):
    x, y, w, h = _rect(rect)
    return CLoadSurfaceDesc(int(fmt), int(alpha), src, int(pitch), x, y, w, h)


def _load_yuv_desc(layout, matrix, rng, transfer, chroma, planes, rect):
    """jh_load_yuv_desc; `planes` = [(device pointer, pitch)] per plane."""
    d = CLoadYuvDesc(int(layout), int(matrix), int(rng), int(transfer), int(chroma), 0)
    if len(planes) > 3:
        raise ValueError("jh_load_yuv: at most three planes")
    for i, (ptr, pitch) in enumerate(planes):
        d.plane[i], d.pitch[i] = ptr, int(pitch)
    d.x, d.y, d.width, d.height = _rect(rect)
    return d


def _frame_rect(rect, w, h, who):
    """The rectangle of a frame given as host arrays of w x h texels: `rect` where it has the frame's size, (0, 0, w, h) for None --
    never 0 x 0, which would name the whole image and let the call read more than was uploaded."""
    if rect is None:
        return (0, 0, w, h)
    if len(rect) != 4 or (int(rect[2]), int(rect[3])) != (w, h):
        raise ValueError("%s: the rectangle has the size of the frame" % who)
    return tuple(int(v) for v in rect)


def _surface_array_source(pixels, rect):
    """What Engine.load_surface uploads and describes for an (H, W, 4) uint8 array: (bytes uint8 [H * W * 4], pitch, rect), rect
    always of the array's size; None for an array without texels."""
    px = np.ascontiguousarray(pixels, np.uint8)
    if px.ndim != 3 or px.shape[2] != 4:
        raise ValueError("jh_load_surface: pixels is an (H, W, 4) uint8 array or a device pointer")
    h, w = px.shape[:2]
    rect = _frame_rect(rect, w, h, "jh_load_surface")
    return None if w * h == 0 else (px.reshape(-1), 4 * w, rect)


def yuv_plane_shapes(width, height, layout):
    """[(rows, bytes per row)] of the planes of a width x height frame (include/jello_frame.h): Y, then CbCr (NV12: layout 0) or Cb and Cr (I420)."""
    cw, ch = (width + 1) // 2, (height + 1) // 2
    return [(height, width), (ch, 2 * cw)] if int(layout) == 0 else [(height, width), (ch, cw), (ch, cw)]


def packed_plane_offsets(shapes):
    """(offsets, total bytes) of planes [(rows, bytes per row)] in a buffer of the engine's own: one after the other, tight rows, each start a multiple of 16."""
    sizes = [(rows * row_bytes + 15) & ~15 for rows, row_bytes in shapes]
    return [sum(sizes[:i]) for i in range(len(sizes))], sum(sizes)


def _yuv_array_source(planes, layout, rect):
    """What Engine.load_yuv uploads and describes for planes given as uint8 arrays: (bytes uint8, [(offset, pitch)] per plane, rect),
    the planes one after the other with tightly packed rows, each starting at a multiple of 16, rect always of the luma plane's size;
    None for a frame without texels."""
    if not all(isinstance(a, np.ndarray) for a in planes):
        raise ValueError("jh_load_yuv: the planes are all arrays or all (device pointer, pitch)")
    arrays = [np.ascontiguousarray(a, np.uint8) for a in planes]
    if not arrays or arrays[0].ndim != 2 or any(a.ndim not in (2, 3) for a in arrays) or int(layout) not in (0, 1):
        raise ValueError("jh_load_yuv: the planes are two-dimensional uint8 arrays (NV12's chroma may be (rows, samples, 2)) of layout NV12 or I420")
    h, w = arrays[0].shape
    shapes = yuv_plane_shapes(w, h, layout)
    if w * h and [a.reshape(a.shape[0], -1).shape for a in arrays] != shapes:
        raise ValueError("jh_load_yuv: the planes do not have the shapes of a frame of the luma plane's size in this layout")
    rect = _frame_rect(rect, w, h, "jh_load_yuv")
    if w * h == 0:
        return None
    offs, total = packed_plane_offsets(shapes)
    host = np.zeros(total, np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + a.size] = a.reshape(-1)
    return host, [(o, b) for o, (_, b) in zip(offs, shapes)], rect


def load_texels(pixels, fmt=None, alpha=LoadAlpha.STRAIGHT, transfer=None, twin=False):
    """jh_load_texel (twin: jl_load_texel, the host twin): the RGBA16F texels of the load rule for `pixels`, a uint8
    array (..., 4) -- in the byte order of the Surface format `fmt`, or, with `transfer` (a YuvTransfer) in its place, RGBA codes
    under that transfer.  Returns the f16 bit patterns, uint16 of the same shape.  No GPU needed.  ValueError for an unknown
    format, transfer or alpha."""
    if (fmt is None) == (transfer is None):
        raise ValueError("jh_load_texel: one of fmt and transfer")
    if not 0 <= int(transfer if fmt is None else fmt) < (2 if fmt is None else LOAD_TRANSFER):
        raise ValueError("jh_load_texel: unknown surface format or transfer")
    px = np.ascontiguousarray(pixels, np.uint8)
    if px.ndim < 1 or px.shape[-1] != 4:
        raise ValueError("jh_load_texel: pixels of four bytes")
    out = np.zeros(px.shape, np.uint16)
    if _query("load_texel", twin)(int(fmt) if transfer is None else LOAD_TRANSFER + int(transfer), int(alpha), px.size // 4, px.ctypes.data, out.ctypes.data) != 0:
        raise ValueError("jh_load_texel: unknown surface format, transfer or alpha mode")
    return out


def load_yuv_codes(y, s_cb, s_cr, matrix, range, twin=False):
    """jh_load_yuv_codes (twin: jl_load_yuv_codes): the R'G'B' codes of the load rule for luma codes `y` and chroma sums `s_cb`,
    `s_cr` (16 x a code, 0 .. 4080), arrays of one shape, under a YuvMatrix and YuvRange: uint8 of shape (..., 3).  No GPU needed.
    ValueError for an unknown matrix or range or a sum above 4080."""
    yy, cb, cr = np.ascontiguousarray(y, np.uint8), np.ascontiguousarray(s_cb, np.uint16), np.ascontiguousarray(s_cr, np.uint16)
    if not (yy.shape == cb.shape == cr.shape):
        raise ValueError("jh_load_yuv_codes: y, s_cb and s_cr have one shape")
    out = np.zeros(yy.shape + (3,), np.uint8)
    if _query("load_yuv_codes", twin)(int(matrix), int(range), yy.size, yy.ctypes.data, cb.ctypes.data, cr.ctypes.data, out.ctypes.data) != 0:
        raise ValueError("jh_load_yuv_codes: unknown matrix or range, or a chroma sum above 4080")
    return out


class ColorSpace(enum.IntEnum):
    """jh_color_space: the values the matrix and the funcs of jh_color_filter act on -- the stored linear ones,
    or the colour channels sRGB-encoded (what the CSS filter functions are defined on); alpha is never encoded."""
    LINEAR = 0
    SRGB = 1


class ColorFunc(enum.IntEnum):
    """jh_color_func_type: feComponentTransfer's function types."""
    IDENTITY = 0
    LINEAR = 1
    GAMMA = 2
    TABLE = 3
    DISCRETE = 4


COLOR_CLAMP = 1  # JH_COLOR_CLAMP
COLOR_MAX_VALUES = 64  # JH_COLOR_MAX_VALUES
COLOR_POST_SHIFT = 4  # jh_color_tables' `which`: bit c is PRE_c, bit 4 + i is POST_i
IDENTITY_MATRIX = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _color_desc(matrix, funcs, space, clamp, rect):
    """jh_color_desc.  `funcs`: None or four entries, each None (IDENTITY) or (ColorFunc.LINEAR, slope, intercept),
    (ColorFunc.GAMMA, amplitude, exponent, offset), (ColorFunc.TABLE, values), (ColorFunc.DISCRETE, values) -- what
    colorfilter.linear / gamma / table / discrete return.  What the rule refuses is left for the call to refuse, except a value
    list that does not fit the struct."""
    d = CColorDesc()
    d.x, d.y, d.width, d.height = _rect(rect)
    m = np.asarray(IDENTITY_MATRIX if matrix is None else matrix, np.float32).reshape(-1)
    if m.size != 20:
        raise ValueError("color_filter: the matrix has 20 entries (row-major 4 x 5)")
    d.matrix[:] = [float(v) for v in m]
    d.space, d.flags = int(space), COLOR_CLAMP if clamp else 0
    funcs = (None,) * 4 if funcs is None else tuple(funcs)
    if len(funcs) != 4:
        raise ValueError("color_filter: four funcs, one per output channel")
    for i, f in enumerate(funcs):
        if f is None:
            continue
        c, kind = d.func[i], int(f[0])
        c.type = kind
        if kind == ColorFunc.LINEAR:
            c.slope, c.intercept = float(f[1]), float(f[2])
        elif kind == ColorFunc.GAMMA:
            c.amplitude, c.exponent, c.offset = float(f[1]), float(f[2]), float(f[3])
        elif kind in (ColorFunc.TABLE, ColorFunc.DISCRETE):
            values = [float(v) for v in f[1]]
            c.n = len(values)  # (0 and more than 64 are the call's to refuse; only 64 fit the struct)
            c.values[:min(len(values), COLOR_MAX_VALUES)] = values[:COLOR_MAX_VALUES]
    return d


def color_tables(funcs=None, space=ColorSpace.LINEAR, clamp=True, twin=False):
    """jh_color_tables (twin: jl_color_tables, the host twin): the tables of the colour-filter rule for these
    funcs, space and clamp setting, one entry per f16 bit pattern: (pre, post, which) -- pre a dict {channel: float32 [65536]},
    post a dict {channel: uint16 [65536]} of the tables that exist, which the bit mask.  No GPU needed.  ValueError for what the
    rule refuses."""
    d = _color_desc(None, funcs, space, clamp, None)
    pre, post = np.zeros((3, 65536), np.float32), np.zeros((4, 65536), np.uint16)
    which = ctypes.c_uint32(0)
    if _query("color_tables", twin)(ctypes.byref(d), pre.ctypes.data, post.ctypes.data, ctypes.byref(which)) != 0:
        raise ValueError("color_tables: unknown space or func type, n = 0 or n > 64 values, or a parameter that is not finite")
    w = which.value
    return ({c: pre[c] for c in range(3) if w >> c & 1}, {i: post[i] for i in range(4) if w >> (COLOR_POST_SHIFT + i) & 1}, w)


LUT3D_MIN_SIZE = 2  # JH_LUT3D_MIN_SIZE
LUT3D_MAX_SIZE = 65  # JH_LUT3D_MAX_SIZE


def _lut3d_desc(size, rect):
    """jh_lut3d_desc: the table's N and the rectangle; what the rule refuses is left for the call to refuse."""
    return CLut3dDesc(int(size), 0, *_rect(rect))


def lut3d_identity(n, twin=False):
    """jh_lut3d_identity (twin: jl_lut3d_identity, the host twin): the identity table of the LUT rule as the
    (n * n, n, 4) uint16 image of f16 bit patterns jh_lut3d takes -- entry (r, g, b) at [g + n * b, r], value f16(index / (n - 1)),
    alpha 1.0.  No GPU needed.  ValueError for an n outside 2..65."""
    n = int(n)
    if not LUT3D_MIN_SIZE <= n <= LUT3D_MAX_SIZE:
        raise ValueError("jh_lut3d_identity: size outside 2..65")
    out = np.empty((n * n, n, 4), np.uint16)
    if _query("lut3d_identity", twin)(n, out.ctypes.data) != 0:
        raise ValueError("jh_lut3d_identity: size outside 2..65")
    return out


def lut3d_texels(lut_image, texels, twin=False):
    """jh_lut3d_texels (twin: jl_lut3d_texels): the LUT rule on the host -- `texels`, (..., 4) uint16 f16 bit
    patterns, through the table `lut_image`, the (n * n, n, 4) uint16 image; returns the same shape.  No GPU needed.  ValueError for
    a table that is not (n * n, n, 4) with n in 2..65."""
    lut = np.ascontiguousarray(lut_image, np.uint16)
    n = lut.shape[1] if lut.ndim == 3 else 0
    if lut.ndim != 3 or lut.shape != (n * n, n, 4) or not LUT3D_MIN_SIZE <= n <= LUT3D_MAX_SIZE:
        raise ValueError("jh_lut3d_texels: the table is not an (n * n, n, 4) image with n in 2..65")
    t = np.ascontiguousarray(texels, np.uint16)
    if t.shape[-1:] != (4,):
        raise ValueError("jh_lut3d_texels: texels of four channels")
    out = np.empty_like(t)
    if _query("lut3d_texels", twin)(n, lut.ctypes.data, t.ctypes.data, t.size // 4, out.ctypes.data) != 0:
        raise ValueError("jh_lut3d_texels: size outside 2..65")
    return out


def composite_clip(src_size, dst_size, src_rect=None, offset=(0, 0)):
    """jl_composite_clip: where the rectangle `src_rect` = (sx, sy, sw, sh) (None: the whole image) of a source of `src_size` =
    (width, height) lands when its top-left is placed at the signed `offset` of a destination of `dst_size` and clipped to it
    (the geometry of DESIGN.md 5.8): (sx', sy', dx', dy', w, h), all zero when nothing is left.  No GPU needed.  ValueError for a
    source rectangle the rule refuses."""
    L = _lib.load_host()
    sx, sy, sw, sh = _rect(src_rect)
    out = (ctypes.c_uint32 * 6)()
    if L.jl_composite_clip(src_size[0], src_size[1], sx, sy, sw, sh, offset[0], offset[1], dst_size[0], dst_size[1], out) != 0:
        raise ValueError(L.jl_last_error().decode())
    return tuple(out)

