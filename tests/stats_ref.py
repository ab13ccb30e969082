"""The stats rule (include/jello_hip.h "Stats") in numpy, written from the set definition: boolean masks over the
rectangle's texels, np.bincount for the bins, a signed integer order for the extremes.  It includes nothing of include/jello_stats.h;
the sRGB code is the encode rule of tests/surface_ref.py (binary64 pow), not the generated threshold table.

stats(bits, ...) -> the record as a numpy structured scalar (RECORD restates jh_stats_record); record_bytes(...) its bytes.  The
keywords after `rect` build the near misses tests/test_stats_spec.py tells the rule from."""
import numpy as np

import surface_ref

ALL, CONTENT = 0, 1
LINEAR, SRGB = 0, 1
BOUNDS, EXTREMES, HISTOGRAM = 1, 2, 4
EVERYTHING = 7
MAX_TEXELS = 1 << 31
SUBNORMAL = 2.0 ** -24  # the smallest positive f16

RECORD = np.dtype([("x", "<u4"), ("y", "<u4"), ("width", "<u4"), ("height", "<u4"), ("what", "<u4"), ("population", "<u4"), ("transfer", "<u4"),
                   ("reserved", "<u4"), ("content_count", "<u4"), ("bounds", "<u4", (4,)), ("population_count", "<u4"), ("nan_count", "<u4", (4,)),
                   ("min_bits", "<u2", (4,)), ("max_bits", "<u2", (4,)), ("histogram", "<u4", (4, 256))])
assert RECORD.itemsize == 4184


def widen(bits):
    """f16 bit patterns as binary32 (exact)."""
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def is_nan(bits):
    return (np.asarray(bits, np.uint16) & 0x7FFF) > 0x7C00


def content_mask(bits, channel, threshold, ge=True):
    """Content: the chosen channel, widened, is >= threshold -- IEEE: a NaN is not, -0 >= +0 holds."""
    v = widen(bits[..., channel])
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        return v >= t if ge else v > t


def order(bits):
    """totalOrder on non-NaN f16 patterns as a signed integer: -Inf < ... < -0 (-1) < +0 (0) < ... < +Inf."""
    h = np.asarray(bits, np.uint16).astype(np.int64)
    return np.where(h & 0x8000, -(h & 0x7FFF) - 1, h)


def codes(bits, srgb, half_even=True):
    """The histogram code of f16 patterns: q = clamp01(v) (NaN -> 0, -0 -> +0, +Inf -> 1); LINEAR: round-half-even of 255 q (the
    binary32 product is exact for an f16); SRGB: rint(255 enc(q)) in binary64."""
    q = surface_ref.clamp01(widen(bits))
    if srgb:
        return surface_ref.srgb8(q).astype(np.int64)
    p = q * np.float32(255.0)
    return (np.rint(p) if half_even else np.floor(p)).astype(np.int64)


def resolve(rect, w, h):
    """The rectangle a descriptor names in a w x h image; ValueError for what the image refuses."""
    x, y, rw, rh = (0, 0, 0, 0) if rect is None else rect
    if rw == 0 and rh == 0:
        x, y, rw, rh = 0, 0, w, h
    elif rw == 0 or rh == 0:
        raise ValueError("jh_stats: the rectangle is empty in one dimension")
    if x + rw > w or y + rh > h:
        raise ValueError("jh_stats: the rectangle is not inside the image")
    if rw * rh > MAX_TEXELS:
        raise ValueError("jh_stats: the rectangle has more than 2^31 texels")
    return x, y, rw, rh


def check(what, channel, threshold, population, transfer):
    if what == 0 or what & ~EVERYTHING:
        raise ValueError("jh_stats: what")
    if channel not in (0, 1, 2, 3) or population not in (ALL, CONTENT) or transfer not in (LINEAR, SRGB):
        raise ValueError("jh_stats: unknown channel, population or transfer")
    if not np.isfinite(np.float32(threshold)):
        raise ValueError("jh_stats: threshold is not finite")


def stats(bits, what=EVERYTHING, channel=3, threshold=SUBNORMAL, population=ALL, transfer=LINEAR, rect=None, ge=True, half_even=True,
          nan_in_histogram=True, nan_in_extremes=False, zero_order=True, exclusive=True, image_coordinates=True, use_population=True,
          alpha_linear=True, inside_only=True):
    """The record of the rectangle `rect` of the (H, W, 4) uint16 image `bits`."""
    with np.errstate(over="ignore"):
        check(what, channel, threshold, population, transfer)
    bits = np.asarray(bits, np.uint16)
    H, W = bits.shape[:2]
    x, y, rw, rh = resolve(rect, W, H)
    out = np.zeros((), RECORD)
    out["x"], out["y"], out["width"], out["height"] = x, y, rw, rh
    out["what"], out["population"], out["transfer"] = what, population, transfer
    if rw * rh == 0:
        return out  # an image without texels: the header and zeros
    if inside_only:
        X0, Y0, X1, Y1 = x, y, x + rw, y + rh
    else:  # (a near miss: the ring of texels around the rectangle counted too)
        X0, Y0, X1, Y1 = max(x - 1, 0), max(y - 1, 0), min(x + rw + 1, W), min(y + rh + 1, H)
    t = bits[Y0:Y1, X0:X1]
    content = content_mask(t, channel, threshold, ge)
    out["content_count"] = int(content.sum())
    if what & BOUNDS and content.any():
        at = np.argwhere(content)
        oy, ox = (Y0, X0) if image_coordinates else (Y0 - y, X0 - x)
        last = 1 if exclusive else 0
        out["bounds"] = [int(at[:, 1].min()) + ox, int(at[:, 0].min()) + oy, int(at[:, 1].max()) + ox + last, int(at[:, 0].max()) + oy + last]
    if not what & (EXTREMES | HISTOGRAM):
        return out
    pop = content if (population == CONTENT and use_population) else np.ones(content.shape, bool)
    out["population_count"] = int(pop.sum())
    for c in range(4):
        h = t[..., c][pop]
        nan = is_nan(h)
        out["nan_count"][c] = int(nan.sum())
        if what & EXTREMES:
            if nan_in_extremes and nan.any():  # (a near miss: a NaN wins the max, as it would under a float max)
                out["min_bits"][c], out["max_bits"][c] = (h[~nan][np.argmin(order(h[~nan]))] if (~nan).any() else 0x7C00), h[nan][0]
            elif (~nan).any():
                v = h[~nan]
                k = order(v)
                if not zero_order:  # (a near miss: +0 below -0)
                    k = np.where(k == -1, 0, np.where(k == 0, -1, k))
                out["min_bits"][c], out["max_bits"][c] = v[np.argmin(k)], v[np.argmax(k)]
            else:
                out["min_bits"][c], out["max_bits"][c] = 0x7C00, 0xFC00
        if what & HISTOGRAM:
            hh = h if nan_in_histogram else h[~nan]
            srgb = transfer == SRGB and (c != 3 or not alpha_linear)
            out["histogram"][c] = np.bincount(codes(hh, srgb, half_even), minlength=256)
    return out


def record_bytes(bits, **kw):
    return stats(bits, **kw).tobytes()
