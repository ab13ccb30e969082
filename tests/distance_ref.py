"""The distance rule (include/jello_hip.h "Distance") in numpy, from the SET definition: all pairs of output texel x
feature in int64.  It includes nothing of include/jello_distance.h and makes no passes.

  seed       a texel whose channel, the f16 widened to binary32, is >= threshold (IEEE: a NaN is no seed, -0 >= +0 holds)
  D          CAP = (R + 1)^2; Dout = min(CAP, min over the seeds of dx^2 + dy^2), Din the same over the non-seeds; under EDGE_ZERO
             every position outside the image is a non-seed too -- the nearest of those is straight across the nearest border, at
             min(X + 1, Y + 1, w - X, h - Y), a closed form -- and under EDGE_CLAMP there is none.  The image is the edge.
  s          OUTER sqrtf(Dout); INNER sqrtf(Din); SIGNED sqrtf(Dout) - 0.5 on a non-seed, 0.5 - sqrtf(Din) on a seed; binary32
  v          minNum(maxNum(fmaf(s, scale, offset), 0), 1)
  store      p = color v; STRAIGHT f16(p); else a_inv = 1 / maxNum(p.a, 1e-6), f16(p.rgb a_inv + 0), f16(p.a + 0)

The keyword arguments of `distance` after `dst_bits` build the nine near misses the battery has to tell from the rule
(tests/test_distance_spec.py)."""
import numpy as np

import image_ref
from image_ref import fmaf32, fmax, fmin, same_bits  # noqa: F401

OUTER, INNER, SIGNED = 0, 1, 2
ZERO, CLAMP = 0, 1
STRAIGHT = 1
MAX_RADIUS = 255
F = np.float32


def seeds(src_bits, channel, threshold, ge=True, nan_seed=False):
    """(H, W) bool: which texels are seeds."""
    with np.errstate(invalid="ignore"):
        v = np.ascontiguousarray(src_bits, np.uint16)[..., channel].view(np.float16).astype(F)
        s = (v >= F(threshold)) if ge else (v > F(threshold))
        if nan_seed:
            s = s | np.isnan(v)
    return s


def squared(features, where, cap, window=None, chessboard=False):
    """(h, w) int64: min(cap, min over the positions set in `features` -- (H, W) bool -- of the squared distance) for the outputs of the
    rectangle `where` = (x, y, w, h), all pairs.  `window`: only features within that many columns and rows count; `chessboard`: the
    squared chessboard distance (near misses both)."""
    x, y, w, h = where
    fy, fx = np.nonzero(features)
    fx, fy = fx.astype(np.int64), fy.astype(np.int64)
    Y, X = np.mgrid[y:y + h, x:x + w]
    X, Y = X.reshape(-1).astype(np.int64), Y.reshape(-1).astype(np.int64)
    out = np.full(X.size, cap, np.int64)
    if fx.size:
        step = max(1, (1 << 22) // fx.size)
        for i in range(0, X.size, step):
            dx, dy = np.abs(fx[None, :] - X[i:i + step, None]), np.abs(fy[None, :] - Y[i:i + step, None])
            d = np.maximum(dx, dy) ** 2 if chessboard else dx * dx + dy * dy
            if window is not None:
                d = np.where((dx > window) | (dy > window), cap, d)
            out[i:i + step] = np.minimum(out[i:i + step], d.min(axis=1))
    return out.reshape(h, w)


def outside(extent, where, cap, window=None):
    """(h, w) int64: min(cap, the squared distance to the nearest integer position outside the rectangle `extent` = (x, y, w, h)) for
    the outputs of `where`, which lies inside it: the closed form."""
    ex, ey, ew, eh = extent
    x, y, w, h = where
    Y, X = np.mgrid[y:y + h, x:x + w].astype(np.int64)
    m = np.minimum(np.minimum(X - ex + 1, ex + ew - X), np.minimum(Y - ey + 1, ey + eh - Y))
    d = m * m
    if window is not None:
        d = np.where(m > window, cap, d)
    return np.minimum(d, cap)


def squared_distances(src_bits, channel, threshold, which, edge, R, rect=None, ge=True, nan_seed=False, cap_r2=False, open_window=False,
                      zero_outside=True, image_edge=True, chessboard=False):
    """(seed, Dout, Din): (h, w) bool and int64 over the resolved rectangle."""
    H, W = src_bits.shape[:2]
    where = image_ref.resolve(src_bits.shape, rect)
    x, y, w, h = where
    extent = (0, 0, W, H) if image_edge else where  # (a near miss: the rectangle as the edge)
    s = seeds(src_bits, channel, threshold, ge, nan_seed)
    inside = np.zeros((H, W), bool)
    inside[extent[1]:extent[1] + extent[3], extent[0]:extent[0] + extent[2]] = True
    cap = R * R if cap_r2 else (R + 1) * (R + 1)
    window = R - 1 if open_window else None
    none = np.zeros((H, W), bool)  # (the distance `which` does not look at is not computed: it comes out as the cap)
    d_out = squared(s & inside if which != INNER else none, where, cap, window, chessboard)
    d_in = squared(~s & inside if which != OUTER else none, where, cap, window, chessboard)
    if edge == ZERO and zero_outside and which != OUTER:
        d_in = np.minimum(d_in, outside(extent, where, cap, window))
    return s[y:y + h, x:x + w], d_out, d_in


def value(seed, d_out, d_in, which, scale, offset, half=True, s_f16=False):
    """(h, w) float32: v of the rule."""
    with np.errstate(all="ignore"):
        so, si = np.sqrt(d_out.astype(F)), np.sqrt(d_in.astype(F))  # (numpy's binary32 sqrt is the correctly rounded one)
        if which == OUTER:
            s = so
        elif which == INNER:
            s = si
        else:
            hf = F(0.5) if half else F(0.0)
            s = np.where(seed, hf - si, so - hf).astype(F)
        if s_f16:
            s = s.astype(np.float16).astype(F)
        return fmin(fmax(fmaf32(s, F(scale), F(offset)), F(0.0)), F(1.0))


def store(p, straight):
    """(..., 4) float32 -> uint16 f16 bit patterns, as the rule stores."""
    with np.errstate(all="ignore"):
        if not straight:
            zero = F(0.0)
            a_inv = (F(1.0) / fmax(p[..., 3], F(1e-6))).astype(F)
            p = np.concatenate([(p[..., :3] * a_inv[..., None]).astype(F) + zero, p[..., 3:] + zero], axis=-1)
        return p.astype(F).astype(np.float16).view(np.uint16)


def distance(src_bits, channel=3, threshold=0.5, which=OUTER, edge=ZERO, R=1, scale=1.0, offset=0.0, color=(1.0, 1.0, 1.0, 1.0), flags=0, rect=None,
             dst_bits=None, half=True, s_f16=False, **variant):
    """What dst holds after the call: (H, W, 4) uint16.  dst_bits: what it held before (None: never written, transparent black)."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    if channel not in (0, 1, 2, 3) or which not in (OUTER, INNER, SIGNED) or edge not in (ZERO, CLAMP) or flags & ~STRAIGHT or not 1 <= R <= MAX_RADIUS:
        raise ValueError("illegal descriptor")
    if not all(np.isfinite(F(v)) for v in (threshold, scale, offset)):
        raise ValueError("threshold, scale or offset is not finite")
    x, y, w, h = image_ref.resolve(src_bits.shape, rect)
    out = np.zeros_like(src_bits) if dst_bits is None else np.array(dst_bits, np.uint16)
    if w == 0 or h == 0:
        return out
    seed, d_out, d_in = squared_distances(src_bits, channel, threshold, which, edge, R, rect, **variant)
    v = value(seed, d_out, d_in, which, scale, offset, half, s_f16)
    with np.errstate(all="ignore"):
        p = (np.asarray(color, F)[None, None, :] * v[..., None]).astype(F)
    out[y:y + h, x:x + w] = store(p, bool(flags & STRAIGHT))
    return out
