"""The turbulence rule (include/jello_hip.h "Turbulence") restated in numpy: the generator and the tables in Python
integers and binary64, the plan in binary64 and Python integers, positions in int64, everything per texel in binary32 with the exact
fmaf the other references use.  It shares no code with include/jello_turbulence.h.

turbulence(shape, rect, dst_bits, **desc) is what jh_turbulence leaves in an image; the keywords after `desc` in its signature are the
NEAR MISSES tests/test_turbulence_spec.py measures the battery's sensitivity with -- each a plausible other reading of the
specification's code, none of them the rule."""
import math

import numpy as np

from image_ref import fmaf32, fmax, fmin, resolve, same_bits  # noqa: F401 (same_bits is part of this module's interface)

F = np.float32
FRACTAL_NOISE, TURBULENCE = 0, 1
KIND_NAMES = ("fractal", "turbulence")
MAX_OCTAVES = 16
M, A, Q, R = 2147483647, 16807, 127773, 2836
DEFAULTS = dict(base_frequency=(0.0, 0.0), octaves=1, seed=0, kind=TURBULENCE, stitch_tile=None, origin=(0.0, 0.0))


def _desc(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown keywords: %s" % sorted(unknown))
    d = dict(DEFAULTS, **kw)
    bf = d["base_frequency"]
    d["base_frequency"] = (float(bf), float(bf)) if isinstance(bf, (int, float)) else (float(bf[0]), float(bf[1]))
    d["origin"] = (float(d["origin"][0]), float(d["origin"][1]))
    return d


# ---- the generator and the tables ----

def setup_seed(seed):
    s = int(seed)
    if s <= 0:
        s = ((-s) % (M - 1)) + 1  # (-(s mod (m - 1)) + 1 with C's remainder, which has the sign of s)
    return min(s, M - 1)


def random(s):
    r = A * (s % Q) - R * (s // Q)
    return r + M if r <= 0 else r


def tables(seed):
    """(P, G, key): uint8 [256], float32 [4][256][2], the seed after setup_seed."""
    s = key = setup_seed(seed)
    G = np.zeros((4, 256, 2), F)
    for k in range(4):
        for i in range(256):
            s = random(s)
            x = ((s % 512) - 256) / 256.0
            s = random(s)
            y = ((s % 512) - 256) / 256.0
            length = math.sqrt(x * x + y * y)
            if length != 0.0:
                G[k, i] = (F(x / length), F(y / length))
    P = list(range(256))
    for i in range(255, 0, -1):
        s = random(s)
        j = s % 256
        P[i], P[j] = P[j], P[i]
    return np.array(P, np.uint8), G, key


# ---- the plan ----

def plan(no_half=False, **kw):
    """The plan as jello_amd.turbulence_plan gives it; ValueError for a descriptor the rule refuses."""
    d = _desc(kw)
    if int(d["kind"]) not in (FRACTAL_NOISE, TURBULENCE):
        raise ValueError("unknown kind")
    octaves = int(d["octaves"])
    if not 0 <= octaves <= MAX_OCTAVES:
        raise ValueError("octaves outside 0 .. 16")
    tile = d["stitch_tile"]
    if tile is not None:
        tile = tuple(float(c) for c in tile)
        if not all(math.isfinite(c) for c in tile) or not (tile[2] > 0.0 and tile[3] > 0.0):
            raise ValueError("the stitch tile")
    shift = max(octaves - 1, 0)
    L = ((1 << 62) - 1) >> shift
    out = dict(frequency=np.zeros(2), step=np.zeros(2, np.int64), start=np.zeros(2, np.int64), wrap=np.zeros(2, np.int32), width=np.zeros(2, np.int32),
               max_extent=np.zeros(2, np.uint32), key=setup_seed(d["seed"]), stitched=int(tile is not None))
    for a in range(2):
        f, o = d["base_frequency"][a], d["origin"][a]
        if not (math.isfinite(f) and f >= 0.0) or not math.isfinite(o):
            raise ValueError("a base_frequency or an origin")
        if tile is not None and f != 0.0:
            t = tile[2 + a] * f
            if not math.isfinite(t):
                raise ValueError("the stitched frequency")
            lo, hi = math.floor(t) / tile[2 + a], math.ceil(t) / tile[2 + a]
            f = lo if (lo != 0.0 and f / lo < hi / f) else hi
        fs = f * 4294967296.0
        if not fs < 2.0 ** 62:
            raise ValueError("a base_frequency too large")
        centre = o if no_half else o + 0.5
        os_ = (centre * f) * 4294967296.0
        if not abs(os_) < 2.0 ** 62:
            raise ValueError("the origin is beyond the position range")
        step, start = round(fs), round(os_)  # (Python rounds a float half to even, exactly)
        if abs(start) > L:
            raise ValueError("the origin is beyond the position range of this many octaves")
        out["frequency"][a], out["step"][a], out["start"][a] = f, step, start
        out["max_extent"][a] = 0xFFFFFFFF if step == 0 else min(0xFFFFFFFF, (L - start) // step + 1)
        if tile is not None:
            wd, fl = tile[2 + a] * f + 0.5, math.floor(tile[a] * f)
            if not (wd < 2.0 ** 31 and abs(fl) < 2.0 ** 31):
                raise ValueError("the stitch tile is beyond the lattice range")
            width = int(wd)
            wrap = int(fl) + width
            lim = 0x7FFFFFFF >> shift
            if width > lim or abs(wrap) > lim:
                raise ValueError("the stitch tile is beyond the lattice range of this many octaves")
            out["width"][a], out["wrap"][a] = width, wrap
    return out


# ---- the texels ----

def _axis(p, k, wrap, width, stitched, mask_first, trunc_cells):
    """Octave k of the positions p (int64): the masked lattice indices b0, b1 (int64) and the fraction r0 (float32)."""
    q = p << k
    cell = q >> 32
    if trunc_cells:
        cell = np.where(q < 0, -((-q) >> 32), cell)
    r0 = ((q & 0xFFFFFFFF) >> 8).astype(F) * F(2.0 ** -24)
    b0, b1 = cell, cell + 1
    if stitched:
        wk, nk = int(wrap) << k, int(width) << k
        if mask_first:
            b0, b1 = b0 & 255, b1 & 255
        b0 = np.where(b0 >= wk, b0 - nk, b0)
        b1 = np.where(b1 >= wk, b1 - nk, b1)
    return b0 & 255, b1 & 255, r0


def _s(t, s_order):
    if s_order:
        return (t * (t * fmaf32(F(-2.0), t, F(3.0))).astype(F)).astype(F)
    return ((t * t).astype(F) * fmaf32(F(-2.0), t, F(3.0))).astype(F)


def _lerp(t, a, b, expanded):
    if expanded:
        return ((a + (t * b).astype(F)).astype(F) - (t * a).astype(F)).astype(F)
    return fmaf32(t, (b - a).astype(F), a)


def values(X, Y, mask_first=False, single_level=False, s_order=False, lerp_expanded=False, ratio_after=False, abs_fractal=False, trunc_cells=False,
           no_half=False, **kw):
    """The four channels, float32 (len(Y), len(X), 4) BEFORE the rounding to f16, at the texels X x Y (int64 arrays) of the image."""
    d = _desc(kw)
    pl = plan(no_half=no_half, **kw)
    P, G, _ = tables(d["seed"])
    P = P.astype(np.int64)
    kind, octaves, stitched = int(d["kind"]), int(d["octaves"]), bool(pl["stitched"])
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    px, py = int(pl["start"][0]) + X * int(pl["step"][0]), int(pl["start"][1]) + Y * int(pl["step"][1])
    total = np.zeros((len(Y), len(X), 4), F)
    for k in range(octaves):
        bx0, bx1, rx0 = _axis(px, k, pl["wrap"][0], pl["width"][0], stitched, mask_first, trunc_cells)
        by0, by1, ry0 = _axis(py, k, pl["wrap"][1], pl["width"][1], stitched, mask_first, trunc_cells)
        rx1, ry1 = (rx0 - F(1.0)).astype(F), (ry0 - F(1.0)).astype(F)
        i, j = (bx0, bx1) if single_level else (P[bx0], P[bx1])
        corners = [P[(i[None, :] + by0[:, None]) & 255], P[(j[None, :] + by0[:, None]) & 255], P[(i[None, :] + by1[:, None]) & 255],
                   P[(j[None, :] + by1[:, None]) & 255]]
        offsets = [(rx0, ry0), (rx1, ry0), (rx0, ry1), (rx1, ry1)]
        sx, sy = _s(rx0, s_order)[None, :], _s(ry0, s_order)[:, None]
        ratio = F(2.0 ** -k)
        for c in range(4):
            u = []
            for b, (rx, ry) in zip(corners, offsets):
                g = G[c][b]  # (H, W, 2)
                u.append(fmaf32(ry[:, None], g[..., 1], (rx[None, :] * g[..., 0]).astype(F)))
            n = _lerp(sy, _lerp(sx, u[0], u[1], lerp_expanded), _lerp(sx, u[2], u[3], lerp_expanded), lerp_expanded)
            v = np.abs(n) if (kind == TURBULENCE or abs_fractal) else n
            if ratio_after:
                total[..., c] = ((total[..., c] + v).astype(F) * ratio).astype(F)
            else:
                total[..., c] = fmaf32(v, ratio, total[..., c])
    v = fmaf32(total, F(0.5), F(0.5)) if kind == FRACTAL_NOISE else total
    return fmin(fmax(v, F(0.0)), F(1.0)).astype(F)


def turbulence(shape, rect=None, dst_bits=None, **kw):
    """What jh_turbulence leaves in an image of `shape` = (H, W): uint16 (H, W, 4).  dst_bits: what the image held (None: never
    written, which reads as transparent black outside the rectangle).  The image extent is checked against the plan's max_extent."""
    H, W = shape[:2]
    variants = {k: kw.pop(k) for k in list(kw) if k not in DEFAULTS}
    pl = plan(no_half=variants.get("no_half", False), **kw)
    if W > pl["max_extent"][0] or H > pl["max_extent"][1]:
        raise ValueError("the image reaches beyond the position range")
    x, y, w, h = resolve((H, W), rect)
    out = np.zeros((H, W, 4), np.uint16) if dst_bits is None else np.array(dst_bits, np.uint16).reshape(H, W, 4).copy()
    if w and h:
        v = values(np.arange(x, x + w), np.arange(y, y + h), **variants, **kw)
        out[y:y + h, x:x + w] = v.astype(np.float16).view(np.uint16)
    return out
