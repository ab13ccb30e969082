"""The battery jh_warp is held to (tests/test_gpu_warp.py) and the reference's sensitivity is measured on (tests/test_warp_spec.py).
A case: name, the source image's size and rectangle, the destination image's size and rectangle, the matrix (source rectangle ->
destination image), filter, edge, flags, the content kind, and what dst held before ('poison' or 'never').  Every image but the one of
the grid-stride case is at most 64 x 48.

Sizes on each side of every boundary of the kernel (jello_amd/csrc/kernels_warp.hip, on the tile constants of warp_taps.h):
  a tile's row, 16 texels = one 128-byte line of dst     destination widths 1, 15, 16, 17, 31, 33
  a wave's tile, 4 rows; a workgroup's, 16               destination heights 1, 3, 4, 5, 15, 16, 17, 31, 33
  the tile grid lies on dst's 128-byte lines             widths that are no multiple of 16 and rectangles at odd offsets: the phase
                                                         of the grid differs from row to row
  the workgroups stride over the tiles                   1040 x 520 = 2 178 tiles, above the launcher's cap of 8 per CU x 256 CUs
Rectangles at odd offsets: the source image outside its rectangle is NaN, which a tap that left the rectangle would carry into the
result, and dst outside its rectangle is POISON, which has to stay."""
import functools
import math
import zlib

import numpy as np

import resample_cases
import warp_ref
from warp_ref import BICUBIC, BILINEAR, CLAMP, EDGE_NAMES, EDGES, FILTER_NAMES, FILTERS, MIRROR, NEAREST, REPEAT, STRAIGHT, ZERO

KINDS = ["finite", "unit", "nonfinite", "never", "subnormal", "zeros", "alpha01", "negalpha", "infalpha0"]
POISON = 0x5A5A  # what dst holds before the call (a finite f16)
NAN = 0x7E00     # what the source holds outside its rectangle
ITEM_WIDTHS = [1, 15, 16, 17, 31, 33]
ITEM_HEIGHTS = [1, 3, 4, 5, 15, 16, 17, 31, 33]
BIG = ((1040, 520), (520, 260))  # the grid-stride case: destination and source sizes


def content(kind, w, h, seed):
    """(h, w, 4) uint16 f16 bit patterns: the kinds of tests/resample_cases.py, and 'negalpha' ('unit' with a negative alpha in
    every other run of texels), 'infalpha0' ('unit' with texels of an infinite colour over alpha 0, whose premultiplied operand is a
    NaN)."""
    if kind not in ("negalpha", "infalpha0"):
        return resample_cases.content(kind, w, h, seed)
    bits = resample_cases.content("unit", w, h, seed)
    rng = np.random.default_rng(seed + 1)
    if kind == "negalpha":
        runs = np.repeat(rng.integers(0, 2, (h, (w + 2) // 3)), 3, axis=1)[:, :w]
        bits[..., 3] = np.where(runs == 1, bits[..., 3] | 0x8000, bits[..., 3] & 0x7FFF)
    else:
        pick = rng.random((h, w)) < 0.1
        bits[pick] = np.array([0x7C00, 0x3C00, 0xFC00, 0x0000], np.uint16)
    return bits


# ---- matrices: (a, b, c, d, e, f), x' = a x + c y + e, y' = b x + d y + f ----

def translate(tx, ty):
    return (1.0, 0.0, 0.0, 1.0, float(tx), float(ty))


def scale(k):
    return (float(k), 0.0, 0.0, float(k), 0.0, 0.0)


def rotate(deg, src_size, dst_size, k=1.0):
    """A rotation by deg (and a scale k) that takes the source's centre to the destination's."""
    t = math.radians(deg)
    a, b, c, d = k * math.cos(t), k * math.sin(t), -k * math.sin(t), k * math.cos(t)
    cx, cy, ox, oy = src_size[0] / 2.0, src_size[1] / 2.0, dst_size[0] / 2.0, dst_size[1] / 2.0
    return (a, b, c, d, ox - (a * cx + c * cy), oy - (b * cx + d * cy))


def octant(k, w, h):
    """The eight flips and quarter turns of a w x h source, each onto [0, w) x [0, h) or [0, h) x [0, w)."""
    return [(1.0, 0.0, 0.0, 1.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 1.0, float(w), 0.0), (1.0, 0.0, 0.0, -1.0, 0.0, float(h)),
            (-1.0, 0.0, 0.0, -1.0, float(w), float(h)), (0.0, 1.0, 1.0, 0.0, 0.0, 0.0), (0.0, 1.0, -1.0, 0.0, float(h), 0.0),
            (0.0, -1.0, 1.0, 0.0, 0.0, float(w)), (0.0, -1.0, -1.0, 0.0, float(h), float(w))][k]


OCTANT_NAMES = ["id", "flipx", "flipy", "rot180", "transpose", "rot90", "rot270", "antitranspose"]


def octant_permutation(k, src):
    """What octant(k) makes of the (h, w, 4) array src."""
    return [src, src[:, ::-1], src[::-1], src[::-1, ::-1], src.transpose(1, 0, 2), src.transpose(1, 0, 2)[:, ::-1],
            src.transpose(1, 0, 2)[::-1], src.transpose(1, 0, 2)[::-1, ::-1]][k]


def _case(tag, matrix, filt, edge, flags, src_size, dst_size, src_rect=None, dst_rect=None, kind="finite", prior="poison"):
    name = "%s_%s_%s_%s_%dx%d%s_to_%dx%d%s_%s%s" % (
        tag, FILTER_NAMES[filt], EDGE_NAMES[edge], "straight" if flags else "premul", src_size[0], src_size[1],
        "" if src_rect is None else "_r%d_%d_%d_%d" % src_rect, dst_size[0], dst_size[1], "" if dst_rect is None else "_r%d_%d_%d_%d" % dst_rect,
        kind, "" if prior == "poison" else "_" + prior)
    return {"name": name, "matrix": tuple(float(v) for v in matrix), "filter": filt, "edge": edge, "flags": flags, "src_size": src_size,
            "dst_size": dst_size, "src_rect": src_rect, "dst_rect": dst_rect, "kind": kind, "prior": prior}


def _battery():
    out, n = [], 0
    S, D = (41, 29), (47, 33)

    def combos():  # every filter x every edge x both operand modes, rotating
        nonlocal n
        n += 1
        return FILTERS[n % 3], EDGES[(n // 3) % 4], STRAIGHT if (n // 12) % 2 else 0

    # every filter x every edge x both operand modes on a rotation with a scale and a fractional offset, unit and finite content
    for filt in FILTERS:
        for edge in EDGES:
            for flags in (0, STRAIGHT):
                out.append(_case("rot30s", rotate(30, S, D, 1.3), filt, edge, flags, S, D, kind="unit"))
                out.append(_case("shear", (1.0, 0.3, 0.5, 1.0, -2.25, 1.5), filt, edge, flags, S, D, kind="finite"))
    # the kernel's tile boundaries
    for dw in ITEM_WIDTHS:
        f, e, fl = combos()
        out.append(_case("tilew", rotate(30, (19, 7), (dw, 5)), f, e, fl, (19, 7), (dw, 5), kind="unit"))
    for dh in ITEM_HEIGHTS:
        f, e, fl = combos()
        out.append(_case("tileh", rotate(45, (9, 21), (17, dh)), f, e, fl, (9, 21), (17, dh)))
    for filt in FILTERS:
        out.append(_case("one", translate(0.25, -0.25), filt, CLAMP, 0, (3, 2), (1, 1)))
        out.append(_case("row", scale(2), filt, MIRROR, STRAIGHT, (20, 1), (37, 1)))
        out.append(_case("col", scale(2), filt, REPEAT, 0, (1, 20), (1, 37)))
    # the matrices
    for filt in FILTERS:
        for edge in (ZERO, REPEAT):
            out.append(_case("identity", translate(0, 0), filt, edge, STRAIGHT, S, S, kind="finite"))
            for t in ((3, 2), (-2, -5), (0.5, 0.5), (-0.5, 1.5), (-7.5, 0.0)):
                out.append(_case("t%g_%g" % t, translate(*t), filt, edge, 0, S, D, kind="unit"))
        for k in range(8):
            w, h = S
            out.append(_case(OCTANT_NAMES[k], octant(k, w, h), filt, EDGES[k % 4], STRAIGHT, S, S if k < 4 else (h, w), kind="finite"))
        out.append(_case("rot30", rotate(30, S, D), filt, ZERO, 0, S, D, kind="unit"))
        out.append(_case("rot45", rotate(45, S, D), filt, CLAMP, 0, S, D, kind="unit"))
        out.append(_case("up2", scale(2), filt, CLAMP, 0, (32, 24), (64, 48), kind="unit"))
        out.append(_case("up3.7", scale(3.7), filt, ZERO, STRAIGHT, (17, 13), (64, 48)))
        out.append(_case("down2", scale(0.5), filt, MIRROR, 0, (64, 48), (32, 24), kind="unit"))
        out.append(_case("down3", scale(1.0 / 3.0), filt, REPEAT, STRAIGHT, (64, 48), (21, 16)))
        out.append(_case("down64", scale(1.0 / 64.0), filt, REPEAT, STRAIGHT, (64, 48), (5, 3)))  # p = t = 64: the legal limit
        out.append(_case("gone", translate(1000, 1000), filt, ZERO, 0, S, D, kind="unit"))
        out.append(_case("gone", translate(-1000, 0), filt, CLAMP, 0, S, D, kind="unit"))
    # U just below, at and just above a multiple of 2^32 (NEAREST), U' negative (floor, not truncation), fractions 0x0000 and 0xffff,
    # and a fraction whose dropped bits are above one half
    eps = 2.0 ** -32
    for e in (-0.5, -0.5 + eps, -0.5 - eps, 0.75, 0.25):
        for edge in (ZERO, REPEAT):
            out.append(_case("edge%+.10f" % e, translate(e, e), NEAREST, edge, STRAIGHT, (23, 9), (25, 11)))
    for filt in (BILINEAR, BICUBIC):
        for e in (0.25, 0.0, 2.0 ** -16, -1.5 * 2.0 ** -17, 0.5 + 3.0 * 2.0 ** -18):
            for edge in (ZERO, REPEAT):
                out.append(_case("frac%+.10f" % e, translate(e, e), filt, edge, STRAIGHT, (23, 9), (25, 11)))
    # REPEAT and MIRROR with n = 1, 2 and 3 and indices far outside
    for n_src in (1, 2, 3):
        for edge in (REPEAT, MIRROR, CLAMP, ZERO):
            f, _, fl = combos()
            out.append(_case("far", (0.31, 0.0, 0.0, 0.43, -9.7, 4.2), f, edge, fl, (n_src, n_src), (40, 30), kind="unit"))
            out.append(_case("far", rotate(30, (n_src, 3), (33, 17), 0.2), BICUBIC, edge, fl, (n_src, 3), (33, 17), kind="unit"))
    # rectangles at odd offsets inside images of odd and even widths, images of different sizes
    for filt in FILTERS:
        for edge in EDGES:
            flags = STRAIGHT if (filt + edge) % 2 else 0
            out.append(_case("rect", rotate(30, (31, 19), (49, 37), 1.2), filt, edge, flags, (45, 29), (49, 37), (3, 5, 31, 19), (5, 3, 33, 21), "unit"))
            out.append(_case("rect", (1.5, 0.25, -0.25, 1.5, 3.0, -2.0), filt, edge, flags, (36, 20), (64, 40), (1, 1, 21, 9), (7, 1, 39, 35), "finite"))
    out.append(_case("rect", rotate(45, (31, 19), (49, 37)), BICUBIC, ZERO, 0, (45, 29), (49, 37), (3, 5, 31, 19), (5, 3, 33, 21), "unit", "never"))
    out.append(_case("rect", translate(18.5, 35.5), BILINEAR, ZERO, STRAIGHT, (33, 9), (20, 37), (32, 8, 1, 1), (19, 36, 1, 1), "finite"))
    # values
    for kind in KINDS:
        for flags in (0, STRAIGHT):
            out.append(_case("values", rotate(30, (37, 11), (41, 17), 1.1), BICUBIC, ZERO, flags, (37, 11), (41, 17), kind=kind))
            out.append(_case("values", (1.7, 0.0, 0.0, 1.7, -0.3, 0.4), BILINEAR, MIRROR, flags, (23, 5), (40, 13), kind=kind))
            out.append(_case("values", translate(1, -1), NEAREST, CLAMP, flags, (23, 5), (25, 6), kind=kind))
    # the grid-stride loop
    out.append(_case("big", scale(2), BILINEAR, ZERO, 0, BIG[1], BIG[0], kind="unit"))
    seen, uniq = set(), []
    for c in out:
        if c["name"] not in seen:
            seen.add(c["name"])
            uniq.append(c)
    return uniq


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}


def rect_of(case, which):
    """(x, y, w, h) of the case's source or destination rectangle."""
    r, (w, h) = case[which + "_rect"], case[which + "_size"]
    return (0, 0, w, h) if r is None else r


def source(case):
    """The source image's bits: the content inside the rectangle, NaN around it."""
    (w, h), (x, y, rw, rh) = case["src_size"], rect_of(case, "src")
    img = np.full((h, w, 4), NAN, np.uint16)
    img[y:y + rh, x:x + rw] = content(case["kind"], rw, rh, zlib.crc32(case["name"].encode()) & 0x7FFFFFFF)
    return img


def before(case):
    """What dst holds before the call, or None for a never-written dst."""
    w, h = case["dst_size"]
    return None if case["prior"] == "never" else np.full((h, w, 4), POISON, np.uint16)


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    w, h = c["dst_size"]
    out = warp_ref.warp(source(c), (h, w), c["matrix"], c["filter"], c["edge"], c["flags"], c["src_rect"], c["dst_rect"], before(c), **dict(variant))
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/warp_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
