"""The battery jh_displace is held to (tests/test_gpu_displace.py) and the reference's sensitivity is measured on
(tests/test_displace_spec.py).  A case: name, the instantiation of the kernel it runs ("filter/edge/operand"), the source image's size
and rectangle, the destination image's size and rectangle, the matrix (source rectangle -> destination image), filter, edge, flags, the
source's content kind, what dst held before ('poison' or 'never'), the scale pair, the channel pair, the map's kind, and which image
the map is: 'own' (a third image), 'dst', 'src', or 'never' (a third image that was never written).  Every image but the grid-stride
case's is at most 64 x 48.

Sizes on each side of every boundary of the kernel (jello_amd/csrc/warp_taps.h; they are jh_warp's, tests/warp_cases.py):
widths 1, 15, 16, 17, 31, 33 against the tile row of 16 texels, heights 1, 3, 4, 5, 15, 16, 17 against the wave's 4 and the workgroup's
16 rows, rectangles at odd offsets (the phase of the tile grid differs from row to row), and 1040 x 520 = 2 178 tiles against the
launcher's cap of 2 048 workgroups.  The source image outside its rectangle is NaN, which a tap that left the rectangle would carry into
the result; dst outside its rectangle is POISON (or, where the map is dst, the map), which has to stay.

Maps (`map_bits`): 'random' (every channel uniform in [0, 1)), 'wide' (uniform in [-1, 2)), 'values' (+-0, subnormals, 0.5, above 1,
negative, +-Inf, NaN, a different order in every channel), 'const:<bits>' (one f16 bit pattern in all four channels), 'edges' (the
values around 0, 0.5 and 1 whose offsets under a power-of-two scale put a position just below, at and just above a texel boundary
and give the fractions 0x0000 and 0xffff)."""
import functools
import zlib

import numpy as np

import displace_ref
import warp_cases
from displace_ref import A, B, CHANNEL_NAMES, CHANNELS, G, IDENTITY, R
from warp_cases import BIG, ITEM_HEIGHTS, ITEM_WIDTHS, KINDS, NAN, POISON, rotate, translate
from warp_cases import scale as scaling
from warp_ref import BICUBIC, BILINEAR, CLAMP, EDGE_NAMES, EDGES, FILTER_NAMES, FILTERS, MIRROR, NEAREST, REPEAT, STRAIGHT, ZERO

HEIGHTS = [h for h in ITEM_HEIGHTS if h <= 17]
# around 0: -2^-24, -0, +0, 2^-24 (t = -0.5 -+ 2^-24: at scale 1 a texel-centre position lands on a boundary from both sides); around 0.5:
# 0.5 - 2^-12, 0.5, 0.5 + 2^-11 (fractions 0xffff and 0x0000 at scales 2^-4 and 2^-5; D = 0.5 and 1.5 at scales 2^-22 and 3 x 2^-22);
# around 1: 1 - 2^-11, 1, 1 + 2^-10 (t = 0.5: the next boundary)
EDGE_VALUES = [0x8001, 0x8000, 0x0000, 0x0001, 0x37FF, 0x3800, 0x3801, 0x3BFF, 0x3C00, 0x3C01]
SPECIAL_VALUES = [0x0000, 0x8000, 0x0001, 0x83FF, 0x03FF, 0x3800, 0x3C00, 0x4200, 0x5640, 0xB800, 0xC500, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x3555]


def map_bits(kind, w, h, seed):
    """(h, w, 4) uint16: the map of that kind."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.random((h, w, 4), dtype=np.float32).astype(np.float16).view(np.uint16)
    if kind == "wide":
        return (rng.random((h, w, 4), dtype=np.float32) * 3.0 - 1.0).astype(np.float16).view(np.uint16)
    if kind.startswith("const:"):
        return np.full((h, w, 4), int(kind[6:], 16), np.uint16)
    values = np.array(EDGE_VALUES if kind == "edges" else SPECIAL_VALUES, np.uint16)
    assert kind in ("edges", "values"), kind
    i = np.arange(w)[None, :, None] + 3 * np.arange(h)[:, None, None] + np.array([0, 1, 5, 7])[None, None, :]
    return values[i % len(values)]


def _case(tag, filt, edge, flags, src_size, dst_size, scale, channels=(R, G), matrix=IDENTITY, map_kind="random", map_is="own", src_rect=None, dst_rect=None,
          kind="unit", prior="poison"):
    sx, sy = scale if isinstance(scale, tuple) else (scale, scale)
    name = "%s_%s_%s_%s_%dx%d%s_to_%dx%d%s_%s%s_s%g_%g_%s%s_%s_%s" % (
        tag, FILTER_NAMES[filt], EDGE_NAMES[edge], "straight" if flags else "premul", src_size[0], src_size[1],
        "" if src_rect is None else "_r%d_%d_%d_%d" % src_rect, dst_size[0], dst_size[1], "" if dst_rect is None else "_r%d_%d_%d_%d" % dst_rect,
        kind, "" if prior == "poison" else "_" + prior, sx, sy, CHANNEL_NAMES[channels[0]], CHANNEL_NAMES[channels[1]], map_kind.replace(":", ""), map_is)
    assert map_is in ("own", "dst", "src", "never") and (map_is != "src" or (src_size == dst_size))
    return {"name": name, "inst": "%s/%s/%s" % (FILTER_NAMES[filt], EDGE_NAMES[edge], "straight" if flags else "premul"),
            "matrix": tuple(float(v) for v in matrix), "filter": filt, "edge": edge, "flags": flags, "src_size": src_size, "dst_size": dst_size,
            "src_rect": src_rect, "dst_rect": dst_rect, "kind": kind, "prior": prior, "scale": (float(sx), float(sy)), "channels": tuple(channels),
            "map_kind": map_kind, "map_is": map_is}


def _battery():
    out, n = [], 0
    S, D = (41, 29), (47, 33)

    def combos():  # every filter x every edge x both operand modes, rotating
        nonlocal n
        n += 1
        return FILTERS[n % 3], EDGES[(n // 3) % 4], STRAIGHT if (n // 12) % 2 else 0

    # every filter x every edge x both operand modes on a random map: the identity between equal sizes, a rotation between others
    for filt in FILTERS:
        for edge in EDGES:
            for flags in (0, STRAIGHT):
                out.append(_case("all", filt, edge, flags, D, D, (9.0, -6.5), kind="unit"))
                out.append(_case("all", filt, edge, flags, S, D, 5.0, (B, A), rotate(30, S, D, 1.3), kind="finite"))
    # the kernel's tile boundaries
    for dw in ITEM_WIDTHS:
        f, e, fl = combos()
        out.append(_case("tilew", f, e, fl, (19, 7), (dw, 5), 4.0, (G, R), rotate(30, (19, 7), (dw, 5))))
    for dh in HEIGHTS:
        f, e, fl = combos()
        out.append(_case("tileh", f, e, fl, (9, 21), (17, dh), 4.0, (A, B), rotate(45, (9, 21), (17, dh)), kind="finite"))
    for filt in FILTERS:
        out.append(_case("one", filt, CLAMP, 0, (3, 2), (1, 1), 2.0, matrix=translate(0.25, -0.25), kind="finite"))
        out.append(_case("row", filt, MIRROR, STRAIGHT, (20, 1), (5, 1), 6.0, matrix=translate(-3, 0), kind="finite"))
        out.append(_case("col", filt, REPEAT, 0, (1, 20), (1, 5), 6.0, matrix=translate(0, -3)))
    # rectangles at odd offsets in both images, NaN around the source's and POISON around the destination's
    for filt in FILTERS:
        for edge in EDGES:
            flags = STRAIGHT if (filt + edge) % 2 else 0
            out.append(_case("rect", filt, edge, flags, (45, 29), (49, 37), (7.0, 3.0), (R, A), rotate(30, (31, 19), (49, 37), 1.2), src_rect=(3, 5, 31, 19),
                             dst_rect=(5, 3, 33, 21)))
            out.append(_case("rect", filt, edge, flags, (36, 20), (64, 40), 3.0, (G, G), (1.5, 0.25, -0.25, 1.5, 3.0, -2.0), src_rect=(1, 1, 21, 9),
                             dst_rect=(7, 1, 39, 35), kind="finite"))
    out.append(_case("rect", BICUBIC, ZERO, 0, (45, 29), (49, 37), 4.0, matrix=rotate(45, (31, 19), (49, 37)), src_rect=(3, 5, 31, 19), dst_rect=(5, 3, 33, 21),
                     prior="never"))
    out.append(_case("rect", BILINEAR, ZERO, STRAIGHT, (33, 9), (20, 37), 0.75, matrix=translate(18.5, 35.5), src_rect=(32, 8, 1, 1), dst_rect=(19, 36, 1, 1),
                     kind="finite"))
    # the grid-stride loop
    out.append(_case("big", NEAREST, ZERO, 0, BIG[1], BIG[0], 8.0, matrix=scaling(2)))
    # positions just below, at and just above a texel boundary, fractions 0x0000 and 0xffff (power-of-two scales: d is exact), and the
    # rounding of D: 0.5 -> 0 and 1.5 -> 2 against a plan two units of 2^-32 below a boundary
    for s in (1.0, -1.0, 2.0 ** -4, 2.0 ** -5, -2.0 ** -5, 2.0 ** -15):
        for filt in FILTERS:
            out.append(_case("edges", filt, (ZERO, REPEAT, MIRROR)[filt], STRAIGHT, (23, 9), (23, 9), s, (R, B), map_kind="edges", kind="finite"))
    below = translate(0.5 + 2.0 ** -31, 0.5 + 2.0 ** -31)  # U = X 2^32 - 2
    for s in (2.0 ** -22, 3 * 2.0 ** -22, -2.0 ** -22, -3 * 2.0 ** -22, 2.0 ** -21):
        for filt in (NEAREST, BILINEAR):
            out.append(_case("rint", filt, REPEAT, STRAIGHT, (23, 9), (23, 9), s, (R, B), below, map_kind="edges", kind="finite"))
    for s in (2.0 ** -22, -2.0 ** -22):  # U = X 2^32 - 1: a half that rounded away from zero would reach the boundary
        out.append(_case("rint1", NEAREST, REPEAT, STRAIGHT, (23, 9), (23, 9), s, (R, B), translate(0.5 + 2.0 ** -32, 0.5 + 2.0 ** -32), map_kind="edges",
                         kind="finite"))
    # scales: 0, -0, negative, unequal, 1e30 (the clamp from both sides), one that just reaches 2^22
    for s in (0.0, -0.0, (-7.0, 11.5), (0.0, 3.0), 1e30, -1e30, (1e30, 0.25), 2.0 ** 23, (2.0 ** 23 * (1 + 2.0 ** -23), -2.0 ** 23)):
        f, e, fl = combos()
        out.append(_case("scale", f, e, fl, D, D, s, kind="finite"))
        out.append(_case("scale", BILINEAR, (REPEAT, MIRROR)[n % 2], fl, (3, 3), (21, 9), s, map_kind="const:3c00", kind="finite"))
    for filt in FILTERS:  # scales of 24 significant bits: the product rounds, and where it rounds shows
        out.append(_case("odd", filt, (MIRROR, CLAMP, REPEAT)[filt], STRAIGHT, D, D, (977.13, -128.06), kind="finite"))
    # map values: +-0, subnormal, 0.5, above 1, negative, +-Inf, NaN -- and a map that was never written
    for s in (3.0, (0.0, -2.5), 1e30, 2.0 ** -140):
        for filt in FILTERS:
            out.append(_case("values", filt, EDGES[(filt + 1) % 4], 0, D, D, s, (R, B), map_kind="values"))
            out.append(_case("values", filt, REPEAT, STRAIGHT, (5, 4), (33, 17), s, (A, G), map_kind="values", kind="finite"))
    for filt in FILTERS:
        out.append(_case("nomap", filt, ZERO, 0, D, D, (8.0, 5.0), map_is="never"))
        out.append(_case("nomap", filt, MIRROR, STRAIGHT, S, D, 64.0, (A, A), rotate(30, S, D), map_is="never", kind="finite"))
    for bits in ("3800", "0000", "7e00", "fc00", "4400"):
        f, e, fl = combos()
        out.append(_case("const", f, e, fl, D, D, (2.0, -4.0), (B, R), map_kind="const:" + bits))
    # every pair of channels
    for cx in CHANNELS:
        for cy in CHANNELS:
            f, e, fl = combos()
            out.append(_case("channels", f, e, fl, (19, 13), (19, 13), (6.0, 5.0), (cx, cy), map_kind="wide", kind="finite"))
    # REPEAT and MIRROR (and the others) on sources of 1, 2 and 3 texels with displacements far outside
    for n_src in (1, 2, 3):
        for edge in (REPEAT, MIRROR, CLAMP, ZERO):
            f, _, fl = combos()
            out.append(_case("far", f, edge, fl, (n_src, n_src), (40, 30), 1e4, (G, A), (0.31, 0.0, 0.0, 0.43, -9.7, 4.2), map_kind="wide"))
            out.append(_case("far", BICUBIC, edge, fl, (n_src, 3), (33, 17), (1e30, 977.0), matrix=rotate(30, (n_src, 3), (33, 17), 0.2), map_kind="wide"))
    # the source's content
    for kind in KINDS:
        for flags in (0, STRAIGHT):
            out.append(_case("content", BICUBIC, ZERO, flags, (37, 11), (41, 17), 3.0, matrix=rotate(30, (37, 11), (41, 17), 1.1), kind=kind))
            out.append(_case("content", BILINEAR, MIRROR, flags, (23, 5), (40, 13), (5.0, 2.0), (A, R), (1.7, 0.0, 0.0, 1.7, -0.3, 0.4), kind=kind))
            out.append(_case("content", NEAREST, CLAMP, flags, (25, 6), (25, 6), 4.0, kind=kind))
    # the matrices: the identity, an integer and a half-texel translation, a rotation, a 2 x scale
    for filt in FILTERS:
        for tag, m, ssize in (("identity", IDENTITY, D), ("t3_-2", translate(3, -2), D), ("thalf", translate(0.5, -0.5), D), ("rot", rotate(30, S, D), S),
                              ("up2", scaling(2), (24, 17))):
            for edge in (ZERO, CLAMP):
                out.append(_case(tag, filt, edge, 0, ssize, D, (6.0, 4.0), matrix=m))
    # the map is the destination; the map is the source
    for filt in FILTERS:
        for edge in EDGES:
            flags = STRAIGHT if (filt + edge) % 2 else 0
            out.append(_case("inplace", filt, edge, flags, S, D, (7.0, -5.0), (R, G), rotate(30, S, D, 1.2), map_is="dst"))
            out.append(_case("inplace", filt, edge, flags, D, D, 12.0, (A, B), map_is="dst", dst_rect=(5, 3, 33, 21), map_kind="wide", kind="finite"))
            out.append(_case("selfmap", filt, edge, flags, D, D, (10.0, 6.0), (G, A), map_is="src"))
    out.append(_case("inplace", BILINEAR, CLAMP, 0, S, D, 7.0, map_is="dst", map_kind="values"))
    seen, uniq = set(), []
    for c in out:
        if c["name"] not in seen:
            seen.add(c["name"])
            uniq.append(c)
    return uniq


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}
rect_of = warp_cases.rect_of


def _seed(case):
    return zlib.crc32(case["name"].encode()) & 0x7FFFFFFF


def the_map(case):
    """The map's bits, of the destination's size; None for a map that was never written.  Where the map is the source it is the
    source image itself."""
    if case["map_is"] == "never":
        return None
    if case["map_is"] == "src":
        return source(case)
    w, h = case["dst_size"]
    return map_bits(case["map_kind"], w, h, _seed(case) ^ 0x5555)


def source(case):
    """The source image's bits: the content inside the rectangle, NaN around it."""
    (w, h), (x, y, rw, rh) = case["src_size"], rect_of(case, "src")
    img = np.full((h, w, 4), NAN, np.uint16)
    img[y:y + rh, x:x + rw] = warp_cases.content(case["kind"], rw, rh, _seed(case))
    return img


def before(case):
    """What dst holds before the call: the map where the map is dst, None for a never-written dst, POISON otherwise."""
    if case["map_is"] == "dst":
        return the_map(case)
    w, h = case["dst_size"]
    return None if case["prior"] == "never" else np.full((h, w, 4), POISON, np.uint16)


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    w, h = c["dst_size"]
    out = displace_ref.displace(source(c), the_map(c), (h, w), c["scale"], c["channels"][0], c["channels"][1], c["matrix"], c["filter"], c["edge"], c["flags"],
                                c["src_rect"], c["dst_rect"], before(c), **dict(variant))
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/displace_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
