"""The battery jh_distance is held to (tests/test_gpu_distance.py) and the reference's sensitivity is measured on
(tests/test_distance_spec.py).  A case: name, w, h, content (kind and its argument), channel, threshold, which, edge, R, scale,
offset, color, flags, rect (or None), in_place, and `inst`, the instantiation of k_dist_rows it runs (jello_amd/csrc/kernels_distance.hip:
<STRAIGHT, SIGNED>).  Images have at most 16 600 texels, so that the all-pairs reference stays well under a second a case.

Sizes: 1x1, 1x5, 5x1, and one on each side of every boundary of the kernels:
  k_dist_cols  a strip of 64 PLANE columns (w + 2 R)        w + 2 R = 63, 64, 65 and 127 .. 129 from the widths and radii below
               a segment of 32 rows (more only on images    heights 31, 32, 33, 63, 64, 65 (one, two and three segments), 127 .. 129, 600 and
               of 2^15 texels and up: the timing tool's)     8300 (19 and 260 segments); the warm-up is R rows: heights below and above R
  k_dist_rows  a row segment of 256 outputs                 widths 255, 256, 257 (257: a second segment of one texel), 600
               16-byte staging units                        odd widths and odd R put the staged run at every phase of the 16-byte
                                                            grid; the last unit of the planes is the one loaded halfword by halfword
               the launcher's grid, 32 workgroups x CUs     2 x 8300: 8300 row items, more than 8192 on 256 CUs -- the grid stride
               (k_dist_cols would need 2^19 items: no case; its stride is the same loop)
Radii: 1, 2, 15, 16, 17, 64, 255."""
import functools
import zlib

import numpy as np

import blur_cases
import distance_ref
from distance_ref import CLAMP, INNER, OUTER, SIGNED, STRAIGHT, ZERO
from jello_amd import distance as ramps

POISON = blur_cases.POISON
ONE, ZERO_BITS, NEG0, HALF, INF, NINF, NAN, SUB, NSUB, TWO = 0x3C00, 0x0000, 0x8000, 0x3800, 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8001, 0x4000
VALUES = [ZERO_BITS, NEG0, SUB, NSUB, HALF, ONE, TWO, INF, NINF, NAN, 0xFE00, 0x3400]
SUBNORMAL = float(np.array(SUB, np.uint16).view(np.float16))  # 2^-24
WHICH_NAMES = {OUTER: "outer", INNER: "inner", SIGNED: "signed"}
COMBOS = [(which, edge, flags) for which in (OUTER, INNER, SIGNED) for edge in (ZERO, CLAMP) for flags in (0, STRAIGHT)]


def inst(which, flags):
    return "k_dist_rows<%s, %s>" % ("true" if flags & STRAIGHT else "false", "true" if which == SIGNED else "false")


def blob(w, h):
    """A glyph-like shape: a ring with a bar through it and a one-texel hole in the bar."""
    Y, X = np.mgrid[0:h, 0:w]
    cx, cy, r = (w - 1) / 2.0, (h - 1) / 2.0, max(1.0, min(w, h) / 2.0 - 1.5)
    d = np.hypot(X - cx, Y - cy)
    m = ((d <= r) & (d >= r * 0.55)) | ((np.abs(Y - cy) <= max(1, h // 8)) & (np.abs(X - cx) <= r))
    m[int(cy), int(cx)] = False
    return m


def content(kind, arg, w, h, channel, seed):
    """(h, w, 4) uint16: 'unit' values everywhere, and in `channel`: 'seeds': 1 at the (x, y) of `arg`, 0 elsewhere; 'random': 1 with
    probability `arg`; 'blob'; 'full': 1 everywhere; 'hole': 1 but at `arg`; 'values': drawn from VALUES; 'never': all zero (the source
    is only created)."""
    if kind == "never":
        return np.zeros((h, w, 4), np.uint16)
    rng = np.random.default_rng(seed)
    bits = blur_cases.content("unit", w, h, seed)
    if kind == "values":
        bits[..., channel] = rng.choice(np.array(VALUES, np.uint16), (h, w))
        return bits
    if kind == "seeds":
        m = np.zeros((h, w), bool)
        for (x, y) in arg:
            m[y, x] = True
    elif kind == "random":
        m = rng.random((h, w)) < arg
    elif kind == "blob":
        m = blob(w, h)
    elif kind == "full":
        m = np.ones((h, w), bool)
    elif kind == "hole":
        m = np.ones((h, w), bool)
        m[arg[1], arg[0]] = False
    else:
        raise ValueError(kind)
    bits[..., channel] = np.where(m, ONE, ZERO_BITS)
    return bits


def _case(w, h, kind, arg=None, which=OUTER, edge=ZERO, flags=0, R=2, channel=3, threshold=0.5, scale=None, offset=None, color=(0.2, 0.5, 0.1, 0.8),
          rect=None, in_place=False, tag=""):
    if scale is None:  # the whole range of s onto (0, 1), so that every distance shows
        scale, offset = (1.0 / (2 * R + 2), 0.5) if which == SIGNED else (1.0 / (R + 2), 0.0)
    name = "%dx%d_%s_%s_%s%s_R%d%s%s%s" % (w, h, kind + tag, WHICH_NAMES[which], "clamp" if edge else "zero", "_straight" if flags else "", R,
                                             "" if channel == 3 else "_ch%d" % channel, "" if rect is None else "_r%d_%d_%d_%d" % rect,
                                             "_inplace" if in_place else "")
    return dict(name=name, w=w, h=h, kind=kind, arg=arg, which=which, edge=edge, flags=flags, R=R, channel=channel, threshold=threshold, scale=scale,
                offset=offset, color=tuple(color), rect=rect, in_place=in_place, inst=inst(which, flags))


def _battery():
    out, n = [], 0

    def combos(k):  # k of the twelve (which, edge, flags), in turn
        nonlocal n
        picked = [COMBOS[(n + 5 * i) % 12] for i in range(k)]
        n += 1
        return picked

    # sizes x radii on random seeds; in place and into a second image in turn
    for (w, h) in [(1, 1), (1, 5), (5, 1), (7, 5), (61, 3), (62, 3), (63, 4), (64, 3), (65, 2), (3, 31), (2, 32), (3, 33), (3, 63), (2, 64), (3, 65), (9, 66),
                   (125, 2), (126, 3), (127, 2), (255, 2), (256, 2), (257, 3)]:
        for R in (1, 2, 15, 16, 17):
            for i, (which, edge, flags) in enumerate(combos(2)):
                out.append(_case(w, h, "random", 0.04, which, edge, flags, R, in_place=(n + i) % 2 == 0))
    for (w, h) in [(3, 127), (2, 128), (3, 129), (36, 24)]:
        for i, (which, edge, flags) in enumerate(combos(3)):
            out.append(_case(w, h, "random", 0.01, which, edge, flags, 64, in_place=i == 1))
    # R = 255: each pass alone meets the cap
    for (w, h) in [(1, 600), (600, 1)]:
        for (which, edge, flags) in COMBOS:
            out.append(_case(w, h, "seeds", ((0, 0),) if w == 1 else ((w - 1, 0),), which, edge, flags, 255))
        out.append(_case(w, h, "random", 0.004, SIGNED, ZERO, STRAIGHT, 255, in_place=True))
    out.append(_case(40, 24, "random", 0.002, OUTER, ZERO, 0, 255))
    out.append(_case(40, 24, "blob", None, SIGNED, CLAMP, STRAIGHT, 255, in_place=True))
    # more row items than the launcher's grid has workgroups
    out.append(_case(2, 8300, "seeds", ((0, 0), (1, 4000), (0, 8299)), OUTER, ZERO, STRAIGHT, 17))
    # single seeds at exactly R and R + 1 along an axis, at (R, R) on the diagonal, Pythagorean ties, two seeds at equal distance
    for R in (1, 2, 5, 16):
        side = 2 * R + 5
        c = side // 2
        for flags in (0, STRAIGHT):
            out.append(_case(side, side, "seeds", ((c, c),), OUTER, CLAMP, flags, R, tag="_centre"))
        out.append(_case(side, side, "hole", (c, c), INNER, CLAMP, STRAIGHT, R, tag="_centre"))
        out.append(_case(side, side, "seeds", ((c, c),), SIGNED, ZERO, STRAIGHT, R, tag="_centre"))
    out.append(_case(13, 9, "seeds", ((0, 0), (5, 0), (3, 4)), OUTER, CLAMP, STRAIGHT, 5, tag="_pythagoras"))  # (8, 4) is 5 from (5, 0) ... and (3, 4)
    out.append(_case(9, 7, "seeds", ((1, 3), (7, 3)), OUTER, ZERO, STRAIGHT, 4, tag="_equal"))
    out.append(_case(9, 7, "seeds", ((1, 3), (7, 3)), SIGNED, ZERO, 0, 4, tag="_equal"))
    # seed sets: none, all, the four corners, a blob, a one-texel hole -- in every which x edge x STRAIGHT
    for (which, edge, flags) in COMBOS:
        out.append(_case(37, 21, "seeds", (), which, edge, flags, 3, tag="_none"))
        out.append(_case(37, 21, "full", None, which, edge, flags, 3))
        out.append(_case(37, 21, "seeds", ((0, 0), (36, 0), (0, 20), (36, 20)), which, edge, flags, 15, tag="_corners"))
        out.append(_case(47, 31, "blob", None, which, edge, flags, 6, in_place=flags == 0))
        out.append(_case(37, 21, "hole", (20, 9), which, edge, flags, 4))
    # rectangles at odd offsets with poison around, seeds only outside the rectangle among them
    for (which, edge, flags) in COMBOS:
        out.append(_case(67, 41, "blob", None, which, edge, flags, 5, rect=(9, 5, 41, 21)))
        out.append(_case(67, 41, "random", 0.03, which, edge, flags, 9, rect=(31, 17, 1, 1), in_place=True))
        out.append(_case(67, 41, "seeds", ((2, 3), (60, 38), (33, 1)), which, edge, flags, 12, rect=(11, 7, 45, 27), tag="_outside"))
        out.append(_case(67, 41, "random", 0.03, which, edge, flags, 3, rect=(21, 11, 46, 30), in_place=True))
    # channels, thresholds, channel content
    for ch in (0, 1, 2, 3):
        out.append(_case(33, 17, "blob", None, SIGNED, ZERO, STRAIGHT, 4, channel=ch))
    for i, t in enumerate((0.0, -0.0, 0.5, SUBNORMAL, 1.0, 7.0e4)):
        for j, (which, edge, flags) in enumerate(((OUTER, ZERO, 0), (INNER, CLAMP, STRAIGHT), (SIGNED, ZERO, STRAIGHT))):
            out.append(_case(33, 17, "values", None, which, edge, flags, 3, channel=(i + j) % 4, threshold=t, tag="_t%d" % i))
            out.append(_case(33, 17, "never", None, which, edge, flags, 3, threshold=t, tag="_t%d" % i))
    # ramps: the four of jello_amd.distance, scale 0, a negative scale, a product that overflows
    for (which, edge, flags) in ((OUTER, ZERO, 0), (INNER, ZERO, STRAIGHT), (SIGNED, CLAMP, STRAIGHT), (OUTER, CLAMP, 0)):
        for tag, r in (("_outline", ramps.outline(2.5)), ("_inset", ramps.inset(1.75)), ("_glow", ramps.glow(5.5)), ("_innerglow", ramps.glow(3.0, True)), ("_sdf", ramps.sdf(8))):
            out.append(_case(41, 23, "blob", None, int(r["which"]), edge, flags, r["max_distance"], scale=r["scale"], offset=r["offset"], tag=tag))
        for tag, (scale, offset) in (("_scale0", (0.0, 0.25)), ("_negative", (-0.125, 0.75)), ("_overflow", (3.0e38, -1.0)), ("_underflow", (-3.0e38, 2.0))):
            out.append(_case(41, 23, "blob", None, which, edge, flags, 7, scale=scale, offset=offset, tag=tag))
    # colours: a negative alpha, an Inf, zeros
    for color in ((0.3, 0.2, 0.1, -0.5), (float("inf"), 0.5, 0.25, 1.0), (0.0, 0.0, 0.0, 0.0), (-0.0, 2.0, -1.0, 1.0)):
        for flags in (0, STRAIGHT):
            out.append(_case(29, 15, "blob", None, OUTER, ZERO, flags, 4, color=color, tag="_c%g_%g" % (color[0], color[3])))
    return out


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES), [c["name"] for c in CASES if sum(d["name"] == c["name"] for d in CASES) > 1][:3]


def source(case):
    return content(case["kind"], case["arg"], case["w"], case["h"], case["channel"], seed=zlib.crc32(case["name"].encode()))


def keywords(case):
    """The case as the keywords of distance_ref.distance."""
    return dict(channel=case["channel"], threshold=case["threshold"], which=case["which"], edge=case["edge"], R=case["R"], scale=case["scale"],
                offset=case["offset"], color=case["color"], flags=case["flags"], rect=case["rect"])


@functools.lru_cache(maxsize=None)
def expected(name, **variant):
    """What dst holds after the case's call, by tests/distance_ref.py (computed once per case and variant; do not modify the result)."""
    c = BY_NAME[name]
    src = source(c)
    before = src if c["in_place"] else np.full_like(src, POISON)
    out = distance_ref.distance(src, dst_bits=before, **keywords(c), **variant)
    out.setflags(write=False)
    return out
