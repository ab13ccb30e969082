"""The battery jh_morphology is held to (tests/test_gpu_morph.py) and the reference's sensitivity is measured on
(tests/test_morph_spec.py).  A case: name, width, height, op, radius (rx, ry), edge, flags, rect (or None), in_place, content.
Images are at most 257 x 140 texels.

Sizes: 1x1, 1x37, 37x1, 7x5, 130x70, and one on each side of every boundary of the kernels (jello_amd/csrc/kernels_morph.hip):
  row segment of a wave, 256 outputs                    widths 255, 256, 257 (257x3: a second segment of one texel)
  the row pass stages 128 texels a step,                widths + 2 rx on either side of 64, 128 and 256 follow from the radii below
    and doubles 64 elements a step                        (63 + 2 x 0, 63 + 2 x 1, 64 + 2 x 32 = 128, 127 / 129 with rx = 0 ...)
  column strip of a wave, 64 columns (one per lane)     widths 63, 64, 65; 130x70 has a strip of two columns
  eight rows in flight per column item                  blocks of 2 ry + 1 = 7 and 9 rows (ry = 3, 4), and the tails the heights leave
  blocks grouped until an item has 32 rows              2 ry + 1 = 31 (two blocks an item) and 33 (one): ry = 15 and 16 -- the one
    (kItemRows; there is no direct small-radius path)     threshold on the radius the kernels have; 14 and 17 are a step further out
  four wave items per workgroup                         1x1 (one item) .. 130x70
Radii: 0, 1, 2, 3, 4, 7, 8, 14..17, 31, 32, equal and unequal per axis, and 255 (beyond the image on both sides).
Blocks of 2 r + 1: heights and widths that are a multiple of it, one off it and neither, three blocks and more per axis (40 x 140 with
ry = 20: five blocks of 41 rows over 180 plane rows; 123 = 3 x 41 with its neighbours 122 and 124, as heights and as widths).
Odd widths put every other row on an 8-byte boundary only (the 16-byte loads fall back to 8-byte ones there)."""
import functools
import zlib

import numpy as np

import blur_cases
import morph_ref

SIZES = [(1, 1), (1, 37), (37, 1), (7, 5), (63, 9), (64, 8), (65, 7), (255, 2), (256, 2), (257, 3), (127, 4), (129, 3), (130, 70)]
RADII = [(0, 0), (1, 1), (2, 0), (0, 2), (3, 4), (4, 3), (7, 8), (8, 7), (15, 16), (16, 15), (14, 17), (17, 14), (31, 2), (2, 32), (32, 31)]
OPS = [morph_ref.ERODE, morph_ref.DILATE]
EDGES = [morph_ref.ZERO, morph_ref.CLAMP]
FLAGS = [0, morph_ref.STRAIGHT]
COMBOS = [(op, edge, flags) for op in OPS for edge in EDGES for flags in FLAGS]
POISON = blur_cases.POISON  # what dst holds before a call into a second image (a finite f16)

TIE_COLOUR = [0x0000, 0x8000, 0x3C00, 0xBC00, 0x3800, 0x7C00]  # +0, -0, 1, -1, 0.5, Inf
TIE_ALPHA = [0x0000, 0x8000, 0x3C00, 0xBC00, 0x3800]           # +0, -0, 1, -1 (a negative alpha), 0.5


def content(kind, w, h, seed):
    """(h, w, 4) uint16 f16 bit patterns: blur_cases.content's 'finite', 'unit', 'nonfinite' and 'never', and 'ties': few values, so
    that windows tie -- +0 and -0 side by side, a negative alpha, alpha 0 next to alpha 1, an Inf colour over alpha 0 (a NaN once
    premultiplied)."""
    if kind != "ties":
        return blur_cases.content(kind, w, h, seed)
    rng = np.random.default_rng(seed)
    bits = np.empty((h, w, 4), np.uint16)
    bits[..., :3] = rng.choice(np.array(TIE_COLOUR, np.uint16), (h, w, 3), p=[0.3, 0.3, 0.12, 0.12, 0.12, 0.04])
    bits[..., 3] = rng.choice(np.array(TIE_ALPHA, np.uint16), (h, w), p=[0.3, 0.2, 0.3, 0.1, 0.1])
    return bits


def _case(w, h, op, radius, edge, flags, rect=None, in_place=False, kind="finite"):
    name = "%dx%d_%s_r%d_%d_%s%s%s%s_%s" % (w, h, "dilate" if op else "erode", radius[0], radius[1], "clamp" if edge else "zero",
                                            "_straight" if flags else "", "" if rect is None else "_r%d_%d_%d_%d" % rect,
                                            "_inplace" if in_place else "", kind)
    return {"name": name, "w": w, "h": h, "op": op, "radius": radius, "edge": edge, "flags": flags, "rect": rect, "in_place": in_place, "kind": kind}


def _battery():
    out, n = [], 0
    for (w, h) in SIZES:
        for radius in RADII:  # two of the eight (op, edge, flags) each, in turn; in place and into a second image in turn
            for combo in (COMBOS[n % 8], COMBOS[(3 * n + 5) % 8]):
                out.append(_case(w, h, *((combo[0], radius) + combo[1:]), in_place=n % 2 == 1))
            n += 1
    for i, (op, edge, flags) in enumerate(COMBOS):  # radius 255: beyond the image on both sides
        out.append(_case(40, 24, op, (255, 255), edge, flags, in_place=i % 2 == 0))
    for i, (w, h, radius) in enumerate([(40, 140, (0, 20)), (40, 140, (20, 20)), (5, 123, (1, 20)), (5, 122, (0, 20)), (5, 124, (2, 20)),
                                        (123, 5, (20, 1)), (122, 5, (20, 0)), (124, 5, (20, 2)), (66, 41, (20, 20)), (66, 82, (3, 20))]):
        for j, (op, edge, flags) in enumerate(COMBOS):
            if (i + j) % 2 == 0:
                out.append(_case(w, h, op, radius, edge, flags, in_place=(i + j) % 4 == 0))
    # rectangles: interior, 1 x 1, touching two edges (the right and the bottom one; the left and the top one), at odd offsets
    for (w, h), rects in (((65, 33), [(9, 5, 40, 20), (31, 17, 1, 1), (20, 10, 45, 23), (0, 0, 33, 9)]),
                          ((130, 70), [(3, 1, 121, 61), (129, 69, 1, 1), (101, 51, 29, 19), (0, 0, 129, 9)])):
        for rect in rects:
            for i, (op, edge, flags) in enumerate(COMBOS):
                out.append(_case(w, h, op, (2, 7) if i % 2 else (7, 2), edge, flags, rect, in_place=i % 4 < 2))
            out.append(_case(w, h, morph_ref.DILATE, (0, 16), morph_ref.CLAMP, 0, rect, True))
            out.append(_case(w, h, morph_ref.ERODE, (16, 0), morph_ref.ZERO, 1, rect, True))
    for kind in ("unit", "nonfinite", "never", "ties"):
        for i, (op, edge, flags) in enumerate(COMBOS):
            out.append(_case(65, 33, op, (2, 7), edge, flags, None, False, kind))
            out.append(_case(65, 33, op, (1, 1), edge, flags, (20, 10, 45, 23), True, kind))
    return out


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def source(case):
    return content(case["kind"], case["w"], case["h"], seed=zlib.crc32(case["name"].encode()))


@functools.lru_cache(maxsize=None)
def expected(name, **variant):
    """What dst holds after the case's call, by tests/morph_ref.py (computed once per case and variant; do not modify the result)."""
    c = BY_NAME[name]
    src = source(c)
    before = src if c["in_place"] else np.full_like(src, POISON)
    out = morph_ref.morph(src, c["op"], c["radius"], c["edge"], c["flags"], c["rect"], before, **variant)
    out.setflags(write=False)
    return out
