"""The battery jh_blur is held to (tests/test_gpu_blur.py) and the reference's sensitivity is measured on (tests/test_blur_spec.py).
A case: name, width, height, sigma (sx, sy), edge, rect (or None), in_place, content.  Images are at most 257 x 70 texels.

Sizes: 1x1, 1x37, 37x1, 7x5, 64x64, 65x33, 130x70, 257x3, and one on each side of every boundary of the kernels
(jello_amd/csrc/kernels_blur.hip):
  row segment of a wave, 256 outputs (64 lanes x 4)    widths 255, 256, 257 (257x3 above: a second segment of one texel)
  column strip of a wave, 128 columns (64 lanes x 2)   widths 127, 128, 129; 130x70 has a strip of one column pair
  eight output rows in flight per column item          heights 7, 8, 9
  four wave items per workgroup                        1x1 (one item) .. 65x33 (33 row items, 5 column items), 130x70 (18 column items)
  the row pass stages 128 texels a step                widths + 2 R on either side of 128 and 256 follow from the sigmas below
  a column item's rows that lie in all eight windows   need 2 R + 1 >= 8: R = 1 (none), R = 3 (none), R = 8 and 21 (some)
Odd widths put every other row on an 8-byte boundary only (the 16-byte loads and stores fall back to 8-byte ones there)."""
import functools

import numpy as np

import blur_ref

SIZES = [(1, 1), (1, 37), (37, 1), (7, 5), (64, 64), (65, 33), (130, 70), (257, 3),
         (255, 2), (256, 2), (127, 8), (128, 9), (129, 7)]
SIGMAS = [(0.0, 0.0), (0.0, 2.5), (2.5, 0.0), (0.3, 0.3), (1.0, 1.0), (2.5, 7.0), (7.0, 2.5)]
EDGES = [blur_ref.ZERO, blur_ref.CLAMP]
SPECIALS = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x3C00, 0xBC00]  # +-0, subnormals, 65504, +-1
NONFINITE = [0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01]


def content(kind, w, h, seed):
    """(h, w, 4) uint16 f16 bit patterns.  'finite': random finite patterns (every exponent, subnormals included, both signs) with a
    tenth of the texels' channels taken from SPECIALS; 'unit': values in [-1, 2) as a renderer leaves them; 'nonfinite': 'unit' with
    Inf and NaN sprinkled in; 'never': a source that was never written (all zero)."""
    rng = np.random.default_rng(seed)
    n = (h, w, 4)
    if kind == "never":
        return np.zeros(n, np.uint16)
    if kind == "finite":
        bits = (rng.integers(0, 0x7C00, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16)
    else:
        bits = (rng.random(n, dtype=np.float32) * 3.0 - 1.0).astype(np.float16).view(np.uint16)
    pick = rng.random(n) < 0.1
    bits[pick] = rng.choice(np.array(SPECIALS, np.uint16), n)[pick]
    if kind == "nonfinite":
        pick = rng.random(n) < 0.03
        bits[pick] = rng.choice(np.array(NONFINITE, np.uint16), n)[pick]
    return bits


def _case(w, h, sigma, edge, rect=None, in_place=False, kind="finite"):
    name = "%dx%d_s%g_%g_%s%s%s_%s" % (w, h, sigma[0], sigma[1], "clamp" if edge else "zero",
                                       "" if rect is None else "_r%d_%d_%d_%d" % rect, "_inplace" if in_place else "", kind)
    return {"name": name, "w": w, "h": h, "sigma": sigma, "edge": edge, "rect": rect, "in_place": in_place, "kind": kind}


def _battery():
    out, n = [], 0
    for (w, h) in SIZES:
        for sigma in SIGMAS:
            for edge in EDGES:
                out.append(_case(w, h, sigma, edge, in_place=n % 2 == 1))  # whole image, in place and into a second image in turn
                n += 1
    for edge in EDGES:  # R = 192: beyond the image on both sides
        out.append(_case(40, 24, (64.0, 64.0), edge))
        out.append(_case(40, 24, (64.0, 64.0), edge, in_place=True))
    # rectangles: interior, 1 x 1, touching two edges (the right and the bottom one; the left and the top one)
    for (w, h), rects in (((65, 33), [(9, 5, 40, 20), (31, 17, 1, 1), (20, 10, 45, 23), (0, 0, 33, 9)]),
                          ((130, 70), [(3, 2, 120, 60), (129, 69, 1, 1), (100, 50, 30, 20), (0, 0, 129, 9)])):
        for rect in rects:
            for edge in EDGES:
                for in_place in (False, True):
                    out.append(_case(w, h, (2.5, 7.0), edge, rect, in_place))
            out.append(_case(w, h, (0.0, 2.5), blur_ref.CLAMP, rect, True))  # (in place with no horizontal blur)
            out.append(_case(w, h, (2.5, 0.0), blur_ref.ZERO, rect, True))
    for kind in ("unit", "nonfinite", "never"):
        for edge in EDGES:
            out.append(_case(65, 33, (2.5, 7.0), edge, None, False, kind))
            out.append(_case(65, 33, (1.0, 1.0), edge, (20, 10, 45, 23), True, kind))
    return out


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
POISON = 0x5A5A  # what dst holds before a blur into a second image (a finite f16)


def source(case):
    return content(case["kind"], case["w"], case["h"], seed=case["w"] * 100003 + case["h"] * 9176 + int(case["sigma"][0] * 16) * 131 + int(case["sigma"][1] * 16) * 17 + case["edge"])


@functools.lru_cache(maxsize=None)
def expected(name, **variant):
    """What dst holds after the case's call, by tests/blur_ref.py (computed once per case and variant; do not modify the result)."""
    c = BY_NAME[name]
    src = source(c)
    before = src if c["in_place"] else np.full_like(src, POISON)
    out = blur_ref.blur(src, c["sigma"], c["edge"], c["rect"], before, **variant)
    out.setflags(write=False)
    return out
