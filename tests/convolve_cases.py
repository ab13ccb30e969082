"""The battery jh_convolve is held to (tests/test_gpu_convolve.py) and the reference's sensitivity is measured on
(tests/test_convolve_spec.py).  A case: name, the images' size, the weights (order_y, order_x) in applied order, the target, edge,
mode, bias, the rectangle, the content kind, what dst held before ('poison' or 'never'), and `inst`: which instantiation of the
kernel (jello_amd/csrc/kernels_convolve.hip) the case runs -- '3x3', '5x5' (compile-time orders) or 'general' (every other order).
Every image but the one of the grid-stride case is at most 130 x 37.

Sizes on each side of every boundary of the kernel:
  a workgroup's tile, 64 texels x 16 rows          1 x 1, 2 x 3, widths 63 / 64 / 65 against heights 15 / 16 / 17, 130 x 33
  a wave's strip, 4 rows                           heights 1, 3, 15, 17, 33 and rectangles of 21 and 17 rows at odd offsets
  the tile grid lies on dst's 128-byte lines       widths that are no multiple of 16 and rectangles at odd offsets
  the footprint in LDS, (64 + ox - 1) x (16 + oy - 1)   orders 1 x 1 .. 15 x 15, targets 0, centre and order - 1
  the workgroups stride over the tiles             3 x 33 000 = 2 063 tiles, above the launcher's cap of 8 per CU x 256 CUs, at 3 x 3
Images smaller than the kernel (n = 1, 2, 3 against order 15) make REPEAT and MIRROR wrap several times.  Rectangles at odd
offsets: the source outside the rectangle is NaN -- the IMAGE is the edge, so the NaN shows up in the result exactly where a window
reaches it -- and dst outside its rectangle is POISON, which has to stay."""
import functools
import zlib

import numpy as np

import convolve_ref
import warp_cases
from convolve_ref import CLAMP, EDGE_NAMES, EDGES, MIRROR, MODE_NAMES, MODES, PREMULTIPLIED, PRESERVE_ALPHA, REPEAT, STRAIGHT, ZERO

KINDS = warp_cases.KINDS  # finite, unit, nonfinite, never, subnormal, zeros, alpha01, negalpha, infalpha0
POISON = 0x5A5A  # what dst holds before the call (a finite f16)
NAN = 0x7E00     # what the source holds outside the rectangle
ORDERS = [(1, 1), (2, 2), (3, 3), (5, 5), (3, 5), (5, 3), (4, 4), (7, 7), (1, 15), (15, 1), (15, 15)]
TILE_SIZES = [(1, 1), (2, 3), (63, 15), (64, 15), (65, 15), (63, 16), (64, 16), (65, 16), (63, 17), (64, 17), (65, 17), (130, 33)]
BIASES = [0.0, -0.0, 0.5, -0.25]
BIG = (3, 33000)
content = warp_cases.content


def instantiation(order):
    return {(3, 3): "3x3", (5, 5): "5x5"}.get(tuple(order), "general")


def kernel(order, seed, style="mixed"):
    """(order_y, order_x) float32 weights.  'mixed': random in [-1, 1) -- negative lobes --, every fourth weight an exact zero (of
    either sign) and, from four taps on, one weight a binary32 subnormal; 'unit': positive, summing to about 1; 'shift': a single 1."""
    ox, oy = order
    rng = np.random.default_rng(seed)
    if style == "shift":
        w = np.zeros(ox * oy, np.float32)
        w[rng.integers(0, ox * oy)] = 1.0
        return w.reshape(oy, ox)
    if style == "unit":
        w = rng.random(ox * oy) + 0.25
        return (w / w.sum()).astype(np.float32).reshape(oy, ox)
    w = (rng.random(ox * oy) * 2.0 - 1.0).astype(np.float32)
    if ox * oy >= 2:
        w[rng.permutation(ox * oy)[:max(1, ox * oy // 4)]] = np.float32(0.0)
        w[rng.integers(0, ox * oy)] = np.float32(-0.0)
    if ox * oy >= 4:
        w[rng.integers(0, ox * oy)] = np.float32(1e-41)
    return w.reshape(oy, ox)


def _case(tag, size, order, target, edge, mode, bias=0.0, rect=None, kind="finite", prior="poison", style="mixed"):
    tx, ty = (order[0] // 2, order[1] // 2) if target is None else target
    name = "%s_%dx%d_t%d_%d_%s_%s_b%s_%dx%d%s_%s%s%s" % (
        tag, order[0], order[1], tx, ty, EDGE_NAMES[edge], MODE_NAMES[mode], repr(float(bias)), size[0], size[1],
        "" if rect is None else "_r%d_%d_%d_%d" % rect, kind, "" if style == "mixed" else "_" + style, "" if prior == "poison" else "_" + prior)
    return {"name": name, "size": size, "order": tuple(order), "target": (tx, ty), "edge": edge, "mode": mode, "bias": float(bias),
            "rect": rect, "kind": kind, "prior": prior, "style": style, "inst": instantiation(order)}


def _battery():
    out, n = [], 0

    def combo():  # every edge x every mode, rotating
        nonlocal n
        n += 1
        return EDGES[n % 4], MODES[(n // 4) % 3]

    # the kernel's tile boundaries, with every instantiation
    for size in TILE_SIZES:
        for order in ((3, 3), (5, 5), (4, 4)):
            e, m = combo()
            out.append(_case("tile", size, order, None, e, m, kind="unit"))
    # every order with its target at 0, at the centre and at order - 1
    for order in ORDERS:
        for target in ((0, 0), None, (order[0] - 1, order[1] - 1)):
            e, m = combo()
            out.append(_case("order", (37, 21), order, target, e, m, bias=BIASES[n % 4], kind="unit"))
    out.append(_case("order", (67, 19), (15, 15), (14, 0), MIRROR, STRAIGHT, kind="finite"))
    out.append(_case("order", (67, 19), (7, 2), (0, 1), REPEAT, PREMULTIPLIED, kind="unit"))
    # every edge with every mode, on every instantiation
    for order in ((3, 3), (5, 5), (7, 7)):
        for edge in EDGES:
            for mode in MODES:
                out.append(_case("edge", (45, 19), order, None, edge, mode, kind="unit"))
    # images smaller than the kernel
    for side in (1, 2, 3):
        for edge in EDGES:
            _, m = combo()
            out.append(_case("small", (side, side), (15, 15), None, edge, m, kind="unit"))
            out.append(_case("small", (side, 4 - side), (5, 5), (0, 4), edge, m, kind="finite"))
            out.append(_case("small", (4 - side, side), (3, 3), (2, 0), edge, m, kind="finite"))
    # rectangles at odd offsets, NaN around them in the source
    for order in ((3, 3), (5, 5), (7, 7)):
        for edge in EDGES:
            _, m = combo()
            out.append(_case("rect", (49, 37), order, None, edge, m, rect=(5, 3, 33, 21), kind="unit"))
            out.append(_case("rect", (77, 25), order, (0, order[1] - 1), edge, m, bias=0.5, rect=(3, 5, 65, 17), kind="finite"))
    out.append(_case("rect", (49, 37), (3, 3), None, ZERO, PREMULTIPLIED, rect=(5, 3, 33, 21), kind="unit", prior="never"))
    out.append(_case("rect", (49, 37), (6, 6), None, CLAMP, PRESERVE_ALPHA, rect=(7, 9, 1, 1), kind="unit", prior="never"))
    out.append(_case("rect", (33, 9), (5, 5), None, MIRROR, STRAIGHT, rect=(32, 8, 1, 1), kind="finite"))
    # the bias
    for bias in BIASES:
        for mode in MODES:
            for order in ((3, 3), (4, 4)):
                out.append(_case("bias", (29, 13), order, None, CLAMP, mode, bias=bias, kind="negalpha" if mode == PREMULTIPLIED else "finite"))
    # values
    for kind in KINDS:
        for mode in MODES:
            out.append(_case("values", (37, 11), (3, 3), None, ZERO, mode, bias=0.0, kind=kind))
            out.append(_case("values", (23, 7), (4, 3), None, MIRROR, mode, bias=-0.25, kind=kind))
            out.append(_case("values", (23, 7), (5, 5), None, REPEAT, mode, bias=0.0, kind=kind))
    # the consequences the header states: the identity, a translation, a constant under a normalised kernel
    for edge in EDGES:
        out.append(_case("identity", (21, 9), (1, 1), None, edge, STRAIGHT, kind="subnormal", style="shift"))
        out.append(_case("shift", (21, 9), (5, 3), None, edge, STRAIGHT, kind="finite", style="shift"))
        out.append(_case("unit", (21, 9), (5, 5), None, edge, PREMULTIPLIED, kind="alpha01", style="unit"))
    # the grid-stride loop
    out.append(_case("big", BIG, (3, 3), None, MIRROR, PREMULTIPLIED, bias=0.5, kind="unit"))
    seen, uniq = set(), []
    for c in out:
        if c["name"] not in seen:
            seen.add(c["name"])
            uniq.append(c)
    return uniq


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}


def _seed(case):
    return zlib.crc32(case["name"].encode()) & 0x7FFFFFFF


def weights(case):
    return kernel(case["order"], _seed(case) ^ 0x5555, case["style"])


def rect_of(case):
    (w, h), r = case["size"], case["rect"]
    return (0, 0, w, h) if r is None else r


def source(case):
    """The source image's bits: the content inside the rectangle, NaN around it."""
    (w, h), (x, y, rw, rh) = case["size"], rect_of(case)
    img = np.full((h, w, 4), NAN, np.uint16)
    img[y:y + rh, x:x + rw] = content(case["kind"], rw, rh, _seed(case))
    return img


def before(case):
    """What dst holds before the call, or None for a never-written dst."""
    w, h = case["size"]
    return None if case["prior"] == "never" else np.full((h, w, 4), POISON, np.uint16)


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    out = convolve_ref.convolve(source(c), weights(c), c["target"], c["edge"], c["mode"], c["bias"], c["rect"], before(c), **dict(variant))
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/convolve_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
