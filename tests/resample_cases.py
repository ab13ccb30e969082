"""The battery jh_resample is held to (tests/test_gpu_resample.py) and the reference's sensitivity is measured on
(tests/test_resample_spec.py).  A case: name, filter, flags, the source image's size and rectangle, the destination image's size and
rectangle, the content kind, and what dst held before ('poison' or 'never').  Sources are at most 1100 x 48 texels.

Ratios, on either axis independently and with every filter: 1:1, 2:1, 3:2, 7:5, 16:1 (1040 -> 65 and 48 -> 3: the 96-tap window),
16 n - 1 : n, 1:3, 1 -> N (a single source texel) and N -> 1.
Sizes on each side of every boundary of the kernels (jello_amd/csrc/kernels_resample.hip):
  row item of a wave, 64 output columns (one per lane)       destination widths 1, 63, 64, 65
  column strip of a wave, 128 columns (64 lanes x 2)         destination widths 127, 128, 129
  four output rows in flight per column item                 destination heights 1, 3, 4, 5
  two row items per workgroup, four column items             1 x 1 (one item) .. 129 x 5 (15 row items, 4 column items)
  the row pass stages 128 source texels a step               spans of 127..130 texels and of 1120 follow from the ratios above
Rectangles at odd offsets inside images of odd width put every other row on an 8-byte boundary only (the 16-byte loads and stores
fall back to 8-byte ones there); there the source image outside its rectangle is NaN, which a window that left the rectangle would
carry into the result, and dst outside its rectangle is POISON, which has to stay."""
import functools

import numpy as np

import blur_cases
import resample_ref
from resample_ref import BOX, CATMULL_ROM, FILTER_NAMES, FILTERS, LANCZOS3, STRAIGHT, TRIANGLE

X_PAIRS = [(65, 65), (130, 65), (96, 64), (91, 65), (1040, 65), (143, 9), (21, 63), (1, 63), (16, 1)]
Y_PAIRS = [(5, 5), (8, 4), (6, 4), (7, 5), (48, 3), (47, 3), (3, 9), (1, 5), (16, 1)]
RATIO_NAMES = ["1:1", "2:1", "3:2", "7:5", "16:1", "16n-1:n", "1:3", "1:N", "N:1"]
ITEM_WIDTHS = [1, 63, 64, 65, 127, 128, 129]
ITEM_HEIGHTS = [1, 3, 4, 5]
KINDS = ["finite", "unit", "nonfinite", "never", "subnormal", "zeros", "alpha01"]
POISON = 0x5A5A  # what dst holds before the call (a finite f16)
NAN = 0x7E00     # what the source holds outside its rectangle


def content(kind, w, h, seed):
    """(h, w, 4) uint16 f16 bit patterns: the kinds of tests/blur_cases.py, and 'subnormal' (f16 subnormals of both signs, alpha
    included), 'zeros' (+0 and -0), 'alpha01' ('unit' colours under an alpha that is 0 or 1 in runs of a few texels: alpha 0 next
    to alpha 1)."""
    if kind in ("finite", "unit", "nonfinite", "never"):
        return blur_cases.content(kind, w, h, seed)
    rng = np.random.default_rng(seed)
    n = (h, w, 4)
    if kind == "subnormal":
        return (rng.integers(1, 0x0400, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16)
    if kind == "zeros":
        return (rng.integers(0, 2, n) << 15).astype(np.uint16)
    bits = (rng.random(n, dtype=np.float32) * 3.0 - 1.0).astype(np.float16).view(np.uint16)
    runs = np.repeat(rng.integers(0, 2, (h, (w + 2) // 3)), 3, axis=1)[:, :w]
    bits[..., 3] = np.where(runs == 1, 0x3C00, 0).astype(np.uint16)
    return bits


def _case(filt, flags, src_size, dst_size, src_rect=None, dst_rect=None, kind="finite", prior="poison"):
    name = "%s_%s_%dx%d%s_to_%dx%d%s_%s%s" % (
        FILTER_NAMES[filt], "straight" if flags else "premul", src_size[0], src_size[1], "" if src_rect is None else "_r%d_%d_%d_%d" % src_rect,
        dst_size[0], dst_size[1], "" if dst_rect is None else "_r%d_%d_%d_%d" % dst_rect, kind, "" if prior == "poison" else "_" + prior)
    return {"name": name, "filter": filt, "flags": flags, "src_size": src_size, "dst_size": dst_size, "src_rect": src_rect, "dst_rect": dst_rect,
            "kind": kind, "prior": prior}


def _battery():
    out, n = [], 0
    # every ratio on x with every filter, the y ratio rotating; then every ratio on y against two x ratios
    for filt in FILTERS:
        for i, (sw, dw) in enumerate(X_PAIRS):
            sh, dh = Y_PAIRS[(i + 1 + filt) % len(Y_PAIRS)]
            out.append(_case(filt, STRAIGHT if n % 2 else 0, (sw, sh), (dw, dh), kind="finite" if n % 3 else "unit"))
            n += 1
        for i, (sh, dh) in enumerate(Y_PAIRS):
            sw, dw = ((130, 65), (21, 63))[(i + filt) % 2]
            out.append(_case(filt, STRAIGHT if n % 2 else 0, (sw, sh), (dw, dh), kind="unit" if n % 3 else "finite"))
            n += 1
    # both flag settings on the 96-tap window of both axes at once
    for flags in (0, STRAIGHT):
        out.append(_case(LANCZOS3, flags, (1040, 48), (65, 3), kind="unit"))
    # the kernels' item sizes
    for filt in (TRIANGLE, CATMULL_ROM):
        for dw in ITEM_WIDTHS:
            out.append(_case(filt, 0, (dw * 3 // 2 + 1, 7), (dw, 5), kind="unit"))
        for dh in ITEM_HEIGHTS:
            out.append(_case(filt, STRAIGHT, (40, dh * 2 + 1), (33, dh)))
    out.append(_case(BOX, 0, (3, 2), (1, 1)))
    # rectangles at odd offsets inside images of odd and even widths: NaN around the source rectangle, POISON around dst's
    for filt in FILTERS:
        for flags in (0, STRAIGHT):
            out.append(_case(filt, flags, (151, 23), (99, 21), (3, 1, 141, 20), (5, 3, 71, 9), "unit"))
            out.append(_case(filt, flags, (64, 20), (140, 41), (1, 1, 31, 9), (7, 2, 129, 37), "finite"))
    out.append(_case(CATMULL_ROM, 0, (151, 23), (99, 21), (3, 1, 141, 20), (5, 3, 71, 9), "unit", "never"))
    out.append(_case(LANCZOS3, STRAIGHT, (33, 9), (20, 7), (32, 8, 1, 1), (19, 6, 1, 1), "finite"))
    # values
    for kind in KINDS:
        for flags in (0, STRAIGHT):
            out.append(_case(CATMULL_ROM, flags, (67, 11), (41, 7), kind=kind))
            out.append(_case(LANCZOS3, flags, (23, 5), (70, 13), kind=kind))
    for filt in (BOX, TRIANGLE, CATMULL_ROM):  # equal sizes: a copy under STRAIGHT
        out.append(_case(filt, STRAIGHT, (65, 5), (65, 5), kind="nonfinite"))
    out.append(_case(BOX, STRAIGHT, (130, 8), (65, 4), kind="unit"))  # the 2 x 2 mean
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
    seed = (w * 100003 + h * 9176 + case["dst_size"][0] * 131 + case["dst_size"][1] * 17 + case["filter"] * 5 + case["flags"]) & 0x7FFFFFFF
    img = np.full((h, w, 4), NAN, np.uint16)
    img[y:y + rh, x:x + rw] = content(case["kind"], rw, rh, seed)
    return img


def before(case):
    """What dst holds before the call, or None for a never-written dst."""
    w, h = case["dst_size"]
    return None if case["prior"] == "never" else np.full((h, w, 4), POISON, np.uint16)


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    w, h = c["dst_size"]
    out = resample_ref.resample(source(c), (h, w), c["filter"], c["flags"], c["src_rect"], c["dst_rect"], before(c), **dict(variant))
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/resample_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
