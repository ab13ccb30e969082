"""The battery jh_shadow is held to (tests/test_gpu_shadow.py) and the reference's sensitivity is measured on
(tests/test_shadow_spec.py).  A case: name, the image's size, the rectangle, what dst held before ('poison', 'finite', 'nan' or
'never'), `desc`: the keywords of shadow_ref.shadow (box, radius, sigma, color, matrix, flags), and `inst`: which instantiation of
the kernel (jello_amd/csrc/kernels_shadow.hip) the case runs -- round|sharp / store|over.  Every image but the grid-stride one is
at most 200 x 100.

Sizes on each side of every boundary of the kernel:
  a workgroup's tile, 64 texels x 16 rows     widths 63 / 64 / 65 against heights 15 / 16 / 17, 130 x 33; 1 x 1, 1 x 5, 5 x 1
  a wave's strip, 4 rows                      heights 1, 5, 15, 17, 33 and rectangles of 21 and 17 rows at odd offsets
  the tile grid lies on dst's 128-byte lines  widths that are no multiple of 16 and rectangles at odd offsets
  the workgroups stride over the tiles        4 x 32 769 = 2 049 tiles, more than the launcher's cap of 8 workgroups per CU x 256 CUs
Rectangles at odd offsets: dst outside its rectangle is POISON, which has to stay."""
import functools
import math

import numpy as np

import shadow_ref
from shadow_ref import IDENTITY, INVERT, OVER

POISON = 0x5A5A  # what dst holds before the call (a finite f16)
TILE_SIZES = [(1, 1), (1, 5), (5, 1), (63, 15), (64, 15), (65, 15), (63, 16), (64, 16), (65, 16), (63, 17), (64, 17), (65, 17), (130, 33)]
GRID_SIZE = (4, 32769)
INF, NAN = math.inf, math.nan
_C30, _S30 = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
MATRICES = {
    "id": IDENTITY,
    "half": (1.0, 0.0, 0.0, 1.0, 0.5, 0.5),
    "rot30": (_C30, _S30, -_S30, _C30, 14.0, -6.0),
    "flip": (-1.0, 0.0, 0.0, 1.0, 60.0, 0.0),
    "scale": (2.0, 0.0, 0.0, 0.5, -6.0, 4.0),
}
SIGMA = 2.0
# r / sigma just below and just above every threshold at which N changes (0.5: 4 -> 8, 1.5: 8 -> 16), sigma = 2
THRESHOLD_RADII = [(1.0, 4), (1.0000001, 8), (3.0, 8), (3.0000002, 16)]


def instantiation(desc):
    d = dict(shadow_ref.DEFAULTS, **desc)
    pl = shadow_ref.plan(d["box"], d["radius"], d["sigma"], d["matrix"], d["flags"])
    return "%s/%s" % ("round" if pl["radius"] > 0 else "sharp", "over" if d["flags"] & OVER else "store")


def _case(name, size, desc, rect=None, prior="poison"):
    return {"name": name, "size": size, "rect": rect, "prior": prior, "desc": desc, "inst": instantiation(desc)}


def _battery():
    out = []
    grey, tint = (0.0, 0.0, 0.0, 0.5), (0.1, 0.2, 0.05, 0.75)
    for n, (w, h) in enumerate(TILE_SIZES):  # every instantiation over the tile sizes, the box about the middle
        box = (w * 0.2, h * 0.25, w * 0.8 + 0.5, h * 0.75 + 0.25)
        r = (0.0, 2.5)[n % 2]
        flags = (0, OVER, INVERT, OVER | INVERT)[(n // 2) % 4]
        out.append(_case("tile_%dx%d" % (w, h), (w, h), dict(box=box, radius=r, sigma=1.5, color=tint, flags=flags)))
        out.append(_case("tile_%dx%d_other" % (w, h), (w, h), dict(box=box, radius=2.5 - r, sigma=0.75, color=grey, flags=flags ^ OVER)))
    for rect in ((3, 5, 41, 21), (17, 1, 70, 17), (1, 2, 1, 1), (64, 16, 13, 9)):  # rectangles at odd offsets, poison around them
        for flags in (0, OVER):
            out.append(_case("rect_%d_%d_%d_%d_f%d" % (rect + (flags,)), (97, 37), dict(box=(10.0, 6.0, 80.0, 30.0), radius=7.0, sigma=SIGMA, color=tint, flags=flags), rect))
    out.append(_case("grid", GRID_SIZE, dict(box=(-10.0, 100.0, 3.0, 32700.0), radius=1.5, sigma=1.0, color=grey)))
    # boxes
    for tag, box in (("subtexel", (20.3, 10.2, 20.6, 10.7)), ("outside", (300.0, 300.0, 340.0, 320.0)), ("covering", (-500.0, -500.0, 600.0, 600.0)),
                     ("empty_x", (20.0, 5.0, 20.0, 25.0)), ("empty_y", (5.0, 12.0, 60.0, 12.0))):
        for r in (0.0, 3.0):
            out.append(_case("box_%s_r%g" % (tag, r), (70, 33), dict(box=box, radius=r, sigma=1.0, color=tint, flags=0 if r else INVERT)))
    # radii: 0, a pill, a disc, above half the smaller side (clamped)
    for tag, box, r in (("sharp", (8.0, 6.0, 60.0, 28.0), 0.0), ("pill", (8.0, 6.0, 60.0, 28.0), 11.0), ("disc", (20.0, 4.0, 44.0, 28.0), 12.0),
                        ("clamped", (8.0, 6.0, 60.0, 28.0), 500.0)):
        out.append(_case("radius_" + tag, (70, 33), dict(box=box, radius=r, sigma=SIGMA, color=tint)))
        out.append(_case("radius_%s_over" % tag, (70, 33), dict(box=box, radius=r, sigma=SIGMA, color=tint, flags=OVER), prior="finite"))
    # sigmas: below 2^-8, 0.5, 8, and 64 on a 100 x 100 image
    for sigma, size in ((0.0, (70, 33)), (0.001, (70, 33)), (0.5, (70, 33)), (8.0, (70, 33)), (64.0, (100, 100))):
        for r in (0.0, 9.0):
            out.append(_case("sigma_%g_r%g" % (sigma, r), size, dict(box=(12.0, 7.0, 58.0, 27.0), radius=r, sigma=sigma, color=grey)))
    for r in (0.0, 3.0):  # texel centres 0.001 outside two edges and on the other two: what the floor of sigma decides
        out.append(_case("sigma_floor_edge_r%g" % r, (70, 33), dict(box=(12.501, 7.499, 58.5, 27.5), radius=r, sigma=0.0, color=grey)))
    for r, n in THRESHOLD_RADII:  # on each side of N's thresholds
        out.append(_case("steps_r%.7f_n%d" % (r, n), (70, 33), dict(box=(12.0, 5.0, 58.0, 29.0), radius=r, sigma=SIGMA, color=tint)))
    # a cap window that is empty for some waves of a tile and live for others: rows 0 .. 3 lie more than K sigma above the cap
    out.append(_case("window_partial", (64, 16), dict(box=(4.0, 7.0, 60.0, 40.0), radius=5.0, sigma=0.5, color=grey)))
    out.append(_case("window_partial_over", (64, 16), dict(box=(4.0, 7.0, 60.0, 40.0), radius=5.0, sigma=0.5, color=grey, flags=OVER), prior="finite"))
    for tag, m in MATRICES.items():
        for r in (0.0, 6.0):
            out.append(_case("matrix_%s_r%g" % (tag, r), (70, 40), dict(box=(10.0, 8.0, 50.0, 30.0), radius=r, sigma=1.25, color=tint, matrix=m)))
    for tag, color in (("alpha0", (0.3, 0.2, 0.1, 0.0)), ("above1", (3.0, 2.0, 0.5, 1.5)), ("inf", (INF, 0.2, 0.1, 0.5)), ("nan", (0.1, NAN, 0.1, 0.5)),
                       ("nan_alpha", (0.1, 0.2, 0.3, NAN)), ("negative", (-0.5, 0.2, 0.1, 0.5))):
        for flags in (0, OVER):
            out.append(_case("color_%s_f%d" % (tag, flags), (33, 17), dict(box=(6.0, 4.0, 27.0, 13.0), radius=3.0, sigma=1.0, color=color, flags=flags), prior="finite"))
    for prior in ("finite", "poison", "never", "nan"):  # OVER onto what dst can hold
        for flags in (OVER, OVER | INVERT):
            out.append(_case("over_%s_f%d" % (prior, flags), (40, 21), dict(box=(6.0, 4.0, 33.0, 16.0), radius=4.0, sigma=1.5, color=tint, flags=flags),
                             (2, 1, 35, 19) if prior == "never" else None, prior))
    out.append(_case("invert_never", (40, 21), dict(box=(6.0, 4.0, 33.0, 16.0), radius=0.0, sigma=1.5, color=tint, flags=INVERT), (2, 1, 35, 19), "never"))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}


def before(case):
    """What dst holds before the call, or None for a never-written dst."""
    w, h = case["size"]
    prior = case["prior"]
    if prior == "never":
        return None
    if prior == "poison":
        return np.full((h, w, 4), POISON, np.uint16)
    rng = np.random.default_rng(w * 1000 + h)
    bits = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16).view(np.uint16)
    if prior == "nan":
        bits[::3, ::5, 1] = 0x7E00
        bits[1::4, 2::7, 3] = 0x7C00
    return bits


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    w, h = c["size"]
    out = shadow_ref.shadow((h, w), c["rect"], before(c), **dict(variant), **c["desc"])
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/shadow_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
