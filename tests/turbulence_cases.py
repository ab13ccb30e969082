"""The battery jh_turbulence is held to (tests/test_gpu_turbulence.py) and the reference's sensitivity is measured on
(tests/test_turbulence_spec.py).  A case: name, the image's size, the rectangle, what dst held before ('poison' or 'never'), `desc`:
the keywords of Engine.turbulence (and of turbulence_ref.turbulence), and `inst`: which instantiation of the kernel
(jello_amd/csrc/kernels_turbulence.hip) the case runs -- kind/stitch.  Every image but those of the grid-stride cases is at most
130 x 37.

Sizes on each side of every boundary of the kernel:
  a workgroup's tile, 64 texels x 16 rows          widths 63 / 64 / 65 against heights 15 / 16 / 17, 130 x 33; 1 x 1, 1 x 5, 5 x 1
  a wave's strip, 4 rows                           heights 1, 3, 4, 5, 15, 17, 33 and rectangles of 21 and 17 rows at odd offsets
  the tile grid lies on dst's 128-byte lines       widths that are no multiple of 16 and rectangles at odd offsets
  the workgroups stride over the tiles             4 x 32 768 = 2 048 tiles and 4 x 32 769 = 2 049, on each side of the launcher's cap of 8
                                                   workgroups per CU x 256 CUs (its other cap, 2^31 - 1 tiles, is beyond any image)
Rectangles at odd offsets: dst outside its rectangle is POISON, which has to stay.  SEED_WITH_A_ZERO_GRADIENT was found by search on the
CPU (tests/test_turbulence_spec.py repeats the search's check): its tables hold G[1][164] = (+0, +0)."""
import functools
import zlib

import numpy as np

import turbulence_ref
from turbulence_ref import FRACTAL_NOISE, KIND_NAMES, TURBULENCE

POISON = 0x5A5A  # what dst holds before the call (a finite f16)
KINDS = (FRACTAL_NOISE, TURBULENCE)
TILE_SIZES = [(1, 1), (1, 5), (5, 1), (2, 4), (63, 15), (64, 15), (65, 15), (63, 16), (64, 16), (65, 16), (63, 17), (64, 17), (65, 17), (130, 33)]
OCTAVES = (0, 1, 2, 5, 16)
SEED_WITH_A_ZERO_GRADIENT = 346
SEEDS = (0, 1, -1, -2000000000, 2147483647, SEED_WITH_A_ZERO_GRADIENT)
GRID_SIZES = [(4, 32768), (4, 32769)]
FREQUENCIES = [(0.0, 0.05), (0.05, 0.0), (0.0, 0.0), (0.01, 0.01), (0.25, 0.25), (1.0, 1.0), (1.5, 1.5), (7.3, 7.3), (0.03, 0.11), (2.5, 0.02)]


def instantiation(desc):
    d = dict(turbulence_ref.DEFAULTS, **desc)
    return "%s/%d" % (KIND_NAMES[int(d["kind"])], int(d["stitch_tile"] is not None))


def _case(tag, size, desc, rect=None, prior="poison"):
    d = dict(turbulence_ref.DEFAULTS, **desc)
    name = "%s_%s_o%d_s%d_%dx%d%s%s%s_%08x" % (
        tag, KIND_NAMES[int(d["kind"])], d["octaves"], d["seed"], size[0], size[1], "" if rect is None else "_r%d_%d_%d_%d" % rect,
        "" if d["stitch_tile"] is None else "_stitch", "" if prior == "poison" else "_" + prior,
        zlib.crc32(repr(sorted((k, repr(v)) for k, v in desc.items())).encode()))
    return {"name": name, "size": size, "rect": rect, "prior": prior, "desc": desc, "inst": instantiation(desc)}


def _battery():
    out, n = [], 0

    def combo(size):  # every kind, stitch on and off, rotating octaves, seeds and frequencies
        nonlocal n
        n += 1
        d = dict(kind=KINDS[n % 2], octaves=OCTAVES[1 + n % 4] if n % 7 else 0, seed=SEEDS[n % 6], base_frequency=FREQUENCIES[3 + n % 7],
                 origin=((0.0, 0.0), (-3.5, 2.25), (100.0, -40.75))[n % 3])
        if (n // 2) % 2:
            d["stitch_tile"] = (1.0, -2.0, max(size[0] // 2, 1) + 0.5, max(size[1] // 2, 1))
        if d["octaves"] == 16:  # (the position range of 16 octaves: 32 768 cells)
            d["base_frequency"] = tuple(min(f, 1.5) for f in d["base_frequency"])
        return d

    # the kernel's tile and strip boundaries, with every instantiation
    for size in TILE_SIZES:
        for _ in range(4):
            out.append(_case("tile", size, combo(size)))
    # octaves x kinds x stitch
    for kind in KINDS:
        for octaves in OCTAVES:
            out.append(_case("oct", (45, 19), dict(kind=kind, octaves=octaves, seed=5, base_frequency=(0.07, 0.04), origin=(-9.25, 4.0))))
            out.append(_case("oct", (45, 19), dict(kind=kind, octaves=octaves, seed=5, base_frequency=(0.07, 0.04), origin=(-9.25, 4.0),
                                                   stitch_tile=(-9.0, 4.0, 30.0, 12.0))))
    # frequencies: 0 on one axis and on both, cells of 100 texels, every texel on a lattice point, cells smaller than a texel, unequal
    for kind in KINDS:
        for f in FREQUENCIES:
            out.append(_case("freq", (37, 11), dict(kind=kind, octaves=3, seed=2, base_frequency=f)))
            out.append(_case("freq", (37, 11), dict(kind=kind, octaves=2, seed=2, base_frequency=f, origin=(-0.5, -0.5))))  # (centres on integers)
    # origins: negative, fractional, large, and at the legality bound of their octave count (frequency 1: 2^30 - 1 and 32 767 cells)
    for kind in KINDS:
        for origin, octaves, f in (((-1000.25, -3.5), 4, (0.3, 0.3)), ((0.125, 0.875), 4, (0.3, 0.3)), ((1e6, -2e6), 4, (0.3, 0.3)),
                                   ((-50.0, -50.0), 5, (0.11, 0.13)), ((1073741823.0 - 37.0, -1073741824.0), 1, (1.0, 1.0)),
                                   ((32767.0 - 37.0, -32768.0), 16, (1.0, 1.0)), ((-20.0, -6.0), 16, (0.9, 1.1))):
            out.append(_case("origin", (37, 11), dict(kind=kind, octaves=octaves, seed=9, base_frequency=f, origin=origin)))
    # stitch: tile edges inside the image, a tile smaller than a cell, a wrap crossed in the first and in the last octave, negative tiles
    for kind in KINDS:
        for tile, f, octaves, origin in (((0.0, 0.0, 20.0, 7.0), (0.21, 0.4), 3, (0.0, 0.0)),      # edges inside a 50 x 19 image
                                         ((5.0, 3.0, 16.0, 8.0), (0.26, 0.3), 5, (0.0, 0.0)),
                                         ((0.0, 0.0, 30.0, 10.0), (0.004, 0.01), 4, (0.0, 0.0)),   # a tile smaller than a cell
                                         ((0.0, 0.0, 40.0, 15.0), (0.05, 0.1), 1, (0.0, 0.0)),     # the wrap crossed in the first octave
                                         ((0.0, 0.0, 49.9, 18.9), (0.02, 0.06), 5, (0.0, 0.0)),    # ... only in the last octaves
                                         ((-30.0, -12.0, 25.0, 9.0), (0.12, 0.35), 4, (-40.0, -15.0)),
                                         ((0.0, 0.0, 25.0, 9.0), (0.0, 0.35), 2, (0.0, 0.0)),
                                         ((2.0, 1.0, 8.0, 4.0), (1.5, 7.3), 2, (3.0, -1.0)),
                                         ((0.0, 0.0, 50.0, 19.0), (1.0, 1.0), 16, (0.0, 0.0))):
            out.append(_case("stitch", (50, 19), dict(kind=kind, octaves=octaves, seed=4, base_frequency=f, origin=origin, stitch_tile=tile)))
    # seeds
    for seed in SEEDS:
        for kind in KINDS:
            out.append(_case("seed", (40, 20), dict(kind=kind, octaves=2, seed=seed, base_frequency=(1.1, 0.9))))
            out.append(_case("seed", (40, 20), dict(kind=kind, octaves=2, seed=seed, base_frequency=(0.3, 0.2), stitch_tile=(0.0, 0.0, 20.0, 10.0))))
    # rectangles at odd offsets
    for kind in KINDS:
        for tile in (None, (5.0, 3.0, 33.0, 21.0)):
            d = dict(kind=kind, octaves=3, seed=8, base_frequency=(0.09, 0.06), origin=(12.5, -7.0), stitch_tile=tile)
            out.append(_case("rect", (49, 37), d, rect=(5, 3, 33, 21)))
            out.append(_case("rect", (77, 25), d, rect=(3, 5, 65, 17)))
    out.append(_case("rect", (49, 37), dict(kind=TURBULENCE, octaves=2, seed=1, base_frequency=(0.1, 0.1)), rect=(5, 3, 33, 21), prior="never"))
    out.append(_case("rect", (49, 37), dict(kind=FRACTAL_NOISE, octaves=2, seed=1, base_frequency=(0.1, 0.1)), rect=(7, 9, 1, 1), prior="never"))
    out.append(_case("rect", (49, 37), dict(kind=FRACTAL_NOISE, octaves=0, seed=1, base_frequency=(0.1, 0.1)), prior="never"))
    out.append(_case("rect", (33, 9), dict(kind=TURBULENCE, octaves=4, seed=1, base_frequency=(0.2, 0.1)), rect=(32, 8, 1, 1)))
    out.append(_case("rect", (33, 9), dict(kind=FRACTAL_NOISE, octaves=4, seed=1, base_frequency=(0.2, 0.1)), rect=(0, 0, 1, 9)))
    # the grid-stride loop, on each side of the launcher's cap
    for size in GRID_SIZES:
        out.append(_case("big", size, dict(kind=TURBULENCE, octaves=1, seed=3, base_frequency=(0.3, 0.013))))
        out.append(_case("big", size, dict(kind=FRACTAL_NOISE, octaves=2, seed=3, base_frequency=(0.3, 0.013), stitch_tile=(0.0, 0.0, 4.0, 1000.0))))
    seen, uniq = set(), []
    for c in out:
        if c["name"] not in seen:
            seen.add(c["name"])
            uniq.append(c)
    return uniq


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}


def before(case):
    """What dst holds before the call, or None for a never-written dst."""
    w, h = case["size"]
    return None if case["prior"] == "never" else np.full((h, w, 4), POISON, np.uint16)


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    w, h = c["size"]
    out = turbulence_ref.turbulence((h, w), c["rect"], before(c), **dict(variant), **c["desc"])
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/turbulence_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
