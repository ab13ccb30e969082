"""The battery jh_lighting is held to (tests/test_gpu_lighting.py) and the reference's sensitivity is measured on
(tests/test_lighting_spec.py).  A case: name, the images' size, the rectangle, the alpha content, what dst held before ('poison' or
'never'), `desc`: the keywords of Engine.lighting (and of lighting_ref.lighting), and `inst`: which instantiation of the kernel
(jello_amd/csrc/kernels_lighting.hip) the case runs -- kind/light/tables, tables the bits of the power tables in use (1: the specular
exponent's, 2: the spot exponent's).  Every image but those of the grid-stride cases is at most 130 x 37.

Sizes on each side of every boundary of the kernel:
  the normal's nine cases                          1 x 1, 1 x 5, 5 x 1, 2 x 2, 3 x 3 (spans of 0, 1 and 2 on either axis)
  a workgroup's tile, 64 texels x 16 rows          widths 63 / 64 / 65 against heights 15 / 16 / 17, 130 x 33
  a wave's strip, 4 rows                           heights 1, 3, 5, 15, 17, 33 and rectangles of 21 and 17 rows at odd offsets
  the tile grid lies on dst's 128-byte lines       widths that are no multiple of 16 and rectangles at odd offsets
  the workgroups stride over the tiles             4 x 32 768 = 2 048 tiles and 4 x 32 769 = 2 049, on each side of the launcher's cap of 8
                                                   workgroups per CU x 256 CUs without tables; 4 x 28 672 and 4 x 28 673 on each side of
                                                   its cap of 7 per CU with one table; 4 x 16 384 and 4 x 16 385, 4 per CU with both
Rectangles at odd offsets: the source's alpha goes on outside the rectangle -- the IMAGE is the edge, so it shows in the normals of the
rectangle's border -- and dst outside its rectangle is POISON, which has to stay."""
import functools
import math
import zlib

import numpy as np

import lighting_ref
from lighting_ref import DIFFUSE, DISTANT, KIND_NAMES, LIGHT_NAMES, POINT, SPECULAR, SPOT

POISON = 0x5A5A  # what dst holds before the call (a finite f16)
KINDS = (DIFFUSE, SPECULAR)
LIGHTS = (DISTANT, POINT, SPOT)
CONTENTS = ("ramp", "disc", "random", "const", "subnormal", "zeros", "above1", "negative", "inf", "nan", "never")
TILE_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (63, 15), (64, 15), (65, 15), (63, 16), (64, 16), (65, 16), (63, 17), (64, 17), (65, 17), (130, 33)]
EXPONENTS = (1.0, 1.5, 20.0, 128.0)
GRID_SIZES = {0: [(4, 32768), (4, 32769)], 1: [(4, 28672), (4, 28673)], 2: [(4, 16384), (4, 16385)]}  # by the number of tables in use


def content(kind, w, h, seed):
    """(h, w, 4) uint16: an RGBA16F image whose ALPHA is the named content; the colour channels are random finite values (they are
    never read)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "ramp":
        a = (0.75 * xx + 0.5 * yy) / max(w + h, 1)
    elif kind == "disc":  # a disc with a soft edge: a blurred alpha mask
        r = np.hypot(xx - 0.45 * w, yy - 0.55 * h)
        a = 1.0 / (1.0 + np.exp((r - 0.3 * max(min(w, h), 2)) / 1.5))
    elif kind == "random":
        a = rng.random((h, w))
    elif kind == "const":
        a = np.full((h, w), 0.5)
    elif kind == "subnormal":
        a = rng.integers(0, 1024, (h, w)) * 2.0 ** -24
    elif kind == "zeros":
        a = np.where(rng.random((h, w)) < 0.5, 0.0, -0.0)
    elif kind == "above1":
        a = rng.random((h, w)) * 6.0
    elif kind == "negative":
        a = rng.random((h, w)) * 2.0 - 1.0
    elif kind in ("inf", "nan"):
        a = rng.random((h, w))
        a[rng.random((h, w)) < 0.08] = np.inf if kind == "inf" else np.nan
        if kind == "inf":
            a[rng.random((h, w)) < 0.04] = -np.inf
    else:  # never: what a never-written image reads as
        return np.zeros((h, w, 4), np.uint16)
    img = (rng.random((h, w, 4)) * 2.0 - 0.5).astype(np.float16)
    with np.errstate(all="ignore"):
        img[..., 3] = a.astype(np.float16)
    return img.view(np.uint16)


def light(which, size, variant="inside", exponent=1.0, cone=-1.0):
    """The light's keywords for an image of `size`."""
    w, h = size
    if which == DISTANT:
        az, el = {"inside": (35.0, 40.0), "low": (200.0, 3.0), "below": (10.0, -20.0), "up": (0.0, 90.0)}[variant]
        az, el = math.radians(az), math.radians(el)
        return dict(light=DISTANT, direction=(math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)))
    pos = {"inside": (0.4 * w + 0.25, 0.6 * h, 7.5), "outside": (-20.5, h + 30.0, 15.0), "far": (1e6, -1e6, 1e6), "below": (0.5 * w, 0.5 * h, -4.0),
           "surface": (float(w // 2) + 0.5, float(h // 2) + 0.5, 1.0)}[variant]  # 'surface': on a texel centre at Z = 1 (const alpha 0.5, surface_scale 2)
    if which == POINT:
        return dict(light=POINT, position=pos)
    return dict(light=SPOT, position=pos, points_at=(w / 3.0, h / 3.0, 0.0), spot_exponent=exponent, cone_cos=cone)


def instantiation(desc):
    d = dict(lighting_ref.DEFAULTS, **desc)
    return "%s/%s/%d" % (KIND_NAMES[int(d["kind"])], LIGHT_NAMES[int(d["light"])], lighting_ref.which(**desc))


def _case(tag, size, desc, rect=None, kind="random", prior="poison"):
    d = dict(lighting_ref.DEFAULTS, **desc)
    name = "%s_%s_%s_e%g_%g_c%g_ss%g_k%g_%dx%d%s_%s%s_%08x" % (
        tag, KIND_NAMES[int(d["kind"])], LIGHT_NAMES[int(d["light"])], d["specular_exponent"], d["spot_exponent"], d["cone_cos"], d["surface_scale"],
        d["constant"], size[0], size[1], "" if rect is None else "_r%d_%d_%d_%d" % rect, kind, "" if prior == "poison" else "_" + prior,
        zlib.crc32(repr(sorted((k, repr(v)) for k, v in desc.items())).encode()))
    return {"name": name, "size": size, "rect": rect, "kind": kind, "prior": prior, "desc": desc, "inst": instantiation(desc)}


def _filter(kind, e=1.0, ss=3.0, k=1.0, color=(1.0, 0.85, 0.6)):
    return dict(kind=kind, surface_scale=ss, constant=k, specular_exponent=e, color=color)


def _battery():
    out, n = [], 0

    def combo(size, tables=True):  # every kind x every light, rotating, with and without tables
        nonlocal n
        n += 1
        kind, which = KINDS[n % 2], LIGHTS[(n // 2) % 3]
        e = EXPONENTS[(n // 6) % 4] if tables else 1.0
        return dict(_filter(kind, e), **light(which, size, exponent=EXPONENTS[(n // 3) % 4] if tables else 1.0, cone=(-1.0, 0.6)[n % 2]))

    # the kernel's tile boundaries and the normal's nine cases, with every kind and light
    for size in TILE_SIZES:
        for _ in range(3):
            out.append(_case("tile", size, combo(size)))
    for size in TILE_SIZES[:5]:
        for kind in KINDS:
            for which in LIGHTS:
                out.append(_case("small", size, dict(_filter(kind, 20.0), **light(which, size, exponent=1.5)), kind="above1"))
    # every kind x light x exponent of each table, and both tables at once
    for kind in KINDS:
        for which in LIGHTS:
            for e in EXPONENTS:
                if kind == SPECULAR or e == 1.0:
                    out.append(_case("exp", (45, 19), dict(_filter(kind, e), **light(which, (45, 19))), kind="disc"))
                if which == SPOT:
                    out.append(_case("exp", (45, 19), dict(_filter(kind, 1.0), **light(which, (45, 19), exponent=e)), kind="disc"))
                    if kind == SPECULAR and e != 1.0:
                        out.append(_case("exp", (45, 19), dict(_filter(kind, e), **light(which, (45, 19), exponent=EXPONENTS[4 - EXPONENTS.index(e)])), kind="disc"))
    # rectangles at odd offsets
    for kind in KINDS:
        for which in LIGHTS:
            d = dict(_filter(kind, 20.0 if which != POINT else 1.0), **light(which, (49, 37), exponent=20.0 if kind == DIFFUSE else 1.0))
            out.append(_case("rect", (49, 37), d, rect=(5, 3, 33, 21)))
            out.append(_case("rect", (77, 25), d, rect=(3, 5, 65, 17), kind="disc"))
    out.append(_case("rect", (49, 37), dict(_filter(DIFFUSE), **light(DISTANT, (49, 37))), rect=(5, 3, 33, 21), prior="never"))
    out.append(_case("rect", (49, 37), dict(_filter(SPECULAR, 20.0), **light(POINT, (49, 37))), rect=(7, 9, 1, 1), prior="never"))
    out.append(_case("rect", (33, 9), dict(_filter(SPECULAR, 1.5), **light(SPOT, (33, 9), exponent=128.0)), rect=(32, 8, 1, 1)))
    out.append(_case("rect", (33, 9), dict(_filter(DIFFUSE), **light(POINT, (33, 9))), rect=(0, 0, 1, 9)))
    # surface_scale 0, negative and large; constant 0 and large
    for ss in (0.0, -0.0, -2.5, 1000.0):
        for kind in KINDS:
            out.append(_case("scale", (29, 13), dict(_filter(kind, 20.0, ss=ss), **light(POINT, (29, 13))), kind="disc"))
            out.append(_case("scale", (29, 13), dict(_filter(kind, 1.0, ss=ss), **light(DISTANT, (29, 13)))))
    for k in (0.0, 7.5):
        for kind in KINDS:
            out.append(_case("const", (29, 13), dict(_filter(kind, 1.5, k=k), **light(SPOT, (29, 13), exponent=20.0)), kind="disc"))
    out.append(_case("black", (21, 9), dict(_filter(DIFFUSE, color=(0.0, 0.0, 0.0)), **light(DISTANT, (21, 9)))))
    out.append(_case("black", (21, 9), dict(_filter(SPECULAR, 20.0, color=(0.0, 2.0, 0.0)), **light(POINT, (21, 9)))))
    # where the light is
    for kind in KINDS:
        for variant in ("inside", "outside", "far", "below"):
            out.append(_case("point_" + variant, (37, 21), dict(_filter(kind, 20.0), **light(POINT, (37, 21), variant)), kind="disc"))
            out.append(_case("spot_" + variant, (37, 21), dict(_filter(kind, 1.5), **light(SPOT, (37, 21), variant, exponent=20.0, cone=0.3)), kind="ramp"))
        out.append(_case("point_surface", (37, 21), dict(_filter(kind, 20.0, ss=2.0), **light(POINT, (37, 21), "surface")), kind="const"))
        out.append(_case("spot_surface", (37, 21), dict(_filter(kind, 1.0, ss=2.0), **light(SPOT, (37, 21), "surface", exponent=1.5)), kind="const"))
        for variant in ("low", "below", "up"):
            out.append(_case("distant_" + variant, (37, 21), dict(_filter(kind, 20.0), **light(DISTANT, (37, 21), variant)), kind="disc"))
    # the cone: none, a half space, a single direction, and edges that cross the tile
    for kind in KINDS:
        for cone in (-1.0, 0.0, 1.0, 0.9, 0.97):
            for e in (1.0, 20.0):
                out.append(_case("cone", (70, 20), dict(_filter(kind, 1.0), **light(SPOT, (70, 20), exponent=e, cone=cone)), kind="ramp"))
    # values
    for kind_name in CONTENTS:
        for kind in KINDS:
            for which in LIGHTS:
                d = dict(_filter(kind, 20.0 if which == DISTANT else 1.0), **light(which, (37, 11), exponent=1.5 if kind == DIFFUSE else 1.0, cone=0.2))
                out.append(_case("values", (37, 11), d, kind=kind_name, prior="never" if kind_name == "never" and which == POINT else "poison"))
    # the grid-stride loop, on each side of the launcher's cap
    for size in GRID_SIZES[0]:
        out.append(_case("big", size, dict(_filter(DIFFUSE), **light(POINT, size))))
    for size in GRID_SIZES[1]:
        out.append(_case("big", size, dict(_filter(SPECULAR, 128.0), **light(DISTANT, size))))
    for size in GRID_SIZES[2]:
        out.append(_case("big", size, dict(_filter(SPECULAR, 20.0), **light(SPOT, size, exponent=1.5, cone=0.1))))
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


def source(case):
    """The source image's bits: the content over the whole image, the rectangle's surroundings included."""
    w, h = case["size"]
    return content(case["kind"], w, h, _seed(case))


def before(case):
    """What dst holds before the call, or None for a never-written dst."""
    w, h = case["size"]
    return None if case["prior"] == "never" else np.full((h, w, 4), POISON, np.uint16)


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    out = lighting_ref.lighting(source(c), c["rect"], before(c), **dict(variant), **c["desc"])
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/lighting_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
