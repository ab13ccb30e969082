"""The battery jh_lut3d is held to tests/lut3d_ref.py on, byte for byte (tests/test_gpu_lut3d.py), and on which the reference is
told from its near misses (tests/test_lut3d_spec.py).

A case is a dict: name; `inst`, the instantiation it runs -- "staged" (the table in LDS, N <= 17) or "global" (gathered from memory;
for N <= 17 forced through jh_debug_lut3d_variant); n and `lut`, the table (lut_image); and either `values` (the source is VALUES or
TIES, into a second image) or the geometry: src_size, dst_size, rect, in_place.

VALUES  256 x 256: every f16 bit pattern once in each channel, decorrelated as in color_cases.py (its first 256 rows).
TIES    texels of the cell (0, 0, 0) of N = 3 whose fractions tie -- f_r == f_g, f_g == f_b, f_r == f_b, above and below the third,
        and all three equal -- and the six strict orders; the tables of TIE_TABLES hold a NaN at the vertices that only another
        order of the tied axes would read.
Tables  identity; random finite in [0, 1] with random alpha bits (alpha is ignored); "wild": negative, subnormal and above-1
        entries; "nonfinite": random with +-Inf and NaN at single vertices (which four vertices a texel touched shows as NaN).
Geometry  the smallest shapes where the pair walk can go wrong: 1 x 1, 1 x 5, 5 x 1; widths on each side of 512 and 1024 (a work
        item is 512 texels, a lane two) by heights 1..3; rectangles at odd x and odd width (first and last texels alone); src and dst
        of different sizes; in place and into a poisoned image, NaN around the source's rectangle; more items than the grid.
No case has more than 2^17 texels."""
import numpy as np

import color_cases
import lut3d_ref

POISON = color_cases.POISON
NAN_BITS = color_cases.NAN_BITS
STAGED_MAX = 17
SIZES = (2, 3, 4, 16, 17, 18, 33, 65)
INSTANTIATIONS = ("global", "staged")

VALUES = np.ascontiguousarray(color_cases.VALUES[:256])


def _f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).view(np.uint16)


# Per tie, the vertices (i, j, k) of the cell (0, 0, 0) that the rule's order never reads on a texel with that tie and another
# order of the tied axes would -- with weight zero, which a NaN shows:
#   r == g  above b: r, g, b reads (1,0,0), (1,1,0), not (0,1,0);  below b: b, r, g reads (0,0,1), (1,0,1), not (0,1,1)
#   g == b  above r: g, b, r reads (0,1,0), (0,1,1), not (0,0,1);  below r: r, g, b reads (1,0,0), (1,1,0), not (1,0,1)
#   r == b  above g: r, b, g reads (1,0,0), (1,0,1), not (0,0,1);  below g: g, r, b reads (0,1,0), (1,1,0), not (0,1,1)
#   all equal: r, g, b reads (1,0,0), (1,1,0) and none of the other four
TIE_TABLES = {"ties_rg": ((0, 1, 0), (0, 1, 1)), "ties_gb": ((0, 0, 1), (1, 0, 1)), "ties_rb": ((0, 0, 1), (0, 1, 1)),
              "ties_all": ((0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1))}


CONSTANT = (0.5, 0.25, 1.0)  # the colour of the "constant" tables


def lut_image(kind, n, seed=0):
    """The LUT image (n * n, n, 4) of a kind."""
    rng = np.random.default_rng(7000 + 131 * n + seed)
    if kind == "identity":
        return lut3d_ref.identity(n)
    if kind == "zeros":
        return np.zeros((n * n, n, 4), np.uint16)
    if kind == "constant":  # one colour of powers of two: every partial sum c (1 - f) is exact, so the colour comes back exactly
        out = np.empty((n * n, n, 4), np.uint16)
        out[...] = _f16(CONSTANT + (0.75,))
        return out
    out = np.empty((n * n, n, 4), np.uint16)
    out[..., :3] = _f16(rng.uniform(0.0, 1.0, (n * n, n, 3)))
    out[..., 3] = rng.integers(0, 65536, (n * n, n)).astype(np.uint16)  # any bits, NaN among them: alpha is ignored
    if kind == "random":
        return out
    if kind == "wild":
        pick = rng.integers(0, 4, (n * n, n, 3))
        neg = _f16(rng.uniform(-4.0, 0.0, pick.shape))
        sub = rng.integers(1, 0x400, pick.shape).astype(np.uint16) | (rng.integers(0, 2, pick.shape).astype(np.uint16) << 15)  # +- subnormals
        big = _f16(rng.uniform(1.0, 60000.0, pick.shape))
        out[..., :3] = np.where(pick == 0, neg, np.where(pick == 1, sub, np.where(pick == 2, big, out[..., :3])))
        return out
    if kind == "nonfinite":
        flat = out.reshape(-1, 4)
        count = max(3, n ** 3 // 9)
        where = rng.choice(n ** 3, size=min(count, n ** 3 - 1), replace=False)
        flat[where, rng.integers(0, 3, len(where))] = rng.choice(np.array([0x7C00, 0xFC00, 0x7E00, 0xFFFF], np.uint16), len(where))
        return out
    if kind in TIE_TABLES:
        assert n == 3
        cube = out.reshape(n, n, n, 4)  # [k, j, i]
        for di, dj, dk in TIE_TABLES[kind]:
            cube[dk, dj, di, :3] = 0x7E00
        return out
    raise ValueError(kind)


def ties_image():
    """(1, K, 4): texels of the cell (0, 0, 0) of N = 3 (value v: fraction 2 v, v < 0.5) -- every tie pattern and, next to each, the
    strict orders around it; alpha counts up."""
    a, b, c = 0.125, 0.25, 0.375
    rows = []
    for hi, lo in ((c, a), (b, a), (c, b)):
        rows += [(hi, hi, lo), (hi, lo, hi), (lo, hi, hi),   # a tie of the two largest: r == g, r == b, g == b
                 (lo, lo, hi), (lo, hi, lo), (hi, lo, lo)]   # a tie of the two smallest
    rows += [(a, a, a), (b, b, b), (c, c, c), (0.0, 0.0, 0.0)]  # all three equal
    rows += [(c, b, a), (c, a, b), (b, c, a), (a, c, b), (b, a, c), (a, b, c)]  # the six strict orders
    out = np.empty((1, len(rows), 4), np.uint16)
    out[0, :, :3] = _f16(rows)
    out[0, :, 3] = np.arange(len(rows), dtype=np.uint16) * 257
    return out


TIES = ties_image()


def geometry_source(size, seed):
    """Colour in [-0.1, 1.1] (both clamps take part), any alpha bits."""
    w, h = size
    rng = np.random.default_rng(seed)
    out = _f16(rng.uniform(-0.1, 1.1, (h, w, 4)))
    out[..., 3] = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    return out


def _geometries():
    out = []
    for w, h in ((1, 1), (1, 5), (5, 1)):
        out.append(dict(src_size=(w, h), dst_size=(w, h), rect=None))
    for w in (511, 512, 513, 1023, 1024, 1025):
        h = 1 + w % 3  # heights 1..3
        out.append(dict(src_size=(w, h), dst_size=(w, h), rect=None))                    # the whole image: even x, the image's pitch
        out.append(dict(src_size=(w + 9, h + 2), dst_size=(w + 9, h + 2), rect=(3, 1, w, h)))  # odd x; w + 9 and w differ in parity
        out.append(dict(src_size=(w + 4, h + 1), dst_size=(w + 7, h + 3), rect=(2, 1, w, h)))  # src and dst of different sizes and parities
    out.append(dict(src_size=(21, 9), dst_size=(40, 12), rect=(5, 2, 11, 5)))           # odd x, odd width, different sizes
    out.append(dict(src_size=(6, 2502), dst_size=(6, 2502), rect=(1, 1, 2, 2500)))      # 2 500 items: more than 8 x 256 workgroups
    return out


def _cases():
    cases = []
    for n in SIZES:
        for inst in INSTANTIATIONS:
            if inst == "staged" and n > STAGED_MAX:
                continue
            for kind in ("identity", "random", "wild", "nonfinite", "constant"):
                cases.append(dict(name="values_%s_n%d_%s" % (kind, n, inst), inst=inst, n=n, lut=kind, values="VALUES"))
    for inst in INSTANTIATIONS:
        for kind in sorted(TIE_TABLES):
            cases.append(dict(name="%s_n3_%s" % (kind, inst), inst=inst, n=3, lut=kind, values="TIES"))
    for inst, n in (("staged", 5), ("staged", 17), ("global", 18), ("global", 4)):
        for g, geo in enumerate(_geometries()):
            if n in (17, 4) and g % 3 != 1:  # (the second size of each instantiation: a third of the shapes)
                continue
            for in_place in (False, True):
                if in_place and geo["src_size"] != geo["dst_size"]:
                    continue
                cases.append(dict(geo, name="geometry_%d_n%d_%s_%s" % (g, n, inst, "in_place" if in_place else "second_image"), inst=inst, n=n,
                                  lut="random", in_place=in_place, seed=100 * g + n))
    return cases


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def inputs(case):
    """(src_bits, lut_bits, prior, rect): what the images hold before the call -- prior is dst's content (the source's for a call in
    place)."""
    lut = lut_image(case["lut"], case["n"])
    if "values" in case:
        src = VALUES if case["values"] == "VALUES" else TIES
        return src, lut, np.full_like(src, POISON), None
    content = geometry_source(case["src_size"], case["seed"])
    rect = case["rect"]
    src = content if rect is None else color_cases.surround(content, rect, NAN_BITS)
    if case["in_place"]:
        return src, lut, src, rect
    w, h = case["dst_size"]
    return src, lut, np.full((h, w, 4), POISON, np.uint16), rect


def expected(case, variant=None):
    """What dst holds after the call, by the reference (or one of its wrong variants)."""
    src, lut, prior, rect = inputs(case)
    x, y, w, h = lut3d_ref.resolve(src.shape, rect)
    out = prior.copy()
    out[y:y + h, x:x + w] = lut3d_ref.texels(src[y:y + h, x:x + w], lut, variant)
    return out
