"""The battery jh_perspective is held to (tests/test_gpu_perspective.py) and the reference's sensitivity is measured on
(tests/test_perspective_spec.py).  A case: name, the source image's size and rectangle, the destination image's size and rectangle,
the matrix (nine entries, source rectangle -> destination image), filter, edge, flags, the content kind, what dst held before
('poison' or 'never'), `inst` = (filter, edge, straight), the instantiation of jh_perspective's kernel it runs, and for the affine cases whose
inverse is dyadic `affine`, the six entries Engine.warp takes.  Every image but the one of the grid-stride case is at most 128 on a
side.

Sizes on each side of every boundary of the kernel (jello_amd/csrc/warp_taps.h): a tile's row of 16 texels (widths 15, 16,
17, 31, 32, 33), a wave's 4 rows and a workgroup's 16 (heights 3, 4, 5, 15, 16, 17), 1 x 1, 1 x 5 and 5 x 1, rectangles at odd offsets
(the tile grid lies on dst's 128-byte lines, so the phase differs from row to row), and warp_cases.BIG's 1040 x 520 = 2 178 tiles,
above the launcher's cap of 8 per CU x 256 CUs.  The source outside its rectangle is NaN and dst outside its rectangle POISON.

from_inverse(N) builds a matrix whose plan is N times a power of two exactly: the forward matrix is the adjugate of N, and the
adjugate of that is det(N) N.  With small dyadic N the horizon, den = N's last row, sits exactly where the case wants it.  tuned()
searches one entry of a matrix, by bisection in the reference, until a chosen texel's U has the wanted low 32 bits; flipped() goes on
to the binary64 values next to such a step until the rule and a one-ULP near miss of it (an fma, a division, a truncation) put U on
different sides of a texel boundary; nudged() moves one entry by one ULP off a den that is exactly 0."""
import functools
import math
from fractions import Fraction

import numpy as np

import perspective_ref
import warp_cases
from warp_cases import KINDS, NAN, POISON, content  # noqa: F401
from warp_ref import BICUBIC, BILINEAR, CLAMP, EDGE_NAMES, EDGES, FILTER_NAMES, FILTERS, MIRROR, NEAREST, REPEAT, STRAIGHT, ZERO

WIDTHS = [15, 16, 17, 31, 32, 33]
HEIGHTS = [3, 4, 5, 15, 16, 17]
BIG = warp_cases.BIG
KEYSTONE = (1.1, 0.05, 1e-3, -0.08, 1.05, 5e-4, 2.25, 1.5, 1.0)  # a mild one: p = 1e-3


def affine(m6):
    return perspective_ref.affine(m6)


def product(a, b):
    """The matrix product a b of two column-major matrices, in binary64."""
    A, B = np.array(a).reshape(3, 3).T, np.array(b).reshape(3, 3).T
    return tuple(float(v) for v in (A @ B).T.reshape(-1))


def from_inverse(N):
    """The column-major matrix whose adjugate is det(N) N: the adjugate of the row-major 3 x 3 N, exact (asserted)."""
    n = [[Fraction(v) for v in row] for row in N]

    def cof(r, c):
        (r0, r1), (c0, c1) = [i for i in range(3) if i != r], [i for i in range(3) if i != c]
        return (n[r0][c0] * n[r1][c1] - n[r0][c1] * n[r1][c0]) * (-1) ** (r + c)

    M = [[cof(c, r) for c in range(3)] for r in range(3)]  # adj = the transposed cofactors
    out = tuple(float(M[r][c]) for c in range(3) for r in range(3))
    assert all(Fraction(out[3 * c + r]) == M[r][c] for c in range(3) for r in range(3))
    return out


def position_of(matrix, X, Y):
    U, V, void = perspective_ref.positions(perspective_ref.plan(matrix), (X, Y, 1, 1))
    return int(U[0, 0]), int(V[0, 0]), bool(void[0, 0])


@functools.lru_cache(maxsize=None)
def tuned(matrix, entry, X, Y, low32):
    """`matrix` with matrix[entry] moved, by bisection in the reference, so that U of destination texel (X, Y) has the low 32 bits
    `low32` (the nearest such U to where it was)."""
    def at(v):
        m = list(matrix)
        m[entry] = v
        return position_of(tuple(m), X, Y)[0]

    u0 = at(matrix[entry])
    goal = ((u0 >> 32) << 32) + low32
    lo, hi = matrix[entry] - 2.0, matrix[entry] + 2.0
    rising = at(hi) > at(lo)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        u = at(mid)
        if u == goal:
            m = list(matrix)
            m[entry] = mid
            return tuple(m)
        if (u < goal) == rising:
            lo = mid
        else:
            hi = mid
    raise AssertionError("tuned: no entry gives that position")


@functools.lru_cache(maxsize=None)
def flipped(matrix, entry, variant, src_size=(23, 19), size=(25, 21)):
    """`matrix` with matrix[entry] moved to where U of a destination texel steps onto a multiple of 2^32, and among the binary64
    values next to that step one at which the rule puts U on the multiple and the near miss `variant` (a keyword of
    perspective_ref.positions) one below it, or the other way round: NEAREST then reads two different texels.  The first texel of
    a fixed walk over a destination of `size` at which the two part."""
    for Y in range(2, size[1] - 1, 3):
        for X in range(2, size[0] - 1, 3):
            m = _flipped_at(matrix, entry, X, Y, variant, src_size)
            if m is not None:
                return m
    raise AssertionError("flipped: the near miss %s never parts from the rule here" % variant)


def _flipped_at(matrix, entry, X, Y, variant, src_size):
    def at(v, **kw):
        m = list(matrix)
        m[entry] = v
        U, V, _ = perspective_ref.positions(perspective_ref.plan(tuple(m)), (X, Y, 1, 1), **kw)
        inside.append(0 <= (int(U[0, 0]) >> 32) < src_size[0] and 0 <= (int(V[0, 0]) >> 32) < src_size[1])
        return int(U[0, 0])

    inside = []  # (the two texels have to lie inside the source, or the edge mode may make them one)

    goal = (at(matrix[entry]) >> 32) << 32
    lo, hi = matrix[entry] - 2.0, matrix[entry] + 2.0
    if at(lo) > at(hi):
        lo, hi = hi, lo  # U rises from lo to hi
    while math.nextafter(lo, hi) != hi:  # U(lo) < goal <= U(hi)
        mid = 0.5 * (lo + hi)
        if at(mid) < goal:
            lo = mid
        else:
            hi = mid
    for toward in (lo + (lo - hi) * 1e6, hi + (hi - lo) * 1e6):
        v = hi
        for _ in range(48):
            a, b = at(v), at(v, **{variant: True})
            if (a >> 32) != (b >> 32) and abs(a - b) < 1 << 20 and inside[-1] and inside[-2]:
                m = list(matrix)
                m[entry] = v
                return tuple(m)
            v = math.nextafter(v, toward)
    return None


def den_of(matrix, X, Y):
    """den of destination texel (X, Y) in the reference (Python floats: one rounding per operation)."""
    G = perspective_ref.plan(matrix)
    return ((G[6] * (X + 0.5)) + (G[7] * (Y + 0.5))) + G[8]


@functools.lru_cache(maxsize=None)
def nudged(matrix, X, Y, sign):
    """`matrix`, whose den is exactly 0 at texel (X, Y), with one entry moved by one ULP so that den there is within a few ULPs of
    its terms above 0 (sign > 0) or below 0: the first such entry and direction, found in the reference."""
    assert den_of(matrix, X, Y) == 0.0
    for entry in (8, 7, 5, 4):
        for toward in (math.inf, -math.inf):
            m = list(matrix)
            m[entry] = math.nextafter(m[entry], toward)
            d = den_of(tuple(m), X, Y)
            if d != 0.0 and abs(d) < 2.0 ** -45 and (d > 0.0) == (sign > 0):
                return tuple(m)
    raise AssertionError("nudged: no entry gives that sign")


def _case(tag, matrix, filt, edge, flags, src_size, dst_size, src_rect=None, dst_rect=None, kind="finite", prior="poison", m6=None):
    name = "%s_%s_%s_%s_%dx%d%s_to_%dx%d%s_%s%s" % (
        tag, FILTER_NAMES[filt], EDGE_NAMES[edge], "straight" if flags else "premul", src_size[0], src_size[1],
        "" if src_rect is None else "_r%d_%d_%d_%d" % src_rect, dst_size[0], dst_size[1], "" if dst_rect is None else "_r%d_%d_%d_%d" % dst_rect,
        kind, "" if prior == "poison" else "_" + prior)
    return {"name": name, "matrix": tuple(float(v) for v in matrix), "filter": filt, "edge": edge, "flags": flags, "src_size": src_size,
            "dst_size": dst_size, "src_rect": src_rect, "dst_rect": dst_rect, "kind": kind, "prior": prior, "inst": (filt, edge, bool(flags)),
            "affine": None if m6 is None else tuple(float(v) for v in m6)}


# N's rows: u's numerator, v's numerator, den -- each (coefficient of x', of y', constant)
def _horizon(den_row, shift=(0.0, 0.0)):
    return from_inverse(((1.0, 0.0, shift[0]), (0.0, 1.0, shift[1]), den_row))


# den = 2^-1033 everywhere, so q = 1 / den overflows: u = n_u Inf -- the clamp, or at X = 6, where n_u = 0, a NaN: void
Q_INF = (2.0 ** -500, 0.0, 0.0, 0.0, 2.0 ** -500, 0.0, 6.5 * 2.0 ** 530, 0.0, 2.0 ** 530)


def _battery():
    out, n = [], 0
    S, D = (41, 29), (47, 33)

    def combos():  # every filter x every edge x both operand modes, rotating
        nonlocal n
        n += 1
        return FILTERS[n % 3], EDGES[(n // 3) % 4], STRAIGHT if (n // 12) % 2 else 0

    # every filter x every edge x both operand modes under the mild keystone, and mirrored (det < 0)
    mirrored = product(KEYSTONE, affine((-1.0, 0.0, 0.0, 1.0, 41.0, 0.0)))
    for filt in FILTERS:
        for edge in EDGES:
            for flags in (0, STRAIGHT):
                out.append(_case("keystone", KEYSTONE, filt, edge, flags, S, D, kind="unit"))
            out.append(_case("mirrored", mirrored, filt, edge, STRAIGHT if (filt + edge) % 2 else 0, S, D, kind="finite"))
    # the kernel's tile boundaries
    for dw in WIDTHS:
        f, e, fl = combos()
        out.append(_case("tilew", KEYSTONE, f, e, fl, (19, 7), (dw, 5), kind="unit"))
    for dh in HEIGHTS:
        f, e, fl = combos()
        out.append(_case("tileh", KEYSTONE, f, e, fl, (9, 21), (17, dh)))
    for filt in FILTERS:
        out.append(_case("one", KEYSTONE, filt, CLAMP, 0, (3, 2), (1, 1)))
        out.append(_case("row", KEYSTONE, filt, MIRROR, STRAIGHT, (20, 3), (5, 1)))
        out.append(_case("col", KEYSTONE, filt, REPEAT, 0, (3, 20), (1, 5)))
    # rectangles at odd offsets inside images of odd and even widths: NaN around the source's, POISON around the destination's
    for filt in FILTERS:
        for edge in EDGES:
            flags = STRAIGHT if (filt + edge) % 2 else 0
            out.append(_case("rect", KEYSTONE, filt, edge, flags, (45, 29), (49, 37), (3, 5, 31, 19), (5, 3, 33, 21), "unit"))
            out.append(_case("rect", product(affine((1.5, 0.25, -0.25, 1.5, 3.0, -2.0)), KEYSTONE), filt, edge, flags, (36, 20), (64, 40), (1, 1, 21, 9),
                             (7, 1, 39, 35), "finite"))
    out.append(_case("rect", KEYSTONE, BICUBIC, ZERO, 0, (45, 29), (49, 37), (3, 5, 31, 19), (5, 3, 33, 21), "unit", "never"))
    out.append(_case("rect", affine(warp_cases.translate(18.5, 35.5)), BILINEAR, ZERO, STRAIGHT, (33, 9), (20, 37), (32, 8, 1, 1), (19, 36, 1, 1), "finite"))
    # the grid-stride loop
    out.append(_case("big", product((1.0, 0.0, 1e-4, 0.0, 1.0, 5e-5, 0.25, 0.5, 1.0), affine(warp_cases.scale(2))), NEAREST, ZERO, 0, BIG[1], BIG[0], kind="unit"))
    # affine matrices whose inverse is dyadic, as 3 x 3: the results are Engine.warp's bit for bit
    for filt in FILTERS:
        for edge in (ZERO, REPEAT):
            out.append(_case("identity", perspective_ref.IDENTITY, filt, edge, STRAIGHT, S, S, m6=warp_cases.translate(0, 0)))
            for t in ((3, 2), (-2, -5), (0.5, 0.5), (-0.5, 1.5), (-7.5, 0.0)):
                out.append(_case("t%g_%g" % t, affine(warp_cases.translate(*t)), filt, edge, 0, S, D, kind="unit", m6=warp_cases.translate(*t)))
        for k in range(8):
            w, h = S
            m6 = warp_cases.octant(k, w, h)
            out.append(_case(warp_cases.OCTANT_NAMES[k], affine(m6), filt, EDGES[k % 4], STRAIGHT, S, S if k < 4 else (h, w), m6=m6))
        out.append(_case("up2", affine(warp_cases.scale(2)), filt, CLAMP, 0, (32, 24), (64, 48), kind="unit", m6=warp_cases.scale(2)))
    # U just below, at and just above a multiple of 2^32 and fractions 0x0000 and 0xffff: dyadic translations, then keystones tuned
    # in the reference
    eps = 2.0 ** -32
    for e in (-0.5, -0.5 + eps, -0.5 - eps):
        out.append(_case("edge%+.10f" % e, affine(warp_cases.translate(e, e)), NEAREST, REPEAT, STRAIGHT, (23, 9), (25, 11), m6=warp_cases.translate(e, e)))
    for tag, low in (("below", 0xFFFFFFFF), ("at", 0), ("above", 1)):
        out.append(_case("tuned_" + tag, tuned(KEYSTONE, 6, 11, 7, low), NEAREST, ZERO if low else REPEAT, STRAIGHT, (23, 19), (25, 21)))
    # where a one-ULP near miss of the position (an fma, a division, a truncation) lands on the other side of a texel boundary
    for variant in ("fused", "divide", "trunc"):
        out.append(_case("flip_" + variant, flipped(KEYSTONE, 6, variant), NEAREST, CLAMP, STRAIGHT, (23, 19), (25, 21)))
    for filt in (BILINEAR, BICUBIC):
        for tag, low in (("frac0000", 0x80000000), ("fracffff", 0x7FFFFFFF), ("frac0000hi", 0x8000FFFF)):
            out.append(_case("tuned_" + tag, tuned(KEYSTONE, 6, 11, 7, low), filt, CLAMP if filt == BILINEAR else MIRROR, STRAIGHT, (23, 19), (25, 21)))
    # the horizon: along a wave's tile edge (y' = 4), along a workgroup's (y' = 16), diagonal inside tiles, and through texel centres
    # (den exactly 0 on the row Y = 6: 13 - 2 y'); the rows above it are in front
    for tag, row in (("edge4", (0.0, -1.0, 4.0)), ("edge16", (0.0, -1.0, 16.0)), ("diagonal", (-0.5, -1.0, 20.0)), ("centres", (0.0, -2.0, 13.0)),
                     ("column16", (-1.0, 0.0, 16.0))):
        for filt in FILTERS:
            f, e, fl = combos()
            out.append(_case("horizon_" + tag, _horizon(tuple(v / 8.0 for v in row), (-3.0, 2.0)), filt, e, fl, (31, 27), (35, 24), kind="unit"))
    # den one ULP of its constant on each side of 0 at the centres of a row: q is huge and every position is at the clamp, or void
    for tag, sign in (("den_above0", 1), ("den_below0", -1)):
        for edge in (CLAMP, REPEAT):
            out.append(_case(tag, nudged(_horizon((0.0, -0.25, 1.625), (-3.0, 2.0)), 5, 6, sign), BILINEAR, edge, STRAIGHT, (7, 5), (19, 9)))
    # a position that just reaches the clamp (X = 3: u = 2^22 exactly), and n_u = 0 meeting q = Inf
    reach = affine(warp_cases.translate(-(4194304.0 - 3.5), 1.0))
    for filt, edge in ((NEAREST, REPEAT), (BILINEAR, MIRROR), (BICUBIC, REPEAT), (BILINEAR, CLAMP)):
        out.append(_case("clamp", reach, filt, edge, STRAIGHT, (3, 5), (9, 7)))
        out.append(_case("qinf", Q_INF, filt, edge, STRAIGHT, (3, 5), (17, 6)))
    # REPEAT and MIRROR with n = 1, 2 and 3 and indices far outside
    far = product(affine((0.31, 0.0, 0.0, 0.43, -9.7, 4.2)), KEYSTONE)
    for n_src in (1, 2, 3):
        for edge in (REPEAT, MIRROR):
            f, _, fl = combos()
            out.append(_case("far", far, f, edge, fl, (n_src, n_src), (40, 30), kind="unit"))
            out.append(_case("far", KEYSTONE, BICUBIC, edge, fl, (n_src, 3), (33, 17), kind="unit"))
    # values
    for kind in KINDS:
        for flags in (0, STRAIGHT):
            out.append(_case("values", KEYSTONE, BICUBIC, ZERO, flags, (37, 11), (41, 17), kind=kind))
            out.append(_case("values", product(KEYSTONE, affine(warp_cases.scale(1.7))), BILINEAR, MIRROR, flags, (23, 5), (40, 13), kind=kind))
            out.append(_case("values", KEYSTONE, NEAREST, CLAMP, flags, (23, 5), (25, 6), kind=kind))
    seen, uniq = set(), []
    for c in out:
        if c["name"] not in seen:
            seen.add(c["name"])
            uniq.append(c)
    return uniq


CASES = _battery()
BY_NAME = {c["name"]: c for c in CASES}
AFFINE = [c["name"] for c in CASES if c["affine"] is not None]

source = warp_cases.source  # the source image's bits: the content inside the rectangle, NaN around it
before = warp_cases.before  # what dst holds before the call, or None for a never-written dst


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    w, h = c["dst_size"]
    out = perspective_ref.perspective(source(c), (h, w), c["matrix"], c["filter"], c["edge"], c["flags"], c["src_rect"], c["dst_rect"], before(c), **dict(variant))
    out.setflags(write=False)
    return out


def expected(name, **variant):
    """What dst holds after the case's call, by tests/perspective_ref.py (computed once per case and variant; do not modify the result)."""
    return _expected(name, tuple(sorted(variant.items())))
