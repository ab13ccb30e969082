"""The perspective rule on the CPU: the plan and the bounds of the library (jh_perspective_plan,
jh_perspective_bounds) and of the host twin (jl_...) against the reference (tests/perspective_ref.py), bit for bit; the queries' null
and illegal arguments; legality from both sides of every boundary; the ctypes mirror; the bounds property by brute force; den > 0 <=>
forward w > 0 on exact rationals; the reference's position against the exact rational one within the bound DESIGN 5.19 derives; the
constructors of jello_amd.perspective; texels worked by hand; the stand-alone check of include/jello_perspective.h
(tools/perspective_check.cpp), whose positions the reference equals; and that the battery (tests/perspective_cases.py) tells the rule
from eight near misses, and does not tell it from a ninth that is the same rule."""
import ctypes
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import jello_amd
from jello_amd import _lib
from jello_amd import perspective as persp
from jello_amd._lib import CPerspectiveDesc

import perspective_cases
import perspective_ref
import warp_cases
from abi_text import INCLUDE, ROOT, c_values
from perspective_ref import BICUBIC, BILINEAR, CLAMP, FILTERS, NEAREST, STRAIGHT, ZERO, same_bits

NAN, INF = math.nan, math.inf
IDENT = perspective_ref.IDENTITY
KEYSTONE = perspective_cases.KEYSTONE
CROSSING = (1.0, 0.0, -0.2, 0.0, 1.0, 0.0, 5.0, 4.0, 1.0)  # w = 1 - 0.2 x: 0 inside a source wider than 5
MATRICES = sorted({c["matrix"] for c in perspective_cases.CASES}) + [
    CROSSING, persp.rotate_y(math.radians(30), 800.0, (64, 64))["matrix"], persp.rotate_x(math.radians(-50), 120.0, (10, 30))["matrix"],
    (3.0, 7.0, 0.01, -2.0, 5.0, 0.02, 11.0, 13.0, 0.5), (1e-150, 0.0, 0.0, 0.0, 1e-150, 0.0, 0.0, 0.0, 1.0), (1e100, 0.0, 0.0, 0.0, 1e100, 0.0, 0.0, 0.0, 1e100),
    (1e154, 0.0, 0.0, 0.0, 1e154, 0.0, 0.0, 0.0, 1e-160), (2.0 ** -600, 0.0, 0.0, 0.0, 2.0 ** 500, 0.0, 0.0, 0.0, 2.0 ** 500)]  # (the last: an entry goes subnormal in the ldexp)
ILLEGAL = [((1.0, NAN, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), "a matrix entry is not finite"), ((1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, INF), "a matrix entry is not finite"),
           ((-INF, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), "a matrix entry is not finite"),
           ((1.4e154, 0.0, 0.0, 0.0, 1.4e154, 0.0, 0.0, 0.0, 1e-160), "an adjugate entry is not finite"),
           ((1e120, 0.0, 0.0, 0.0, 1e120, 0.0, 0.0, 0.0, 1e120), "the determinant is not finite"),
           ((1.0, 2.0, 0.0, 2.0, 4.0, 0.0, 0.0, 0.0, 1.0), "the determinant is 0"), ((1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0), "the determinant is 0"),
           ((0.0,) * 9, "the determinant is 0")]


def _bits(values):
    return tuple(np.array(values, np.float64).view(np.uint64).tolist())


@pytest.mark.parametrize("twin", [False, True], ids=["library", "twin"])
def test_the_plan_and_the_bounds_of_the_library_and_of_the_twin_are_the_references(built, twin):
    for m in MATRICES:
        G = jello_amd.perspective_plan(m, twin=twin)
        assert _bits(G) == _bits(perspective_ref.plan(m)), m
        assert max(abs(g) for g in G) <= 1.0 and max(abs(g) for g in G) > 0.5
        for filt in FILTERS:
            for src, dst in (((41, 29), (47, 33)), ((9, 7), (40, 30)), ((520, 260), (1040, 520)), ((1, 1), (1, 1)), ((32768, 32768), (32768, 32768)), ((5, 5), (0, 0))):
                assert jello_amd.perspective_bounds(m, src, filt, dst, twin=twin) == perspective_ref.bounds(m, src, filt, dst), (m, filt, src, dst)


def test_a_matrix_whose_inverse_is_dyadic_has_an_exact_plan():
    assert jello_amd.perspective_plan(IDENT) == IDENT
    assert jello_amd.perspective_plan(perspective_ref.affine(warp_cases.translate(3.5, -2.25))) == (0.25, 0.0, -0.875, 0.0, 0.25, 0.5625, 0.0, 0.0, 0.25)
    assert jello_amd.perspective_plan(perspective_ref.affine(warp_cases.scale(4))) == (0.25, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 1.0)
    assert jello_amd.perspective_plan((0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 8.0, 0.0, 1.0)) == (0.0, 0.125, 0.0, -0.125, 0.0, 1.0, 0.0, 0.0, 0.125)
    # det < 0: G is negated, den stays positive in front
    assert jello_amd.perspective_plan((-1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 8.0, 0.0, 1.0)) == (-0.125, 0.0, 1.0, 0.0, 0.125, 0.0, 0.0, 0.0, 0.125)


def test_null_and_illegal_arguments_of_both_queries_leave_the_outputs_untouched(built):
    L = _lib.load_host()
    m9 = (ctypes.c_double * 9)
    for plan_f, bounds_f in ((L.hip.jh_perspective_plan, L.hip.jh_perspective_bounds), (L.jl_perspective_plan, L.jl_perspective_bounds)):
        G, r = m9(*([77.0] * 9)), (ctypes.c_uint32 * 4)(7, 7, 7, 7)
        assert plan_f(None, G) == -1 and plan_f(m9(*IDENT), None) == -1 and plan_f(None, None) == -1
        assert bounds_f(None, 4, 4, 1, 8, 8, r) == -1 and bounds_f(m9(*IDENT), 4, 4, 1, 8, 8, None) == -1
        for m, _ in ILLEGAL:
            assert plan_f(m9(*m), G) == -1 and bounds_f(m9(*m), 4, 4, 1, 8, 8, r) == -1, m
        for args in ((32769, 4, 1, 8, 8), (4, 32769, 1, 8, 8), (4, 4, 1, 32769, 8), (4, 4, 1, 8, 32769), (4, 4, 3, 8, 8), (4, 4, -1, 8, 8)):
            assert bounds_f(m9(*IDENT), *args, r) == -1, args
        assert list(G) == [77.0] * 9 and list(r) == [7, 7, 7, 7]
        assert plan_f(m9(*IDENT), G) == 0 and bounds_f(m9(*IDENT), 32768, 32768, 2, 32768, 32768, r) == 0 and list(r) == [0, 0, 32768, 32768]
    L.jl_perspective_plan(m9(*ILLEGAL[3][0]), m9())
    assert L.jl_last_error() == b"perspective_plan: an adjugate entry is not finite"
    for f in (jello_amd.perspective_plan, lambda m: jello_amd.perspective_bounds(m, (4, 4), 1, (8, 8))):
        with pytest.raises(ValueError, match="jh_perspective: "):
            f(ILLEGAL[0][0])
        with pytest.raises(ValueError, match="9 entries"):
            f(IDENT[:6])


@pytest.mark.parametrize("k", range(len(ILLEGAL)))
def test_the_legality_boundaries_from_both_sides(k):
    m, why = ILLEGAL[k]
    with pytest.raises(ValueError, match=why):
        perspective_ref.plan(m)
    with pytest.raises(ValueError):
        jello_amd.perspective_plan(m)
    legal = {0: IDENT, 1: (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.7e308), 2: (-1.7e308, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1e-300),
             3: (1e154, 0.0, 0.0, 0.0, 1e154, 0.0, 0.0, 0.0, 1e-160), 4: (1e100, 0.0, 0.0, 0.0, 1e100, 0.0, 0.0, 0.0, 1e100),
             5: (1.0, 2.0, 0.0, 2.0, math.nextafter(4.0, 5.0), 0.0, 0.0, 0.0, 1.0), 6: (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 5e-324),
             7: (5e-324, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)}[k]
    assert _bits(jello_amd.perspective_plan(legal)) == _bits(perspective_ref.plan(legal))


def test_the_headers_constants_and_the_mirrors_layout():
    fields = ["matrix", "filter", "edge", "flags", "src_x", "src_y", "src_width", "src_height", "dst_x", "dst_y", "dst_width", "dst_height"]
    vals = c_values(["JH_PERSPECTIVE_STRAIGHT", "sizeof(jh_perspective_desc)"] + ["offsetof(jh_perspective_desc, %s)" % f for f in fields])
    assert vals[0] == STRAIGHT == jello_amd.engine.PERSPECTIVE_STRAIGHT
    assert vals[1] == ctypes.sizeof(CPerspectiveDesc)
    assert vals[2:] == [getattr(CPerspectiveDesc, f).offset for f in fields]


def _alpha_ones(w, h):
    bits = warp_cases.content("unit", w, h, seed=5)
    bits[..., 3] = 0x3C00  # alpha 1 everywhere: a texel that a tap reaches is not +0
    bits[..., 0] = 0x3C00
    return bits


@pytest.mark.parametrize("filt", FILTERS)
def test_outside_the_bounds_every_texel_is_zero(filt):
    """Brute force under ZERO on small images: the reference's image outside jh_perspective_bounds' rectangle is +0, and the rectangle
    is not the whole image unless the matrix crosses w = 0, where it is."""
    for m, src, dst, whole in ((KEYSTONE, (9, 7), (40, 30), False), (perspective_cases.product(KEYSTONE, perspective_ref.affine((-1.0, 0.0, 0.0, 1.0, 9.0, 0.0))), (9, 7), (40, 30), False),
                               (persp.compose(persp.affine(warp_cases.translate(14, 9)), persp.rotate_y(math.radians(40), 60.0, (5.5, 4.0)))["matrix"], (11, 8), (48, 36), False),
                               (CROSSING, (9, 7), (40, 30), True), (perspective_ref.affine(warp_cases.translate(100, 3)), (9, 7), (40, 30), False),
                               (perspective_ref.affine((2.0, 0.0, 0.0, 2.0, -3.0, -3.0)), (30, 30), (24, 20), True)):
        x, y, w, h = rect = jello_amd.perspective_bounds(m, src, filt, dst)
        assert rect == perspective_ref.bounds(m, src, filt, dst)
        out = perspective_ref.perspective(_alpha_ones(*src), (dst[1], dst[0]), m, filt, ZERO, STRAIGHT)
        live = out.any(axis=-1)
        inside = np.zeros_like(live)
        inside[y:y + h, x:x + w] = True
        assert not (live & ~inside).any(), (m, rect)
        assert (rect == (0, 0) + dst) == whole, (m, rect)
        if m is KEYSTONE:
            assert live.any() and w < dst[0] and h < dst[1]
    assert jello_amd.perspective_bounds(perspective_ref.affine(warp_cases.translate(100, 3)), (9, 7), filt, (40, 30)) == (0, 0, 0, 0)


def _exact(G, X, Y):
    """(n_u, n_v, den) of destination texel (X, Y) as exact rationals from the plan G."""
    g = [Fraction(v) for v in G]
    xp, yp = Fraction(2 * X + 1, 2), Fraction(2 * Y + 1, 2)
    return g[0] * xp + g[1] * yp + g[2], g[3] * xp + g[4] * yp + g[5], g[6] * xp + g[7] * yp + g[8]


def test_den_is_positive_where_the_forward_w_is_on_exact_rationals():
    """Integer matrices, so that the plan is the exact adjugate times a power of two: the exact source position of a destination texel
    has a forward w of the sign of the exact den, and the reference's void mask is that sign."""
    rng = np.random.default_rng(11)
    seen = {True: 0, False: 0}
    for _ in range(300):
        m = tuple(float(v) for v in rng.integers(-9, 10, 9))
        try:
            G = perspective_ref.plan(m)
        except ValueError:
            continue
        a, b, p, c, d, q, e, f, s = (Fraction(v) for v in m)
        _, _, void = perspective_ref.positions(G, (0, 0, 6, 5))
        for Y in range(5):
            for X in range(6):
                nu, nv, den = _exact(G, X, Y)
                if den == 0:
                    assert void[Y, X]
                    continue
                u, v = nu / den, nv / den
                w = p * u + q * v + s
                xw, yw = a * u + c * v + e, b * u + d * v + f
                assert w != 0 and xw / w == Fraction(2 * X + 1, 2) and yw / w == Fraction(2 * Y + 1, 2)  # the position is the inverse
                assert (den > 0) == (w > 0) == (not void[Y, X])
                seen[den > 0] += 1
    assert min(seen.values()) > 1000


DELTA = Fraction(7, 1 << 38)  # each three-term sum is within 7 x 2^15 x 2^-53 of its exact value
EPS = Fraction(1, 1 << 53)


def position_bound(u, den):
    """DESIGN 5.19's bound on |U 2^-32 - u| in texels for the exact rational position u and the exact den > DELTA."""
    return (1 + abs(u)) * (DELTA / (den - DELTA) * (1 + 3 * EPS) + 3 * EPS) + Fraction(1, 1 << 33)


def test_the_position_is_the_exact_one_within_the_derived_bound():
    """The reference's (U, V) against the exact rational position from the same plan, wherever den > 2 DELTA and the exact position is
    inside the clamp; the bound grows with 1 / den, and texels with a small den are among those checked."""
    checked, small, worst = 0, 0, Fraction(0)
    rects = ((0, 0, 13, 11), (32755, 32757, 13, 11), (1000, 20000, 9, 9))
    for m in MATRICES + [perspective_cases.from_inverse(((1.0, 0.0, -3.0), (0.0, 1.0, 2.0), (0.0, -2.0 ** -20, 6.6 * 2.0 ** -20)))]:
        G = perspective_ref.plan(m)
        for rect in rects:
            U, V, void = perspective_ref.positions(G, rect)
            for j in range(rect[3]):
                for i in range(rect[2]):
                    nu, nv, den = _exact(G, rect[0] + i, rect[1] + j)
                    if den <= 2 * DELTA:
                        continue
                    assert not void[j, i]
                    for n, got in ((nu, U[j, i]), (nv, V[j, i])):
                        u = n / den
                        if abs(u) >= 1 << 22:
                            continue
                        err, bound = abs(Fraction(int(got), 1 << 32) - u), position_bound(u, den)
                        assert err <= bound, (m, rect, i, j, float(err), float(bound))
                        worst = max(worst, err / bound)
                        checked += 1
                        small += den < Fraction(1, 1 << 12)
    assert checked > 20000 and small > 100 and worst > Fraction(1, 1000)  # (the bound is within three orders of what occurs)


def test_the_constructors():
    m6 = (1.5, 0.25, -0.25, 1.5, 3.0, -2.0)
    a = persp.affine(m6)["matrix"]
    assert tuple(a[i] for i in (0, 1, 3, 4, 6, 7)) == m6 and (a[2], a[5], a[8]) == (0.0, 0.0, 1.0)
    assert _bits(a) == _bits(perspective_ref.affine(m6))
    # from_quad maps the four corners onto the four points
    for size, quad in (((10, 10), ((0, 0), (10, 1), (9, 9), (1, 10))), ((640, 360), ((100.5, 50.25), (500, 20), (610, 300), (40, 340))),
                       ((29, 21), ((3, 3), (32, 3), (32, 24), (3, 24)))):
        m = persp.from_quad(size, quad)["matrix"]
        for (x, y), (qx, qy) in zip(((0, 0), (size[0], 0), size, (0, size[1])), quad):
            w = m[2] * x + m[5] * y + m[8]
            assert w > 0 and abs((m[0] * x + m[3] * y + m[6]) / w - qx) < 1e-9 and abs((m[1] * x + m[4] * y + m[7]) / w - qy) < 1e-9
        jello_amd.perspective_plan(m)
    for bad in (((0, 0), (10, 0), (0, 10), (10, 10)), ((0, 0), (10, 0), (3, 1), (0, 10)), ((0, 0), (5, 0), (10, 0), (0, 10))):  # crossing, concave, three on a line
        with pytest.raises(ValueError, match="from_quad"):
            persp.from_quad((10, 10), bad)
    # CSS matrix3d(a1 b1 c1 d1 a2 b2 c2 d2 a3 b3 c3 d3 a4 b4 c4 d4) on (x, y, 0, 1): x' w = a1 x + a2 y + a4, y' w = b1 x + b2 y + b4, w = d1 x + d2 y + d4
    m16 = [float(v) for v in range(1, 17)]
    a1, b1, c1, d1, a2, b2, c2, d2, a3, b3, c3, d3, a4, b4, c4, d4 = m16
    assert persp.from_matrix3d(m16)["matrix"] == (a1, b1, d1, a2, b2, d2, a4, b4, d4)
    # CSS perspective(d) rotateY(t) about the origin o: the matrices of the specification written out literally
    t, dist, (ox, oy) = math.radians(30), 800.0, (64.0, 48.0)
    rot = np.array([[math.cos(t), 0, math.sin(t), 0], [0, 1, 0, 0], [-math.sin(t), 0, math.cos(t), 0], [0, 0, 0, 1]])
    per = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, -1 / dist, 1]])
    to, back = np.eye(4), np.eye(4)
    to[:2, 3], back[:2, 3] = (ox, oy), (-ox, -oy)
    full = to @ per @ rot @ back
    got = np.array(persp.rotate_y(t, dist, (ox, oy))["matrix"]).reshape(3, 3).T
    for x, y in ((0, 0), (128, 0), (128, 96), (0, 96), (64, 48), (13.5, 77.25)):
        X = full @ np.array([x, y, 0, 1.0])
        P = got @ np.array([x, y, 1.0])
        assert abs(X[0] / X[3] - P[0] / P[2]) < 1e-9 and abs(X[1] / X[3] - P[1] / P[2]) < 1e-9
    x, y = 100.0, 30.0  # and in closed form: x' = ox + (x - ox) cos t / w, w = 1 + (x - ox) sin t / d
    w = 1 + (x - ox) * math.sin(t) / dist
    P = got @ np.array([x, y, 1.0])
    assert abs(P[0] / P[2] - (ox + (x - ox) * math.cos(t) / w)) < 1e-9 and abs(P[1] / P[2] - (oy + (y - oy) / w)) < 1e-9
    gx = np.array(persp.rotate_x(t, dist, (ox, oy))["matrix"]).reshape(3, 3).T
    w = 1 - (y - oy) * math.sin(t) / dist
    P = gx @ np.array([x, y, 1.0])
    assert abs(P[0] / P[2] - (ox + (x - ox) / w)) < 1e-9 and abs(P[1] / P[2] - (oy + (y - oy) * math.cos(t) / w)) < 1e-9
    # compose(a, b) applies b first
    c = persp.compose(persp.affine(warp_cases.translate(5, 7)), persp.affine(warp_cases.scale(2)))["matrix"]
    assert c == perspective_ref.affine((2.0, 0.0, 0.0, 2.0, 5.0, 7.0))
    with pytest.raises(ValueError):
        persp.rotate_y(0.1, 0.0)


def test_texels_by_hand():
    """A 4 x 2 source of distinct values under w = 1 + x / 4 (x' = x / w): destination texel X reads u = x' / (1 - x' / 4)."""
    src = np.zeros((2, 4, 4), np.uint16)
    for j in range(2):
        for i in range(4):
            src[j, i] = np.array([i + 1, 10 * (j + 1), 0.5, 1.0], np.float16).view(np.uint16)
    m = (1.0, 0.0, 0.25, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    assert perspective_ref.plan(m) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.25, 0.0, 1.0)
    U, V, void = perspective_ref.positions(perspective_ref.plan(m), (0, 0, 5, 1))
    # x' = 0.5: den 0.875, u = 4/7; 1.5: den 0.625, u = 2.4; 2.5: den 0.375, u = 20/3; 3.5: den 0.125, u = 28; 4.5: den -0.125, void
    assert list(void[0]) == [False, False, False, False, True]
    assert [int(v) for v in U[0][:4]] == [round(4 / 7 * 2 ** 32), int(np.rint(np.float64(1.5) * (1 / np.float64(0.625)) * 2 ** 32)), round(20 / 3 * 2 ** 32), 28 << 32]
    assert [int(v) for v in V[0][:4]] == [round(4 / 7 * 2 ** 32), 0x0CCCCCCCD, round(4 / 3 * 2 ** 32), 4 << 32]  # v = 0.5 / den
    out = perspective_ref.perspective(src, (1, 5), m, NEAREST, ZERO, STRAIGHT).view(np.float16)
    assert out[0, 0].tolist() == [1.0, 10.0, 0.5, 1.0] and out[0, 1].tolist() == [3.0, 10.0, 0.5, 1.0]  # (u, v) = (0.57, 0.57), (2.4, 0.8)
    assert not out[0, 2].any() and not out[0, 3].any() and not out[0, 4].any()  # u = 6.7 and 28: outside under ZERO; X = 4: void
    clamped = perspective_ref.perspective(src, (1, 5), m, NEAREST, CLAMP, STRAIGHT).view(np.float16)
    assert clamped[0, 2].tolist() == [4.0, 20.0, 0.5, 1.0] and clamped[0, 3].tolist() == [4.0, 20.0, 0.5, 1.0]
    assert not clamped[0, 4].any()  # a void texel is +0 whatever the edge mode
    bil = perspective_ref.perspective(src, (1, 5), m, BILINEAR, CLAMP, STRAIGHT).view(np.float16)
    f = np.float32(((int(U[0, 1]) - (1 << 31)) >> 16 & 0xFFFF) * 2.0 ** -16)  # u = 2.4: texels 1 and 2, fraction 0.9 truncated to 16 bits
    assert bil[0, 1, 0] == np.float16(np.float32(2.0) * (np.float32(1.0) - f) + np.float32(3.0) * f)


def test_the_stand_alone_check_builds_and_passes(tmp_path):
    """tools/perspective_check.cpp is include/jello_perspective.h with a main of its own.  Its header has the command with the
    sanitizers; here it is built without them and run, and the positions it prints -- the text the kernel compiles, on the host --
    equal the reference's bit for bit."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "perspective_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", INCLUDE, os.path.join(ROOT, "tools", "perspective_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.splitlines()[-1].startswith("ok: "), out
    for m, rect in ((KEYSTONE, (0, 0, 47, 33)), (perspective_cases.Q_INF, (0, 0, 17, 6)), (CROSSING, (3, 5, 20, 9)), (MATRICES[0], (30000, 32700, 40, 68)),
                    (perspective_cases.BY_NAME[[n for n in perspective_cases.BY_NAME if n.startswith("den_above0")][0]]["matrix"], (0, 0, 19, 9)),
                    (perspective_cases.BY_NAME[[n for n in perspective_cases.BY_NAME if n.startswith("horizon_centres")][0]]["matrix"], (0, 0, 35, 24))):
        text = subprocess.check_output([exe] + [float(v).hex() for v in m] + [str(v) for v in rect]).decode()
        U, V, void = perspective_ref.positions(perspective_ref.plan(m), rect)
        want = ["void" if void[j, i] else "%d %d" % (U[j, i], V[j, i]) for j in range(rect[3]) for i in range(rect[2])]
        assert text.split("\n")[:-1] == want, (m, rect)


NEAR_MISSES = {"an fma in the numerator": dict(fused=True), "n / den": dict(divide=True), "den >= 0 in front": dict(den_ge=True),
               "centres at +0": dict(centre0=True), "truncation": dict(trunc=True), "no clamp": dict(clamp=False),
               "a void texel under CLAMP": dict(void_clamp=True), "row-major": dict(row_major=True)}


def _small_first():
    return sorted(perspective_cases.CASES, key=lambda c: (not c["name"].startswith("flip_"), c["dst_size"][0] * c["dst_size"][1]))


@pytest.mark.parametrize("what", sorted(NEAR_MISSES))
def test_the_battery_tells_the_rule_from_a_near_miss(what):
    variant = NEAR_MISSES[what]
    for c in _small_first():
        if c["dst_size"][0] * c["dst_size"][1] > 2000:
            continue
        try:
            other = perspective_cases.expected(c["name"], **variant)
        except ValueError:
            return  # (the near miss refuses a matrix the rule takes)
        if not same_bits(other, perspective_cases.expected(c["name"])):
            return
    pytest.fail("no case of the battery tells the rule from: " + what)


def test_a_division_by_the_power_of_two_is_the_same_rule():
    """The ninth: G = adj / 2^k in place of the ldexp.  The scaling rounds nothing either way, so the plans are the same bits and no
    case of the battery can differ; a scale that is no power of two cancels in n (1 / den) only up to rounding, which is why the rule
    fixes the power of two."""
    for m in MATRICES[:-4]:
        assert _bits(perspective_ref.plan(m, norm_divide=True)) == _bits(perspective_ref.plan(m))
    for c in perspective_cases.CASES:
        if c["dst_size"][0] * c["dst_size"][1] <= 2000:
            assert same_bits(perspective_cases.expected(c["name"], norm_divide=True), perspective_cases.expected(c["name"])), c["name"]


def test_the_battery_covers_what_it_claims():
    cases = perspective_cases.CASES
    assert len({c["inst"] for c in cases}) == 24
    sizes = {c["dst_size"] for c in cases}
    assert {(1, 1), (1, 5), (5, 1)} <= sizes and {w for w, _ in sizes} >= set(perspective_cases.WIDTHS) and {h for _, h in sizes} >= set(perspective_cases.HEIGHTS)
    assert all(max(c["src_size"] + c["dst_size"]) <= 128 for c in cases if not c["name"].startswith("big_"))
    big = [c for c in cases if c["name"].startswith("big_")]
    assert len(big) == 1 and big[0]["filter"] == NEAREST and big[0]["dst_size"] == warp_cases.BIG[0]
    assert any(c["dst_rect"] and c["dst_rect"][0] % 16 and c["src_rect"] for c in cases) and any(c["prior"] == "never" for c in cases)
    assert any(perspective_ref.adjugate(c["matrix"])[1] < 0 for c in cases)  # a mirrored view
    for tag, low in (("tuned_below", 0xFFFFFFFF), ("tuned_at", 0), ("tuned_above", 1), ("tuned_frac0000_", 0x80000000), ("tuned_fracffff", 0x7FFFFFFF)):
        c = [c for c in cases if c["name"].startswith(tag)][0]
        assert perspective_cases.position_of(c["matrix"], 11, 7)[0] & 0xFFFFFFFF == low, tag
    d0 = [c for c in cases if c["name"].startswith("horizon_centres")][0]
    assert all(perspective_cases.den_of(d0["matrix"], X, 6) == 0.0 for X in range(35)) and perspective_cases.den_of(d0["matrix"], 0, 5) > 0
    up = [c for c in cases if c["name"].startswith("den_above0")][0]
    down = [c for c in cases if c["name"].startswith("den_below0")][0]
    assert 0 < perspective_cases.den_of(up["matrix"], 5, 6) < 2.0 ** -45 and 0 > perspective_cases.den_of(down["matrix"], 5, 6) > -2.0 ** -45
    qinf = [c for c in cases if c["name"].startswith("qinf")][0]
    _, _, void = perspective_ref.positions(perspective_ref.plan(qinf["matrix"]), (0, 0, 17, 6))
    assert void[:, 6].all() and void.sum() == 6  # n_u = 0 meets q = Inf: a NaN, void; the other texels are at the clamp
    reach = [c for c in cases if c["name"].startswith("clamp_")][0]
    U, _, _ = perspective_ref.positions(perspective_ref.plan(reach["matrix"]), (0, 0, 9, 1))
    assert [int(u) for u in U[0][2:5]] == [(1 << 54) - (1 << 32), 1 << 54, 1 << 54]
    assert {c["src_size"][0] for c in cases if c["name"].startswith("far_")} == {1, 2, 3}
    assert {c["kind"] for c in cases} >= set(warp_cases.KINDS)
