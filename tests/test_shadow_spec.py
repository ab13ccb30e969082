"""The shadow rule on the CPU: the plan and the bounds of the library (jh_shadow_plan, jh_shadow_bounds) and of the host
twin (jl_...) against the reference (tests/shadow_ref.py), bit for bit; legality from both sides of every boundary; the queries' own
rows; the ctypes mirrors; the sweep of the erf approximant; the accuracy conditions of the binary64 restatement against the exact
convolution; the reference against the restatement within the derived rounding bound; consequences of the rule; texels worked by
hand; the bounds property by brute force; box_shadow's CSS arithmetic; that the battery (tests/shadow_cases.py) tells the rule from
its near misses; and the stand-alone check of include/jello_shadow.h (tools/shadow_check.cpp), whose texels the reference equals.

Accuracy of the rule (binary64 restatement against the exact convolution, the grid of _grid below, K = 4), measured here once:
r / sigma = 0: 0, 1/4: 9.1e-5 (N = 4), 1: 3.9e-4 (N = 8), 2: 3.7e-4, 4: 1.05e-3, 8: 1.99e-3, 16: 3.96e-3, 32: 4.9e-3, 128: 3.2e-3 (N = 16)."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import _lib
from jello_amd.engine import _shadow_desc

import shadow_cases
import shadow_ref
from abi_text import INCLUDE, ROOT, c_values
from image_ref import same_bits
from shadow_ref import F, IDENTITY, INVERT, OVER

FILL = 0xA5
NAN, INF = math.nan, math.inf


def _desc(box=(10.0, 8.0, 50.0, 30.0), radius=6.0, sigma=2.0, matrix=None, flags=0, rect=None):
    with np.errstate(all="ignore"):
        d = _shadow_desc(box, radius, sigma, (0.0, 0.0, 0.0, 1.0), matrix, rect)
    d.flags = flags
    return d


def _plan_tuple(p):
    return (tuple(p.m), tuple(p.centre)) + tuple(np.float32(getattr(p, k)).view(np.uint32) for k in ("a", "b", "radius", "core", "straight", "sigma", "inv_s", "window")) + (p.n, p.k)


def _ref_tuple(pl):
    return (tuple(pl["m"]), tuple(pl["centre"])) + tuple(np.float32(pl[k]).view(np.uint32) for k in ("a", "b", "radius", "core", "straight", "sigma", "inv_s", "window")) + (pl["n"], pl["k"])


PLAN_INPUTS = [dict(shadow_ref.DEFAULTS, **c["desc"]) for c in shadow_cases.CASES] + [
    dict(box=(0.1, 0.2, 0.3, 0.7), radius=1e-30, sigma=2.0 ** -8, matrix=IDENTITY),
    dict(box=(-2.0 ** 22, -2.0 ** 22, 2.0 ** 22, 2.0 ** 22), radius=3.0e38, sigma=65536.0, matrix=(64.0, 0.0, 0.0, -64.0, 2.0 ** 22, -2.0 ** 22)),
    dict(box=(1.0, 1.0, 9.0, 9.0), radius=2.0, sigma=4.0, matrix=(1.0 / 64.0, 0.0, 0.0, 1.0 / 64.0, 0.0, 0.0)),
]


# ---- the plan and the bounds: library, host twin and reference ----

@pytest.mark.parametrize("twin", [False, True])
def test_the_plan_and_the_bounds_of_the_library_and_of_the_twin_are_the_references(built, twin):
    L = jello_amd.load_host()
    plan_f = L.jl_shadow_plan if twin else L.hip.jh_shadow_plan
    bounds_f = L.jl_shadow_bounds if twin else L.hip.jh_shadow_bounds
    for d in PLAN_INPUTS:
        desc, plan, rect = _desc(d["box"], d["radius"], d["sigma"], d["matrix"]), _lib.CShadowPlan(), (ctypes.c_uint32 * 4)()
        assert plan_f(ctypes.byref(desc), ctypes.byref(plan)) == 0
        assert _plan_tuple(plan) == _ref_tuple(shadow_ref.plan(d["box"], d["radius"], d["sigma"], d["matrix"])), d
        for size in ((70, 40), (4096, 4096), (1, 1), (1 << 23, 3)):
            assert bounds_f(ctypes.byref(desc), size[0], size[1], rect) == 0
            assert tuple(rect) == shadow_ref.bounds(d["box"], d["radius"], d["sigma"], d["matrix"], size), (d, size)
    got = jello_amd.shadow_plan((10.0, 8.0, 50.0, 30.0), 100.0, 0.0, twin=twin)
    assert (got["a"], got["b"], got["radius"], got["core"], got["straight"], got["sigma"], got["n"], got["k"]) == (20.0, 11.0, 11.0, 9.0, 0.0, 2.0 ** -8, 16, 4)
    assert tuple(got["centre"]) == (30 << 32, 19 << 32) and got["m"] == (1 << 31, 0, 0, 0, 1 << 31, 0)
    assert jello_amd.shadow_bounds((100.0, 50.0, 400.0, 250.0), 10.0, 8.0, (4096, 4096), twin=twin) == (70, 20, 360, 260)  # grown by 29, -1 and +1


def test_a_card_in_a_large_frame_costs_a_launch_over_its_shadow(built):
    x, y, w, h = jello_amd.shadow_bounds((1000.0, 2000.0, 1300.0, 2200.0), 12.0, 6.0, (4096, 4096))
    assert (w, h) == (300 + 2 * 22 + 2, 200 + 2 * 22 + 2) and w * h < 4096 * 4096 // 100


# ---- legality, from both sides of every boundary ----

LEGALITY = [
    # (legal, illegal, the reason)
    (dict(box=(0.0, 0.0, 2.0 ** 22, 1.0)), dict(box=(0.0, 0.0, INF, 1.0)), "the box is not finite"),
    (dict(box=(0.0, 0.0, 1.0, 1.0)), dict(box=(0.0, NAN, 1.0, 1.0)), "the box is not finite"),
    (dict(box=(2.0, 0.0, 2.0, 1.0)), dict(box=(2.0, 0.0, 1.9999999, 1.0)), "the box has x1 < x0 or y1 < y0"),
    (dict(box=(0.0, 5.0, 1.0, 5.0)), dict(box=(0.0, 5.0, 1.0, 4.9999995)), "the box has x1 < x0 or y1 < y0"),
    (dict(box=(-2.0 ** 22, 0.0, 2.0 ** 22, 1.0)), dict(box=(-2.0 ** 22 - 0.5, 0.0, 1.0, 1.0)), "a box coordinate above 2^22"),
    (dict(box=(0.0, 0.0, 1.0, 2.0 ** 22)), dict(box=(0.0, 0.0, 1.0, 2.0 ** 22 + 0.5)), "a box coordinate above 2^22"),
    (dict(radius=0.0), dict(radius=-1e-45), "the radius is negative or not finite"),
    (dict(radius=3.0e38), dict(radius=INF), "the radius is negative or not finite"),
    (dict(radius=1.0), dict(radius=NAN), "the radius is negative or not finite"),
    (dict(sigma=0.0), dict(sigma=-1e-45), "sigma is outside [0, 2^16] or not finite"),
    (dict(sigma=65536.0), dict(sigma=65536.008), "sigma is outside [0, 2^16] or not finite"),
    (dict(sigma=1.0), dict(sigma=NAN), "sigma is outside [0, 2^16] or not finite"),
    (dict(flags=3), dict(flags=4), "unknown flag bits"),
    (dict(matrix=(1.0, 2.0, 2.0, 4.5, 0.0, 0.0)), dict(matrix=(1.0, 2.0, 2.0, 4.0, 0.0, 0.0)), "the determinant is 0"),
    (dict(matrix=(1.0 / 64.0, 0.0, 0.0, 1.0, 0.0, 0.0)), dict(matrix=(1.0 / 65.0, 0.0, 0.0, 1.0, 0.0, 0.0)), "an inverse coefficient above 64 (a minification beyond 64:1)"),
    (dict(matrix=(1.0, 0.0, 0.0, 1.0, 2.0 ** 22, 0.0)), dict(matrix=(1.0, 0.0, 0.0, 1.0, 2.0 ** 22 + 1.0, 0.0)), "an inverse offset above 2^22"),
    (dict(matrix=(1e300, 0.0, 0.0, 1.0, 0.0, 0.0)), dict(matrix=(NAN, 0.0, 0.0, 1.0, 0.0, 0.0)), "a matrix entry is not finite"),
]


@pytest.mark.parametrize("legal, illegal, why", LEGALITY)
def test_legality_from_both_sides(built, legal, illegal, why):
    """The library, the twin (whose text is the reason) and the reference agree on each side; a refusal leaves the outputs untouched."""
    L = jello_amd.load_host()
    for kw, ok in ((legal, True), (illegal, False)):
        desc = _desc(**kw)
        for f, g in ((L.hip.jh_shadow_plan, L.hip.jh_shadow_bounds), (L.jl_shadow_plan, L.jl_shadow_bounds)):
            plan, rect = _lib.CShadowPlan(), (ctypes.c_uint32 * 4)()
            ctypes.memset(ctypes.byref(plan), FILL, ctypes.sizeof(plan))
            ctypes.memset(rect, FILL, 16)
            rp, rb = f(ctypes.byref(desc), ctypes.byref(plan)), g(ctypes.byref(desc), 64, 64, rect)
            if ok:
                assert (rp, rb) == (0, 0)
            else:
                assert (rp, rb) == (-1, -1)
                assert bytes(plan) == bytes([FILL]) * ctypes.sizeof(plan) and bytes(rect) == bytes([FILL]) * 16
        if not ok:
            assert L.jl_last_error().decode() == "shadow_bounds: " + why
        args = dict(dict(box=(10.0, 8.0, 50.0, 30.0), radius=6.0, sigma=2.0, matrix=IDENTITY, flags=0), **kw)
        if ok:
            shadow_ref.legal(**args)
        else:
            with pytest.raises(ValueError):
                shadow_ref.legal(**args)


def test_the_extent_limit_from_both_sides(built):
    L = jello_amd.load_host()
    desc, rect = _desc(), (ctypes.c_uint32 * 4)()
    for f in (L.hip.jh_shadow_bounds, L.jl_shadow_bounds):
        assert f(ctypes.byref(desc), 1 << 23, 1 << 23, rect) == 0
        assert f(ctypes.byref(desc), (1 << 23) + 1, 1, rect) == -1 and f(ctypes.byref(desc), 1, (1 << 23) + 1, rect) == -1
    assert L.jl_last_error().decode() == "shadow_bounds: an image extent above 2^23"
    with pytest.raises(ValueError):
        shadow_ref.shadow(((1 << 23) + 1, 1), box=(0.0, 0.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        jello_amd.shadow_bounds((0.0, 0.0, 1.0, 1.0), 0.0, 1.0, ((1 << 23) + 1, 1))


# ---- the queries' own rows ----

def test_the_queries_null_arguments_and_the_twins_text(built):
    L = jello_amd.load_host()
    desc, plan, rect = _desc(), _lib.CShadowPlan(), (ctypes.c_uint32 * 4)()
    for lib, prefix in ((L.hip, "jh_"), (L, "jl_")):
        pf, bf = getattr(lib, prefix + "shadow_plan"), getattr(lib, prefix + "shadow_bounds")
        assert pf(ctypes.byref(desc), ctypes.byref(plan)) == 0 and bf(ctypes.byref(desc), 64, 64, rect) == 0
        assert pf(None, ctypes.byref(plan)) == -1 and pf(ctypes.byref(desc), None) == -1
        assert bf(None, 64, 64, rect) == -1 and bf(ctypes.byref(desc), 64, 64, None) == -1
    assert L.jl_last_error().decode() == "shadow_bounds: null argument"
    L.jl_shadow_plan(None, ctypes.byref(plan))
    assert L.jl_last_error().decode() == "shadow_plan: null argument"
    assert L.jl_shadow_plan.argtypes == L.hip.jh_shadow_plan.argtypes and L.jl_shadow_bounds.argtypes == L.hip.jh_shadow_bounds.argtypes


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    d = _shadow_desc((1.0, 2.0, 3.0, 4.0), 0.5, 1.5, (0.1, 0.2, 0.3, 0.4), (2.0, 0.0, 0.0, 2.0, 1.0, -1.0), (1, 2, 3, 4), True, True)
    assert (list(d.matrix), (d.x, d.y, d.width, d.height), d.flags, d.radius, d.sigma, list(d.box)) == ([2.0, 0.0, 0.0, 2.0, 1.0, -1.0], (1, 2, 3, 4), 3, 0.5, 1.5, [1.0, 2.0, 3.0, 4.0])
    assert [np.float32(v) for v in d.color] == [np.float32(v) for v in (0.1, 0.2, 0.3, 0.4)]
    plain = _shadow_desc((1.0, 2.0, 3.0, 4.0), 0.5, 1.5, (0, 0, 0, 1))
    assert (list(plain.matrix), plain.flags, plain.width, plain.height) == ([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], 0, 0, 0)
    assert hip.jh_shadow(None, 1, ctypes.byref(d)) == -1 and hip.jh_shadow(None, 1, None) == -1


def test_the_headers_constants_and_the_mirrors_layout():
    assert c_values(["JH_SHADOW_OVER", "JH_SHADOW_INVERT"]) == [1, 2] == [int(jello_amd.ShadowFlags.OVER), int(jello_amd.ShadowFlags.INVERT)] == [OVER, INVERT]
    for mirror, name in ((_lib.CShadowDesc, "jh_shadow_desc"), (_lib.CShadowPlan, "jh_shad_plan")):
        fields = [f for f, _ in mirror._fields_]
        want = c_values(["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, f) for f in fields])
        assert [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want
    assert [f for f, _ in _lib.CShadowDesc._fields_] == ["matrix", "x", "y", "width", "height", "flags", "radius", "sigma", "box", "color"]


# ---- G, the erf approximant ----

def test_the_approximant_is_within_2_to_the_minus_20_of_phi_and_monotone():
    """Phi(t) = (1 + G(t / sqrt 2)) / 2: |G - erf| <= 2^-19 over a dense sweep of binary32 arguments, every binary32 between 0.5 and
    0.5005 in turn and 2^21 others; G is odd, non-decreasing along every sweep, exactly 1 from 4 on and exactly 0 at 0."""
    sweeps = [np.linspace(-4.5, 4.5, (1 << 21) + 1).astype(F), np.arange(np.float32(0.5).view(np.uint32), np.float32(0.5005).view(np.uint32), dtype=np.uint32).view(F),
              np.geomspace(1e-30, 4.0, 100001).astype(F)]
    worst = 0.0
    for z in sweeps:
        g = shadow_ref.erf32(z)
        worst = max(worst, float(np.abs(g.astype(np.float64) - shadow_ref._erf64(z.astype(np.float64))).max()))
        assert np.all(np.diff(g) >= 0) and np.all(np.abs(g) <= 1)
        assert np.array_equal(shadow_ref.erf32(-z).view(np.uint32), (-g).view(np.uint32))
    print("max |G - erf| = %.3e (Phi: %.3e; allowed 2^-20 = %.3e)" % (worst, worst / 2, 2.0 ** -20))
    assert worst / 2 <= 2.0 ** -20
    assert shadow_ref.erf32(F(4.0)) == 1 and shadow_ref.erf32(F(3.0e38)) == 1 and shadow_ref.erf32(F(-INF)) == -1 and shadow_ref.erf32(F(0.0)) == 0
    assert 1 - 0.5 * (1 + math.erf(4.0)) < 2.0 ** -24  # the clamp lies beyond the point where 1 - Phi < 2^-24 (in erf's argument: 4 = 5.66 sigma)


# ---- the accuracy conditions ----

RATIOS = (0, 0.25, 1, 2, 4, 8, 16, 32, 128)


def _grid(ratio, sigma=2.0):
    """(a, b, r, points): positions on, inside and outside each corner (five directions, seven radii) and each straight side."""
    r = ratio * sigma
    a, b = r + 3 * sigma + 5.0, r + 2 * sigma + 3.0
    pts = []
    for sx in (1, -1):
        for sy in (1, -1):
            cx, cy = sx * (a - r), sy * (b - r)
            for ang in (10, 30, 45, 60, 80):
                for rad in (r - 2 * sigma, r - sigma, r - 0.5 * sigma, r, r + 0.5 * sigma, r + sigma, r + 2 * sigma):
                    rad = max(rad, 0.0)
                    pts.append((cx + sx * rad * math.cos(math.radians(ang)), cy + sy * rad * math.sin(math.radians(ang))))
            pts.append((sx * a, sy * b))
    for d in (-2 * sigma, -sigma, 0, sigma, 2 * sigma):
        pts += [(a + d, 0.3), (-a - d, -0.7), (0.2, b + d), (-0.4, -b - d), (a + d, b - r), (a - r, b + d)]
    return a, b, r, pts


@pytest.mark.parametrize("ratio", RATIOS)
def test_the_restatement_is_within_the_accuracy_conditions_of_the_exact_convolution(ratio):
    """1/512 for r <= 4 sigma, 1/128 for every r / sigma; the exact convolution is the closed form with math.erf for r = 0 and a
    dense binary64 row integration otherwise.  N is the plan's."""
    sigma = 2.0
    a, b, r, pts = _grid(ratio, sigma)
    pl = shadow_ref.plan((-a, -b, a, b), r, sigma)
    pl64 = dict(a=a, radius=r, core=a - r, straight=b - r, inv_s=1.0 / (sigma * math.sqrt(2.0)), window=shadow_ref.K * sigma, n=pl["n"])
    x, y = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    s = shadow_ref.coverage(pl64, x, y, np.float64)
    if r == 0:
        e = np.array([0.25 * (math.erf((py + b) * pl64["inv_s"]) - math.erf((py - b) * pl64["inv_s"])) * (math.erf((px + a) * pl64["inv_s"]) - math.erf((px - a) * pl64["inv_s"]))
                      for px, py in pts])
    else:
        e = np.array([shadow_ref.exact(a, b, r, sigma, px, py) for px, py in pts])
    worst = float(np.abs(s - e).max())
    print("r / sigma = %g, N = %d: max |S - exact| = %.3e" % (ratio, pl["n"], worst))
    assert worst <= (1.0 / 512.0 if ratio <= 4 else 1.0 / 128.0)


def _rounding_bound(pl, extent):
    """The binary32 rule against its binary64 restatement at the same int64 positions and plan scalars ("Rounding"):
    one G differs by e_G = 2^-19 (the approximant) + (2 / sqrt pi) inv_s 2^-24 (|p| + |w| + |p + w|) 1.5 (the rounding of the position, of
    the sum and of the product, where |z| < 4; beyond, both are 1) with |p|, |w| <= extent; the straight product by 2 e_G; each cap by
    3 e_G (the band term by 2 e_G against weights that sum to at most 2, the weights by summation by parts against band terms in [0, 2]);
    2^-20 for the accumulations and the final product."""
    e_g = 2.0 ** -19 + 1.1284 * float(pl["inv_s"]) * 2.0 ** -24 * (4.0 * extent) * 1.5
    return 8.0 * e_g + 2.0 ** -20


@pytest.mark.parametrize("name", ["radius_pill", "radius_disc", "radius_sharp", "matrix_rot30_r6", "matrix_scale_r6", "sigma_8_r9", "sigma_0.5_r9", "steps_r3.0000002_n16"])
def test_the_reference_is_the_restatement_within_the_rounding_bound(name):
    c = shadow_cases.BY_NAME[name]
    d = dict(shadow_ref.DEFAULTS, **c["desc"])
    w, h = c["size"]
    pl = shadow_ref.plan(d["box"], d["radius"], d["sigma"], d["matrix"])
    dU, dV = shadow_ref.positions(pl, (0, 0, w, h))
    s32 = shadow_ref.coverage(pl, shadow_ref.to_f32(dU), shadow_ref.to_f32(dV))
    s64 = shadow_ref.restate(pl, (0, 0, w, h))
    extent = float(max(np.abs(dU).max(), np.abs(dV).max())) / 2.0 ** 32 + float(max(pl["a"], pl["b"]))
    worst, bound = float(np.abs(s32.astype(np.float64) - s64).max()), _rounding_bound(pl, extent)
    print("%s: max |binary32 - binary64| = %.3e, bound %.3e" % (name, worst, bound))
    assert worst <= bound < 1.0 / 512.0


# ---- consequences of the rule ----

def _s(box, radius, sigma, size, matrix=IDENTITY):
    pl = shadow_ref.plan(box, radius, sigma, matrix)
    dU, dV = shadow_ref.positions(pl, (0, 0, size[0], size[1]))
    return shadow_ref.coverage(pl, shadow_ref.to_f32(dU), shadow_ref.to_f32(dV)), pl


def test_symmetry_under_the_boxs_two_reflections():
    """The centre on a texel corner: the reflection in x is exact (G is odd), the one in y swaps the order the caps add in."""
    s, _ = _s((10.0, 8.0, 50.0, 32.0), 9.0, 2.0, (60, 40))
    assert np.array_equal(s, s[:, ::-1])
    assert np.abs(s - s[::-1]).max() <= 64 * 2.0 ** -24


def test_deep_inside_far_outside_and_the_decay_along_a_normal():
    s, pl = _s((-40.0, -40.0, 140.0, 100.0), 10.0, 2.0, (100, 60))
    assert np.all(s == 1.0)  # every band is saturated and the caps' windows are empty
    s, pl = _s((10.0, 10.0, 90.0, 50.0), 12.0, 2.0, (100, 60))
    assert abs(float(s[30, 50]) - 1.0) <= 2 * (1 - 0.5 * (1 + math.erf(shadow_ref.K / math.sqrt(2.0)))) + 2.0 ** -19  # (the window cuts the caps' tails)
    assert s[0, 0] == 0 and np.all(s >= 0) and np.all(s <= 1)
    row = s[30, 50:]  # along the normal of the right side
    assert np.all(np.diff(row) <= 0) and row[0] > 0.999 and row[-1] < 1e-4
    cut = 2 * (1 - 0.5 * (1 + math.erf(shadow_ref.K / math.sqrt(2.0)))) + 2.0 ** -20  # (where a cap is in reach its window moves with the row: the tails it cuts)
    col = s[30:, 50]
    assert np.all(np.diff(col) <= cut) and col[-1] < 1e-3
    diag = np.array([s[30 + k, 70 + k] for k in range(25)])  # through the corner
    assert np.all(np.diff(diag) <= cut) and diag[0] > 0.99 and diag[-1] < 1e-4


def test_a_vanishing_radius_is_the_sharp_path_within_the_bound():
    sharp, pl0 = _s((10.0, 8.0, 50.0, 30.0), 0.0, 1.5, (60, 40))
    tiny, pl = _s((10.0, 8.0, 50.0, 30.0), 1e-6, 1.5, (60, 40))
    assert pl0["radius"] == 0 and pl["radius"] > 0 and pl["n"] == 4
    assert np.abs(sharp - tiny).max() <= _rounding_bound(pl, 60.0)
    empty, _ = _s((10.0, 8.0, 10.0, 30.0), 3.0, 1.5, (60, 40))
    assert np.all(empty == 0)


def test_texels_worked_by_hand():
    """sigma = 1, r = 0, the box from (10.5, 5.5) far to the right and down: texel (10, y) has its centre ON the left edge, texel (10, 5)
    on the corner; texel (11, 20) lies 1 sigma inside the edge: Phi(1)."""
    box = (10.5, 5.5, 1000.0, 1000.0)
    s, _ = _s(box, 0.0, 1.0, (40, 30))
    assert s[20, 10] == 0.5 and s[5, 10] == 0.25 and s[20, 30] == 1.0 and s[20, 0] == 0.0 and s[0, 20] < 1e-6  # (5 sigma above the top edge)
    assert abs(float(s[20, 11]) - 0.8413447460685429) <= 2.0 ** -20 and abs(float(s[20, 9]) - 0.15865525393145707) <= 2.0 ** -20
    out = shadow_ref.shadow((30, 40), None, None, box=box, radius=0.0, sigma=1.0, color=(0.0, 0.0, 0.0, 1.0))
    assert [int(out[20, 10, 3]), int(out[5, 10, 3]), int(out[20, 30, 3]), int(out[20, 0, 3])] == [0x3800, 0x3400, 0x3C00, 0]
    inv = shadow_ref.shadow((30, 40), None, None, box=box, radius=0.0, sigma=1.0, color=(0.5, 0.0, 0.0, 1.0), flags=INVERT)
    assert [int(inv[20, 10, 3]), int(inv[5, 10, 3]), int(inv[20, 30, 3]), int(inv[20, 0, 3])] == [0x3800, 0x3A00, 0, 0x3C00]
    assert int(inv[20, 0, 0]) == 0x3800  # the colour is stored un-premultiplied: 0.5 S' / S'
    # OVER of an opaque half-covered texel onto opaque white: alpha 1, colour 0.5 white + 0.5 x 0 black
    white = np.full((30, 40, 4), 0x3C00, np.uint16)
    over = shadow_ref.shadow((30, 40), None, white, box=box, radius=0.0, sigma=1.0, color=(0.0, 0.0, 0.0, 1.0), flags=OVER)
    assert list(over[20, 10]) == [0x3800, 0x3800, 0x3800, 0x3C00] and list(over[20, 30]) == [0, 0, 0, 0x3C00] and list(over[20, 0]) == [0x3C00] * 4
    # a half-texel translation moves the edge onto the texel corners: texel 10 is then half a texel outside
    moved, _ = _s(box, 0.0, 1.0, (40, 30), (1.0, 0.0, 0.0, 1.0, 0.5, 0.0))
    assert abs(float(moved[20, 10]) - 0.5 * (1 + math.erf(-0.5 / math.sqrt(2.0)))) <= 2.0 ** -20
    assert abs(float(moved[20, 11]) - 0.5 * (1 + math.erf(0.5 / math.sqrt(2.0)))) <= 2.0 ** -20


def test_the_position_is_the_texel_centre_through_the_inverse():
    pl = shadow_ref.plan((0.0, 0.0, 20.0, 10.0), 0.0, 1.0, (2.0, 0.0, 0.0, 0.5, -6.0, 4.0))
    dU, dV = shadow_ref.positions(pl, (0, 0, 8, 8))
    x, y = shadow_ref.to_f32(dU), shadow_ref.to_f32(dV)
    assert x[0, 3] == (3.5 + 6.0) / 2.0 - 10.0 and y[5, 0] == (5.5 - 4.0) / 0.5 - 5.0
    big = np.array([(1 << 61) + 77, -((7 << 40) + 99), 255, 256, -1], np.int64)
    assert np.all(np.abs(shadow_ref.to_f32(big).astype(np.float64) - big / 2.0 ** 32) <= 2.0 ** -24 + np.abs(big / 2.0 ** 32) * 2.0 ** -24)


# ---- the bounds ----

@pytest.mark.parametrize("matrix", sorted(shadow_cases.MATRICES))
def test_outside_the_bounds_the_coverage_is_below_2_to_the_minus_12(matrix):
    m = shadow_cases.MATRICES[matrix]
    for box, r, sigma in (((10.0, 8.0, 30.0, 20.0), 0.0, 0.5), ((10.0, 8.0, 30.0, 20.0), 4.0, 2.0), ((12.0, 12.0, 24.0, 24.0), 6.0, 1.0), ((-5.0, -5.0, 8.0, 50.0), 3.0, 3.0),
                          ((0.0, 0.0, 40.0, 30.0), 20.0, 6.0)):
        s, _ = _s(box, r, sigma, (56, 48), m)
        x, y, w, h = shadow_ref.bounds(box, r, sigma, m, (56, 48))
        inside = np.zeros((48, 56), bool)
        inside[y:y + h, x:x + w] = True
        assert not (~inside).any() or s[~inside].max() < 2.0 ** -12, (box, r, sigma)
    assert shadow_ref.bounds((5.0, 5.0, 5.0, 9.0), 0.0, 1.0, m, (56, 48)) == (0, 0, 0, 0)  # empty in a dimension
    assert shadow_ref.bounds((500.0, 500.0, 540.0, 520.0), 0.0, 1.0, IDENTITY, (56, 48)) == (0, 0, 0, 0)


# ---- box_shadow's CSS arithmetic ----

def test_box_shadows_css_arithmetic():
    g = jello_amd.box_shadow_geometry
    assert g((30.0, 40.0, 90.0, 80.0), 6.0, (4.0, 6.0), 2.0) == ((32.0, 44.0, 96.0, 88.0), 8.0)  # shifted, grown on every side, the radius with it
    assert g((30.0, 40.0, 90.0, 80.0), 0.0, (0.0, 0.0), 5.0) == ((25.0, 35.0, 95.0, 85.0), 0.0)  # a sharp corner stays sharp
    assert g((30.0, 40.0, 90.0, 80.0), 6.0, (-3.0, 0.0), -10.0) == ((37.0, 50.0, 77.0, 70.0), 0.0)  # a negative spread shrinks; the radius not below 0
    assert g((30.0, 40.0, 40.0, 80.0), 2.0, (0.0, 0.0), -8.0) == ((35.0, 48.0, 35.0, 72.0), 0.0)  # shrunk to nothing: the sides meet in the middle
    assert jello_amd.Engine.box_shadow.__doc__ and jello_amd.Engine.shadow.__doc__


# ---- the battery tells the rule from its near misses ----

NEAR_MISSES = {
    "the centre at +0 instead of +0.5": (dict(centre_half=False), "radius_pill"),
    "the half-width at a sub-interval's end, not its midpoint": (dict(midpoint=False), "radius_pill"),
    "an unclamped radius": (dict(clamp_radius=False), "radius_clamped"),
    "K one smaller": (dict(k=3), "radius_disc"),
    "the blend order under OVER": (dict(src_over=False), "radius_pill_over"),
    "sigma not floored": (dict(floor_sigma=False), "sigma_floor_edge_r0"),
    "sigma not floored, round": (dict(floor_sigma=False), "sigma_floor_edge_r3"),
}


@pytest.mark.parametrize("what", sorted(NEAR_MISSES))
def test_the_battery_tells_the_rule_from_a_near_miss(what):
    variant, name = NEAR_MISSES[what]
    want = shadow_cases.expected(name)
    with np.errstate(all="ignore"):
        wrong = shadow_cases.expected(name, **variant)
    assert not same_bits(want, wrong)


def test_the_battery_covers_what_it_claims():
    cases = shadow_cases.CASES
    assert {c["inst"] for c in cases} == {"round/store", "round/over", "sharp/store", "sharp/over"}
    assert {c["size"] for c in cases} >= set(shadow_cases.TILE_SIZES) | {shadow_cases.GRID_SIZE}
    assert max(c["size"][0] * c["size"][1] for c in cases if c["name"] != "grid") <= 200 * 100
    for r, n in shadow_cases.THRESHOLD_RADII:
        assert shadow_ref.plan((12.0, 5.0, 58.0, 29.0), r, shadow_cases.SIGMA)["n"] == n
    assert {c["prior"] for c in cases if c["desc"].get("flags", 0) & OVER} == {"poison", "finite", "never", "nan"}
    partial = shadow_cases.BY_NAME["window_partial"]
    pl = shadow_ref.plan(partial["desc"]["box"], partial["desc"]["radius"], partial["desc"]["sigma"])
    top = float(partial["desc"]["box"][1])
    assert top - 3.5 > float(pl["window"]) and top - 7.5 < float(pl["window"])  # rows 0 .. 3 (one wave) see no cap, rows 4 .. 7 (the next) do


# ---- the stand-alone check ----

def test_the_stand_alone_check_builds_and_passes_and_its_texels_are_the_references(tmp_path):
    """tools/shadow_check.cpp is include/jello_shadow.h with a main of its own: the plan against long double and __int128, G against
    erfl, legality, the bounds by brute force.  Its header has the command with the sanitizers; here it is built without them and
    run, and the coverage it prints for a descriptor -- the text the kernel compiles -- equals the reference's bit for bit."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shadow_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", INCLUDE, os.path.join(ROOT, "tools", "shadow_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.splitlines()[-1].startswith("ok: "), out
    for name in ("radius_pill", "radius_sharp", "matrix_rot30_r6", "matrix_scale_r6", "matrix_flip_r0", "sigma_0.001_r9", "sigma_64_r9", "box_subtexel_r3", "steps_r1.0000001_n8"):
        c = shadow_cases.BY_NAME[name]
        d = dict(shadow_ref.DEFAULTS, **c["desc"])
        w, h = c["size"]
        args = [repr(float(F(v))) for v in d["box"]] + [repr(float(F(d["radius"]))), repr(float(F(d["sigma"])))] + [repr(float(v)) for v in d["matrix"]] + [str(w), str(h)]
        text = subprocess.check_output([exe] + args).decode()
        got = np.array([[int(t, 16) for t in line.split()] for line in text.strip().split("\n")], np.uint32)
        want, _ = _s(d["box"], d["radius"], d["sigma"], (w, h), d["matrix"])
        assert np.array_equal(got, want.view(np.uint32)), name
