"""The warp rule on the CPU: the plan of the library (jh_warp_plan) and of the host twin (jl_warp_plan) against the
reference (tests/warp_ref.py) bit for bit, the legality boundaries, the consequences the rule states, the bounds rectangle, the
reference against the binary64 definition, texels worked by hand, the ctypes mirror, the stand-alone check of include/jello_warp.h
(tools/warp_plan_check.cpp), and that the battery (tests/warp_cases.py) tells the rule from its near misses."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import WarpEdge, WarpFilter, _lib

import warp_cases
import warp_ref
from abi_text import INCLUDE, ROOT, c_values
from warp_ref import BICUBIC, BILINEAR, CLAMP, EDGES, FILTERS, MIRROR, NEAREST, REPEAT, STRAIGHT, ZERO

ONE, HALF, TWO, NEG0 = 0x3C00, 0x3800, 0x4000, 0x8000


def _is_nan(bits):
    return (np.asarray(bits, np.uint16) & 0x7FFF) > 0x7C00


def _f16(values):
    return np.asarray(values, np.float16).view(np.uint16)


def _grey(rows):
    """(h, w, 4) bits from rows of one value per texel, the same in all four channels."""
    return np.repeat(_f16(rows)[..., None], 4, axis=-1)


# ---- the plan: library, host twin and reference ----

def _random_matrices(n, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k, t, sh = math.exp(rng.uniform(-4.0, 8.0)), rng.uniform(-3.2, 3.2), rng.uniform(-1.0, 1.0)
        out.append((k * math.cos(t), k * math.sin(t), k * (sh * math.cos(t) - math.sin(t)), k * (sh * math.sin(t) + math.cos(t)),
                    rng.uniform(-40000.0, 40000.0), rng.uniform(-40000.0, 40000.0)))
    return out


def test_the_plan_of_the_library_and_of_the_twin_is_the_references(built):
    matrices = [c["matrix"] for c in warp_cases.CASES] + _random_matrices(4000)
    legal = 0
    for m in matrices:
        try:
            want = warp_ref.plan(m)
        except ValueError:
            for twin in (False, True):
                with pytest.raises(ValueError):
                    jello_amd.warp_plan(m, twin=twin)
            continue
        legal += 1
        assert jello_amd.warp_plan(m) == want and jello_amd.warp_plan(m, twin=True) == want, m
    assert legal > 3000


def test_the_bounds_of_the_library_and_of_the_twin_are_the_references(built):
    for c in warp_cases.CASES:
        size = warp_cases.rect_of(c, "src")[2:]
        want = warp_ref.bounds(c["matrix"], size, c["filter"], c["dst_size"])
        for twin in (False, True):
            assert jello_amd.warp_bounds(c["matrix"], size, c["filter"], c["dst_size"], twin=twin) == want, c["name"]


LEGALITY = [
    # (legal, illegal, the word of the reason)
    ((1.0, 0.0, 0.0, 1.0, 0.0, 0.0), (math.nan, 0.0, 0.0, 1.0, 0.0, 0.0), "not finite"),
    ((1.0, 0.0, 0.0, 1.0, 1e300, 0.0), (1.0, 0.0, 0.0, 1.0, math.inf, 0.0), "not finite"),
    ((1e150, 0.0, 0.0, 1e150, 0.0, 0.0), (1e200, 0.0, 0.0, 1e200, 0.0, 0.0), "determinant is not finite"),
    ((1.0, 2.0, 2.0, 4.125, 0.0, 0.0), (1.0, 2.0, 2.0, 4.0, 0.0, 0.0), "determinant is 0"),
    ((1.0 / 64.0, 0.0, 0.0, 1.0, 0.0, 0.0), (1.0 / 64.0 * (1.0 - 2.0 ** -50), 0.0, 0.0, 1.0, 0.0, 0.0), "above 64"),
    ((1.0, 0.0, 0.0, 1.0 / 64.0, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0 / 65.0, 0.0, 0.0), "above 64"),
    ((1.0, 0.0, 64.0, 1.0, 0.0, 0.0), (1.0, 0.0, 64.0 + 2.0 ** -40, 1.0, 0.0, 0.0), "above 64"),
    ((1.0, -64.0, 0.0, 1.0, 0.0, 0.0), (1.0, -64.0 - 2.0 ** -40, 0.0, 1.0, 0.0, 0.0), "above 64"),
    ((1.0, 0.0, 0.0, 1.0, 2.0 ** 22, 0.0), (1.0, 0.0, 0.0, 1.0, 2.0 ** 22 + 2.0 ** -20, 0.0), "above 2^22"),
    ((1.0, 0.0, 0.0, 1.0, 0.0, -2.0 ** 22), (1.0, 0.0, 0.0, 1.0, 0.0, -2.0 ** 22 - 2.0 ** -20), "above 2^22"),
]


@pytest.mark.parametrize("k", range(len(LEGALITY)))
def test_the_legality_boundaries_from_both_sides(built, k):
    legal, illegal, word = LEGALITY[k]
    if k == 1:  # (an offset of 1e300 is finite but above 2^22: the finite side of this boundary is illegal for the next reason)
        with pytest.raises(ValueError, match="above 2\\^22"):
            warp_ref.plan(legal)
    else:
        assert jello_amd.warp_plan(legal) == jello_amd.warp_plan(legal, twin=True) == warp_ref.plan(legal)
    with pytest.raises(ValueError, match=word.replace("^", "\\^")):
        warp_ref.plan(illegal)
    hip, L = jello_amd.load_host().hip, jello_amd.load_host()
    m, plan = (ctypes.c_double * 6)(*illegal), (ctypes.c_int64 * 6)(*([77] * 6))
    assert hip.jh_warp_plan(m, plan) == -1 and L.jl_warp_plan(m, plan) == -1 and list(plan) == [77] * 6
    assert word in L.jl_last_error().decode()


def test_the_integers_stay_below_2_to_the_58():
    for m in ((1.0 / 64.0, 1.0 / 64.0, -1.0 / 64.0, 1.0 / 64.0, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0, -2.0 ** 22, 2.0 ** 22)):
        P, Q, R, S, T, W = warp_ref.plan(m)
        for X in (0, 32767):
            for Y in (0, 32767):
                assert abs(P * (2 * X + 1) + Q * (2 * Y + 1) + R) < 2 ** 58 and abs(S * (2 * X + 1) + T * (2 * Y + 1) + W) < 2 ** 58


# ---- the consequences the rule states ----

def _finite(w, h, seed):
    src = warp_cases.content("finite", w, h, seed)
    src[src == NEG0] = 0  # (a -0 comes out as +0: the sums start at +0)
    return src


@pytest.mark.parametrize("filt", FILTERS)
def test_identity_flips_and_quarter_turns_are_permutations(filt):
    src = _finite(13, 9, 3)
    for edge in EDGES:
        for k in range(8):
            shape = (9, 13) if k < 4 else (13, 9)
            got = warp_ref.warp(src, shape, warp_cases.octant(k, 13, 9), filt, edge, STRAIGHT)
            assert np.array_equal(got, warp_cases.octant_permutation(k, src)), (warp_cases.OCTANT_NAMES[k], edge)


@pytest.mark.parametrize("filt", FILTERS)
def test_an_integer_translation_under_zero_is_a_shifted_copy(filt):
    src = _finite(13, 9, 4)
    for tx, ty in ((3, 2), (-4, 1), (0, -8), (20, 0)):
        got = warp_ref.warp(src, (9, 13), warp_cases.translate(tx, ty), filt, ZERO, STRAIGHT)
        want = np.zeros_like(src)
        ys, xs = np.mgrid[0:9, 0:13]
        ok = (ys - ty >= 0) & (ys - ty < 9) & (xs - tx >= 0) & (xs - tx < 13)
        want[ok] = src[(ys - ty)[ok], (xs - tx)[ok]]
        assert np.array_equal(got, want), (tx, ty)


def test_a_constant_image_stays_constant_under_bilinear():
    src = np.full((7, 9, 4), _f16(0.7), np.uint16)
    for edge in (CLAMP, REPEAT, MIRROR):
        for m in (warp_cases.rotate(30, (9, 7), (16383, 5), 1.3), warp_cases.rotate(30, (9, 7), (31, 23), 1.3), (1.0, 0.3, 0.5, 1.0, -2.25, 1.5)):
            got = warp_ref.warp(src, (23, 31), m, BILINEAR, edge, STRAIGHT)
            assert np.all(got == _f16(0.7)), edge


def test_a_doubled_ramp_is_reproduced_exactly():
    """x' = 2 x: destination texel X reads u = (X + 0.5) / 2, and a ramp p[i] = i + 0.5 gives u itself: exact in binary32 and f16."""
    src = _grey([[i + 0.5 for i in range(12)]] * 3)
    for filt, inner in ((BILINEAR, slice(1, 23)), (BICUBIC, slice(3, 21))):
        got = warp_ref.warp(src, (3, 24), (2.0, 0.0, 0.0, 1.0, 0.0, 0.0), filt, CLAMP, STRAIGHT)
        want = _f16([(X + 0.5) / 2.0 for X in range(24)])
        assert np.array_equal(got[1, inner, 0], want[inner]), filt


def test_a_warp_in_four_quadrants_is_the_whole_image_warp():
    src = warp_cases.content("unit", 21, 17, 5)
    m = warp_cases.rotate(30, (21, 17), (27, 19), 1.2)
    for filt in FILTERS:
        whole = warp_ref.warp(src, (19, 27), m, filt, MIRROR)
        parts = None
        for rect in ((0, 0, 13, 9), (13, 0, 14, 9), (0, 9, 13, 10), (13, 9, 14, 10)):
            parts = warp_ref.warp(src, (19, 27), m, filt, MIRROR, dst_rect=rect, dst_bits=parts)
        assert warp_ref.same_bits(parts, whole)


# ---- the bounds rectangle ----

def test_outside_the_bounds_a_zero_warp_is_transparent_black():
    checked = 0
    for c in warp_cases.CASES:
        if c["name"].startswith("big"):
            continue
        src = warp_cases.source(c)
        x, y, w, h = warp_cases.rect_of(c, "src")
        dw, dh = c["dst_size"]
        got = warp_ref.warp(src, (dh, dw), c["matrix"], c["filter"], ZERO, c["flags"], c["src_rect"])
        bx, by, bw, bh = warp_ref.bounds(c["matrix"], (w, h), c["filter"], (dw, dh))
        outside = np.ones((dh, dw), bool)
        outside[by:by + bh, bx:bx + bw] = False
        assert not got[outside].any(), c["name"]
        checked += int(outside.sum())
    assert checked > 20000
    assert warp_ref.bounds(warp_cases.translate(1000, 1000), (41, 29), BILINEAR, (47, 33)) == (0, 0, 0, 0)
    assert warp_ref.bounds(warp_cases.translate(0, 0), (4, 3), NEAREST, (10, 10)) == (0, 0, 6, 5)  # floor(-0.5) - 1 clipped, ceil(4.5) + 1


# ---- the reference against the binary64 definition ----

@pytest.mark.parametrize("filt", [BILINEAR, BICUBIC])
def test_the_reference_is_the_binary64_definition_within_the_rules_roundings(filt):
    """STRAIGHT, CLAMP, random values in [-1, 2) (|p| <= M = 2).  The bound is derived from the rule, not measured.
    Position, per axis: the fraction is truncated to 16 bits, below 2^-16; the coefficients are rounded to 2^-32 half-texels, 2^-32
    ((2 X + 1) + (2 Y + 1)) / 2 + 2^-33; the binary64 inverse evaluated in binary64, below 2^-40 here.  du = their sum.
    Value: the sampled surface is continuous, piecewise polynomial in the position with a slope of at most L per axis -- BILINEAR:
    the largest difference of neighbouring texels on that axis; BICUBIC: sum |w_k'| <= 4 times the other axis's sum |w_k| <= 1.25
    times M -- so the position costs L_x du + L_y dv.  The sums: every fmaf rounds once, 2^-24 of a magnitude of at most A M with
    A = 1 (BILINEAR, convex weights) or 1.25^2 (BICUBIC); there are 6 or 20 of them; a cubic weight is within 5e-7 of its exact
    value (tools/warp_plan_check.cpp asserts it), 8 weights, each on at most 1.25 M.  The store rounds to f16: 2^-11 of the value,
    or 2^-25 below the normal range."""
    src = (np.random.default_rng(21).random((17, 23, 4), dtype=np.float32) * 3.0 - 1.0).astype(np.float16).view(np.uint16)
    sh, sw = src.shape[:2]
    dw, dh = 40, 31
    m = warp_cases.rotate(30, (sw, sh), (dw, dh), 1.3)
    got = warp_ref.warp(src, (dh, dw), m, filt, CLAMP, STRAIGHT).view(np.float16).astype(np.float64)
    want, _ = warp_ref.direct(src, (dh, dw), m, filt, CLAMP, STRAIGHT)
    p = src.view(np.float16).astype(np.float64)
    M = np.abs(p).max()
    assert M <= 2.0
    ys, xs = np.mgrid[0:dh, 0:dw]
    du = 2.0 ** -16 + 2.0 ** -32 * ((2 * xs + 1) + (2 * ys + 1)) / 2.0 + 2.0 ** -33 + 2.0 ** -40
    if filt == BILINEAR:
        Lx, Ly = np.abs(np.diff(p, axis=1)).max(), np.abs(np.diff(p, axis=0)).max()
        sums = 6 * 2.0 ** -24 * M
    else:
        Lx = Ly = 4.0 * 1.25 * M
        sums = 20 * 2.0 ** -24 * 1.25 ** 2 * M + 8 * 5e-7 * 1.25 * M
    before_store = ((Lx + Ly) * du + sums)[..., None]
    bound = before_store + 2.0 ** -11 * (np.abs(want) + before_store) + 2.0 ** -25
    err = np.abs(got - want)
    print("largest error %.3g, at most %.3g of the bound" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    assert err.max() > 0.0


def test_the_fixed_point_position_is_the_inverse_within_the_stated_error():
    m = warp_cases.rotate(30, (9, 7), (16383, 11), 1.3)
    P, Q, R, S, T, W = warp_ref.plan(m)
    ip, iq, ir, _, _, _ = warp_ref.inverse(m)
    from fractions import Fraction
    for X, Y in ((0, 0), (16382, 10), (8000, 3)):
        exact = Fraction(ip) * (Fraction(X) + Fraction(1, 2)) + Fraction(iq) * (Fraction(Y) + Fraction(1, 2)) + Fraction(ir)
        fixed = Fraction(P * (2 * X + 1) + Q * (2 * Y + 1) + R, 2 ** 32)
        assert abs(fixed - exact) <= Fraction((2 * X + 1) + (2 * Y + 1), 2 ** 33) + Fraction(1, 2 ** 33)


# ---- texels worked by hand ----

def test_texels_by_hand():
    src = _grey([[0.0, 1.0], [2.0, 4.0]])
    # a quarter-texel translation: destination (0, 0) reads u = v = 0.25, U' = -2^30: i0 = -1 (a floor), f = 0.75
    t = warp_cases.translate(0.25, 0.25)
    assert warp_ref.warp(src, (2, 2), t, NEAREST, ZERO, STRAIGHT)[0, 0, 0] == _f16(0.0)
    got = warp_ref.warp(src, (2, 2), t, BILINEAR, CLAMP, STRAIGHT)[..., 0].view(np.float16)
    # (1, 1) reads u = v = 1.25: i0 = 0, f = 0.75: rows 0.75, 3.5, then 0.25 x 0.75 + 0.75 x 3.5
    assert got[0, 0] == 0.0 and got[1, 1] == np.float16(0.25 * 0.75 + 0.75 * 3.5)
    zero = warp_ref.warp(src, (2, 2), t, BILINEAR, ZERO, STRAIGHT)[..., 0].view(np.float16)
    assert zero[0, 0] == 0.0 and zero[0, 1] == np.float16(0.75 * (0.25 * 0.0 + 0.75 * 1.0))  # the row above is +0 with weight 0.25
    # the index rules at tap -1 and tap 2 of a two-texel axis
    assert [int(warp_ref.index(e, -1, 2)) for e in EDGES] == [-1, 0, 1, 0] and [int(warp_ref.index(e, 2, 2)) for e in EDGES] == [-1, 1, 0, 1]
    assert [int(warp_ref.index(MIRROR, i, 3)) for i in range(-7, 8)] == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert [int(warp_ref.index(REPEAT, i, 3)) for i in range(-4, 5)] == [2, 0, 1, 2, 0, 1, 2, 0, 1]
    # the cubic weights at f = 0 and f = 0.5
    w = [float(v) for v in warp_ref.cubic_weights(np.float32(0.0))]
    assert w == [0.0, 1.0, 0.0, 0.0] and math.copysign(1.0, w[0]) == -1.0  # (w0 = -0: it still multiplies, and changes nothing)
    assert [float(v) for v in warp_ref.cubic_weights(np.float32(0.5))] == [-0.0625, 0.5625, 0.5625, -0.0625]
    # premultiplied: (colour 1, alpha 0.5) next to (colour 0.5, alpha 1) halfway: (0.5 + 0.5) / 2 over alpha 0.75
    pair = np.array([[[ONE, ONE, ONE, HALF], [HALF, HALF, HALF, ONE]]], np.uint16)
    out = warp_ref.warp(pair, (1, 1), warp_cases.translate(-0.5, 0.0), BILINEAR, CLAMP)[0, 0].view(np.float16)
    assert out[3] == np.float16(0.75) and out[0] == np.float16(np.float32(0.5) * (np.float32(1.0) / np.float32(0.75)))
    # nothing is clamped: BICUBIC overshoots a step
    step = _grey([[0.0, 0.0, 1.0, 1.0]])
    over = warp_ref.warp(step, (1, 8), (2.0, 0.0, 0.0, 1.0, 0.0, 0.0), BICUBIC, CLAMP, STRAIGHT)[0, :, 0].view(np.float16)
    assert over.max() > 1.0 and over.min() < 0.0


def test_the_refusals_of_the_reference():
    src = warp_cases.content("unit", 6, 4, 1)
    ident = warp_cases.translate(0, 0)
    for kw in (dict(filt=3), dict(edge=4), dict(flags=2), dict(src_rect=(0, 0, 7, 4)), dict(dst_rect=(1, 1, 0, 2)), dict(dst_rect=(0, 0, 9, 1)),
               dict(matrix=(0.0,) * 6), dict(matrix=(1.0, 0.0, 0.0, 1.0, math.inf, 0.0))):
        args = dict(matrix=ident, filt=BILINEAR, edge=ZERO, flags=0, src_rect=None, dst_rect=None)
        args.update(kw)
        with pytest.raises(ValueError):
            warp_ref.warp(src, (5, 8), args["matrix"], args["filt"], args["edge"], args["flags"], args["src_rect"], args["dst_rect"])


# ---- the C ABI without a device ----

def test_the_headers_constants_and_the_mirrors_layout():
    names = ["JH_WARP_NEAREST", "JH_WARP_BILINEAR", "JH_WARP_BICUBIC", "JH_WARP_EDGE_ZERO", "JH_WARP_EDGE_CLAMP", "JH_WARP_EDGE_REPEAT",
             "JH_WARP_EDGE_MIRROR", "JH_WARP_STRAIGHT", "JH_WARP_MAX_SIDE"]
    assert c_values(names) == [0, 1, 2, 0, 1, 2, 3, 1, 32768]
    assert [int(f) for f in WarpFilter] == list(FILTERS) and [int(e) for e in WarpEdge] == list(EDGES)
    assert (jello_amd.engine.WARP_STRAIGHT, jello_amd.engine.WARP_MAX_SIDE) == (STRAIGHT, warp_ref.MAX_SIDE)
    fields = ["matrix", "filter", "edge", "flags", "src_x", "src_y", "src_width", "src_height", "dst_x", "dst_y", "dst_width", "dst_height"]
    assert [name for name, _ in _lib.CWarpDesc._fields_] == fields
    want = c_values(["sizeof(jh_warp_desc)"] + ["offsetof(jh_warp_desc, %s)" % f for f in fields])
    assert [ctypes.sizeof(_lib.CWarpDesc)] + [getattr(_lib.CWarpDesc, f).offset for f in fields] == want


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    d = jello_amd.engine._warp_desc(warp_cases.translate(1, 2), WarpFilter.BICUBIC, WarpEdge.MIRROR, (1, 2, 3, 4), None, False)
    assert (list(d.matrix), d.filter, d.edge, d.flags) == ([1.0, 0.0, 0.0, 1.0, 1.0, 2.0], 2, 3, 1)
    assert (d.src_x, d.src_y, d.src_width, d.src_height, d.dst_x, d.dst_y, d.dst_width, d.dst_height) == (1, 2, 3, 4, 0, 0, 0, 0)
    assert hip.jh_warp(None, 1, 2, ctypes.byref(d)) == -1  # JH_ERR_INVALID
    assert hip.jh_warp(None, 1, 2, None) == -1
    assert hip.jh_warp_plan(None, None) == -1 and hip.jh_warp_bounds(None, 1, 1, 0, 1, 1, None) == -1
    with pytest.raises(ValueError):
        jello_amd.warp_bounds(warp_cases.translate(0, 0), (4, 4), 3, (4, 4))
    with pytest.raises(ValueError):
        jello_amd.warp_bounds(warp_cases.translate(0, 0), (4, 32769), 0, (4, 4))


def test_the_stand_alone_check_builds_and_passes(tmp_path):
    """tools/warp_plan_check.cpp is include/jello_warp.h with a main of its own: legal and illegal matrices, the plan against
    __int128 arithmetic, the index rules against a walk, the bounds against the plan.  Its header has the command with the
    sanitizers; here it is built without them and run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "warp_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", INCLUDE, os.path.join(ROOT, "tools", "warp_plan_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok: "), out


# ---- sensitivity: the battery tells the rule from its near misses ----

NEAR_MISSES = {
    # variant: (the keyword that builds it, the case of the battery that catches it)
    "truncation instead of floor": (dict(floor=False), "shear_bilinear_repeat_straight_41x29_to_47x33_finite"),
    "the fraction rounded instead of truncated": (dict(frac_round=True), "frac-0.0000114441_bicubic_repeat_straight_23x9_to_25x11_finite"),
    "coefficients at 2^-16": (dict(coef_bits=16), "up3.7_bilinear_zero_straight_17x13_to_64x48_finite"),
    "columns before rows": (dict(rows_first=False), "down2_bicubic_mirror_premul_64x48_to_32x24_unit"),
    "multiply then add instead of fmaf": (dict(fused=False), "down2_bicubic_mirror_premul_64x48_to_32x24_unit"),
    "MIRROR with period 2 n - 2": (dict(mirror_2n=False), "far_bilinear_mirror_premul_3x3_to_40x30_unit"),
    "the image as the edge instead of the rectangle": (dict(edge_rect=False), "rect_bicubic_clamp_straight_36x20_r1_1_21_9_to_64x40_r7_1_39_35_finite"),
    "straight operands where premultiplied are asked for": (dict(premultiply=False), "up2_bilinear_clamp_premul_32x24_to_64x48_unit"),
}


@pytest.mark.parametrize("what", sorted(NEAR_MISSES))
def test_the_battery_tells_the_rule_from_a_near_miss(what):
    variant, name = NEAR_MISSES[what]
    want, got = warp_cases.expected(name), warp_cases.expected(name, **variant)
    differ = int(np.count_nonzero((want != got) & ~(_is_nan(want) & _is_nan(got))))
    print("%s: %d of %d values differ on %s" % (what, differ, want.size, name))
    assert differ > 0, (what, name)


def test_the_battery_covers_what_it_claims():
    cases = warp_cases.CASES
    assert len(cases) > 250
    assert all(max(c["src_size"] + c["dst_size"]) <= 64 and min(c["src_size"][1], c["dst_size"][1]) <= 48 for c in cases if not c["name"].startswith("big"))
    big = [c for c in cases if c["name"].startswith("big")]
    assert len(big) == 1 and (big[0]["filter"], big[0]["edge"]) == (BILINEAR, ZERO)
    bw, bh = big[0]["dst_size"]
    assert ((bw + 30) // 16) * ((bh + 15) // 16) > 8 * 256  # more tiles than the launcher's grid has workgroups
    for w in warp_cases.ITEM_WIDTHS:
        assert any(c["dst_size"][0] == w for c in cases), w
    for h in warp_cases.ITEM_HEIGHTS:
        assert any(c["dst_size"][1] == h for c in cases), h
    assert any(c["dst_size"] == (1, 1) for c in cases) and any(c["dst_size"][1] == 1 and c["dst_size"][0] > 1 for c in cases)
    for filt in FILTERS:
        for edge in EDGES:
            for flags in (0, STRAIGHT):
                assert any((c["filter"], c["edge"], c["flags"]) == (filt, edge, flags) for c in cases)
    for kind in warp_cases.KINDS:
        assert any(c["kind"] == kind for c in cases), kind
    assert any(c["prior"] == "never" for c in cases)
    assert any(c["dst_rect"] is not None and c["dst_rect"][0] % 2 and c["dst_rect"][1] % 2 for c in cases)
    assert any(c["src_rect"] is not None and c["src_rect"][0] % 2 and c["src_rect"][1] % 2 for c in cases)
    for n in (1, 2, 3):
        for edge in (REPEAT, MIRROR):
            assert any(c["src_size"][0] == n and c["edge"] == edge for c in cases)
    assert any(abs(v) == 64 * 2 ** 31 for c in cases for v in warp_ref.plan(c["matrix"])[:2])  # the legal limit
    # U at, just below and just above a multiple of 2^32; U' negative; fractions 0x0000 and 0xffff
    low = set()
    fracs = set()
    for c in cases:
        P, Q, R = warp_ref.plan(c["matrix"])[:3]
        U = P + Q + R  # texel (0, 0)
        if c["filter"] == NEAREST:
            low.add(U & 0xFFFFFFFF)
        else:
            fracs.add(((U - 2 ** 31) >> 16) & 0xFFFF)
            low.add("negative" if U - 2 ** 31 < 0 else "positive")
    assert {0, 1, 0xFFFFFFFF, "negative", "positive"} <= low and {0, 0xFFFF} <= fracs
    nonfinite = warp_cases.content("infalpha0", 37, 11, seed=1)
    assert ((nonfinite[..., 0] == 0x7C00) & (nonfinite[..., 3] == 0)).any()
    assert (warp_cases.content("negalpha", 37, 11, seed=1)[..., 3] & 0x8000).any()
