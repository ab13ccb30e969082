"""The displacement rule on the CPU: the offset of the library (jh_displace_offset) and of the host twin
(jl_displace_offset) against the reference (tests/displace_ref.py) over every f16 bit pattern, bit for bit; the ctypes mirror; the
legality boundaries; texels worked by hand; the consequences the rule states; the reference's position against the exact rational
one and its values against the binary64 definition at the same positions; the stand-alone check of include/jello_displace.h
(tools/displace_check.cpp); and that the battery (tests/displace_cases.py) tells the rule from its near misses."""
import ctypes
import inspect
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import jello_amd
from jello_amd import DisplaceChannel, WarpEdge, WarpFilter, _lib

import displace_cases
import displace_ref
import warp_cases
import warp_ref
from abi_text import INCLUDE, ROOT, c_values
from displace_ref import A, B, G, IDENTITY, R
from warp_ref import BICUBIC, BILINEAR, CLAMP, EDGES, FILTERS, MIRROR, NEAREST, REPEAT, STRAIGHT, ZERO

ONE, HALF = 0x3C00, 0x3800
SCALES = [0.0, -0.0, 1.0, -1.0, 0.5, 20.0, -7.3, 256.0, 1e-3, math.pi, 1e30, -1e30, 2.0 ** 23, 2.0 ** 23 + 1.0, -2.0 ** 23, 128.06, 1e-30, 1e-44,
          2.0 ** -32, 2.0 ** -22, 3 * 2.0 ** -22, 3.4028234663852886e38, 2.0 ** 22, 65.0078125]


def _is_nan(bits):
    return (np.asarray(bits, np.uint16) & 0x7FFF) > 0x7C00


def _f16(values):
    return np.asarray(values, np.float16).view(np.uint16)


def _grey(rows):
    return np.repeat(_f16(rows)[..., None], 4, axis=-1)


def _const_map(shape, bits):
    return np.full(tuple(shape) + (4,), bits, np.uint16)


# ---- the offset: library, host twin and reference ----

@pytest.mark.parametrize("twin", [False, True])
def test_the_offset_of_the_library_and_of_the_twin_is_the_references(built, twin):
    """Every f16 bit pattern x the scale list, bit for bit."""
    L = jello_amd.load_host()
    f = L.jl_displace_offset if twin else L.hip.jh_displace_offset
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    out = ctypes.c_int64(0)
    for s in SCALES:
        want = displace_ref.offset(s, bits)
        got = np.empty(65536, np.int64)
        c = float(np.float32(s))
        for h in range(65536):
            f(c, h, ctypes.byref(out))
            got[h] = out.value
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (s, hex(int(bad[0])), int(got[bad[0]]), int(want[bad[0]]))
    assert f(1.0, 0, None) == -1
    assert jello_amd.displace_offset(20.0, ONE, twin=twin) == 10 << 32


def test_the_offset_by_hand():
    off = lambda s, h: int(displace_ref.offset(s, np.uint16(h)))  # noqa: E731
    assert off(20.0, ONE) == 10 << 32 and off(20.0, 0) == -(10 << 32) and off(20.0, HALF) == 0 and off(-4.0, 0x3400) == 1 << 32  # m = 0.25
    # the rounding of D: t = 2^-11; 2^-22 t 2^32 = 0.5 -> 0, 3 x 2^-22: 1.5 -> 2 (ties to even), and their negatives
    assert [off(k * 2.0 ** -22, 0x3801) for k in (1, 3, 5, -1, -3)] == [0, 2, 2, 0, -2]
    assert [int(displace_ref.offset(k * 2.0 ** -22, np.uint16(0x3801), trunc=True)) for k in (3, -3)] == [1, -1]
    # the clamp from both sides, NaN, Inf, 0 x Inf
    top = 1 << 54
    assert off(1e30, ONE) == top and off(1e30, 0) == -top and off(2.0 ** 23, ONE) == top and off(2.0 ** 23 - 0.5, ONE) == top - (1 << 30)
    assert off(1.0, 0x7C00) == top and off(1.0, 0xFC00) == -top and off(0.0, 0x7C00) == 0 and off(3.0, 0x7E00) == 0 and off(-0.0, 0x4000) == 0
    # t is exact for every finite f16: the binary32 difference is the binary64 one
    finite = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    finite = finite[(finite & 0x7C00) != 0x7C00]
    m = finite.view(np.float16)
    assert np.array_equal((m.astype(np.float32) - np.float32(0.5)).astype(np.float64), m.astype(np.float64) - 0.5)


# ---- the C ABI without a device ----

def test_the_headers_constants_and_the_mirrors_layout():
    names = ["JH_DISPLACE_R", "JH_DISPLACE_G", "JH_DISPLACE_B", "JH_DISPLACE_A", "JH_DISPLACE_STRAIGHT"]
    assert c_values(names) == [0, 1, 2, 3, 1]
    assert [int(c) for c in DisplaceChannel] == [R, G, B, A] and jello_amd.engine.DISPLACE_STRAIGHT == STRAIGHT
    fields = ["matrix", "filter", "edge", "flags", "src_x", "src_y", "src_width", "src_height", "dst_x", "dst_y", "dst_width", "dst_height", "scale_x",
              "scale_y", "x_channel", "y_channel"]
    assert [name for name, _ in _lib.CDisplaceDesc._fields_] == fields
    want = c_values(["sizeof(jh_displace_desc)"] + ["offsetof(jh_displace_desc, %s)" % f for f in fields])
    assert [ctypes.sizeof(_lib.CDisplaceDesc)] + [getattr(_lib.CDisplaceDesc, f).offset for f in fields] == want


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    d = jello_amd.engine._displace_desc((3.0, -2.0), DisplaceChannel.A, DisplaceChannel.B, warp_cases.translate(1, 2), WarpFilter.BICUBIC, WarpEdge.MIRROR,
                                        (1, 2, 3, 4), None, False)
    assert (list(d.matrix), d.filter, d.edge, d.flags) == ([1.0, 0.0, 0.0, 1.0, 1.0, 2.0], 2, 3, 1)
    assert (d.src_x, d.src_y, d.src_width, d.src_height, d.dst_x, d.dst_y, d.dst_width, d.dst_height) == (1, 2, 3, 4, 0, 0, 0, 0)
    assert (d.scale_x, d.scale_y, d.x_channel, d.y_channel) == (3.0, -2.0, 3, 2)
    one = jello_amd.engine._displace_desc(1.5, 0, 1, IDENTITY, 1, 0, None, None, True)
    assert (one.scale_x, one.scale_y, one.flags) == (1.5, 1.5, 0)  # a scalar scale means both axes
    assert inspect.signature(jello_amd.Engine.displace).parameters["matrix"].default == IDENTITY  # what feDisplacementMap needs
    assert hip.jh_displace(None, 1, 2, 3, ctypes.byref(d)) == -1  # JH_ERR_INVALID
    assert hip.jh_displace(None, 1, 2, 3, None) == -1
    assert hip.jh_displace_offset(1.0, 0, None) == -1


# ---- legality, from both sides of every boundary ----

def _ref_call(**kw):
    args = dict(scale=1.0, x_channel=R, y_channel=G, matrix=IDENTITY, filt=BILINEAR, edge=ZERO, flags=0, src_rect=None, dst_rect=None, map_shape=(5, 8))
    args.update(kw)
    src = warp_cases.content("unit", 6, 4, 1)
    m = _const_map(args.pop("map_shape"), HALF)
    return displace_ref.displace(src, m, (5, 8), args.pop("scale"), args.pop("x_channel"), args.pop("y_channel"), args.pop("matrix"), **args)


LEGALITY = [
    # (legal, illegal, a word of the reason)
    (dict(filt=2), dict(filt=3), "filter"),
    (dict(edge=3), dict(edge=4), "filter, edge"),
    (dict(flags=1), dict(flags=2), "flag"),
    (dict(x_channel=3), dict(x_channel=4), "channel"),
    (dict(y_channel=0), dict(y_channel=-1), "channel"),
    (dict(scale=3.4028234663852886e38), dict(scale=math.inf), "scale is not finite"),
    (dict(scale=(0.0, -3.4028234663852886e38)), dict(scale=(0.0, -math.inf)), "scale is not finite"),
    (dict(scale=(1.0, 1e-45)), dict(scale=(1.0, math.nan)), "scale is not finite"),
    (dict(map_shape=(5, 8)), dict(map_shape=(5, 9)), "map's size"),
    (dict(map_shape=(5, 8)), dict(map_shape=(4, 8)), "map's size"),
    (dict(matrix=(1.0, 0.0, 0.0, 1.0 / 64.0, 0.0, 0.0)), dict(matrix=(1.0, 0.0, 0.0, 1.0 / 65.0, 0.0, 0.0)), "above 64"),
    (dict(matrix=(1.0, 0.0, 0.0, 1.0, 2.0 ** 22, 0.0)), dict(matrix=(1.0, 0.0, 0.0, 1.0, 2.0 ** 22 + 2.0 ** -20, 0.0)), "above 2\\^22"),
    (dict(src_rect=(0, 0, 6, 4)), dict(src_rect=(0, 0, 7, 4)), "rectangle"),
    (dict(dst_rect=(1, 1, 7, 4)), dict(dst_rect=(1, 1, 0, 2)), "rectangle"),
]


@pytest.mark.parametrize("k", range(len(LEGALITY)))
def test_the_legality_boundaries_from_both_sides(k):
    legal, illegal, word = LEGALITY[k]
    assert _ref_call(**legal).shape == (5, 8, 4)
    with pytest.raises(ValueError, match=word):
        _ref_call(**illegal)


# ---- texels worked by hand ----

def test_texels_by_hand():
    ramp = _grey([[float(i) for i in range(8)]] * 3)  # texel i holds i
    # a constant map of 1.0 under scale (4, 0): t = 0.5, d = 2: every texel reads two texels to its right
    got = displace_ref.displace(ramp, _const_map((3, 8), ONE), (3, 8), (4.0, 0.0), filt=NEAREST, edge=ZERO, flags=STRAIGHT)[1, :, 0].view(np.float16)
    assert list(got) == [2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 0.0, 0.0]
    # a map of 0.75 under scale 2: d = 0.5, halfway between texels X and X + 1 under BILINEAR; CLAMP holds the last
    got = displace_ref.displace(ramp, _const_map((3, 8), _f16(0.75)), (3, 8), (2.0, 0.0), filt=BILINEAR, edge=CLAMP, flags=STRAIGHT)[1, :, 0].view(np.float16)
    assert list(got) == [0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.0]
    # the y channel moves the rows: scale (0, -2) and a map of 1.0 read the row above; the x channel's value is not looked at under scale 0
    rows = _grey([[1.0] * 4, [2.0] * 4, [3.0] * 4])
    m = _const_map((3, 4), ONE)
    m[..., R] = 0x7C00
    got = displace_ref.displace(rows, m, (3, 4), (0.0, -2.0), filt=NEAREST, edge=REPEAT, flags=STRAIGHT)[:, 0, 0].view(np.float16)
    assert list(got) == [3.0, 1.0, 2.0]
    # a per-texel map: texel X reads X + 2 (m_x - 0.5) with m = 0, 0.5, 1 in turn
    m = _const_map((3, 8), HALF)
    m[..., R] = np.array([0x0000, HALF, ONE, 0x0000, HALF, ONE, 0x0000, HALF], np.uint16)[None, :]
    got = displace_ref.displace(ramp, m, (3, 8), 2.0, filt=NEAREST, edge=ZERO, flags=STRAIGHT)[1, :, 0].view(np.float16)
    assert list(got) == [0.0, 1.0, 3.0, 2.0, 4.0, 6.0, 5.0, 7.0]  # (texel 0 reads -1: outside, +0)
    # the map is read as stored: colour 1.0 under alpha 0 still displaces (a premultiplied reading would give t = -0.5)
    m = _const_map((3, 8), ONE)
    m[..., A] = 0
    got = displace_ref.displace(ramp, m, (3, 8), (4.0, 0.0), filt=NEAREST, edge=ZERO)[1, :, 3].view(np.float16)
    assert list(got) == [2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 0.0, 0.0]
    # a never-written map reads 0: t = -0.5
    got = displace_ref.displace(ramp, None, (3, 8), (2.0, 0.0), filt=NEAREST, edge=CLAMP, flags=STRAIGHT)[1, :, 0].view(np.float16)
    assert list(got) == [0.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]


# ---- the consequences the rule states ----

@pytest.mark.parametrize("filt", FILTERS)
def test_scale_zero_and_a_half_map_are_the_warp(filt):
    src = warp_cases.content("unit", 21, 17, 5)
    rng_map = displace_cases.map_bits("values", 27, 19, 3)
    half = _const_map((19, 27), HALF)
    for edge in EDGES:
        for flags in (0, STRAIGHT):
            for m in (warp_cases.rotate(30, (21, 17), (27, 19), 1.2), warp_cases.translate(0.5, -2.0)):
                want = warp_ref.warp(src, (19, 27), m, filt, edge, flags)
                assert np.array_equal(displace_ref.displace(src, rng_map, (19, 27), 0.0, matrix=m, filt=filt, edge=edge, flags=flags), want)
                assert np.array_equal(displace_ref.displace(src, rng_map, (19, 27), -0.0, B, A, matrix=m, filt=filt, edge=edge, flags=flags), want)
                assert np.array_equal(displace_ref.displace(src, half, (19, 27), (1e30, -77.0), A, R, matrix=m, filt=filt, edge=edge, flags=flags), want)


@pytest.mark.parametrize("filt", FILTERS)
def test_a_constant_map_with_an_integer_product_is_the_integer_translation(filt):
    src = warp_cases.content("finite", 13, 9, 4)
    src[src == 0x8000] = 0
    for (sx, sy), bits, (tx, ty) in (((6.0, -4.0), ONE, (-3, 2)), ((8.0, 8.0), 0x3400, (2, 2)), ((-2.0, 10.0), 0x4000, (3, -15))):  # m = 1, 0.25, 2
        got = displace_ref.displace(src, _const_map((9, 13), bits), (9, 13), (sx, sy), filt=filt, edge=ZERO, flags=STRAIGHT)
        assert np.array_equal(got, warp_ref.warp(src, (9, 13), warp_cases.translate(tx, ty), filt, ZERO, STRAIGHT)), (sx, sy)
        want = np.zeros_like(src)
        ys, xs = np.mgrid[0:9, 0:13]
        ok = (ys - ty >= 0) & (ys - ty < 9) & (xs - tx >= 0) & (xs - tx < 13)
        want[ok] = src[(ys - ty)[ok], (xs - tx)[ok]]
        assert np.array_equal(got, want), (sx, sy)


def test_a_call_in_four_quadrants_is_the_whole_image_call():
    src = warp_cases.content("unit", 21, 17, 5)
    dmap = displace_cases.map_bits("random", 27, 19, 9)
    m = warp_cases.rotate(30, (21, 17), (27, 19), 1.2)
    for filt in FILTERS:
        whole = displace_ref.displace(src, dmap, (19, 27), (5.0, -3.0), matrix=m, filt=filt, edge=MIRROR)
        parts = None
        for rect in ((0, 0, 13, 9), (13, 0, 14, 9), (0, 9, 13, 10), (13, 9, 14, 10)):
            parts = displace_ref.displace(src, dmap, (19, 27), (5.0, -3.0), matrix=m, filt=filt, edge=MIRROR, dst_rect=rect, dst_bits=parts)
        assert displace_ref.same_bits(parts, whole)
        # and with the map being dst: each quadrant reads the map texels it is about to overwrite, and no others
        inplace = dmap
        for rect in ((0, 0, 13, 9), (13, 0, 14, 9), (0, 9, 13, 10), (13, 9, 14, 10)):
            inplace = displace_ref.displace(src, inplace, (19, 27), (5.0, -3.0), matrix=m, filt=filt, edge=MIRROR, dst_rect=rect, dst_bits=inplace)
        assert displace_ref.same_bits(inplace, whole)


def test_under_a_translation_the_displacement_is_in_destination_space_too():
    """The displacement is added after the affine map, in texels of the source rectangle.  Under a translation that is the same as
    displacing in destination space; under a 2 x scale a destination-space displacement of d is a source-space one of d / 2."""
    src = warp_cases.content("unit", 24, 17, 6)
    dmap = displace_cases.map_bits("random", 48, 34, 2)
    up = displace_ref.displace(src, dmap, (34, 48), 8.0, matrix=warp_cases.scale(2), filt=BILINEAR, edge=CLAMP)
    _, (U, V) = displace_ref.direct(src, dmap, (34, 48), 8.0, matrix=warp_cases.scale(2), filt=BILINEAR, edge=CLAMP)
    U0, V0 = warp_ref.positions(warp_ref.plan(warp_cases.scale(2)), (0, 0, 48, 34))
    assert np.array_equal(U - U0, displace_ref.offset(8.0, dmap[..., R])) and np.abs(U - U0).max() > 3 << 32  # source texels, not halved
    assert up.shape == (34, 48, 4)


# ---- the reference's position and values ----

def test_the_position_is_the_exact_one_within_the_stated_error():
    """Exact: p (X + 1/2) + q (Y + 1/2) + r + d with the binary64 inverse (p, q, r) and d the rule's clamped binary32 product, all as
    rationals.  The plan's coefficients are rounded to 2^-32 half-texels and its offset to 2^-32 texel: ((2 X + 1) + (2 Y + 1)) 2^-33 +
    2^-33 (5.12); D = rint(d 2^32) adds 2^-33."""
    m = warp_cases.rotate(30, (9, 7), (16383, 11), 1.3)
    P, Q, Rr, S, T, W = warp_ref.plan(m)
    ip, iq, ir, is_, it, iw = warp_ref.inverse(m)
    worst = Fraction(0)
    for X, Y, bits, scale in ((0, 0, 0x3555, 7.3), (16382, 10, 0x3BFF, -977.13), (8000, 3, 0x0001, 1e-3), (5, 9, 0x7BFF, 1e30), (77, 2, 0xC500, 3.0)):
        with np.errstate(all="ignore"):
            d = np.float32(scale) * (np.array(bits, np.uint16).view(np.float16).astype(np.float32) - np.float32(0.5))
        d = Fraction(float(np.clip(d, -2.0 ** 22, 2.0 ** 22)))
        D = int(displace_ref.offset(scale, np.uint16(bits)))
        for (a, b, c), (A_, B_, C_) in (((ip, iq, ir), (P, Q, Rr)), ((is_, it, iw), (S, T, W))):
            exact = Fraction(a) * (Fraction(X) + Fraction(1, 2)) + Fraction(b) * (Fraction(Y) + Fraction(1, 2)) + Fraction(c) + d
            fixed = Fraction(A_ * (2 * X + 1) + B_ * (2 * Y + 1) + C_ + D, 2 ** 32)
            bound = Fraction((2 * X + 1) + (2 * Y + 1), 2 ** 33) + Fraction(1, 2 ** 33) + Fraction(1, 2 ** 33)
            assert abs(fixed - exact) <= bound
            worst = max(worst, abs(fixed - exact) / bound)
    print("at most %.3f of the bound" % float(worst))


@pytest.mark.parametrize("filt", [BILINEAR, BICUBIC])
def test_the_reference_is_the_binary64_definition_at_the_same_positions(filt):
    """STRAIGHT, CLAMP, values in [-1, 2) (|p| <= M = 2), a random map under scale (9, -6.5).  `direct` samples in binary64 at the
    rule's own int64 positions with the whole 32-bit fraction, so the position costs only the fraction's truncation to 16 bits, below
    2^-16 per axis, times the local slope L (5.12: BILINEAR the largest difference of neighbouring texels on that axis; BICUBIC sum
    |w_k'| <= 4 times the other axis's sum |w_k| <= 1.25 times M) -- and no texel has to be left out near a cell boundary, because both
    sides take the index from the same integer.  The sums are 5.12's: every fmaf rounds once, 2^-24 of at most A M (A = 1 or 1.25^2), 6
    or 20 of them; a cubic weight is within 5e-7 of its exact value, 8 weights on at most 1.25 M.  The store: 2^-11 of the value, or
    2^-25 below the normal range."""
    src = (np.random.default_rng(21).random((17, 23, 4), dtype=np.float32) * 3.0 - 1.0).astype(np.float16).view(np.uint16)
    dmap = displace_cases.map_bits("random", 40, 31, 8)
    args = dict(matrix=warp_cases.rotate(30, (23, 17), (40, 31), 1.3), filt=filt, edge=CLAMP, flags=STRAIGHT)
    got = displace_ref.displace(src, dmap, (31, 40), (9.0, -6.5), **args).view(np.float16).astype(np.float64)
    want, _ = displace_ref.direct(src, dmap, (31, 40), (9.0, -6.5), **args)
    p = src.view(np.float16).astype(np.float64)
    M = np.abs(p).max()
    assert M <= 2.0
    du = 2.0 ** -16
    if filt == BILINEAR:
        Lx, Ly = np.abs(np.diff(p, axis=1)).max(), np.abs(np.diff(p, axis=0)).max()
        sums = 6 * 2.0 ** -24 * M
    else:
        Lx = Ly = 4.0 * 1.25 * M
        sums = 20 * 2.0 ** -24 * 1.25 ** 2 * M + 8 * 5e-7 * 1.25 * M
    before_store = (Lx + Ly) * du + sums
    bound = before_store + 2.0 ** -11 * (np.abs(want) + before_store) + 2.0 ** -25
    err = np.abs(got - want)
    print("largest error %.3g, at most %.3g of the bound" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    assert err.max() > 0.0


def test_nearest_is_the_binary64_definition_exactly():
    src = warp_cases.content("finite", 23, 17, 2)
    dmap = displace_cases.map_bits("wide", 40, 31, 8)
    args = dict(matrix=warp_cases.rotate(30, (23, 17), (40, 31), 1.3), filt=NEAREST, edge=MIRROR, flags=STRAIGHT)
    got = displace_ref.displace(src, dmap, (31, 40), 30.0, **args)
    want, _ = displace_ref.direct(src, dmap, (31, 40), 30.0, **args)
    with np.errstate(all="ignore"):
        assert displace_ref.same_bits(got, want.astype(np.float16).view(np.uint16))  # (a -0 comes out as +0 on both sides: the sums start at +0)


# ---- the stand-alone check ----

def test_the_stand_alone_check_builds_and_passes(tmp_path):
    """tools/displace_check.cpp is include/jello_displace.h with a main of its own: jdisp_offset over every bit pattern x a list of
    scales against long double and __int128, the clamp from both sides, NaN, the legality boundaries.  Its header has the command
    with the sanitizers; here it is built without them and run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "displace_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", INCLUDE, os.path.join(ROOT, "tools", "displace_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok: "), out


# ---- sensitivity: the battery tells the rule from its near misses ----

NEAR_MISSES = {
    # variant: (the keyword that builds it, the case of the battery that catches it)
    "t rounded after the product instead of before": (dict(t_after=True), "odd_bilinear_clamp_straight_47x33_to_47x33_finite_s977.13_-128.06_rg_random_own"),
    "truncation instead of rint": (dict(trunc=True), "rint_nearest_repeat_straight_23x9_to_23x9_finite_s7.15256e-07_7.15256e-07_rb_edges_own"),
    "no clamp": (dict(clamp=False), "far_bicubic_repeat_premul_3x3_to_33x17_unit_s1e+30_977_rg_wide_own"),
    "NaN not zeroed": (dict(nan_zero=False), "values_bilinear_repeat_premul_47x33_to_47x33_unit_s3_3_rb_values_own"),
    "the map read premultiplied": (dict(map_premultiplied=True), "channels_bilinear_clamp_premul_19x13_to_19x13_finite_s6_5_rr_wide_own"),
    "x and y channels swapped": (dict(swap_channels=True), "all_nearest_clamp_premul_41x29_to_47x33_finite_s5_5_ba_random_own"),
    "the fraction taken before the half-texel shift": (dict(frac_unshifted=True), "identity_bilinear_zero_premul_47x33_to_47x33_unit_s6_4_rg_random_own"),
    "the map sampled at the source position": (dict(map_at_source=True), "t3_-2_bicubic_clamp_premul_47x33_to_47x33_unit_s6_4_rg_random_own"),
    "ties away from zero instead of to even": (dict(ties_away=True), "rint1_nearest_repeat_straight_23x9_to_23x9_finite_s2.38419e-07_2.38419e-07_rb_edges_own"),
}


@pytest.mark.parametrize("what", sorted(NEAR_MISSES))
def test_the_battery_tells_the_rule_from_a_near_miss(what):
    variant, name = NEAR_MISSES[what]
    assert name in displace_cases.BY_NAME, name
    want = displace_cases.expected(name)
    got = displace_cases.expected(name, **variant)
    differ = int(np.count_nonzero((want != got) & ~(_is_nan(want) & _is_nan(got))))
    print("%s: %d of %d values differ on %s" % (what, differ, want.size, name))
    assert differ > 0, (what, name)


def test_the_battery_covers_what_it_claims():
    cases = displace_cases.CASES
    assert len(cases) > 250
    big = [c for c in cases if c["name"].startswith("big")]
    assert all(max(c["src_size"] + c["dst_size"]) <= 64 and min(c["src_size"][1], c["dst_size"][1]) <= 48 for c in cases if c not in big)
    assert len(big) == 1 and (big[0]["filter"], big[0]["dst_size"], big[0]["src_size"]) == (NEAREST, warp_cases.BIG[0], warp_cases.BIG[1])
    bw, bh = big[0]["dst_size"]
    assert ((bw + 30) // 16) * ((bh + 15) // 16) > 8 * 256  # more tiles than the launcher's grid has workgroups
    insts = {c["inst"] for c in cases}
    assert insts == {"%s/%s/%s" % (f, e, o) for f in warp_ref.FILTER_NAMES.values() for e in warp_ref.EDGE_NAMES.values() for o in ("premul", "straight")}
    for filt in FILTERS:  # every filter x every edge x both operand modes on a random map
        for edge in EDGES:
            for flags in (0, STRAIGHT):
                assert any((c["filter"], c["edge"], c["flags"], c["map_kind"]) == (filt, edge, flags, "random") for c in cases)
    for w in warp_cases.ITEM_WIDTHS:
        assert any(c["dst_size"][0] == w for c in cases), w
    for h in (3, 4, 5, 15, 16, 17):
        assert any(c["dst_size"][1] == h for c in cases), h
    for size in ((1, 1), (1, 5), (5, 1)):
        assert any(c["dst_size"] == size for c in cases), size
    assert any(c["dst_rect"] is not None and c["dst_rect"][0] % 2 and c["dst_rect"][1] % 2 and c["src_rect"] is not None and c["src_rect"][0] % 2 for c in cases)
    assert {(cx, cy) for c in cases for cx, cy in [c["channels"]]} == {(cx, cy) for cx in range(4) for cy in range(4)}
    for kind in warp_cases.KINDS:
        assert any(c["kind"] == kind for c in cases), kind
    assert {"own", "dst", "src", "never"} == {c["map_is"] for c in cases} and any(c["prior"] == "never" for c in cases)
    for n in (1, 2, 3):
        for edge in (REPEAT, MIRROR):
            assert any(c["src_size"][0] == n and c["edge"] == edge and max(abs(s) for s in c["scale"]) >= 1e4 for c in cases)
    scales = {s for c in cases for s in c["scale"]}
    assert {0.0, 1e30, -1e30, 2.0 ** 23, 2.0 ** -22, 3 * 2.0 ** -22} <= scales and any(math.copysign(1.0, s) < 0 and s == 0 for c in cases for s in c["scale"])
    assert any(c["scale"][0] != c["scale"][1] for c in cases) and any(s < 0 for s in scales)
    special = set(displace_cases.SPECIAL_VALUES)
    assert {0x0000, 0x8000, 0x3800, 0x7C00, 0xFC00, 0x7E00} <= special and any(0 < v < 0x400 for v in special) and any(0x3C00 < v < 0x7C00 for v in special)
    # positions of texel (0, 0) at, just below and just above a multiple of 2^32 (NEAREST); fractions 0x0000 and 0xffff (the others)
    low, fracs = set(), set()
    for c in cases:
        if c["map_kind"] != "edges":
            continue
        w, h = c["dst_size"]
        U, _ = displace_ref.positions(displace_cases.the_map(c), warp_ref.plan(c["matrix"]), (0, 0, w, h), c["scale"], *c["channels"])
        if c["filter"] == NEAREST:
            low |= set(int(v) for v in np.unique(U & 0xFFFFFFFF))
        else:
            fracs |= set(int(v) for v in np.unique(((U - 2 ** 31) >> 16) & 0xFFFF))
    assert {0, 1 << 8, 0xFFFFFFFF - 0xFF, 0xFFFFFFFE} <= low, sorted(low)[:8]
    assert {0, 0xFFFF} <= fracs
    # the matrices
    for m in (IDENTITY, warp_cases.translate(3, -2), warp_cases.translate(0.5, -0.5), warp_cases.scale(2)):
        assert any(c["matrix"] == tuple(float(v) for v in m) for c in cases)
    assert any(c["matrix"][1] != 0.0 for c in cases)
