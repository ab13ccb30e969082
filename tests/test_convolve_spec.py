"""The convolve rule on the CPU: the weights of the library (jh_convolve_weights) and of the host twin
(jl_convolve_weights) against the reference's bit for bit, the ctypes mirror's layout, the consequences the header states, the
reference (tests/convolve_ref.py) against the binary64 definition within a derived bound, texels worked by hand, the stand-alone check
(tools/convolve_check.cpp), and the sensitivity of the battery (tests/convolve_cases.py) to every near miss of the rule."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import ConvolveEdge, ConvolveMode, _lib, convolution

import convolve_cases
import convolve_ref
from abi_text import INCLUDE, ROOT, c_values
from convolve_ref import CLAMP, EDGES, MIRROR, PREMULTIPLIED, PRESERVE_ALPHA, REPEAT, STRAIGHT, ZERO


def f16(values):
    return np.asarray(values, np.float32).astype(np.float16).view(np.uint16)


def as_f32(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def half_ulp16(magnitude):
    """Half an f16 ULP of any value whose magnitude is at most `magnitude` (subnormal spacing 2^-24 at the least)."""
    e = np.floor(np.log2(np.maximum(np.asarray(magnitude, np.float64), 2.0 ** -14)))
    return 2.0 ** (e - 10.0) / 2.0


# ---- jh_convolve_weights ----

def _matrices():
    rng = np.random.default_rng(11)
    out = [((3, 3), [1, 2, 3, 4, 5, 6, 7, 8, 9], 0.0), ((3, 3), [-1, 0, 1, -2, 0, 2, -1, 0, 1], 0.0), ((3, 2), [1, 2, 3, 4, 5, 6], 7.0),
           ((1, 1), [3.0], 0.0), ((2, 2), [0.1, 0.2, 0.3, -0.6], 0.0), ((3, 1), [1e17, 1.0, -1e17], 0.0), ((15, 15), list(range(225)), 0.0),
           ((2, 1), [1e-30, 3e-42], 1.0), ((1, 2), [1.0, 1.0], -0.0), ((2, 2), [1, 1, 1, 1], 3.0)]
    for order in convolve_cases.ORDERS:
        out.append((order, list(rng.normal(size=order[0] * order[1])), float(rng.normal()) if order[0] % 2 else 0.0))
    return out


@pytest.mark.parametrize("twin", [False, True], ids=["library", "host twin"])
def test_weights_equal_the_reference_bit_for_bit(built, twin):
    for order, km, divisor in _matrices():
        got = jello_amd.convolve_weights(order, km, divisor, twin=twin)
        want = convolve_ref.weights(order, km, divisor)
        assert got.shape == want.shape == (order[1], order[0])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (order, km, divisor)


@pytest.mark.parametrize("twin", [False, True], ids=["library", "host twin"])
def test_weights_refusals(built, twin):
    for order, km, divisor in (((0, 1), [], 0.0), ((16, 1), [1.0] * 16, 0.0), ((1, 1), [float("nan")], 0.0), ((1, 1), [float("inf")], 1.0),
                               ((1, 1), [1.0], float("nan")), ((1, 1), [1.0], float("inf")), ((1, 1), [1e300], 1.0), ((1, 1), [1.0], 1e-300),
                               ((2, 1), [1e308, 1e308], 0.0), ((2, 2), [1.0, 2.0, 3.0], 0.0)):
        with pytest.raises(ValueError):
            jello_amd.convolve_weights(order, km, divisor, twin=twin)
        if len(km) == order[0] * order[1]:
            with pytest.raises(ValueError):
                convolve_ref.weights(order, km, divisor)
    L = _lib.load_host()
    f = L.jl_convolve_weights if twin else L.hip.jh_convolve_weights
    assert f(1, 1, None, 0.0, (ctypes.c_float * 1)()) != 0 and f(1, 1, (ctypes.c_double * 1)(1.0), 0.0, None) != 0


def test_the_flip_is_a_rotation_by_180_degrees():
    km = np.arange(1.0, 16.0).reshape(3, 5)  # order_x 5, order_y 3
    w = convolve_ref.weights((5, 3), km.ravel(), 1.0)
    assert np.array_equal(w, km[::-1, ::-1].astype(np.float32))
    assert np.array_equal(convolve_ref.weights((5, 3), km.ravel())[0, 0], np.float32(15.0 / 120.0))


# ---- the C ABI ----

def test_ctypes_mirror_has_the_headers_layout():
    mirror = _lib.CConvolveDesc
    fields = [name for name, _ in mirror._fields_]
    want = c_values(["sizeof(jh_convolve_desc)"] + ["offsetof(jh_convolve_desc, %s)" % f for f in fields])
    assert [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want
    assert fields == ["order_x", "order_y", "target_x", "target_y", "edge", "mode", "bias", "x", "y", "width", "height", "weights"]


def test_enums_and_limits_match_the_header():
    names = ["JH_CONVOLVE_EDGE_" + e.name for e in ConvolveEdge] + ["JH_CONVOLVE_" + m.name for m in ConvolveMode]
    assert c_values(names) == [int(e) for e in ConvolveEdge] + [int(m) for m in ConvolveMode] == [0, 1, 2, 3, 0, 1, 2]
    assert c_values(["JH_WARP_EDGE_" + e.name for e in ConvolveEdge]) == [int(e) for e in ConvolveEdge]
    assert c_values(["JH_CONVOLVE_MAX_ORDER", "JH_CONVOLVE_MAX_TAPS", "sizeof(((jh_convolve_desc*)0)->weights) / 4"]) == [15, 225, 225]
    from jello_amd import engine
    assert (engine.CONVOLVE_MAX_ORDER, engine.CONVOLVE_MAX_TAPS) == (15, 225)
    assert (convolve_ref.MAX_ORDER, convolve_ref.MAX_TAPS) == (15, 225)


def test_the_python_constructors():
    k = convolution.from_svg(3, [1, 2, 3, 4, 5, 6, 7, 8, 9], edge_mode="wrap", preserve_alpha=True, bias=0.25)
    assert np.array_equal(k["weights"], convolve_ref.weights(3, [1, 2, 3, 4, 5, 6, 7, 8, 9]))
    assert (k["edge"], k["mode"], k["bias"], k["order"], k["target"]) == (ConvolveEdge.REPEAT, ConvolveMode.PRESERVE_ALPHA, 0.25, (3, 3), None)
    assert convolution.from_svg((3, 1), [1, 0, -1], edge_mode="none")["edge"] == ConvolveEdge.ZERO
    with pytest.raises(ValueError):
        convolution.from_svg(3, [1] * 9, edge_mode="reflect")
    with pytest.raises(ValueError):
        convolution.box(16)
    for k in (convolution.sharpen(0.5), convolution.box(3), convolution.box(1)):
        assert abs(float(k["weights"].astype(np.float64).sum()) - 1.0) < 1e-6 and k["mode"] == ConvolveMode.PREMULTIPLIED
    for k in (convolution.sobel_x(), convolution.sobel_y(), convolution.laplacian(), convolution.laplacian(True)):
        assert float(k["weights"].sum()) == 0.0 and k["order"] == (3, 3) and k["mode"] == ConvolveMode.PRESERVE_ALPHA
    assert np.array_equal(convolution.sobel_x()["weights"], convolution.sobel_y()["weights"].T)
    assert convolution.emboss()["bias"] == 0.5
    # a descriptor as Engine.convolve builds it
    d = jello_amd.engine._convolve_desc(**{**convolution.sobel_x(), "rect": (1, 2, 3, 4)})
    assert (d.order_x, d.order_y, d.target_x, d.target_y, d.edge, d.mode, d.x, d.y, d.width, d.height) == (3, 3, 1, 1, 1, 2, 1, 2, 3, 4)
    assert list(d.weights[:9]) == [-1.0, 0.0, 1.0, -2.0, 0.0, 2.0, -1.0, 0.0, 1.0] and not any(d.weights[9:])
    d = jello_amd.engine._convolve_desc(np.ones((2, 5), np.float32), None, None, 0, 0, 0.0, None)
    assert (d.order_x, d.order_y, d.target_x, d.target_y) == (5, 2, 2, 1)
    for bad in (dict(weights=np.ones(9), order=None), dict(weights=np.ones(8), order=3), dict(weights=np.ones(16), order=(16, 1))):
        with pytest.raises(ValueError, match="jh_convolve: "):
            jello_amd.engine._convolve_desc(bad["weights"], bad["order"], None, 0, 0, 0.0, None)


# ---- the consequences the header states ----

@pytest.mark.parametrize("edge", EDGES)
def test_straight_identity_copies_every_non_nan_value(edge):
    bits = np.concatenate([convolve_cases.content(k, 16, 6, 5) for k in ("finite", "subnormal", "zeros", "nonfinite")])
    got = convolve_ref.convolve(bits, np.ones((1, 1), np.float32), None, edge, STRAIGHT)
    nan = (bits & 0x7FFF) > 0x7C00
    want = np.where(bits == 0x8000, 0, bits)  # (-0 comes out as +0)
    assert np.array_equal(got[~nan], want[~nan]) and np.all((got[nan] & 0x7FFF) > 0x7C00)
    assert (bits == 0x8000).any() and (bits == 0x7C00).any() and nan.any()


def test_a_single_one_is_an_integer_translation_under_zero():
    bits = convolve_cases.content("finite", 23, 11, 9)
    bits[bits == 0x8000] = 0
    for (ox, oy), (i, j), (tx, ty) in (((5, 3), (4, 0), (2, 1)), ((1, 15), (0, 14), (0, 0)), ((15, 15), (0, 7), (14, 14)), ((2, 2), (1, 1), (1, 1))):
        w = np.zeros((oy, ox), np.float32)
        w[j, i] = 1.0
        got = convolve_ref.convolve(bits, w, (tx, ty), ZERO, STRAIGHT)
        sx, sy = i - tx, j - ty  # out(X, Y) = src(X + sx, Y + sy)
        want = np.zeros_like(bits)
        H, W, _ = bits.shape
        ys, xs = np.arange(H) + sy, np.arange(W) + sx
        oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        want[np.ix_(oky, okx)] = bits[np.ix_(ys[oky], xs[okx])]
        assert np.array_equal(got, want), ((ox, oy), (i, j), (tx, ty))


@pytest.mark.parametrize("edge", [CLAMP, REPEAT, MIRROR])
def test_a_constant_image_stays_constant_up_to_the_chains_rounding(edge):
    """The weights sum to 1 exactly (multiples of 2^-12, the last one the remainder): |V - c| <= gamma_n |c| sum |w|, and the store adds
    half an f16 ULP.  Equality does not hold: with weights near +-1000 that cancel, the bound is above an f16 ULP and some kernel
    does move the constant."""
    u, moved = 2.0 ** -24, {512.0: False, 2.0 ** 22: False}
    rng = np.random.default_rng(3)
    for scale in moved:
        for order in ((3, 3), (5, 5), (7, 3), (15, 15)) if scale == 512.0 else ((3, 3),) * 12:
            n = order[0] * order[1]
            w = np.round(rng.normal(size=n) * scale) / 4096.0
            w[-1] = 1.0 - w[:-1].sum()
            assert np.all(w.astype(np.float32) == w) and w.sum() == 1.0
            for c in (0.7001953125, 1.0, -3.140625, 60000.0, 6.103515625e-05):
                assert float(np.float16(c)) == c
                bits = np.tile(f16([c] * 4), (9, 11, 1))
                got = as_f32(convolve_ref.convolve(bits, w.reshape(order[1], order[0]), None, edge, STRAIGHT)).astype(np.float64)
                bound = n * u / (1.0 - n * u) * abs(c) * np.abs(w).sum()
                assert np.all(np.abs(got - c) <= bound + half_ulp16(abs(c) + bound)), (order, c)
                moved[scale] = moved[scale] or bool(np.any(got != c))
    assert moved == {512.0: False, 2.0 ** 22: True}
    box = np.full((2, 2), 0.25, np.float32)  # every partial sum exact: equality
    bits = np.tile(f16([0.3, 0.3, 0.3, 0.3]), (5, 5, 1))
    assert np.array_equal(convolve_ref.convolve(bits, box, None, edge, STRAIGHT), bits)


# ---- the reference against the definition ----

@pytest.mark.parametrize("mode", [PREMULTIPLIED, STRAIGHT, PRESERVE_ALPHA])
def test_reference_against_the_binary64_definition(mode):
    """Before the store the chain of n = ox oy fmaf's differs from the exact sum S by at most gamma_n sum |w p| (one rounding per
    step: the standard bound of a recursive sum whose products are exact); the bias adds at most two roundings more, hence gamma_(n +
    2) over sum |w p| + |bias| (+ |bias V.a| under PREMULTIPLIED), and the f16 store half an ULP of the result (subnormal spacing
    2^-24 at the least).  STRAIGHT and PRESERVE_ALPHA store V itself, so the bound is checked on them; PREMULTIPLIED is checked on
    alpha, whose store is f16(V.a + 0)."""
    u = 2.0 ** -24
    for case in [c for c in convolve_cases.CASES if c["mode"] == mode and c["kind"] in ("unit", "finite") and c["rect"] is None][:40]:
        w, bias = convolve_cases.weights(case), float(np.float32(case["bias"]))
        src = convolve_cases.source(case)
        x, y, rw, rh = convolve_cases.rect_of(case)
        got = as_f32(convolve_cases.expected(case["name"])[y:y + rh, x:x + rw]).astype(np.float64)
        total, mag = convolve_ref.direct(src, w, case["target"], case["edge"], mode, case["rect"])
        n = w.size + 2
        gamma = n * u / (1.0 - n * u)
        channels = [3] if mode == PREMULTIPLIED else ([0, 1, 2] if mode == PRESERVE_ALPHA else [0, 1, 2, 3])
        for ch in channels:
            want = total[..., ch] + bias
            bound = gamma * (mag[..., ch] + abs(bias))
            ok = np.isfinite(want) & (np.abs(want) + bound < 65504.0)
            assert ok.any()
            assert np.all(np.abs(got[..., ch] - want)[ok] <= (bound + half_ulp16(np.abs(want) + bound))[ok]), case["name"]


# ---- texels worked by hand ----

def test_texels_by_hand():
    # a 3 x 1 image, alpha 1: (1, 2, 4); kernel (1, 2, 3) at target 1: out(X) = 1 src(X - 1) + 2 src(X) + 3 src(X + 1)
    row = np.array([[[1, 1, 1, 1], [2, 2, 2, 1], [4, 4, 4, 1]]], np.float32)
    bits = f16(row)
    w = np.array([[1, 2, 3]], np.float32)
    by_edge = {ZERO: (0 + 2 + 6, 1 + 4 + 12, 2 + 8 + 0), CLAMP: (1 + 2 + 6, 17, 2 + 8 + 12), REPEAT: (4 + 2 + 6, 17, 2 + 8 + 3), MIRROR: (1 + 2 + 6, 17, 2 + 8 + 12)}
    for edge, want in by_edge.items():
        got = as_f32(convolve_ref.convolve(bits, w, (1, 0), edge, STRAIGHT))
        assert tuple(got[0, :, 0]) == want, edge
    # alpha under STRAIGHT is convolved like colour: ZERO gives (2 + 3, 6, 1 + 2), the others 6
    assert tuple(as_f32(convolve_ref.convolve(bits, w, (1, 0), ZERO, STRAIGHT))[0, :, 3]) == (5.0, 6.0, 3.0)
    assert tuple(as_f32(convolve_ref.convolve(bits, w, (1, 0), CLAMP, STRAIGHT))[0, :, 3]) == (6.0, 6.0, 6.0)
    # target 0: out(X) = 1 src(X) + 2 src(X + 1) + 3 src(X + 2); MIRROR at X = 2 reads indices 2, 2, 1
    assert tuple(as_f32(convolve_ref.convolve(bits, w, (0, 0), MIRROR, STRAIGHT))[0, :, 0]) == (1 + 4 + 12, 2 + 8 + 12, 4 + 8 + 6)
    # PRESERVE_ALPHA: colour as stored, alpha copied; bias on colour only
    half = f16(np.array([[[1, 1, 1, 0.5], [2, 2, 2, 0.25], [4, 4, 4, 0.0]]], np.float32))
    got = convolve_ref.convolve(half, w, (1, 0), ZERO, PRESERVE_ALPHA, bias=0.5)
    assert tuple(as_f32(got)[0, :, 1]) == (8.5, 17.5, 10.5) and np.array_equal(got[..., 3], half[..., 3])
    # PREMULTIPLIED: operands (0.5, 0.5), (0.5, 0.25), (0, 0); the box (1, 1, 1) under ZERO: premultiplied colour (1, 1, 0.5) over
    # alpha (0.75, 0.75, 0.25), stored un-premultiplied
    got = as_f32(convolve_ref.convolve(half, np.ones((1, 3), np.float32), (1, 0), ZERO, PREMULTIPLIED))
    assert tuple(got[0, :, 3]) == (0.75, 0.75, 0.25)
    third = np.float32(1.0) / np.float32(0.75)
    assert tuple(got[0, :, 0]) == tuple(float(np.float16(np.float32(v) * np.float32(inv))) for v, inv in ((1.0, third), (1.0, third), (0.5, 4.0)))
    # PREMULTIPLIED with a bias of 0.25: alpha 0.75 + 0.25 = 1, colour fmaf(0.25, 1, 1) = 1.25 over alpha 1
    got = as_f32(convolve_ref.convolve(half, np.ones((1, 3), np.float32), (1, 0), ZERO, PREMULTIPLIED, bias=0.25))
    assert tuple(got[0, :2, 3]) == (1.0, 1.0) and tuple(got[0, :2, 2]) == (1.25, 1.25)
    assert (got[0, 2, 3], got[0, 2, 0]) == (0.5, float(np.float16(np.float32(0.5 + 0.25 * 0.5) * np.float32(2.0))))
    # a zero weight still multiplies: 0 x Inf is a NaN; and a bias of -0 is no bias: acc = -0 stays -0 under STRAIGHT
    inf = f16(np.array([[[np.inf, 1, 1, 1], [1, 1, 1, 1]]], np.float32))
    got = convolve_ref.convolve(inf, np.array([[0.0, 1.0]], np.float32), (1, 0), CLAMP, STRAIGHT)
    assert (got[0, 1, 0] & 0x7FFF) > 0x7C00 and got[0, 1, 1] == 0x3C00
    neg = f16(np.array([[[-1, -1, -1, -1]]], np.float32))
    assert tuple(convolve_ref.convolve(neg, np.array([[1e-41]], np.float32), None, CLAMP, STRAIGHT, bias=-0.0)[0, 0]) == (0x8000,) * 4
    assert tuple(convolve_ref.convolve(neg, np.array([[1e-41]], np.float32), None, CLAMP, STRAIGHT, bias=0.5)[0, 0]) == (0x3800,) * 4


# ---- the stand-alone check ----

def test_the_stand_alone_check_builds_and_passes(tmp_path):
    """tools/convolve_check.cpp is include/jello_convolve.h with a main of its own: every legal and a set of illegal descriptors,
    jconv_weights against long double, the default divisor, and the index rules on n = 1..5 against a walk.  Its header has the
    command with the sanitizers; here it is built without them and run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "convolve_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", INCLUDE, os.path.join(ROOT, "tools", "convolve_check.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode() == "ok\n"


# ---- the battery ----

def test_battery_covers_what_it_names():
    cases = convolve_cases.CASES
    assert len({c["name"] for c in cases}) == len(cases) >= 250
    assert {c["inst"] for c in cases} == {"3x3", "5x5", "general"}
    for inst in ("3x3", "5x5", "general"):  # every instantiation: every edge with every mode, a rectangle, a bias
        mine = [c for c in cases if c["inst"] == inst]
        assert {(c["edge"], c["mode"]) for c in mine} == {(e, m) for e in EDGES for m in convolve_ref.MODES}
        assert any(c["rect"] for c in mine) and any(c["bias"] != 0.0 for c in mine)
    assert {c["order"] for c in cases} >= set(convolve_cases.ORDERS)
    assert {c["size"] for c in cases} >= set(convolve_cases.TILE_SIZES)
    for order in convolve_cases.ORDERS:
        assert {c["target"] for c in cases if c["order"] == order} >= {(0, 0), (order[0] // 2, order[1] // 2), (order[0] - 1, order[1] - 1)}
    assert {c["kind"] for c in cases} == set(convolve_cases.KINDS)
    assert {repr(c["bias"]) for c in cases} == {"0.0", "-0.0", "0.5", "-0.25"}
    w, h = convolve_cases.BIG
    assert ((w + 15 + 63) // 64) * ((h + 15) // 16) > 8 * 256  # more tiles than the launcher's cap
    some = np.concatenate([convolve_cases.weights(c).ravel() for c in cases])
    assert (some < 0).any() and (some == 0).any() and ((some != 0) & (np.abs(some) < 1.1754944e-38)).any()


def test_nan_around_a_rectangle_shows_exactly_where_the_window_reaches():
    for c in [c for c in convolve_cases.CASES if c["rect"] and c["kind"] == "unit" and c["prior"] == "poison" and c["rect"][2] > 1]:
        x, y, rw, rh = c["rect"]
        (ox, oy), (tx, ty) = c["order"], c["target"]
        got = convolve_cases.expected(c["name"])
        nan = (got & 0x7FFF) > 0x7C00
        channels = [0, 1, 2] if c["mode"] == PRESERVE_ALPHA else [0, 1, 2, 3]
        want = np.zeros((rh, rw), bool)  # the window [X - tx, X - tx + ox) x [Y - ty, Y - ty + oy) leaves the rectangle (all images are larger)
        want[:ty] = want[rh - (oy - 1 - ty):] = True
        want[:, :tx] = want[:, rw - (ox - 1 - tx):] = True
        for ch in channels:
            assert np.array_equal(nan[y:y + rh, x:x + rw, ch], want), c["name"]
        outside = np.ones(got.shape[:2], bool)
        outside[y:y + rh, x:x + rw] = False
        assert np.all(got[outside] == convolve_cases.POISON)


NEAR_MISSES = [dict(flipped=True), dict(fused=False), dict(descending=True), dict(row_sums=True), dict(target_shift=1), dict(edge_rect=True),
               dict(skip_zero=True), dict(bias_source_alpha=True), dict(mirror_2n=False)]


@pytest.mark.parametrize("variant", NEAR_MISSES, ids=[next(iter(v)) for v in NEAR_MISSES])
def test_battery_tells_every_near_miss_from_the_rule(variant):
    for c in convolve_cases.CASES:
        miss = convolve_ref.convolve(convolve_cases.source(c), convolve_cases.weights(c), c["target"], c["edge"], c["mode"], c["bias"], c["rect"],
                                     convolve_cases.before(c), **variant)
        if not convolve_ref.same_bits(miss, convolve_cases.expected(c["name"])):
            return
    pytest.fail("no case of the battery tells %r from the rule" % (variant,))
