"""The blur rule on the CPU: the library's taps against the reference's bit for bit, what the taps have to satisfy,
the reference (tests/blur_ref.py) against the definition it rounds, and that the battery (tests/blur_cases.py) tells the rule from
four near misses."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd

import blur_cases
import blur_ref


def _sigma_sweep():
    """0, the smallest sigma with R = 1, 64, values just either side of every R step up to 8 and of some beyond, and a spread."""
    f32 = np.float32
    out = [f32(0.0), np.nextafter(f32(0.0), f32(1.0)), f32(1e-3), f32(0.05), f32(0.07), f32(0.3), f32(64.0), np.nextafter(f32(64.0), f32(0.0))]
    for r in list(range(1, 9)) + [21, 64, 100, 191]:
        step = f32(r / 3.0)
        out += [step, np.nextafter(step, f32(0.0)), np.nextafter(step, f32(100.0))]
    out += [f32(v) for v in np.linspace(0.01, 64.0, 97)]
    return out


def test_taps_equal_the_references_bit_for_bit(built):
    for s in _sigma_sweep():
        w, r = jello_amd.blur_taps(s)
        want, r_want = blur_ref.taps(s)
        assert r == r_want == math.ceil(3.0 * float(s)), s
        assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), want.view(np.uint32)), s


def test_the_host_twin_compiles_the_same_rule(built):
    L = jello_amd.load_host()
    for s in _sigma_sweep():
        r = ctypes.c_uint32(0)
        assert L.jl_blur_taps(float(s), None, ctypes.byref(r)) == 0
        w = np.empty(2 * r.value + 1, np.float32)
        assert L.jl_blur_taps(float(s), w.ctypes.data, None) == 0
        assert np.array_equal(w.view(np.uint32), jello_amd.blur_taps(s)[0].view(np.uint32)), s
    assert L.jl_blur_taps(-1.0, None, None) == -1


def test_taps_are_symmetric_monotone_and_sum_to_one(built):
    for s in _sigma_sweep():
        w, r = jello_amd.blur_taps(s)
        assert len(w) == 2 * r + 1 and r <= 192
        assert np.array_equal(w, w[::-1])
        assert np.all(np.diff(w[r:]) <= 0.0) and np.all(w >= 0.0)
        # every tap is within 2^-24 relative of g_k / S (which sum to 1 within a few binary64 ulps), so |sum - 1| <= 2^-24 + slack
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= (2 * r + 2) * 2.0 ** -24, s
    assert list(jello_amd.blur_taps(0.0)[0]) == [1.0] and jello_amd.blur_taps(0.0)[1] == 0
    assert jello_amd.blur_taps(np.nextafter(np.float32(0.0), np.float32(1.0)))[1] == 1
    assert jello_amd.blur_taps(64.0)[1] == 192


def test_bad_sigmas_are_refused(built):
    hip = jello_amd.load_host().hip
    for s in (-1.0, -1e-30, float(np.nextafter(np.float32(64.0), np.float32(100.0))), 1e9, float("inf"), float("-inf"), float("nan")):
        assert hip.jh_blur_taps(s, None, None) == -1, s  # JH_ERR_INVALID
        with pytest.raises(ValueError):
            jello_amd.blur_taps(s)
        with pytest.raises(ValueError):
            blur_ref.taps(s)
    r = ctypes.c_uint32(7)
    assert hip.jh_blur_taps(-0.0, None, ctypes.byref(r)) == 0 and r.value == 0  # (-0 is 0)


def _f16_ulp(v):
    a = np.maximum(np.abs(v), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


@pytest.mark.parametrize("edge", blur_cases.EDGES)
@pytest.mark.parametrize("sigma", [(1.0, 1.0), (2.5, 7.0), (0.0, 2.5), (7.0, 0.3)])
def test_reference_against_the_definition(sigma, edge):
    """The reference rounds the direct 2-D Gaussian sum D (binary64, unrounded taps).  With M = max |src|: a tap is within 2^-24
    relative of its exact value, so a pass's exact sum over the rounded taps is within 2^-24 M' of the one over the exact taps (the
    taps are positive and sum to 1; M' = the largest input of the pass, <= M (1 + small)); each of the pass's n = 2R + 1 fmaf rounds
    a partial sum of magnitude <= M' once, <= 2^-24 M' each (2^-25 relative, and room for the second-order terms).  That is
    (2R + 2) 2^-24 M per pass and (2Rx + 2Ry + 4) 2^-24 M for both -- the vertical pass averages the horizontal one's errors, it does
    not amplify them -- and 2 more for M' against M.  The final rounding to f16 moves the value by at most half an f16 ulp of the
    computed value, which is at most one f16 ulp of the exact one.  So
        |f16(V) - D| <= ulp_f16(D) + (2Rx + 2Ry + 6) 2^-24 M."""
    src = blur_cases.content("unit", 23, 17, seed=5)
    got = blur_ref.blur(src, sigma, edge).view(np.float16).astype(np.float64)
    want = blur_ref.direct(src, sigma, edge)
    m = float(np.abs(src.view(np.float16).astype(np.float64)).max())
    bound = _f16_ulp(want) + (2 * blur_ref.radius(sigma[0]) + 2 * blur_ref.radius(sigma[1]) + 6) * 2.0 ** -24 * m
    err = np.abs(got - want)
    print("max err / bound:", float((err / bound).max()))
    assert np.all(err <= bound)


def test_sigma_zero_is_the_identity():
    """(0, 0): every value is copied; by the rule fmaf(1, -0, +0) = +0, so a -0 comes out as +0 (and a NaN as a NaN)."""
    for kind in ("finite", "nonfinite"):
        src = blur_cases.content(kind, 19, 11, seed=9)
        want = np.where(src == 0x8000, np.uint16(0), src)
        for edge in blur_cases.EDGES:
            assert blur_ref.same_bits(blur_ref.blur(src, (0.0, 0.0), edge), want)


def test_an_impulse_gives_the_outer_product_of_the_taps():
    """One texel of 1.0 in a black image that holds the whole kernel: H is the horizontal taps exactly (1.0 w + 0), V multiplies
    each by one vertical tap and adds zeros -- one rounding to binary32, then the one to f16."""
    sigma = (1.5, 2.0)
    (wx, rx), (wy, ry) = blur_ref.taps(sigma[0]), blur_ref.taps(sigma[1])
    h, w = 2 * ry + 3, 2 * rx + 3
    src = np.zeros((h, w, 4), np.uint16)
    src[ry + 1, rx + 1] = 0x3C00
    want = np.zeros((h, w), np.float16)
    want[1:-1, 1:-1] = (wy.astype(np.float64)[:, None] * wx.astype(np.float64)[None, :]).astype(np.float32).astype(np.float16)
    for edge in blur_cases.EDGES:
        got = blur_ref.blur(src, sigma, edge)
        for ch in range(4):
            assert np.array_equal(got[:, :, ch], want.view(np.uint16))


VARIANTS = {"unfused": {"fused": False}, "descending": {"descending": True}, "f16_intermediate": {"f16_intermediate": True},
            "binary32_taps": {"binary32_taps": True}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_battery_tells_the_rule_from_a_near_miss(variant):
    """Each wrong variant differs from the reference in at least one texel of at least one case of the battery (the search stops at
    the first such case; the count of cases tried is printed)."""
    tried = 0
    for c in blur_cases.CASES:
        if c["sigma"] == (0.0, 0.0) or c["w"] * c["h"] > 2500:
            continue  # (the small cases are enough to tell, and quick)
        tried += 1
        src = blur_cases.source(c)
        before = src if c["in_place"] else np.full_like(src, blur_cases.POISON)
        wrong = blur_ref.blur(src, c["sigma"], c["edge"], c["rect"], before, **VARIANTS[variant])
        if not blur_ref.same_bits(wrong, blur_cases.expected(c["name"])):
            print(variant, "differs on", c["name"], "after", tried, "cases")
            return
    pytest.fail("no case of the battery tells the variant '%s' from the rule: add a case" % variant)


def test_the_battery_covers_what_it_claims():
    names = set(blur_cases.BY_NAME)
    assert len(names) > 200
    for (w, h) in blur_cases.SIZES:
        for sigma in blur_cases.SIGMAS:
            for edge in blur_cases.EDGES:
                assert any(c["w"] == w and c["h"] == h and c["sigma"] == sigma and c["edge"] == edge for c in blur_cases.CASES)
    assert {c["kind"] for c in blur_cases.CASES} == {"finite", "unit", "nonfinite", "never"}
    assert any(c["in_place"] and c["rect"] for c in blur_cases.CASES) and any(not c["in_place"] and c["rect"] for c in blur_cases.CASES)
    assert any(c["sigma"] == (64.0, 64.0) and c["w"] == 40 and c["h"] == 24 for c in blur_cases.CASES)
