"""The resample rule on the CPU: the library's windows and taps against the reference's bit for bit, what they have
to satisfy (the tap bound, no empty window, S > 0), the consequences the rule states, the ctypes mirror of the descriptor, the
reference (tests/resample_ref.py) against the definition it rounds, and that the battery (tests/resample_cases.py) tells the rule
from six near misses."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import _lib

import resample_cases
import resample_ref
from abi_text import c_values
from resample_ref import BOX, CATMULL_ROM, FILTERS, LANCZOS3, STRAIGHT, TRIANGLE


def _size_pairs():
    """(n_in, n_out): every n_out of a spread, against the n_in at and next to every ratio the rule singles out."""
    pairs = set()
    for n_out in list(range(1, 13)) + [31, 32, 33, 63, 64, 65, 129]:
        for n_in in (1, 2, 3, 5, 17, 100, n_out - 1, n_out, n_out + 1, 2 * n_out, 2 * n_out + 1, 3 * n_out // 2, 7 * n_out // 5, 3 * n_out,
                     n_out // 3, 16 * n_out - 1, 16 * n_out, 15 * n_out + 1):
            if resample_ref.sizes_ok(n_in, n_out):
                pairs.add((n_in, n_out))
    return sorted(pairs)


PAIRS = _size_pairs()


def _c_taps(fn, filt, n_in, n_out, i):
    w = np.full(resample_ref.MAX_TAPS + 1, -7.0, np.float32)  # (one more than the bound: the call must not write it)
    first, count = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert fn(filt, n_in, n_out, i, w.ctypes.data, ctypes.byref(first), ctypes.byref(count)) == 0
    assert w[resample_ref.MAX_TAPS] == -7.0
    return first.value, w[:count.value]


@pytest.mark.parametrize("filt", FILTERS)
def test_taps_equal_the_references_bit_for_bit(built, filt):
    """jh_resample_taps and its host twin jl_resample_taps against resample_ref.window, over the sweep; and what the rule promises of
    every window: at least one tap, at most 96, inside the axis, S > 0."""
    L = jello_amd.load_host()
    most, least_s = 0, np.inf
    for n_in, n_out in PAIRS:
        by_engine = jello_amd.resample_taps(filt, n_in, n_out)
        assert len(by_engine) == n_out
        for i in range(n_out):
            first, w, s = resample_ref.window(filt, n_in, n_out, i)
            assert 1 <= len(w) <= resample_ref.MAX_TAPS and first + len(w) <= n_in and s > 0.0, (n_in, n_out, i)
            most, least_s = max(most, len(w)), min(least_s, s)
            for got_first, got_w in (by_engine[i], _c_taps(L.jl_resample_taps, filt, n_in, n_out, i)):
                assert got_first == first and got_w.dtype == np.float32, (n_in, n_out, i)
                assert np.array_equal(got_w.view(np.uint32), w.view(np.uint32)), (n_in, n_out, i)
    print("filter", filt, "most taps", most, "least S", least_s)
    assert least_s >= 0.48
    if filt == LANCZOS3:
        assert most == 96  # (the bound is reached: 16:1)


def test_the_tap_bound_is_the_headers_constant():
    assert c_values(["JH_RESAMPLE_MAX_TAPS", "JH_RESAMPLE_STRAIGHT", "JH_RESAMPLE_BOX", "JH_RESAMPLE_TRIANGLE", "JH_RESAMPLE_CATMULL_ROM",
                     "JH_RESAMPLE_LANCZOS3"]) == [resample_ref.MAX_TAPS, STRAIGHT, BOX, TRIANGLE, CATMULL_ROM, LANCZOS3]
    assert [int(f) for f in jello_amd.ResampleFilter] == list(FILTERS)


def test_bad_axes_are_refused(built):
    L = jello_amd.load_host()
    for fn in (L.hip.jh_resample_taps, L.jl_resample_taps):
        for filt, n_in, n_out, i in ((-1, 4, 4, 0), (4, 4, 4, 0), (0, 0, 4, 0), (0, 4, 0, 0), (0, 65, 4, 0), (2, 4, 4, 4), (3, 0xFFFFFFFF, 0x0FFFFFFF, 0)):
            assert fn(filt, n_in, n_out, i, None, None, None) == -1, (filt, n_in, n_out, i)
        count = ctypes.c_uint32(0)
        assert fn(3, 64, 4, 3, None, None, ctypes.byref(count)) == 0 and count.value > 0  # (weights may be NULL)
    for bad in ((7, 4, 4), (0, 65, 4), (0, 0, 1)):
        with pytest.raises(ValueError):
            jello_amd.resample_taps(*bad)
        with pytest.raises(ValueError):
            resample_ref.window(bad[0], bad[1], bad[2], 0)


def test_equal_sizes_give_the_single_tap_one():
    for n in (1, 2, 7, 64, 129):
        for filt in (BOX, TRIANGLE, CATMULL_ROM):
            for i in range(n):
                first, w, _ = resample_ref.window(filt, n, n, i)
                assert first == i and list(w) == [1.0], (filt, n, i)
    # not LANCZOS3: sin(k pi) is not 0 in binary64, so the neighbours keep taps of about 1e-17
    assert any(len(resample_ref.window(LANCZOS3, 7, 7, i)[1]) > 1 for i in range(7))


def test_the_ctypes_mirror_has_the_headers_layout():
    mirror = _lib.CResampleDesc
    fields = [name for name, _ in mirror._fields_]
    assert fields == ["filter", "flags", "src_x", "src_y", "src_width", "src_height", "dst_x", "dst_y", "dst_width", "dst_height"]
    want = c_values(["sizeof(jh_resample_desc)"] + ["offsetof(jh_resample_desc, %s)" % f for f in fields])
    assert [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want


def test_straight_with_equal_sizes_is_a_copy():
    """The single tap 1.0f on both axes: every value is copied; fmaf(1, -0, +0) = +0, so a -0 comes out as +0 (and a NaN as a NaN)."""
    for kind in ("finite", "nonfinite", "subnormal", "zeros"):
        src = resample_cases.content(kind, 19, 11, seed=9)
        want = np.where(src == 0x8000, np.uint16(0), src)
        for filt in (BOX, TRIANGLE, CATMULL_ROM):
            assert resample_ref.same_bits(resample_ref.resample(src, (11, 19), filt, STRAIGHT), want)


def test_straight_box_at_two_to_one_is_the_mean_of_four():
    """Taps 0.5f, 0.5f on both axes: H = fl32(0.5 a + 0.5 b) (the first fmaf is exact), V likewise over two rows, then f16.  The sums
    of two halves are exact in binary64 (f16 inputs: 51 bits at most; H: multiples of 2^-26 below 2^17), so binary64 arithmetic
    followed by one rounding states each step."""
    src = resample_cases.content("unit", 26, 14, seed=4)
    f = src.view(np.float16).astype(np.float64)
    hor = (0.5 * f[:, 0::2] + 0.5 * f[:, 1::2]).astype(np.float32).astype(np.float64)
    want = (0.5 * hor[0::2] + 0.5 * hor[1::2]).astype(np.float32).astype(np.float16).view(np.uint16)
    for n in (13, 7):
        assert [list(w) for _, w in resample_ref.axis_taps(BOX, 2 * n, n)] == [[0.5, 0.5]] * n
    assert np.array_equal(resample_ref.resample(src, (7, 13), BOX, STRAIGHT), want)


def _f16_ulp(v):
    a = np.maximum(np.abs(v), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def _bound(filt, src_size, dst_size, m, d):
    """|f16(V) - D| for the STRAIGHT rule against the binary64 sum D with unrounded taps, M = max |src|, u = 2^-24.  Per axis let n
    be the most taps of a window and A the largest sum of |w_k| of one (1 for BOX and TRIANGLE, above 1 with negative lobes).
    Horizontal: a tap is within u relative of its exact value, so the exact sum over the rounded taps is within u A_x M of the one
    over the exact taps; each of the n_x fmaf rounds a partial sum of magnitude <= A_x M once, <= u A_x M each: |H - H*| <=
    (n_x + 1) u A_x M.  Vertical: the horizontal errors pass through sum |w_k| = A_y, the taps' rounding adds u A_y (A_x M) and the
    n_y fmaf u A_y A_x M each: |V - D| <= (n_x + n_y + 2) u A_x A_y M, and 2 more of the same for the second-order terms (M' of a
    pass against M, A over rounded against exact taps): E = (n_x + n_y + 4) u A_x A_y M.  The rounding to f16 moves V by at most
    half an f16 ulp of V, and |V| <= |D| + E.  So |f16(V) - D| <= ulp_f16(|D| + E) / 2 + E."""
    n, a = [], []
    for n_in, n_out in zip(src_size, dst_size):
        ws = [resample_ref.window(filt, n_in, n_out, i, exact=True)[1] for i in range(n_out)]
        n.append(max(len(w) for w in ws))
        a.append(max(float(np.abs(w).sum()) for w in ws))
    e = (n[0] + n[1] + 4) * 2.0 ** -24 * a[0] * a[1] * m
    return 0.5 * _f16_ulp(np.abs(d) + e) + e


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("sizes", [((23, 17), (23, 17)), ((46, 17), (23, 12)), ((35, 21), (25, 15)), ((160, 16), (10, 1)), ((7, 5), (21, 16))])
def test_reference_against_the_definition(filt, sizes):
    """On values in [-1, 2) (no f16 overflow under the overshoot of the filters with negative lobes, which the bound does not model)."""
    (sw, sh), (dw, dh) = sizes
    src = (np.random.default_rng(5).random((sh, sw, 4), dtype=np.float32) * 3.0 - 1.0).astype(np.float16).view(np.uint16)
    got = resample_ref.resample(src, (dh, dw), filt, STRAIGHT).view(np.float16).astype(np.float64)
    want = resample_ref.direct(src, (dh, dw), filt, STRAIGHT)
    m = float(np.abs(src.view(np.float16).astype(np.float64)).max())
    bound = _bound(filt, (sw, sh), (dw, dh), m, want)
    err = np.abs(got - want)
    print("max err / bound:", float((err / bound).max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("filt", FILTERS)
def test_a_constant_straight_image_stays_constant(filt):
    """D of a constant image is the constant (the exact taps of a window sum to 1), so the bound above holds against it."""
    for bits in (0x3C00, 0x3555, 0xB8CD, 0x57FF):
        src = np.full((9, 37, 4), bits, np.uint16)
        c = float(np.uint16(bits).view(np.float16))
        for (dw, dh) in ((37, 9), (11, 4), (53, 20), (3, 1)):
            got = resample_ref.resample(src, (dh, dw), filt, STRAIGHT).view(np.float16).astype(np.float64)
            d = np.full(got.shape, c)
            assert np.all(np.abs(got - d) <= _bound(filt, (37, 9), (dw, dh), abs(c), d)), (bits, dw, dh)


VARIANTS = {"unfused": {"fused": False}, "descending": {"descending": True}, "centre_i_scale": {"centre_half": False},
            "unrenormalised": {"renormalise": False}, "no_premultiply": {"premultiply": False}, "columns_first": {"rows_first": False}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_battery_tells_the_rule_from_a_near_miss(variant):
    """Each wrong variant differs from the reference in at least one texel of at least one case of the battery (the search stops at
    the first such case; the count of cases tried is printed)."""
    tried = 0
    for c in resample_cases.CASES:
        if c["src_size"][0] * c["src_size"][1] > 3000 or c["kind"] in ("never", "zeros"):
            continue  # (the small cases are enough to tell, and quick)
        tried += 1
        w, h = c["dst_size"]
        wrong = resample_ref.resample(resample_cases.source(c), (h, w), c["filter"], c["flags"], c["src_rect"], c["dst_rect"], resample_cases.before(c),
                                      **VARIANTS[variant])
        if not resample_ref.same_bits(wrong, resample_cases.expected(c["name"])):
            print(variant, "differs on", c["name"], "after", tried, "cases")
            return
    pytest.fail("no case of the battery tells the variant '%s' from the rule: add a case" % variant)


def test_the_battery_covers_what_it_claims():
    cases = resample_cases.CASES
    assert len(cases) > 120 and len(resample_cases.BY_NAME) == len(cases)
    ext = lambda c, which, k: resample_cases.rect_of(c, which)[2 + k]  # noqa: E731
    for filt in FILTERS:
        for k, pairs in ((0, resample_cases.X_PAIRS), (1, resample_cases.Y_PAIRS)):
            for pair in pairs:
                assert any(c["filter"] == filt and (ext(c, "src", k), ext(c, "dst", k)) == pair for c in cases), (filt, k, pair)
    for flags in (0, STRAIGHT):
        assert any(c["flags"] == flags and (ext(c, "src", 0), ext(c, "dst", 0), ext(c, "src", 1), ext(c, "dst", 1)) == (1040, 65, 48, 3) for c in cases)
        assert {c["kind"] for c in cases if c["flags"] == flags} == set(resample_cases.KINDS)
        assert any(c["flags"] == flags and c["src_rect"] and c["src_rect"][0] % 2 and c["dst_rect"][0] % 2 for c in cases)
    assert {ext(c, "dst", 0) for c in cases} >= set(resample_cases.ITEM_WIDTHS)
    assert {ext(c, "dst", 1) for c in cases} >= set(resample_cases.ITEM_HEIGHTS)
    assert all(c["src_size"][0] <= 1100 and c["src_size"][1] <= 48 for c in cases)
    assert any(c["prior"] == "never" for c in cases)
    # 16 n - 1 : n is legal and 16 n + 1 : n is not
    assert resample_ref.sizes_ok(143, 9) and not resample_ref.sizes_ok(145, 9)
