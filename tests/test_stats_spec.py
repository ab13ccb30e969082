"""The stats rule on the CPU: the codes of the library and of its host twin over every f16 pattern, the plan from
both, the ctypes mirrors against the compiled header, records worked by hand, the consequences the rule states, jello_amd.stats'
merge, levels and equalize against their stated arithmetic, the stand-alone check of include/jello_stats.h (tools/stats_check.cpp)
built with the sanitizers and its printed record against the reference, and that the battery (tests/stats_cases.py) tells the rule
from ten near misses."""
import ctypes
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import jello_amd
from jello_amd import StatsPopulation, StatsTransfer, StatsWhat, _lib
from jello_amd import stats as jstats
from jello_amd.imagecalls import ColorFunc

import stats_cases
import stats_ref
import surface_ref
from abi_text import INCLUDE, ROOT, c_values, go_calls, header_arity
from stats_ref import ALL, BOUNDS, CONTENT, EVERYTHING, EXTREMES, HISTOGRAM, LINEAR, SRGB

ONE, HALF, NAN, NEG0, INF, NINF = 0x3C00, 0x3800, 0x7E00, 0x8000, 0x7C00, 0xFC00
PATTERNS = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def _stats(bits, **kw):
    return jstats.Stats(stats_ref.record_bytes(np.asarray(bits, np.uint16), **kw))


# ---- the codes ----

def _half_even(x):
    """Round-half-even of a Fraction."""
    f = x.numerator // x.denominator
    r = x - f
    return f + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2) else 0)


@pytest.mark.parametrize("twin", [False, True])
def test_the_linear_codes_are_round_half_even_of_255_q_exactly(built, twin):
    got = jello_amd.stats_codes(PATTERNS, StatsTransfer.LINEAR, twin=twin)
    v = PATTERNS.view(np.float16).astype(np.float64)
    want = np.zeros(65536, np.int64)
    ties = 0
    for i in np.flatnonzero((v > 0) & (v < 1)):  # (NaN, -0 and everything <= 0 clamp to 0, +Inf and everything >= 1 to 1)
        x = 255 * Fraction(float(v[i]))
        want[i] = _half_even(x)
        ties += x.denominator == 2
    want[v >= 1] = 255
    assert np.array_equal(got, want) and ties == 1  # (255 is odd, so 255 q has q's denominator: the one tie is 127.5 at q = 1/2)
    assert got[HALF] == 128 and got[0x1804] == 0 and got[NAN] == 0 and got[0xFE00] == 0 and got[NEG0] == 0 and got[INF] == 255 and got[NINF] == 0
    assert np.array_equal(got, stats_ref.codes(PATTERNS, False))


@pytest.mark.parametrize("twin", [False, True])
def test_the_srgb_codes_are_jh_blits(built, twin):
    """Against tests/surface_ref.py's encode rule (binary64 pow), which is what jh_blit's surfaces are held to."""
    got = jello_amd.stats_codes(PATTERNS, StatsTransfer.SRGB, twin=twin)
    want = surface_ref.srgb8(surface_ref.clamp01(PATTERNS.view(np.float16).astype(np.float32)))
    assert np.array_equal(got, want) and len(np.unique(got)) == 256
    assert got[NAN] == 0 and got[NEG0] == 0 and got[INF] == 255 and got[ONE] == 255 and got[HALF] == 188


def test_the_codes_queries_refuse_what_the_rule_refuses(built):
    for twin in (False, True):
        for bad in (2, -1):
            with pytest.raises(ValueError, match="jh_stats: "):
                jello_amd.stats_codes(PATTERNS[:4], bad, twin=twin)
        q = jello_amd.imagecalls._query("stats_codes", twin)
        codes = np.full(4, 0xA5, np.uint8)
        bits = PATTERNS[:4].copy()
        assert q(0, 4, None, codes.ctypes.data) != 0 and q(0, 4, bits.ctypes.data, None) != 0 and q(5, 4, bits.ctypes.data, codes.ctypes.data) != 0
        assert np.all(codes == 0xA5)
        assert q(1, 0, None, None) == 0


# ---- the header, the plan ----

def test_the_headers_constants_and_the_mirrors_layout():
    names = ["JH_STATS_ALL", "JH_STATS_CONTENT", "JH_STATS_LINEAR", "JH_STATS_SRGB", "JH_STATS_BOUNDS", "JH_STATS_EXTREMES", "JH_STATS_HISTOGRAM",
             "JH_STATS_MAX_TEXELS", "JH_STATS_MAX_PARTIALS"]
    assert c_values(names) == [0, 1, 0, 1, 1, 2, 4, 1 << 31, 1024]
    assert [int(v) for v in StatsPopulation] == [ALL, CONTENT] and [int(v) for v in StatsTransfer] == [LINEAR, SRGB]
    assert [int(StatsWhat.BOUNDS), int(StatsWhat.EXTREMES), int(StatsWhat.HISTOGRAM), int(StatsWhat.ALL)] == [BOUNDS, EXTREMES, HISTOGRAM, EVERYTHING]
    assert jello_amd.engine.STATS_MAX_TEXELS == stats_ref.MAX_TEXELS and jello_amd.engine.STATS_MAX_PARTIALS == 1024
    for struct, ctype in (("jh_stats_desc", _lib.CStatsDesc), ("jh_stats_record", _lib.CStatsRecord), ("jh_stats_plan_t", _lib.CStatsPlan)):
        fields = [name for name, _ in ctype._fields_]
        want = c_values(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, f) for f in fields])
        assert [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] == want, struct
    # the numpy views of the record: jello_amd.stats' and the reference's
    for dtype in (jstats.RECORD, stats_ref.RECORD):
        assert dtype.itemsize == ctypes.sizeof(_lib.CStatsRecord) == jello_amd.engine.STATS_RECORD_BYTES
        assert [dtype.fields[name][1] for name, _ in _lib.CStatsRecord._fields_] == [getattr(_lib.CStatsRecord, name).offset for name, _ in _lib.CStatsRecord._fields_]


def test_the_abi_text_names_the_call():
    arity = header_arity()
    assert (arity["jh_stats"], arity["jh_stats_plan"], arity["jh_stats_codes"]) == (4, 4, 4)
    calls = dict(go_calls())
    for name in ("jh_stats", "jh_stats_plan", "jh_stats_codes"):
        assert calls.get(name) == arity[name], name


def test_the_descriptor_python_builds():
    d = jello_amd.engine._stats_desc(StatsWhat.BOUNDS | StatsWhat.HISTOGRAM, 2, 0.25, StatsPopulation.CONTENT, StatsTransfer.SRGB, (1, 2, 3, 4))
    assert (d.what, d.channel, d.threshold, d.population, d.transfer, d.x, d.y, d.width, d.height) == (5, 2, 0.25, 1, 1, 1, 2, 3, 4)
    d = jello_amd.engine._stats_desc()
    assert (d.what, d.channel, d.threshold, d.population, d.transfer, d.width, d.height) == (7, 3, 2.0 ** -24, 0, 0, 0, 0)
    for bad in (dict(what=-1), dict(what=2.5), dict(what=1 << 32)):
        with pytest.raises(ValueError, match="jh_stats: "):
            jello_amd.engine._stats_desc(**bad)


def test_the_plan_from_the_library_and_from_its_twin(built):
    """Bit for bit the same plan, and the same legality on both sides of every boundary.  Descriptor arithmetic only."""
    size = (100, 50)
    legal = [dict(what=w) for w in range(1, 8)] + [dict(channel=0), dict(channel=3, population=StatsPopulation.CONTENT, transfer=StatsTransfer.SRGB),
                                                    dict(threshold=-3.0e38), dict(threshold=3.0e38), dict(rect=(99, 49, 1, 1)), dict(rect=(0, 0, 100, 50)),
                                                    dict(rect=(3, 5, 40, 20))]
    for kw in legal:
        a, b = jello_amd.stats_plan(size, **kw), jello_amd.stats_plan(size, twin=True, **kw)
        assert a == b, kw
        assert a == dict(rect=kw.get("rect") or (0, 0) + size, launches=2, record_bytes=4184, scratch_bytes=1024 * 4168), kw
    for twin in (False, True):
        assert jello_amd.stats_plan((0, 0), twin=twin) == dict(rect=(0, 0, 0, 0), launches=1, record_bytes=4184, scratch_bytes=0)
        # 2^31 texels are legal, one more is refused
        assert jello_amd.stats_plan((65536, 32768), twin=twin)["rect"] == (0, 0, 65536, 32768)
        assert jello_amd.stats_plan((1 << 31, 1), twin=twin)["launches"] == 2
        assert jello_amd.stats_plan(((1 << 31) + 1, 1), rect=(1, 0, 1 << 31, 1), twin=twin)["rect"] == (1, 0, 1 << 31, 1)
    inf, nan = float("inf"), float("nan")
    illegal = [dict(what=0), dict(what=8), dict(what=15), dict(channel=-1), dict(channel=4), dict(population=2), dict(population=-1), dict(transfer=2),
               dict(transfer=-1), dict(threshold=inf), dict(threshold=-inf), dict(threshold=nan), dict(threshold=1e39), dict(rect=(99, 49, 2, 1)),
               dict(rect=(0, 0, 100, 51)), dict(rect=(100, 0, 1, 1)), dict(rect=(2, 2, 0, 4)), dict(rect=(2, 2, 4, 0)), dict(rect=(0xFFFFFFFF, 0, 2, 2))]
    for kw in illegal:
        for twin in (False, True):
            with pytest.raises(ValueError, match="jh_stats: "):
                jello_amd.stats_plan(size, twin=twin, **kw)
            with pytest.raises(ValueError, match="jh_stats: "):
                jello_amd.stats_plan(((1 << 31) + 1, 1), twin=twin)
            with pytest.raises(ValueError, match="jh_stats: "):
                jello_amd.stats_plan((65536, 32769), twin=twin)
    for kw in illegal:  # the reference refuses the same
        with pytest.raises(ValueError, match="jh_stats: "):
            stats_ref.stats(np.zeros((50, 100, 4), np.uint16), **kw)
    d = jello_amd.engine._stats_desc()
    for twin in (False, True):
        q = jello_amd.imagecalls._query("stats_plan", twin)
        plan = _lib.CStatsPlan()
        ctypes.memset(ctypes.byref(plan), 0xA5, ctypes.sizeof(plan))
        bad = jello_amd.engine._stats_desc(what=8)
        assert q(ctypes.byref(bad), 10, 10, ctypes.byref(plan)) != 0 and q(None, 10, 10, ctypes.byref(plan)) != 0 and q(ctypes.byref(d), 10, 10, None) != 0
        plan2 = _lib.CStatsPlan()
        ctypes.memset(ctypes.byref(plan2), 0xA5, ctypes.sizeof(plan2))
        assert q(ctypes.byref(bad), 10, 10, ctypes.byref(plan2)) != 0 and bytes(plan2) == b"\xa5" * ctypes.sizeof(plan2)  # untouched on refusal
    if not hasattr(jello_amd.load_host(), "jl_stats_plan"):
        pytest.fail("the host twin lacks jl_stats_plan")


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    d = jello_amd.engine._stats_desc()
    assert hip.jh_stats(None, 1, ctypes.byref(d), 8) == -1  # JH_ERR_INVALID
    assert hip.jh_stats(None, 1, None, None) == -1


# ---- records worked by hand ----

def _texel(r, g, b, a):
    return [np.float16(v).view(np.uint16) for v in (r, g, b, a)]


def test_a_three_by_two_image_by_hand():
    """Row 0: transparent, half-red at alpha 1, white at alpha 0.5.  Row 1: a NaN green at alpha 1, transparent, black at alpha 0.25."""
    bits = np.array([[_texel(0, 0, 0, 0), _texel(0.5, 0, 0, 1), _texel(1, 1, 1, 0.5)],
                     [[0, NAN, 0, ONE], _texel(0, 0, 0, 0), _texel(0, -0.0, 0, 0.25)]], np.uint16)
    s = _stats(bits, threshold=0.5)  # content: alpha >= 0.5
    assert s.rect == (0, 0, 3, 2) and (int(s.what), s.population, s.transfer) == (7, ALL, LINEAR)
    assert s.content_count == 3 and tuple(s.record["bounds"]) == (0, 0, 3, 2) and s.bounds == (0, 0, 3, 2)
    assert s.population_count == 6 and s.nan_count == (0, 1, 0, 0)
    assert s.min_bits == (0, NEG0, 0, 0) and s.max_bits == (ONE, ONE, ONE, ONE)  # (the NaN is no extreme; -0 < +0)
    h = s.histogram
    assert h[0][0] == 4 and h[0][128] == 1 and h[0][255] == 1 and h[0].sum() == 6
    assert h[1][0] == 5 and h[1][255] == 1  # (the NaN and the -0 count in bin 0)
    assert h[3][0] == 2 and h[3][255] == 2 and h[3][128] == 1 and h[3][64] == 1  # alpha: 0, 0, 1, 1, 0.5 -> 127.5 -> 128, 0.25 -> 63.75 -> 64
    c = _stats(bits, threshold=0.5, population=CONTENT, transfer=SRGB)
    assert c.population_count == 3 and c.nan_count == (0, 1, 0, 0) and c.content_count == 3
    assert c.min_bits == (0, 0, 0, HALF) and c.max_bits == (ONE, ONE, ONE, ONE)
    assert c.histogram[0][188] == 1 and c.histogram[0][255] == 1 and c.histogram[0][0] == 1  # sRGB(0.5) = 188
    assert c.histogram[3][128] == 1 and c.histogram[3][255] == 2  # alpha stays LINEAR
    r = _stats(bits, threshold=0.5, rect=(1, 0, 1, 2))
    assert r.content_count == 1 and tuple(r.record["bounds"]) == (1, 0, 2, 1) and r.population_count == 2


def test_a_nan_only_channel_signed_zeros_and_no_content_by_hand():
    bits = np.zeros((2, 2, 4), np.uint16)
    bits[..., 0] = [[NAN, 0xFE00], [0x7FFF, 0xFC01]]
    bits[..., 1] = [[0, NEG0], [NEG0, 0]]
    bits[..., 2] = [[NEG0, NEG0], [NEG0, NEG0]]
    s = _stats(bits, threshold=0.5)
    assert s.content_count == 0 and tuple(s.record["bounds"]) == (0, 0, 0, 0) and s.bounds is None
    assert s.nan_count == (4, 0, 0, 0) and s.min_bits[0] == 0x7C00 and s.max_bits[0] == 0xFC00  # the neutral elements
    assert (s.min_bits[1], s.max_bits[1]) == (NEG0, 0) and (s.min_bits[2], s.max_bits[2]) == (NEG0, NEG0) and (s.min_bits[3], s.max_bits[3]) == (0, 0)
    assert s.histogram[0][0] == 4 and s.population_count == 4  # a NaN counts in bin 0 and in nan_count
    assert s.minimum[0] == float("inf") and s.maximum[0] == float("-inf")
    c = _stats(bits, threshold=0.5, population=CONTENT)
    assert c.population_count == 0 and not c.histogram.any() and c.min_bits == (0x7C00,) * 4 and c.max_bits == (0xFC00,) * 4
    z = _stats(bits, threshold=-0.0, channel=2)  # -0 >= -0, and -0 >= +0 holds as well
    assert z.content_count == 4 and _stats(bits, threshold=0.0, channel=2).content_count == 4


def test_parts_not_asked_for_are_zeros_and_an_image_without_texels_is_zeros():
    bits = stats_cases.content("values", None, 9, 7, 3, None, seed=3)
    full = _stats(bits, threshold=0.5).record
    for what in range(1, 8):
        r = _stats(bits, threshold=0.5, what=what).record
        assert r["content_count"] == full["content_count"]
        assert np.array_equal(r["bounds"], full["bounds"] if what & BOUNDS else np.zeros(4))
        assert r["population_count"] == (full["population_count"] if what & (EXTREMES | HISTOGRAM) else 0)
        assert np.array_equal(r["nan_count"], full["nan_count"] if what & (EXTREMES | HISTOGRAM) else np.zeros(4))
        assert np.array_equal(r["min_bits"], full["min_bits"] if what & EXTREMES else np.zeros(4))  # zeros, not the neutral elements
        assert np.array_equal(r["max_bits"], full["max_bits"] if what & EXTREMES else np.zeros(4))
        assert np.array_equal(r["histogram"], full["histogram"] if what & HISTOGRAM else np.zeros((4, 256)))
    none = stats_ref.stats(np.zeros((0, 0, 4), np.uint16), population=CONTENT, transfer=SRGB)
    assert none.tobytes() == np.array([0, 0, 0, 0, 7, 1, 1, 0], "<u4").tobytes() + bytes(4184 - 32)


# ---- the consequences the rule states ----

def _random_image(rng, w, h):
    return rng.choice(np.array(stats_cases.VALUES, np.uint16), (h, w, 4))


def test_each_histogram_row_sums_to_the_population():
    for name in [c["name"] for c in stats_cases.CASES if c["what"] & HISTOGRAM]:
        r = jstats.Stats(stats_cases.expected(name))
        assert np.all(r.histogram.sum(axis=1) == r.population_count), name


def test_content_with_the_most_negative_threshold_is_all_on_a_nan_free_image():
    rng = np.random.default_rng(5)
    bits = rng.choice(np.array([v for v in stats_cases.VALUES if (v & 0x7FFF) <= 0x7C00 and v != NINF], np.uint16), (11, 13, 4))
    lowest = float(np.finfo(np.float32).min)
    a = stats_ref.stats(bits, population=ALL, threshold=lowest)
    c = stats_ref.stats(bits, population=CONTENT, threshold=lowest)
    c["population"] = ALL
    assert a.tobytes() == c.tobytes() and a["content_count"] == 11 * 13
    with pytest.raises(ValueError, match="jh_stats: "):  # -Inf would say it outright, and is refused
        stats_ref.stats(bits, population=CONTENT, threshold=float("-inf"))
    with pytest.raises(ValueError, match="jh_stats: "):
        jello_amd.stats_plan((13, 11), population=StatsPopulation.CONTENT, threshold=float("-inf"))


def test_merge_of_four_quadrants_is_the_whole():
    rng = np.random.default_rng(6)
    for n in range(50):
        w, h = int(rng.integers(1, 12)) * 2 + 1, int(rng.integers(1, 10)) * 2 + 1  # odd sizes from 3 up
        bits = _random_image(rng, w, h)
        kw = dict(what=int(rng.integers(1, 8)), channel=int(rng.integers(0, 4)), threshold=[0.0, 0.5, 2.0 ** -24][n % 3], population=n & 1,
                  transfer=(n >> 1) & 1)
        cx, cy = int(rng.integers(1, w)), int(rng.integers(1, h))
        whole = _stats(bits, **kw)
        parts = [_stats(bits, rect=r, **kw) for r in ((0, 0, cx, cy), (cx, 0, w - cx, cy), (0, cy, cx, h - cy), (cx, cy, w - cx, h - cy))]
        merged = jstats.merge(jstats.merge(parts[0], parts[1]), jstats.merge(parts[2], parts[3]))
        assert merged == whole, (n, w, h, kw)
        assert jstats.merge(jstats.merge(parts[3], parts[0]), jstats.merge(parts[1], parts[2])) == whole  # (in any order)
    empty = _stats(np.zeros((0, 0, 4), np.uint16), **kw)
    assert jstats.merge(empty, whole) == whole and jstats.merge(whole, empty) == whole
    with pytest.raises(ValueError, match="jh_stats: "):
        jstats.merge(whole, _stats(bits, **dict(kw, population=1 - kw["population"])))
    with pytest.raises(ValueError, match="jh_stats: "):
        jstats.Stats(b"\0" * 100)
    assert jstats.parse(whole.tobytes()) == whole


def test_the_bounds_are_the_box_of_argwhere():
    rng = np.random.default_rng(7)
    for n in range(30):
        w, h = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        bits = np.zeros((h, w, 4), np.uint16)
        bits[..., 3] = np.where(rng.random((h, w)) < 0.03, ONE, 0)
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        rect = (x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1)))
        s = _stats(bits, what=BOUNDS, rect=rect, threshold=0.5)
        inside = np.zeros((h, w), bool)
        inside[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
        at = np.argwhere((bits[..., 3] == ONE) & inside)
        if len(at) == 0:
            assert s.bounds is None and s.content_count == 0
        else:
            (y0, x0), (y1, x1) = at.min(axis=0), at.max(axis=0)
            assert s.bounds == (x0, y0, x1 - x0 + 1, y1 - y0 + 1) and s.content_count == len(at)


# ---- levels and equalize ----

def _hist_record(rows, transfer=LINEAR):
    r = np.zeros((), stats_ref.RECORD)
    r["what"], r["width"], r["height"], r["transfer"] = HISTOGRAM, 1, 1, transfer
    r["histogram"] = rows
    r["population_count"] = int(np.sum(rows[0]))
    return jstats.Stats(r.tobytes())


def test_levels_against_its_arithmetic():
    two = np.zeros(256, np.int64)
    two[51], two[204] = 30, 70  # two spikes at 0.2 and 0.8
    flat = np.ones(256, np.int64) * 4
    tail = two.copy()
    tail[0], tail[255] = 1, 1  # 102 texels: one outlier at each end
    none = np.zeros(256, np.int64)
    s = _hist_record([two, flat, tail, none])
    assert jstats.percentile_codes(two) == (51, 204) and jstats.percentile_codes(flat) == (0, 255) and jstats.percentile_codes(tail) == (0, 255)
    assert jstats.percentile_codes(none) is None
    # 1 %: floor(0.01 N) texels may saturate at each end -- none of 100, one of 102, ten of 1024 (the flat one: 4 to a bin: bins 2 and 253)
    assert jstats.percentile_codes(two, (0.01, 0.01)) == (51, 204) and jstats.percentile_codes(tail, (0.01, 0.01)) == (51, 204)
    assert jstats.percentile_codes(flat, (0.01, 0.01)) == (2, 253)
    assert jstats.percentile_codes(two, (0.3, 0.0)) == (204, 204) and jstats.percentile_codes(two, (0.29, 0.0)) == (51, 204)
    lv = jstats.levels(s)
    assert lv[0] == (ColorFunc.LINEAR, 255.0 / 153, -51.0 / 153) and lv[1] == (ColorFunc.LINEAR, 1.0, 0.0) and lv[2] == (ColorFunc.LINEAR, 1.0, 0.0)
    assert lv[3] == (ColorFunc.LINEAR, 1.0, 0.0)  # no population: the identity
    for (_, slope, intercept), (lo, hi) in ((lv[0], (51, 204)),):
        assert abs(lo / 255.0 * slope + intercept) < 1e-15 and abs(hi / 255.0 * slope + intercept - 1) < 1e-15
    lv = jstats.levels(s, (0.01, 0.01))
    assert lv[2] == (ColorFunc.LINEAR, 255.0 / 153, -51.0 / 153) and lv[1] == (ColorFunc.LINEAR, 255.0 / 251, -2.0 / 251)
    assert jstats.levels(_hist_record([two * 0 + np.eye(256, dtype=np.int64)[7]] * 4))[0] == (ColorFunc.LINEAR, 1.0, 0.0)  # one spike: hi == lo
    for bad in ((-0.1, 0), (0, 1.0)):
        with pytest.raises(ValueError, match="jh_stats: "):
            jstats.levels(s, bad)
    with pytest.raises(ValueError, match="jh_stats: "):
        jstats.levels(_stats(np.zeros((2, 2, 4), np.uint16), what=BOUNDS))


def test_equalize_against_its_arithmetic():
    two = np.zeros(256, np.int64)
    two[51], two[204] = 30, 70
    flat = np.ones(256, np.int64) * 4
    s = _hist_record([two, flat, np.zeros(256, np.int64), np.eye(256, dtype=np.int64)[9] * 5])
    eq = jstats.equalize(s, 6)  # inputs k / 5: codes 0, 51, 102, 153, 204, 255
    assert eq[0] == (ColorFunc.TABLE, (0.0, 0.0, 0.0, 0.0, 1.0, 1.0))  # m = 30: (30 - 30) / 70 up to code 203, (100 - 30) / 70 from 204
    assert eq[1] == (ColorFunc.TABLE, tuple((4 * (51 * k + 1) - 4) / 1020 for k in range(6)))  # flat: the identity ramp k / 5
    assert eq[1][1] == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
    assert eq[2] == eq[3] == (ColorFunc.TABLE, (0.0, 0.2, 0.4, 0.6, 0.8, 1.0))  # no population, one occupied bin: the identity
    full = jstats.equalize(s)
    assert len(full[0][1]) == 64 and full[1][1][0] == 0.0 and full[1][1][-1] == 1.0 and all(b >= a for a, b in zip(full[1][1], full[1][1][1:]))
    for bad in (1, 65):
        with pytest.raises(ValueError, match="jh_stats: "):
            jstats.equalize(s, bad)


# ---- the stand-alone check ----

@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/stats_check.cpp, a program with a main of its own, built with ASan and UBSan as its header says."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("stats_check") / "stats_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wno-comment", "-I", INCLUDE, os.path.join(ROOT, "tools", "stats_check.cpp"), "-o", exe])
    return exe


def test_the_stand_alone_check_passes_under_the_sanitizers(check_program):
    """Legality, the 16-bit key against jmorph_key over all patterns, the codes, the record from the header's pieces against a brute
    force, the combine over every split."""
    out = subprocess.check_output([check_program]).decode()
    assert out.startswith("ok: 2688 records from the pieces, 99 splits"), out


@pytest.mark.parametrize("population", [ALL, CONTENT])
@pytest.mark.parametrize("transfer", [LINEAR, SRGB])
def test_the_programs_record_is_the_references(check_program, population, transfer):
    """The record the program prints for a rectangle of an 11 x 7 image -- the header's pieces, three partials -- against
    tests/stats_ref.py -- the set."""
    w, h = 11, 7
    bits = _random_image(np.random.default_rng(10 + 2 * population + transfer), w, h)
    for what, rect, threshold, channel in ((7, (0, 0, 0, 0), 0.5, 3), (7, (3, 1, 7, 5), 0.0, 1), (5, (10, 6, 1, 1), 2.0 ** -24, 0), (2, (0, 2, 11, 3), 7.0e4, 2)):
        text = subprocess.check_output([check_program, str(w), str(h), str(what), str(channel), repr(threshold), str(population), str(transfer)] +
                                       [str(v) for v in rect] + ["".join("%04x" % v for v in bits.reshape(-1))]).decode()
        got = np.array([int(t) for t in text.split()], "<u4").tobytes()
        want = stats_ref.record_bytes(bits, what=what, channel=channel, threshold=threshold, population=population, transfer=transfer, rect=rect)
        assert got == want, (what, rect)


# ---- sensitivity: the battery tells the rule from its near misses ----

NEAR_MISSES = {
    # variant: (the keywords that build it, a case of the battery that catches it)
    "> in place of >=": (dict(ge=False), "37x21_values_thalf_w7_content_linear_ch0"),
    "truncation in the LINEAR code": (dict(half_even=False), "37x21_values_thalf_w7_content_linear_ch0"),
    "a NaN skipped by the histogram": (dict(nan_in_histogram=False), "37x21_nan_channel_w7_all_srgb_ch3"),
    "a NaN taking part in the extremes": (dict(nan_in_extremes=True), "37x21_values_thalf_w7_content_linear_ch0"),
    "+0 below -0": (dict(zero_order=False), "37x21_set_zeros_w7_all_srgb_ch3"),
    "an inclusive x1": (dict(exclusive=False), "67x41_mask_one_w1_all_linear_ch2_r11_7_45_27"),
    "bounds relative to the rectangle": (dict(image_coordinates=False), "67x41_mask_one_w1_all_linear_ch2_r11_7_45_27"),
    "the population ignored": (dict(use_population=False), "67x41_mask_corners_w7_content_linear_ch3_r11_7_45_27"),
    "alpha under the sRGB code": (dict(alpha_linear=False), "515x5_alternate_w7_all_srgb_ch3"),
    "texels just outside the rectangle counted": (dict(inside_only=False), "67x41_mask_none_w1_all_linear_ch2_r11_7_45_27"),
}


@pytest.mark.parametrize("what", sorted(NEAR_MISSES))
def test_the_battery_tells_the_rule_from_a_near_miss(what):
    variant, name = NEAR_MISSES[what]
    want, got = stats_cases.expected(name), stats_cases.expected(name, **variant)
    differ = int(np.count_nonzero(np.frombuffer(want, np.uint8) != np.frombuffer(got, np.uint8)))
    print("%s: %d of %d bytes differ on %s" % (what, differ, len(want), name))
    assert differ > 0, (what, name)
    caught = [c["name"] for c in stats_cases.CASES if stats_cases.expected(c["name"]) != stats_cases.expected(c["name"], **variant)]
    print("    caught by %d of %d cases" % (len(caught), len(stats_cases.CASES)))


def test_the_battery_covers_what_it_claims():
    cases = stats_cases.CASES
    assert len(cases) > 150 and all(c["w"] * c["h"] <= 65536 for c in cases)
    for size in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (1, 1024), (1, 1030)) + tuple((w, h) for w in (511, 512, 513, 514) for h in (1, 2, 3)):
        assert any((c["w"], c["h"]) == size for c in cases), size
    assert {c["inst"] for c in cases} == set(stats_cases.INSTANTIATIONS)
    for i in stats_cases.INSTANTIATIONS:  # every instantiation on the smallest sizes, across an item's end and beyond the grid cap
        for size in ((1, 1), (3, 3), (513, 3), (1, 1030)):
            assert any(c["inst"] == i and (c["w"], c["h"]) == size for c in cases), (i, size)
    assert {(c["what"], c["population"], c["transfer"]) for c in cases if c["kind"] == "patterns"} == set(stats_cases.COMBOS)
    assert {c["channel"] for c in cases} == {0, 1, 2, 3}
    assert {c["kind"] for c in cases} >= {"values", "patterns", "constant", "alternate", "set", "nan_channel", "mask", "blob", "diagonal", "never"}
    assert any(c["rect"] is not None and c["rect"][0] % 2 and c["rect"][1] % 2 for c in cases) and any(c["rect"] == (33, 17, 1, 1) for c in cases)
    thresholds = {np.float32(c["threshold"]).tobytes() for c in cases}
    for t in (0.0, -0.0, 0.5, 2.0 ** -24, stats_cases.ABOVE_FINITE):
        assert np.float32(t).tobytes() in thresholds, t
    for v in stats_cases.VALUES:
        assert (stats_cases.content("values", None, 37, 21, 3, None, seed=1) == v).any(), hex(v)
    assert np.array_equal(np.sort(stats_cases.all_patterns().reshape(-1, 4), axis=0), np.repeat(PATTERNS[:, None], 4, axis=1))
