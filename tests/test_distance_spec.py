"""The distance rule on the CPU: the ctypes mirrors and the enums against the compiled header, the plan from the
library and from its host twin, the stand-alone check of include/jello_distance.h (tools/distance_check.cpp) built with the sanitizers
and its printed D against the reference, texels worked by hand, the consequences the rule states, and that the battery
(tests/distance_cases.py) tells the rule from nine near misses."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import DistanceEdge, DistanceFlags, DistanceWhich, _lib
from jello_amd import distance as ramps

import distance_cases
import distance_ref
from abi_text import INCLUDE, ROOT, c_values
from distance_ref import CLAMP, INNER, OUTER, SIGNED, STRAIGHT, ZERO

ONE, HALF = 0x3C00, 0x3800
F = np.float32


def _image(rows):
    """(h, w, 4) uint16 from rows of 0 / 1: alpha 1 on the seeds."""
    m = np.array(rows, np.uint16)
    bits = np.zeros(m.shape + (4,), np.uint16)
    bits[..., 3] = np.where(m != 0, ONE, 0)
    return bits


def _values(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def _s(src, which, R, edge=ZERO, **kw):
    """(seed, Dout, Din) of alpha >= 0.5, as the reference has them."""
    return distance_ref.squared_distances(src, 3, 0.5, which, edge, R, **kw)


# ---- the header and the program ----

def test_the_headers_constants_and_the_mirrors_layout():
    names = ["JH_DISTANCE_OUTER", "JH_DISTANCE_INNER", "JH_DISTANCE_SIGNED", "JH_DISTANCE_EDGE_ZERO", "JH_DISTANCE_EDGE_CLAMP", "JH_DISTANCE_STRAIGHT",
             "JH_DISTANCE_MAX_RADIUS"]
    assert c_values(names) == [0, 1, 2, 0, 1, 1, 255]
    assert [int(v) for v in DistanceWhich] == [OUTER, INNER, SIGNED] and [int(v) for v in DistanceEdge] == [ZERO, CLAMP]
    assert int(DistanceFlags.STRAIGHT) == STRAIGHT and jello_amd.engine.DISTANCE_MAX_RADIUS == distance_ref.MAX_RADIUS
    for struct, ctype in (("jh_distance_desc", _lib.CDistanceDesc), ("jh_dist_plan", _lib.CDistPlan)):
        fields = [name for name, _ in ctype._fields_]
        want = c_values(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, f) for f in fields])
        assert [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] == want, struct


def test_the_descriptor_python_builds():
    d = jello_amd.engine._distance_desc(2, 0.25, DistanceWhich.SIGNED, DistanceEdge.CLAMP, 17, -0.5, 1.5, (0.1, 0.2, 0.3, 0.4), (1, 2, 3, 4), True)
    assert (d.channel, d.threshold, d.which, d.edge, d.max_distance, d.scale, d.offset, d.flags, d.x, d.y, d.width, d.height) == \
        (2, 0.25, 2, 1, 17, -0.5, 1.5, 1, 1, 2, 3, 4)
    assert [F(v) for v in d.color] == [F(0.1), F(0.2), F(0.3), F(0.4)]
    d = jello_amd.engine._distance_desc()
    assert (d.channel, d.threshold, d.which, d.edge, d.max_distance, d.flags, d.width, d.height) == (3, 0.5, 0, 0, 1, 0, 0, 0)
    for bad in (dict(max_distance=-1), dict(max_distance=2.5), dict(color=(1, 1, 1))):
        with pytest.raises(ValueError, match="jh_distance: "):
            jello_amd.engine._distance_desc(**bad)


def test_the_plan_from_the_library_and_from_its_twin(built):
    """Bit for bit the same plan, and the same legality on both sides of every boundary."""
    size = (100, 50)
    legal = [dict(max_distance=1), dict(max_distance=255, which=DistanceWhich.SIGNED), dict(channel=0), dict(channel=3, edge=DistanceEdge.CLAMP, straight=True),
             dict(threshold=-3.0e38, scale=3.0e38, offset=-3.0e38), dict(rect=(99, 49, 1, 1)), dict(rect=(0, 0, 100, 50), which=DistanceWhich.INNER),
             dict(rect=(3, 5, 40, 20), which=DistanceWhich.SIGNED, max_distance=7)]
    for kw in legal:
        a, b = jello_amd.distance_plan(size, **kw), jello_amd.distance_plan(size, twin=True, **kw)
        assert a == b, kw
        R, planes = kw.get("max_distance", 1), 2 if kw.get("which") == DistanceWhich.SIGNED else 1
        x, y, w, h = kw.get("rect") or (0, 0) + size
        assert a == dict(rect=(x, y, w, h), radius=R, cap=(R + 1) ** 2, planes=planes, plane_columns=w + 2 * R, plane_rows=h,
                         scratch_bytes=planes * h * (w + 2 * R) * 2), kw
    assert jello_amd.distance_plan((0, 0))["scratch_bytes"] == 0
    inf, nan = float("inf"), float("nan")
    illegal = [dict(max_distance=0), dict(max_distance=256), dict(channel=-1), dict(channel=4), dict(which=-1), dict(which=3), dict(edge=-1), dict(edge=2),
               dict(threshold=inf), dict(threshold=nan), dict(scale=inf), dict(scale=nan), dict(offset=-inf), dict(offset=nan), dict(scale=1e39),
               dict(rect=(99, 49, 2, 1)), dict(rect=(0, 0, 100, 51)), dict(rect=(2, 2, 0, 4)), dict(rect=(2, 2, 4, 0)), dict(rect=(0xFFFFFFFF, 0, 2, 2))]
    for kw in illegal:
        for twin in (False, True):
            with pytest.raises(ValueError, match="jh_distance: "):
                jello_amd.distance_plan(size, twin=twin, **kw)
    d = jello_amd.engine._distance_desc()
    d.flags = 2
    for twin in (False, True):
        assert jello_amd.imagecalls._query("distance_plan", twin)(ctypes.byref(d), 10, 10, ctypes.byref(_lib.CDistPlan())) != 0
        assert jello_amd.imagecalls._query("distance_plan", twin)(None, 10, 10, ctypes.byref(_lib.CDistPlan())) != 0
        assert jello_amd.imagecalls._query("distance_plan", twin)(ctypes.byref(jello_amd.engine._distance_desc()), 10, 10, None) != 0


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    d = jello_amd.engine._distance_desc()
    assert hip.jh_distance(None, 1, 2, ctypes.byref(d)) == -1  # JH_ERR_INVALID
    assert hip.jh_distance(None, 1, 2, None) == -1


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/distance_check.cpp, a program with a main of its own, built with ASan and UBSan as its header says."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("distance_check") / "distance_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I", INCLUDE, os.path.join(ROOT, "tools", "distance_check.cpp"), "-o", exe])
    return exe


def test_the_stand_alone_check_passes_under_the_sanitizers(check_program):
    """The descriptors, the two passes built from the header's pieces (with the early stop) against the all-pairs set definition, the
    plane geometry against a count, and no NaN from any finite ramp."""
    out = subprocess.check_output([check_program]).decode()
    assert out.startswith("ok: 1440 decompositions"), out


@pytest.mark.parametrize("which", [OUTER, INNER, SIGNED])
@pytest.mark.parametrize("edge", [ZERO, CLAMP])
def test_the_programs_d_is_the_references(check_program, which, edge):
    """The D the program prints for a 19 x 13 image -- the header's pieces, two passes -- against tests/distance_ref.py -- the set."""
    w, h = 19, 13
    m = np.random.default_rng(which * 2 + edge).random((h, w)) < (0.7 if which == INNER else 0.12)
    src = _image(m.astype(np.uint16))
    for R in (1, 3, 255):
        text = subprocess.check_output([check_program, str(w), str(h), str(R), str(which), str(edge), "".join("1" if v else "0" for v in m.reshape(-1))]).decode()
        got = np.array([[int(t) for t in line.split()] for line in text.splitlines()], np.int64)
        seed, d_out, d_in = distance_ref.squared_distances(src, 3, 0.5, which, edge, R)
        want = d_out if which == OUTER else (d_in if which == INNER else np.where(seed, -d_in, d_out))
        assert np.array_equal(got, want), (which, edge, R)


# ---- texels worked by hand ----

def test_a_single_seed_by_hand():
    src = _image([[0] * 7] * 5)
    src[2, 3, 3] = ONE
    seed, d_out, d_in = _s(src, SIGNED, 2)
    assert d_out.tolist() == [[9, 8, 5, 4, 5, 8, 9], [9, 5, 2, 1, 2, 5, 9], [9, 4, 1, 0, 1, 4, 9], [9, 5, 2, 1, 2, 5, 9], [9, 8, 5, 4, 5, 8, 9]]  # CAP = 9: (3, 0) is 3 away
    assert seed.sum() == 1 and d_in[2, 3] == 1 and d_in[0, 0] == 0
    # OUTER, scale -1, offset 2.5: the disc of radius 2 -- 1 up to s = 1.5, 0.5 at s = 2, 2.5 - sqrt(5) at the knight's move, 0 from s = 2.5 on
    out = _values(distance_ref.distance(src, R=3, scale=-1.0, offset=2.5, flags=STRAIGHT))[..., 3]
    assert out[2, 3] == 1 and out[1, 2] == 1 and out[2, 1] == 0.5 and out[0, 3] == 0.5 and out[2, 0] == 0 and out[0, 0] == 0
    assert out[1, 1] == np.float64(np.float16(F(2.5) - np.sqrt(F(5.0))))


def test_the_edge_modes_by_hand():
    """A full 5 x 3 image: under ZERO the inner distance ends at the border -- min(X + 1, Y + 1, w - X, h - Y) -- under CLAMP nothing
    is a non-seed and every Din is the cap."""
    src = _image([[1] * 5] * 3)
    assert _s(src, INNER, 4, ZERO)[2].tolist() == [[1, 1, 1, 1, 1], [1, 4, 4, 4, 1], [1, 1, 1, 1, 1]]
    assert np.all(_s(src, INNER, 4, CLAMP)[2] == 25)
    assert np.all(_s(src, OUTER, 4, ZERO)[1] == 0)
    empty = _image([[0] * 5] * 3)
    assert np.all(_s(empty, OUTER, 4, ZERO)[1] == 25) and np.all(_s(empty, INNER, 4, CLAMP)[2] == 0)


def test_signed_by_hand():
    """Seeds in the right half of a row: s = ... -2.5, -1.5, -0.5 | 0.5, 1.5 ...: the zero crossing on the texel edge."""
    src = _image([[0, 0, 0, 1, 1, 1]])
    out = _values(distance_ref.distance(src, which=SIGNED, edge=CLAMP, R=5, scale=0.125, offset=0.5, flags=STRAIGHT))[0, :, 3]
    assert out.tolist() == [0.5 + 2.5 / 8, 0.5 + 1.5 / 8, 0.5 + 0.5 / 8, 0.5 - 0.5 / 8, 0.5 - 1.5 / 8, 0.5 - 2.5 / 8]
    far = _values(distance_ref.distance(_image([[0] * 4]), which=SIGNED, R=255, scale=1.0 / 512, offset=0.5, flags=STRAIGHT))[0, :, 3]
    assert np.all(far == np.float64(np.float16(0.5 + 255.5 / 512)))  # D = CAP: +255.5, "farther than R"


def test_the_seed_test_by_hand():
    vals = np.array([0x0000, 0x8000, 0x0001, 0x8001, HALF, ONE, 0x7C00, 0xFC00, 0x7E00, 0xFE00], np.uint16)
    src = np.zeros((1, len(vals), 4), np.uint16)
    src[0, :, 1] = vals
    s = lambda t: distance_ref.seeds(src, 1, t)[0].tolist()  # noqa: E731
    assert s(0.0) == s(-0.0) == [True, True, True, False, True, True, True, False, False, False]  # -0 >= +0 holds, a NaN is no seed
    assert s(2.0 ** -24) == [False, False, True, False, True, True, True, False, False, False]
    assert s(7.0e4) == [False] * 6 + [True] + [False] * 3
    assert s(-3.0e38) == [True] * 7 + [False] * 3  # (-Inf is below every finite threshold)


# ---- the consequences the rule states ----

def test_outer_with_the_outline_ramp_is_the_disc_dilate_and_inner_the_disc_erode():
    """Away from the one-texel ramp the coverage is 0 or 1 exactly as the disc says: 1 where a seed lies within w - 0.5, 0 where none
    lies within w + 0.5; the erode likewise on the complement."""
    src = distance_cases.content("blob", None, 41, 23, 3, seed=4)
    for w in (1.0, 2.5, 4.25):
        r = ramps.outline(w)
        _, d_out, _ = distance_ref.squared_distances(src, 3, 0.5, OUTER, ZERO, r["max_distance"])
        v = _values(distance_ref.distance(src, R=r["max_distance"], scale=r["scale"], offset=r["offset"], flags=STRAIGHT))[..., 3]
        s = np.sqrt(d_out.astype(np.float64))
        assert np.all(v[s <= w - 0.5] == 1) and np.all(v[s >= w + 0.5] == 0) and np.all((v[(s > w - 0.5) & (s < w + 0.5)] > 0) & (v[(s > w - 0.5) & (s < w + 0.5)] < 1))
        r = ramps.inset(w)
        _, _, d_in = distance_ref.squared_distances(src, 3, 0.5, INNER, CLAMP, r["max_distance"])
        v = _values(distance_ref.distance(src, which=INNER, edge=CLAMP, R=r["max_distance"], scale=r["scale"], offset=r["offset"], flags=STRAIGHT))[..., 3]
        s = np.sqrt(d_in.astype(np.float64))
        assert np.all(v[s <= w - 0.5] == 0) and np.all(v[s >= w + 0.5] == 1) and (v == 1).any() == (s >= w + 0.5).any()


def test_four_quadrant_calls_equal_one_call():
    src = distance_cases.content("random", 0.05, 37, 21, 3, seed=5)
    kw = dict(which=SIGNED, R=6, scale=1.0 / 12, offset=0.5, color=(0.2, 0.4, 0.6, 0.8))
    whole = distance_ref.distance(src, **kw)
    parts = None
    for rect in ((0, 0, 17, 9), (17, 0, 20, 9), (0, 9, 17, 12), (17, 9, 20, 12)):
        parts = distance_ref.distance(src, rect=rect, dst_bits=parts, **kw)
    assert np.array_equal(whole, parts)


def test_outer_is_monotone_in_the_seed_set():
    a = distance_cases.content("random", 0.03, 37, 21, 3, seed=6)
    b = a.copy()
    b[..., 3] |= distance_cases.content("random", 0.03, 37, 21, 3, seed=7)[..., 3]  # (ONE | 0: more seeds)
    for R in (2, 9, 255):
        da, db = distance_ref.squared_distances(a, 3, 0.5, OUTER, ZERO, R)[1], distance_ref.squared_distances(b, 3, 0.5, OUTER, ZERO, R)[1]
        assert np.all(db <= da) and (db < da).any()


def test_no_nan_for_any_finite_ramp_over_all_reachable_s():
    """Every s the rule can produce -- sqrtf(D) for D = 0 .. 65536, and +-(that - 0.5) -- under extreme finite ramps: v is in [0, 1]."""
    d = np.arange(0, 65537, dtype=np.int64)
    root = np.sqrt(d.astype(F))
    s = np.concatenate([root, root - F(0.5), F(0.5) - root]).astype(F)
    big, tiny = F(3.4028235e38), F(1e-45)
    for scale in (big, -big, tiny, -tiny, F(0.0), F(-0.0), F(1.0), F(-1.0 / 255)):
        for offset in (big, -big, tiny, -tiny, F(0.0), F(-0.0), F(0.5)):
            v = distance_ref.fmin(distance_ref.fmax(distance_ref.fmaf32(s, scale, offset), F(0.0)), F(1.0))
            assert not np.isnan(v).any() and np.all((v >= 0) & (v <= 1)), (scale, offset)


def test_the_reference_against_a_float64_euclidean_distance():
    """s of the reference is the binary64 Euclidean distance to the nearest seed within the one rounding of the square root (half an
    ulp of binary32), wherever that distance is at most R."""
    src = distance_cases.content("seeds", ((5, 5), (50, 30), (30, 2), (31, 2)), 61, 35, 3, seed=8)
    R = 12
    _, d_out, _ = distance_ref.squared_distances(src, 3, 0.5, OUTER, ZERO, R)
    ys, xs = np.nonzero(distance_ref.seeds(src, 3, 0.5))
    Y, X = np.mgrid[0:35, 0:61]
    exact = np.sqrt(((X[..., None] - xs) ** 2 + (Y[..., None] - ys) ** 2).astype(np.float64)).min(axis=-1)
    s = np.sqrt(d_out.astype(F)).astype(np.float64)
    near = exact <= R
    assert near.any() and (~near).any()
    assert np.all(np.abs(s[near] - exact[near]) <= np.spacing(exact[near].astype(F)).astype(np.float64) / 2)
    assert np.all(d_out[~near] >= R * R) and np.all(d_out[exact >= R + 1] == (R + 1) ** 2)


def test_the_python_ramps_state_their_arithmetic():
    assert ramps.outline(2.5) == dict(which=DistanceWhich.OUTER, max_distance=3, scale=-1.0, offset=3.0)
    assert ramps.outline(0) == dict(which=DistanceWhich.OUTER, max_distance=1, scale=-1.0, offset=0.5)
    assert ramps.outline(2.75)["max_distance"] == 4 and ramps.outline(254.5)["max_distance"] == 255
    assert ramps.inset(1.75) == dict(which=DistanceWhich.INNER, max_distance=3, scale=1.0, offset=-1.25)
    assert ramps.glow(5.5) == dict(which=DistanceWhich.OUTER, max_distance=6, scale=-1.0 / 5.5, offset=1.0)
    assert ramps.glow(3, inner=True) == dict(which=DistanceWhich.INNER, max_distance=3, scale=-1.0 / 3, offset=1.0)
    assert ramps.sdf(8) == dict(which=DistanceWhich.SIGNED, max_distance=8, scale=1.0 / 16, offset=0.5)
    for bad in (lambda: ramps.outline(-1), lambda: ramps.outline(255), lambda: ramps.inset(float("nan")), lambda: ramps.glow(0), lambda: ramps.glow(256),
                lambda: ramps.sdf(0), lambda: ramps.sdf(2.5), lambda: ramps.sdf(256)):
        with pytest.raises(ValueError, match="jh_distance: "):
            bad()
    # max_distance is enough: at s of the cap the ramp has reached an end value, so a texel farther away would have it as well
    for r in (ramps.outline(2.5), ramps.inset(1.75), ramps.glow(5.5), ramps.glow(3, True), ramps.sdf(8)):
        s_cap = r["max_distance"] + 1.0 - (0.5 if r["which"] == DistanceWhich.SIGNED else 0.0)
        v_cap = r["scale"] * s_cap + r["offset"]
        assert v_cap <= 0 or v_cap >= 1, r


# ---- sensitivity: the battery tells the rule from its near misses ----

NEAR_MISSES = {
    # variant: (the keywords that build it, a case of the battery that catches it)
    "a cap of R^2": (dict(cap_r2=True), "37x21_seeds_none_outer_zero_R3"),
    "a window of |dx| < R": (dict(open_window=True), "9x9_seeds_centre_outer_clamp_straight_R2"),
    "> in place of >=": (dict(ge=False), "33x17_values_t4_inner_clamp_straight_R3_ch1"),
    "a NaN as a seed": (dict(nan_seed=True), "33x17_values_t2_signed_zero_straight_R3_ch0"),
    "INNER / ZERO without the outside positions": (dict(zero_outside=False), "37x21_full_inner_zero_R3"),
    "the rectangle as the edge": (dict(image_edge=False), "67x41_seeds_outside_outer_zero_R12_r11_7_45_27"),
    "SIGNED without the half": (dict(half=False), "9x7_seeds_equal_signed_zero_R4"),
    "s rounded to f16 before the ramp": (dict(s_f16=True), "47x31_blob_outer_zero_straight_R6"),
    "the chessboard metric": (dict(chessboard=True), "9x9_seeds_centre_outer_clamp_straight_R2"),
}


@pytest.mark.parametrize("what", sorted(NEAR_MISSES))
def test_the_battery_tells_the_rule_from_a_near_miss(what):
    variant, name = NEAR_MISSES[what]
    want, got = distance_cases.expected(name), distance_cases.expected(name, **variant)
    nan = lambda b: (b & 0x7FFF) > 0x7C00  # noqa: E731
    differ = int(np.count_nonzero((want != got) & ~(nan(want) & nan(got))))
    print("%s: %d of %d values differ on %s" % (what, differ, want.size, name))
    assert differ > 0, (what, name)


def test_the_battery_covers_what_it_claims():
    cases = distance_cases.CASES
    assert len(cases) > 400 and all(c["w"] * c["h"] <= 16600 for c in cases)
    for size in ((1, 1), (1, 5), (5, 1), (1, 600), (600, 1), (255, 2), (256, 2), (257, 3), (3, 31), (2, 32), (3, 33), (3, 63), (2, 64), (3, 65), (3, 127), (2, 128), (3, 129), (2, 8300)):
        assert any((c["w"], c["h"]) == size for c in cases), size
    for R in (1, 2, 15, 16, 17, 64, 255):
        assert any(c["R"] == R for c in cases), R
    for pc in (63, 64, 65, 127, 128, 129):
        assert any((c["rect"][2] if c["rect"] else c["w"]) + 2 * c["R"] == pc for c in cases), pc
    for (which, edge, flags) in distance_cases.COMBOS:
        for in_place in (False, True):
            assert any((c["which"], c["edge"], c["flags"], c["in_place"]) == (which, edge, flags, in_place) for c in cases), (which, edge, flags, in_place)
    assert {c["inst"] for c in cases} == {"k_dist_rows<%s, %s>" % (a, b) for a in ("true", "false") for b in ("true", "false")}
    assert {c["channel"] for c in cases} == {0, 1, 2, 3}
    assert {c["kind"] for c in cases} >= {"seeds", "random", "blob", "full", "hole", "values", "never"}
    assert any(c["rect"] is not None and c["rect"][0] % 2 and c["rect"][1] % 2 for c in cases) and any(c["rect"] == (31, 17, 1, 1) for c in cases)
    assert any(c["scale"] == 0.0 for c in cases) and any(c["scale"] < 0 for c in cases) and any(abs(c["scale"]) > 1e38 for c in cases)
    assert any(c["color"][3] < 0 for c in cases) and any(c["color"][0] == float("inf") for c in cases) and any(not any(c["color"]) for c in cases)
    values = distance_cases.content("values", None, 33, 17, 2, seed=1)[..., 2]
    for v in distance_cases.VALUES:
        assert (values == v).any(), hex(v)
