"""The morphology rule on the CPU: the reference (tests/morph_ref.py) against the consequences the rule states and
windows worked by hand, the ctypes mirror and the enums against the compiled header, the call without a context, the stand-alone
check of include/jello_morph.h (tools/morph_check.cpp), and that the battery (tests/morph_cases.py) tells the rule from its near
misses."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import MorphEdge, MorphOp, _lib

import morph_cases
import morph_ref
from abi_text import INCLUDE, ROOT, c_values
from morph_ref import CLAMP, DILATE, ERODE, STRAIGHT, ZERO

NEG0, POS0, ONE, MINUS_ONE, HALF, INF, NAN = 0x8000, 0x0000, 0x3C00, 0xBC00, 0x3800, 0x7C00, 0x7E00


def _is_nan(bits):
    return (np.asarray(bits, np.uint16) & 0x7FFF) > 0x7C00


def _keys(bits, op=DILATE):
    """The order keys of f16 bit patterns as stored (a NaN: the operator's extreme)."""
    return morph_ref.key(np.asarray(bits, np.uint16).view(np.float16).astype(np.float32), op)


def _image(rows):
    """(h, w, 4) from rows of one value per texel, the same in all four channels."""
    a = np.array(rows, np.uint16)
    return np.repeat(a[..., None], 4, axis=-1)


# ---- the consequences the rule states ----

@pytest.mark.parametrize("kind", ["finite", "nonfinite", "ties"])
def test_straight_radius_zero_is_a_copy_of_every_value(kind):
    """STRAIGHT with rx = ry = 0: every non-NaN value bit for bit, -0 included (unlike the blur); a NaN as a NaN."""
    src = morph_cases.content(kind, 19, 11, seed=9)
    assert (src == NEG0).any()
    for op in (ERODE, DILATE):
        for edge in (ZERO, CLAMP):
            out = morph_ref.morph(src, op, 0, edge, STRAIGHT)
            assert np.array_equal(out[~_is_nan(src)], src[~_is_nan(src)])
            assert np.array_equal(_is_nan(out), _is_nan(src))


def test_premultiplied_radius_zero_leaves_the_stores_rounding():
    """Without STRAIGHT radius 0 is the store applied to (c a, a): the rounding of c a / a, alpha through + 0.0f."""
    src = morph_cases.content("unit", 23, 9, seed=4)
    want = morph_ref.store(morph_ref.operands(src, False), False)
    for op in (ERODE, DILATE):
        assert morph_ref.same_bits(morph_ref.morph(src, op, 0, CLAMP), want)
    assert not np.array_equal(want, src)  # (it is not a copy: the colour of a texel with alpha 0 becomes 0, a -0 alpha +0)


def test_straight_erode_is_the_flipped_dilate_of_the_flipped_image():
    """CLAMP: exactly.  ZERO: the flipped route pads with -0 seen from the original, so the two differ exactly where the window
    reaches outside the image and no operand inside the image is below +0 -- erode gives +0 there (the padding), the flipped route
    -0 -- and nowhere else."""
    src = morph_cases.content("ties", 21, 13, seed=5)
    src[_is_nan(src.view(np.uint16))] = ONE
    src[src == INF] = HALF
    src[:, :10] &= 0x7FFF  # (the left half holds nothing below +0, so that both kinds of border window occur)
    r = (2, 3)
    flipped = src ^ 0x8000
    for edge in (CLAMP, ZERO):
        erode = morph_ref.morph(src, ERODE, r, edge, STRAIGHT)
        route = morph_ref.morph(flipped, DILATE, r, edge, STRAIGHT) ^ 0x8000
        if edge == CLAMP:
            assert np.array_equal(erode, route)
            continue
        inside_min = _keys(morph_ref.morph(src, ERODE, r, CLAMP, STRAIGHT), ERODE)
        ys, xs = np.mgrid[0:13, 0:21]
        reaches_out = ((xs < r[0]) | (xs >= 21 - r[0]) | (ys < r[1]) | (ys >= 13 - r[1]))[..., None]
        differ = reaches_out & (inside_min >= 0)
        assert differ.any() and (reaches_out & ~differ).any()
        assert np.array_equal(erode != route, differ)
        assert np.all(erode[differ] == POS0) and np.all(route[differ] == NEG0)


def test_dilate_source_erode_are_ordered_and_monotone_in_the_radius_under_clamp():
    src = morph_cases.content("finite", 17, 12, seed=6)
    k = _keys(src)
    prev_d = prev_e = k
    for r in (0, 1, 2, 5):
        d, e = _keys(morph_ref.morph(src, DILATE, r, CLAMP, STRAIGHT)), _keys(morph_ref.morph(src, ERODE, r, CLAMP, STRAIGHT))
        assert np.all(d >= k) and np.all(k >= e)
        assert np.all(d >= prev_d) and np.all(e <= prev_e)
        prev_d, prev_e = d, e
    assert not np.array_equal(prev_d, k) and not np.array_equal(prev_e, k)


def test_radius_zero_is_idempotent():
    """On the rule's values (STRAIGHT) radius 0 applied twice is radius 0 applied once: the identity.  (Premultiplied, a second
    application rounds c a / a again, which is the store's property, not the operator's.)"""
    src = morph_cases.content("finite", 17, 12, seed=7)
    for op in (ERODE, DILATE):
        once = morph_ref.morph(src, op, 0, ZERO, STRAIGHT)
        assert np.array_equal(morph_ref.morph(once, op, 0, ZERO, STRAIGHT), once)


def test_opening_never_exceeds_the_source():
    """Erode by r then dilate by r (STRAIGHT, CLAMP) is at most the source, texel by texel; closing is at least it."""
    src = morph_cases.content("finite", 23, 14, seed=8)
    k = _keys(src)
    for r in (1, (2, 1), 3):
        opened = morph_ref.morph(morph_ref.morph(src, ERODE, r, CLAMP, STRAIGHT), DILATE, r, CLAMP, STRAIGHT)
        closed = morph_ref.morph(morph_ref.morph(src, DILATE, r, CLAMP, STRAIGHT), ERODE, r, CLAMP, STRAIGHT)
        assert np.all(_keys(opened) <= k) and np.all(_keys(closed) >= k)
        assert (_keys(opened) < k).any()


# ---- windows worked by hand ----

def test_a_single_texel_grows_into_its_box_and_is_eaten_by_an_erode():
    src = _image([[0] * 7] * 5)
    src[2, 3] = ONE
    out = morph_ref.morph(src, DILATE, (2, 1), ZERO, STRAIGHT)
    want = _image([[0] * 7] * 5)
    want[1:4, 1:6] = ONE
    assert np.array_equal(out, want)
    assert not morph_ref.morph(src, ERODE, (1, 0), ZERO, STRAIGHT).any()


def test_the_edge_modes_at_the_border():
    """A row of ones: ZERO's erode eats the border texels (the padding +0 is the least), CLAMP's leaves them; a row of -1 under
    DILATE: ZERO's padding +0 is the greatest at the border, CLAMP keeps -1."""
    ones = _image([[ONE] * 5])
    assert np.array_equal(morph_ref.morph(ones, ERODE, (1, 0), ZERO, STRAIGHT)[0, :, 0], [POS0, ONE, ONE, ONE, POS0])
    assert np.array_equal(morph_ref.morph(ones, ERODE, (1, 0), CLAMP, STRAIGHT), ones)
    assert not morph_ref.morph(ones, ERODE, (0, 1), ZERO, STRAIGHT).any()  # (one row: every window reaches above and below)
    minus = _image([[MINUS_ONE] * 5])
    assert np.array_equal(morph_ref.morph(minus, DILATE, (1, 0), ZERO, STRAIGHT)[0, :, 0], [POS0, MINUS_ONE, MINUS_ONE, MINUS_ONE, POS0])
    assert np.array_equal(morph_ref.morph(minus, DILATE, (1, 0), CLAMP, STRAIGHT), minus)


def test_the_zeros_are_ordered_and_a_nan_is_sticky():
    row = _image([[NEG0, POS0, NEG0, NEG0, NAN, NEG0, NEG0, NEG0]])
    d = morph_ref.morph(row, DILATE, (1, 0), CLAMP, STRAIGHT)[0, :, 0]
    e = morph_ref.morph(row, ERODE, (1, 0), CLAMP, STRAIGHT)[0, :, 0]
    assert list(d[:3]) == [POS0, POS0, POS0] and list(e[:3]) == [NEG0, NEG0, NEG0]
    assert list(_is_nan(d)) == list(_is_nan(e)) == [False, False, False, True, True, True, False, False]
    assert d[6] == NEG0 and e[7] == NEG0
    neg_nan = _image([[ONE, 0xFE00, ONE]])  # (the sign of a NaN does not matter: it wins under both operators)
    assert _is_nan(morph_ref.morph(neg_nan, DILATE, (1, 0), CLAMP, STRAIGHT)).all() and _is_nan(morph_ref.morph(neg_nan, ERODE, (1, 0), CLAMP, STRAIGHT)).all()


def test_premultiplied_operands_by_hand():
    """(colour 1, alpha 0.5) next to (colour 0.5, alpha 1): both premultiply to 0.5, so the dilated colour is 0.5 over the dilated
    alpha 1 -> 0.5; eroded it is 0.5 over alpha 0.5 -> 1.  An Inf colour over alpha 0 is a NaN once premultiplied and spreads; with
    STRAIGHT it is an Inf and spreads under DILATE only."""
    a, b = [ONE, ONE, ONE, HALF], [HALF, HALF, HALF, ONE]
    src = np.array([[a, b]], np.uint16)
    assert np.array_equal(morph_ref.morph(src, DILATE, (1, 0), CLAMP), np.array([[b, b]], np.uint16))
    assert np.array_equal(morph_ref.morph(src, ERODE, (1, 0), CLAMP), np.array([[a, a]], np.uint16))
    src = np.array([[[INF, ONE, ONE, POS0], [HALF, HALF, HALF, ONE]]], np.uint16)
    out = morph_ref.morph(src, ERODE, (1, 0), CLAMP)
    assert _is_nan(out[0, :, 0]).all() and not _is_nan(out[0, :, 1:]).any()
    assert np.array_equal(morph_ref.morph(src, DILATE, (1, 0), CLAMP, STRAIGHT)[0, :, 0], [INF, INF])
    assert np.array_equal(morph_ref.morph(src, ERODE, (1, 0), CLAMP, STRAIGHT)[0, :, 0], [HALF, HALF])


def test_the_image_is_the_edge_not_the_rectangle():
    src = _image([[ONE, 0, 0, 0, ONE]])
    before = np.full_like(src, morph_cases.POISON)
    out = morph_ref.morph(src, DILATE, (1, 0), ZERO, STRAIGHT, rect=(1, 0, 3, 1), dst_bits=before)
    assert list(out[0, :, 0]) == [morph_cases.POISON, ONE, POS0, ONE, morph_cases.POISON]


def test_a_radius_beyond_the_image_and_the_refusals_of_the_reference():
    src = morph_cases.content("unit", 6, 4, seed=1)
    big, whole = morph_ref.morph(src, DILATE, 255, CLAMP, STRAIGHT), morph_ref.morph(src, DILATE, (6, 4), CLAMP, STRAIGHT)
    assert np.array_equal(big, whole) and all(len(np.unique(big[..., c])) == 1 for c in range(4))
    for kw in (dict(op=2), dict(edge=2), dict(flags=2), dict(radius=256), dict(radius=(0, -1)), dict(rect=(0, 0, 7, 4)), dict(rect=(1, 1, 0, 2))):
        args = dict(op=DILATE, radius=1, edge=ZERO, flags=0, rect=None)
        args.update(kw)
        with pytest.raises(ValueError):
            morph_ref.morph(src, args["op"], args["radius"], args["edge"], args["flags"], args["rect"])


# ---- the C ABI without a device ----

def test_the_headers_constants_and_the_mirrors_layout():
    assert c_values(["JH_MORPH_ERODE", "JH_MORPH_DILATE", "JH_MORPH_EDGE_ZERO", "JH_MORPH_EDGE_CLAMP", "JH_MORPH_STRAIGHT", "JH_MORPH_MAX_RADIUS"]) == [0, 1, 0, 1, 1, 255]
    assert [int(o) for o in MorphOp] == [ERODE, DILATE] and [int(e) for e in MorphEdge] == [ZERO, CLAMP]
    assert (jello_amd.engine.MORPH_STRAIGHT, jello_amd.engine.MORPH_MAX_RADIUS) == (STRAIGHT, morph_ref.MAX_RADIUS)
    fields = ["op", "edge", "flags", "radius_x", "radius_y", "x", "y", "width", "height"]
    assert [name for name, _ in _lib.CMorphDesc._fields_] == fields
    want = c_values(["sizeof(jh_morph_desc)"] + ["offsetof(jh_morph_desc, %s)" % f for f in fields])
    assert [ctypes.sizeof(_lib.CMorphDesc)] + [getattr(_lib.CMorphDesc, f).offset for f in fields] == want


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    d = jello_amd.engine._morph_desc(MorphOp.DILATE, 1, MorphEdge.ZERO, None, True)
    assert hip.jh_morphology(None, 1, 2, ctypes.byref(d)) == -1  # JH_ERR_INVALID
    assert hip.jh_morphology(None, 1, 2, None) == -1


def test_the_descriptor_python_builds():
    d = jello_amd.engine._morph_desc(MorphOp.ERODE, (3, 255), MorphEdge.CLAMP, (1, 2, 3, 4), False)
    assert (d.op, d.edge, d.flags, d.radius_x, d.radius_y, d.x, d.y, d.width, d.height) == (0, 1, 1, 3, 255, 1, 2, 3, 4)
    d = jello_amd.engine._morph_desc(MorphOp.DILATE, 7, MorphEdge.ZERO, None, True)
    assert (d.op, d.edge, d.flags, d.radius_x, d.radius_y, d.x, d.y, d.width, d.height) == (1, 0, 0, 7, 7, 0, 0, 0, 0)
    for radius in (256, -1, (0, 256), (-1, 0)):
        with pytest.raises(ValueError, match="jh_morphology: "):
            jello_amd.engine._morph_desc(MorphOp.DILATE, radius, MorphEdge.ZERO, None, True)


def test_the_stand_alone_check_builds_and_passes(tmp_path):
    """tools/morph_check.cpp is include/jello_morph.h with a main of its own: the descriptors, the key order over every f16 pattern,
    the kernels' decomposition against a brute-force window.  Its header has the command with the sanitizers; here it is built
    without them and run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "morph_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", INCLUDE, os.path.join(ROOT, "tools", "morph_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("ok: 65536 + "), out


# ---- sensitivity: the battery tells the rule from its near misses ----

NEAR_MISSES = {
    # variant: (the keyword that builds it, the case of the battery that catches it)
    "a NaN ignored instead of sticky": (dict(nan_sticky=False), "65x33_erode_r2_7_zero_nonfinite"),
    "-0 and +0 taken for equal": (dict(signed_zero=False), "65x33_erode_r1_1_clamp_straight_r20_10_45_23_inplace_ties"),
    "the window clipped to the rectangle": (dict(window_image=False), "65x33_erode_r7_2_zero_r9_5_40_20_inplace_finite"),
    "ZERO's padding left out": (dict(zero_pad=False), "1x1_erode_r1_1_zero_inplace_finite"),
    "straight operands where premultiplied are asked for": (dict(premultiply=False), "65x33_dilate_r2_7_zero_unit"),
    "a window of [-r, r)": (dict(closed_window=False), "1x37_erode_r1_1_zero_finite"),
}


@pytest.mark.parametrize("what", sorted(NEAR_MISSES))
def test_the_battery_tells_the_rule_from_a_near_miss(what):
    variant, name = NEAR_MISSES[what]
    want, got = morph_cases.expected(name), morph_cases.expected(name, **variant)
    differ = int(np.count_nonzero((want != got) & ~(_is_nan(want) & _is_nan(got))))
    print("%s: %d of %d values differ on %s" % (what, differ, want.size, name))
    assert differ > 0, (what, name)


def test_the_battery_covers_what_it_claims():
    names = set(morph_cases.BY_NAME)
    assert len(names) > 400
    cases = morph_cases.CASES
    assert all(c["w"] <= 260 and c["h"] <= 150 for c in cases)
    for size in morph_cases.SIZES:
        assert any((c["w"], c["h"]) == size for c in cases), size
    for r in (0, 1, 2, 3, 4, 7, 8, 14, 15, 16, 17, 31, 32, 255):
        assert any(c["radius"][0] == r for c in cases) and any(c["radius"][1] == r for c in cases), r
    assert any(c["radius"][0] != c["radius"][1] for c in cases)
    for op in morph_cases.OPS:
        for edge in morph_cases.EDGES:
            for flags in morph_cases.FLAGS:
                for in_place in (False, True):
                    assert any((c["op"], c["edge"], c["flags"], c["in_place"]) == (op, edge, flags, in_place) for c in cases)
    for kind in ("finite", "unit", "nonfinite", "never", "ties"):
        assert any(c["kind"] == kind for c in cases), kind
    assert any(c["rect"] == (31, 17, 1, 1) for c in cases) and any(c["rect"] is not None and c["rect"][0] % 2 and c["rect"][1] % 2 for c in cases)
    assert any(c["h"] == 140 and c["radius"][1] == 20 for c in cases)  # five blocks of 41 rows
    ties = morph_cases.content("ties", 65, 33, seed=1)
    assert (ties == NEG0).any() and (ties == POS0).any() and (ties[..., 3] == MINUS_ONE).any()
    assert ((ties[..., 0] == INF) & ((ties[..., 3] & 0x7FFF) == 0)).any()  # an Inf colour over alpha 0
