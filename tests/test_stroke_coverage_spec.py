"""CPU: the oracle's stroker against the float64 stroker of tests/exact_stroke.py, per pixel, on the stroke battery of
tests/coverage_scenes.py (families 11-15) in all three AA modes -- the checks and tolerances of
tests/test_gpu_stroke_coverage.py and tests/test_gpu_coverage.py, run on the oracle.  On top of that:

* the guards of the reference hold for every entry (no miter decision on a knife edge, no arc whose line count an f32
  rounding could change), and the 28.9 / 29 degree pair straddles the flip of limit 4;
* a bracket for arcs that knows no flattening rule: the area alpha lies between the exact alpha of the outline whose
  arcs are dense polylines at radius w / 2 - 0.25 and the one whose arcs are circumscribed at w / 2;
* sensitivity: a reference with one defect each (the miter point on the wrong side, the inner join routed through the
  path point, a square cap extended by w, an arc of n + 1 or n - 1 lines, the width as w (1 + 2^-10), the closing join
  missing) fails the check.

test_stroke_spec.py (image-wide sums) and test_invariants stay as they are."""
import numpy as np
import pytest

from jello_amd import Host
from oracle.oracle_engine import OracleEngine

import coverage_scenes as C
import exact_coverage as X
from test_coverage_spec import oracle_alpha
from test_gpu_coverage import AAS, area_tolerance, check, record
from test_gpu_stroke_coverage import CASES, ROUND, ZERO_LENGTH, check_arc_lines


@pytest.mark.parametrize("eid,aa,variant", CASES, ids=["-".join(c) for c in CASES])
def test_oracle_stroke_coverage(built, request, eid, aa, variant):
    entry = C.BY_ID[eid]
    record(request, entry, aa, check(entry, "nonzero", aa, oracle_alpha(entry, "nonzero", aa, variant)))


def test_reference_guards_hold_and_the_miter_pair_straddles_the_flip():
    for e in C.STROKE_BATTERY:
        e.outline()         # asserts MITER_GUARD and ARC_GUARD / ARC_MAX_LINES
    for suffix in ("", "-mirror"):
        below, above = (C.BY_ID["f13-angle-%s%s" % (a, suffix)].outline().miters for a in ("28.9", "29"))
        assert [m for _, m in below] == [False] and [m for _, m in above] == [True]
    lines = sorted(a.n for e in C.STROKE_BATTERY for a in e.outline().arcs)
    assert lines[0] == 1 and lines[-1] >= 60


@pytest.mark.parametrize("aa", list(AAS))
def test_zero_length_segment_is_dropped(built, aa):
    a, b = (oracle_alpha(C.BY_ID[eid], "nonzero", aa) for eid in ZERO_LENGTH)
    assert np.array_equal(a, b)
    assert all(np.array_equal(p, q) for p, q in zip(*(C.BY_ID[eid].reference_contours() for eid in ZERO_LENGTH)))


def _similarity(e):
    if e.transform is None:
        return True
    a, b, c, d, _, _ = e.transform
    return abs(np.hypot(a, b) - np.hypot(c, d)) < 1e-9 and abs(a * c + b * d) < 1e-9


@pytest.mark.parametrize("eid", [eid for eid in ROUND if _similarity(C.BY_ID[eid])])
def test_arcs_lie_between_the_inscribed_and_the_circumscribed_outline(built, eid):
    """Whatever the flattening rule: with its vertices on the circle and a sagitta of at most 0.25, every arc lies
    between the polyline at radius w / 2 - 0.25 and the one circumscribed at w / 2, and the integral of the winding
    number over a pixel grows with the outline (all of a stroke's outline winds one way).  The slack is the bound of
    the sharp check.  0.25 is a distance in device space, so the entries under an anisotropic scale or a skew are left
    to the sharp check (see exact_stroke)."""
    entry = C.BY_ID[eid]
    W, H = entry.width, entry.height
    alpha = oracle_alpha(entry, "nonzero", "area")
    lower = X.area_alpha(X.area_acc(entry.outline("lower").contours, W, H), "nonzero")
    upper = X.area_alpha(X.area_acc(entry.outline("upper").contours, W, H), "nonzero")
    assert (lower <= upper + 1e-12).all()
    tol = area_tolerance(entry, alpha)
    assert (alpha >= lower - tol).all() and (alpha <= upper + tol).all(), \
        (float((lower - tol - alpha).max()), float((alpha - upper - tol).max()))


@pytest.mark.parametrize("eid", ROUND)
def test_oracle_arc_lines_follow_the_arc_rule(built, eid):
    entry = C.BY_ID[eid]
    rec = Host().record(entry.scene(), entry.params(AAS["area"]))
    o = OracleEngine()
    o.run(rec)
    n = int(o.get(rec, "bumpBuf", np.uint32)[7])
    check_arc_lines(entry, o.get(rec, "linesBuf", np.uint32)[:n * 6].reshape(-1, 6))


@pytest.mark.parametrize("eid,defect", [("f11-stadium", "arc-n+1"), ("f11-stadium", "arc-n-1"), ("f15-zoom-40-w0.8-round", "arc-n-1"),
                                        ("f14-w0.3-round-join", "arc-n+1")])
def test_arc_lines_of_another_count_are_caught(built, eid, defect):
    entry = C.BY_ID[eid]
    rec = Host().record(entry.scene(), entry.params(AAS["area"]))
    o = OracleEngine()
    o.run(rec)
    n = int(o.get(rec, "bumpBuf", np.uint32)[7])
    with pytest.raises(AssertionError):
        check_arc_lines(entry.with_defect(defect), o.get(rec, "linesBuf", np.uint32)[:n * 6].reshape(-1, 6))


def _width(e):
    return e.with_defect(stroke_width=float(np.float32(e.stroke_width)) * (1.0 + 2.0 ** -10))


SENSITIVITY = [
    ("miter-wrong-side", "f13-angle-90", lambda e: e.with_defect("miter-wrong-side")),
    ("miter-wrong-side", "f13-angle-30-mirror", lambda e: e.with_defect("miter-wrong-side")),
    ("inner-through-point", "f14-w40-on-segments-of-10", lambda e: e.with_defect("inner-through-point")),
    ("square-cap-w", "f11-L-miter-butt-square", lambda e: e.with_defect("square-cap-w")),
    ("arc-n+1", "f11-L-round-round-butt", lambda e: e.with_defect("arc-n+1")),
    ("arc-n-1", "f11-L-round-round-butt", lambda e: e.with_defect("arc-n-1")),
    ("arc-n+1", "f15-zoom-40-w0.8-round", lambda e: e.with_defect("arc-n+1")),
    ("arc-n-1", "f15-zoom-40-w0.8-round", lambda e: e.with_defect("arc-n-1")),
    ("width-2^-10", "f11-L-miter-butt-square", _width),
    ("width-2^-10", "f15-rotate-30-round", _width),
    ("no-closing-join", "f12-triangle-miter", lambda e: e.with_defect("no-closing-join")),
]


@pytest.mark.parametrize("defect,eid,make", SENSITIVITY, ids=["%s-%s" % s[:2] for s in SENSITIVITY])
def test_a_defective_reference_is_caught(built, defect, eid, make):
    """The oracle's image passes against the correct outline and fails against one that is wrong in one respect."""
    entry = C.BY_ID[eid]
    alpha = oracle_alpha(entry, "nonzero", "area")
    check(entry, "nonzero", "area", alpha)
    wrong = make(entry)
    assert any(len(a) != len(b) or not np.array_equal(a, b) for a, b in zip(entry.reference_contours(), wrong.reference_contours()))
    with pytest.raises(AssertionError, match="out of bound"):
        check(wrong, "nonzero", "area", alpha)
