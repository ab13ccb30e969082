"""CPU: the dash rule.

* the host route (jello_amd.dash, C++) equals tests/dash_ref.py byte for byte on the battery of tests/dash_cases.py;
* structure checks that know nothing of dash_ref's code: for the polyline cases the dashes are measured on the output itself
  (where each starts along the source, how long it is) and compared with intervals computed here in plain float arithmetic --
  count, order, no empty piece, joints on source vertices, the merge of a closed subpath exactly where the rule defines it;
* sensitivity: dash_ref with the merge removed, and with the intervals closed at the other end, fails those checks;
* accuracy: the true arc length (scipy quad with breakpoints at the speed's minima) of every emitted piece against its nominal
  length, bound 2^-10 user units, on the seeded curve families;
* every rejected input; Scene.stroke with a pattern against Scene.stroke of dash(path); and end to end through the oracle: a
  dashed, butt-capped horizontal line on whole-pixel edges against the closed-form coverage of its dashes, with the tolerance
  of tests/test_stroke_coverage_spec.py (tests/test_gpu_coverage.check).  (tests/exact_stroke.py strokes polylines only, so
  there is no dashed curve against it; dashed curves go through parity.compare in tests/test_gpu_dash.py.)"""
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, Join, Path, RenderParams, Scene, Stroke
from jello_amd.scene import dash as host_dash

import coverage_scenes as C
import dash_cases
import dash_ref
from dash_cases import CLOSE, LINE, MOVE

CASES = dash_cases.cases()
IDS = [c[0] for c in CASES]


def as_path(els):
    p = Path()
    p.els = list(els)
    return p


@pytest.mark.parametrize("name,path,pattern,offset", CASES, ids=IDS)
def test_host_route_equals_the_reference_byte_for_byte(built, name, path, pattern, offset):
    got = host_dash(as_path(path), pattern, offset).els
    want = dash_ref.dash(path, pattern, offset)
    assert dash_ref.to_bytes(got) == dash_ref.to_bytes(want)
    for kind, pts in got:  # doubles that are exactly representable in binary32
        assert all(float(np.float32(v)) == v for v in pts)


def test_the_batch_paths_too(built):
    for path, pattern, offset in dash_cases.batch_cases()[:40]:
        assert dash_ref.to_bytes(host_dash(as_path(path), pattern, offset).els) == dash_ref.to_bytes(dash_ref.dash(path, pattern, offset))


# ---- structure, measured on the output ----
def source_subpaths(path):
    """Polyline cases only: [(points, closed)] with the closing vertex appended to a closed subpath."""
    subs, cur = [], None
    for kind, pts in path:
        if kind == MOVE:
            cur = [(pts[0], pts[1])]
            subs.append([cur, False])
        elif kind == LINE:
            cur.append((pts[0], pts[1]))
        elif kind == CLOSE:
            if cur[-1] != cur[0]:
                cur.append(cur[0])
            subs[-1][1] = True
            cur = [cur[0]]
            subs.append([cur, False])
        else:
            raise ValueError("polylines only")
    return [(p, c) for p, c in subs if len(p) > 1]


def expected_intervals(total, pattern, offset):
    """The dashes of a subpath of length `total` in plain floats: half-open "on" intervals clipped to [0, total), empty
    ones dropped, touching ones joined."""
    entries = list(pattern) * (2 if len(pattern) % 2 else 1)
    period = sum(entries)
    pos = -(offset % period)
    out = []
    while pos < total - 1e-9:
        for i in range(0, len(entries), 2):
            a, b = pos, pos + entries[i]
            if b - a > 1e-9 and a < total - 1e-9 and b > 1e-9:
                a, b = max(a, 0.0), min(b, total)
                if out and abs(out[-1][1] - a) < 1e-9:
                    out[-1][1] = b
                else:
                    out.append([a, b])
            pos = pos + entries[i] + entries[i + 1]
    return out


def locate(points, cum, p, at_least):
    """The smallest arc-length position >= at_least (minus slack) at which the polyline passes through p."""
    best = None
    for i in range(len(points) - 1):
        (x0, y0), (x1, y1) = points[i], points[i + 1]
        seg = cum[i + 1] - cum[i]
        if seg == 0:
            continue
        t = ((p[0] - x0) * (x1 - x0) + (p[1] - y0) * (y1 - y0)) / (seg * seg)
        t = min(max(t, 0.0), 1.0)
        if math.hypot(x0 + t * (x1 - x0) - p[0], y0 + t * (y1 - y0) - p[1]) < 1e-4:
            s = cum[i] + t * seg
            if s >= at_least - 1e-4 and (best is None or s < best):
                best = s
    assert best is not None, "a dash starts off the source path at %r" % (p,)
    return best


def check_structure(path, pattern, offset, out):
    """Raises AssertionError unless `out` is the dashing of the polyline `path`: see the module docstring."""
    subs = source_subpaths(path)
    dashes, cur = [], None
    for kind, pts in out:
        if kind == MOVE:
            cur = {"start": (pts[0], pts[1]), "pts": [(pts[0], pts[1])], "closed": False}
            dashes.append(cur)
        elif kind == LINE:
            assert cur is not None and not cur["closed"]
            assert (pts[0], pts[1]) != cur["pts"][-1], "a zero-length piece"
            cur["pts"].append((pts[0], pts[1]))
        elif kind == CLOSE:
            cur["closed"] = True
        else:
            raise AssertionError("a polyline's dashes are lines")
    for d in dashes:
        assert len(d["pts"]) >= 2, "an empty dash"
    k = 0
    for points, closed in subs:
        cum = [0.0]
        for (x0, y0), (x1, y1) in zip(points, points[1:]):
            cum.append(cum[-1] + math.hypot(x1 - x0, y1 - y0))
        total = cum[-1]
        if total < 1e-6:
            continue
        want = expected_intervals(total, pattern, offset)
        whole = closed and len(want) == 1 and want[0][0] < 1e-9 and want[0][1] > total - 1e-9
        merged = closed and not whole and len(want) >= 2 and want[0][0] < 1e-9 and want[-1][1] > total - 1e-9
        if merged:  # the last dash and the first are one, emitted last, starting where the last one starts
            want = want[1:-1] + [[want[-1][0], want[-1][1] + want[0][1]]]
        vertices = {(float(np.float32(x)), float(np.float32(y))) for x, y in points}
        # every segment's length is rounded once to the 2^-20 grid (2^-21 each, they add up along the subpath: the rule's phase
        # drift), pattern and offset likewise, and both ends of a dash are rounded to binary32 (half an ulp per coordinate)
        tol = (len(points) + 4) * 2.0 ** -21 + 4 * 2.0 ** -24 * max(1.0, max(abs(v) for p in points for v in p)) + 1e-9
        at = 0.0
        for a, b in want:
            assert k < len(dashes), "fewer dashes than the pattern has on this subpath"
            d = dashes[k]
            k += 1
            s = locate(points, cum, d["start"], at)
            assert abs(s - a) <= tol, "dash %d starts at %.6f, expected %.6f" % (k - 1, s, a)
            length = sum(math.hypot(q[0] - p[0], q[1] - p[1]) for p, q in zip(d["pts"], d["pts"][1:]))
            assert abs(length - (b - a)) <= tol, "dash %d is %.6f long, expected %.6f" % (k - 1, length, b - a)
            assert all(p in vertices for p in d["pts"][1:-1]), "a joint inside a dash is not a source vertex"
            assert d["closed"] == whole
            at = a
    assert k == len(dashes), "more dashes than the pattern has"


POLYLINE_CASES = [c for c in CASES if c[1] and all(kind in (MOVE, LINE, CLOSE) for kind, _ in c[1]) and c[0] not in
                  ("no_moveto", "draw_after_close", "zero_length_segments", "tiny_segment_vanishes", "pattern_below_grid")]


@pytest.mark.parametrize("name,path,pattern,offset", POLYLINE_CASES, ids=[c[0] for c in POLYLINE_CASES])
def test_structure_of_the_host_route(built, name, path, pattern, offset):
    check_structure(path, pattern, offset, host_dash(as_path(path), pattern, offset).els)


def test_structure_cases_cover_what_they_are_there_for():
    by = {c[0]: c for c in CASES}
    out = lambda n: dash_ref.dash(*by[n][1:])
    assert [k for k, _ in out("line12_boundary_on_end")] == [MOVE, LINE, MOVE, LINE]          # no empty dash at 12
    assert [k for k, _ in out("closed_whole")][-1] == CLOSE and sum(k == MOVE for k, _ in out("closed_whole")) == 1
    assert sum(k == MOVE for k, _ in out("closed_merged")) == 3 and out("closed_merged")[-1][1][:2] == (2.0, 0.0)  # [14,16)+[0,2)
    assert sum(k == MOVE for k, _ in out("closed_start_in_gap")) == sum(k == MOVE for k, _ in dash_ref.dash(*by["closed_start_in_gap"][1:], merge=False))
    assert sum(k == MOVE for k, _ in out("closed_end_in_gap")) == 2 and sum(k == MOVE for k, _ in out("closed_run_starts_on_end")) == 2
    assert out("pattern_nothing") == [] and len(out("pattern_solid")) == 3
    assert out("345_vertices_on_boundaries")[1][1][:2] == (3.0, 0.0) and len(out("345_vertices_on_boundaries")) == 4


@pytest.mark.parametrize("name,variant", [("closed_merged", {"merge": False}), ("closed_merged_clipped_last", {"merge": False}),
                                          ("closed_merged_last_ends_on_end", {"merge": False}),
                                          ("offset_on_boundary", {"closed_left": False})])
def test_a_defective_rule_is_caught(name, variant):
    _, path, pattern, offset = [c for c in CASES if c[0] == name][0]
    check_structure(path, pattern, offset, dash_ref.dash(path, pattern, offset))
    wrong = dash_ref.dash(path, pattern, offset, **variant)
    assert wrong != dash_ref.dash(path, pattern, offset)
    with pytest.raises(AssertionError):
        check_structure(path, pattern, offset, wrong)


# ---- accuracy ----
BOUND = 2.0 ** -10


def true_length(g, ta, tb):
    from scipy.integrate import quad
    from scipy.optimize import minimize_scalar
    if not tb > ta:
        return 0.0
    f = lambda t: dash_ref.speed(g, t)
    ts = np.linspace(ta, tb, 200)
    sp = np.array([f(t) for t in ts])
    points = []
    for i in range(1, len(ts) - 1):  # breakpoints at the minima of the speed: a near-cusp is a kink for the quadrature
        if sp[i] <= sp[i - 1] and sp[i] <= sp[i + 1]:
            points.append(minimize_scalar(f, bounds=(ts[i - 1], ts[i + 1]), method="bounded", options={"xatol": 1e-14}).x)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return quad(f, ta, tb, points=points or None, epsabs=1e-10, epsrel=1e-13, limit=400)[0]


@pytest.mark.parametrize("family", dash_cases.FAMILIES)
def test_arc_length_of_every_piece_is_within_the_bound(family, request):
    size = float(family.split(":")[1]) if family.startswith("cusp") else 4096.0
    worst, panels, n = 0.0, 0, 0
    for kind, pts in dash_cases.family(family, 8, seed=7):
        assert all(0.0 <= v <= 4096.0 for p in pts for v in p)
        trace = []
        dash_ref.dash(dash_cases.curve_path(kind, pts), [size / 37.0, size / 91.0], size / 300.0, trace=trace)
        for g, ta, tb, nominal in trace:
            worst = max(worst, abs(true_length(g, ta, tb) - nominal))
            panels = max(panels, g.panels)
            n += 1
    print("%s: %d pieces, max |true - nominal| = %.3g, K <= %d" % (family, n, worst, panels))
    request.node.user_properties.append(("dash_max_length_error", "%.3g" % worst))
    assert n >= 10
    assert worst <= BOUND


# ---- rejected inputs ----
LINE12 = dash_cases.polyline([(0, 0), (12, 0)])
REJECTED = [
    ("negative entry", LINE12, [4, -1], 0.0), ("nan entry", LINE12, [4, float("nan")], 0.0), ("inf entry", LINE12, [float("inf"), 1], 0.0),
    ("period 0", LINE12, [0, 0], 0.0), ("period quantises to 0", LINE12, [2.0 ** -22, 2.0 ** -23], 0.0),
    ("65 entries", LINE12, [1.0] * 65, 0.0), ("nan offset", LINE12, [4, 2], float("nan")), ("inf offset", LINE12, [4, 2], float("inf")),
    ("nan coordinate", [dash_cases.M(0, 0), dash_cases.L(float("nan"), 1)], [4, 2], 0.0),
    ("inf coordinate", [dash_cases.M(0, 0), dash_cases.C(1, 1, 2, float("inf"), 3, 3)], [4, 2], 0.0),
    ("inf moveto", [dash_cases.M(float("-inf"), 0), dash_cases.L(1, 1)], [4, 2], 0.0),
]


@pytest.mark.parametrize("what,path,pattern,offset", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_inputs(built, what, path, pattern, offset):
    with pytest.raises(dash_ref.Rejected):
        dash_ref.dash(path, pattern, offset)
    with pytest.raises(ValueError):
        host_dash(as_path(path), pattern, offset)
    s = Scene()
    with pytest.raises(ValueError):
        s.stroke(Stroke(2.0, dash_pattern=pattern, dash_offset=offset), None, Brush.solid(C.WHITE), None, as_path(path))
    assert s.stream("path_tags") == b"" and s.stream("draw_tags") == b"" and s.stream("transforms") == b""  # nothing was encoded


def test_an_empty_pattern_is_not_dashing(built):
    with pytest.raises(ValueError):
        host_dash(as_path(LINE12), [], 0.0)
    a, b = Scene(), Scene()
    a.stroke(Stroke(2.0, dash_pattern=(), dash_offset=3.0), None, Brush.solid(C.WHITE), None, as_path(LINE12))
    b.stroke(Stroke(2.0), None, Brush.solid(C.WHITE), None, as_path(LINE12))
    assert all(a.stream(w) == b.stream(w) for w in STREAMS)


# ---- Scene.stroke ----
STREAMS = ("path_tags", "path_data", "draw_tags", "draw_data", "transforms", "styles")
SCENE_CASES = ["sub_300_segments", "70_subpaths", "closed_merged", "closed_whole", "mixed_kinds", "pattern_nothing", "cubic_0", "empty_path"]


@pytest.mark.parametrize("name", SCENE_CASES)
def test_scene_stroke_with_a_pattern_encodes_the_dashed_path(built, name):
    _, path, pattern, offset = [c for c in CASES if c[0] == name][0]
    xf = (1.5, 0.25, -0.5, 2.0, 3.0, 4.0)
    for caps in ((Cap.Butt, Cap.Butt), (Cap.Round, Cap.Square)):
        a, b = Scene(), Scene()
        for s in (a, b):  # something in front, so the de-duplication of transforms and styles has a history
            s.fill(jello_amd.Fill.NonZero, None, Brush.solid(C.WHITE), None, Path.rect(0, 0, 5, 5))
        a.stroke(Stroke(3.0, Join.Miter, 4.0, *caps, dash_pattern=pattern, dash_offset=offset), xf, Brush.solid(C.WHITE), None, as_path(path))
        b.stroke(Stroke(3.0, Join.Miter, 4.0, *caps), xf, Brush.solid(C.WHITE), None, host_dash(as_path(path), pattern, offset))
        for w in STREAMS:
            assert a.stream(w) == b.stream(w), w
        assert a.counts() == b.counts() and a.bump_estimate() == b.bump_estimate()
        assert a.bump_sizes(256, 256).as_dict() == b.bump_sizes(256, 256).as_dict()


# ---- end to end: closed-form coverage of a dashed line ----
def dashed_line_scene(offset):
    s = Scene()
    style = Stroke(4.0, Join.Miter, 4.0, Cap.Butt, Cap.Butt, dash_pattern=[8, 4], dash_offset=offset)
    s.stroke(style, None, Brush.solid(C.WHITE), None, Path().move_to(8, 16).line_to(56, 16))
    return s


def dashed_line_entry(offset):
    """What the scene above must cover, worked out by hand: [8, 4] along x from 8, shifted left by the offset and clipped to
    [8, 56]; every dash a butt-capped line of width 4 -- a rectangle, rows 14 to 18."""
    spans = [(max(8 + 12 * k - offset, 8.0), min(8 + 12 * k - offset + 8, 56.0)) for k in range(0, 6)]
    spans = [(a, b) for a, b in spans if b > a]
    return C.StrokeEntry("dashed-line-offset-%g" % offset, 23, 64, 32, [([(a, 16.0), (b, 16.0)], False) for a, b in spans], 4.0)


def check_dashed_line(alpha, offset):
    from test_gpu_coverage import area_tolerance, check
    entry = dashed_line_entry(offset)
    check(entry, "nonzero", "area", alpha)
    tol = area_tolerance(entry, np.ones_like(alpha))
    want = np.zeros((32, 64))
    for x in range(64):  # the closed form: a column's coverage is its overlap with the dashes, in rows 14..17
        phase = (x - 8 + offset) % 12.0
        inside = 8 <= x < 56
        cover = 0.0
        if inside:
            cover = max(0.0, min(phase + 1.0, 8.0) - phase) if phase < 8.0 else 0.0
            if phase > 11.0:  # the column straddles the start of the next dash
                cover += phase + 1.0 - 12.0
            if x + 1 > 56:
                cover = 0.0
        want[14:18, x] = cover
    if offset == 0.5:
        assert want[15, 8] == 1.0 and want[15, 15] == 0.5 and want[15, 19] == 0.5 and want[15, 16] == 0.0
    assert (np.abs(alpha - want) <= tol).all(), float(np.abs(alpha - want).max())


@pytest.mark.parametrize("offset", [0.0, 0.5])
def test_dashed_line_coverage_through_the_oracle(built, offset):
    from jello_amd import Aa, Host
    from oracle.oracle_engine import OracleEngine
    rec = Host().record(dashed_line_scene(offset), RenderParams(64, 32, aa=Aa.Area))
    o = OracleEngine()
    o.run(rec)
    assert int(o.get(rec, "bumpBuf", np.uint32)[0]) == 0
    check_dashed_line(o.target(rec).view(np.float16).astype(np.float64)[..., 3], offset)
