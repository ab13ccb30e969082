"""CPU: the oracle's flattener against the exact curves of tests/exact_curve.py, on the curve battery of
tests/coverage_scenes.py (families 16-22) -- the check functions and bounds of tests/test_gpu_curves.py, run on the
oracle's line buffer.  On top of that:

* the reference itself: the dense polyline's sagitta is what it claims (measured between its vertices, hairpins
  included), its distance routines agree with brute force, a quad is evaluated as a quad;
* the battery reaches the routes its entries name (oracle_flatten_depth / _stats / _routes): depth 9, >= 10, >= 13 (and
  16 with pieces accepted at SUBDIV_LIMIT, on an entry outside the battery), more than 640 pieces from 64 cubics, a piece of exactly 100 lines, each of
  the three `robust` branches of the line distribution, the DERIV_THRESH fix-up.  A battery that has drifted off its
  routes fails here, without a GPU;
* sensitivity: the checks fail on outlines perturbed in one respect (a run of lines bridged by one line, every second
  vertex dropped, two runs of vertices swapped, a stroke rendered 2 % wider, a fill that ends one line early).

test_invariants.py's curve test stays as it is."""
import ctypes

import numpy as np
import pytest

from jello_amd import Host
from oracle import oracle_engine
from oracle.oracle_engine import OracleEngine

import coverage_scenes as C
import exact_curve as X
import test_gpu_curves as T
from test_gpu_coverage import AAS

ROUTES = ("robust_normal", "robust_low_k1", "robust_low_dist", "pieces_of_100_lines", "accepted_at_subdiv_limit",
          "deriv_fixups", "chords_below_deriv_thresh", "most_lines_in_a_piece")
_cache = {}


def oracle_lines(entry):
    """(line buffer, statistics of the flatten stage) of one entry on the oracle; computed once."""
    if entry.id not in _cache:
        lib = oracle_engine.lib()
        lib.oracle_flatten_routes.argtypes = lib.oracle_flatten_depth.argtypes = lib.oracle_flatten_stats.argtypes = \
            [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
        depth, stats, routes = (ctypes.c_uint64 * 20)(), (ctypes.c_uint64 * 32)(), (ctypes.c_uint64 * 8)()

        def read_and_reset():
            lib.oracle_flatten_depth(depth, 1), lib.oracle_flatten_stats(stats, 1), lib.oracle_flatten_routes(routes, 1)
        rec = Host().record(entry.scene(), entry.params(AAS["area"]))
        o = OracleEngine()
        read_and_reset()
        o.run(rec, stop_after="flatten")
        read_and_reset()
        n = int(o.get(rec, "bumpBuf", np.uint32)[7])
        lines = o.get(rec, "linesBuf", np.uint32)[:n * 6].reshape(-1, 6).copy()
        st = dict(zip(ROUTES, routes))
        st.update(depth=max(i for i, v in enumerate(depth) if v), jobs=stats[0], lines=stats[2], pieces=stats[3])
        _cache[entry.id] = (lines, st)
    return _cache[entry.id]


@pytest.mark.parametrize("eid", T.FILLS)
def test_oracle_fill_lines_follow_the_curve(built, request, eid):
    entry = C.BY_ID[eid]
    T.record_fill(request, entry, T.check_fill(entry, oracle_lines(entry)[0]))


@pytest.mark.parametrize("eid", T.STROKES)
def test_oracle_stroke_lines_follow_the_parallel_curves(built, request, eid):
    entry = C.BY_ID[eid]
    T.record_stroke(request, entry, T.check_stroke(entry, oracle_lines(entry)[0]))


def test_the_battery_reaches_its_routes(built):
    st = {e.id: oracle_lines(e)[1] for e in C.CURVE_BATTERY}
    assert st["f16-plain"]["depth"] == 3 and st["f16-cusp"]["depth"] == 7
    assert st["f18-hairpin-4000"]["depth"] == 9             # FLQ_MAX_LEVEL: the last level of the cooperative route
    assert st["f18-hairpin-1e5"]["depth"] >= 10             # beyond it: the sequential walk
    assert st["f18-hairpin-1e6"]["depth"] >= 13
    assert all(s["accepted_at_subdiv_limit"] == 0 for eid, s in st.items() if not C.BY_ID[eid].unbounded)
    many = st["f18-hairpins-64"]                            # jobs: 64 cubics and their 64 closing lines
    assert many["jobs"] == 128 and many["pieces"] - 64 > 640 and many["depth"] == 9
    assert st["f18-clamped-arc"]["pieces_of_100_lines"] >= 1
    assert all(s["pieces_of_100_lines"] == 0 for eid, s in st.items() if not C.BY_ID[eid].unbounded)
    assert st["f18-large-arc"]["most_lines_in_a_piece"] >= 20
    for branch in ROUTES[:3]:
        assert any(s[branch] for s in st.values()), branch
    assert any(s["robust_normal"] for eid, s in st.items() if eid.startswith("f21")), "the offset route runs the general branch"
    assert st["f16-cusp"]["deriv_fixups"] >= 1 and st["f17-p2=p3"]["deriv_fixups"] >= 1


def test_subdiv_limit_is_reached_only_outside_the_pipelines_domain(built):
    """The forced acceptance at SUBDIV_LIMIT (flatten stage of the oracle alone): the +-1e8 hairpin reaches depth 16 and
    has pieces accepted with their error above tol; its lines still hold the structure rules.  It is not in the battery:
    one of its lines crosses more than 65535 tiles, which path_count's 16-bit index within a line cannot count."""
    entry = C.SUBDIV_LIMIT_ENTRY
    lines, st = oracle_lines(entry)
    assert st["depth"] == 16 and st["accepted_at_subdiv_limit"] >= 1
    T.check_fill(entry, lines)
    p = T.xy(lines)
    assert (np.abs(p[:, 1] - p[:, 0]).sum(axis=1) / 16).max() > 65535
    for e in C.CURVE_BATTERY:
        q = T.xy(oracle_lines(e)[0])
        assert (np.abs(q[:, 1] - q[:, 0]).sum(axis=1) / 16 + 2).max() < 65535, e.id


# --- the reference ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eid", ["f16-plain", "f16-cusp", "f18-hairpin-4000", "f18-hairpin-1e6", "f18-large-arc", "f19-quad-hairpin"])
def test_dense_polyline_sagitta(eid):
    """Between two vertices the curve stays within SAGITTA of the chord: measured at 15 parameters per interval."""
    curve = X.Curve(C.BY_ID[eid].control_points(0)[0][0])
    t, pts = X.dense_polyline(curve)
    assert t[0] == 0.0 and t[-1] == 1.0 and (np.diff(t) > 0).all() and len(t) < 50000
    a, d = pts[:-1], pts[1:] - pts[:-1]
    dd = (d * d).sum(axis=1)
    for w in np.linspace(0.0, 1.0, 17)[1:-1]:
        p = curve.at(t[:-1] + w * np.diff(t))
        s = np.clip(((p - a) * d).sum(axis=1) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
        assert np.hypot(*(a + s[:, None] * d - p).T).max() <= X.SAGITTA * (1 + 1e-9)


def test_a_quad_is_its_own_curve():
    p = np.array([(40.0, 60.0), (300.0, 480.0), (470.0, 90.0)])
    raised = np.array([p[0], p[0] + 2 / 3 * (p[1] - p[0]), p[2] + 2 / 3 * (p[1] - p[2]), p[2]])     # exact in float64
    t = np.linspace(0, 1, 33)
    q, c = X.Curve(p), X.Curve(raised.astype(np.float32))
    assert np.abs(q.at(t) - X.Curve.at(q, t)).max() == 0 and q.degree == 2
    assert 0 < np.abs(q.at(t) - c.at(t)).max() < 1e-4          # the f32 elevation is not the quad, and is close to it
    assert np.allclose(q.d1(t), (q.at(t + 1e-6) - q.at(t - 1e-6)) / 2e-6, atol=1e-3)
    assert np.allclose(q.d2(t), 2 * (p[2] - 2 * p[1] + p[0]))


def test_distance_routines_agree_with_brute_force():
    rng = np.random.default_rng(5)
    _, poly = X.dense_polyline(X.Curve(C.PLAIN), 1e-3)
    assert len(poly) > 4 * X.GROUP                              # the grouped path
    P = rng.uniform(0, 512, (300, 2))
    brute = X._point_segment(P, poly[:-1], poly[1:])[0].min(axis=1)
    assert np.allclose(X.dist_to_polyline(P, poly), brute, rtol=0, atol=1e-12)
    small = poly[::40]
    assert np.allclose(X.dist_to_polyline(P, small), X._point_segment(P, small[:-1], small[1:])[0].min(axis=1), rtol=0, atol=1e-12)
    # segment_cover: the polyline against itself moved by 0.3 in x (no point is farther than 0.3, the steep ones nearly so)
    moved = poly + np.array([0.3, 0.0])
    assert X.segment_cover(poly[:-1], poly[1:], moved[:-1], moved[1:], 0.1)[1] is not None
    worst, far = X.segment_cover(poly[:-1], poly[1:], moved[:-1], moved[1:], 0.3 + 1e-9)
    assert far is None and 0.2 < worst <= 0.3 + 1e-9
    assert abs(worst - X.dist_to_polyline(poly, moved).max()) < 1e-9
    assert X.monotone_match(poly[::7], poly, 1e-9) == -1 and X.monotone_match(poly[::-7], poly, 1.0) == 1


# --- sensitivity ------------------------------------------------------------------------------------------------------

def _lines_from_vertices(template, verts_bits):
    """Lines of path 0 through the given vertices (uint32 pairs), each starting on the bits the previous one ends on."""
    out = np.zeros((len(verts_bits) - 1, 6), np.uint32)
    out[:, 0], out[:, 1] = template[0, 0], template[0, 1]
    out[:, 2:4], out[:, 4:6] = verts_bits[:-1], verts_bits[1:]
    return out


def _plain_polyline(built):
    """(entry, its oracle lines, vertices of the cubic's polyline as bits, the closing line)."""
    entry = C.BY_ID["f16-plain"]
    lines = oracle_lines(entry)[0]
    T.check_fill(entry, lines)
    curve, closing = lines[:-1], lines[-1:]
    return entry, np.vstack([curve[:, 2:4], curve[-1:, 4:6]]), closing


def test_a_bridged_run_of_lines_is_caught(built):
    """Lines 10 ... 13 replaced by one line: every point of the polyline is still near the curve; the curve is not near it."""
    entry, v, closing = _plain_polyline(built)
    wrong = np.vstack([_lines_from_vertices(closing, np.vstack([v[:10], v[14:]])), closing])
    with pytest.raises(AssertionError, match="from the curve, bound|the curve at .* is farther than"):
        T.check_fill(entry, wrong)


def test_a_missing_stretch_is_seen_from_the_curve_alone(built):
    """f17-collinear-overshoot is one line from p0 to p3 on the curve's own line: every point of it is ON the curve, and
    only the second direction of the distance check sees the 88 px the curve runs past an end (the entry says why the
    shader gives no bound there; held to D it fails, and for this reason)."""
    import copy
    entry = copy.copy(C.BY_ID["f17-collinear-overshoot"])
    lines = oracle_lines(entry)[0]
    assert len(lines) == 2
    worst, _ = T.check_fill(entry, lines)
    assert worst > 50
    entry.unbounded = None
    with pytest.raises(AssertionError, match="the curve at .* is farther than"):
        T.check_fill(entry, lines)


def test_every_second_vertex_dropped_is_caught(built):
    entry, v, closing = _plain_polyline(built)
    wrong = np.vstack([_lines_from_vertices(closing, np.vstack([v[:-1:2], v[-1:]])), closing])
    with pytest.raises(AssertionError, match="from the curve, bound|farther than"):
        T.check_fill(entry, wrong)


def test_two_swapped_runs_are_caught(built):
    """Vertices 8 ... 11 and 12 ... 15 change places: connected bit for bit, out of order along the curve."""
    entry, v, closing = _plain_polyline(built)
    order = np.vstack([v[:8], v[12:16], v[8:12], v[16:]])
    pts = order.copy().view(np.float32).astype(np.float64)
    assert X.monotone_match(pts, X.dense_polyline(X.Curve(C.PLAIN))[1], T.bound(entry)) == 12
    with pytest.raises(AssertionError, match="out of order along the curve"):
        T.check_fill(entry, np.vstack([_lines_from_vertices(closing, order), closing]))


def test_a_fill_that_ends_one_line_early_is_caught(built):
    entry, v, closing = _plain_polyline(built)
    early = closing.copy()
    early[0, 2:4] = v[-2]           # the closing line starts where the shortened polyline ends
    with pytest.raises(AssertionError, match="no line ends on its last point"):
        T.check_fill(entry, np.vstack([_lines_from_vertices(closing, v[:-1]), early]))


@pytest.mark.parametrize("eid", ["f21-stroke-plain-w120", "f21-stroke-loop-w120", "f21-stroke-plain-w20"])
def test_a_stroke_two_percent_wider_is_caught(built, eid):
    """The outline of the same curve stroked with w * 1.02, held to w.  The end points give it away first (they are
    held to f32_term); with that check out of the way the boundary points do, where 1 % of w exceeds D."""
    entry = C.BY_ID[eid]
    T.check_stroke(entry, oracle_lines(entry)[0])
    w = entry.stroke[0]
    wider = C.CurveEntry(entry.name + "-wider", 99, entry.width, entry.height, entry.paths, "sensitivity",
                         stroke=(w * 1.02,) + tuple(entry.stroke[1:]))
    lines = oracle_lines(wider)[0]
    with pytest.raises(AssertionError, match="side (starts|ends) at"):
        T.check_stroke(entry, lines)
    if 0.01 * w > T.bound(entry):
        with pytest.raises(AssertionError, match="from the outline, bound|farther than w / 2"):
            T.check_stroke(entry, lines, end_points=False)
