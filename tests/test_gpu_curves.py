"""-m gpu: the lines the HIP flattener writes for curves against the exact curve of tests/exact_curve.py, on the curve
battery of tests/coverage_scenes.py (families 16-22: CURVE_BATTERY).  tests/test_curve_spec.py runs the same check
functions on the oracle's line buffer, proves that the battery reaches the routes it names, and keeps the checks
honest with perturbed outlines.

Structure, per subpath (check_fill / check_stroke):
* no NaN or Inf; every line of a segment's polyline starts on the very bits the previous one ends on;
* a fill's polyline starts on the f32-transformed first control point of its segment and ends on the last one, bit for
  bit (the transform is two f32 products and two f32 sums per coordinate, in that order: shared/transform.wgsl); the
  closing line the encoder adds is there; nothing is left over;
* order: the vertices can be assigned, in their order, to positions on the true curve that never go back, each within
  D of its vertex (exact_curve.monotone_match).  This is "the nearest-point parameter never decreases by more than the
  length of D" in a form that still holds where the curve crosses or doubles back on itself: there the nearest point
  of a vertex may lie on the other branch, but a position within D on its own branch exists.  Two swapped pieces, or
  lines emitted in reverse, have no such assignment;
* a stroked segment is its + side (lines run forward, chained end to start), its - side (written in walking order,
  each line reversed: line k + 1 ends on the bits line k starts on), then its join or end cap; the start cap comes
  last (the encoder's cap marker segment).  Both sides start and end within f32_term of c +- (w / 2) n at t = 0 and 1,
  are held to the same order rule (against the centre curve, within w / 2 + D), a butt cap joins the two ends bit for
  bit, a bevel join starts / ends on them, and a join whose two tangents are equal (cr = 0) adds only lines shorter than
  f32_term, whatever its style.

Distance, fills (two-sided): nine points per line lie within D of the curve, and every point of the dense curve
(sagitta <= 1e-4 px) lies within D of the polyline (exact_curve.segment_cover: exact for polylines, no sampling).
D = 2 * 0.25 px (flatten.wgsl: cubic -> Euler spiral within tol = 0.25, spiral -> chords within tol again; the bound
tests/test_invariants.py already uses) + f32_term(entry) of tests/test_gpu_coverage.py.  Two entries say `unbounded`:
one has a piece clamped to 100 lines (3.4 px off), one is a collinear cubic that runs past its end points, for which
flatten.wgsl's error measure is zero (88 px).  The shader promises no distance there; their distances are recorded,
only their structure is held.

Distance, strokes: every point of the outline (nine per line, caps and joins included) lies within w / 2 + D of the
curve; every boundary point of the two parallel curves lies within D of the outline.  A point c(t) +- (w / 2) n(t) is a
boundary point when its distance to the whole curve is at least w / 2 - 1e-3.  Left out are those where the parallel
curve's OWN radius of curvature is below w / 2: that radius is rho(t) + w / 2 on the outer side of a bend (never left
out) and rho(t) - w / 2 on the inner side, so these are the inner-side points with rho(t) < w -- a subset of "rho(t) <
w", which on both sides together leaves out 19 % of plain-w120 and 24 % of ess-w120.  Why that radius: the shader's
error measure is the centre curve's.  A direction error dtheta of a spiral piece, which that measure does not see,
moves the offset point by (w / 2) dtheta ALONG the parallel curve, which takes it (w / 2 dtheta)^2 / (2 r) off a curve
of radius r: nothing where r is large, as much as the move itself where r falls below w / 2.  At most MAX_EXCLUDED
of an entry's boundary points (taken at equal steps of arc length) may be left out; the lines of a miter join that
has its point are outside w / 2 by definition and are not held to the first check.  Under a transform the stroke is
w / 2 wide in local space: the first check is made there (the excess over w / 2, times the smallest singular value, is
a lower bound of the device distance); the second in device space.

Every entry also goes through parity.compare (area AA; the entries of PARITY_MSAA in both MSAA modes): that is what
runs the product's sequential-walk and overflow fall-backs, and flatten_fast.h's decisions, against the oracle.
"""
import math

import numpy as np
import pytest

import coverage_scenes as C
import exact_curve as X
import exact_stroke
from test_gpu_coverage import AAS, f32_term

TOL = 0.25                  # flatten.wgsl: the tolerance of each of the two approximations
MAX_EXCLUDED = 0.10
ZERO_LENGTH = 1e-12         # the encoder drops a segment whose control polygon is at most this wide and high
POINTS_PER_LINE = np.linspace(0.0, 1.0, 9)
FILLS = [e.id for e in C.CURVE_BATTERY if not e.stroke]
STROKES = [e.id for e in C.CURVE_BATTERY if e.stroke]
PARITY_MSAA = ["f18-hairpin-4000", "f18-hairpin-1e5", "f18-hairpin-1e6", "f18-hairpins-64", "f21-stroke-plain-w120"]


def bound(entry):
    return 2 * TOL + f32_term(entry)


def f32_transform(entry, p):
    """transform_apply of shared/transform.wgsl on f32 values: m0 x + m2 y + t0 without contraction."""
    p = np.asarray(p, np.float32).reshape(-1, 2)
    if entry.transform is None:
        return p
    a, b, c, d, e, f = (np.float32(v) for v in entry.transform)
    return np.stack([a * p[:, 0] + c * p[:, 1] + e, b * p[:, 0] + d * p[:, 1] + f], axis=1).astype(np.float32)


def bits(p):
    return np.ascontiguousarray(p, np.float32).view(np.uint32)


def xy(raw):
    """(n, 6) uint32 lines -> (n, 2, 2) float64 points."""
    return raw[:, 2:].copy().view(np.float32).astype(np.float64).reshape(-1, 2, 2)


def fill_segments(entry, k):
    """What path k's line buffer must hold, in order: (subpath, control polygon) per encoded segment, the closing line
    included."""
    out = []
    for i, polys in enumerate(entry.control_points(k)):
        segs = [p for p in polys if np.ptp(p[:, 0]) > ZERO_LENGTH or np.ptp(p[:, 1]) > ZERO_LENGTH]
        if not segs:
            continue
        if not np.array_equal(segs[-1][-1], segs[0][0]):
            segs.append(np.array([segs[-1][-1], segs[0][0]]))
        out += [(i, p) for p in segs]
    return out


def _points_on(pts):
    w = POINTS_PER_LINE[None, :, None]
    return (pts[:, None, 0] * (1.0 - w) + pts[:, None, 1] * w).reshape(-1, 2)


def check_fill(entry, lines):
    """Returns (largest distance between polyline and curve seen, lines checked)."""
    D = bound(entry)
    assert np.isfinite(lines[:, 2:].copy().view(np.float32)).all(), "%s: a line with NaN or Inf" % entry.id
    assert set(np.unique(lines[:, 0])) <= set(range(len(entry.paths))), "%s: lines of an unknown path" % entry.id
    worst = 0.0
    for k in range(len(entry.paths)):
        raw = lines[lines[:, 0] == k]
        pts = xy(raw)
        pos = 0
        for sub, poly in fill_segments(entry, k):
            what = "%s path %d subpath %d segment %s" % (entry.id, k, sub, poly.tolist())
            first, last = bits(f32_transform(entry, poly[0])).ravel(), bits(f32_transform(entry, poly[-1])).ravel()
            assert pos < len(raw) and np.array_equal(raw[pos, 2:4], first), "%s: does not start on its first point" % what
            ends = np.flatnonzero((raw[pos:, 4] == last[0]) & (raw[pos:, 5] == last[1]))
            assert len(ends), "%s: no line ends on its last point" % what
            n = int(ends[0]) + 1
            assert np.array_equal(raw[pos + 1:pos + n, 2:4], raw[pos:pos + n - 1, 4:6]), "%s: lines not connected bit for bit" % what
            seg = pts[pos:pos + n]
            pos += n
            curve = X.Curve(poly, entry.transform)
            _, dense = X.dense_polyline(curve)
            verts = np.vstack([seg[:, 0], seg[-1:, 1]])
            bad = X.monotone_match(verts, dense, D)
            assert bad < 0, "%s: vertex %d %s is out of order along the curve (or farther than %.3g from it)" % (what, bad, verts[bad], D)
            fwd = float(X.dist_to_polyline(_points_on(seg), dense).max())
            if entry.unbounded:     # (reported only, at the dense curve's vertices)
                back, far = float(X.dist_to_segments(dense, seg[:, 0], seg[:, 1]).max()), None
            else:
                back, far = X.segment_cover(dense[:-1], dense[1:], seg[:, 0], seg[:, 1], D)
            worst = max(worst, fwd, back)
            if not entry.unbounded:
                assert fwd <= D, "%s: a point of the polyline is %.4g from the curve, bound %.4g" % (what, fwd, D)
                assert far is None, "%s: the curve at %s is farther than %.4g from the polyline" % (what, far, D)
        assert pos == len(raw), "%s path %d: %d line(s) left over" % (entry.id, k, len(raw) - pos)
    return worst, len(lines)


# --- strokes -----------------------------------------------------------------------------------------------------------

def arc_lines(radius, angle):
    """flatten_arc's line count (flatten.wgsl:490-517)."""
    radius = max(TOL, radius)
    theta = max(exact_stroke.MIN_THETA, 2.0 * math.acos(1.0 - TOL / radius))
    return max(1, int(math.ceil(angle / theta)))


class StrokeLayout:
    """Where the sides, joins and caps of a stroked open subpath are in its line buffer."""
    def __init__(self, entry, lines):
        self.entry = entry
        w, self.join, limit, cap0, cap1 = entry.stroke
        self.h = 0.5 * float(np.float32(w))
        self.M = X.linear_part(entry.transform)
        self.sigma = np.linalg.svd(self.M, compute_uv=False)           # largest, smallest
        self.polys = entry.control_points(0)[0]
        self.curves = [X.Curve(p) for p in self.polys]                  # local space
        raw = self.raw = lines[lines[:, 0] == 0]
        assert len(raw) == len(lines)
        self.pts = xy(raw)
        tan = [(c.d1(np.array([0.0]))[0], c.d1(np.array([1.0]))[0]) for c in self.curves]
        assert all(np.hypot(*t).min() > 0 for pair in tan for t in pair)
        self.tan = [tuple(t / np.hypot(*t) for t in pair) for pair in tan]
        m = len(self.curves)

        def cap_lines(style, t):
            n = self.h * np.array([-t[1], t[0]])
            return {"butt": 1, "square": 3}.get(style) or arc_lines(float(np.hypot(*(self.M @ n))), exact_stroke.PI_F32)
        self.n_start_cap, self.n_end_cap = cap_lines(cap0, self.tan[0][0]), cap_lines(cap1, self.tan[-1][1])
        self.sides, self.tails = [], []
        pos = 0
        for i in range(m):
            a = 1
            while pos + a < len(raw) and np.array_equal(raw[pos + a, 2:4], raw[pos + a - 1, 4:6]):
                a += 1
            if i == m - 1:
                b = len(raw) - pos - a - self.n_end_cap - self.n_start_cap
                tail = self.n_end_cap
            else:
                b = 1
                while pos + a + b < len(raw) and np.array_equal(raw[pos + a + b, 4:6], raw[pos + a + b - 1, 2:4]):
                    b += 1
                tail = self.join_lines(i, limit)
            assert b >= 1, "%s segment %d: no room for a - side (%d lines, + side %d)" % (entry.id, i, len(raw) - pos, a)
            self.sides.append((slice(pos, pos + a), slice(pos + a, pos + a + b)))
            self.tails.append(slice(pos + a + b, pos + a + b + tail))
            pos += a + b + tail
        self.start_cap = slice(pos, pos + self.n_start_cap)
        # the lines that stay within w / 2 of the curve by definition: all but those of a miter join that has its point
        self.within_half_width = np.ones(len(raw), bool)
        for i in range(m - 1):
            if self.join == "miter" and self.tails[i].stop - self.tails[i].start == 3:
                self.within_half_width[self.tails[i]] = False
        assert pos + self.n_start_cap == len(raw), "%s: %d line(s) left over" % (entry.id, len(raw) - pos - self.n_start_cap)

    def join_lines(self, i, limit):
        t0, t1 = self.tan[i][1], self.tan[i + 1][0]
        cr, d = t0[0] * t1[1] - t0[1] * t1[0], t0[0] * t1[0] + t0[1] * t1[1]
        if self.join == "bevel":
            return 2
        if self.join == "miter":
            hyp = math.hypot(cr, d)
            lim = exact_stroke.f16(limit)
            return 3 if (2.0 * hyp < (hyp + d) * lim * lim and abs(cr) > 1e-9) else 2
        n = self.h * np.array([-t0[1], t0[0]])
        return arc_lines(float(np.hypot(*(self.M @ n))), abs(math.atan2(cr, d))) + 1

    def smooth(self, i):
        t0, t1 = self.tan[i][1], self.tan[i + 1][0]
        return abs(t0[0] * t1[1] - t0[1] * t1[0]) < 1e-12 and t0 @ t1 > 0

    def device(self, p):
        return X.apply(self.entry.transform, p)

    def offset_point(self, i, end, sign):
        """c +- (w / 2) n at t = 0 or 1 of segment i, device space."""
        t = self.tan[i][end]
        return self.device(self.polys[i][-1 if end else 0] + sign * self.h * np.array([-t[1], t[0]]))

    def plus_vertices(self, i):
        s = self.pts[self.sides[i][0]]
        return np.vstack([s[:, 0], s[-1:, 1]])

    def minus_vertices(self, i):
        """In walking order (t from 0 to 1)."""
        s = self.pts[self.sides[i][1]]
        return np.vstack([s[:1, 1], s[:, 0]])


def check_stroke(entry, lines, end_points=True):
    """Returns (largest distance of a boundary point from the outline, share of the boundary points left out, largest
    excess of an outline point over w / 2 in device px).  end_points=False leaves out the checks that hold the sides'
    end points and the start cap to f32_term (the sensitivity tests: what do the distance checks catch on their own)."""
    D, tol = bound(entry), f32_term(entry)
    assert np.isfinite(lines[:, 2:].copy().view(np.float32)).all(), "%s: a line with NaN or Inf" % entry.id
    L = StrokeLayout(entry, lines)
    raw, h = L.raw, L.h
    smax, smin = L.sigma
    dense_local = [X.dense_polyline(c, X.SAGITTA / smax, 1.0 / smax) for c in L.curves]
    centre_local = np.vstack([p for _, p in dense_local])
    centre = L.device(centre_local)
    for i in range(len(L.curves)):
        what = "%s segment %d" % (entry.id, i)
        plus, minus = L.sides[i]
        assert np.array_equal(raw[plus][1:, 2:4], raw[plus][:-1, 4:6]), "%s: + side not connected bit for bit" % what
        assert np.array_equal(raw[minus][1:, 4:6], raw[minus][:-1, 2:4]), "%s: - side not connected bit for bit (reversed lines)" % what
        seg_dense = L.device(dense_local[i][1])
        for sign, verts in ((1.0, L.plus_vertices(i)), (-1.0, L.minus_vertices(i))):
            for end in (0, 1):
                want = L.offset_point(i, end, sign)
                got = verts[-1 if end else 0]
                assert not end_points or np.abs(got - want).max() <= tol, "%s: the %s side %s at %s, not at %s" % (
                    what, "+-"[sign < 0], ("starts", "ends")[end], got, want)
            bad = X.monotone_match(verts, seg_dense, h * smax + D)
            assert bad < 0, "%s: vertex %d of the %s side is out of order along the curve (or farther than w / 2 + D from it)" % (what, bad, "+-"[sign < 0])
        tail = raw[L.tails[i]]
        tpts = L.pts[L.tails[i]]
        if i == len(L.curves) - 1:
            if entry.stroke[4] == "butt":
                assert np.array_equal(tail[0, 2:4], raw[plus][-1, 4:6]) and np.array_equal(tail[0, 4:6], raw[minus][-1, 2:4]), \
                    "%s: the end cap does not join the two sides bit for bit" % what
            else:
                assert np.array_equal(tail[0, 2:4], raw[plus][-1, 4:6]) and np.array_equal(tail[-1, 4:6], raw[minus][-1, 2:4]), \
                    "%s: the end cap does not start / end on the two sides" % what
        elif L.smooth(i):
            assert np.abs(tpts[:, 1] - tpts[:, 0]).max() <= tol, "%s: a join with cr = 0 adds a visible line" % what
        elif L.join == "bevel":
            assert np.array_equal(tail[0, 2:4], raw[plus][-1, 4:6]) and np.array_equal(tail[1, 4:6], raw[minus][-1, 2:4])
            assert np.abs(tpts[0, 1] - L.offset_point(i + 1, 0, 1.0)).max() <= tol
            assert np.abs(tpts[1, 0] - L.offset_point(i + 1, 0, -1.0)).max() <= tol
    cap = L.pts[L.start_cap]
    assert not end_points or np.abs(cap[0, 0] - L.offset_point(0, 0, -1.0)).max() <= tol and np.abs(cap[-1, 1] - L.offset_point(0, 0, 1.0)).max() <= tol, \
        "%s: the start cap does not run from the - side's start to the + side's" % entry.id
    # every outline point within w / 2 + D of the curve (local space, see the module docstring)
    P = _points_on(L.pts[L.within_half_width])
    if entry.transform is not None:
        P = (P - X.f32(entry.transform)[4:6]) @ np.linalg.inv(L.M).T
    excess = float((X.dist_to_polyline(P, centre_local).max() - h) * smin)
    assert excess <= D, "%s: an outline point is %.4g farther than w / 2 from the curve, bound %.4g" % (entry.id, excess, D)
    # every boundary point of the parallel curves within D of the outline
    worst, n_boundary, n_out = 0.0, 0, 0
    for c, (t, p) in zip(L.curves, dense_local):
        dev = L.device(p)
        s = np.concatenate([[0.0], np.cumsum(np.hypot(*(dev[1:] - dev[:-1]).T))])
        tu = np.interp(np.arange(0.0, s[-1], 0.5), s, t)               # equal steps of 0.5 device px
        off = X.Offsets(c, 2.0 * h, tu, centre_local)
        for side, on, keep in ((off.plus, off.on_boundary_plus, off.rho_plus >= h), (off.minus, off.on_boundary_minus, off.rho_minus >= h)):
            n_boundary += int(on.sum())
            n_out += int((on & ~keep).sum())
            q = L.device(side[on & keep])
            if len(q):
                d = X.dist_to_segments(q, L.pts[:, 0], L.pts[:, 1])
                j = int(np.argmax(d))
                worst = max(worst, float(d[j]))
                assert d[j] <= D, "%s: the boundary point %s is %.4g from the outline, bound %.4g" % (entry.id, q[j], d[j], D)
    share = n_out / max(1, n_boundary)
    assert share <= MAX_EXCLUDED, "%s: %.3g of the boundary points have rho < w" % (entry.id, share)
    return worst, share, excess


def record(request, entry, **values):
    request.node.user_properties.append(("curve_class", entry.tclass))
    request.node.user_properties.append(("curve_bound", "%.4g" % bound(entry)))
    for k, v in values.items():
        request.node.user_properties.append(("curve_" + k, "%.4g" % v))
    request.node.add_report_section("call", "curve", "%s (%s): D = %.4g; %s" % (
        entry.id, entry.tclass, bound(entry), ", ".join("%s %.4g" % kv for kv in values.items())))


def record_fill(request, entry, result):
    worst, n = result
    record(request, entry, max_distance=worst, max_share_of_bound=worst / bound(entry), lines=n)


def record_stroke(request, entry, result):
    worst, share, excess = result
    record(request, entry, boundary_max_distance=worst, boundary_max_share_of_bound=worst / bound(entry), excluded_share=share,
           outline_max_excess=excess)


@pytest.mark.gpu
@pytest.mark.parametrize("eid", FILLS)
def test_fill_lines_follow_the_curve(engine, request, eid):
    from test_gpu_stroke_coverage import gpu_lines
    entry = C.BY_ID[eid]
    record_fill(request, entry, check_fill(entry, gpu_lines(engine, entry)))


@pytest.mark.gpu
@pytest.mark.parametrize("eid", STROKES)
def test_stroke_lines_follow_the_parallel_curves(engine, request, eid):
    from test_gpu_stroke_coverage import gpu_lines
    entry = C.BY_ID[eid]
    record_stroke(request, entry, check_stroke(entry, gpu_lines(engine, entry)))


@pytest.mark.gpu
@pytest.mark.parametrize("eid", FILLS + STROKES)
def test_curve_parity(engine, eid):
    """Every buffer (the line buffer included) and the image bit for bit against the oracle, area AA."""
    from parity import compare
    entry = C.BY_ID[eid]
    compare(engine, entry.scene(), entry.params(AAS["area"]))


@pytest.mark.gpu
@pytest.mark.parametrize("eid", PARITY_MSAA)
@pytest.mark.parametrize("aa", ["msaa8", "msaa16"])
def test_curve_parity_msaa(engine, eid, aa):
    from parity import compare
    entry = C.BY_ID[eid]
    compare(engine, entry.scene(), entry.params(AAS[aa]))
