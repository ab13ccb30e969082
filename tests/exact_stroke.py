"""The outline of a stroked polyline in float64, from its definition: the independent reference that
tests/test_stroke_coverage_spec.py (oracle) and tests/test_gpu_stroke_coverage.py (HIP image) hand to the exact
coverage of tests/exact_coverage.py.  Pure numpy; it imports neither the oracle nor the product.

Inputs are what the encoder stores: f32 points, the f32 width, the miter limit as an f16 value, the join and cap
styles (strings) and an optional f32 transform.  Stroking happens in local space; the transform is applied to the
outline points afterwards, in float64.  The result is a list of closed contours in device pixels whose edges are the
lines the pipeline emits (the tolerance of the coverage check counts edges per row and tile, so the same winding
function alone would not do):

* per segment a -> b with unit tangent t and n = (w / 2) (-t.y, t.x): the sides a + n -> b + n and b - n -> a - n;
* per join at p: the front line p + n_prev -> p + n_next and the back line p - n_next -> p - n_prev.  The inner side is
  a straight connection like the outer one; the overlap it creates is part of the (non-zero) winding function;
* miter (flatten.wgsl:545-614): with cr = t_prev x t_next and d = t_prev . t_next, when 2 hypot(cr, d) <
  (hypot(cr, d) + d) limit^2 and cr != 0 the intersection of the two outer offset lines is inserted, on the back side
  when cr > 0, else on the front side;
* caps (flatten.wgsl:519-543): butt, one line across; square, three lines, extended by w / 2 along the tangent;
* round caps and joins (flatten.wgsl:490-517): radius = max(0.25, |T(begin) - T(centre)|) in device space, theta =
  max(1e-4, 2 acos(1 - 0.25 / radius)), n = max(1, ceil(angle / theta)) lines: n - 1 rotations of begin - centre by
  theta in local space, the last vertex is the exact end point.  angle = |atan2(cr, d)| for a join, f32 pi for a
  cap; the arc is on the back side when cr > 0;
* a closed subpath has a join at its start point and no caps; an open one has a start cap and an end cap.

An open subpath is one contour (start cap, front sides and joins, end cap, back sides and joins); a closed one is two
(the front loop and the back loop).

arcs="rule" follows the arc rule above.  arcs="lower" / "upper" replace every arc by a dense polyline at radius
w / 2 - 0.25 between its two exact end points / circumscribed about the circle of radius w / 2: any flattening with
vertices on the circle and sagitta <= 0.25 lies between them, whatever its rule.  (0.25 is in device pixels: "lower"
needs the transform to be a similarity.  Under an anisotropic transform the rule takes its radius from the transformed
begin point alone, and the sagitta along the long axis exceeds 0.25; only the sharp check holds such entries.)

Guards (an entry that trips one is badly chosen; it is not a tolerance problem):
* every miter decision is at least MITER_GUARD (relative) away from the limit condition;
* for every arc, angle / theta is at least ARC_GUARD from the nearest integer, and n <= ARC_MAX_LINES.
Then the f32 decisions of the pipeline cannot differ from the float64 ones here.

`defect` produces deliberately wrong outlines for the sensitivity tests: "miter-wrong-side", "inner-through-point",
"square-cap-w", "arc-n+1", "arc-n-1", "no-closing-join"."""
import math

import numpy as np

ZERO_LENGTH = 1e-12      # the encoder drops a line whose extent is at most this in both axes
TOL = 0.25               # flatten.wgsl:490-517
MIN_THETA = 1e-4
MITER_GUARD = 1e-4
ARC_GUARD = 1e-3
ARC_MAX_LINES = 64
PI_F32 = float(np.float32(math.pi))
DENSE = 1024


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def f16(v):
    return float(np.float16(v))


def encoded_points(points, closed):
    """The vertices of the lines the encoder keeps: zero-length lines dropped, the closing line added."""
    pts = f32(points).reshape(-1, 2)
    out = [pts[0]]
    for p in pts[1:]:
        if abs(p[0] - out[-1][0]) > ZERO_LENGTH or abs(p[1] - out[-1][1]) > ZERO_LENGTH:
            out.append(p)
    if closed and (out[-1][0] != out[0][0] or out[-1][1] != out[0][1]):
        out.append(out[0])
    return np.array(out)


class Arc:
    """One arc the outline holds: where it is in the contour, and what the line buffer must show for it."""
    def __init__(self, contour, first, n, local, device, centre, radius, angle, theta):
        self.contour, self.first, self.n = contour, first, n       # vertices first .. first + n of that contour
        self.local, self.device = local, device                    # (n + 1, 2) each: begin, n - 1 rotated, end
        self.centre = centre                                       # device space
        self.radius, self.angle, self.theta = radius, angle, theta


class Outline:
    def __init__(self):
        self.contours, self.arcs, self.miters = [], [], []


class _Stroker:
    def __init__(self, width, join, miter_limit, start_cap, end_cap, transform, arcs, defect):
        self.h = 0.5 * float(np.float32(width))
        self.join, self.limit = join, f16(miter_limit)
        self.start_cap, self.end_cap = start_cap, end_cap
        self.t = None if transform is None else f32(transform)
        self.mode, self.defect = arcs, defect
        self.out = Outline()

    def apply(self, p):
        p = np.asarray(p, np.float64)
        if self.t is None:
            return p
        a, b, c, d, e, f = self.t
        return np.stack([a * p[..., 0] + c * p[..., 1] + e, b * p[..., 0] + d * p[..., 1] + f], axis=-1)

    def scale(self):
        """The factor of a similarity transform (the bracket needs one: 0.25 is a distance in device space)."""
        if self.t is None:
            return 1.0
        a, b, c, d, _, _ = self.t
        sx, sy = math.hypot(a, b), math.hypot(c, d)
        assert abs(sx - sy) <= 1e-6 * sx and abs(a * c + b * d) <= 1e-6 * sx * sy, "the bracket needs a similarity transform"
        return sx

    # --- arcs -------------------------------------------------------------------------------------------------------
    def arc(self, begin, end, centre, angle, cur):
        """Vertices after `begin` up to and including `end`, in local space."""
        r0 = begin - centre
        if self.mode != "rule":
            # the sweep is clockwise in the rotation below: r' = (c r.x + s r.y, -s r.x + c r.y)
            a0 = math.atan2(r0[1], r0[0])
            if self.mode == "lower":    # inscribed at radius w / 2 - 0.25 (device units), between the exact end points
                rad = max(self.h - TOL / self.scale(), 0.0)
                ang = a0 - angle * np.arange(1, DENSE) / DENSE
            else:                       # circumscribed at w / 2: every line is tangent to the circle
                rad = self.h / math.cos(0.5 * angle / DENSE)
                ang = a0 - angle * (np.arange(DENSE) + 0.5) / DENSE
            mid = centre + rad * np.stack([np.cos(ang), np.sin(ang)], axis=1)
            return list(mid) + [end]
        radius = max(TOL, float(np.hypot(*(self.apply(begin) - self.apply(centre)))))
        theta = max(MIN_THETA, 2.0 * math.acos(1.0 - TOL / radius))
        q = angle / theta
        assert q == 0.0 or abs(q - round(q)) >= ARC_GUARD, "arc: angle / theta = %.6f is within %g of an integer" % (q, ARC_GUARD)
        n = max(1, int(math.ceil(q)))
        assert n <= ARC_MAX_LINES, "arc of %d lines" % n
        if self.defect == "arc-n+1":
            n += 1
        if self.defect == "arc-n-1":
            n = max(1, n - 1)
        cs, sn = math.cos(theta), math.sin(theta)
        pts, r = [], r0
        for _ in range(n - 1):
            r = np.array([cs * r[0] + sn * r[1], -sn * r[0] + cs * r[1]])
            pts.append(centre + r)
        pts.append(end)
        local = np.array([begin] + pts)
        self.out.arcs.append(Arc(len(self.out.contours), len(cur) - 1, n, local, self.apply(local), self.apply(centre), radius, angle, theta))
        return pts

    # --- caps -------------------------------------------------------------------------------------------------------
    def cap(self, style, point, cap0, cap1, tangent, cur):
        """Vertices after cap0 up to and including cap1; `tangent` (length w / 2) points away from the stroke."""
        if style == "round":
            return self.arc(cap0, cap1, point, PI_F32, cur)
        if style == "square":
            v = tangent * (2.0 if self.defect == "square-cap-w" else 1.0)
            return [cap0 + v, cap1 + v, cap1]
        assert style == "butt"
        return [cap1]

    # --- joins ------------------------------------------------------------------------------------------------------
    def join_side(self, p, t_prev, t_next, front, cur):
        """Vertices of the join at p on the front (+n) or back (-n) side, after its first point up to and including
        its last.  Front runs p + n_prev -> p + n_next, back p - n_next -> p - n_prev."""
        n_prev = self.h * np.array([-t_prev[1], t_prev[0]])
        n_next = self.h * np.array([-t_next[1], t_next[0]])
        first, last = (p + n_prev, p + n_next) if front else (p - n_next, p - n_prev)
        cr = t_prev[0] * t_next[1] - t_prev[1] * t_next[0]
        d = t_prev[0] * t_next[0] + t_prev[1] * t_next[1]
        backside = cr > 0.0
        outer = backside != front           # the outer side is the back when cr > 0, the front otherwise
        if self.defect == "inner-through-point" and not outer and cr != 0.0:
            return [p, last]
        if self.join == "bevel" or cr == 0.0 and self.join == "miter":
            return [last]
        if self.join == "miter":
            hyp = math.hypot(cr, d)
            lhs, rhs = 2.0 * hyp, (hyp + d) * self.limit * self.limit
            if front:                       # (each join is visited twice: guard and record once)
                assert abs(lhs - rhs) >= MITER_GUARD * max(lhs, abs(rhs)), \
                    "miter decision on a knife edge: %.9g against %.9g" % (lhs, rhs)
                self.out.miters.append((tuple(p), lhs < rhs))
            if not lhs < rhs:
                return [last]
            # the intersection of the two outer offset lines: a on the previous segment's, b on the next one's
            sign = 1.0 if not backside else -1.0
            a, b = p + sign * n_prev, p + sign * n_next
            v = b - a
            miter = b - t_next * ((t_prev[0] * v[1] - t_prev[1] * v[0]) / cr)
            if self.defect == "miter-wrong-side":
                return [last] if outer else [2.0 * p - miter, last]
            return [miter, last] if outer else [last]
        assert self.join == "round"
        if outer:
            return self.arc(first, last, p, abs(math.atan2(cr, d)), cur)
        return [last]

    # --- subpaths ---------------------------------------------------------------------------------------------------
    def subpath(self, points, closed):
        P = encoded_points(points, closed)
        if len(P) < 2:
            return
        seg = P[1:] - P[:-1]
        T = seg / np.hypot(seg[:, 0], seg[:, 1])[:, None]
        N = self.h * np.stack([-T[:, 1], T[:, 0]], axis=1)
        m = len(T)
        if closed:
            skip = self.defect == "no-closing-join"
            cur = [P[0] + N[0]]
            for i in range(m):
                cur.append(P[i + 1] + N[i])
                if not (skip and i == m - 1):
                    cur += self.join_side(P[i + 1], T[i], T[(i + 1) % m], True, cur)
            self.finish(cur)
            cur = [P[m] - N[m - 1]]
            for i in range(m - 1, -1, -1):
                cur.append(P[i] - N[i])
                if not (skip and i == 0):
                    cur += self.join_side(P[i], T[i - 1], T[i], False, cur)
            self.finish(cur)
            return
        cur = [P[0] - N[0]]
        cur += self.cap(self.start_cap, P[0], P[0] - N[0], P[0] + N[0], -self.h * T[0], cur)
        for i in range(m):
            cur.append(P[i + 1] + N[i])
            if i + 1 < m:
                cur += self.join_side(P[i + 1], T[i], T[i + 1], True, cur)
        cur += self.cap(self.end_cap, P[m], P[m] + N[m - 1], P[m] - N[m - 1], self.h * T[m - 1], cur)
        for i in range(m - 1, -1, -1):
            cur.append(P[i] - N[i])
            if i > 0:
                cur += self.join_side(P[i], T[i - 1], T[i], False, cur)
        self.finish(cur)

    def finish(self, cur):
        c = np.array(cur)
        if len(c) > 1 and np.array_equal(c[0], c[-1]):      # the loop is closed by its own last line
            c = c[:-1]
        self.out.contours.append(self.apply(c))


def stroke_outline(subpaths, width, join, miter_limit, start_cap, end_cap, transform=None, arcs="rule", defect=None):
    """subpaths: a list of (points, closed).  Returns an Outline: .contours (device pixels, float64), .arcs (arcs="rule"
    only) and .miters ((point, mitered) per miter join)."""
    s = _Stroker(width, join, miter_limit, start_cap, end_cap, transform, arcs, defect)
    for points, closed in subpaths:
        s.subpath(points, closed)
    return s.out
