"""Bezier curves in float64, from their definition: the independent reference that tests/test_curve_spec.py (oracle)
and tests/test_gpu_curves.py (HIP line buffer) hold the flattener's lines to.  Pure numpy; it imports neither the oracle
nor the product.

Inputs are what the encoder stores: f32 control points and an optional f32 transform.  A quad is evaluated as the
quadratic it is (the pipeline raises it to a cubic in f32; that rounding is part of what is checked).  The transform is
applied to the control points in float64 (an affine map of a Bezier curve is the Bezier curve of the mapped points).

* Curve(points): points (2, 2) line, (3, 2) quad or (4, 2) cubic; .at(t), .d1(t), .d2(t), .radius(t).
* dense_polyline(curve, sagitta, max_step): parameters 0 = t_0 < ... < t_n = 1 such that the curve between t_i and
  t_i+1 stays within `sagitta` of the chord.  The bound is rigorous: e(t) = c(t) - chord(t) vanishes at both ends, so
  |e| <= max|c''| dt^2 / 8, and c'' is linear in t for a cubic: its largest norm is at an end of the interval.  Across
  the chord only the component of c'' along the chord's normal counts; that sharper bound is used where the curve
  cannot run past the chord's ends, i.e. where c'(t) . u >= min(c'(a) . u, c'(b) . u) - |c''' . u| dt^2 / 8 > 0 (c' . u
  is a quadratic).  So a hairpin whose arms are 10^6 px long takes a few thousand chords, most of them where it turns.
  No fixed sample count.  max_step (device px) caps the chord length on top of that, for callers who need points and
  not only chords.
* dist_to_polyline(points, polyline): distance of each point to the nearest SEGMENT of the polyline, blocked.
* segment_cover(A, B, lines, D): which of the segments A_i B_i lie within D of the polyline `lines` as a whole -- the
  distance to one straight line is convex along a segment, so a segment whose two ends are within D of the same line
  lies within D of it; others are halved until they are.  It fails as soon as an end is farther than D from every
  line; a piece shorter than MIN_PIECE whose ends are within D of two different lines is let through.
* Offsets(curve, width, t): the two parallel curves c(t) +- (w / 2) n(t), n = (-c'.y, c'.x) / |c'|, at the parameters
  t, with rho(t) = |c'|^3 / |c' x c''|, the parallel curves' own radii of curvature |rho -+ w / 2| and the predicate
  "this offset point is on the boundary of the stroke": its distance to the whole curve is at least
  w / 2 - BOUNDARY_EPS.
"""
import numpy as np

SAGITTA = 1e-4
BOUNDARY_EPS = 1e-3
MIN_PIECE = 1e-3
BLOCK = 1 << 21          # elements of one distance matrix
GROUP = 32               # chords per bounding box in dist_to_segments


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def apply(transform, p):
    """The f32-rounded transform (a, b, c, d, e, f), applied in float64."""
    p = np.asarray(p, np.float64)
    if transform is None:
        return p
    a, b, c, d, e, f = f32(transform)
    return np.stack([a * p[..., 0] + c * p[..., 1] + e, b * p[..., 0] + d * p[..., 1] + f], axis=-1)


def linear_part(transform):
    if transform is None:
        return np.eye(2)
    a, b, c, d, _, _ = f32(transform)
    return np.array([[a, c], [b, d]])


class Curve:
    def __init__(self, points, transform=None):
        self.p = apply(transform, f32(points).reshape(-1, 2))
        self.degree = len(self.p) - 1
        assert 1 <= self.degree <= 3

    def _t(self, t):
        return np.asarray(t, np.float64)[..., None]

    def at(self, t):
        t, p = self._t(t), self.p
        m = 1.0 - t
        if self.degree == 1:
            return m * p[0] + t * p[1]
        if self.degree == 2:
            return m * m * p[0] + 2 * m * t * p[1] + t * t * p[2]
        return m * m * m * p[0] + 3 * m * m * t * p[1] + 3 * m * t * t * p[2] + t * t * t * p[3]

    def d1(self, t):
        t, p = self._t(t), self.p
        m = 1.0 - t
        if self.degree == 1:
            return (p[1] - p[0]) + 0 * t
        if self.degree == 2:
            return 2 * (m * (p[1] - p[0]) + t * (p[2] - p[1]))
        return 3 * (m * m * (p[1] - p[0]) + 2 * m * t * (p[2] - p[1]) + t * t * (p[3] - p[2]))

    def d2(self, t):
        t, p = self._t(t), self.p
        if self.degree == 1:
            return np.zeros(2) + 0 * t
        if self.degree == 2:
            return 2 * (p[2] - 2 * p[1] + p[0]) + 0 * t
        return 6 * ((1.0 - t) * (p[2] - 2 * p[1] + p[0]) + t * (p[3] - 2 * p[2] + p[1]))

    def d3(self):
        p = self.p
        return 6 * (p[3] - 3 * p[2] + 3 * p[1] - p[0]) if self.degree == 3 else np.zeros(2)

    def radius(self, t):
        """The radius of curvature (inf on a straight stretch, 0 at a cusp)."""
        q, a = self.d1(t), self.d2(t)
        cr = np.abs(q[..., 0] * a[..., 1] - q[..., 1] * a[..., 0])
        sp = np.hypot(q[..., 0], q[..., 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(cr > 0, sp ** 3 / cr, np.where(sp > 0, np.inf, 0.0))


def _chord_bound(curve, a, b):
    """An upper bound of the distance of c([a, b]) from the chord c(a) c(b), per interval (see the module docstring)."""
    dt = b - a
    pa, pb = curve.at(a), curve.at(b)
    ca, cb = curve.d2(a), curve.d2(b)
    full = np.maximum(np.hypot(ca[:, 0], ca[:, 1]), np.hypot(cb[:, 0], cb[:, 1])) * dt * dt / 8
    ch = pb - pa
    L = np.hypot(ch[:, 0], ch[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = ch / L[:, None]
    nrm = np.stack([-u[:, 1], u[:, 0]], axis=1)
    across = np.maximum(np.abs((ca * nrm).sum(axis=1)), np.abs((cb * nrm).sum(axis=1))) * dt * dt / 8
    qa, qb = (curve.d1(a) * u).sum(axis=1), (curve.d1(b) * u).sum(axis=1)
    forward = np.minimum(qa, qb) - np.abs(u @ curve.d3()) * dt * dt / 8
    return np.where((L > 0) & (forward > 0), np.minimum(across, full), full), L


def dense_parameters(curve, sagitta=SAGITTA, max_step=None):
    t = np.linspace(0.0, 1.0, 17)
    for _ in range(64):
        a, b = t[:-1], t[1:]
        bound, L = _chord_bound(curve, a, b)
        k = np.ceil(np.sqrt(bound / sagitta))
        if max_step is not None:
            k = np.maximum(k, np.ceil(L / max_step))
        k = np.clip(k, 1, 64).astype(np.int64)
        if (k == 1).all():
            return t
        # interval i becomes k_i equal parts
        start = np.repeat(a, k)
        step = np.repeat((b - a) / k, k)
        j = np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k)
        t = np.concatenate([start + j * step, [1.0]])
    raise AssertionError("dense_parameters did not converge")


def dense_polyline(curve, sagitta=SAGITTA, max_step=None):
    """(t, points): the curve stays within `sagitta` of the polyline through points = c(t)."""
    t = dense_parameters(curve, sagitta, max_step)
    return t, curve.at(t)


def _point_segment(P, A, B):
    """(len(P), len(A)) distances of points to segments A_j B_j, and the parameter of the nearest point on each."""
    d = B - A
    dd = (d * d).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = ((P[:, None, :] - A[None]) * d[None]).sum(axis=2) / dd[None]
    s = np.where(dd[None] > 0, np.clip(s, 0.0, 1.0), 0.0)
    q = A[None] + s[..., None] * d[None]
    return np.hypot(P[:, None, 0] - q[..., 0], P[:, None, 1] - q[..., 1]), s


def dist_to_segments(P, A, B):
    """Distance of each point of P to the nearest of the segments A_j B_j.  The segments are taken in runs of GROUP
    consecutive ones; a run is looked at for a point only if its bounding box is no farther from the point than the
    nearest run's first vertex, so memory and time stay small for a polyline of 10^4 chords."""
    P, A, B = (np.asarray(x, np.float64).reshape(-1, 2) for x in (P, A, B))
    out = np.full(len(P), np.inf)
    if len(A) == 0 or len(P) == 0:
        return out
    if len(A) <= 4 * GROUP:
        rows = max(1, BLOCK // len(A))
        for i in range(0, len(P), rows):
            out[i:i + rows] = _point_segment(P[i:i + rows], A, B)[0].min(axis=1)
        return out
    pad = -len(A) % GROUP
    A, B = np.vstack([A, np.repeat(A[-1:], pad, axis=0)]), np.vstack([B, np.repeat(B[-1:], pad, axis=0)])
    ga, gb = A.reshape(-1, GROUP, 2), B.reshape(-1, GROUP, 2)
    lo, hi = np.minimum(ga, gb).min(axis=1), np.maximum(ga, gb).max(axis=1)
    rows = max(1, BLOCK // len(ga))
    for i in range(0, len(P), rows):
        p = P[i:i + rows]
        gap = np.maximum(np.maximum(lo[None] - p[:, None], p[:, None] - hi[None]), 0.0)
        lower = np.hypot(gap[..., 0], gap[..., 1])
        upper = np.hypot(p[:, None, 0] - ga[None, :, 0, 0], p[:, None, 1] - ga[None, :, 0, 1]).min(axis=1)
        pi, gj = np.nonzero(lower <= upper[:, None])
        step = max(1, BLOCK // GROUP)
        for k in range(0, len(pi), step):
            a, b, q = ga[gj[k:k + step]], gb[gj[k:k + step]], p[pi[k:k + step], None, :]
            d = b - a
            dd = (d * d).sum(axis=2)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((q - a) * d).sum(axis=2) / dd
            t = np.where(dd > 0, np.clip(t, 0.0, 1.0), 0.0)
            n = a + t[..., None] * d - q
            np.minimum.at(out, i + pi[k:k + step], np.hypot(n[..., 0], n[..., 1]).min(axis=1))
    return out


def dist_to_polyline(points, polyline):
    polyline = np.asarray(polyline, np.float64).reshape(-1, 2)
    if len(polyline) == 1:
        polyline = np.vstack([polyline, polyline])
    return dist_to_segments(points, polyline[:-1], polyline[1:])


def segment_cover(A, B, LA, LB, D):
    """Are the segments A_i B_i within D of the union of the lines LA_j LB_j?  Returns (largest distance seen at an
    evaluated point, the first point found farther than D away or None).  Every point evaluated lies on a segment.
    Only pairs (segment, line) with both ends of the segment inside the line's bounding box grown by D are computed."""
    A, B, LA, LB = (np.asarray(x, np.float64).reshape(-1, 2) for x in (A, B, LA, LB))
    lo, hi = np.minimum(LA, LB) - D, np.maximum(LA, LB) + D
    worst = 0.0
    while len(A):
        ok = np.zeros(len(A), bool)
        rows = max(1, BLOCK // max(1, len(LA)))
        for i in range(0, len(A), rows):
            a, b = A[i:i + rows], B[i:i + rows]
            ina = ((a[:, None] >= lo[None]) & (a[:, None] <= hi[None])).all(axis=2)
            inb = ((b[:, None] >= lo[None]) & (b[:, None] <= hi[None])).all(axis=2)
            best = np.full((2, len(a)), np.inf)
            for which, (p, inside) in enumerate(((a, ina), (b, inb))):
                pi, lj = np.nonzero(inside)
                d = LB[lj] - LA[lj]
                dd = (d * d).sum(axis=1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = ((p[pi] - LA[lj]) * d).sum(axis=1) / dd
                t = np.where(dd > 0, np.clip(t, 0.0, 1.0), 0.0)
                n = LA[lj] + t[:, None] * d - p[pi]
                dist = np.hypot(n[:, 0], n[:, 1])
                np.minimum.at(best[which], pi, dist)
                near = np.zeros(inside.shape, bool)
                near[pi, lj] = dist <= D
                if which == 0:
                    near_a = near
                else:
                    ok[i:i + rows] = (near_a & near).any(axis=1)
            far = np.flatnonzero((best[0] > D) | (best[1] > D))
            if len(far):
                k = far[0]
                return max(worst, float(best[best <= D].max(initial=0.0))), (a[k] if best[0, k] > D else b[k])
            worst = max(worst, float(best.max()))
        A, B = A[~ok], B[~ok]
        # (a piece shorter than MIN_PIECE with both ends within D of some line, but of no common one, is let through)
        long = np.hypot(*(B - A).T) >= MIN_PIECE
        A, B = A[long], B[long]
        M = 0.5 * (A + B)
        A, B = np.concatenate([A, M]), np.concatenate([M, B])
    return worst, None


def monotone_match(vertices, polyline, D):
    """Can the vertices be assigned, in their order, to positions on the polyline (arc length s) that never decrease,
    each within D of its vertex?  Greedy: the earliest position at or after the previous one; if that fails no other
    choice works.  Returns the index of the first vertex that has no such position, or -1."""
    polyline = np.asarray(polyline, np.float64)
    A, B = polyline[:-1], polyline[1:]
    d = B - A
    L = np.hypot(d[:, 0], d[:, 1])
    s0 = np.concatenate([[0.0], np.cumsum(L)])[:-1]
    safe = np.where(L > 0, L, 1.0)
    u = d / safe[:, None]
    s_prev = 0.0
    for k, v in enumerate(np.asarray(vertices, np.float64)):
        r = v[None] - A
        along = (r * u).sum(axis=1)
        across2 = (r * r).sum(axis=1) - along * along
        h2 = D * D - across2
        ok = h2 >= 0
        h = np.sqrt(np.where(ok, h2, 0.0))
        lo, hi = np.clip(along - h, 0.0, L), np.clip(along + h, 0.0, L)
        ok &= (along + h >= 0) & (along - h <= L)
        lo, hi = s0 + lo, s0 + hi
        ok &= hi >= s_prev
        if not ok.any():
            return k
        s_prev = float(np.maximum(lo[ok], s_prev).min())
    return -1


class Offsets:
    """The two parallel curves of `curve` at +-width / 2, at the parameters t (local space: apply the transform to
    .plus / .minus afterwards)."""
    def __init__(self, curve, width, t, polyline=None):
        h = 0.5 * float(np.float32(width))
        q = curve.d1(t)
        sp = np.hypot(q[:, 0], q[:, 1])
        self.valid = sp > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.stack([-q[:, 1], q[:, 0]], axis=1) / sp[:, None]
        n[~self.valid] = 0.0
        c = curve.at(t)
        self.t, self.h = t, h
        self.plus, self.minus = c + h * n, c - h * n
        self.rho = curve.radius(t)
        a = curve.d2(t)
        turn = q[:, 0] * a[:, 1] - q[:, 1] * a[:, 0]        # > 0: the curve turns towards +n, the + side is the inner one
        # the parallel curves' own radii of curvature: rho - h on the inner side (0 where it folds), rho + h on the outer
        self.rho_plus = np.where(turn > 0, np.maximum(self.rho - h, 0.0), self.rho + h)
        self.rho_minus = np.where(turn < 0, np.maximum(self.rho - h, 0.0), self.rho + h)
        poly = c if polyline is None else polyline
        self.on_boundary_plus = self.valid & (dist_to_polyline(self.plus, poly) >= h - BOUNDARY_EPS)
        self.on_boundary_minus = self.valid & (dist_to_polyline(self.minus, poly) >= h - BOUNDARY_EPS)
