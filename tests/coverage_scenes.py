"""A deterministic battery of hostile fill geometry for the exact-coverage checks (tests/test_coverage_spec.py on the
oracle, tests/test_gpu_coverage.py on the HIP image).  Every entry is one opaque white fill (or one stroked line
segment, whose outline is an exact rectangle) on a transparent base, in both fill rules, together with the float64
contours that tests/exact_coverage.py integrates and a tolerance class:

* "ident"  -- identity transform, f32-exact coordinates (entries about rounding say so);
* "large"  -- vertices at +-2^12 ... +-2^16: path_tiling's intersection formulas run on absolute f32 coordinates;
* "xform"  -- a non-identity transform, applied by flatten in f32 (the reference applies it in float64 to the same
  f32 inputs);
* "stroke" -- the outline is computed by the stroker in f32;
* "stroke-xform" -- a stroke under a non-identity transform: the stroker works in local space, flatten transforms its
  lines in f32.

Families (the `family` field): 1 rectangles on and near pixel / tile lines, 2 geometry outside the viewport,
3 near-horizontal / near-vertical / corner-crossing edges, 4 degenerate contours, 5 winding other than +-1, 6 large
coordinates, 7 transforms, 8 stroked segments, 9 target sizes, 10 the same expected alpha through the CLIPS and PAINTS
instantiations of fine (see `variants`).

STROKE_BATTERY holds stroked polylines (StrokeEntry), whose reference outline is tests/exact_stroke.py's and which are
rendered non-zero only (the outline overlaps itself at every join): 11 joins x caps on an open L, 12 closed subpaths,
13 turning angles and miter limits, 14 extremes, 15 transforms.  The encoder writes every path point as f32 (it has no
i16 form to choose), so there is no entry per point format.  Family 3 also holds the outline that showed how far the
MSAA band reaches past the end of an edge (near-vertical-cap-end) and its siblings.

CURVE_BATTERY holds curves (CurveEntry), whose reference is tests/exact_curve.py and whose LINES are checked
(tests/test_curve_spec.py on the oracle, tests/test_gpu_curves.py on the HIP line buffer): 16 one filled cubic (plain,
loop, cusps, inflection, sub-pixel), 17 degenerate control polygons, 18 deep subdivision trees, a full batch, long and
clamped pieces, 19 quads and contours of several segments, 20 transforms and large coordinates, 21 stroked cubics at
widths 0.3 ... 120, 22 joins between cubics, round caps and strokes under transforms.  Every entry names the route of
the flattener it is there for; test_curve_spec.test_the_battery_reaches_its_routes holds it to that."""
import math

import numpy as np

import exact_stroke

from jello_amd import Brush, Cap, ColorStop, Compose, Fill, Join, Mix, Path, RenderParams, Scene, Stroke

WHITE = (1.0, 1.0, 1.0, 1.0)
RULES = ("nonzero", "evenodd")


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


class Entry:
    def __init__(self, name, family, width, height, contours, tclass="ident", transform=None, stroke=None):
        self.name, self.family, self.width, self.height = name, family, width, height
        self.contours = [f32(c).reshape(-1, 2) for c in contours]   # the inputs, as the encoder stores them
        self.tclass, self.transform, self.stroke = tclass, transform, stroke

    @property
    def id(self):
        return "f%d-%s" % (self.family, self.name)

    def path(self):
        p = Path()
        if self.stroke is not None:
            (x0, y0), (x1, y1) = self.contours[0]
            return p.move_to(float(x0), float(y0)).line_to(float(x1), float(y1))
        for c in self.contours:
            p.move_to(float(c[0, 0]), float(c[0, 1]))
            for x, y in c[1:]:
                p.line_to(float(x), float(y))
            p.close()
        return p

    def reference_contours(self):
        """The outline in device pixels, float64."""
        if self.stroke is not None:
            width, cap = self.stroke
            (x0, y0), (x1, y1) = self.contours[0]
            w = float(np.float32(width))
            L = math.hypot(x1 - x0, y1 - y0)
            ux, uy = (x1 - x0) / L, (y1 - y0) / L
            nx, ny = -uy * w / 2, ux * w / 2
            ext = w / 2 if cap == Cap.Square else 0.0
            ax, ay, bx, by = x0 - ux * ext, y0 - uy * ext, x1 + ux * ext, y1 + uy * ext
            return [np.array([[ax + nx, ay + ny], [bx + nx, by + ny], [bx - nx, by - ny], [ax - nx, ay - ny]])]
        if self.transform is None:
            return self.contours
        a, b, c, d, e, f = f32(self.transform)   # the encoder stores the transform as f32
        return [np.stack([a * p[:, 0] + c * p[:, 1] + e, b * p[:, 0] + d * p[:, 1] + f], axis=1) for p in self.contours]

    def max_coordinate(self):
        m = max(self.width, self.height, 16)
        for c in self.reference_contours():
            m = max(m, float(np.abs(c).max()))
        return m

    def scene(self, rule, variant="plain"):
        """variant "plain": the fill alone; "clip": inside a clip layer whose clip is the exact viewport rectangle
        (the CLIPS instantiation of k_fine_area and coarse's walk for scenes with clip layers); "paint": filled with a
        linear gradient whose two stops are opaque white (the PAINTS instantiation)."""
        s = Scene()
        fill = Fill.NonZero if rule == "nonzero" else Fill.EvenOdd
        brush = Brush.solid(WHITE)
        if variant == "paint":
            brush = Brush.linear((0.0, 0.0), (float(self.width), float(self.height) + 1.0),
                                 [ColorStop(0.0, WHITE), ColorStop(1.0, WHITE)])
        if variant == "clip":
            s.push_layer(Mix.Clip, Compose.SrcOver, 1.0, None, Path.rect(0, 0, self.width, self.height))
        if self.stroke is not None:
            width, cap = self.stroke
            s.stroke(Stroke(width, Join.Miter, 4.0, cap, cap), None, brush, None, self.path())
        else:
            s.fill(fill, self.transform, brush, None, self.path())
        if variant == "clip":
            s.pop_layer()
        return s

    def params(self, aa):
        return RenderParams(self.width, self.height, aa=aa)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def reverse(c):
    return list(reversed(c))


def star(cx, cy, r, n, k, phase=0.1):
    """Regular star polygon {n/k}: winding k at its centre."""
    return [(cx + r * math.cos(phase + 2 * math.pi * k * i / n), cy + r * math.sin(phase + 2 * math.pi * k * i / n)) for i in range(n)]


def _battery():
    E = []
    # --- 1: rectangle edges on pixel lines, tile lines, 2^-10 / 2^-20 off them, and on the viewport's four edges
    E.append(Entry("pixel-lines", 1, 64, 48, [rect(3, 5, 61, 45)]))
    E.append(Entry("tile-lines", 1, 64, 64, [rect(16, 16, 48, 64)]))
    for k in (10, 20):
        e = 2.0 ** -k
        E.append(Entry("tile-lines+2^-%d" % k, 1, 64, 64, [rect(16 + e, 16 + e, 48 + e, 48 + e)]))
        E.append(Entry("tile-lines-2^-%d" % k, 1, 64, 64, [rect(16 - e, 16 - e, 48 - e, 48 - e)]))
        E.append(Entry("pixel-lines+-2^-%d" % k, 1, 48, 40, [rect(5 + e, 3 - e, 37 - e, 29 + e)]))
    E.append(Entry("viewport", 1, 48, 40, [rect(0, 0, 48, 40)]))
    E.append(Entry("viewport-reversed", 1, 48, 40, [reverse(rect(0, 0, 48, 40))]))
    # --- 2: outside the viewport: left edge (backdrop), top, right, bottom; entering the tile box through each side
    W, H = 80, 64
    E.append(Entry("left-shallow", 2, W, H, [[(-40.0, 10.0), (50.5, 21.25), (-30.0, 55.0)]]))
    E.append(Entry("left-steep", 2, W, H, [[(-3.0, -20.0), (30.25, 70.0), (-9.5, 90.0)]]))
    E.append(Entry("left-only", 2, W, H, [[(-40.0, 3.5), (-1.0, 33.25), (-60.0, 60.75)]]))   # only the backdrop carries it
    E.append(Entry("top", 2, W, H, [[(10.0, -30.0), (70.0, -25.0), (40.25, 37.5)]]))
    E.append(Entry("right", 2, W, H, [[(120.0, 5.0), (20.5, 30.5), (150.0, 60.0)]]))
    E.append(Entry("bottom", 2, W, H, [[(5.0, 100.0), (41.5, 9.75), (77.0, 130.0)]]))
    E.append(Entry("all-sides", 2, W, H, [[(-20.0, 30.0), (40.0, -17.0), (107.0, 33.0), (41.0, 96.0)]]))
    E.append(Entry("shallow-through-box", 2, W, H, [[(-300.0, 20.0), (400.0, 27.0), (400.0, 50.0), (-300.0, 41.0)]]))
    E.append(Entry("steep-through-box", 2, W, H, [[(30.0, -300.0), (37.0, 400.0), (60.0, 400.0), (51.0, -300.0)]]))
    big = rect(-50, -50, W + 50, H + 50)
    E.append(Entry("cover-w1", 2, W, H, [big]))
    E.append(Entry("cover-w2", 2, W, H, [big, big]))
    E.append(Entry("cover-w0", 2, W, H, [big, reverse(big)]))
    rng = np.random.default_rng(20261016)
    E.append(Entry("random-outside", 2, W, H, [rng.uniform(-60, 140, (9, 2))]))
    # --- 3: near-horizontal edges spanning the width, many in one tile row; near-vertical; corners; 45 degrees
    W = 96
    bands = []
    for i, s in enumerate((1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 3e-4, 3e-5, 3e-6, 3e-7, 2e-3, 5e-4, 5e-5)):
        y = 33.0 + 1.25 * i
        bands.append([(-2.0, y), (W + 2.0, y + s * (W + 4)), (W + 2.0, y + 0.625), (-2.0, y + 0.625 - s * (W + 4))])
    E.append(Entry("near-horizontal-one-tile-row", 3, W, 64, bands))
    E.append(Entry("near-horizontal-each", 3, W, 64,
                   [[(-1.0, 8.0 + 9 * i), (W + 1.0, 8.0 + 9 * i + 10.0 ** -(3 + i)), (W + 1.0, 12.0 + 9 * i)] for i in range(5)]))
    E.append(Entry("near-vertical", 3, 64, 96, [[(20.0 + 9 * i, -1.0), (20.0 + 9 * i + 10.0 ** -(3 + i), 97.0), (24.0 + 9 * i, 97.0)]
                                                for i in range(5)]))
    E.append(Entry("tile-corners", 3, 64, 64, [[(0.0, 0.0), (64.0, 64.0), (0.0, 64.0)], [(64.0, 0.0), (16.0, 48.0), (64.0, 48.0)]]))
    E.append(Entry("pixel-corners", 3, 64, 48, [[(3.0, 5.0), (43.0, 25.0), (61.0, 44.0), (7.0, 39.0)]]))
    E.append(Entry("diagonal-45", 3, 64, 64, [[(8.0, 2.0), (58.0, 52.0), (8.0, 52.0)], [(60.5, 3.5), (20.5, 43.5), (60.5, 43.5)]]))
    # a near-vertical edge that ends inside a pixel where a horizontal edge begins: the outline of a 6-px butt-capped
    # miter stroke through a 0.1-degree turn (its end cap is 1.7e-3 off vertical; at 8 samples the quantised LUT line of
    # the bottom edge, y = 50.93, puts the sample at (100.3125, 50.9375) above it although the edge has ended at
    # x = 100.005), and quads with the same corner at other offsets inside the pixel, slopes 5e-4 ... 5e-3, mirrored
    cap = exact_stroke.stroke_outline([([(20.0, 48.0), (60.0, 48.0), (100.0, 47.93)], False)], 6.0, "miter", 4.0, "butt", "butt")
    E.append(Entry("near-vertical-cap-end", 3, 128, 96, cap.contours))
    quads = [[(bx - 12.0, cy - 6.0), (bx + fx - 6.0 * slope, cy - 6.0), (bx + fx, cy), (bx - 12.0, cy)]
             for (bx, fx) in ((20.0, 0.00525), (50.0, 0.25), (80.0, 0.6), (110.0, 0.95))
             for (cy, slope) in ((20.93, 5e-4), (50.93, 1.75e-3), (80.93, 5e-3))]
    for name, mx, my in (("", 1, 1), ("-mirror-x", -1, 1), ("-mirror-y", 1, -1), ("-mirror-xy", -1, -1)):
        E.append(Entry("near-vertical-ends-in-pixel" + name, 3, 128, 96,
                       [[(x if mx > 0 else 128.0 - x, y if my > 0 else 96.0 - y) for x, y in q] for q in quads]))
    # --- 4: slivers, sub-pixel triangles, zero-area and repeated / zero-length edges
    E.append(Entry("sliver-1e-4", 4, 64, 48, [[(3.0, 4.0), (60.0, 40.0), (60.0, 40.0001)]]))
    E.append(Entry("sliver-vertical", 4, 64, 48, [[(20.25, 2.0), (20.2501, 45.0), (20.2502, 2.0)]]))
    E.append(Entry("in-one-pixel", 4, 32, 32, [[(5.25, 7.25), (5.875, 7.375), (5.5, 7.875)], [(16.0625, 16.0625), (16.9375, 16.5), (16.125, 16.875)]]))
    E.append(Entry("collinear", 4, 48, 48, [[(3.0, 3.0), (20.0, 20.0), (45.0, 45.0)], [(40.0, 5.0), (10.0, 5.0), (25.0, 5.0)]]))
    E.append(Entry("repeated-vertices", 4, 48, 48, [[(4.5, 4.5), (4.5, 4.5), (40.25, 9.0), (40.25, 9.0), (40.25, 9.0), (20.0, 44.0)]]))
    E.append(Entry("zero-closing-edge", 4, 48, 48, [[(6.0, 40.5), (43.0, 30.25), (17.5, 3.0), (6.0, 40.5)]]))
    # --- 5: winding beyond +-1, nested squares, a tile full of edges
    E.append(Entry("star-7", 5, 96, 96, [star(48.0, 48.0, 44.0, 15, 7)]))
    E.append(Entry("star-minus-7", 5, 96, 96, [reverse(star(48.0, 48.0, 44.0, 15, 7))]))
    E.append(Entry("star-3-and-5", 5, 96, 96, [star(30.0, 40.0, 26.0, 7, 3), star(62.0, 56.0, 30.0, 11, 5, 0.3)]))
    E.append(Entry("nested-squares-20", 5, 96, 96, [rect(4 + 2.0 * i + 0.25, 4 + 2.0 * i + 0.25, 92 - 2.0 * i - 0.25, 92 - 2.0 * i - 0.25)
                                                    for i in range(20)]))
    zig = [(16.25 + 15.5 * (i % 2), 16.0 + 0.075 * i) for i in range(210)] + [(40.0, 40.0)]
    E.append(Entry("zigzag-one-tile", 5, 64, 64, [zig]))
    # --- 6: large coordinates crossing the viewport
    for k in (12, 14, 16):
        L = 2.0 ** k
        E.append(Entry("large-2^%d" % k, 6, 64, 64, [[(-L, -L + 3.0), (L, 7.0 - L * 0.25), (20.5, L)]], tclass="large"))
    E.append(Entry("large-far-left", 6, 64, 64, [[(-2.0 ** 16, 10.0), (40.0, 23.0), (-2.0 ** 15, 60.0)]], tclass="large"))
    # --- 7: transforms
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    tri = [[(2.0, 3.0), (40.0, 8.0), (14.0, 36.0)], rect(20, 20, 36, 28)]
    E.append(Entry("rotate-30", 7, 64, 64, tri, "xform", (c, s, -s, c, 20.0, 4.0)))
    E.append(Entry("scale-3x0.5", 7, 128, 32, tri, "xform", (3.0, 0.0, 0.0, 0.5, 1.5, 7.25)))
    E.append(Entry("skew", 7, 96, 64, tri, "xform", (1.0, 0.0, 0.75, 1.0, 0.0, 10.0)))
    E.append(Entry("mirror", 7, 64, 64, tri, "xform", (-1.0, 0.0, 0.0, 1.0, 60.0, 3.0)))
    # --- 8: stroked single line segments (butt / square caps): exact rectangles
    for i, (ang, w) in enumerate(((0.0, 3.0), (17.0, 0.05), (45.0, 40.0), (90.0, 0.7), (123.0, 7.5), (200.0, 1.0))):
        r = math.radians(ang)
        p0 = (48.0 - 30.0 * math.cos(r), 48.0 - 30.0 * math.sin(r))
        p1 = (48.0 + 30.0 * math.cos(r), 48.0 + 30.0 * math.sin(r))
        for cap in (Cap.Butt, Cap.Square):
            E.append(Entry("stroke-%g-w%g-%s" % (ang, w, cap.name.lower()), 8, 96, 96, [[p0, p1]], "stroke", stroke=(w, cap)))
    # --- 9: target sizes
    E.append(Entry("1x1", 9, 1, 1, [[(0.25, -0.5), (1.5, 0.75), (-0.25, 0.875)]]))
    rng = np.random.default_rng(9)
    for w, h in ((15, 17), (17, 33), (250, 130)):
        E.append(Entry("%dx%d" % (w, h), 9, w, h, [rng.uniform(-5, [w + 5, h + 5], (7, 2)), rng.uniform(-5, [w + 5, h + 5], (5, 2))]))
    rng = np.random.default_rng(1024)
    for k in range(2):
        E.append(Entry("1024x1024-%d" % k, 9, 1024, 1024, [rng.uniform(-40, 1064, (n, 2)) for n in (17, 11, 23)]))
    return E


JOINS = {"miter": Join.Miter, "bevel": Join.Bevel, "round": Join.Round}
CAPS = {"butt": Cap.Butt, "square": Cap.Square, "round": Cap.Round}


class StrokeEntry(Entry):
    """A stroked polyline (families 11-15): `subpaths` is a list of (points, closed); join and caps are the style names
    of tests/exact_stroke.py, which computes the reference outline.  Strokes are filled non-zero whatever the rule."""
    def __init__(self, name, family, width, height, subpaths, stroke_width, join="miter", limit=4.0, caps=("butt", "butt"),
                 transform=None, defect=None):
        self.name, self.family, self.width, self.height = name, family, width, height
        self.subpaths = [(f32(p).reshape(-1, 2), bool(closed)) for p, closed in subpaths]
        self.contours = [p for p, _ in self.subpaths]
        self.stroke_width, self.join, self.limit, self.caps = stroke_width, join, limit, caps
        self.transform, self.defect = transform, defect
        self.tclass = "stroke" if transform is None else "stroke-xform"
        self.stroke = None
        self._outline = {}

    def with_defect(self, defect=None, **changes):
        """A copy whose reference outline is wrong in one respect (the sensitivity tests)."""
        kw = dict(stroke_width=self.stroke_width, join=self.join, limit=self.limit, caps=self.caps, transform=self.transform)
        kw.update(changes)
        return StrokeEntry(self.name, self.family, self.width, self.height, self.subpaths, defect=defect, **kw)

    def outline(self, arcs="rule"):
        if arcs not in self._outline:
            self._outline[arcs] = exact_stroke.stroke_outline(self.subpaths, self.stroke_width, self.join, self.limit, self.caps[0],
                                                              self.caps[1], self.transform, arcs, self.defect)
        return self._outline[arcs]

    def path(self):
        p = Path()
        for pts, closed in self.subpaths:
            p.move_to(float(pts[0, 0]), float(pts[0, 1]))
            for x, y in pts[1:]:
                p.line_to(float(x), float(y))
            if closed:
                p.close()
        return p

    def reference_contours(self):
        return self.outline().contours

    def transform_norm(self):
        """The largest factor by which the linear part stretches an error bounded per coordinate."""
        if self.transform is None:
            return 1.0
        a, b, c, d, _, _ = self.transform
        return max(abs(a) + abs(c), abs(b) + abs(d))

    def max_local_coordinate(self):
        """The largest coordinate of the outline before the transform."""
        if self.transform is None:
            return self.max_coordinate()
        local = exact_stroke.stroke_outline(self.subpaths, self.stroke_width, self.join, self.limit, self.caps[0], self.caps[1],
                                            None, "upper")
        return max(float(np.abs(c).max()) for c in local.contours)

    def arc_edges(self):
        """(edge index in exact_coverage.edges_of(reference_contours()), arc) for every line of every arc."""
        contours = self.reference_contours()
        base = np.concatenate([[0], np.cumsum([len(c) for c in contours])])
        out = []
        for arc in self.outline().arcs:
            n = len(contours[arc.contour])
            out += [(int(base[arc.contour]) + (arc.first + k) % n, arc) for k in range(arc.n)]
        return out

    def scene(self, rule="nonzero", variant="plain"):
        s = Scene()
        brush = Brush.solid(WHITE)
        if variant == "paint":
            brush = Brush.linear((0.0, 0.0), (float(self.width), float(self.height) + 1.0),
                                 [ColorStop(0.0, WHITE), ColorStop(1.0, WHITE)])
        if variant == "clip":
            s.push_layer(Mix.Clip, Compose.SrcOver, 1.0, None, Path.rect(0, 0, self.width, self.height))
        style = Stroke(self.stroke_width, JOINS[self.join], self.limit, CAPS[self.caps[0]], CAPS[self.caps[1]])
        s.stroke(style, self.transform, brush, None, self.path())
        if variant == "clip":
            s.pop_layer()
        return s


def corner(apex, leg, interior_deg, mirror=False, heading_deg=0.0):
    """Two legs of length `leg` meeting at `apex` with the given interior angle; the first leg arrives with the given
    heading.  mirror flips the turning direction (the sign of cr)."""
    h = math.radians(heading_deg)
    turn = math.radians(180.0 - interior_deg) * (-1.0 if mirror else 1.0)
    ax, ay = apex
    return [(ax - leg * math.cos(h), ay - leg * math.sin(h)), (ax, ay), (ax + leg * math.cos(h + turn), ay + leg * math.sin(h + turn))]


def _stroke_battery():
    E = []
    # --- 11: joins x caps on an open L whose outline mixes tile lines (x = 64, y = 16), pixel lines and fractions
    L = [(13.0, 19.0), (61.0, 19.0), (61.0, 70.25)]
    caps = ("butt", "square", "round")
    for join in ("miter", "bevel", "round"):
        for k, c in enumerate(caps):
            E.append(StrokeEntry("L-%s-%s-%s" % (join, c, caps[(k + 1) % 3]), 11, 96, 96, [(L, False)], 6.0, join, 4.0, (c, caps[(k + 1) % 3])))
    E.append(StrokeEntry("L-fraction-round", 11, 96, 96, [([(12.3, 20.7), (70.1, 31.9), (40.6, 80.2)], False)], 7.3, "round", 4.0, ("round", "round")))
    E.append(StrokeEntry("stadium", 11, 96, 96, [([(20.5, 30.25), (70.0, 60.0)], False)], 12.0, "miter", 4.0, ("round", "round")))
    # --- 12: closed subpaths (the closing join); the outer outline of the mitered ones lies on tile / pixel lines
    for join in ("miter", "bevel", "round"):
        E.append(StrokeEntry("rect-%s" % join, 12, 96, 96, [(rect(19, 19, 77, 61), True)], 6.0, join))
        E.append(StrokeEntry("triangle-%s" % join, 12, 96, 96, [([(20.0, 76.0), (76.0, 76.0), (20.0, 20.0)], True)], 8.0, join))
    E.append(StrokeEntry("triangle-explicit-close", 12, 96, 96, [([(20.5, 70.25), (80.0, 60.0), (33.0, 12.0), (20.5, 70.25)], True)], 5.0, "miter"))
    E.append(StrokeEntry("two-subpaths", 12, 96, 96, [([(10.0, 10.0), (40.0, 12.0), (20.0, 40.0)], True),
                                                       ([(50.0, 50.0), (85.0, 55.0), (60.0, 85.0)], False)], 4.0, "miter", 4.0, ("square", "butt")))
    # --- 13: turning angles.  Limit 4 flips at an interior angle of 28.955 degrees, 1.5 at 83.62, 10 at 11.48
    for ang in (5.0, 28.0, 28.9, 29.0, 30.0, 90.0, 150.0, 175.0, 179.9):
        for mirror in (False, True):
            E.append(StrokeEntry("angle-%g%s" % (ang, "-mirror" if mirror else ""), 13, 128, 96,
                                 [(corner((90.25, 48.5), 60.0, ang, mirror), False)], 6.0, "miter", 4.0))
    for limit, ang in ((1.5, 80.0), (1.5, 90.0), (10.0, 10.0), (10.0, 15.0)):
        for mirror in (False, True):
            E.append(StrokeEntry("limit-%g-angle-%g%s" % (limit, ang, "-mirror" if mirror else ""), 13, 128, 96,
                                 [(corner((90.25, 48.5), 60.0, ang, mirror, 10.0), False)], 6.0, "miter", limit))
    for join in ("miter", "bevel", "round"):
        E.append(StrokeEntry("reversal-%s" % join, 13, 96, 96, [([(20.0, 40.5), (70.0, 40.5), (35.0, 40.5)], False)], 8.0, join))
        E.append(StrokeEntry("collinear-%s" % join, 13, 96, 96, [([(40.5, 10.0), (40.5, 50.0), (40.5, 85.0)], False)], 8.0, join))
    for ang in (30.0, 90.0, 150.0, 179.0):
        for mirror in (False, True):
            E.append(StrokeEntry("round-angle-%g%s" % (ang, "-mirror" if mirror else ""), 13, 128, 96,
                                 [(corner((84.25, 48.5), 55.0, ang, mirror, -7.0), False)], 9.0, "round"))
    # --- 14: extremes
    stairs = [(30.0 + 10.0 * ((i + 1) // 2), 30.0 + 10.0 * (i // 2)) for i in range(8)]
    E.append(StrokeEntry("w40-on-segments-of-10", 14, 128, 128, [(stairs, False)], 40.0, "miter", 4.0, ("square", "butt")))
    E.append(StrokeEntry("w40-on-segments-of-10-round", 14, 128, 128, [(stairs, False)], 40.0, "round", 4.0, ("round", "round")))
    zz = [(10.0 + 19.25 * i, 30.0 + 41.5 * (i % 2)) for i in range(5)]
    E.append(StrokeEntry("w0.05", 14, 96, 96, [(zz, False)], 0.05, "miter"))
    E.append(StrokeEntry("w0.3", 14, 96, 96, [(zz, False)], 0.3, "miter", 4.0, ("square", "square")))
    E.append(StrokeEntry("w0.3-round-join", 14, 96, 96, [(zz, False)], 0.3, "round"))          # arcs of one line
    E.append(StrokeEntry("w0.6-round", 14, 96, 96, [(zz, False)], 0.6, "round", 4.0, ("round", "round")))
    joins = [(17.25 + 13.5 * (i % 2), 17.0 + 0.14 * i) for i in range(102)]
    E.append(StrokeEntry("100-joins-one-tile", 14, 64, 64, [(joins, False)], 1.0, "miter"))
    E.append(StrokeEntry("100-joins-one-tile-bevel", 14, 64, 64, [(joins, False)], 0.5, "bevel", 4.0, ("square", "square")))
    out = [(-20.0, 30.0), (48.0, -25.0), (120.0, 50.0), (40.0, 125.0), (-25.0, 60.0)]
    E.append(StrokeEntry("leaves-all-sides", 14, 96, 96, [(out, False)], 9.0, "miter"))
    E.append(StrokeEntry("leaves-all-sides-round-closed", 14, 96, 96, [(out, True)], 9.0, "round"))
    zl = [(20.0, 25.5), (60.25, 30.0), (60.25, 30.0), (30.0, 75.0)]
    E.append(StrokeEntry("zero-length-segment", 14, 96, 96, [(zl, False)], 5.0, "miter", 4.0, ("square", "round")))
    E.append(StrokeEntry("zero-length-segment-removed", 14, 96, 96, [(zl[:2] + zl[3:], False)], 5.0, "miter", 4.0, ("square", "round")))
    rng = np.random.default_rng(20261017)
    E.append(StrokeEntry("random-12-open", 14, 96, 96, [(rng.uniform(8, 88, (12, 2)), False)], 3.0, "miter", 4.0, ("butt", "square")))
    E.append(StrokeEntry("random-12-closed", 14, 96, 96, [(rng.uniform(8, 88, (12, 2)), True)], 3.0, "miter"))
    E.append(StrokeEntry("random-12-closed-round", 14, 96, 96, [(rng.uniform(8, 88, (12, 2)), True)], 4.5, "round"))
    # a round cap of 60 lines: radius 735, its arc crosses the viewport near y = 25
    E.append(StrokeEntry("round-cap-60-lines", 14, 96, 96, [([(48.0, 760.0), (48.0, 900.0)], False)], 1470.0, "miter", 4.0, ("round", "butt")))
    # --- 15: transforms (class "stroke-xform")
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    Lx = [(4.0, 6.0), (40.0, 8.5), (30.0, 36.0)]
    for join, cp in (("miter", ("butt", "square")), ("round", ("round", "round"))):
        E.append(StrokeEntry("rotate-30-%s" % join, 15, 64, 64, [(Lx, False)], 5.0, join, 4.0, cp, (c, s, -s, c, 22.0, 4.0)))
        E.append(StrokeEntry("scale-3x0.5-%s" % join, 15, 144, 32, [(Lx, False)], 5.0, join, 4.0, cp, (3.0, 0.0, 0.0, 0.5, 6.5, 3.25)))
        E.append(StrokeEntry("skew-%s" % join, 15, 96, 64, [(Lx, False)], 5.0, join, 4.0, cp, (1.0, 0.0, 0.75, 1.0, 4.0, 10.0)))
        E.append(StrokeEntry("mirror-%s" % join, 15, 64, 64, [(Lx, False)], 5.0, join, 4.0, cp, (-1.0, 0.0, 0.0, 1.0, 60.0, 8.0)))
        E.append(StrokeEntry("zoom-40-w0.8-%s" % join, 15, 96, 96, [([(0.3, 0.4), (1.7, 0.55), (1.2, 1.9)], False)], 0.8, join, 4.0, cp,
                             (40.0, 0.0, 0.0, 40.0, 2.0, 3.0)))
        E.append(StrokeEntry("shrink-8-w200-%s" % join, 15, 288, 128, [([(250.0, 300.0), (1900.0, 420.0), (1500.0, 800.0)], False)], 200.0, join,
                             4.0, cp, (0.125, 0.0, 0.0, 0.125, 3.0, -10.0)))
    E.append(StrokeEntry("closed-rotate-30-round", 15, 64, 64, [([(6.0, 6.0), (38.0, 9.0), (20.0, 34.0)], True)], 4.0, "round", 4.0,
                         ("butt", "butt"), (c, s, -s, c, 22.0, 4.0)))
    return E


class CurveEntry:
    """Curves (families 16-22) for tests/test_curve_spec.py and tests/test_gpu_curves.py, whose reference is
    tests/exact_curve.py.  `paths` is a list of paths, each a list of subpaths (start point, segments); a segment is
    the tuple of its remaining control points: one (line), two (quad) or three (cubic).  A fill draws every path as its
    own non-zero fill (the encoder closes each subpath with a line unless it ends on its start point, bit for bit); a
    stroke entry has one path of one open subpath and `stroke` = (width, join, miter limit, start cap, end cap).
    `route` says what the entry is there for; `unbounded` says why the shader promises no distance for it (a piece
    accepted at SUBDIV_LIMIT without an error test, a piece clamped to 100 lines): the structure checks still hold."""
    def __init__(self, name, family, width, height, paths, route, tclass=None, transform=None, stroke=None, unbounded=None):
        self.name, self.family, self.width, self.height = name, family, width, height
        self.paths = [[(tuple(start), [tuple(tuple(q) for q in seg) for seg in segs]) for start, segs in path] for path in paths]
        self.route, self.transform, self.stroke, self.unbounded = route, transform, stroke, unbounded
        if tclass is None:
            tclass = ("stroke" if transform is None else "stroke-xform") if stroke else ("ident" if transform is None else "xform")
        self.tclass = tclass

    @property
    def id(self):
        return "f%d-%s" % (self.family, self.name)

    def path(self, k):
        p = Path()
        for start, segs in self.paths[k]:
            p.move_to(*start)
            for seg in segs:
                flat = [float(v) for q in seg for v in q]
                {1: p.line_to, 2: p.quad_to, 3: p.cubic_to}[len(seg)](*flat)
        return p

    def control_points(self, k=None):
        """Per subpath of path k (or of all paths): the control polygons of its segments, f32 values, local space."""
        out = []
        for path in (self.paths if k is None else [self.paths[k]]):
            for start, segs in path:
                cur, polys = start, []
                for seg in segs:
                    polys.append(f32([cur] + list(seg)))
                    cur = seg[-1]
                out.append(polys)
        return out

    def transform_norm(self):
        if self.transform is None:
            return 1.0
        a, b, c, d, _, _ = self.transform
        return max(abs(a) + abs(c), abs(b) + abs(d))

    def _local_points(self):
        return np.concatenate([p for polys in self.control_points() for p in polys])

    def max_local_coordinate(self):
        half = 0.5 * self.stroke[0] if self.stroke else 0.0
        return float(np.abs(self._local_points()).max()) + half

    def max_coordinate(self):
        """The control polygon bounds the curve, and the roundings of an f32 evaluation scale with its points."""
        p = self._local_points()
        if self.transform is not None:
            a, b, c, d, e, f = f32(self.transform)
            p = np.stack([a * p[:, 0] + c * p[:, 1] + e, b * p[:, 0] + d * p[:, 1] + f], axis=1)
        half = 0.5 * self.stroke[0] * self.transform_norm() if self.stroke else 0.0
        return max(self.width, self.height, 16, float(np.abs(p).max()) + half)

    def scene(self, rule="nonzero", variant="plain"):
        s = Scene()
        brush = Brush.solid(WHITE)
        for k in range(len(self.paths)):
            if self.stroke:
                w, join, limit, cap0, cap1 = self.stroke
                s.stroke(Stroke(w, JOINS[join], limit, CAPS[cap0], CAPS[cap1]), self.transform, brush, None, self.path(k))
            else:
                s.fill(Fill.NonZero if rule == "nonzero" else Fill.EvenOdd, self.transform, brush, None, self.path(k))
        return s

    def params(self, aa):
        return RenderParams(self.width, self.height, aa=aa)


PLAIN = [(40, 40), (200, 400), (300, 20), (460, 300)]
LOOP = [(100, 300), (450, 50), (50, 50), (400, 300)]
CUSP = [(100, 400), (400, 100), (100, 100), (400, 400)]          # c'(1/2) = 0 exactly, symmetric about x = 250
CUSP_SHEARED = [(150, 400), (375, 100), (75, 100), (450, 400)]   # its image under x + y / 4 - 50: a cusp, not symmetric
ESS = [(60, 250), (250, -50), (260, 550), (450, 250)]


def hairpin(right, left, dx=0.0):
    return [(100 + dx, 100), (right + dx, 110), (left + dx, 120), (120 + dx, 130)]


HAIRPIN = hairpin(4000, -3000)
TWO_SMOOTH = [(60, 300), [((100, 100), (200, 80), (260, 200)), ((320, 320), (380, 440), (460, 200))]]   # tangent (60, 120) both sides
TWO_CORNER = [(60, 300), [((100, 100), (200, 80), (260, 200)), ((380, 140), (400, 300), (460, 380))]]   # (60, 120) then (120, -60)


def one(points):
    return [[(points[0], [tuple(points[1:])])]]


def _curve_battery():
    E = []
    BUTT = ("butt", "butt")
    # --- 16: one cubic, filled
    E.append(CurveEntry("plain", 16, 512, 512, one(PLAIN), "cooperative subdivision, depth 3"))
    E.append(CurveEntry("loop", 16, 512, 512, one(LOOP), "a self-crossing"))
    E.append(CurveEntry("cusp", 16, 512, 512, one(CUSP), "an exact, symmetric cusp: the derivative vanishes at a subdivision point"))
    E.append(CurveEntry("cusp-sheared", 16, 512, 512, one(CUSP_SHEARED), "an exact cusp that is not symmetric"))
    E.append(CurveEntry("ess", 16, 512, 512, one(ESS), "an inflection"))
    E.append(CurveEntry("sub-pixel", 16, 256, 256, one([(100.25, 100.25), (100.5, 100.75), (100.75, 100.0), (100.9, 100.6)]),
                        "accepted at the root, one line per piece"))
    # --- 17: degenerate control polygons
    E.append(CurveEntry("p0=p1", 17, 512, 512, one([(60, 60), (60, 60), (400, 100), (300, 400)]), "vanishing start derivative"))
    E.append(CurveEntry("p2=p3", 17, 512, 512, one([(60, 400), (100, 100), (420, 300), (420, 300)]), "vanishing end derivative"))
    E.append(CurveEntry("p0=p1-p2=p3", 17, 512, 512, one([(50, 70), (50, 70), (450, 390), (450, 390)]),
                        "a straight line with both end derivatives zero"))
    E.append(CurveEntry("collinear-doubling-back", 17, 512, 512, one([(100, 100), (500, 200), (-100, 50), (300, 150)]),
                        "collinear control points: the curve doubles back on its own line, between its end points"))
    E.append(CurveEntry("collinear-overshoot", 17, 512, 512, one([(100, 100), (1000, 325), (-600, -75), (300, 150)]),
                        "collinear control points: the curve runs up to 88 px past its end points on its own line",
                        unbounded="both end tangents lie along the chord: th0 = th1 = 0 makes every term of flatten.wgsl's error "
                                  "measure zero, the root is accepted and becomes the one line p0 -> p3"))
    E.append(CurveEntry("all-equal", 17, 512, 512, [[((200, 200), [((200, 200), (200, 200), (200, 200))]),
                                                      (PLAIN[0], [tuple(PLAIN[1:])])]],
                        "a subpath whose four points are equal adds no line"))
    # --- 18: deep subdivision trees, full batches, long pieces
    E.append(CurveEntry("hairpin-4000", 18, 512, 512, one(HAIRPIN), "depth 9: the last level of the cooperative route"))
    E.append(CurveEntry("hairpin-1e5", 18, 512, 512, one(hairpin(1e5, -1e5)), "depth >= 10: the sequential walk"))
    E.append(CurveEntry("hairpin-1e6", 18, 512, 512, one(hairpin(1e6, -1e6)), "depth >= 13: the sequential walk"))
    E.append(CurveEntry("hairpins-64", 18, 512, 512, [one(hairpin(4000, -3000, float(i)))[0] for i in range(64)],
                        "more than 640 pieces from the 64 jobs of one batch: the piece list overflows"))
    E.append(CurveEntry("large-arc", 18, 512, 512, one([(0, 0), (0, 60000), (60000, 60000), (60000, 0)]),
                        "long pieces of up to 27 lines", tclass="large"))
    R, phi = 3e6, 0.3          # the arc's last 0.3 rad before its top at (256, 256)
    kk = 4.0 / 3.0 * math.tan(phi / 4) * R
    a0 = (256 - R * math.sin(phi), 256 + R - R * math.cos(phi))
    E.append(CurveEntry("clamped-arc", 18, 512, 512, one([a0, (a0[0] + kk * math.cos(phi), a0[1] - kk * math.sin(phi)), (256 - kk, 256), (256, 256)]),
                        "0.3 rad of a circle of radius 3e6: pieces at the clamp of 100 lines", tclass="large",
                        unbounded="a piece that needs more than 100 lines gets 100: their sagitta is whatever that gives"))
    # --- 19: quads, contours of several segments
    E.append(CurveEntry("quad", 19, 512, 512, [[((40, 60), [((300, 480), (470, 90))])]], "a quad, raised to a cubic in f32"))
    E.append(CurveEntry("quad-p1=p2", 19, 512, 512, [[((60, 60), [((400, 300), (400, 300))])]], "a quad whose end derivative vanishes"))
    E.append(CurveEntry("quad-hairpin", 19, 512, 512, [[((100, 100), [((5000, 115), (120, 130))])]], "a quad that turns back"))
    k = 0.6
    cx, cy, r = 250.5, 240.25, 180.0
    four = [((cx + r, cy), [((cx + r, cy + k * r), (cx + k * r, cy + r), (cx, cy + r)),
                            ((cx - k * r, cy + r), (cx - r, cy + k * r), (cx - r, cy)),
                            ((cx - r, cy - k * r), (cx - k * r, cy - r), (cx, cy - r)),
                            ((cx + k * r, cy - r), (cx + r, cy - k * r), (cx + r, cy))])]
    E.append(CurveEntry("four-cubics", 19, 512, 512, [four], "a closed contour: the last cubic ends on the start point, no closing line"))
    mixed = [((50, 60), [((200, 40),), ((330, 30), (420, 160)), ((500, 300), (300, 330), (380, 460)), ((120, 470),),
                         ((20, 400), (90, 250))])]
    E.append(CurveEntry("mixed", 19, 512, 512, [mixed], "lines, quads and cubics in one contour, closed by the encoder's line"))
    # --- 20: transforms and large coordinates
    E.append(CurveEntry("zoom-64", 20, 512, 512, one([(0.5, 0.5), (2.0, 6.0), (4.0, -1.0), (6.5, 5.5)]), "the transform in f32",
                        transform=(64.0, 0.0, 0.0, 64.0, 20.0, 30.0)))
    E.append(CurveEntry("zoom-3000", 20, 512, 512, one([(0.01, 0.01), (0.05, 0.12), (0.09, -0.02), (0.14, 0.11)]), "the transform in f32",
                        transform=(3000.0, 0.0, 0.0, 3000.0, 10.0, 90.0)))
    E.append(CurveEntry("large-3e4", 20, 512, 512, one([(-30000, 200), (100, -29000), (400, 31000), (30500, 300)]),
                        "absolute f32 coordinates near 3e4", tclass="large"))
    # --- 21: stroked cubics, butt caps (one segment: the bevel join is never drawn)
    for name, pts in (("plain", PLAIN), ("loop", LOOP), ("cusp", CUSP), ("ess", ESS), ("hairpin-4000", HAIRPIN)):
        for w in (0.3, 2.0, 20.0, 120.0):
            E.append(CurveEntry("stroke-%s-w%g" % (name, w), 21, 512, 512, one(pts), "the offset route of flatten_euler",
                                stroke=(w, "bevel", 4.0) + BUTT))
    # --- 22: joins between cubics, a round cap, strokes under transforms
    for join in ("miter", "round"):
        E.append(CurveEntry("stroke-smooth-%s" % join, 22, 512, 512, [[TWO_SMOOTH]], "cr = 0 at the join: it adds nothing visible",
                            stroke=(14.0, join, 4.0) + BUTT))
        E.append(CurveEntry("stroke-corner-%s" % join, 22, 512, 512, [[TWO_CORNER]], "a 90 degree corner between two cubics",
                            stroke=(14.0, join, 4.0) + BUTT))
    E.append(CurveEntry("stroke-round-caps", 22, 512, 512, one(PLAIN), "round caps on a cubic", stroke=(30.0, "bevel", 4.0, "round", "round")))
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    small = [(10, 10), (50, 100), (75, 5), (115, 75)]
    E.append(CurveEntry("stroke-similarity", 22, 512, 512, one(small), "scale = 3 in flatten_euler's offset route",
                        transform=(3 * c, 3 * s, -3 * s, 3 * c, 150.0, 40.0), stroke=(6.0, "bevel", 4.0) + BUTT))
    E.append(CurveEntry("stroke-anisotropic", 22, 512, 512, one(small), "flatten_euler's scale formula under an anisotropic transform",
                        transform=(4.0, 0.0, 1.0, 1.5, 20.0, 60.0), stroke=(6.0, "bevel", 4.0) + BUTT))
    return E


# Not in the battery: the forced acceptance at SUBDIV_LIMIT needs a tree of depth 16, which this family reaches at
# +-1e8.  There a line of the polyline crosses more than 65535 tiles, past the 16 bits path_count has for a crossing's
# index in its line, and everything after flatten is undefined (path_tiling reads tiles that nobody wrote).  Only the
# oracle's flatten stage runs it (tests/test_curve_spec.py).
SUBDIV_LIMIT_ENTRY = CurveEntry("hairpin-1e8", 18, 512, 512, one(hairpin(1e8, -1e8)),
                                "depth 16: pieces accepted at SUBDIV_LIMIT whatever their error",
                                unbounded="SUBDIV_LIMIT accepts a piece without an error test (and one f32 step is 8 px at 1e8)")
BATTERY = _battery()
STROKE_BATTERY = _stroke_battery()
CURVE_BATTERY = _curve_battery()
# these stroke entries are rendered again inside a viewport clip and with an opaque gradient
STROKE_VARIANT_ENTRIES = ["f11-L-miter-butt-square", "f12-triangle-round", "f14-leaves-all-sides"]
# family 10: these entries of families 1-5 are rendered again inside a viewport clip and with an opaque gradient
VARIANT_ENTRIES = ["f1-tile-lines", "f1-tile-lines-2^-10", "f1-viewport", "f2-left-shallow", "f2-left-only", "f2-cover-w2",
                   "f3-near-horizontal-one-tile-row", "f3-tile-corners", "f4-sliver-1e-4", "f5-star-7", "f5-zigzag-one-tile"]
BY_ID = {e.id: e for e in BATTERY + STROKE_BATTERY + CURVE_BATTERY}
