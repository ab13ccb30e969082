"""A deterministic battery of hostile fill geometry for the exact-coverage checks (tests/test_coverage_spec.py on the
oracle, tests/test_gpu_coverage.py on the HIP image).  Every entry is one opaque white fill (or one stroked line
segment, whose outline is an exact rectangle) on a transparent base, in both fill rules, together with the float64
contours that tests/exact_coverage.py integrates and a tolerance class:

* "ident"  -- identity transform, f32-exact coordinates (entries about rounding say so);
* "large"  -- vertices at +-2^12 ... +-2^16: path_tiling's intersection formulas run on absolute f32 coordinates;
* "xform"  -- a non-identity transform, applied by flatten in f32 (the reference applies it in float64 to the same
  f32 inputs);
* "stroke" -- the outline is computed by the stroker in f32.

Families (the `family` field): 1 rectangles on and near pixel / tile lines, 2 geometry outside the viewport,
3 near-horizontal / near-vertical / corner-crossing edges, 4 degenerate contours, 5 winding other than +-1, 6 large
coordinates, 7 transforms, 8 stroked segments, 9 target sizes, 10 the same expected alpha through the CLIPS and PAINTS
instantiations of fine (see `variants`)."""
import math

import numpy as np

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


BATTERY = _battery()
# family 10: these entries of families 1-5 are rendered again inside a viewport clip and with an opaque gradient
VARIANT_ENTRIES = ["f1-tile-lines", "f1-tile-lines-2^-10", "f1-viewport", "f2-left-shallow", "f2-left-only", "f2-cover-w2",
                   "f3-near-horizontal-one-tile-row", "f3-tile-corners", "f4-sliver-1e-4", "f5-star-7", "f5-zigzag-one-tile"]
BY_ID = {e.id: e for e in BATTERY}
