"""The battery of tests/test_paint_spec.py (oracle) and tests/test_gpu_paint.py (HIP image): what a pixel is painted
with, against tests/exact_paint.py.  Targets are at most 64 x 48; the largest are no multiple of 16 wide or high where
that matters (60 x 44), so they cross tile seams and the 4-pixel strips of a lane.  Every case names what it is there for.

A case is a list of draws on one base colour.  A draw fills a rectangle on pixel lines (its area is exactly 1 inside
and 0 outside, in every AA mode), so that everything a pixel shows is its paint; the draws of a case do not overlap.
`frac` cases fill one rectangle with fractional edges instead: the area then is tests/exact_coverage.py's, held with
the "ident" bound of tests/test_gpu_coverage.py.

Left out: p0 = p1 for a linear gradient and t0 = t1 for a sweep.  Both are divisions by zero whose result the
definitions do not give (the encoder turns the second into a transparent colour); oracle parity keeps covering them."""
import math

import numpy as np

import exact_coverage as X
import exact_paint as P
from coverage_scenes import Entry, rect as rect_contour

from jello_amd import Aa, Brush, ColorStop, Compose, Extend, Fill, Mix, Path, RenderParams, Scene

INLINE_IMAGES = 8       # JH_FINE_INLINE_IMAGES of jello_amd/csrc/kcommon.h: more images than this take the table route
KNEE = 0.0031308

# ---- ramps -----------------------------------------------------------------------------------------------------------
RAMPS = {
    "2-opaque": [(0.0, (1, 0, 0, 1)), (1.0, (0, 0, 1, 1))],
    "2-alpha0-end": [(0.0, (1, 0.5, 0, 0)), (1.0, (0, 0.25, 1, 0.75))],
    "3-knee": [(0.0, (0, 0, 0, 1)), (0.5, (KNEE, 1, KNEE, 1)), (1.0, (1, 1, 1, 1))],
    "3-translucent": [(0.0, (1, 1, 0, 0.25)), (0.5, (0, 1, 1, 1.0)), (1.0, (1, 0, 1, 0.5))],
    # first stop > 0, a hard stop (two stops at 0.35: a 0-sample segment), last stop < 1
    "4-hard-stop": [(0.1, (1, 0.2, 0, 0.9)), (0.35, (0, 1, 0.3, 0.4)), (0.35, (0.1, 0, 1, 1.0)), (0.8, (1, 1, 0.5, 0.6))],
    # 512 * 0.2509765625 = 128.5: a tie, rounded away from zero
    "5-opaque": [(0.0, (1, 0, 0, 1)), (0.25, (0, 1, 0, 1)), (0.5, (0, 0, 1, 1)), (0.5 + 257.0 / 1024, (1, 1, 0, 1)), (1.0, (0, 1, 1, 1))],
    "5-translucent": [(0.0, (1, 0, 0, 0.5)), (0.2, (0, 1, 0, 1)), (0.45, (0, 0, 1, 0.25)), (0.7, (1, 1, 0, 0.75)), (1.0, (0, 1, 1, 0))],
    # 129/1024 (64.5 samples: a tie), then a segment narrower than 1/512 (0.25 sample: none), then one of exactly 1/512
    "6-narrow": [(0.0, (1, 0, 0, 1)), (129.0 / 1024, (0, 1, 0, 1)), (129.0 / 1024 + 1.0 / 2048, (1, 1, 1, 1)),
                 (129.0 / 1024 + 1.0 / 2048 + 1.0 / 512, (0, 0, 1, 0.5)), (0.6, (1, 1, 0, 1)), (1.0, (0, 0, 0, 1))],
    "17-opaque": [(k / 16.0, ((k % 3) / 2.0, ((k * 5) % 7) / 6.0, ((k * 3) % 4) / 3.0, 1.0)) for k in range(17)],
    "17-translucent": [(k / 16.0, (((k * 2) % 5) / 4.0, (k % 2) * 1.0, ((k * 3) % 7) / 6.0, ((k * 7) % 9) / 8.0)) for k in range(17)],
}


# ---- images: sRGB texels with alpha 0, 128 and 255 next to one another ------------------------------------------------
def _image(w, h, seed):
    r = np.random.RandomState(seed)
    px = r.randint(0, 256, (h, w, 4)).astype(np.uint8)
    px[..., 3] = np.array([255, 128, 0])[(np.arange(h)[:, None] * 2 + np.arange(w)[None, :] + seed) % 3]
    return px


IMAGES = {"1x1": _image(1, 1, 0), "2x2": _image(2, 2, 1), "4x4": _image(4, 4, 2), "5x3": _image(5, 3, 3)}
IMAGES["1x1"][0, 0, 3] = 128


class Draw:
    def __init__(self, kind, rect, path_transform=None, brush_transform=None, **kw):
        self.kind, self.rect, self.path_transform, self.brush_transform = kind, rect, path_transform, brush_transform
        self.extend = int(kw.pop("extend", P.PAD))
        self.srgb = True
        self.__dict__.update(kw)
        if kind != "image":
            self.stops = RAMPS[self.ramp]
        t = path_transform
        if brush_transform is not None:
            t = brush_transform if t is None else P.affine_mul(t, brush_transform)
        self.transform = t      # float64; the encoder stores it as f32

    def brush(self):
        if self.kind == "image":
            return Brush.image(self.pixels)
        stops = [ColorStop(o, c) for o, c in self.stops]
        ext = Extend(self.extend)
        if self.kind == "linear":
            return Brush.linear(tuple(self.p0), tuple(self.p1), stops, ext)
        if self.kind == "radial":
            return Brush.radial(tuple(self.p0), self.r0, tuple(self.p1), self.r1, stops, ext)
        return Brush.sweep(tuple(self.p0), self.t0, self.t1, stops, ext)


class Case:
    def __init__(self, name, why, width, height, draws, base=(0, 0, 0, 0), layer_alpha=None, aa="area", frac=None):
        self.name, self.why, self.width, self.height, self.draws = name, why, width, height, draws
        self.base, self.layer_alpha, self.aa, self.frac = base, layer_alpha, aa, frac
        assert width <= 64 and height <= 48

    def device_rect(self, d):
        x0, y0, x1, y1 = d.rect
        if d.path_transform is not None:
            a, b, c, dd, e, f = d.path_transform
            assert b == 0 and c == 0, "path transforms of the battery keep the rectangle axis-aligned"
            x0, x1 = sorted((a * x0 + e, a * x1 + e))
            y0, y1 = sorted((dd * y0 + f, dd * y1 + f))
        return x0, y0, x1, y1

    def area(self, d):
        """(area, bound of its error) of draw d, (H, W) each."""
        W, H = self.width, self.height
        x0, y0, x1, y1 = self.device_rect(d)
        if self.frac:
            from test_gpu_coverage import area_tolerance     # the "ident" bound: imported, not copied
            e = Entry(self.name, 0, W, H, [rect_contour(x0, y0, x1, y1)])
            area = X.area_alpha(X.area_acc(e.reference_contours(), W, H), "nonzero")
            return area, area_tolerance(e, area)
        # on pixel lines, or beyond the target: area 1 inside, 0 outside, exactly
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        assert all(float(v).is_integer() for v in (cx0, cy0, cx1, cy1)), (self.name, d.rect)
        area = np.zeros((H, W))
        area[int(cy0):int(cy1), int(cx0):int(cx1)] = 1.0
        return area, np.zeros((H, W))

    def scene(self):
        s = Scene()
        if self.layer_alpha is not None:
            s.push_layer(Mix.Normal, Compose.SrcOver, self.layer_alpha, None, Path.rect(0, 0, self.width, self.height))
        for d in self.draws:
            s.fill(Fill.NonZero, d.path_transform, d.brush(), d.brush_transform, Path.rect(*d.rect))
        if self.layer_alpha is not None:
            s.pop_layer()
        return s

    def params(self):
        return RenderParams(self.width, self.height, base_color=self.base, aa={"area": Aa.Area, "msaa8": Aa.Msaa8}[self.aa])

    def ramps(self):
        out = []
        for d in self.draws:
            if d.kind != "image" and d.ramp not in out:
                out.append(d.ramp)
        return out


def bands(width, height, n):
    """n rectangles on pixel lines that tile the target from top to bottom; the seams are not on tile lines."""
    ys = [int(round(i * height / n)) for i in range(n + 1)]
    return [(0, ys[i], width, ys[i + 1]) for i in range(n)]


def three_extends(kind, width, height, **kw):
    return [Draw(kind, r, extend=e, **kw) for r, e in zip(bands(width, height, 3), (P.PAD, P.REPEAT, P.REFLECT))]


def rot(deg, s=1.0, tx=0.0, ty=0.0):
    c, sn = s * math.cos(math.radians(deg)), s * math.sin(math.radians(deg))
    return (c, sn, -sn, c, tx, ty)


def _battery():
    B = []
    W, H = 60, 44
    FULL = (0, 0, W, H)
    add = lambda *a, **k: B.append(Case(*a, **k))
    # ---- ramps ----
    add("ramp-rows", "three different ramps and a repeated one: rows 0-2, the repeat shares row 0", W, H,
        [Draw("linear", r, p0=(2.5, 0), p1=(57.25, 0), ramp=n) for r, n in zip(bands(W, H, 4), ("2-opaque", "6-narrow", "17-opaque", "2-opaque"))])
    add("ramp-translucent-rows", "translucent ramps of 2, 3, 5 and 17 stops, alpha 0 at an end", W, H,
        [Draw("linear", r, p0=(1.0, 0), p1=(59.0, 3.0), ramp=n) for r, n in
         zip(bands(W, H, 4), ("2-alpha0-end", "3-translucent", "5-translucent", "17-translucent"))])
    add("ramp-knee-5", "colours at 0, the sRGB knee and 1; the five-stop ramp with a tie in its counts", W, H,
        [Draw("linear", r, p0=(0.0, 0), p1=(60.0, 0), ramp=n) for r, n in zip(bands(W, H, 2), ("3-knee", "5-opaque"))])
    # ---- linear ----
    add("linear-axis", "axis-aligned, p0 and p1 fractional, wrap points inside, all extends", W, H,
        three_extends("linear", W, H, p0=(10.5, 0), p1=(30.25, 0), ramp="2-opaque"))
    add("linear-hard-stop", "the four-stop translucent ramp with a hard stop, diagonal, all extends", 40, 20,
        three_extends("linear", 40, 20, p0=(5.3, 7.7), p1=(21.9, 14.1), ramp="4-hard-stop"))
    add("linear-vertical", "along y: every lane of a row reads one texel", W, H,
        three_extends("linear", W, H, p0=(0, 3.75), p1=(0, 17.5), ramp="3-translucent"))
    add("linear-similarity", "a rotation and uniform scale as brush transform", W, H,
        three_extends("linear", W, H, p0=(0, 0), p1=(20, 10), ramp="5-translucent", brush_transform=rot(23.0, 1.3, 12.5, 6.25)))
    add("linear-path-transform", "a path transform (scale 1.5, translation): it moves the gradient with the path", W, H,
        [Draw("linear", (-10, -10, 50, 40), path_transform=(1.5, 0, 0, 1.5, 3.0, 2.0), p0=(2.5, 1.0), p1=(22.0, 14.0), ramp="4-hard-stop",
              extend=P.REFLECT)])
    # ---- radial: one case per route of draw_leaf and fine ----
    geoms = {
        "concentric": ((30.5, 22.25), 4.0, (30.5, 22.25), 15.0),
        "inside": ((24, 20), 3.0, (30, 23), 16.0),
        "cone": ((12, 14), 3.0, (40, 28), 7.0),
    }
    whys = {"concentric": "kind circular: the shifted centre", "inside": "start circle inside the end circle: radius > 1",
            "cone": "neither circle inside the other: radius < 1, with an unpainted region"}
    for k, (c0, r0, c1, r1) in geoms.items():
        add("radial-" + k, whys[k] + ", all extends", W, H, three_extends("radial", W, H, p0=c0, r0=r0, p1=c1, r1=r1, ramp="3-translucent"))
    one = lambda name, why, c0, r0, c1, r1, **kw: add("radial-" + name, why, W, H, [Draw("radial", FULL, p0=c0, r0=r0, p1=c1, r1=r1,
                                                                                     ramp=kw.pop("ramp", "2-opaque"), **kw)])
    one("strip", "r0 = r1: kind strip", (14, 24), 8.0, (48, 24.5), 8.0)
    one("focal-on-circle", "r0 = 0 with the focus on the end circle (between two pixel columns: t = (x^2 + y^2) / x has its pole there)",
        (15.5, 24), 0.0, (31.5, 24), 16.0)
    one("focal-inside", "r0 = 0 with the focus inside the end circle", (28, 22), 0.0, (34, 24), 28.0, ramp="5-translucent")
    one("swapped", "r1 = 0: points and radii swapped, 1 - t", (30, 24), 26.0, (36, 20), 0.0)
    one("r0-gt-r1", "r0 > r1: focal_x > 1, t_sign = -1", (32, 24), 30.0, (36, 26), 6.0, ramp="4-hard-stop")
    one("anisotropic", "an anisotropic brush transform: the inverse transform", (5, 10), 4.0, (15, 20), 30.0,
        brush_transform=(1.5 * math.cos(0.4), 1.5 * math.sin(0.4), -0.8 * math.sin(0.4), 0.8 * math.cos(0.4), 20.0, 4.0), ramp="3-translucent")
    # ---- sweep ----
    add("sweep-full-corner", "a full turn, its centre on a pixel corner: that one pixel is given up (the angle of a zero vector; the shader's 0 / 0 "
        "becomes phi = 0 through its NaN test); those around it are held through their own delta, which grows as 1 / r", W, H,
        three_extends("sweep", W, H, p0=(32, 24), t0=0.0, t1=2 * math.pi, ramp="17-opaque"))
    add("sweep-arc", "an arc 0.5 -> 4.0 rad, centre off the pixel grid, all extends", W, H,
        three_extends("sweep", W, H, p0=(30.4, 21.7), t0=0.5, t1=4.0, ramp="3-translucent"))
    add("sweep-reflection", "a brush transform with a reflection: the sweep turns the other way", W, H,
        [Draw("sweep", FULL, p0=(0.3, -0.2), t0=0.5, t1=4.0, ramp="5-opaque", extend=P.REPEAT, brush_transform=(-1.25, 0, 0, 1.25, 28.0, 25.0))])
    # ---- images ----
    im = lambda name, r, bt: Draw("image", r, pixels=IMAGES[name], brush_transform=bt)
    add("image-integer", "integer placement: the pixel is the texel", 16, 12, [im("5x3", (0, 0, 16, 12), (1, 0, 0, 1, 3, 2))])
    add("image-1x1", "one texel, translated by (0.25, 0.5)", 16, 12, [im("1x1", (0, 0, 16, 12), (1, 0, 0, 1, 3.25, 2.5))])
    add("image-translated", "translated by (0.25, 0.5); ends inside the fill on all four sides", 16, 12,
        [im("4x4", (0, 0, 16, 12), (1, 0, 0, 1, 5.25, 3.5))])
    add("image-scaled", "scaled 2.5 x; ends inside the fill on all four sides", 28, 20, [im("5x3", (0, 0, 28, 20), (2.5, 0, 0, 2.5, 6.5, 5.25))])
    add("image-rotated", "rotated 30 degrees and scaled 3 x", 28, 24, [im("4x4", (0, 0, 28, 24), rot(30.0, 3.0, 12.0, 3.0))])
    add("image-flipped", "flipped in x and scaled", 20, 12, [im("2x2", (0, 0, 20, 12), (-3.0, 0, 0, 2.0, 14.0, 4.0))])
    add("image-two", "two images in a scene, and the first once more (one atlas entry)", 24, 18,
        [im(n, r, (2.0, 0, 0, 2.0, 3.5, r[1] + 0.25)) for n, r in zip(("4x4", "5x3", "4x4"), bands(24, 18, 3))])
    nine = [_image(3, 2, 10 + i) for i in range(INLINE_IMAGES + 1)]
    add("image-table", "JH_FINE_INLINE_IMAGES + 1 images: the table route", 36, 9,
        [Draw("image", (4 * i, 0, 4 * i + 4, 9), pixels=nine[i], brush_transform=(1, 0, 0, 2.0, 4 * i + 0.5, 1.5)) for i in range(INLINE_IMAGES + 1)])
    # ---- with coverage and layers ----
    grad = lambda r: Draw("linear", r, p0=(3.5, 2.0), p1=(25.0, 12.0), ramp="4-hard-stop", extend=P.REFLECT)
    img = lambda r: im("5x3", r, (2.5, 0, 0, 2.5, 4.5, r[1] + 1.25))
    two = lambda w, h: [grad(bands(w, h, 2)[0]), img(bands(w, h, 2)[1])]
    add("over-opaque-base", "a gradient and an image over an opaque base colour", 28, 24, two(28, 24), base=(0.25, 0.5, 0.75, 1.0))
    add("over-translucent-base", "a gradient and an image over a translucent base colour", 28, 24, two(28, 24), base=(0.5, 0.25, 0.125, 0.5))
    add("frac-gradient", "a gradient under a rectangle with fractional edges", 28, 20,
        [Draw("linear", (2.5, 3.25, 24.75, 17.5), p0=(3.5, 2.0), p1=(25.0, 12.0), ramp="5-translucent")], base=(0.25, 0.5, 0.75, 1.0), frac=True)
    add("frac-image", "an image under a rectangle with fractional edges", 28, 20,
        [Draw("image", (2.5, 3.25, 24.75, 17.5), pixels=IMAGES["5x3"], brush_transform=(4.0, 0, 0, 4.0, 4.5, 4.25))], base=(0.5, 0.25, 0.125, 0.5),
        frac=True)
    add("layer-half", "a gradient and an image inside a push_layer with alpha 0.5", 28, 24, two(28, 24), base=(0.25, 0.5, 0.75, 1.0), layer_alpha=0.5)
    # ---- MSAA8: the paint does not depend on the AA mode ----
    add("msaa8-linear", "MSAA8: the four-stop ramp, all extends", 40, 20,
        three_extends("linear", 40, 20, p0=(5.3, 7.7), p1=(21.9, 14.1), ramp="4-hard-stop"), aa="msaa8")
    add("msaa8-radial", "MSAA8: the cone with its unpainted region", W, H,
        [Draw("radial", FULL, p0=(12, 14), r0=3.0, p1=(40, 28), r1=7.0, ramp="3-translucent")], aa="msaa8")
    add("msaa8-image", "MSAA8: a scaled image over a translucent base", 28, 20, [im("5x3", (0, 0, 28, 20), (2.5, 0, 0, 2.5, 6.5, 5.25))],
        base=(0.5, 0.25, 0.125, 0.5), aa="msaa8")
    return B


BATTERY = _battery()
BY_NAME = {c.name: c for c in BATTERY}
assert len(BY_NAME) == len(BATTERY)


def stops_of(name):
    return RAMPS[name]


# ---- shared by the CPU and the GPU test --------------------------------------------------------------------------------
LEFT_OUT_MAX = 0.02     # of a case's painted pixels: a condition on the case's inputs, kept by the reference alone


def paint_class(case):
    kinds = sorted({d.kind for d in case.draws})
    return "+".join(kinds) + ("/" + case.aa if case.aa != "area" else "")


def check_case(case, img16, rows=None):
    """img16: (H, W, 4) f16 bit patterns of the rendered case; rows: the uploaded ramp image (f16 bit patterns) or None.
    Asserts the ramps bit for bit and every pixel that is not left out within its bound; returns check_image's dict."""
    names = case.ramps()
    if names:
        assert rows is not None and rows.shape[0] == len(names), "%s: %d ramp rows for %d ramps" % (case.name, len(rows), len(names))
        for i, n in enumerate(names):
            want = P.ramp(RAMPS[n])[1].view(np.uint16)
            diff = np.argwhere(rows[i] != want)
            assert len(diff) == 0, "%s: ramp %s (row %d) differs in %d values; first texel %d channel %d: 0x%04x, by the rule 0x%04x" % (
                case.name, n, i, len(diff), diff[0][0], diff[0][1], rows[i][tuple(diff[0])], want[tuple(diff[0])])
    img = img16.view(np.float16).astype(np.float64)
    r = P.check_image(case, img)
    if r["bad"].any():
        ys, xs = np.nonzero(r["bad"])
        k = int(np.argmax(r["ratio"][ys, xs]))
        raise AssertionError("%s: %d pixel(s) out of bound; worst (x=%d, y=%d): %s, %.3g of the bound" %
                             (case.name, len(ys), xs[k], ys[k], img[ys[k], xs[k]], r["ratio"][ys[k], xs[k]]))
    assert r["left_out"] <= LEFT_OUT_MAX, "%s: %.2f %% of the painted pixels left out" % (case.name, 100 * r["left_out"])
    return r


def record(request, case, r):
    """The largest error as a share of its bound and the left-out share, for the per-class maxima of a run (-rP)."""
    request.node.user_properties.append(("paint_class", paint_class(case)))
    request.node.user_properties.append(("paint_max_share_of_bound", "%.3g" % r["share"]))
    request.node.user_properties.append(("paint_left_out_share", "%.4f" % r["left_out"]))
    request.node.add_report_section("call", "paint", "class %s, %s: at most %.3g of the bound, %.2f %% of the painted pixels left out" %
                                    (paint_class(case), case.name, r["share"], 100 * r["left_out"]))


# ---- the ramp cache: many small gradients in one frame -------------------------------------------------------------------
COLS, ROWS, CELL = 10, 7, 4


def cache_stops(i, frame):
    a = ((i % 5) / 4.0, ((i * 3 + frame) % 7) / 6.0, ((i + 2 * frame) % 11) / 10.0, 1.0)
    b = (((i + frame) % 3) / 2.0, ((i * 5) % 9) / 8.0, ((i * 7 + frame) % 13) / 12.0, 1.0)
    return [(0.0, a), (1.0, b)]


def cache_scene(stops_list):
    s = Scene()
    for k, stops in enumerate(stops_list):
        x0, y0 = CELL * (k % COLS), CELL * (k // COLS)
        s.fill(Fill.NonZero, None, Brush.linear((x0, 0), (x0 + CELL, 0), [ColorStop(o, c) for o, c in stops]), None,
               Path.rect(x0, y0, x0 + CELL, y0 + CELL))
    return s, RenderParams(COLS * CELL, ROWS * CELL)


def cache_pixel(k, stops):
    """(x, y, the four f16 bit patterns) of the pixel of gradient k at t = 1/4: texel round(511 / 4) = 128 of its ramp
    (opaque over a transparent base: the pixel is the texel)."""
    want = P.ramp(stops)[1].view(np.uint16)[128]
    return CELL * (k % COLS) + 1, CELL * (k // COLS) + 1, [int(v) for v in want]
