"""-m gpu: what a pixel of the HIP image is painted with, against the float64 reference of tests/exact_paint.py, on the
battery of tests/paint_cases.py: gradient ramps of 2 to 17 stops, every route of draw_leaf and fine for linear, radial
and sweep gradients in the three extend modes, images on both descriptor routes, over base colours, under partial
coverage, inside a layer and in MSAA8.  Every case is held at EVERY pixel that is not left out (below), and bit for bit
against the oracle; tests/test_paint_spec.py runs the same checks on the oracle and shows that thirteen near misses of
the rule fail them.

The check.  A gradient pixel is painted with the f16 ramp texel at round(extend(t) * 511); the device evaluates t in
f32, so the reference gives the SET of indices reachable within t +- delta (both ends where a wrap or fold lies
inside), and the stored pixel must equal fine's pixel rule for one index of the set within the store's bound.  An image
pixel has one expected paint with a bound of its own.  No margin is kept around wrap points.

Bounds, one term per source (fine.wgsl / draw_leaf.wgsl line numbers of the reference shaders; k_draw_leaf in
csrc/kernels_scan.hip and the paint commands of csrc/kernels_fine.hip perform the same f32 operations in the same
order).  Constants are roundings counted in units of 2^-24 times the largest intermediate; none is fitted.

  term          bound                                               source
  ramp texel    bit for bit                                         make_ramp (host/renderer.cpp): float64, rounded to
                                                                    f32 RTNE and to f16 with ties away from zero (the
                                                                    reference's gfx/color.go:11-25 through
                                                                    jmath.Float16bits; exact_paint.to_f16).  libm's
                                                                    pow and numpy's agree on every texel of the battery
  store         half an f16 ULP of the value                        the RGBA16F target, fine.wgsl:1100
  over          2^-24 * (3 c + 3 base) on a premultiplied           fine.wgsl:985-986 (and :1029-1030, 1063-1064,
                channel c: fg * area, bg * k and their sum are      1082-1083): fg_i = fg * area; rgba * (1 - fg_i.a) +
                each relative to a term <= c (3); fg.a * area       fg_i.  exact_paint.C_OVER_RESULT, C_OVER_BG
                and 1 - that scale the base, which the host
                premultiplied in f32 (3)
  division      (err c + v * err a) / a + 2 * 2^-24 * v for         fine.wgsl:1098-1099: a_inv = 1 / max(a, 1e-6);
                v = c / a: the errors above through the             rgb * a_inv.  exact_paint.C_DIV.  The division
                quotient, its own two roundings                     amplifies whatever c carries, the ramp texel's f16
                                                                    rounding included: hence the texel is rounded first
  layer         3 more on c and on the base, per layer              fine.wgsl:969-970 and blend.wgsl's src-over: rgba *
                                                                    area * alpha (2), bg * (1 - a) + src.  C_LAYER
  area          err(area) * (fg + base * fg.a)                      a rectangle with fractional edges: the "ident" bound
                                                                    of tests/test_gpu_coverage.py (area_tolerance),
                                                                    imported; 0 for the rectangles on pixel lines

delta of t, per class (exact_paint.gradient_paint):

  linear        24 * 2^-24 * (M / |p1' - p0'|) * (1 + |t|)          draw_leaf.wgsl:133-146: two transformed points (4
                M: the largest device coordinate of the points      each), their difference (1), dot (3), 1 / dot (1),
                or the target                                       the product (1), line_c (3); fine.wgsl:980-982: two
                                                                    products and two sums, f32(i)'s product and sum (6)
  radial        40 * 2^-24 * M * cond(T) * |grad t|_1               as a displacement of the pixel: draw_leaf.wgsl:157
                + 20 * 2^-24 * A * (|t| + |focal_x| + 1)            (inverse transform: 4 per coefficient, 7 per
                A = max(1, max(R^2, 1) / |R^2 - 1|), R the          translation), :272-277 (two_point_to_unit_line: the
                radius of draw_leaf.wgsl:194: the quotient by       same), :168-171 / :195-198 and :204-216 (two matrix
                R^2 - 1 of :209-212 scales x and y                  products, 3 + 5 each; the scale, 1), fine.wgsl:1003
                                                                    (4).  On t: focal_x (2), cf (4), its length (4),
                                                                    radius (1), 1 / radius (1), fine.wgsl:1006-1022 (6),
                                                                    :1025 focal_x + t_sign * t (2)
                |grad t|_1 is the float64 central difference of the definition (step 2^-10 px) at the pixel: it grows without
                bound where t is ill-conditioned -- the root of a difference near 0 (fine.wgsl:1012, 1021), the quotient by
                x of focal-on-circle (:1015), the focus -- so delta is per pixel there by construction
  nudge         2^-12 * scale * |grad t|_1 * max(1, |1 - t|)        draw_leaf.wgsl:178-181: a concentric gradient's p0
                                                                    is moved by (2^-12, 2^-12), c(t) by (1 - t) of it
  thresholds    0 for the battery                                   draw_leaf.wgsl:164 (strip: |r0 - r1| <= 2^-12) and
                                                                    :201 (focal on circle: |radius - 1| <= 2^-12): the
                                                                    cases sit on them exactly (r0 = r1, radius = 1) or
                                                                    64 thresholds away; exact_paint asserts it
  sweep         in turns: P + 12 * 2^-24                            P = 2.652e-5: the distance of the four-term
                + 16 * 2^-24 * M * cond(T) * sqrt 2 / (2 pi r),     polynomial of fine.wgsl:1054 from atan(s) / 2 pi
                times 1 / |t1 - t0|; on t: 6 * 2^-24 *              over s in [0, 1], measured by the test itself on a
                (1 + |t| + max(|t0|, |t1|) / |t1 - t0|)             grid of 2^16 steps (exact_paint.
                r: the pixel's device distance from the centre      sweep_polynomial_distance); fine.wgsl:1047-1057: the
                                                                    quotient, s, four Horner steps, two folds (12);
                                                                    draw_leaf.wgsl:230-243 and fine.wgsl:1040 (16);
                                                                    :1037, 1059 and t0, t1 as stored f32 (6)
  extend        4 * 2^-24 * (1 + |t|), every class                  fine.wgsl:800-812 and the product with 511
  image         u, v: 12 * 2^-24 * |row of T^-1|_1 * M *            draw_leaf.wgsl:244-255 (inverse transform, 4 + 4),
                (|ad| + |bc|) / |det|; the paint: the largest       fine.wgsl:1072 (4).  The bilinear sample is
                difference of the sample over (u, v) +- that,       continuous in (u, v), across texel lines too, and
                an integer u or v inside included, + 12 * 2^-24     fades to nothing at the cut, so the bound of (u, v)
                                                                    becomes one of the paint.  fine.wgsl:1077-1081:
                                                                    alpha / 255, the sRGB table's one rounding
                                                                    (csrc/srgb_lut.h), premultiply (3), two mixes of
                                                                    1 - t, two products and a sum (8)

Left out, never more than 2 % of a case's painted pixels (a condition on the case's inputs, which the reference alone
keeps: tests/test_paint_spec.py asserts the same shares without a GPU): a pixel whose delta * 511 exceeds 2 ramp steps
is not checked; a pixel within 2^-10 px of the boundary between valid and invalid t (fine.wgsl:1013-1022) may be painted
or untouched, as may an image pixel within its bound of u = width or v = height (where the two readings are the same
value anyway, so it still counts as checked).  "sweep-full-corner" puts the centre on a pixel corner and gives up that
one pixel.

Every case records its largest error as a share of its bound and its left-out share in the test's user properties
(paint_class, paint_max_share_of_bound, paint_left_out_share) and in its report section "paint" (shown with -rP), so
that the slack of every class can be read off a run.  An opaque gradient pixel is its texel exactly (share 0); a
translucent one comes within 0.999 of its bound, which is the f16 half ULP of the store."""
import numpy as np
import pytest

from jello_amd import Host

import kat_scenes as K
import paint_cases as C
from parity import compare

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in C.BATTERY])
def test_paint(engine, request, name):
    """One render through Engine: every buffer and the image bit for bit against the oracle (parity.compare), and the
    HIP image against the reference."""
    case = C.BY_NAME[name]
    out = compare(engine, case.scene(), case.params())
    rows = K.ramp_rows(Host().record(case.scene(), case.params())) if case.ramps() else None
    C.record(request, case, C.check_case(case, out["image"], rows))


def test_ramp_rows_above_the_retained_64(engine):
    """One frame with 70 gradients: load_grad reads ramp rows 64..69.  Bit for bit against the oracle, and every
    gradient's pixel at t = 1/4 is texel 128 of its own ramp."""
    stops_list = [C.cache_stops(i, 0) for i in range(70)]
    scene, params = C.cache_scene(stops_list)
    assert K.ramp_rows(Host().record(scene, params)).shape[0] == 70
    img = compare(engine, scene, params)["image"]
    for k, stops in enumerate(stops_list):
        x, y, want = C.cache_pixel(k, stops)
        assert [int(v) for v in img[y, x]] == want, "gradient %d" % k
