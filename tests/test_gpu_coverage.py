"""-m gpu: per-pixel fill coverage of the HIP image against the exact float64 reference of tests/exact_coverage.py, on
the battery of tests/coverage_scenes.py, in all three AA modes.  Area AA is held at EVERY pixel (max, no percentile)
to a bound derived term by term below; MSAA8 / MSAA16 to the exact sample count, except for the k samples of a pixel
that lie within msaa_delta of an edge.  tests/test_coverage_spec.py runs the same checks on the oracle.

Area tolerance of a pixel, one term per source (fine.wgsl / path_tiling.wgsl line numbers of the reference shaders):

  term        per             bound                                   source
  f16 store   pixel           half an f16 ULP of the value            the RGBA16F target
  clamp       edge within     1e-3 for every pixel of the tile        path_tiling.wgsl:99,105,114,120: xt / yt are
              1e-3 of the                                             clamped to tile_xy + 1e-3.  :99 (top edge) and
              tile's top-                                             :114 (bottom edge) move an x crossing within 1e-3
              left, top-                                              of the left corners, :105 / :120 a y crossing
              right or                                                within 1e-3 of the top corners (a vertical edge
              bottom-left                                             on a tile column reads 0.999 in every tile row
              corner                                                  after its first)
  nudges      edge in the     2e-6                                    path_tiling.wgsl:129-164 (EPSILON = 1e-6 on
              row, tile                                               p.x), fine.wgsl:851 (xmin - 1e-6)
  f32         edge in the     C_F32 * 2^-24 * max|coordinate|         path_tiling.wgsl:99-120 intersections on absolute
              row, tile                                               f32 coordinates; flatten's transform (classes
              (to the left)                                           "xform", "large") and stroker ("stroke")
  cancel      piece of edge   2^-24 * (2 m^2 + 2 m) / (w + 1e-6) * h  fine.wgsl:851-856: a = (b + (d^2 - c^2) / 2 -
              in the pixel    (m: the piece's largest x inside the    xmin) / (xmax - xmin).  The roundings of d*d, c*c
                              pixel, w / h: its width / height)       (<= 2^-24 m^2 each) and of b + ... (<= 2^-24 m)
                                                                      are divided by xmax - xmin, which is 1e-6 for a
                                                                      vertical edge: up to 0.16 at x = 0.75 (measured
                                                                      0.044).  m = 0 for an edge on a pixel line: the
                                                                      nudge of path_tiling.wgsl:159-164 puts it at
                                                                      k - 1e-6, where the formula is exact, as it is
                                                                      in every pixel left or right of a piece (test_
                                                                      coverage_spec.test_fine_area_formula_...)

  arc         line of an      (n - 1) * r * (5 * 2^-24 + dtheta),     flatten.wgsl:490-517: vertex i of an arc of n
              arc, added to   dtheta = 2^-24 * (1 / sin(theta / 2)    lines is the begin point rotated i <= n - 1 times
              f32 for that    + 3 theta), r the largest device        in f32.  One step rounds two products and a sum
              line alone      distance of a vertex from the centre    per component (<= 2^-24 r (1 + 1 + sqrt 2)) with
                                                                      cs, sn rounded once each (<= 2^-24 r sqrt 2): 5.
                                                                      theta = 2 acos(1 - 0.25 / radius): the rounding of
                                                                      1 - x (<= 2^-25) is divided by sin(theta / 2) and
                                                                      doubled, acos and the radius round once more
                                                                      (<= 3 * 2^-24 theta); step i is off by i dtheta.
                                                                      Linear in n: 1.3e-4 px for a cap of radius 20
                                                                      (10 lines), 0.11 for the 61 lines of radius 735

The f32 constant per class, in units of 2^-24 * max|coordinate| (device pixels, at least the target's size):

  class          C_F32     roundings counted
  ident          4         path_tiling's intersection: a difference, a quotient, a product, a sum
  large, xform   8         the same, and the transform's two products and two sums per coordinate
  stroke         16        the tangent's difference, its normalisation (square, sum, root, quotient), the product with
                           w / 2 and the sum with the point, for both ends of a line; for the miter point the difference
                           of the two offset points, the cross product, the quotient by cr and the final product and
                           difference.  The quotient by cr does not amplify: it moves the miter point ALONG the next
                           edge by err / |cr|, which moves the previous edge across by err (the cross product again).
  stroke-xform   16 * |T| * max|local coordinate| + 8 * max|device coordinate|: the normal and the miter point are
                           computed in f32 in LOCAL space, and that error is stretched by the transform (|T|: the
                           larger absolute row sum of its linear part, errors being bounded per coordinate); then the
                           f32 transform of the outline points as in class "xform".  At a 40x zoom of local
                           coordinates near 2 both parts are about the same; at a 1/8 shrink of coordinates near 2000
                           the local part is twice the device part.

"edge in the row, tile" counts the distinct edges that touch the pixel's row inside its tile at or left of the pixel
(a moved crossing changes the cover of everything right of it in the tile).  For the identity classes the bound of a
pixel crossed by one edge away from tile corners is about 2.4e-4 + 1e-5; next to a tile corner it is near 1.3e-3 per
edge (2e-3 for the two edges of a rectangle corner).  Only pieces that are nearly vertical and sit at a fractional x
inside their pixel get a cancellation term above 2e-4: 1e-3 of width already brings it below 1.2e-4 * h.

MSAA: delta (exact_coverage.msaa_delta) = 0.0558 px for 8 samples, 0.0286 px for 16 (LUT quantisation + the 1e-3 clamp),
plus the f32 term above (and the arc term around the lines of an arc).  Counts k / S are exact in f16.  The band is
measured from the edge's LINE in every pixel the edge has a piece in, and from the edge itself in the pixels around
them: fine classifies the samples of such a pixel against the LUT line and cuts an edge that ends inside it by sample
row only, so a sample past the end point of a near-horizontal edge but within delta of its line can be misread like
any other sample near it (exact_coverage.near_mask; found by f3-near-vertical-cap-end).

Section-5 allowance (GPU = oracle != reference, explained by the WGSL): fill_path_ms_evenodd sets is_bump = xy0.x == 0
for the first pixel of a segment (fine.wgsl:623) without the `y0i != xy0.y` test of fill_path_ms (fine.wgsl:282),
and also flips the row parity through y_edge (fine.wgsl:539-552) and sets is_delta (fine.wgsl:622).  A segment that
enters a tile through its left edge exactly on a pixel row line is therefore counted twice in the pixel it enters:
y_edge already flips the parity of that row from the tile's left edge on, and the bump flips every sample of the pixel
once more (the delta for the pixels right of it is cancelled by the y_edge flip, as in fill_path_ms).  Whether the f32
crossing lands exactly on the row line, and whether the tile's piece then is a horizontal line that fine skips, is
decided by f32 roundings that the reference does not model.  So in those pixels of the entries in
EVENODD_MSAA_ROW_FLIP (even-odd MSAA only) the alpha is held to the exact value or to its complement 1 - exact, with
the same k / S band: every sample is still checked, and only the one parity flip of the double count is allowed.

Every render records its largest error (k = 0 pixels for MSAA) and its class in the test's user properties
(coverage_class, coverage_max_error, coverage_max_share_of_bound) and in its report section "coverage" (shown with
-rP), so that the slack of every class can be read off a run.
"""
import numpy as np
import pytest

from jello_amd import Aa, Host
from jello_amd.engine import RUN_DISPATCHES, RUN_UPLOADS

import coverage_scenes as C
import exact_coverage as X

pytestmark = pytest.mark.gpu

C_F32 = {"ident": 4.0, "large": 8.0, "xform": 8.0, "stroke": 16.0}
ROTATION = 5.0      # roundings of one rotation step of flatten_arc, per component, in units of 2^-24 * radius
NUDGE = 2e-6
CANCEL = 2.0 ** -24
DELTA = {8: X.msaa_delta(8), 16: X.msaa_delta(16)}
AAS = {"area": Aa.Area, "msaa8": Aa.Msaa8, "msaa16": Aa.Msaa16}
# even-odd MSAA entries with an edge that enters a tile through its left side exactly on a pixel row line (see above)
EVENODD_MSAA_ROW_FLIP = {
    "f2-shallow-through-box",           # caught it: (-300, 20)-(400, 27) enters tile column 0 at y = 23.0
    "f3-near-horizontal-one-tile-row",  # y = 43 + 6e-7 rounds to 43.0 in f32 at x = 0
    "f3-near-horizontal-each",          # the closing edge crosses x = 48 at y = 10.0
}


def f16_half_ulp(v):
    v = np.maximum(np.abs(v), 2.0 ** -14)
    return 0.5 * 2.0 ** (np.floor(np.log2(v)) - 10)


def _edges(entry):
    e = X.edges_of(entry.reference_contours())
    return e[(e[:, 0] != e[:, 2]) | (e[:, 1] != e[:, 3])]


def f32_term(entry):
    if entry.tclass == "stroke-xform":
        return 2.0 ** -24 * (C_F32["stroke"] * entry.transform_norm() * entry.max_local_coordinate() +
                             C_F32["xform"] * entry.max_coordinate())
    return C_F32[entry.tclass] * 2.0 ** -24 * entry.max_coordinate()


def arc_term(arc):
    """The distance by which the f32 vertices of one arc may leave their float64 positions, beyond f32_term (table
    above, row "arc"): vertex i is rotated i <= n - 1 times."""
    r = float(np.hypot(*(arc.device - arc.centre).T).max())     # no vertex is farther from the centre than this
    dtheta = 2.0 ** -24 * (1.0 / np.sin(0.5 * arc.theta) + 3.0 * arc.theta)
    return (arc.n - 1) * r * (ROTATION * 2.0 ** -24 + dtheta)


def edge_extra(entry):
    """Per edge of _edges(entry): what its end points may be off by beyond f32_term(entry) (the lines of arcs only)."""
    e = X.edges_of(entry.reference_contours())
    extra = np.zeros(len(e))
    for i, arc in (entry.arc_edges() if hasattr(entry, "arc_edges") else ()):
        extra[i] = max(extra[i], arc_term(arc))
    return extra[(e[:, 0] != e[:, 2]) | (e[:, 1] != e[:, 3])]


def area_tolerance(entry, value):
    """(height, width) bound of |alpha - exact| for area AA (table above)."""
    W, H = entry.width, entry.height
    e = _edges(entry)
    tol = f16_half_ulp(value)
    if len(e) == 0:
        return tol
    xa, ya, xb, yb, col, row, i = X._pieces(e, W, H)
    ok = (row >= 0) & (row < H) & (col < W)
    colc = np.maximum(col, 0)
    # distinct edges per (row, tile column) at or left of each pixel
    tx = colc // 16
    key, first = np.unique(((row[ok] * 4096 + tx[ok]) * len(e) + i[ok]), return_index=True)
    mincol = np.full(key.shape, W, np.int64)
    np.minimum.at(mincol, np.searchsorted(key, (row[ok] * 4096 + tx[ok]) * len(e) + i[ok]), colc[ok])
    krow = key // (4096 * len(e))
    starts = np.zeros((H, W + 1))
    np.add.at(starts, (krow, mincol), 1.0)
    per_row = np.zeros((H, W))
    for t0 in range(0, W, 16):
        per_row[:, t0:t0 + 16] = np.cumsum(starts[:, t0:min(t0 + 16, W)], axis=1)
    tol = tol + per_row * (f32_term(entry) + NUDGE)
    extra = edge_extra(entry)
    if extra.any():        # the lines of arcs: their own term, counted like the edges themselves
        starts = np.zeros((H, W + 1))
        np.add.at(starts, (krow, mincol), extra[key % len(e)])
        for t0 in range(0, W, 16):
            tol[:, t0:t0 + 16] += np.cumsum(starts[:, t0:min(t0 + 16, W)], axis=1)
    # cancellation in fine's area formula, in the pixel that holds the piece.  Beside a piece the formula is exact
    # (b, c, d and xmin are the constants 1, 1, 1 - 1e-6 left of it, and a = 1 exactly right of it).  For transformed
    # or computed outlines an edge on a pixel line may land just left of it: give the left neighbour the full term.
    w, h = np.abs(xb - xa), np.abs(ya - yb)
    inside = ok & (col >= 0)
    m = np.clip(np.maximum(xa, xb)[inside] - col[inside], 0.0, 1.0)
    cancel = np.zeros((H, W))
    np.add.at(cancel, (row[inside], col[inside]), CANCEL * (2 * m * m + 2 * m) / (w[inside] + 1e-6) * h[inside])
    if entry.tclass != "ident":
        lx = np.minimum(xa, xb)[inside] - col[inside]
        left = (col[inside] >= 1) & (lx <= f32_term(entry) + extra[i[inside]])
        np.add.at(cancel, (row[inside][left], col[inside][left] - 1), CANCEL * 4.0 / (w[inside][left] + 1e-6) * h[inside][left])
    tol = tol + cancel
    # the 1e-3 clamp: edges within 1e-3 of the top-left, top-right or bottom-left corner of the tile
    wt, ht = (W + 15) // 16, (H + 15) // 16
    cx, cy = np.meshgrid(np.arange(wt + 1) * 16.0, np.arange(ht + 1) * 16.0)
    cx, cy = cx.ravel(), cy.ravel()
    x0, y0, x1, y1 = (e[:, k][:, None] for k in range(4))
    dx, dy = x1 - x0, y1 - y0
    t = np.clip(((cx - x0) * dx + (cy - y0) * dy) / (dx * dx + dy * dy), 0.0, 1.0)
    d = np.hypot(cx - (x0 + t * dx), cy - (y0 + t * dy))
    near = (d <= X.TILE_CLAMP + f32_term(entry) + extra[:, None]).sum(axis=0).reshape(ht + 1, wt + 1)
    n_tile = near[:-1, :-1] + near[:-1, 1:] + near[1:, :-1]
    clamp = np.repeat(np.repeat(n_tile, 16, axis=0), 16, axis=1)[:H, :W] * X.TILE_CLAMP
    return tol + clamp


def evenodd_row_flip_mask(entry):
    """The pixels where an edge enters a tile through its left side on a pixel row line (f32 y) and goes down from there
    (that crossing is the upper end, xy0, of the tile's piece)."""
    W, H = entry.width, entry.height
    m = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in _edges(entry):
        if x0 == x1 or (y1 - y0) * (x1 - x0) < 0:
            continue
        for X0 in range(0, W, 16):
            if min(x0, x1) < X0 < max(x0, x1) or (X0 == 0 and min(x0, x1) < 0 < max(x0, x1)):
                y = float(np.float32(y0 + (X0 - x0) * (y1 - y0) / (x1 - x0)))
                if y == np.floor(y) and 0 <= y < H:
                    m[int(y), X0] = True
    return m


def check(entry, rule, aa, alpha):
    """Assert the alpha channel of one render against the reference; returns the largest error (for MSAA: of the
    pixels with no sample in the delta band) and the largest ratio of error to bound over the pixels."""
    ref = entry.reference_contours()
    W, H = entry.width, entry.height
    if aa == "area":
        want = X.area_alpha(X.area_acc(ref, W, H), rule)
        err = np.abs(alpha - want)
        tol = area_tolerance(entry, np.maximum(alpha, want))
        slack = err - tol
        ratio = float((err / tol).max()) if err.size else 0.0
    else:
        S = 8 if aa == "msaa8" else 16
        want = X.sample_alpha(X.sample_winding(ref, W, H, S), rule)
        near = X.near_mask(ref, W, H, S, DELTA[S] + f32_term(entry))
        extra = edge_extra(entry)
        if extra.any():    # the lines of arcs: a wider band by their own term, around those lines alone
            e = _edges(entry)
            for x in np.unique(extra[extra > 0]):
                lines = [l.reshape(2, 2) for l in e[extra == x]]
                near |= X.near_mask(lines, W, H, S, DELTA[S] + f32_term(entry) + x)
        k = near.sum(axis=-1)
        err = np.abs(alpha - want)
        if rule == "evenodd" and entry.id in EVENODD_MSAA_ROW_FLIP:
            flip = evenodd_row_flip_mask(entry)
            err = np.where(flip, np.minimum(err, np.abs(alpha - (1.0 - want))), err)
        slack = err - (k / S + 1e-7)
        err = np.where(k == 0, err, 0.0)
        ratio = float(((slack + k / S + 1e-7) / (k / S + 1e-7)).max()) if err.size else 0.0
    if slack.max() > 0:
        y, x = np.unravel_index(int(np.argmax(slack)), slack.shape)
        raise AssertionError("%s %s %s: %d pixel(s) out of bound; worst (x=%d, y=%d): alpha %.6f, exact %.6f, over by %.3g" %
                             (entry.id, rule, aa, int((slack > 0).sum()), x, y, alpha[y, x], want[y, x], slack[y, x]))
    return (float(err.max()) if err.size else 0.0), ratio


def record(request, entry, aa, result):
    """The observed error of one render and its largest share of the bound, for the per-class maxima."""
    m, ratio = result
    request.node.user_properties.append(("coverage_class", "%s/%s" % (entry.tclass, aa)))
    request.node.user_properties.append(("coverage_max_error", "%.3g" % m))
    request.node.user_properties.append(("coverage_max_share_of_bound", "%.3g" % ratio))
    request.node.add_report_section("call", "coverage", "class %s, %s: max error %.3g, at most %.3g of the bound" %
                                    (entry.tclass, aa, m, ratio))


CASES = [(e.id, rule, aa, "plain") for e in C.BATTERY for rule in C.RULES for aa in AAS]
CASES += [(eid, rule, aa, v) for eid in C.VARIANT_ENTRIES for v in ("clip", "paint") for rule in C.RULES for aa in AAS]


def render(engine, entry, rule, aa, variant):
    rec = Host().record(entry.scene(rule, variant), entry.params(AAS[aa]))
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    engine.sync()
    try:
        assert int(engine.download(rec.buffer("bumpBuf")[0], dtype=np.uint32)[0]) == 0
        t = rec.target
        img = engine.download_image(t["id"], t["width"], t["height"])
    finally:
        engine.release(rec)
    return img.view(np.float16).astype(np.float64)[..., 3]


@pytest.mark.parametrize("eid,rule,aa,variant", CASES, ids=["-".join(c) for c in CASES])
def test_coverage(engine, request, eid, rule, aa, variant):
    entry = C.BY_ID[eid]
    record(request, entry, aa, check(entry, rule, aa, render(engine, entry, rule, aa, variant)))


PARITY = ["f2-left-only", "f2-shallow-through-box", "f3-near-horizontal-one-tile-row", "f5-nested-squares-20", "f6-large-2^16"]


@pytest.mark.parametrize("eid", PARITY)
@pytest.mark.parametrize("aa", list(AAS))
def test_coverage_parity(engine, eid, aa):
    """Every buffer and the image bit for bit against the oracle: a coverage failure above says at once whether the
    oracle shares it."""
    from parity import compare
    entry = C.BY_ID[eid]
    for rule in C.RULES:
        compare(engine, entry.scene(rule), entry.params(AAS[aa]))
