"""Exact float64 coverage of closed polylines: the independent reference that tests/test_coverage_spec.py (oracle) and
tests/test_gpu_coverage.py (HIP image) judge fill coverage against.  It shares no code with the oracle, the host or
tests/fine_by_hand.py: it is written from the definitions alone.

Winding convention: the winding number of a point is the signed count of edges that a ray from it towards -x crosses,
+1 for an edge going up (y decreasing), -1 for one going down -- the sign fine.wgsl's accumulation gives (area += a * dy
with dy = y0 - y1, fine.wgsl:839-857).  A contour is an (n, 2) float64 array of vertices; its closing edge is implied.

* area_acc: the exact integral of the winding number over every pixel square (fine.wgsl's `area` before the fold).
* area_alpha: the non-zero and even-odd folds of fine.wgsl:865-875.
* sample_winding: the winding number at every sample point of the 8x / 16x patterns of renderer/mask.go.
* msaa_delta: the distance from an edge within which the quantised mask LUT may misclassify a sample (see its docstring
  for the numbers).
"""
import numpy as np

# renderer/mask.go: sample i of a pixel sits in row i (y = (i + 0.5) / n) at column pattern[i] (x = (pattern[i] + 0.5) / n).
# The y half-plane masks of fine.wgsl:308-315 cut bit i by row, which fixes the row of bit i; the LUT definition
# evaluates the same points for both slope signs (the negative block mirrors y and the line together).
PATTERN = {8: np.array([0, 5, 3, 7, 1, 4, 6, 2]), 16: np.array([1, 8, 4, 11, 15, 7, 3, 12, 0, 9, 5, 13, 2, 10, 6, 14])}
LUT_SHAPE = {8: (32, 32), 16: (64, 64)}   # (MASK_WIDTH, MASK_HEIGHT) of fine.wgsl:60-71: offsets x slopes (two blocks)
TILE_CLAMP = 1e-3                         # path_tiling.wgsl:99-120


def sample_points(samples):
    """(samples, 2) pixel-local (x, y) sample positions, bit order."""
    k = np.arange(samples, dtype=np.float64)
    return np.stack([(PATTERN[samples] + 0.5) / samples, (k + 0.5) / samples], axis=1)


def edges_of(contours):
    """(n, 4) float64 array x0, y0, x1, y1 of every edge of every closed contour (closing edges included)."""
    out = []
    for c in contours:
        c = np.asarray(c, np.float64).reshape(-1, 2)
        if len(c) == 0:
            continue
        nxt = np.roll(c, -1, axis=0)
        out.append(np.concatenate([c, nxt], axis=1))
    return np.concatenate(out, axis=0) if out else np.zeros((0, 4))


def _crossings(lo, hi, lim):
    """For intervals (lo, hi) per edge: the integers k with lo < k < hi and 0 <= k <= lim, as (edge index, k)."""
    first = np.maximum(np.floor(lo) + 1.0, 0.0)
    last = np.minimum(np.ceil(hi) - 1.0, float(lim))
    n = np.maximum(last - first + 1.0, 0.0).astype(np.int64)
    idx = np.repeat(np.arange(len(lo)), n)
    start = np.repeat(np.cumsum(n) - n, n)
    k = np.repeat(first, n) + (np.arange(int(n.sum())) - start)
    return idx, k


def _pieces(e, width, height):
    """Split every edge at the pixel rows and columns of the viewport (outside it only at its border lines).
    Returns the pieces' end points (xa, ya, xb, yb) in float64 and their cell (col, row), with col -1 / width and
    row -1 / height standing for everything left / right / above / below the viewport."""
    x0, y0, x1, y1 = e.T
    ix, kx = _crossings(np.minimum(x0, x1), np.maximum(x0, x1), width)
    iy, ky = _crossings(np.minimum(y0, y1), np.maximum(y0, y1), height)
    tx = (kx - x0[ix]) / (x1[ix] - x0[ix])
    ty = (ky - y0[iy]) / (y1[iy] - y0[iy])
    n = len(e)
    idx = np.concatenate([np.arange(n), np.arange(n), ix, iy])
    t = np.concatenate([np.zeros(n), np.ones(n), tx, ty])
    order = np.lexsort((t, idx))
    idx, t = idx[order], t[order]
    same = idx[1:] == idx[:-1]
    i, ta, tb = idx[:-1][same], t[:-1][same], t[1:][same]
    keep = tb > ta
    i, ta, tb = i[keep], ta[keep], tb[keep]
    dx, dy = x1[i] - x0[i], y1[i] - y0[i]
    xa, ya = x0[i] + ta * dx, y0[i] + ta * dy
    xb, yb = x0[i] + tb * dx, y0[i] + tb * dy
    # exact end points where the split was on a grid line (x0 + t * dx may miss the integer by an ulp)
    xa = np.where(ta == 0.0, x0[i], xa)
    ya = np.where(ta == 0.0, y0[i], ya)
    xb = np.where(tb == 1.0, x1[i], xb)
    yb = np.where(tb == 1.0, y1[i], yb)
    xm, ym = 0.5 * (xa + xb), 0.5 * (ya + yb)
    col = np.clip(np.floor(xm), -1, width).astype(np.int64)
    row = np.clip(np.floor(ym), -1, height).astype(np.int64)
    return xa, ya, xb, yb, col, row, i


def area_acc(contours, width, height):
    """(height, width) float64: the integral of the winding number over each pixel square.  Every piece of an edge
    inside a cell adds its signed height times the part of the cell's strip to its right (a trapezoid) to that cell and
    its signed height to every cell right of it (a prefix sum of 'cover' along the row); pieces left of the viewport
    only carry cover into column 0, pieces right of it or outside the rows add nothing."""
    e = edges_of(contours)
    e = e[e[:, 1] != e[:, 3]]          # horizontal edges have no area
    acc = np.zeros((height, width + 1))
    if len(e) == 0 or width == 0 or height == 0:
        return acc[:, :width]
    xa, ya, xb, yb, col, row, _ = _pieces(e, width, height)
    h = ya - yb                        # +1 per unit of height for an upward edge
    inrow = (row >= 0) & (row < height)
    inside = inrow & (col >= 0) & (col < width)
    area = h[inside] * (1.0 - (0.5 * (xa[inside] + xb[inside]) - col[inside]))
    flat = row[inside] * (width + 1) + col[inside]
    a = np.bincount(flat, area, minlength=height * (width + 1))
    cov = inrow & (col < width)
    flat = row[cov] * (width + 1) + col[cov] + 1
    c = np.bincount(flat, h[cov], minlength=height * (width + 1))
    acc = a.reshape(height, width + 1) + np.cumsum(c.reshape(height, width + 1), axis=1)
    return acc[:, :width]


def area_alpha(acc, rule):
    """fine.wgsl:865-875: non-zero min(|acc|, 1); even-odd |acc - 2 round(acc / 2)| (round half to even, as WGSL)."""
    if rule == "nonzero":
        return np.minimum(np.abs(acc), 1.0)
    return np.abs(acc - 2.0 * np.round(0.5 * acc))


def sample_winding(contours, width, height, samples):
    """(height, width, samples) int32: the winding number at each sample point (pixel + sample_points(samples)).
    An edge counts for a sample row y if min(y0, y1) <= y < max(y0, y1), and for a sample if it crosses that row at
    an x strictly less than the sample's."""
    e = edges_of(contours)
    e = e[e[:, 1] != e[:, 3]]
    sp = sample_points(samples)
    nrows = height * samples
    diff = np.zeros((nrows, width + 1), np.int64)
    if len(e):
        x0, y0, x1, y1 = e.T
        lo, hi = np.minimum(y0, y1), np.maximum(y0, y1)
        # sample rows m with (m + 0.5) / S in [lo, hi): m in [ceil(lo * S - 0.5), ceil(hi * S - 0.5))
        m0 = np.clip(np.ceil(lo * samples - 0.5), 0, nrows).astype(np.int64)
        m1 = np.clip(np.ceil(hi * samples - 0.5), 0, nrows).astype(np.int64)
        n = m1 - m0
        idx = np.repeat(np.arange(len(e)), n)
        m = np.repeat(m0, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
        ys = (m + 0.5) / samples
        xc = x0[idx] + (ys - y0[idx]) * (x1[idx] - x0[idx]) / (y1[idx] - y0[idx])
        sx = sp[m % samples, 0]
        # samples px + sx > xc  <=>  px > xc - sx  <=>  px >= floor(xc - sx) + 1
        j = np.clip(np.floor(xc - sx) + 1, 0, width).astype(np.int64)
        sign = np.where(y1[idx] < y0[idx], 1, -1)
        np.add.at(diff, (m, j), sign)
    w = np.cumsum(diff, axis=1)[:, :width]                 # (height * S, width): row m = pixel row m // S, sample m % S
    return w.reshape(height, samples, width).transpose(0, 2, 1).astype(np.int32)


def sample_alpha(wind, rule):
    """Fraction of samples inside: non-zero (fill_path_ms) or odd (fill_path_ms_evenodd) winding."""
    inside = (wind != 0) if rule == "nonzero" else (wind % 2 != 0)
    return inside.mean(axis=-1)


def near_samples(contours, width, height, samples, delta):
    """(height, width) int: the number k of a pixel's samples within `delta` (< 1) of some edge, end points included."""
    return near_mask(contours, width, height, samples, delta).sum(axis=-1)


def near_mask(contours, width, height, samples, delta):
    """(height, width, samples) bool: the samples that an edge may misclassify.  In a pixel that the edge passes through
    or ends in, fine looks every sample of the rows the edge spans up in the mask LUT of the edge's LINE -- an edge that
    ends inside the pixel is cut by sample row only (fine.wgsl:308-315), never along its length -- so there the
    distance is taken from the line; a horizontal edge cuts no row at all, and a sample beyond its end point but within
    `delta` of its line is classified by the quantised LUT line like any other.  In the eight pixels around such a
    pixel the distance is taken from the edge itself, end points included (`delta` < 1)."""
    e = edges_of(contours)
    e = e[(e[:, 0] != e[:, 2]) | (e[:, 1] != e[:, 3])]
    near = np.zeros((height, width, samples), bool)
    if len(e) == 0:
        return near
    _, _, _, _, col, row, i = _pieces(e, width, height)
    horiz = e[:, 1] == e[:, 3]                     # horizontal edges have no pieces of their own: add their cells
    for j in np.flatnonzero(horiz):
        x0, y, x1, _ = e[j]
        c = np.arange(max(int(np.floor(min(x0, x1))), -1), min(int(np.floor(max(x0, x1))), width) + 1)
        col = np.concatenate([col, c])
        row = np.concatenate([row, np.full(len(c), int(np.floor(y)))])
        i = np.concatenate([i, np.full(len(c), j)])
    own = np.unique((i * (height + 2) + row) * (width + 2) + col)     # (edge, pixel) pairs the edge has a piece in
    off = np.array([(dc, dr) for dc in (-1, 0, 1) for dr in (-1, 0, 1)])
    col = (col[:, None] + off[None, :, 0]).ravel()
    row = (row[:, None] + off[None, :, 1]).ravel()
    i = np.repeat(i, 9)
    ok = (col >= 0) & (col < width) & (row >= 0) & (row < height)
    col, row, i = col[ok], row[ok], i[ok]
    key = np.unique((i * (height + 2) + row) * (width + 2) + col)
    on_line = np.isin(key, own)
    col = key % (width + 2)
    row = (key // (width + 2)) % (height + 2)
    i = key // ((width + 2) * (height + 2))
    sp = sample_points(samples)
    qx = col[:, None] + sp[None, :, 0]
    qy = row[:, None] + sp[None, :, 1]
    x0, y0, x1, y1 = (e[i, k][:, None] for k in range(4))
    dx, dy = x1 - x0, y1 - y0
    t = ((qx - x0) * dx + (qy - y0) * dy) / (dx * dx + dy * dy)
    t = np.where(on_line[:, None], t, np.clip(t, 0.0, 1.0))
    d = np.hypot(qx - (x0 + t * dx), qy - (y0 + t * dy))
    r, s = np.nonzero(d <= delta)
    near[row[r], col[r], s] = True
    return near


def lut_from_definition(samples):
    """The half-plane mask LUT of renderer/mask.go, restated: entry (v, u) for a line of slope (v % half + 0.5) / half
    crossing the pixel's anti-diagonal at offset (u + 0.5) / width; v >= half is the positive-slope block."""
    W, H = LUT_SHAPE[samples]
    half = H // 2
    sp = sample_points(samples)
    v, u = np.divmod(np.arange(W * H), W)
    slope = ((v % half) + 0.5) / half
    t = (u + 0.5) / W
    return _classify(sp, slope, t, v >= half)


def _classify(sp, a, t, is_pos):
    """Bit i set iff sample i lies on the +x side of the line (or on it).  In the pixel's own frame the line has
    |dx| / (|dx| + dy) = a and crosses the anti-diagonal x + y = 1 at x = t (positive slope) or, mirrored, at x = 1 - t
    (fine.wgsl:238-262: zf - z is that offset in the frame where x grows along the line).  Returns bits and the signed
    distances (samples, lines) of the samples from the line."""
    a, t, is_pos = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(t, np.float64), np.asarray(is_pos))
    px = np.where(is_pos, t, 1.0 - t)
    py = 1.0 - t
    nx = 1.0 - a
    ny = np.where(is_pos, -a, a)
    d = ((sp[:, 0:1] - px[None]) * nx[None] + (sp[:, 1:2] - py[None]) * ny[None]) / np.hypot(nx, ny)[None]
    bits = (d >= 0.0)
    return bits, d


def lut_bits(lut_words, samples):
    """(entries, samples) bool of an uploaded LUT (uint8 per entry for 8 samples, uint16 for 16)."""
    w = np.asarray(lut_words).astype(np.int64)
    return ((w[:, None] >> np.arange(samples)[None, :]) & 1).astype(bool)


def msaa_delta(samples, lut=None, per_cell=12, slack=1e-4):
    """Brute force over the LUT's cells: for `per_cell` x `per_cell` lines in every (slope row, offset column) cell of
    both blocks -- widened by `slack` on every side, so that f32 rounding of a and zf into a neighbouring cell is
    covered -- the largest distance from the true line of a sample whose LUT bit disagrees with its true side.
    Returns that maximum plus the 1e-3 tile clamp: the distance from an edge beyond which a sample is never
    misclassified.  Measured on the LUT of renderer/mask.go: 0.0548 px + 1e-3 = 0.0558 for 8 samples and
    0.0276 px + 1e-3 = 0.0286 for 16 (the same with 24 or 48 lines per cell side: the maximum sits at cell corners)."""
    W, H = LUT_SHAPE[samples]
    half = H // 2
    if lut is None:
        bits_lut = lut_from_definition(samples)[0].T                      # (entries, samples)
    else:
        bits_lut = lut_bits(lut, samples)
    sp = sample_points(samples)
    f = np.linspace(-slack, 1.0 + slack, per_cell)
    worst = 0.0
    for blk in (0, 1):
        for v in range(half):
            hi = (v + 1) / half if v < half - 1 else 1.0
            a = np.clip(v / half + f * (hi - v / half), 0.0, 1.0)
            u = np.arange(W)
            t = (u[:, None] + f[None, :]) / W                              # (W, per_cell)
            A, T = np.meshgrid(a, t.ravel(), indexing="ij")
            U = np.broadcast_to(np.repeat(u, per_cell)[None, :], A.shape)
            bits, d = _classify(sp, A.ravel(), T.ravel(), np.full(A.size, blk == 1))
            want = bits_lut[(blk * half + v) * W + U.ravel()].T           # (samples, lines)
            wrong = bits != want
            if wrong.any():
                worst = max(worst, float(np.abs(d[wrong]).max()))
    return worst + TILE_CLAMP
