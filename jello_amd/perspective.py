"""Projective matrices as arguments of Engine.perspective (jh_perspective, the rule: DESIGN.md 5.19).

Every constructor returns a dict of perspective's keywords, `dict(matrix=(a, b, p, c, d, q, e, f, s))` --
`engine.perspective(src, dst, **perspective.rotate_y(math.radians(30), 800, (w / 2, h / 2)))`,
`engine.project_layer(layer, target, scratch_image_id=s, layer_size=..., target_size=..., **perspective.from_quad(size, quad))`.

The matrix is column-major, x' w = a x + c y + e, y' w = b x + d y + f, w = p x + q y + s, and takes continuous coordinates of the
source rectangle to continuous coordinates of the destination image.  The arithmetic here is plain binary64 and is no part of the
rule: the rule starts at the nine numbers the call is given.  `compose` and every argument called `m` take such a dict or the nine
numbers themselves."""
import math

import numpy as np


def _nine(m):
    m = m["matrix"] if isinstance(m, dict) else m
    m = tuple(float(v) for v in m)
    if len(m) != 9:
        raise ValueError("perspective: a matrix has 9 entries (a, b, p, c, d, q, e, f, s)")
    return m


def _keywords(m):
    return dict(matrix=tuple(float(v) for v in m))


def affine(m6):
    """jh_warp's matrix (a, b, c, d, e, f) as a projective one: p = q = 0, s = 1."""
    a, b, c, d, e, f = (float(v) for v in m6)
    return _keywords((a, b, 0.0, c, d, 0.0, e, f, 1.0))


def compose(a, b):
    """The map that applies `b` first and `a` to its result: the matrix product a b."""
    A, B = np.array(_nine(a)).reshape(3, 3).T, np.array(_nine(b)).reshape(3, 3).T  # (column-major: rows of the reshape are columns)
    return _keywords((A @ B).T.reshape(-1))


def from_quad(src_size, four_points):
    """The map that takes the source rectangle (0, 0) .. `src_size` = (width, height) onto the quadrilateral `four_points` =
    ((x0, y0), (x1, y1), (x2, y2), (x3, y3)), the images of its top-left, top-right, bottom-right and bottom-left corners in that
    order: the closed form for the unit square (Heckbert 1989), scaled.  ValueError for a quad that has three corners on a line or
    that puts a corner of the rectangle at w <= 0 (a concave or self-crossing quad)."""
    W, H = float(src_size[0]), float(src_size[1])
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = ((float(x), float(y)) for x, y in four_points)
    if not (W > 0.0 and H > 0.0):
        raise ValueError("perspective.from_quad: an empty source rectangle")
    dx1, dy1, dx2, dy2 = x1 - x2, y1 - y2, x3 - x2, y3 - y2
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dy1 * dx2
    if den == 0.0 or not math.isfinite(den):
        raise ValueError("perspective.from_quad: three corners of the quad are on a line")
    g, h = (sx * dy2 - sy * dx2) / den, (dx1 * sy - dy1 * sx) / den
    if not (1.0 + g > 0.0 and 1.0 + h > 0.0 and 1.0 + g + h > 0.0):
        raise ValueError("perspective.from_quad: the quad puts a corner of the rectangle at w <= 0")
    a, b, c, d = x1 - x0 + g * x1, y1 - y0 + g * y1, x3 - x0 + h * x3, y3 - y0 + h * y3
    return _keywords((a / W, b / W, g / W, c / H, d / H, h / H, x0, y0, 1.0))


def from_matrix3d(m16):
    """CSS matrix3d(m11, m12, m13, m14, m21, ..., m44) -- sixteen numbers, column-major -- acting on the plane z = 0: the z row
    and the z column dropped.  x' w = m11 x + m21 y + m41, y' w = m12 x + m22 y + m42, w = m14 x + m24 y + m44."""
    m = tuple(float(v) for v in m16)
    if len(m) != 16:
        raise ValueError("perspective.from_matrix3d: sixteen numbers")
    return _keywords((m[0], m[1], m[3], m[4], m[5], m[7], m[12], m[13], m[15]))


def _about(origin, distance, rotation):
    ox, oy = float(origin[0]), float(origin[1])
    d = float(distance)
    if not d > 0.0:
        raise ValueError("perspective: the distance is positive")
    to, back, persp = np.eye(4), np.eye(4), np.eye(4)
    to[0, 3], to[1, 3], back[0, 3], back[1, 3] = ox, oy, -ox, -oy
    persp[3, 2] = -1.0 / d
    return from_matrix3d((to @ persp @ rotation @ back).T.reshape(-1))


def rotate_x(angle, distance, origin=(0.0, 0.0)):
    """CSS `perspective(distance) rotateX(angle)` about `origin` = (x, y) (transform-origin and perspective-origin alike), `angle`
    in radians: translate(origin) perspective(distance) rotateX(angle) translate(-origin) on the plane z = 0."""
    c, s = math.cos(angle), math.sin(angle)
    r = np.eye(4)
    r[1, 1], r[1, 2], r[2, 1], r[2, 2] = c, -s, s, c
    return _about(origin, distance, r)


def rotate_y(angle, distance, origin=(0.0, 0.0)):
    """CSS `perspective(distance) rotateY(angle)` about `origin`, `angle` in radians, as rotate_x."""
    c, s = math.cos(angle), math.sin(angle)
    r = np.eye(4)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = c, s, -s, c
    return _about(origin, distance, r)
