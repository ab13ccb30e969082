"""The ramps of jh_distance as the keywords of ``Engine.distance``: each returns dict(which, max_distance, scale,
offset) -- ``engine.distance(src, dst, color=..., **distance.outline(2.5))``.  The value of a texel is v = clamp(s scale + offset, 0,
1) with s the distance `which` selects, in texels, measured between texel centres; s = max_distance + 1 where nothing lies within
max_distance."""
import math

from .imagecalls import DISTANCE_MAX_RADIUS, DistanceWhich


def _radius(reach):
    """The smallest legal max_distance that is at least `reach`."""
    r = max(1, int(math.ceil(reach)))
    if r > DISTANCE_MAX_RADIUS:
        raise ValueError("jh_distance: the ramp reaches %g texels, more than max_distance = 255 covers" % reach)
    return r


def outline(width):
    """The coverage of the shape dilated by a disc of radius `width` >= 0 (fractional widths welcome): OUTER, v = clamp(width + 0.5
    - s, 0, 1) -- 1 up to s = width - 0.5, a ramp one texel wide, 0 from s = width + 0.5 on.  scale = -1, offset = width + 0.5,
    max_distance = ceil(width + 0.5): a texel farther than that has v = 0 either way."""
    if not width >= 0:
        raise ValueError("jh_distance: an outline's width is >= 0")
    return dict(which=DistanceWhich.OUTER, max_distance=_radius(width + 0.5), scale=-1.0, offset=width + 0.5)


def inset(width):
    """The coverage of the shape eroded by a disc of radius `width` >= 0: INNER, v = clamp(s + 0.5 - width, 0, 1) -- 0 up to s =
    width - 0.5, 1 from s = width + 0.5 on (s >= 1 on every seed, s = 0 outside the shape).  scale = 1, offset = 0.5 - width,
    max_distance = ceil(width + 0.5)."""
    if not width >= 0:
        raise ValueError("jh_distance: an inset's width is >= 0")
    return dict(which=DistanceWhich.INNER, max_distance=_radius(width + 0.5), scale=1.0, offset=0.5 - width)


def glow(radius, inner=False):
    """A linear falloff over `radius` > 0 texels: v = clamp(1 - s / radius, 0, 1), 1 on the shape (OUTER; inner: on its complement,
    INNER) and 0 from s = radius on.  scale = -1 / radius, offset = 1, max_distance = ceil(radius)."""
    if not radius > 0:
        raise ValueError("jh_distance: a glow's radius is > 0")
    return dict(which=DistanceWhich.INNER if inner else DistanceWhich.OUTER, max_distance=_radius(radius), scale=-1.0 / radius, offset=1.0)


def sdf(spread):
    """The usual signed distance field texture over an integer `spread` in [1, 255]: SIGNED, v = clamp(0.5 + s / (2 spread), 0, 1) --
    0.5 on the texel edge between inside and outside, 0 at `spread` inside, 1 at `spread` outside.  scale = 1 / (2 spread), offset =
    0.5, max_distance = spread.  Store it with straight=True."""
    if int(spread) != spread or not 1 <= spread <= DISTANCE_MAX_RADIUS:
        raise ValueError("jh_distance: an SDF's spread is an integer in [1, 255]")
    return dict(which=DistanceWhich.SIGNED, max_distance=int(spread), scale=1.0 / (2.0 * int(spread)), offset=0.5)
