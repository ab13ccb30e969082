"""The colour filters of Filter Effects Level 1 as arguments of Engine.color_filter (jh_color_filter, the rule: DESIGN.md 5.10).

Every constructor returns a dict of color_filter's keywords -- `engine.color_filter(image, **colorfilter.grayscale(1))`,
`engine.capture(rec, color=colorfilter.sepia(0.5))`.  A matrix is computed in binary64 from the specification's coefficients and
rounded once to binary32; it is row-major 4 x 5 on the un-premultiplied (r, g, b, a, 1).

The CSS filter functions are defined on sRGB-encoded colour, the images hold linear values: grayscale, sepia, saturate, hue_rotate,
invert, brightness and contrast ask for ColorSpace.SRGB with the clamp on.  opacity asks for LINEAR: it changes alpha only, alpha
is never encoded, and in LINEAR space the colour channels keep their bits where the round trip through the sRGB curve would
not (DESIGN.md 5.10 has the deviation).  luminance_to_alpha and tint are LINEAR too: feColorMatrix's luminanceToAlpha on the
stored values, and a colour given as linear values.  LINEAR without funcs needs no tables on the device.

linear, gamma, table and discrete make the entries of `funcs` (feComponentTransfer's function types; None is the identity)."""
import math

import numpy as np

from .imagecalls import ColorFunc, ColorSpace


def linear(slope, intercept=0.0):
    return (ColorFunc.LINEAR, float(slope), float(intercept))


def gamma(amplitude, exponent, offset=0.0):
    return (ColorFunc.GAMMA, float(amplitude), float(exponent), float(offset))


def table(values):
    return (ColorFunc.TABLE, tuple(float(v) for v in values))


def discrete(values):
    return (ColorFunc.DISCRETE, tuple(float(v) for v in values))


def _matrix(rgb_rows, alpha_row=(0.0, 0.0, 0.0, 1.0, 0.0)):
    """Three rows of 3 (the colour block; no alpha column, no offset) or of 5, and the alpha row, as 20 binary32 values."""
    rows = [tuple(r) + (0.0, 0.0) if len(r) == 3 else tuple(r) for r in rgb_rows] + [tuple(alpha_row)]
    return np.array(rows, np.float64).astype(np.float32).reshape(20)


def _unit(amount):
    return min(max(float(amount), 0.0), 1.0)


def _css(matrix=None, funcs=None):
    return dict(matrix=matrix, funcs=funcs, space=ColorSpace.SRGB, clamp=True)


def grayscale(amount=1.0):
    """grayscale(): amount in [0, 1] (clamped), 1 is fully grey."""
    a = 1.0 - _unit(amount)
    return _css(_matrix([(0.2126 + 0.7874 * a, 0.7152 - 0.7152 * a, 0.0722 - 0.0722 * a),
                         (0.2126 - 0.2126 * a, 0.7152 + 0.2848 * a, 0.0722 - 0.0722 * a),
                         (0.2126 - 0.2126 * a, 0.7152 - 0.7152 * a, 0.0722 + 0.9278 * a)]))


def sepia(amount=1.0):
    """sepia(): amount in [0, 1] (clamped)."""
    a = 1.0 - _unit(amount)
    return _css(_matrix([(0.393 + 0.607 * a, 0.769 - 0.769 * a, 0.189 - 0.189 * a),
                         (0.349 - 0.349 * a, 0.686 + 0.314 * a, 0.168 - 0.168 * a),
                         (0.272 - 0.272 * a, 0.534 - 0.534 * a, 0.131 + 0.869 * a)]))


def saturate(amount=1.0):
    """saturate(): amount >= 0, 0 is fully unsaturated, above 1 oversaturates.  With the luminance coefficients of grayscale()
    (0.2126, 0.7152, 0.0722), so that saturate(0) is grayscale(1); SVG 1.1's feColorMatrix type="saturate" rounds them to three
    digits."""
    s = max(float(amount), 0.0)
    return _css(_matrix([(0.2126 + 0.7874 * s, 0.7152 - 0.7152 * s, 0.0722 - 0.0722 * s),
                         (0.2126 - 0.2126 * s, 0.7152 + 0.2848 * s, 0.0722 - 0.0722 * s),
                         (0.2126 - 0.2126 * s, 0.7152 - 0.7152 * s, 0.0722 + 0.9278 * s)]))


def hue_rotate(degrees=0.0):
    """hue-rotate(): feColorMatrix type="hueRotate", the angle in degrees."""
    t = math.radians(float(degrees))
    c, s = math.cos(t), math.sin(t)
    return _css(_matrix([(0.213 + c * 0.787 - s * 0.213, 0.715 - c * 0.715 - s * 0.715, 0.072 - c * 0.072 + s * 0.928),
                         (0.213 - c * 0.213 + s * 0.143, 0.715 + c * 0.285 + s * 0.140, 0.072 - c * 0.072 - s * 0.283),
                         (0.213 - c * 0.213 - s * 0.787, 0.715 - c * 0.715 + s * 0.715, 0.072 + c * 0.928 + s * 0.072)]))


def luminance_to_alpha():
    """feColorMatrix type="luminanceToAlpha": colour becomes 0, alpha the luminance 0.2125 r + 0.7154 g + 0.0721 b of the stored
    (linear) values -- the first half of `mask-type: luminance` (Engine.luminance_mask)."""
    zero = (0.0, 0.0, 0.0)
    return dict(matrix=_matrix([zero, zero, zero], (0.2125, 0.7154, 0.0721, 0.0, 0.0)), funcs=None, space=ColorSpace.LINEAR, clamp=True)


def invert(amount=1.0):
    """invert(): feFuncR/G/B type="table" tableValues="amount (1 - amount)", which is the line (1 - 2 amount) c + amount."""
    a = _unit(amount)
    f = linear(1.0 - 2.0 * a, a)
    return _css(funcs=(f, f, f, None))


def opacity(amount=1.0):
    """opacity(): alpha times amount in [0, 1] (clamped); feFuncA type="table" tableValues="0 amount"."""
    return dict(matrix=None, funcs=(None, None, None, linear(_unit(amount), 0.0)), space=ColorSpace.LINEAR, clamp=True)


def brightness(amount=1.0):
    """brightness(): feFuncR/G/B type="linear" slope="amount", amount >= 0."""
    f = linear(max(float(amount), 0.0), 0.0)
    return _css(funcs=(f, f, f, None))


def contrast(amount=1.0):
    """contrast(): feFuncR/G/B type="linear" slope="amount" intercept="-(0.5 amount) + 0.5", amount >= 0."""
    c = max(float(amount), 0.0)
    f = linear(c, -(0.5 * c) + 0.5)
    return _css(funcs=(f, f, f, None))


def tint(color):
    """The tint half of drop-shadow(): every texel takes the colour (r, g, b) of `color` = (r, g, b, a), linear values, and its
    alpha is scaled by a -- feFlood + feComposite operator="in" on the source's alpha."""
    r, g, b, a = (float(v) for v in color)
    return dict(matrix=_matrix([(0.0, 0.0, 0.0, 0.0, r), (0.0, 0.0, 0.0, 0.0, g), (0.0, 0.0, 0.0, 0.0, b)], (0.0, 0.0, 0.0, a, 0.0)),
                funcs=None, space=ColorSpace.LINEAR, clamp=True)
