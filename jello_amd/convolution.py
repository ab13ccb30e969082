"""Convolution kernels as arguments of Engine.convolve (jh_convolve, the rule: DESIGN.md 5.13).

Every constructor returns a dict of convolve's keywords -- `engine.convolve(src, dst, **convolution.sharpen(1))`,
`engine.capture(rec, convolve=dict(dst=image, **convolution.box(3)))`.

jh_convolve takes its weights in the order they are applied (weights[j][i] multiplies the texel at (X - target_x + i, Y - target_y +
j)) and never divides.  from_svg takes feConvolveMatrix's attributes instead: the kernelMatrix, which the specification applies
rotated by 180 degrees, and the divisor; jello_amd.convolve_weights (jh_convolve_weights) flips and divides, in binary64, rounded
once to binary32.  The named kernels below are written in applied order; sobel_x and sobel_y are positive where the image grows
with x and with y."""
import numpy as np

from .imagecalls import ConvolveEdge, ConvolveMode, convolve_weights

EDGE_MODES = {"none": ConvolveEdge.ZERO, "duplicate": ConvolveEdge.CLAMP, "wrap": ConvolveEdge.REPEAT, "mirror": ConvolveEdge.MIRROR}


def _keywords(weights, edge=ConvolveEdge.CLAMP, mode=ConvolveMode.PREMULTIPLIED, bias=0.0, target=None):
    w = np.asarray(weights, np.float64).astype(np.float32)
    return dict(weights=w, order=(w.shape[1], w.shape[0]), target=target, edge=edge, mode=mode, bias=float(bias))


def from_svg(order, kernel_matrix, divisor=0, bias=0, target=None, edge_mode="duplicate", preserve_alpha=False):
    """feConvolveMatrix: `order` a scalar or (orderX, orderY), `kernel_matrix` its orderX * orderY numbers, `divisor` (0: their sum,
    or 1 if that is 0), `bias`, `target` = (targetX, targetY) (None: the centre), `edge_mode` 'duplicate', 'wrap', 'none' (or
    'mirror'), `preserve_alpha`."""
    if edge_mode not in EDGE_MODES:
        raise ValueError("convolution.from_svg: edge_mode is one of " + ", ".join(sorted(EDGE_MODES)))
    w = convolve_weights(order, kernel_matrix, divisor)
    mode = ConvolveMode.PRESERVE_ALPHA if preserve_alpha else ConvolveMode.PREMULTIPLIED
    return dict(weights=w, order=(w.shape[1], w.shape[0]), target=target, edge=EDGE_MODES[edge_mode], mode=mode, bias=float(bias))


def sharpen(amount=1.0):
    """The identity plus `amount` times the 4-neighbour Laplacian: centre 1 + 4 amount, the four neighbours -amount.  The weights sum
    to 1: flat areas keep their value."""
    a = float(amount)
    return _keywords([[0.0, -a, 0.0], [-a, 1.0 + 4.0 * a, -a], [0.0, -a, 0.0]])


def box(n):
    """The n x n mean, n in 1..15 (each weight the binary32 nearest 1 / n^2)."""
    n = int(n)
    if not 1 <= n <= 15:
        raise ValueError("convolution.box: n outside 1..15")
    return _keywords(np.full((n, n), 1.0 / (n * n)))


def emboss():
    """A relief lit from the top left, on the stored colour with the alpha kept: flat areas come out mid-grey (bias 0.5)."""
    return _keywords([[-2.0, -1.0, 0.0], [-1.0, 1.0, 1.0], [0.0, 1.0, 2.0]], mode=ConvolveMode.PRESERVE_ALPHA, bias=0.5)


def sobel_x():
    """The horizontal Sobel derivative on the stored colour, alpha kept.  Signed: nothing is clamped."""
    return _keywords([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], mode=ConvolveMode.PRESERVE_ALPHA)


def sobel_y():
    """The vertical Sobel derivative on the stored colour, alpha kept."""
    return _keywords([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]], mode=ConvolveMode.PRESERVE_ALPHA)


def laplacian(diagonals=False):
    """The 4-neighbour Laplacian (centre -4), or with `diagonals` the 8-neighbour one (centre -8), on the stored colour, alpha kept."""
    if diagonals:
        return _keywords([[1.0, 1.0, 1.0], [1.0, -8.0, 1.0], [1.0, 1.0, 1.0]], mode=ConvolveMode.PRESERVE_ALPHA)
    return _keywords([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]], mode=ConvolveMode.PRESERVE_ALPHA)
