"""The battery jh_color_filter is held to tests/color_ref.py on, byte for byte (tests/test_gpu_color.py), and on which the
reference is told from its near misses (tests/test_color_spec.py).

VALUES: one image the value cases run on, 256 wide:
  rows   0..255  every f16 bit pattern once in each channel; the channels are decorrelated by fixed bijections of the 16-bit
                 index (odd multipliers), so every entry of every table is read and NaN, +-Inf, subnormals and +-0 meet finite
                 values and each other in the matrix
  rows 256..351  random values in [-0.25, 1.25], where colour lives and the clamp, the sRGB curve and the funcs have their bends
VALUE_CASES: name -> the keywords of color_filter (matrix, funcs, space, clamp).
GEOMETRY: the rectangle widths at the kernel's seams (a work item is 512 texels, a lane two), by heights, x offsets of both
parities and image widths of both parities (with an odd width the 16-byte phase of a row's first texel alternates by row)."""
import math

import numpy as np

from jello_amd import colorfilter as cf

import color_ref

POISON = 0x5A5A  # f16 210.5: what a destination holds around the rectangle
NAN_BITS = 0x7FFF  # what a source holds around the rectangle


def values_image():
    i = np.arange(65536, dtype=np.uint32)
    ch = [i, (i * 40503 + 12345) & 0xFFFF, (i * 25173 + 13849) & 0xFFFF, (i * 0x9E37 + 0x79B9) & 0xFFFF]
    allbits = np.stack(ch, axis=-1).astype(np.uint16).reshape(256, 256, 4)
    for c in range(4):
        assert np.array_equal(np.sort(allbits[..., c].reshape(-1)), np.arange(65536, dtype=np.uint32).astype(np.uint16))
    rng = np.random.default_rng(510)
    unit = rng.uniform(-0.25, 1.25, (96, 256, 4)).astype(np.float16)
    unit[::7, ::5, 3] = 1.0
    unit[1::7, 1::5, 3] = 0.0
    return np.concatenate([allbits, unit.view(np.uint16)], axis=0)


VALUES = values_image()

_rng = np.random.default_rng(5100)
DENSE = tuple(float(v) for v in _rng.uniform(-1.5, 1.5, 20).astype(np.float32))
# entries whose products overflow binary32 (3e38 x 65504), an offset of -0 under zero coefficients (fmaf(0, t, -0) is -0 for a
# negative t), and rows whose terms cancel exactly
HOSTILE = (3.0e38, 0.0, 0.0, 0.0, -0.0,
           0.0, -3.0e38, 3.0e38, 0.0, 0.0,
           1.0, -1.0, 0.0, 0.0, -0.0,
           0.5, 0.5, -1.0, 1.0, -0.0)
_RAMP64 = tuple(float(v) for v in np.linspace(0.0, 1.0, 64) ** 2)
_STEPS64 = tuple(float(v) for v in np.linspace(1.0, 0.0, 64))

FUNC_SETS = {
    "linear": (cf.linear(1.5, -0.25), cf.linear(-1.0, 1.0), cf.linear(0.5, 0.5), cf.linear(0.75, 0.0)),
    "gamma": (cf.gamma(1.0, 2.2, 0.0), cf.gamma(1.1, 1.0 / 2.2, -0.05), cf.gamma(0.9, 3.0, 0.1), cf.gamma(1.0, 0.5, 0.0)),
    "table": (cf.table([0.25]), cf.table([0.0, 1.0]), cf.table([1.0, 0.2, 0.7]), cf.table(_RAMP64)),
    "discrete": (cf.discrete([0.3]), cf.discrete([0.0, 1.0]), cf.discrete([0.2, 0.9, 0.4]), cf.discrete(_STEPS64)),
    "mixed": (None, cf.gamma(1.0, 2.0, 0.0), None, cf.discrete([0.0, 0.5, 1.0])),
}


def _plain(matrix=None, funcs=None, space=color_ref.LINEAR, clamp=True):
    return dict(matrix=matrix, funcs=funcs, space=int(space), clamp=clamp)


def _value_cases():
    out = {}
    for clamp in (True, False):
        tag = "clamp" if clamp else "free"
        out["identity_" + tag] = _plain(clamp=clamp)                      # TABLES = false
        out["dense_" + tag] = _plain(DENSE, clamp=clamp)                  # TABLES = false
        out["hostile_" + tag] = _plain(HOSTILE, clamp=clamp)
        out["identity_srgb_" + tag] = _plain(space=color_ref.SRGB, clamp=clamp)
        out["dense_srgb_" + tag] = _plain(DENSE, space=color_ref.SRGB, clamp=clamp)
        for name, fs in FUNC_SETS.items():
            out["%s_linear_%s" % (name, tag)] = _plain(DENSE if name == "mixed" else None, fs, color_ref.LINEAR, clamp)
            out["%s_srgb_%s" % (name, tag)] = _plain(DENSE if name == "mixed" else None, fs, color_ref.SRGB, clamp)
    css = {"grayscale": cf.grayscale(1.0), "grayscale_half": cf.grayscale(0.5), "sepia": cf.sepia(1.0), "saturate": cf.saturate(1.8),
           "hue_rotate_90": cf.hue_rotate(90.0), "invert": cf.invert(1.0), "brightness_2": cf.brightness(2.0), "contrast_half": cf.contrast(0.5),
           "opacity": cf.opacity(0.4), "luminance_to_alpha": cf.luminance_to_alpha(), "tint": cf.tint((0.1, 0.2, 0.9, 0.5))}
    for name, kw in css.items():
        out[name] = dict(kw, space=int(kw["space"]))
    return out


VALUE_CASES = _value_cases()

WIDTHS = (1, 2, 3, 511, 512, 513, 1025)
HEIGHTS = (1, 3)


def geometry(width):
    """The calls of one rectangle width: dicts with the image size, the rectangle and which filter (tables or none)."""
    out = []
    for h in HEIGHTS:
        for x in (2, 5):  # an even and an odd offset
            for image_w in (width + 8, width + 9):  # an even and an odd image width (the parities of width + 8 and + 9 differ)
                for tables in (False, True):
                    out.append(dict(size=(image_w, h + 3), rect=(x, 1, width, h), tables=tables))
    return out


def geometry_filter(tables):
    return VALUE_CASES["grayscale_half"] if tables else VALUE_CASES["dense_clamp"]


def geometry_source(size, seed):
    """A source whose rectangle will hold colour and whose surroundings hold NaN."""
    w, h = size
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16).view(np.uint16)


def surround(bits, rect, value):
    """bits with everything outside rect set to the bit pattern `value`."""
    x, y, w, h = rect
    out = np.full_like(bits, value)
    out[y:y + h, x:x + w] = bits[y:y + h, x:x + w]
    return out
