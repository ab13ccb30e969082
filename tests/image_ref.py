"""What the numpy references of the image calls (tests/*_ref.py) share: the exact binary32 fmaf and its wrong variant, the equality
of f16 bit patterns, minNum / maxNum, the rectangle a descriptor names, the operands of a source, and the index a tap outside the
rectangle reads.  Each reference keeps its own rule and its own deliberately wrong variants; only what they had in common is here.

binary32 fmaf is emulated exactly (fmaf32): the product of two binary32 values is exact in binary64 (24 + 24 bits), its sum with
the accumulator is rounded to odd in binary64 (TwoSum gives the error of the rounded sum; a sum that is inexact and even moves to
its odd neighbour on the error's side), and one conversion to binary32 follows -- 53 >= 24 + 2 bits, so the double rounding is
innocuous, subnormal results included.  A plain binary64 add in its place is not proven and is not used."""
import numpy as np

ZERO, CLAMP, REPEAT, MIRROR = 0, 1, 2, 3  # jwarp_index's edge modes (jh_warp_edge, jh_convolve_edge)


def fmaf32(w, x, acc):
    """fmaf(w, x, acc) in binary32, exactly, elementwise (w a scalar or an array)."""
    with np.errstate(all="ignore"):
        p = np.asarray(w, np.float32).astype(np.float64) * np.asarray(x, np.float32).astype(np.float64)  # exact
        a = np.asarray(acc, np.float32).astype(np.float64)
        s = p + a
        bb = s - p  # TwoSum (Knuth): err = the exact p + a - s wherever s is finite
        err = (p - (s - bb)) + (a - bb)
        odd_wanted = np.isfinite(s) & (err != 0.0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(odd_wanted, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def mul_add32(w, x, acc):
    """The wrong variant of fmaf32 that the references' `fused=False` takes: the product rounded to binary32 before the add."""
    with np.errstate(all="ignore"):
        return (np.asarray(w, np.float32) * np.asarray(x, np.float32) + np.asarray(acc, np.float32)).astype(np.float32)


def same_bits(a, b):
    """Equal f16 bit patterns, a NaN equal to any NaN."""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    nan_a, nan_b = (a & 0x7FFF) > 0x7C00, (b & 0x7FFF) > 0x7C00
    return bool(np.all((a == b) | (nan_a & nan_b)))


def _f(a):
    return np.asarray(a, np.float32)


def fmin(a, b):
    """IEEE minNum with -0 below +0."""
    a, b = np.broadcast_arrays(_f(a), _f(b))
    both_zero = (a == 0) & (b == 0)
    pick_a = np.isnan(b) | (a < b) | (both_zero & np.signbit(a))
    return np.where(np.isnan(a), b, np.where(pick_a, a, b)).astype(np.float32)


def fmax(a, b):
    """IEEE maxNum with -0 below +0."""
    a, b = np.broadcast_arrays(_f(a), _f(b))
    both_zero = (a == 0) & (b == 0)
    pick_a = np.isnan(b) | (a > b) | (both_zero & ~np.signbit(a))
    return np.where(np.isnan(a), b, np.where(pick_a, a, b)).astype(np.float32)


def resolve(shape, rect, why="the rectangle is outside the image or empty in one dimension", texels=False):
    """(x, y, w, h) of the rectangle `rect` names in an image of `shape` = (H, W, ...), None or 0 x 0: the whole image; ValueError(why)
    for one outside the image or empty in one dimension -- with `texels`, for one without texels too."""
    H, W = shape[:2]
    x, y, w, h = (0, 0, W, H) if rect is None or (rect[2] == 0 and rect[3] == 0) else rect
    if ((w == 0 or h == 0) if texels else (w == 0) != (h == 0)) or x + w > W or y + h > H:
        raise ValueError(why)
    return x, y, w, h


def operands(bits, premultiply, dtype=np.float32):
    """(H, W, 4) `dtype`: the values of the f16 bit patterns `bits`, the colour channels times alpha with `premultiply`."""
    with np.errstate(all="ignore"):
        p = np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(dtype)
        if premultiply:
            p = np.concatenate([p[..., :3] * p[..., 3:], p[..., 3:]], axis=-1).astype(dtype)
    return p


def index(edge, i, n):
    """jwarp_index: the index in [0, n) a tap i reads, -1 where it reads +0 (ZERO outside); i an int64 array."""
    i = np.asarray(i, np.int64)
    if edge == ZERO:
        return np.where((i >= 0) & (i < n), i, -1)
    if edge == CLAMP:
        return np.minimum(np.maximum(i, 0), n - 1)
    if edge == REPEAT:
        return np.mod(i, n)  # (numpy's mod of a positive modulus is non-negative)
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)
