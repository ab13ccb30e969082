"""The convolve rule (include/jello_hip.h "Convolve") in numpy, written from the rule alone: what jh_convolve has to
produce, bit for bit.  Sums are binary32 with the rule's fmaf (image_ref.fmaf32), one chain per channel.

  weights(order, kernel_matrix, divisor)   jh_convolve_weights: feConvolveMatrix's matrix flipped and divided (ValueError when refused)
  convolve(...)                            the image jh_convolve leaves in dst
  direct(...)                              the definition the rule rounds: the sum in binary64, and the sum of the |w p|

convolve() takes keyword switches that build near misses of the rule (tests/test_convolve_spec.py asserts that the battery of
tests/convolve_cases.py tells each of them from the rule): flipped=True (the weights applied rotated by 180 degrees), fused=False
(multiply, round, add), descending=True (the chain walked from the last tap to the first), row_sums=True (a chain per kernel row,
the rows added), target_shift=1 (the target off by one in x and y), edge_rect=True (the rectangle is the edge, not the image),
skip_zero=True (a zero weight does not multiply), bias_source_alpha=True (bias times the source texel's alpha instead of the
result's), mirror_2n=False (MIRROR with period n: the copies not flipped)."""
import math

import numpy as np

import image_ref
from image_ref import fmaf32, fmax, mul_add32, resolve, same_bits  # noqa: F401 (same_bits is part of this module's interface)

ZERO, CLAMP, REPEAT, MIRROR = 0, 1, 2, 3
EDGES = (ZERO, CLAMP, REPEAT, MIRROR)
EDGE_NAMES = {ZERO: "zero", CLAMP: "clamp", REPEAT: "repeat", MIRROR: "mirror"}
PREMULTIPLIED, STRAIGHT, PRESERVE_ALPHA = 0, 1, 2
MODES = (PREMULTIPLIED, STRAIGHT, PRESERVE_ALPHA)
MODE_NAMES = {PREMULTIPLIED: "premul", STRAIGHT: "straight", PRESERVE_ALPHA: "preserve"}
MAX_ORDER, MAX_TAPS = 15, 225


def weights(order, kernel_matrix, divisor=0.0):
    """(order_y, order_x) float32: weights[j][i] = (float)(km[(oy - 1 - j) ox + (ox - 1 - i)] / d), the quotient in binary64."""
    ox, oy = order if isinstance(order, (tuple, list)) else (order, order)
    km = [float(v) for v in kernel_matrix]
    if not (1 <= ox <= MAX_ORDER and 1 <= oy <= MAX_ORDER) or len(km) != ox * oy:
        raise ValueError("an order outside 1..15")
    d = float(divisor)
    if not math.isfinite(d) or not all(math.isfinite(v) for v in km):
        raise ValueError("a non-finite input")
    total = 0.0
    for v in km:
        total = total + v
    if d == 0.0:
        if not math.isfinite(total):
            raise ValueError("the sum of kernelMatrix is not finite")
        d = 1.0 if total == 0.0 else total
    out = np.empty(ox * oy, np.float32)
    with np.errstate(all="ignore"):
        for k in range(ox * oy):
            out[k] = np.float32(np.float64(km[ox * oy - 1 - k]) / np.float64(d))  # (numpy: an overflowing quotient is an Inf, as in C)
    if not np.all(np.isfinite(out)):
        raise ValueError("a weight does not come out finite")
    return out.reshape(oy, ox)


def index(edge, i, n, mirror_2n=True):
    """jwarp_index: the index in [0, n) a tap i reads, -1 where it reads +0 (ZERO outside); i an int64 array."""
    return image_ref.index(edge if mirror_2n or edge != MIRROR else REPEAT, i, n)  # (the wrong variant of MIRROR: period n)


def operands(src_bits, mode):
    """(H, W, 4) float32: what the sums take of every source texel (PRESERVE_ALPHA: the alpha channel is there and is not used)."""
    return image_ref.operands(src_bits, mode == PREMULTIPLIED)


def check(w, target, edge, mode, bias):
    w = np.asarray(w, np.float32)
    if w.ndim != 2 or not (1 <= w.shape[0] <= MAX_ORDER and 1 <= w.shape[1] <= MAX_ORDER):
        raise ValueError("an order outside 1..15")
    oy, ox = w.shape
    tx, ty = (ox // 2, oy // 2) if target is None else target
    if not (0 <= tx < ox and 0 <= ty < oy):
        raise ValueError("the target is outside the kernel")
    if edge not in EDGES or mode not in MODES:
        raise ValueError("unknown edge or mode")
    if not (np.all(np.isfinite(w)) and math.isfinite(float(np.float32(bias)))):
        raise ValueError("a weight or the bias is not finite")
    return w, ox, oy, tx, ty


def convolve(src_bits, w, target=None, edge=CLAMP, mode=PREMULTIPLIED, bias=0.0, rect=None, dst_bits=None, flipped=False, fused=True,
             descending=False, row_sums=False, target_shift=0, edge_rect=False, skip_zero=False, bias_source_alpha=False, mirror_2n=True):
    """The image jh_convolve leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero).  w: (order_y,
    order_x) float32 in applied order; target = (target_x, target_y), None: the centre.  rect = (x, y, width, height), None: the whole
    image.  dst_bits: what dst held (None: a never-written dst, transparent black).  Returns (H, W, 4) uint16."""
    w, ox, oy, tx, ty = check(w, target, edge, mode, bias)
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    H, W, _ = src_bits.shape
    out = np.zeros_like(src_bits) if dst_bits is None else np.array(dst_bits, np.uint16)
    x, y, rw, rh = resolve(src_bits.shape, rect)
    if rw == 0 or rh == 0:
        return out
    if flipped:
        w = w[::-1, ::-1]
    tx, ty = tx + target_shift, ty + target_shift
    p = operands(src_bits, mode)
    step = fmaf32 if fused else mul_add32
    X, Y = x + np.arange(rw, dtype=np.int64), y + np.arange(rh, dtype=np.int64)

    def operand(i, j):
        if edge_rect:  # (a wrong variant)
            ix, iy = index(edge, X - x - tx + i, rw, mirror_2n), index(edge, Y - y - ty + j, rh, mirror_2n)
            ix, iy = np.where(ix >= 0, ix + x, -1), np.where(iy >= 0, iy + y, -1)
        else:
            ix, iy = index(edge, X - tx + i, W, mirror_2n), index(edge, Y - ty + j, H, mirror_2n)
        live = (iy >= 0)[:, None] & (ix >= 0)[None, :]
        return np.where(live[..., None], p[np.maximum(iy, 0)][:, np.maximum(ix, 0)], np.float32(0.0)).astype(np.float32)

    zero4 = np.zeros((rh, rw, 4), np.float32)
    taps = [(j, i) for j in range(oy) for i in range(ox)]
    with np.errstate(all="ignore"):
        if row_sums:  # (a wrong variant)
            acc = zero4
            for j in range(oy):
                h = zero4
                for i in range(ox):
                    h = step(w[j, i], operand(i, j), h)
                acc = (acc + h).astype(np.float32)
        else:
            acc = zero4
            for j, i in (taps[::-1] if descending else taps):
                if skip_zero and w[j, i] == 0.0:
                    continue
                acc = step(w[j, i], operand(i, j), acc)
        b = np.float32(bias)
        v = acc.copy()
        if b != 0.0:
            if mode == PREMULTIPLIED:
                v[..., 3] = acc[..., 3] + b
                alpha = p[y:y + rh, x:x + rw, 3] if bias_source_alpha else v[..., 3]
                v[..., :3] = fmaf32(b, alpha[..., None], acc[..., :3])
            elif mode == STRAIGHT:
                v = (acc + b).astype(np.float32)
            else:
                v[..., :3] = acc[..., :3] + b
        if mode == PREMULTIPLIED:
            zero = np.float32(0.0)
            a_inv = np.float32(1.0) / fmax(v[..., 3], np.float32(1e-6))
            v = np.concatenate([v[..., :3] * a_inv[..., None] + zero, v[..., 3:] + zero], axis=-1)
        bits = v.astype(np.float32).astype(np.float16).view(np.uint16)
        if mode == PRESERVE_ALPHA:
            bits[..., 3] = src_bits[y:y + rh, x:x + rw, 3]
        out[y:y + rh, x:x + rw] = bits
    return out


def direct(src_bits, w, target=None, edge=CLAMP, mode=PREMULTIPLIED, rect=None):
    """The definition the rule rounds, before the bias and the store: ((rh, rw, 4) float64 sums of w p over the window, the sums of
    |w p|), of the rectangle, premultiplied under PREMULTIPLIED."""
    w, ox, oy, tx, ty = check(w, target, edge, mode, 0.0)
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    H, W, _ = src_bits.shape
    x, y, rw, rh = resolve(src_bits.shape, rect)
    p = operands(src_bits, mode).astype(np.float64)
    X, Y = x + np.arange(rw, dtype=np.int64), y + np.arange(rh, dtype=np.int64)
    total, mag = np.zeros((rh, rw, 4)), np.zeros((rh, rw, 4))
    for j in range(oy):
        for i in range(ox):
            ix, iy = index(edge, X - tx + i, W), index(edge, Y - ty + j, H)
            live = (iy >= 0)[:, None] & (ix >= 0)[None, :]
            t = float(w[j, i]) * np.where(live[..., None], p[np.maximum(iy, 0)][:, np.maximum(ix, 0)], 0.0)
            total += t
            mag += np.abs(t)
    return total, mag
