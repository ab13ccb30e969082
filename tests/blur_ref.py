"""The blur rule of DESIGN.md 5.7 in numpy, written from the rule alone: the reference jh_blur is compared with byte for byte.

  taps        sigma as binary32, used as binary64; R = ceil(3 sigma); sigma = 0: the single tap 1.0f; otherwise
              g_k = exp(-(double)(k k) / (2.0 sigma sigma)), S = g_0 + 2 (g_1 + ... + g_R) with the bracket summed in that order,
              w_k = (float)(g_k / S), w_-k = w_k.  math.exp is the libm exp the library's std::exp calls on the same machine.
  horizontal  H = 0.0f; for k = -Rx..Rx ascending: H = fmaf(w_k, (float)src[x + k], H)       (binary32, never rounded to f16)
  vertical    V = 0.0f; for k = -Ry..Ry ascending: V = fmaf(w_k, H[y + k], V); dst = f16(V)  (round to nearest even, once)
  edges       ZERO: a tap outside the image is not executed; CLAMP: it reads the nearest texel of the image.

binary32 fmaf is emulated exactly (image_ref.fmaf32).

The keyword arguments of `blur` after `dst` build the four WRONG variants the battery has to tell from the rule
(tests/test_blur_spec.py): unfused multiply then add, descending k, an f16 intermediate, taps normalised in binary32."""
import math

import numpy as np

from image_ref import fmaf32, mul_add32, same_bits  # noqa: F401 (same_bits is part of this module's interface)

ZERO, CLAMP = 0, 1
MAX_SIGMA = 64.0


def radius(sigma):
    return int(math.ceil(3.0 * float(np.float32(sigma))))


def taps(sigma, binary32_normalise=False):
    """(weights float32 [2R + 1], R) of one axis."""
    s = float(np.float32(sigma))
    if not (0.0 <= s <= MAX_SIGMA):
        raise ValueError("sigma is negative, above 64 or NaN")
    R = int(math.ceil(3.0 * s))
    if R == 0:
        return np.ones(1, np.float32), 0
    den = 2.0 * s * s
    g = [math.exp(-float(k * k) / den) for k in range(R + 1)]
    side = g[1]
    for k in range(2, R + 1):
        side = side + g[k]
    S = g[0] + 2.0 * side
    if binary32_normalise:  # (a wrong variant)
        half = [np.float32(np.float32(v) / np.float32(S)) for v in g]
    else:
        half = [np.float32(v / S) for v in g]
    return np.array(half[:0:-1] + half, np.float32), R


def exact_taps(sigma):
    """The taps before their rounding to binary32, as binary64 (for the comparison with the definition)."""
    s = float(np.float32(sigma))
    R = int(math.ceil(3.0 * s))
    if R == 0:
        return np.ones(1, np.float64), 0
    g = np.exp(-np.arange(-R, R + 1, dtype=np.float64) ** 2 / (2.0 * s * s))
    return g / g.sum(), R


def _pass(src, w, R, edge, axis, step, descending):
    """One axis of the rule on a float32 array (H, W, 4): out = sum over k of w_k src[.. + k ..] by `step`, in order."""
    src = np.moveaxis(src, axis, 0)
    n = src.shape[0]
    acc = np.zeros_like(src, dtype=np.float32)
    pos = np.arange(n)
    order = range(R, -R - 1, -1) if descending else range(-R, R + 1)
    for k in order:
        at = pos + k
        if edge == CLAMP:
            acc = step(w[k + R], src[np.clip(at, 0, n - 1)], acc)
        else:
            ok = (at >= 0) & (at < n)
            if ok.any():
                acc[ok] = step(w[k + R], src[at[ok]], acc[ok])
    return np.moveaxis(acc, 0, axis)


def blur(src_bits, sigma, edge=ZERO, rect=None, dst_bits=None, fused=True, descending=False, f16_intermediate=False,
         binary32_taps=False):
    """The image jh_blur leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero).
    sigma: a scalar or (sigma_x, sigma_y).  rect = (x, y, w, h) or None: the whole image.  dst_bits: what dst held (None: a
    never-written dst, transparent black).  Returns (H, W, 4) uint16."""
    sx, sy = sigma if isinstance(sigma, (tuple, list)) else (sigma, sigma)
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    H, W, _ = src_bits.shape
    x, y, w, h = (0, 0, W, H) if rect is None or (rect[2] == 0 and rect[3] == 0) else rect
    wx, Rx = taps(sx, binary32_taps)
    wy, Ry = taps(sy, binary32_taps)
    step = fmaf32 if fused else mul_add32
    out = np.zeros_like(src_bits) if dst_bits is None else np.array(dst_bits, np.uint16)
    if w == 0 or h == 0:
        return out
    r0, r1 = max(0, y - Ry), min(H, y + h + Ry)  # the rows of H the rectangle's columns read
    with np.errstate(all="ignore"):
        f = src_bits.view(np.float16).astype(np.float32)
        hor = np.zeros((H, W, 4), np.float32)
        hor[r0:r1] = _pass(f[r0:r1], wx, Rx, edge, 1, step, descending)
        if f16_intermediate:  # (a wrong variant)
            hor = hor.astype(np.float16).astype(np.float32)
        ver = _pass(hor[:, x:x + w], wy, Ry, edge, 0, step, descending)
        out[y:y + h, x:x + w] = ver[y:y + h].astype(np.float16).view(np.uint16)
    return out


def direct(src_bits, sigma, edge=ZERO):
    """The definition the rule rounds: the direct 2-D Gaussian sum in binary64 with unrounded taps, (H, W, 4) float64."""
    sx, sy = sigma if isinstance(sigma, (tuple, list)) else (sigma, sigma)
    f = np.ascontiguousarray(src_bits, np.uint16).view(np.float16).astype(np.float64)
    H, W, _ = f.shape
    (gx, Rx), (gy, Ry) = exact_taps(sx), exact_taps(sy)
    out = np.zeros_like(f)
    ys, xs = np.arange(H), np.arange(W)
    for ky in range(-Ry, Ry + 1):
        for kx in range(-Rx, Rx + 1):
            yy, xx = ys + ky, xs + kx
            if edge == CLAMP:
                out += gy[ky + Ry] * gx[kx + Rx] * f[np.clip(yy, 0, H - 1)][:, np.clip(xx, 0, W - 1)]
            else:
                oy, ox = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
                if oy.any() and ox.any():
                    out[np.ix_(oy, ox)] += gy[ky + Ry] * gx[kx + Rx] * f[np.ix_(yy[oy], xx[ox])]
    return out
