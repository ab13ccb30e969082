"""The resample rule of DESIGN.md 5.9 in numpy, written from the rule alone: the reference jh_resample is compared with byte for byte.

  axis        n_in source texels (the source RECTANGLE's extent) onto n_out, binary64: scale = n_in / n_out, fs = max(scale, 1),
              support = base fs (base 0.5 BOX, 1 TRIANGLE, 2 CATMULL_ROM, 3 LANCZOS3); legal: 1 <= n_in <= 16 n_out, n_out >= 1.
  window      c = (i + 0.5) scale; lo = max(0, trunc(c - support + 0.5)); hi = min(n_in, trunc(c + support + 0.5));
              g_k = f((k - c + 0.5) / fs), k = lo .. hi - 1; leading and trailing g_k == 0.0 are dropped, interior zeros stay;
              S = the sum of the g_k ascending; w_k = (float)(g_k / S).  math.sin is the libm sin the library calls on the same machine.
  source      the f16 texel widened to (c, a); p = (c a, a) (exact), or with STRAIGHT p = (c, a).  Never written: transparent black.
  horizontal  H = 0.0f; for k ascending over the x window: H = fmaf(w_k, p[k], H)            (binary32, never rounded to f16)
  vertical    V = 0.0f; for k ascending over the y window: V = fmaf(w_k, H[k], V)            (rows before columns)
  store       STRAIGHT: f16(V).  Default: a_inv = 1.0f / max(V.a, 1e-6f); f16(V.rgb a_inv + 0.0f), f16(V.a + 0.0f)  (maxNum)
Nothing is clamped: the negative lobes of CATMULL_ROM and LANCZOS3 can leave alpha below 0 or colour above 1.

The keyword arguments of `resample` after `dst_bits` build the six WRONG variants the battery has to tell from the rule
(tests/test_resample_spec.py): unfused multiply then add, descending k, the centre i scale, a clipped window left un-renormalised, the
premultiply skipped in default mode, columns before rows."""
import math

import numpy as np

from image_ref import fmaf32, fmax, mul_add32, resolve, same_bits  # noqa: F401 (same_bits is part of this module's interface)

BOX, TRIANGLE, CATMULL_ROM, LANCZOS3 = 0, 1, 2, 3
FILTERS = (BOX, TRIANGLE, CATMULL_ROM, LANCZOS3)
FILTER_NAMES = ("box", "triangle", "catmull_rom", "lanczos3")
BASE = (0.5, 1.0, 2.0, 3.0)
STRAIGHT = 1
MAX_RATIO = 16
MAX_TAPS = 96  # JRESAMPLE_MAX_TAPS


def _sinc(x):
    if x == 0.0:
        return 1.0
    t = x * math.pi
    return math.sin(t) / t


def kernel(filt, x):
    """f(x), the operations in the rule's order."""
    if filt == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if filt == TRIANGLE:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if filt == CATMULL_ROM:
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
        if x < 2.0:
            return (((x - 5.0) * x + 8.0) * x - 4.0) * a
        return 0.0
    if filt == LANCZOS3:
        return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0
    raise ValueError("unknown filter")


def sizes_ok(n_in, n_out):
    return n_in >= 1 and n_out >= 1 and n_in <= MAX_RATIO * n_out


def window(filt, n_in, n_out, i, centre_half=True, renormalise=True, exact=False):
    """(first, weights, S) of output i: weights float32 (float64 and unrounded with exact=True), S the binary64 sum."""
    if filt not in FILTERS or not sizes_ok(n_in, n_out) or not (0 <= i < n_out):
        raise ValueError("unknown filter, illegal sizes or an index outside the axis")
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = BASE[filt] * fs
    c = (float(i) + 0.5) * scale if centre_half else float(i) * scale  # (the second: a wrong variant)
    lo_raw, hi_raw = int(c - support + 0.5), int(c + support + 0.5)  # int() truncates
    lo, hi = max(0, lo_raw), min(n_in, hi_raw)
    g = [kernel(filt, (float(k) - c + 0.5) / fs) for k in range(lo, hi)]
    a, b = 0, len(g)
    while a < b and g[a] == 0.0:
        a += 1
    while b > a and g[b - 1] == 0.0:
        b -= 1
    g = g[a:b]
    S = 0.0
    for v in g:
        S = S + v
    if not renormalise:  # (a wrong variant: the sum runs over the window before it is clipped to the rectangle)
        S = 0.0
        for k in range(lo_raw, hi_raw):
            S = S + kernel(filt, (float(k) - c + 0.5) / fs)
    if exact:
        return lo + a, np.array(g, np.float64) / S, S
    return lo + a, np.array([np.float32(v / S) for v in g], np.float32), S


def axis_taps(filt, n_in, n_out, **variant):
    """[(first, weights)] for every output index of the axis."""
    return [window(filt, n_in, n_out, i, **variant)[:2] for i in range(n_out)]


def _pass(src, taps, step, descending):
    """One axis of the rule along axis 0 of a float32 array (n_in, m, 4): out (n_out, m, 4), out[i] = the sum over the window of i."""
    out = np.zeros((len(taps),) + src.shape[1:], np.float32)
    for i, (first, w) in enumerate(taps):
        acc = np.zeros(src.shape[1:], np.float32)
        order = range(len(w) - 1, -1, -1) if descending else range(len(w))
        for j in order:
            acc = step(w[j], src[first + j], acc)
        out[i] = acc
    return out


def _rects(src_shape, dst_shape, src_rect, dst_rect):
    why = "a rectangle is outside its image or empty in one dimension"
    (sx, sy, sw, sh), (dx, dy, dw, dh) = resolve(src_shape, src_rect, why, texels=True), resolve(dst_shape, dst_rect, why, texels=True)
    if not sizes_ok(sw, dw) or not sizes_ok(sh, dh):
        raise ValueError("a ratio above 16:1")
    return (sx, sy, sw, sh), (dx, dy, dw, dh)


def resample(src_bits, dst_shape, filt, flags=0, src_rect=None, dst_rect=None, dst_bits=None, fused=True, descending=False,
             centre_half=True, renormalise=True, premultiply=True, rows_first=True):
    """The image jh_resample leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero).
    dst_shape = (height, width) of dst; dst_bits: what dst held (None: a never-written dst, transparent black).  flags: 0 or STRAIGHT.
    Rectangles are (x, y, width, height), None: the whole image.  Returns (height, width, 4) uint16."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    out = np.zeros(tuple(dst_shape[:2]) + (4,), np.uint16) if dst_bits is None else np.array(dst_bits, np.uint16)
    (sx, sy, sw, sh), (dx, dy, dw, dh) = _rects(src_bits.shape, out.shape, src_rect, dst_rect)
    variant = dict(centre_half=centre_half, renormalise=renormalise)
    tx, ty = axis_taps(filt, sw, dw, **variant), axis_taps(filt, sh, dh, **variant)
    step = fmaf32 if fused else mul_add32
    straight = bool(flags & STRAIGHT)
    with np.errstate(all="ignore"):
        p = src_bits[sy:sy + sh, sx:sx + sw].view(np.float16).astype(np.float32)
        if not straight and premultiply:
            p = np.concatenate([p[..., :3] * p[..., 3:], p[..., 3:]], axis=-1).astype(np.float32)
        if rows_first:
            hor = _pass(np.moveaxis(p, 1, 0), tx, step, descending)  # (dw, sh, 4)
            ver = _pass(np.moveaxis(hor, 1, 0), ty, step, descending)  # (dh, dw, 4)
        else:  # (a wrong variant)
            ver = _pass(p, ty, step, descending)  # (dh, sw, 4)
            ver = np.moveaxis(_pass(np.moveaxis(ver, 1, 0), tx, step, descending), 1, 0)
        if straight:
            texels = ver
        else:
            zero = np.float32(0.0)
            a_inv = np.float32(1.0) / fmax(ver[..., 3], np.float32(1e-6))
            texels = np.concatenate([ver[..., :3] * a_inv[..., None] + zero, ver[..., 3:] + zero], axis=-1)
        out[dy:dy + dh, dx:dx + dw] = texels.astype(np.float32).astype(np.float16).view(np.uint16)
    return out


def direct(src_bits, dst_shape, filt, flags=0, src_rect=None, dst_rect=None):
    """The definition the rule rounds: the 2-D sum in binary64 with unrounded taps, before the store -- (dh, dw, 4) float64 of the
    destination rectangle (premultiplied by alpha unless STRAIGHT)."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    (sx, sy, sw, sh), (dx, dy, dw, dh) = _rects(src_bits.shape, tuple(dst_shape[:2]), src_rect, dst_rect)
    p = src_bits[sy:sy + sh, sx:sx + sw].view(np.float16).astype(np.float64)
    if not flags & STRAIGHT:
        p = np.concatenate([p[..., :3] * p[..., 3:], p[..., 3:]], axis=-1)
    mx, my = np.zeros((dw, sw)), np.zeros((dh, sh))
    for m, n_in, n_out in ((mx, sw, dw), (my, sh, dh)):
        for i in range(n_out):
            first, w, _ = window(filt, n_in, n_out, i, exact=True)
            m[i, first:first + len(w)] = w
    return np.einsum("ys,xt,stc->yxc", my, mx, p)
