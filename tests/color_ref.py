"""The colour-filter rule of DESIGN.md 5.10 in numpy, written from the rule alone: the reference jh_color_filter and
jh_color_tables are compared with bit for bit.  Nothing here reads include/jello_color.h.

Per texel, binary32 (h_c: the stored f16 bit pattern of channel c, un-premultiplied):
  input    t_c = PRE_c[h_c] for c = r, g, b in SRGB space; otherwise, and always for alpha, h_c widened
  matrix   m = M[i][4]; m = fmaf(M[i][k], t_k, m) for k = 0, 1, 2, 3           (image_ref.fmaf32: the exact binary32 fmaf)
  clamp    with the flag: m = m > 0 ? m : 0; m = m < 1 ? m : 1               (np.where on the comparison: NaN and -0 become +0)
  round    g = f16(m), round to nearest even; a NaN m gives 0x7e00
  output   POST_i[g] where channel i has a table, else g
The tables, binary64, one entry per f16 bit pattern (x: the index pattern's value):
  enc      a = |x|; 12.92 a if a <= 0.0031308 else 1.055 pow(a, 1.0 / 2.4) - 0.055; with x's sign.   dec: a / 12.92 if a <= 0.04045
           else pow((a + 0.055) / 1.055, 2.4); with x's sign.  pow is math.pow, the libm pow the library calls on the same machine.
  PRE_c    (float)enc(x); NaN: 0x7fc00000
  func_i   IDENTITY x; LINEAR slope x + intercept; GAMMA amplitude pow(x, exponent) + offset; TABLE (N = n - 1): v_0 if N = 0 else
           c = clamp01(x), k = min((int)(c N), N - 1), v_k + ((x - k / N) N) (v_k+1 - v_k); DISCRETE: k = min((int)(c n), n - 1), v_k
  POST_i   y = func_i(x); the clamp with the flag; dec for r, g, b in SRGB space; f16(y) rounded once; NaN y and NaN x: 0x7e00
  exists   PRE_c in SRGB space; POST_i where func_i is not IDENTITY or dec applies

A func is None (IDENTITY) or (type, parameters ...): (1, slope, intercept), (2, amplitude, exponent, offset), (3, values),
(4, values) -- the tuples of jello_amd.colorfilter.  `variant` of `apply` builds the WRONG rules the battery has to tell from the
rule (tests/test_color_spec.py)."""
import functools
import math

import numpy as np

from image_ref import fmaf32, mul_add32

LINEAR, SRGB = 0, 1
F_IDENTITY, F_LINEAR, F_GAMMA, F_TABLE, F_DISCRETE = 0, 1, 2, 3, 4
NAN16 = 0x7E00
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
VARIANTS = ("offset_last", "unfused", "clamp_after_round", "enc_alpha", "func_after_dec", "minmax_nan")

ALL16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)
X64 = ALL16.view(np.float16).astype(np.float64)  # the value of every f16 bit pattern, exactly


def _odd_integer(y):
    return y == math.floor(y) and math.fmod(y, 2.0) != 0.0


def pow64(x, y):
    """C's pow(x, y) through math.pow, which raises where C sets errno."""
    try:
        return math.pow(x, y)
    except ValueError:  # a pole (0 to a negative power) or a negative base to a fractional power
        if x == 0.0:
            return -math.inf if math.copysign(1.0, x) < 0.0 and _odd_integer(y) else math.inf
        return math.nan
    except OverflowError:
        return -math.inf if x < 0.0 and _odd_integer(y) else math.inf


def enc(x):
    a = abs(x)
    r = 12.92 * a if a <= 0.0031308 else 1.055 * pow64(a, 1.0 / 2.4) - 0.055
    return math.copysign(r, x)


def dec(x):
    a = abs(x)
    r = a / 12.92 if a <= 0.04045 else pow64((a + 0.055) / 1.055, 2.4)
    return math.copysign(r, x)


def _each(f, values):
    return np.array([f(float(v)) for v in values], np.float64)


def _clamp01(v):
    """Compare and select: NaN and -0 become +0."""
    v = np.where(v > 0.0, v, 0.0)
    return np.where(v < 1.0, v, 1.0)


def func64(f, x):
    """func_i on a float64 array."""
    if f is None or int(f[0]) == F_IDENTITY:
        return x.copy()
    kind = int(f[0])
    with np.errstate(all="ignore"):
        if kind == F_LINEAR:
            return float(np.float32(f[1])) * x + float(np.float32(f[2]))
        if kind == F_GAMMA:
            e = float(np.float32(f[2]))
            return float(np.float32(f[1])) * _each(lambda v: pow64(v, e), x) + float(np.float32(f[3]))
        v = np.array(f[1], np.float32).astype(np.float64)
        N = len(v) - 1 if kind == F_TABLE else len(v)
        if N == 0:
            return np.full(x.shape, v[0])
        c = _clamp01(x)
        k = np.minimum((c * float(N)).astype(np.int64), N - 1)
        if kind == F_DISCRETE:
            return v[k]
        return v[k] + ((x - k.astype(np.float64) / float(N)) * float(N)) * (v[k + 1] - v[k])


def _f16_bits(y):
    with np.errstate(all="ignore"):
        bits = y.astype(np.float16).view(np.uint16).copy()
    bits[np.isnan(y)] = NAN16
    return bits


def _norm(f):
    if f is None or int(f[0]) == F_IDENTITY:
        return None
    return (int(f[0]),) + tuple(tuple(float(np.float32(v)) for v in p) if isinstance(p, (tuple, list, np.ndarray)) else float(np.float32(p))
                                for p in f[1:])


@functools.lru_cache(maxsize=None)
def pre_table():
    t = _each(enc, X64).astype(np.float32)
    t[np.isnan(X64)] = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    return t


@functools.lru_cache(maxsize=None)
def _post_table(f, clamp, with_dec, func_after_dec):
    x = X64
    if func_after_dec:  # (a wrong variant: decode first, then the func and the clamp)
        y = func64(f, _each(dec, x) if with_dec else x)
        if clamp:
            y = _clamp01(y)
    else:
        y = func64(f, x)
        if clamp:
            y = _clamp01(y)
        if with_dec:
            y = _each(dec, y)
    bits = _f16_bits(y)
    bits[np.isnan(x)] = NAN16
    return bits


def tables(funcs=None, space=LINEAR, clamp=True, func_after_dec=False):
    """(pre, post, which): dicts channel -> table of the tables that exist (float32 / uint16, 65 536 entries), and the bit mask
    (bit c: PRE_c, bit 4 + i: POST_i)."""
    funcs = (None,) * 4 if funcs is None else tuple(_norm(f) for f in funcs)
    pre = {c: pre_table() for c in range(3)} if space == SRGB else {}
    post = {}
    for i in range(4):
        with_dec = space == SRGB and i < 3
        if funcs[i] is not None or with_dec:
            post[i] = _post_table(funcs[i], bool(clamp), with_dec, func_after_dec)
    which = sum(1 << c for c in pre) | sum(1 << (4 + i) for i in post)
    return pre, post, which


def texels(bits, matrix=None, funcs=None, space=LINEAR, clamp=True, variant=None):
    """The rule on an array (..., 4) of f16 bit patterns; returns the same shape, uint16."""
    assert variant is None or variant in VARIANTS
    bits = np.ascontiguousarray(bits, np.uint16)
    M = np.asarray(IDENTITY if matrix is None else matrix, np.float32).reshape(4, 5)
    pre, post, _ = tables(funcs, space, clamp, func_after_dec=variant == "func_after_dec")
    step = mul_add32 if variant == "unfused" else fmaf32
    with np.errstate(all="ignore"):
        t = bits.view(np.float16).astype(np.float32)
        for c in range(4 if variant == "enc_alpha" and space == SRGB else 3):
            if space == SRGB:
                t[..., c] = pre_table()[bits[..., c]]
        out = np.empty_like(bits)
        for i in range(4):
            if variant == "offset_last":
                m = np.zeros(bits.shape[:-1], np.float32)
            else:
                m = np.full(bits.shape[:-1], M[i, 4], np.float32)
            for k in range(4):
                m = step(M[i, k], t[..., k], m)
            if variant == "offset_last":
                m = (m + M[i, 4]).astype(np.float32)
            if variant == "clamp_after_round":
                m = m.astype(np.float16).astype(np.float32)
            if clamp:
                if variant == "minmax_nan":  # (min and max that hand a NaN on)
                    m = np.minimum(np.maximum(m, np.float32(0.0)), np.float32(1.0))
                else:
                    m = _clamp01(m).astype(np.float32)
            g = m.astype(np.float16).view(np.uint16).copy()
            g[np.isnan(m)] = NAN16
            out[..., i] = post[i][g] if i in post else g
    return out


def apply(src_bits, matrix=None, funcs=None, space=LINEAR, clamp=True, rect=None, dst_bits=None, variant=None):
    """The image jh_color_filter leaves in dst.  src_bits: (H, W, 4) uint16 (a never-written source: all zero).  rect = (x, y, w,
    h) or None: the whole of src.  dst_bits: what dst held -- None: a never-written dst of src's size, transparent black; the
    source itself for a call in place."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    H, W, _ = src_bits.shape
    x, y, w, h = (0, 0, W, H) if rect is None or (rect[2] == 0 and rect[3] == 0) else rect
    out = np.zeros_like(src_bits) if dst_bits is None else np.array(dst_bits, np.uint16)
    if w and h:
        out[y:y + h, x:x + w] = texels(src_bits[y:y + h, x:x + w], matrix, funcs, space, clamp, variant)
    return out


def definition(bits, matrix=None, funcs=None, space=LINEAR, clamp=True):
    """What the rule rounds, wholly in binary64 on finite texels: encode, the plain sum M t + offset, the clamp, the func, the clamp,
    decode -- (..., 4) float64, nothing rounded to binary32 or f16 on the way."""
    bits = np.ascontiguousarray(bits, np.uint16)
    M = np.asarray(IDENTITY if matrix is None else matrix, np.float32).astype(np.float64).reshape(4, 5)
    funcs = (None,) * 4 if funcs is None else tuple(funcs)
    t = bits.view(np.float16).astype(np.float64)
    if space == SRGB:
        t[..., :3] = _each(enc, t[..., :3].reshape(-1)).reshape(t[..., :3].shape)
    out = np.empty(bits.shape, np.float64)
    for i in range(4):
        m = M[i, 4] + M[i, 0] * t[..., 0] + M[i, 1] * t[..., 1] + M[i, 2] * t[..., 2] + M[i, 3] * t[..., 3]
        if clamp:
            m = _clamp01(m)
        y = func64(funcs[i], m)
        if clamp:
            y = _clamp01(y)
        if space == SRGB and i < 3:
            y = _each(dec, y.reshape(-1)).reshape(y.shape)
        out[..., i] = y
    return out
