"""The LUT rule of DESIGN.md 5.23 in numpy, written from the rule alone: the reference jh_lut3d, jh_lut3d_texels and
jh_lut3d_identity are compared with bit for bit.  Nothing here reads include/jello_lut3d.h.

The LUT is an RGBA16F image N texels wide and N^2 high, 2 <= N <= 65.  Entry (i, j, k) indexes (red, green, blue) and is the texel
(x = i, y = j + N k): red varies fastest, the .cube order.  Its r, g, b are the output colour for the input (i, j, k) / (N - 1); its
alpha is ignored.  A never-written LUT reads as zeros.

Per texel, binary32, nothing contracted but the stated fmaf (h_c: the stored f16 of channel c, widened):
  1 clamp     c = h > 0 ? h : 0; c = c < 1 ? c : 1            (np.where on the comparison: NaN and -0 become +0)
  2 position  p = c (N - 1), k = min((int)p, N - 2), f = p - (float)k   (all exact: test_lut3d_spec.py checks every f16 and N)
  3 walk      from V0 = (k_r, k_g, k_b) step +1 along one axis at a time in descending order of fraction: V1, V2, V3 = V0 + (1, 1, 1).
              Ties go r before g before b: a stable sort of the (fraction, axis) pairs.  With f1 >= f2 >= f3 in that order
              w0 = 1 - f1, w1 = f1 - f2, w2 = f2 - f3, w3 = f3.
  4 sum       per colour channel m = w0 V0.c; m = fmaf(w1, V1.c, m); m = fmaf(w2, V2.c, m); m = fmaf(w3, V3.c, m)
              (image_ref.fmaf32).  Zero weights are multiplied, not skipped: 0 x Inf is NaN.
  5 store     f16(m), round to nearest even; a NaN result is any NaN.  Alpha is the source's bit pattern, copied.

`variant` of `texels` builds the WRONG rules the battery has to tell from the rule (tests/test_lut3d_spec.py)."""
import numpy as np

from image_ref import fmaf32, mul_add32, resolve

MIN_SIZE, MAX_SIZE = 2, 65
VARIANTS = ("trilinear", "ties_g_first", "round_index", "wrap_index", "difference_form", "unfused", "skip_zero", "minmax_nan", "alpha_through")
F = np.float32


def size_of(lut_bits):
    """N of a LUT image (N * N, N, 4)."""
    lut_bits = np.asarray(lut_bits)
    n = lut_bits.shape[1]
    assert lut_bits.shape == (n * n, n, 4) and MIN_SIZE <= n <= MAX_SIZE, lut_bits.shape
    return n


def identity(n):
    """The identity LUT image: entry value f16(i / (N - 1)) rounded once from binary64, alpha 1.0."""
    v = (np.arange(n, dtype=np.float64) / float(n - 1)).astype(np.float16).view(np.uint16)
    out = np.empty((n, n, n, 4), np.uint16)  # [k, j, i]
    out[..., 0] = v[None, None, :]
    out[..., 1] = v[None, :, None]
    out[..., 2] = v[:, None, None]
    out[..., 3] = 0x3C00
    return out.reshape(n * n, n, 4)


def _clamp01(v):
    """Compare and select: NaN and -0 become +0."""
    v = np.where(v > 0.0, v, F(0.0))
    return np.where(v < 1.0, v, F(1.0)).astype(F)


def position(bits, n, variant=None):
    """(k, f) of steps 1 and 2 for an array of f16 bit patterns: int64 cell indices and float32 fractions."""
    with np.errstate(all="ignore"):
        h = np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(F)
        c = np.minimum(np.maximum(h, F(0.0)), F(1.0)) if variant == "minmax_nan" else _clamp01(h)  # (min and max that hand a NaN on)
        p = (c * F(n - 1)).astype(F)
        if variant == "round_index":
            k = (p + F(0.5)).astype(F)
            k = np.where(np.isnan(k), F(0.0), k).astype(np.int64)
        else:
            k = np.where(np.isnan(p), F(0.0), p).astype(np.int64)
        k = np.minimum(k, n - 1 if variant == "wrap_index" else n - 2)
        f = (p - k.astype(F)).astype(F)
    return k, f


def walk(f, variant=None):
    """Step 3 on fractions (..., 3): (order, w) -- order (..., 3) the axes 0 = r, 1 = g, 2 = b in the order they are stepped, by an
    explicit stable sort of the (fraction, axis) pairs in descending fraction; w (..., 4) float32."""
    f = np.asarray(f, F)
    flat = f.reshape(-1, 3)
    axes = (1, 0, 2) if variant == "ties_g_first" else (0, 1, 2)  # the order ties are resolved in
    order = np.empty(flat.shape, np.int64)
    for t in range(len(flat)):
        pairs = sorted(((float(flat[t, a]), a) for a in axes), key=lambda pair: -pair[0])  # (sorted is stable: ties keep `axes` order)
        order[t] = [a for _, a in pairs]
    order = order.reshape(f.shape)
    fs = np.take_along_axis(f, order, axis=-1)
    one = F(1.0)
    w = np.stack([one - fs[..., 0], fs[..., 0] - fs[..., 1], fs[..., 1] - fs[..., 2], fs[..., 2]], axis=-1).astype(F)
    return order, w


def _walk_fast(f, ties_g_first=False):
    """walk() for large arrays: numpy's stable argsort of the negated fractions (the axes listed in tie order) -- the same explicit
    stable sort of (fraction, axis) pairs, vectorised; test_lut3d_spec.py holds it against walk()."""
    f = np.asarray(f, F)
    axes = np.array((1, 0, 2) if ties_g_first else (0, 1, 2))
    idx = np.argsort(-f[..., axes], axis=-1, kind="stable")
    order = axes[idx]
    fs = np.take_along_axis(f, order, axis=-1)
    one = F(1.0)
    w = np.stack([one - fs[..., 0], fs[..., 0] - fs[..., 1], fs[..., 1] - fs[..., 2], fs[..., 2]], axis=-1).astype(F)
    return order, w


def vertices(k, order):
    """The four vertices (..., 4, 3) of step 3 from the cell indices (..., 3) and the order of the axes."""
    v = np.repeat(k[..., None, :], 4, axis=-2).copy()
    for step in range(3):
        bump = np.zeros(k.shape, np.int64)
        np.put_along_axis(bump, order[..., step:step + 1], 1, axis=-1)
        v[..., step + 1:, :] += bump[..., None, :]
    return v


def texels(bits, lut_bits, variant=None):
    """The rule on an array (..., 4) of f16 bit patterns under the LUT image lut_bits (N * N, N, 4); returns the same shape, uint16."""
    assert variant is None or variant in VARIANTS
    n = size_of(lut_bits)
    bits = np.ascontiguousarray(bits, np.uint16)
    lut = np.ascontiguousarray(lut_bits, np.uint16).reshape(n, n, n, 4)  # [k, j, i]
    with np.errstate(all="ignore"):
        lutf = lut.view(np.float16).astype(F)
        k, f = position(bits[..., :3], n, variant)
        nchan = 4 if variant == "alpha_through" else 3
        out = bits.copy()
        if variant == "trilinear":
            m = np.zeros(bits.shape[:-1] + (nchan,), F)
            first = True
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        w = ((f[..., 0] if dx else F(1) - f[..., 0]) * (f[..., 1] if dy else F(1) - f[..., 1])).astype(F)
                        w = (w * (f[..., 2] if dz else F(1) - f[..., 2])).astype(F)
                        e = lutf[k[..., 2] + dz, k[..., 1] + dy, k[..., 0] + dx][..., :nchan]
                        m = (w[..., None] * e).astype(F) if first else fmaf32(w[..., None], e, m)
                        first = False
        else:
            order, w = _walk_fast(f, ties_g_first=variant == "ties_g_first")
            v = vertices(k, order)
            if variant == "wrap_index":
                v = np.mod(v, n)
            e = lutf[v[..., 2], v[..., 1], v[..., 0]][..., :nchan]  # (..., 4 vertices, channels)
            if variant == "difference_form":  # V0 + f1 (V1 - V0) + f2 (V2 - V1) + f3 (V3 - V2)
                fs = np.take_along_axis(f, order, axis=-1)
                m = e[..., 0, :]
                for i in range(3):
                    m = fmaf32(fs[..., i:i + 1], (e[..., i + 1, :] - e[..., i, :]).astype(F), m)
            else:
                step = mul_add32 if variant == "unfused" else fmaf32
                m = (w[..., 0:1] * e[..., 0, :]).astype(F)
                if variant == "skip_zero":
                    m = np.where(w[..., 0:1] == 0, F(0.0), m).astype(F)
                for i in range(1, 4):
                    nxt = step(w[..., i:i + 1], e[..., i, :], m)
                    m = np.where(w[..., i:i + 1] == 0, m, nxt).astype(F) if variant == "skip_zero" else nxt
        out[..., :nchan] = m.astype(np.float16).view(np.uint16)
    return out


def apply(src_bits, lut_bits, rect=None, dst_bits=None, variant=None):
    """The image jh_lut3d leaves in dst.  src_bits: (H, W, 4) uint16 (a never-written source: all zero); lut_bits: the LUT image (a
    never-written one: all zero).  rect = (x, y, w, h) or None: the whole of src.  dst_bits: what dst held -- None: a never-written
    dst of src's size, transparent black; the source itself for a call in place."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    x, y, w, h = resolve(src_bits.shape, rect)
    out = np.zeros_like(src_bits) if dst_bits is None else np.array(dst_bits, np.uint16)
    if w and h:
        out[y:y + h, x:x + w] = texels(src_bits[y:y + h, x:x + w], lut_bits, variant)
    return out


def definition(bits, lut_bits):
    """What the rule rounds, in binary64 on finite texels and entries: the tetrahedral interpolation with exact positions and one
    plain sum of the four products -- (..., 3) float64."""
    n = size_of(lut_bits)
    bits = np.ascontiguousarray(bits, np.uint16)
    lut = np.ascontiguousarray(lut_bits, np.uint16).reshape(n, n, n, 4).view(np.float16).astype(np.float64)
    k, f = position(bits[..., :3], n)
    order, w = _walk_fast(f)
    v = vertices(k, order)
    e = lut[v[..., 2], v[..., 1], v[..., 0]][..., :3]
    return (w.astype(np.float64)[..., None] * e).sum(axis=-2)


def trilinear64(bits, lut_bits):
    """binary64 trilinear interpolation of the same table at the same (exact) positions -- (..., 3) float64."""
    n = size_of(lut_bits)
    bits = np.ascontiguousarray(bits, np.uint16)
    lut = np.ascontiguousarray(lut_bits, np.uint16).reshape(n, n, n, 4).view(np.float16).astype(np.float64)
    k, f = position(bits[..., :3], n)
    f = f.astype(np.float64)
    out = np.zeros(bits.shape[:-1] + (3,), np.float64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[..., 0] if dx else 1 - f[..., 0]) * (f[..., 1] if dy else 1 - f[..., 1]) * (f[..., 2] if dz else 1 - f[..., 2])
                out += w[..., None] * lut[k[..., 2] + dz, k[..., 1] + dy, k[..., 0] + dx][..., :3]
    return out
