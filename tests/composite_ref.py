"""The composite rule of DESIGN.md 5.8 in numpy, written from the rule alone: the reference jh_composite is compared with byte for
byte.  Everything is binary32 (numpy float32 arrays and float32 constants: every operation rounded once, nothing contracted).

  source    (c_s, a_s) = the f16 texel widened; with a tint c_s = tint.rgb (binary32) and a_s = a_s * tint.a; a_s = a_s * opacity;
            p_s = c_s * a_s
  backdrop  (c_b, a_b) = the dst texel widened (a never-written dst: transparent black); p_b = c_b * a_b
  blend     R = blend_mix_compose((p_b, a_b), (p_s, a_s), mix << 8 | compose) -- shared/blend.wgsl as the fine stage applies it:
            Normal + SrcOver is R = p_b * (1 - a_s) + p_s (alpha too); otherwise un-premultiply both by 1 / max(a, 1e-15), mix the
            colours, c_s = mix(c_s, mixed, a_b), and compose with the Porter-Duff factors.
            min / max are IEEE minNum / maxNum -- a NaN operand yields the other one -- with -0 below +0, coded here explicitly.
  store     a_inv = 1 / max(R.a, 1e-6); dst = f16(R.rgb * a_inv + 0.0f), f16(R.a + 0.0f), round to nearest even
  geometry  the source rectangle (sx, sy, sw, sh) (sw == sh == 0: the whole image) is placed with its top-left at the signed
            (dx, dy) of dst and clipped to dst; only those texels are written.

The keyword arguments of `composite` after `dst_bits` build the four WRONG variants the battery has to tell from the rule
(tests/test_composite_spec.py)."""
import numpy as np

from image_ref import fmaf32, fmax, fmin, same_bits  # noqa: F401 (same_bits is part of this module's interface)

F = np.float32
ZERO, ONE, TWO, HALF = F(0.0), F(1.0), F(2.0), F(0.5)
EPSILON = F(1e-15)
STORE_FLOOR = F(1e-6)
N_MIX, N_COMPOSE = 16, 14
MIX_NAMES = ["Normal", "Multiply", "Screen", "Overlay", "Darken", "Lighten", "ColorDodge", "ColorBurn", "HardLight", "SoftLight",
             "Difference", "Exclusion", "Hue", "Saturation", "Color", "Luminosity"]
COMPOSE_NAMES = ["SrcOver", "Copy", "Dest", "Clear", "DestOver", "SrcIn", "DestIn", "SrcOut", "DestOut", "SrcAtop", "DestAtop", "Xor",
                 "Plus", "PlusLighter"]


def _f(a):
    return np.asarray(a, np.float32)


def _mix(a, b, t):
    return a * (ONE - t) + b * t


def _screen(cb, cs):
    return [b + s - (b * s) for b, s in zip(cb, cs)]


def _color_dodge(cb, cs):
    return np.where(cb == 0, ZERO, np.where(cs == 1, ONE, fmin(ONE, cb / (ONE - cs)))).astype(np.float32)


def _color_burn(cb, cs):
    return np.where(cb == 1, ONE, np.where(cs == 0, ZERO, ONE - fmin(ONE, (ONE - cb) / cs))).astype(np.float32)


def _hard_light1(cb, cs):
    scr = TWO * cs - ONE
    a = cb + scr - (cb * scr)
    b = cb * TWO * cs
    return np.where(cs <= HALF, b, a).astype(np.float32)


def _hard_light(cb, cs):
    return [_hard_light1(b, s) for b, s in zip(cb, cs)]


def _soft_light1(cb, cs):
    d = np.where(cb <= F(0.25), ((F(16.0) * cb - F(12.0)) * cb + F(4.0)) * cb, np.sqrt(cb)).astype(np.float32)
    t = cb + (TWO * cs - ONE) * (d - cb)
    f = cb - (ONE - TWO * cs) * cb * (ONE - cb)
    return np.where(cs <= HALF, f, t).astype(np.float32)


def _sat(c):
    return fmax(c[0], fmax(c[1], c[2])) - fmin(c[0], fmin(c[1], c[2]))


def _lum(c):
    return c[0] * F(0.3) + c[1] * F(0.59) + c[2] * F(0.11)


def _clip_color(c):
    l = _lum(c)  # noqa: E741
    n = fmin(c[0], fmin(c[1], c[2]))
    x = fmax(c[0], fmax(c[1], c[2]))
    neg = n < 0
    c = [np.where(neg, l + (((v - l) * l) / (l - n)), v).astype(np.float32) for v in c]
    big = x > 1
    return [np.where(big, l + (((v - l) * (ONE - l)) / (x - l)), v).astype(np.float32) for v in c]


def _set_lum(c, l):  # noqa: E741
    d = l - _lum(c)
    return _clip_color([v + d for v in c])


def _set_sat_inner(cmin, cmid, cmax, s):
    grows = cmax > cmin
    mid = np.where(grows, ((cmid - cmin) * s) / (cmax - cmin), ZERO).astype(np.float32)
    top = np.where(grows, s, ZERO).astype(np.float32)
    return np.zeros_like(mid), mid, top


def _set_sat(c, s):
    r, g, b = c
    r, g, b, s = np.broadcast_arrays(r, g, b, s)
    rg, gb, rb = r <= g, g <= b, r <= b
    # (condition, the order (min, mid, max) the branch passes to set_sat_inner as indices into (r, g, b))
    branches = [(rg & gb, (0, 1, 2)), (rg & ~gb & rb, (0, 2, 1)), (rg & ~gb & ~rb, (2, 0, 1)),
                (~rg & rb, (1, 0, 2)), (~rg & ~rb & gb, (1, 2, 0)), (~rg & ~rb & ~gb, (2, 1, 0))]
    out = [np.zeros(r.shape, np.float32) for _ in range(3)]
    ch = (r, g, b)
    for cond, order in branches:
        res = _set_sat_inner(ch[order[0]], ch[order[1]], ch[order[2]], s)
        for k in range(3):
            out[order[k]] = np.where(cond, res[k], out[order[k]]).astype(np.float32)
    return out


def blend_mix(cb, cs, mode):
    """blend.wgsl:142-195 on lists of three float32 arrays."""
    if mode == 1:
        return [b * s for b, s in zip(cb, cs)]
    if mode == 2:
        return _screen(cb, cs)
    if mode == 3:
        return _hard_light(cs, cb)
    if mode == 4:
        return [fmin(b, s) for b, s in zip(cb, cs)]
    if mode == 5:
        return [fmax(b, s) for b, s in zip(cb, cs)]
    if mode == 6:
        return [_color_dodge(b, s) for b, s in zip(cb, cs)]
    if mode == 7:
        return [_color_burn(b, s) for b, s in zip(cb, cs)]
    if mode == 8:
        return _hard_light(cb, cs)
    if mode == 9:
        return [_soft_light1(b, s) for b, s in zip(cb, cs)]
    if mode == 10:
        return [np.abs(b - s) for b, s in zip(cb, cs)]
    if mode == 11:
        return [b + s - TWO * b * s for b, s in zip(cb, cs)]
    if mode == 12:
        return _set_lum(_set_sat(cs, _sat(cb)), _lum(cb))
    if mode == 13:
        return _set_lum(_set_sat(cb, _sat(cs)), _lum(cb))
    if mode == 14:
        return _set_lum(cs, _lum(cb))
    if mode == 15:
        return _set_lum(cb, _lum(cs))
    return list(cs)


_FACTORS = {1: ("one", "zero"), 2: ("zero", "one"), 0: ("one", "1-as"), 4: ("1-ab", "one"), 5: ("ab", "zero"), 6: ("zero", "as"),
            7: ("1-ab", "zero"), 8: ("zero", "1-as"), 9: ("ab", "1-as"), 10: ("1-ab", "as"), 11: ("1-ab", "1-as"), 12: ("one", "one")}


def blend_compose(cb, cs, ab, as_, mode):
    """blend.wgsl:216-284: (r, g, b, a) as four arrays."""
    if mode == 13:
        return [fmin(ONE, as_ * s + ab * b) for b, s in zip(cb, cs)] + [fmin(ONE, as_ + ab)]
    values = {"one": ONE, "zero": ZERO, "as": as_, "ab": ab, "1-as": ONE - as_, "1-ab": ONE - ab}
    fa, fb = (values[k] for k in _FACTORS.get(mode, ("zero", "zero")))
    as_fa = as_ * fa
    ab_fb = ab * fb
    return [as_fa * s + ab_fb * b for b, s in zip(cb, cs)] + [fmin(as_fa + ab_fb, ONE)]


def blend_mix_compose(backdrop, src, mode, fused_src_over=False):
    """blend.wgsl:288-310 on premultiplied (..., 4) float32 arrays; mode = mix << 8 | compose.  Returns (..., 4) float32."""
    backdrop, src = _f(backdrop), _f(src)
    with np.errstate(all="ignore"):
        b = [backdrop[..., k] for k in range(4)]
        s = [src[..., k] for k in range(4)]
        if (mode & 0x7FFF) == 0:
            k = ONE - s[3]
            if fused_src_over:  # (a wrong variant: the multiply-add contracted)
                out = [fmaf32(b[i], k, s[i]) for i in range(4)]
            else:
                out = [b[i] * k + s[i] for i in range(4)]
            return np.stack(np.broadcast_arrays(*out), axis=-1).astype(np.float32)
        inv_src_a = ONE / fmax(s[3], EPSILON)
        cs = [v * inv_src_a for v in s[:3]]
        inv_backdrop_a = ONE / fmax(b[3], EPSILON)
        cb = [v * inv_backdrop_a for v in b[:3]]
        mixed = blend_mix(cb, cs, mode >> 8)
        cs = [_mix(c, m, b[3]) for c, m in zip(cs, mixed)]
        compose = mode & 0xFF
        if compose == 0:
            out = [_mix(b[i], cs[i], s[3]) for i in range(3)] + [s[3] + b[3] * (ONE - s[3])]
        else:
            out = blend_compose(cb, cs, b[3], s[3], compose)
        return np.stack(np.broadcast_arrays(*out), axis=-1).astype(np.float32)


def texels(src_bits, dst_bits, mix=0, compose=0, opacity=1.0, tint=None, store_floor=STORE_FLOOR, opacity_after_premultiply=False,
           tint_ignores_alpha=False, fused_src_over=False):
    """The rule on texel arrays of one shape: (..., 4) uint16 source and backdrop bits -> (..., 4) uint16."""
    with np.errstate(all="ignore"):
        s = np.ascontiguousarray(src_bits, np.uint16).view(np.float16).astype(np.float32)
        d = np.ascontiguousarray(dst_bits, np.uint16).view(np.float16).astype(np.float32)
        c_s, a_s = s[..., :3], s[..., 3]
        if tint is not None:
            t = np.array(tint, np.float32)
            c_s = np.broadcast_to(t[:3], c_s.shape)
            if not tint_ignores_alpha:
                a_s = a_s * t[3]
        op = F(opacity)
        if opacity_after_premultiply:  # (a wrong variant: the premultiplied colour scaled instead of alpha)
            p_s = (c_s * a_s[..., None]) * op
            a_s = a_s * op
        else:
            a_s = a_s * op
            p_s = c_s * a_s[..., None]
        src = np.concatenate([p_s, a_s[..., None]], axis=-1).astype(np.float32)
        a_b = d[..., 3]
        backdrop = np.concatenate([d[..., :3] * a_b[..., None], a_b[..., None]], axis=-1).astype(np.float32)
        r = blend_mix_compose(backdrop, src, (int(mix) << 8) | int(compose), fused_src_over)
        a_inv = ONE / fmax(r[..., 3], F(store_floor))
        out = np.concatenate([r[..., :3] * a_inv[..., None] + ZERO, r[..., 3:] + ZERO], axis=-1)
        return out.astype(np.float16).view(np.uint16)


def clip(src_size, dst_size, src_rect=None, offset=(0, 0)):
    """The geometry: (sx', sy', dx', dy', w, h) of what is written, all zero when nothing is left; ValueError for a source
    rectangle that is not inside the source image or that is empty in exactly one dimension.  Python integers: no width to run out of."""
    (sw_img, sh_img), (dw, dh) = src_size, dst_size
    sx, sy, sw, sh = (0, 0, 0, 0) if src_rect is None else src_rect
    if sw == 0 and sh == 0:
        sx, sy, sw, sh = 0, 0, sw_img, sh_img
    elif sw == 0 or sh == 0:
        raise ValueError("the source rectangle is empty in one dimension")
    if sx + sw > sw_img or sy + sh > sh_img:
        raise ValueError("the source rectangle is not inside the source image")
    dx, dy = offset
    x0, x1 = max(dx, 0), min(dx + sw, dw)
    y0, y1 = max(dy, 0), min(dy + sh, dh)
    if x1 <= x0 or y1 <= y0:
        return (0, 0, 0, 0, 0, 0)
    return (sx + x0 - dx, sy + y0 - dy, x0, y0, x1 - x0, y1 - y0)


def composite(src_bits, dst_bits, mix=0, compose=0, opacity=1.0, tint=None, src_rect=None, offset=(0, 0), dst_shape=None, **variant):
    """The image jh_composite leaves in dst.  src_bits: (h, w, 4) uint16 f16 bit patterns (a never-written source: all zero);
    dst_bits: what dst held, or None with dst_shape = (H, W): a never-written dst, transparent black.  Returns (H, W, 4) uint16."""
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    out = np.zeros(tuple(dst_shape) + (4,), np.uint16) if dst_bits is None else np.array(dst_bits, np.uint16)
    sx, sy, dx, dy, w, h = clip((src_bits.shape[1], src_bits.shape[0]), (out.shape[1], out.shape[0]), src_rect, offset)
    if w == 0 or h == 0:
        return out
    out[dy:dy + h, dx:dx + w] = texels(src_bits[sy:sy + h, sx:sx + w], out[dy:dy + h, dx:dx + w], mix, compose, opacity, tint, **variant)
    return out
