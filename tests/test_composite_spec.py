"""The composite rule on the CPU: the reference's blend step (tests/composite_ref.py) against the oracle's
blend_mix_compose bit for bit, the whole reference against the float64 W3C formulas, a composed pair of renders against the oracle's
single render of the layered scene, the consequences the rule promises, the geometry (jl_composite_clip) against a Python
restatement, and that the battery (tests/composite_cases.py) tells the rule from four near misses."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, Compose, Fill, Host, Join, Mix, Path, RenderParams, Scene, Stroke
from jello_amd._lib import CCompositeDesc
from oracle import oracle_engine
from oracle.oracle_engine import OracleEngine

import composite_cases
import composite_ref
from test_blend_spec import expected as w3c_expected  # the W3C formulas in float64, written from the specification

MODES = [(mix, compose) for mix in range(composite_ref.N_MIX) for compose in range(composite_ref.N_COMPOSE)]


# ---- (a) the blend step against the oracle ----

def _premultiplied_pairs(n, seed):
    """n pairs of premultiplied texels (n, 4) float32, every value an f16 value, finite and non-negative; alphas 0 and 1 and
    colours 0 and 1 over-represented."""
    rng = np.random.default_rng(seed)

    def one():
        f = rng.random((n, 4), dtype=np.float32)
        pick = rng.random((n, 4))
        f[pick < 0.15] = 0.0
        f[pick > 0.85] = 1.0
        f = f.astype(np.float16).astype(np.float32)  # (c, a) as f16 values
        f[:, :3] = (f[:, :3] * f[:, 3:]).astype(np.float16).astype(np.float32)  # premultiplied, again f16 values
        return np.ascontiguousarray(f)
    return one(), one()


def test_blend_step_equals_the_oracles(built):
    """All 224 modes x 4 000 pairs: equal as values -- the same bits, or both zero, or both NaN."""
    L = oracle_engine.lib()
    L.oracle_blend_mix_compose.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]  # (float[4] each)
    L.oracle_blend_mix_compose.restype = None
    n = 4000
    bg, fg = _premultiplied_pairs(n, seed=11)
    out = np.empty((n, 4), np.float32)
    for mix, compose in MODES:
        mode = mix << 8 | compose
        pb, pf, po = bg.ctypes.data, fg.ctypes.data, out.ctypes.data
        for at in range(0, 16 * n, 16):
            L.oracle_blend_mix_compose(pb + at, pf + at, mode, po + at)
        got = composite_ref.blend_mix_compose(bg, fg, mode)
        same = (got.view(np.uint32) == out.view(np.uint32)) | ((got == 0) & (out == 0)) | (np.isnan(got) & np.isnan(out))
        if not same.all():
            i = int(np.argwhere(~same)[0][0])
            pytest.fail("%s + %s: %d of %d values differ; first: backdrop %s, source %s: reference %s, oracle %s" % (
                composite_ref.MIX_NAMES[mix], composite_ref.COMPOSE_NAMES[compose], int((~same).sum()), same.size, bg[i], fg[i], got[i], out[i]))


# ---- (b) the reference against the W3C formulas ----

def _f16_ulp(v):
    a = np.maximum(np.abs(v), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


W3C_TEXELS = [((0.8125, 0.3125, 0.125, 1.0), (0.1875, 0.625, 0.875, 1.0)),
              ((0.25, 0.5, 0.75, 0.625), (0.875, 0.125, 0.375, 0.75)),
              ((0.125, 0.125, 0.125, 0.875), (0.9375, 0.875, 0.1875, 0.5)),
              ((0.625, 0.1875, 0.6875, 1.0), (0.3125, 0.3125, 0.3125, 1.0)),
              ((0.0, 0.4375, 1.0, 0.25), (1.0, 0.0, 0.5625, 0.375)),
              ((0.75, 0.0625, 0.4375, 0.0625), (0.3125, 0.9375, 0.5, 0.03125)),   # small alphas: a_o down to 2^-9 (SrcIn)
              ((0.5, 0.8125, 0.25, 2.0 ** -7), (0.6875, 0.375, 0.125, 1.0)),
              ((0.4375, 0.25, 0.9375, 1.0), (0.1875, 0.5625, 0.8125, 2.0 ** -6))]  # (backdrop, source), un-premultiplied; every value an f16 value


@pytest.mark.parametrize("opacity", [1.0, 0.5])
def test_reference_against_the_w3c_formulas(opacity):
    """Every mix mode with every operator but PlusLighter (the specification writes it without the blend term; the reference's
    PlusLighter is held through the oracle comparison above).  The inputs are f16 values, so both sides start from the same numbers.
    The tolerance is the f16 quantisation of the output plus what the binary32 operations in front of it leave, which is counted
    here per stage for the longest route, a hue mode: un-premultiply 2 (a division, a product), sat 1, set_sat 3, lum 5, set_lum 2
    and its clip_color 5 + 4 + 4, the mix with the backdrop alpha 4, the Porter-Duff factors 3 and the two weighted products and their
    sum 3, the store's division and product 2: 42 roundings, taken as 64.  Each rounds a colour of magnitude at most 4 (inputs are
    in [0, 1]; the soft-light polynomial's 16 b - 12 is the largest intermediate) by 2^-24 of it, so a blended colour carries at most
    64 * 4 * 2^-24 = 2^-16.  The output is a sum of such colours with non-negative weights (a_s F_a, a_b F_b) that add up to the output
    alpha a_o, divided by a_o: the weights cancel, so the colour's error does not grow as a_o shrinks, and the weights' own relative
    roundings are among the 64.  The rounding to f16 moves the computed value by half an f16 ulp of it, at most one f16 ulp of
    the exact value.  So |got - want| <= ulp_f16(want) + 2^-16 for colour and alpha alike, at every a_o the store does not floor
    (a_o >= 1e-6; below it -- here only a_o = 0 -- the colour is not defined and only alpha is held)."""
    worst = 0.0
    for mix, compose in MODES:
        if compose == Compose.PlusLighter:
            continue
        for backdrop, source in W3C_TEXELS:
            s = np.array([source], np.float16).view(np.uint16)
            d = np.array([backdrop], np.float16).view(np.uint16)
            got = composite_ref.texels(s, d, mix, compose, opacity)[0].view(np.float16).astype(np.float64)
            want = np.array(w3c_expected(Mix(mix), Compose(compose), backdrop, source, opacity))
            a_o = want[3]
            bound = _f16_ulp(want) + 2.0 ** -16
            err = np.abs(got - want)
            held = slice(0, 4) if a_o >= 1e-6 else slice(3, 4)
            worst = max(worst, float((err[held] / bound[held]).max()))
            assert np.all(err[held] <= bound[held]), (Mix(mix).name, Compose(compose).name, backdrop, source, got, want)
    print("max err / bound:", worst)


# ---- (c) a layered scene ----

W, H = 64, 48


def _backdrop(s):
    s.fill(Fill.NonZero, None, Brush.solid((0.9, 0.4, 0.1, 1.0)), None, Path.circle(24, 20, 13))
    s.fill(Fill.NonZero, None, Brush.solid((0.2, 0.7, 0.3, 0.6)), None, Path.rect(30.5, 8.25, 58.5, 40.75))


def _layer(s):
    curve = Path().move_to(6, 40).cubic_to(20, 2, 44, 46, 58, 8)
    s.stroke(Stroke(5, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None, curve)
    s.fill(Fill.NonZero, None, Brush.solid((0.95, 0.9, 0.2, 0.5)), None, Path.circle(40, 26, 10.5))


def _oracle_render(build):
    s = Scene()
    build(s)
    rec = Host().record(s, RenderParams(W, H))  # transparent base colour
    o = OracleEngine()
    o.run(rec)
    return o.target(rec).reshape(H, W, 4).copy()


def _layered(s):
    _backdrop(s)
    s.push_layer(Mix.Normal, Compose.SrcOver, 1.0, None, Path.rect(0, 0, W, H))
    _layer(s)
    s.pop_layer()


def test_two_renders_composed_equal_the_layered_render(built):
    """Normal + SrcOver.  The single render blends the binary32 layer (p_s, a_s) onto the binary32 backdrop (p_b, a_b):
    R = p (1 - a_s) + p_s for colour and alpha, o = f16(R_rgb / R_a), f16(R_a).  The composed pair goes through the same operations
    on the two stored images, whose texels are f16(p / a), f16(a): with u = 2^-11 (half an f16 ulp, relative) and t = 2^-25 (half
    the f16 subnormal spacing, absolute) a stored colour c' is within u |c| + t of c and a stored alpha within u a + t, so the
    premultiplied value the reference forms, c' a', is within  e(p) = 2 u |p| + t (|c| + a)  of p to first order, and alpha within
    e(a) = u a + t.  Through R:  |dR_rgb| <= e(p_b) (1 - a_s) + |p_b| e(a_s) + e(p_s)   and   |dR_a| <= e(a_b) (1 - a_s) + a_b e(a_s) + e(a_s).
    The stored colour is the quotient:  |do| <= (|dR_rgb| + |o| |dR_a|) / R_a, and both sides round to f16 once, half an ulp each:
        |composed - single| <= (|dR_rgb| + |o| |dR_a|) / max(R_a, 1e-6) + ulp_f16(o)        alpha: |dR_a| + ulp_f16(R_a).
    The bound is evaluated with the stored values for the exact ones, and multiplied by 1 + 2^-8 for that substitution, the second-order
    terms and the binary32 roundings (2^-24 relative each, a few dozen) -- all far below the f16 terms."""
    backdrop, layer, single = _oracle_render(_backdrop), _oracle_render(_layer), _oracle_render(_layered)
    composed = composite_ref.composite(layer, backdrop)
    f = lambda bits: bits.view(np.float16).astype(np.float64)  # noqa: E731
    b, s, one, two = f(backdrop), f(layer), f(single), f(composed)
    u, t = 2.0 ** -11, 2.0 ** -25
    cb, ab, cs, as_ = b[..., :3], b[..., 3:], s[..., :3], s[..., 3:]
    pb, ps = np.abs(cb) * ab, np.abs(cs) * as_
    e_pb, e_ps = 2 * u * pb + t * (np.abs(cb) + ab), 2 * u * ps + t * (np.abs(cs) + as_)
    e_ab, e_as = u * ab + t, u * as_ + t
    d_rgb = e_pb * (1 - as_) + pb * e_as + e_ps
    d_a = e_ab * (1 - as_) + ab * e_as + e_as
    r_a = np.maximum(one[..., 3:], 1e-6)
    bound = np.concatenate([(d_rgb + np.abs(one[..., :3]) * d_a) / r_a + _f16_ulp(one[..., :3]), d_a + _f16_ulp(one[..., 3:])], axis=-1) * (1 + 2.0 ** -8)
    err = np.abs(two - one)
    covered = (ab[..., 0] > 0) & (as_[..., 0] > 0)
    assert covered.sum() > 200 and ((as_[..., 0] > 0) & (as_[..., 0] < 1)).sum() > 50  # (the scene overlaps, with partial coverage)
    print("max err / bound:", float((err / bound).max()), "over", int(covered.sum()), "texels under both;",
          int((one != two).any(axis=-1).sum()), "texels differ")
    assert np.all(err <= bound)


# ---- (d) consequences and geometry ----

def _values():
    return composite_cases.value_pair()


def test_opacity_zero_gives_the_backdrop_back():
    """Normal + SrcOver with a_s = 0 (the opacity, or the source): k = 1 - 0 = 1, R = p_b * 1 + 0 = p_b, exactly.  p_b = c_b a_b is
    exact (two f16 values: 11 + 11 bits).  a_inv = fl(1 / a_b) and fl(p_b * a_inv) are two binary32 roundings, each within 2^-24
    relative: the stored colour is within 2^-23 (1 + 2^-24) of c_b, and f16 values are 2^-11 |c_b| or more apart (2^-10 relative to
    the binade's base, subnormals absolutely 2^-24 and exact here) -- so it rounds back to c_b.  That needs a_b >= 1e-6, the
    store's floor; alpha is R.a = a_b itself.  A -0 comes out as +0.  (Source texels have to be finite: Inf * 0 is a NaN.)"""
    c = composite_cases.BY_NAME["random_Normal_op0.3_plain"]
    for (src, dst), enough in ((_values(), 60), ((composite_cases.source(c)[:33, :257], composite_cases.destination(c)[3:36, 21:278]), 5000)):
        finite = ((dst & 0x7FFF) <= 0x7C00).all(axis=-1) & ((dst[..., :3] & 0x7FFF) < 0x7C00).all(axis=-1)  # no NaN, no infinite colour
        finite &= ((src & 0x7FFF) < 0x7C00).all(axis=-1)  # (an infinite or NaN source value times 0 is a NaN, not 0)
        a_b = dst[..., 3].view(np.float16).astype(np.float32)
        held = finite & (a_b >= 1e-6) & (a_b < 65504)
        assert held.sum() > enough
        want = np.where(dst == 0x8000, np.uint16(0), dst)
        for got in (composite_ref.composite(src, dst, opacity=0.0), composite_ref.composite(np.zeros_like(src), dst),
                    composite_ref.composite(src, dst, opacity=0.0, tint=(1.5, 0.2, 2.25, 1.0))):
            if not np.array_equal(got[held], want[held]):
                bad = np.argwhere((got != want).any(axis=-1) & held)[0]
                pytest.fail("texel %s: %s became %s" % (tuple(bad), dst[tuple(bad)], got[tuple(bad)]))


def test_a_transparent_backdrop_texel_loses_its_colour():
    """a_b = 0: p_b = c_b * 0 = 0 for a finite colour, and with a transparent source R = 0: every channel is stored as +0."""
    src, dst = _values()
    finite = ((dst[..., :3] & 0x7FFF) < 0x7C00).all(axis=-1) & ((src & 0x7FFF) < 0x7C00).all(axis=-1)
    clear = finite & ((dst[..., 3] & 0x7FFF) == 0)
    assert clear.sum() > 10 and (dst[clear][:, :3] != 0).any()
    got = composite_ref.composite(src, dst, opacity=0.0)
    assert not got[clear].any()


def test_clear_clears_the_rectangle_and_nothing_else():
    """Compose.Clear: both factors are 0, R = 0 for finite texels; outside the placed rectangle nothing is written -- also by Copy and
    SrcIn, which would erase the backdrop where the layer is absent: the layer is its rectangle."""
    src = composite_cases.unit(9, 5, 1)
    dst = composite_cases.unit(20, 11, 2)
    for mix in (0, 1, 12):
        got = composite_ref.composite(src, dst, mix, Compose.Clear, offset=(4, 3))
        assert not got[3:8, 4:13].any()
        got[3:8, 4:13] = dst[3:8, 4:13]
        assert np.array_equal(got, dst)
    for compose in (Compose.Copy, Compose.SrcIn, Compose.DestIn, Compose.SrcOut, Compose.DestAtop):
        got = composite_ref.composite(src, dst, 0, compose, src_rect=(1, 1, 7, 3), offset=(-2, 9))  # clipped at the left and the bottom
        changed = (got != dst).any(axis=-1)
        assert changed[9:11, 0:5].any() and not changed[:9].any() and not changed[:, 5:].any()


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def test_clip_against_a_python_restatement(built):
    """jl_composite_clip (include/jello_composite.h compiled by the host twin) against composite_ref.clip (Python integers), per axis
    over offsets {INT32_MIN, -w - 1, -w, -1, 0, 1, W - 1, W, INT32_MAX} and sizes {1, 2, 0xffffffff} of source, rectangle and dst."""
    sizes = (1, 2, 0xFFFFFFFF)
    n = 0
    for src_w in sizes:
        for dst_w in sizes:
            rects = {(0, 0)} | {(sx, sw) for sw in sizes for sx in (0, 1, src_w - sw) if sw <= src_w and 0 <= sx <= src_w - sw}
            for sx, sw in sorted(rects):
                w = sw or src_w
                for d in (INT32_MIN, -w - 1, -w, -1, 0, 1, dst_w - 1, dst_w, INT32_MAX):
                    if not INT32_MIN <= d <= INT32_MAX:
                        continue
                    # the same numbers on the x axis (y trivial) and on the y axis (x trivial)
                    for src_size, dst_size, rect, off in (((src_w, 3), (dst_w, 2), (sx, 1, sw, 2 if sw else 0), (d, -1)),
                                                          ((3, src_w), (2, dst_w), (1, sx, 2 if sw else 0, sw), (-1, d))):
                        want = composite_ref.clip(src_size, dst_size, rect, off)
                        assert jello_amd.composite_clip(src_size, dst_size, rect, off) == want, (src_size, dst_size, rect, off)
                        n += 1
    assert n > 300
    assert jello_amd.composite_clip((5, 4), (3, 3)) == (0, 0, 0, 0, 3, 3)
    assert jello_amd.composite_clip((5, 4), (3, 3), None, (3, 0)) == (0, 0, 0, 0, 0, 0)
    assert jello_amd.composite_clip((0, 0), (3, 3)) == (0, 0, 0, 0, 0, 0)  # an image without texels: nothing to place


def test_clip_refuses_a_bad_source_rectangle(built):
    for rect in ((0, 0, 0, 2), (0, 0, 2, 0), (4, 0, 2, 1), (0, 3, 1, 2), (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2), (0, 0, 6, 1), (5, 4, 1, 1)):
        with pytest.raises(ValueError):
            jello_amd.composite_clip((5, 4), (8, 8), rect)
        with pytest.raises(ValueError):
            composite_ref.clip((5, 4), (8, 8), rect)
    L = jello_amd.load_host()
    assert L.jl_composite_clip(5, 4, 0, 0, 0, 0, 0, 0, 8, 8, None) == -1


def test_the_abi_has_the_call(built):
    hip = jello_amd.load_host().hip
    assert hip.jh_composite.argtypes[3]._type_ is CCompositeDesc
    assert hip.jh_composite(None, 1, 2, None) == -1  # JH_ERR_INVALID without a context


# ---- (e) sensitivity ----

VARIANTS = {"store_floor_1e-15": {"store_floor": 1e-15}, "opacity_after_premultiply": {"opacity_after_premultiply": True},
            "tint_ignores_alpha": {"tint_ignores_alpha": True}, "fused_src_over": {"fused_src_over": True}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_battery_tells_the_rule_from_a_near_miss(variant):
    """Each wrong variant differs from the reference in at least one value of at least one case of the battery (the search stops at
    the first such case; the count of cases tried is printed)."""
    tried = 0
    for c in composite_cases.RANDOM + composite_cases.TINTED + composite_cases.VALUES[:14]:
        tried += 1
        wrong = composite_ref.composite(composite_cases.source(c), composite_cases.destination(c), c["mix"], c["compose"], c["opacity"], c["tint"],
                                        c["src_rect"], c["offset"], **VARIANTS[variant])
        if not composite_ref.same_bits(wrong, composite_cases.expected(c["name"])):
            print(variant, "differs on", c["name"], "after", tried, "cases")
            return
    pytest.fail("no case of the battery tells the variant '%s' from the rule: add a case" % variant)


def test_the_battery_covers_what_it_claims():
    names = set(composite_cases.BY_NAME)
    assert len(composite_cases.VALUES) == 224 and len(names) == len(composite_cases.CASES)
    geo = composite_cases.GEOMETRY
    for W_ in (1, 2, 3, 511, 512, 513, 1025):
        for H_ in (1, 3):
            for mix in (0, 1):
                assert any(c["dst_size"] == (W_, H_) and c["mix"] == mix for c in geo)
    clips = [composite_ref.clip(c["src_size"], c["dst_size"], c["src_rect"], c["offset"]) for c in geo]
    assert any(r[4] == 0 for r in clips)                                                   # fully outside
    for dx_par in (0, 1):
        for rel_par in (0, 1):                                                             # dx and sx - dx, even and odd
            assert any(r[4] and r[2] % 2 == dx_par and (r[0] - r[2]) % 2 == rel_par for r in clips)
    assert any(c["offset"][0] < 0 for c in geo) and any(c["offset"][1] < 0 for c in geo)
    assert any(c["offset"][0] + c["src_size"][0] > c["dst_size"][0] for c in geo) and any(c["offset"][1] + c["src_size"][1] > c["dst_size"][1] for c in geo)
    assert any(c["src_size"][0] % 2 == 1 for c in geo) and any(c["src_rect"] for c in geo)
    assert any(c["src_size"][0] > c["dst_size"][0] and c["src_size"][1] > c["dst_size"][1] for c in geo)
    src, dst = composite_cases.value_pair()
    for img in (src, dst):
        assert set(composite_cases.COLOURS) <= set(img[..., :3].ravel().tolist()) and set(composite_cases.ALPHAS) <= set(img[..., 3].ravel().tolist())
    pairs = set(zip(src[..., 3].ravel().tolist(), dst[..., 3].ravel().tolist()))
    assert len(pairs) >= 81
    assert {c["opacity"] for c in composite_cases.TINTED} == {0.0, 0.5, 1.0} and any(c["tint"] and max(c["tint"][:3]) > 1 for c in composite_cases.TINTED)
