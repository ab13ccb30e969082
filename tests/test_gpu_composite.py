"""-m gpu: jh_composite against the rule of DESIGN.md 5.8 (tests/composite_ref.py) byte for byte -- the battery of
tests/composite_cases.py, never-written images, a drop shadow on a rendered frame, a captured frame -- and the call's frame: its
refusals, its profile query, the held-back commands in front of it."""
import ctypes

import numpy as np
import pytest

from jello_amd import Compose, ImageFormat, Mix
from jello_amd._lib import CCompositeDesc

import blur_ref
import composite_cases
import composite_ref
from devmem import DevBuf, Image, _id, target_of
from image_call import (assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query,
                        run_case, scene)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in composite_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.composite: the whole of dst is compared -- the placed rectangle with the reference, everything else
    with the poison it held -- and the source is unchanged.  (Among the value cases' texels are the +-0 ties of composite_cases.TIES;
    in this rule the sign of a zero that min / max return cannot reach a stored value, so they hold the orderings of equal
    channels, not the device's ordering of zeros: test_the_devices_min_and_max_are_the_rules asks that directly.)"""
    c = composite_cases.BY_NAME[name]
    call = lambda src, dst: engine.composite(src.id, dst.id, Mix(c["mix"]), Compose(c["compose"]), c["opacity"], c["tint"], c["src_rect"], c["offset"])  # noqa: E731
    got = run_case(engine, c, call, composite_cases.source(c), composite_cases.destination(c))
    assert_same_bits(got, composite_cases.expected(name), name)


def test_the_devices_min_and_max_are_the_rules(engine):
    """The sign of a zero that min / max return cannot reach a value jh_composite stores, so the battery's tie
    entries cannot tell a device that orders zeros differently.  This asks the device directly: fmin_ / fmax_ of dmath.h -- the
    functions blend_rule.h calls -- through the self-test launcher, on every pair of the special values, against the reference's
    explicit minNum / maxNum with -0 below +0, bit for bit (a NaN equal to any NaN)."""
    FP = ctypes.POINTER(ctypes.c_float)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, 0.5, 1e-40, -1e-40, 2.0 ** -24, 65504.0, 1e-15, 1e-6], np.float32)
    a, b = (np.ascontiguousarray(v.ravel()) for v in np.meshgrid(special, special))
    engine.hip.jh_selftest_math.argtypes = [ctypes.c_void_p, ctypes.c_int, FP, FP, FP, ctypes.c_uint32]
    for op, rule in ((14, composite_ref.fmin), (15, composite_ref.fmax)):
        got = np.empty_like(a)
        assert engine.hip.jh_selftest_math(engine.ctx, op, a.ctypes.data_as(FP), b.ctypes.data_as(FP), got.ctypes.data_as(FP), a.size) == 0
        want = rule(a, b)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (op, a[~same], b[~same], got[~same], want[~same])
    ties = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
    assert ties.sum() == 2 and np.signbit(composite_ref.fmin(a, b)[ties]).all() and not np.signbit(composite_ref.fmax(a, b)[ties]).any()


def test_a_never_written_destination_is_cleared_outside_the_rectangle(engine):
    """... and is the transparent backdrop inside it; placed over the whole of dst nothing has to be cleared first."""
    bits = composite_cases.unit(21, 9, seed=3)
    for size, offset in (((33, 21), (5, 4)), ((33, 21), (-3, 17)), ((21, 9), (0, 0)), ((20, 8), (-1, -1))):
        with images(engine, bits, size) as (src, dst):
            engine.composite(src.id, dst.id, Mix.Multiply, Compose.SrcOver, 0.75, offset=offset)
            got = dst.bits()
        want = composite_ref.composite(bits, None, Mix.Multiply, Compose.SrcOver, 0.75, offset=offset, dst_shape=(size[1], size[0]))
        assert_same_bits(got, want, (size, offset))


def test_a_never_written_source_is_transparent_black(engine):
    """Normal + SrcOver leaves the backdrop (by the rule's consequence: its colours where a_b >= 1e-6, 0 where a_b = 0), SrcIn
    erases the rectangle, and a tint colours nothing: the alpha it scales is 0."""
    bits = composite_cases.unit(40, 11, seed=4)
    for mix, compose, tint in ((Mix.Normal, Compose.SrcOver, None), (Mix.Normal, Compose.SrcIn, None), (Mix.Screen, Compose.Xor, (0.5, 0.25, 1.0, 1.0))):
        with images(engine, (17, 6), bits) as (src, dst):
            engine.composite(src.id, dst.id, mix, compose, tint=tint, offset=(3, 2))
            got = dst.bits()
        want = composite_ref.composite(np.zeros((6, 17, 4), np.uint16), bits, mix, compose, tint=tint, offset=(3, 2))
        assert_same_bits(got, want, (mix, compose))


def test_drop_shadow_of_a_rendered_frame(engine):
    """A rendered 64 x 48 frame (a circle and a stroked curve) as the layer: Engine.drop_shadow onto an 80 x 60 target =
    blur_ref, then composite_ref with the tint and the offset, then composite_ref of the layer itself."""
    rec, _, _ = engine.render(*scene((64, 48), 3))
    layer = target_of(engine, rec)
    assert layer.any()
    backdrop = composite_cases.unit(80, 60, seed=5)
    sigma, offset, color = (2.0, 3.5), (7, 5), (0.05, 0.0, 0.1, 0.6)
    with images(engine, backdrop, (64, 48)) as (target, scratch):
        engine.drop_shadow(rec.target["id"], target.id, 64, 48, sigma, offset, color, scratch.id)
        got, blurred = target.bits(), scratch.bits()
        assert np.array_equal(target_of(engine, rec), layer)
    shadow = blur_ref.blur(layer, sigma, blur_ref.ZERO)
    assert blur_ref.same_bits(blurred, shadow)
    want = composite_ref.composite(layer, composite_ref.composite(shadow, backdrop, tint=color, offset=offset))
    assert_same_bits(got, want, "drop shadow")
    assert (want != composite_ref.composite(layer, backdrop)).any()  # (the shadow shows)


def test_captured_with_the_frame(engine):
    """capture(composite=..., surface=...): render, composite an overlay onto the target, blit -- two more kernel launches than the
    plain capture (the composite, the blit); replayed twice, the bytes of the eager calls."""
    what = dict(mix=Mix.Screen, compose=Compose.SrcAtop, opacity=0.625, src_rect=(3, 2, 30, 20), offset=(-5, 33))
    overlay_bits = composite_cases.unit(41, 29, seed=6)
    with images(engine, overlay_bits) as (overlay,):
        captured_with_the_frame(engine, scene((64, 48), 3), lambda target, _: engine.composite(overlay.id, target, **what),
                                lambda _: dict(composite=dict(src=overlay.id, **what)),
                                lambda plain: composite_ref.composite(overlay_bits, plain, **what), extra_launches=2)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_composite: ", no texel of either image and no
    byte of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    nan, inf = float("nan"), float("inf")
    with images(engine, canary, canary, (W, H, ImageFormat.RGBA8)) as (src, dst, rgba8):
        def call(s=None, d=None, null=False, mix=0, compose=0, opacity=1.0, flags=0, tint=(0.0, 0.0, 0.0, 0.0), rect=(0, 0, 0, 0), at=(0, 0)):
            desc = CCompositeDesc(mix, compose, opacity, flags, (ctypes.c_float * 4)(*tint), rect[0], rect[1], rect[2], rect[3], at[0], at[1])
            return hip.jh_composite(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, rects=(("", "source ", "rect"),)), **{
            "source is the destination": (lambda: call(d=src.id), b""),
            "mix 16": (lambda: call(mix=16), b""),
            "Mix.Clip": (lambda: call(mix=int(Mix.Clip)), b""),
            "compose 14": (lambda: call(compose=14), b""),
            "opacity negative": (lambda: call(opacity=-0.25), b""),
            "opacity above 1": (lambda: call(opacity=1.5), b""),
            "opacity NaN": (lambda: call(opacity=nan), b""),
            "tint alpha negative": (lambda: call(flags=1, tint=(0.5, 0.5, 0.5, -0.5)), b""),
            "tint alpha above 1": (lambda: call(flags=1, tint=(0.5, 0.5, 0.5, 1.25)), b""),
            "tint alpha NaN": (lambda: call(flags=1, tint=(0.5, 0.5, 0.5, nan)), b""),
            "tint red infinite": (lambda: call(flags=1, tint=(inf, 0.5, 0.5, 1.0)), b""),
            "tint green NaN": (lambda: call(flags=1, tint=(0.5, nan, 0.5, 1.0)), b""),
            "tint blue -infinite": (lambda: call(flags=1, tint=(0.5, 0.5, -inf, 1.0)), b""),
            "flag bit 1": (lambda: call(flags=2), b""),
            "flag bit 31": (lambda: call(flags=0x80000001, tint=(0.5, 0.5, 0.5, 1.0)), b""),
        })
        check_refusals(engine, "jh_composite", call, refused, untouched=((src, canary), (dst, canary)),
                       raises=(lambda: engine.composite(src.id, dst.id, opacity=2.0), lambda: engine.composite(src.id, src.id)),
                       accepted=(lambda: call(at=(W, 0)), lambda: call(at=(0, -H)), lambda: call(at=(-2 ** 31, 2 ** 31 - 1))))  # placed outside: accepted, nothing to do
        assert np.array_equal(src.bits(), canary) and np.array_equal(dst.bits(), canary)
        assert call(opacity=0.0, tint=(nan, inf, 0.0, 7.0)) == 0  # (the tint is read only with the flag)
        assert np.array_equal(src.bits(), canary)
        assert call(compose=int(Compose.Clear)) == 0  # (and a call with nothing wrong is accepted and does its work)
        assert np.array_equal(src.bits(), canary) and not dst.bits().any()


def test_the_call_is_one_query_of_the_tree(engine):
    a, b = composite_cases.unit(48, 33, seed=7), composite_cases.unit(48, 33, seed=8)
    with images(engine, a, b) as (src, dst):
        one_query(engine, "composite", lambda: engine.composite(src.id, dst.id, opacity=0.5))
        got = dst.bits()
    once = composite_ref.composite(a, b, opacity=0.5)
    assert composite_ref.same_bits(got, composite_ref.composite(a, once, opacity=0.5))


def test_the_call_launches_what_is_held_back_first(engine):
    """A whole-buffer clear of a buffer of a JlBump's size is held back; a composite that reads or writes that memory -- imported as
    a 2 x 2 image -- has to launch it first."""
    hip, ctx = engine.hip, engine.ctx
    ones = np.full((2, 2, 4), 0x3C00, np.uint16)
    bufs = [DevBuf(engine, 32), DevBuf(engine, 32)]
    over = [_id(), _id()]
    plain = [Image(engine, np.full((2, 2, 4), composite_cases.POISON, np.uint16)), Image(engine, ones)]
    try:
        for b, i in zip(bufs, over):
            engine._check(hip.jh_image_import(ctx, i, b.ptr, 2, 2, ImageFormat.RGBA16_FLOAT), "image_import")
        # as the source: without the flush Copy copies the canary
        engine.clear(bufs[0].id)
        engine.composite(over[0], plain[0].id, compose=Compose.Copy)
        assert not plain[0].bits().any()
        # as the destination: without the flush the clear runs after the composite and wipes it
        engine.clear(bufs[1].id)
        engine.composite(plain[1].id, over[1])
        assert np.array_equal(bufs[1].bytes().view(np.uint16).reshape(2, 2, 4), ones)
    finally:
        for i in over:
            engine.free_image(i)
        for b in bufs + plain:
            b.free()
