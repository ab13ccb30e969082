"""-m gpu: jh_blur against the rule of DESIGN.md 5.7 (tests/blur_ref.py) byte for byte -- the battery of tests/blur_cases.py, a
rendered frame, a captured frame -- and the call's frame: its refusals, its profile query, the held-back commands in front of it."""
import ctypes

import numpy as np
import pytest

from jello_amd import BlurEdge, ImageFormat
from jello_amd._lib import CBlurDesc

import blur_cases
import blur_ref
from devmem import DevBuf, Image, _id, target_of
from image_call import (JH_ERR_OOM, assert_same_bits, canary_bits, captured_call, captured_with_the_frame, check_refusals, common_refusals, images,
                        one_query, run_case, scene)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in blur_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.blur: dst is poisoned first (or is the source), the whole of dst is compared -- the rectangle with
    the reference, the texels outside it with what they held."""
    c = blur_cases.BY_NAME[name]
    src_bits = blur_cases.source(c)
    call = lambda src, dst: engine.blur(src.id, c["w"], c["h"], c["sigma"], dst_image_id=None if c["in_place"] else dst.id,  # noqa: E731
                                        edge=BlurEdge(c["edge"]), rect=c["rect"])
    got = run_case(engine, c, call, src_bits, np.full_like(src_bits, blur_cases.POISON), in_place=c["in_place"])
    assert_same_bits(got, blur_cases.expected(name), name)


def test_a_never_written_destination_is_cleared_outside_the_rectangle(engine):
    bits = blur_cases.content("unit", 33, 21, seed=3)
    rect = (5, 4, 20, 9)
    with images(engine, bits, (33, 21)) as (src, dst):
        engine.blur(src.id, 33, 21, (1.0, 2.5), dst_image_id=dst.id, rect=rect)
        got = dst.bits()
    assert np.array_equal(got, blur_ref.blur(bits, (1.0, 2.5), blur_ref.ZERO, rect, None))


@pytest.mark.parametrize("edge", list(BlurEdge))
def test_rendered_scene_in_place(engine, edge):
    """A rendered 64 x 48 frame (a circle and a stroked curve) blurred in place = the reference on the download of the same render."""
    rec, _, _ = engine.render(*scene((64, 48), 3))
    t = rec.target
    plain = target_of(engine, rec)
    assert plain.any()
    engine.blur(t["id"], 64, 48, (2.0, 3.5), edge=edge)
    assert blur_ref.same_bits(target_of(engine, rec), blur_ref.blur(plain, (2.0, 3.5), int(edge)))


def test_captured_with_the_frame(engine):
    """capture(blur=..., surface=...): render, blur in place, blit -- three launches more than the frame alone (rows, columns,
    blit), replayed twice, the bytes of the eager calls."""
    sigma, rect = (3.0, 1.5), (8, 4, 50, 40)
    captured_with_the_frame(engine, scene((64, 48), 3), lambda target, _: engine.blur(target, 64, 48, sigma, edge=BlurEdge.CLAMP, rect=rect),
                            lambda _: dict(blur=dict(sigma=sigma, edge=BlurEdge.CLAMP, rect=rect)),
                            lambda plain: blur_ref.blur(plain, sigma, blur_ref.CLAMP, rect, plain), extra_launches=3)


def test_capture_without_scratch_is_refused_with_advice(engine):
    hip, ctx = engine.hip, engine.ctx
    bits = blur_cases.content("unit", 64, 48, seed=1)
    d = CBlurDesc(2.0, 2.0, 0, 0, 0, 0, 0)
    enqueue = lambda: hip.jh_blur(ctx, img.id, img.id, 64, 48, ctypes.byref(d))  # noqa: E731
    g = None
    with images(engine, bits, 64) as (img, other):
        try:
            engine.trim_scratch()  # the intermediate has to be allocated again
            rc, msg, refused = captured_call(engine, enqueue, clear_first=other.id)
            engine.graph_destroy(refused)
            assert rc == JH_ERR_OOM and msg.startswith("jh_blur: ") and "blur a rectangle of this size once eagerly first" in msg, (rc, msg)
            assert np.array_equal(img.bits(), bits)
            # ... and after that eager call the same capture works
            engine.blur(img.id, 64, 48, 2.0)
            once = img.bits()
            assert blur_ref.same_bits(once, blur_ref.blur(bits, 2.0))
            rc, msg, g = captured_call(engine, enqueue)
            assert rc == 0
            assert np.array_equal(img.bits(), once)  # a capture runs nothing
            engine.replay(g)
            assert blur_ref.same_bits(img.bits(), blur_ref.blur(once, 2.0))
        finally:
            if g is not None:
                engine.graph_destroy(g)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_blur: ", no texel of either image and no byte of
    a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    nan, inf = float("nan"), float("inf")
    with images(engine, canary, canary, (W, H, ImageFormat.RGBA8)) as (src, dst, rgba8):
        def call(s=None, d=None, w=W, h=H, sigma=(1.0, 1.0), edge=0, rect=(0, 0, 0, 0), null=False):
            return hip.jh_blur(ctx, src.id if s is None else s, dst.id if d is None else d, w, h, None if null else ctypes.byref(CBlurDesc(*sigma, edge, *rect)))

        refused = dict(common_refusals(call, rgba8), **{
            "width differs": (lambda: call(w=W + 1), b""),
            "height differs": (lambda: call(h=H - 1), b""),
            "sigma_x negative": (lambda: call(sigma=(-0.5, 1.0)), b""),
            "sigma_y negative": (lambda: call(sigma=(1.0, -1e-20)), b""),
            "sigma_x above 64": (lambda: call(sigma=(64.5, 1.0)), b""),
            "sigma_y infinite": (lambda: call(sigma=(1.0, inf)), b""),
            "sigma_x NaN": (lambda: call(sigma=(nan, 1.0)), b""),
            "sigma_y NaN": (lambda: call(sigma=(1.0, nan)), b""),
            "edge mode 2": (lambda: call(edge=2), b""),
            "edge mode -1": (lambda: call(edge=-1), b""),
        })
        check_refusals(engine, "jh_blur", call, refused, untouched=((src, canary), (dst, canary)),
                       raises=(lambda: engine.blur(src.id, W, H, 65.0),),
                       accepted=(call,))  # (and the same call with nothing wrong is accepted)


def test_the_call_is_one_query_of_the_tree(engine):
    bits = blur_cases.content("unit", 48, 33, seed=2)
    with images(engine, bits) as (img,):
        one_query(engine, "blur", lambda: engine.blur(img.id, 48, 33, (2.0, 1.0)))
        got = img.bits()
    once = blur_ref.blur(bits, (2.0, 1.0))
    assert blur_ref.same_bits(got, blur_ref.blur(once, (2.0, 1.0)))


def test_the_call_launches_what_is_held_back_first(engine):
    """A whole-buffer clear of a buffer of a JlBump's size is held back; a blur that reads or writes that memory -- imported as a
    2 x 2 image -- has to launch it first."""
    hip, ctx = engine.hip, engine.ctx
    ones = np.full((2, 2, 4), 0x3C00, np.uint16)
    bufs = [DevBuf(engine, 32), DevBuf(engine, 32)]
    over = [_id(), _id()]
    plain = [Image(engine, np.full((2, 2, 4), blur_cases.POISON, np.uint16)), Image(engine, ones)]
    try:
        for b, i in zip(bufs, over):
            engine._check(hip.jh_image_import(ctx, i, b.ptr, 2, 2, ImageFormat.RGBA16_FLOAT), "image_import")
        # as the source: without the flush the blur copies the canary
        engine.clear(bufs[0].id)
        engine.blur(over[0], 2, 2, 0.0, dst_image_id=plain[0].id)
        assert not plain[0].bits().any()
        # as the destination: without the flush the clear runs after the blur and wipes it
        engine.clear(bufs[1].id)
        engine.blur(plain[1].id, 2, 2, 0.0, dst_image_id=over[1])
        assert np.array_equal(bufs[1].bytes().view(np.uint16).reshape(2, 2, 4), ones)
    finally:
        for i in over:
            engine.free_image(i)
        for b in bufs + plain:
            b.free()
