"""-m gpu: jh_morphology against the rule of DESIGN.md 5.11 (tests/morph_ref.py) byte for byte -- the battery of
tests/morph_cases.py, never-written images, a rendered frame, Engine.outline and drop_shadow(spread=...), a captured frame -- and
the call's frame: its refusals, its profile query."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import ImageFormat, MorphEdge, MorphOp
from jello_amd._lib import CMorphDesc

import blur_ref
import composite_cases
import composite_ref
import morph_cases
import morph_ref
from devmem import target_of
from image_call import (JH_ERR_OOM, assert_same_bits, canary_bits, captured_call, captured_with_the_frame, check_refusals, common_refusals, images,
                        one_query, run_case, scene)

pytestmark = pytest.mark.gpu

MORPH_LAUNCHES = 3  # rows, block prefix, block suffix + store (include/jello_hip.h)


@pytest.mark.parametrize("name", [c["name"] for c in morph_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.morphology: dst is poisoned first (or is the source), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held -- and the source of a call into a second image is only read."""
    c = morph_cases.BY_NAME[name]
    src_bits = morph_cases.source(c)
    call = lambda src, dst: engine.morphology(src.id, None if c["in_place"] else dst.id, op=MorphOp(c["op"]), radius=c["radius"],  # noqa: E731
                                              edge=MorphEdge(c["edge"]), rect=c["rect"], premultiplied=not c["flags"])
    got = run_case(engine, c, call, src_bits, np.full_like(src_bits, morph_cases.POISON), in_place=c["in_place"])
    assert_same_bits(got, morph_cases.expected(name), name)


def test_a_never_written_destination_is_cleared_outside_the_rectangle(engine):
    bits = morph_cases.content("unit", 33, 21, seed=3)
    rect = (5, 4, 20, 9)
    with images(engine, bits, (33, 21)) as (src, dst):
        engine.morphology(src.id, dst.id, op=MorphOp.ERODE, radius=(1, 2), edge=MorphEdge.CLAMP, rect=rect)
        got = dst.bits()
    assert_same_bits(got, morph_ref.morph(bits, morph_ref.ERODE, (1, 2), morph_ref.CLAMP, 0, rect, None), "a never-written destination")


def test_a_never_written_source_reads_as_transparent_black(engine):
    with images(engine, (33, 21), np.full((21, 33, 4), morph_cases.POISON, np.uint16)) as (src, dst):
        engine.morphology(src.id, dst.id, op=MorphOp.DILATE, radius=3, premultiplied=False)
        got = dst.bits()
    assert not got.any()


@pytest.mark.parametrize("op", list(MorphOp))
def test_rendered_scene_in_place(engine, op):
    """A rendered 64 x 48 frame (a circle and a stroked curve) in place = the reference on the download of the same render."""
    rec, _, _ = engine.render(*scene((64, 48), 3))
    plain = target_of(engine, rec)
    assert plain.any()
    engine.morphology(rec.target["id"], op=op, radius=(2, 3))
    got, want = target_of(engine, rec), morph_ref.morph(plain, int(op), (2, 3), morph_ref.ZERO)
    assert_same_bits(got, want, op.name)
    assert (want != plain).any()


def test_outline_of_a_rendered_frame(engine):
    """Engine.outline onto an 80 x 60 target = morph_ref (dilate, ZERO), composite_ref with the tint, composite_ref of the layer."""
    rec, _, _ = engine.render(*scene((64, 48), 3))
    layer = target_of(engine, rec)
    backdrop = composite_cases.unit(80, 60, seed=5)
    color = (0.0, 0.6, 0.2, 0.9)
    with images(engine, backdrop, (64, 48)) as (target, scratch):
        engine.outline(rec.target["id"], target.id, 2, color, scratch.id)
        got, grown = target.bits(), scratch.bits()
        assert np.array_equal(target_of(engine, rec), layer)
    halo = morph_ref.morph(layer, morph_ref.DILATE, 2, morph_ref.ZERO)
    assert_same_bits(grown, halo, "the halo")
    want = composite_ref.composite(layer, composite_ref.composite(halo, backdrop, tint=color))
    assert_same_bits(got, want, "the outline")
    assert (want != composite_ref.composite(layer, backdrop)).any()  # (the outline shows)


def test_drop_shadow_with_spread_and_without(engine):
    """spread=3: the layer dilated into the scratch, the scratch blurred in place, then the two composites -- against morph_ref,
    blur_ref and composite_ref.  The default spread: the bytes of the three calls drop_shadow has always made."""
    rec, _, _ = engine.render(*scene((64, 48), 3))
    layer = target_of(engine, rec)
    backdrop = composite_cases.unit(80, 60, seed=5)
    sigma, offset, color = (2.0, 3.5), (7, 5), (0.05, 0.0, 0.1, 0.6)
    got = {}
    for spread in (3, 0, None):
        with images(engine, backdrop, (64, 48)) as (target, scratch):
            if spread is None:  # the three calls, spelled out
                engine.blur(rec.target["id"], 64, 48, sigma, dst_image_id=scratch.id, edge=jello_amd.BlurEdge.ZERO)
                engine.composite(scratch.id, target.id, tint=color, offset=offset)
                engine.composite(rec.target["id"], target.id)
            elif spread == 0:
                engine.drop_shadow(rec.target["id"], target.id, 64, 48, sigma, offset, color, scratch.id)
            else:
                engine.drop_shadow(rec.target["id"], target.id, 64, 48, sigma, offset, color, scratch.id, spread=spread)
            got[spread] = (target.bits(), scratch.bits())
            assert np.array_equal(target_of(engine, rec), layer)
    assert np.array_equal(got[0][0], got[None][0]) and np.array_equal(got[0][1], got[None][1])
    plain_shadow = blur_ref.blur(layer, sigma, blur_ref.ZERO)
    assert blur_ref.same_bits(got[0][1], plain_shadow)
    shadow = blur_ref.blur(morph_ref.morph(layer, morph_ref.DILATE, 3, morph_ref.ZERO), sigma, blur_ref.ZERO)
    assert_same_bits(got[3][1], shadow, "the shadow")
    want = composite_ref.composite(layer, composite_ref.composite(shadow, backdrop, tint=color, offset=offset))
    assert_same_bits(got[3][0], want, "the target")
    assert (shadow != plain_shadow).any()


def test_captured_with_the_frame(engine):
    """capture(morphology=..., surface=...): render, dilate in place, blit -- replayed twice, the bytes of the eager calls, and
    MORPH_LAUNCHES + 1 more kernel nodes than the plain capture."""
    what = dict(op=MorphOp.DILATE, radius=(3, 5), edge=MorphEdge.CLAMP, rect=(8, 4, 50, 40))
    captured_with_the_frame(engine, scene((64, 48), 3), lambda target, _: engine.morphology(target, **what), lambda _: dict(morphology=what),
                            lambda plain: morph_ref.morph(plain, morph_ref.DILATE, (3, 5), morph_ref.CLAMP, 0, what["rect"], plain),
                            extra_launches=MORPH_LAUNCHES + 1)


def test_capture_without_scratch_is_refused_with_advice(engine):
    hip, ctx = engine.hip, engine.ctx
    bits = morph_cases.content("unit", 64, 48, seed=1)
    d = CMorphDesc(1, 0, 1, 2, 2, 0, 0, 0, 0)
    enqueue = lambda: hip.jh_morphology(ctx, img.id, img.id, ctypes.byref(d))  # noqa: E731
    g = None
    with images(engine, bits) as (img,):
        try:
            engine.trim_scratch()  # the planes have to be allocated again
            rc, msg, refused = captured_call(engine, enqueue)
            engine.graph_destroy(refused)
            assert rc == JH_ERR_OOM and msg.startswith("jh_morphology: ") and "once eagerly first" in msg, (rc, msg)
            assert np.array_equal(img.bits(), bits)
            # ... the context stays usable, and after that eager call the same capture works
            engine.morphology(img.id, radius=2, premultiplied=False)
            once = img.bits()
            assert np.array_equal(once, morph_ref.morph(bits, morph_ref.DILATE, 2, morph_ref.ZERO, morph_ref.STRAIGHT))
            rc, msg, g = captured_call(engine, enqueue)
            assert rc == 0
            assert np.array_equal(img.bits(), once)  # a capture runs nothing
            engine.replay(g)
            assert np.array_equal(img.bits(), morph_ref.morph(once, morph_ref.DILATE, 2, morph_ref.ZERO, morph_ref.STRAIGHT))
        finally:
            if g is not None:
                engine.graph_destroy(g)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_morphology: ", no texel of any image and no byte
    of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    with images(engine, canary, canary, canary_bits(W + 1, H), (W, H, ImageFormat.RGBA8)) as (src, dst, wider, rgba8):
        def call(s=None, d=None, head=(1, 0, 0, 1, 1), rect=(0, 0, 0, 0), null=False):
            return hip.jh_morphology(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(CMorphDesc(*head, *rect)))

        refused = dict(common_refusals(call, rgba8), **{
            "sizes differ": (lambda: call(d=wider.id), b""),
            "op 2": (lambda: call(head=(2, 0, 0, 1, 1)), b""),
            "op -1": (lambda: call(head=(-1, 0, 0, 1, 1)), b""),
            "edge 2": (lambda: call(head=(1, 2, 0, 1, 1)), b""),
            "edge -1": (lambda: call(head=(1, -1, 0, 1, 1)), b""),
            "flag bit 1": (lambda: call(head=(1, 0, 2, 1, 1)), b""),
            "flag bit 31": (lambda: call(head=(1, 0, 0x80000001, 1, 1)), b""),
            "radius_x 256": (lambda: call(head=(1, 0, 0, 256, 1)), b""),
            "radius_y 256": (lambda: call(head=(1, 0, 0, 1, 256)), b""),
            "radius_x 2^32 - 1": (lambda: call(head=(1, 0, 0, 0xFFFFFFFF, 1)), b""),
        })
        check_refusals(engine, "jh_morphology", call, refused, untouched=((src, canary), (dst, canary), (wider, canary_bits(W + 1, H))),
                       raises=(lambda: engine.morphology(src.id, dst.id, radius=256), lambda: engine.morphology(src.id, dst.id, rect=(8, 0, 9, 4))),
                       accepted=(call,))  # (and the same call with nothing wrong is accepted)


def test_the_call_is_one_query_of_the_tree(engine):
    bits = morph_cases.content("unit", 48, 33, seed=2)
    with images(engine, bits) as (img,):
        one_query(engine, "morphology", lambda: engine.morphology(img.id, radius=(2, 1), premultiplied=False))
        got = img.bits()
    once = morph_ref.morph(bits, morph_ref.DILATE, (2, 1), morph_ref.ZERO, morph_ref.STRAIGHT)
    assert np.array_equal(got, morph_ref.morph(once, morph_ref.DILATE, (2, 1), morph_ref.ZERO, morph_ref.STRAIGHT))
