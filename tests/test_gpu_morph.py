"""-m gpu: jh_morphology against the rule of DESIGN.md 5.11 (tests/morph_ref.py) byte for byte -- the battery of
tests/morph_cases.py, never-written images, a rendered frame, Engine.outline and drop_shadow(spread=...), a captured frame -- and
the call's frame: its refusals, its profile query."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, Fill, ImageFormat, Join, MorphEdge, MorphOp, Path, RenderParams, Scene, Stroke, Surface
from jello_amd._lib import CMorphDesc
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS

import blur_ref
import composite_cases
import composite_ref
import morph_cases
import morph_ref
import surface_ref
from devmem import CANARY, DevBuf, Image, _id, target_of

pytestmark = pytest.mark.gpu

JH_ERR_OOM = -5
MORPH_LAUNCHES = 3  # rows, block prefix, block suffix + store (include/jello_hip.h)


def _differences(got, want):
    bad = np.argwhere((got != want) & ~(((got & 0x7FFF) > 0x7C00) & ((want & 0x7FFF) > 0x7C00)))
    if len(bad) == 0:
        return "equal"
    i = tuple(bad[0])
    return "%d of %d values differ, first at (y, x, ch) = %s: got %#06x, want %#06x" % (len(bad), got.size, i, got[i], want[i])


@pytest.mark.parametrize("name", [c["name"] for c in morph_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.morphology: dst is poisoned first (or is the source), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held -- and the source of a call into a second image is only read."""
    c = morph_cases.BY_NAME[name]
    src_bits = morph_cases.source(c)
    src = Image(engine, None, c["w"], c["h"]) if c["kind"] == "never" else Image(engine, src_bits)
    dst = src if c["in_place"] else Image(engine, np.full_like(src_bits, morph_cases.POISON))
    try:
        engine.morphology(src.id, None if c["in_place"] else dst.id, op=MorphOp(c["op"]), radius=c["radius"], edge=MorphEdge(c["edge"]),
                          rect=c["rect"], premultiplied=not c["flags"])
        got = dst.bits()
        if not c["in_place"] and c["kind"] != "never":  # (a never-written image reads as zero; its memory holds anything)
            assert np.array_equal(src.bits(), src_bits)
    finally:
        src.free()
        if dst is not src:
            dst.free()
    want = morph_cases.expected(name)
    assert morph_ref.same_bits(got, want), name + ": " + _differences(got, want)


def test_a_never_written_destination_is_cleared_outside_the_rectangle(engine):
    bits = morph_cases.content("unit", 33, 21, seed=3)
    src, dst = Image(engine, bits), Image(engine, None, 33, 21)
    rect = (5, 4, 20, 9)
    try:
        engine.morphology(src.id, dst.id, op=MorphOp.ERODE, radius=(1, 2), edge=MorphEdge.CLAMP, rect=rect)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    want = morph_ref.morph(bits, morph_ref.ERODE, (1, 2), morph_ref.CLAMP, 0, rect, None)
    assert morph_ref.same_bits(got, want), _differences(got, want)


def test_a_never_written_source_reads_as_transparent_black(engine):
    src, dst = Image(engine, None, 33, 21), Image(engine, np.full((21, 33, 4), morph_cases.POISON, np.uint16))
    try:
        engine.morphology(src.id, dst.id, op=MorphOp.DILATE, radius=3, premultiplied=False)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    assert not got.any()


def _scene():
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid((0.9, 0.4, 0.1, 1.0)), None, Path.circle(24, 20, 13))
    curve = Path().move_to(6, 40).cubic_to(20, 2, 44, 46, 58, 8)
    s.stroke(Stroke(3, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None, curve)
    return s, RenderParams(64, 48)


@pytest.mark.parametrize("op", list(MorphOp))
def test_rendered_scene_in_place(engine, op):
    """A rendered 64 x 48 frame (a circle and a stroked curve) in place = the reference on the download of the same render."""
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    plain = target_of(engine, rec)
    assert plain.any()
    engine.morphology(rec.target["id"], op=op, radius=(2, 3))
    got, want = target_of(engine, rec), morph_ref.morph(plain, int(op), (2, 3), morph_ref.ZERO)
    assert morph_ref.same_bits(got, want), _differences(got, want)
    assert (want != plain).any()


def test_outline_of_a_rendered_frame(engine):
    """Engine.outline onto an 80 x 60 target = morph_ref (dilate, ZERO), composite_ref with the tint, composite_ref of the layer."""
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    layer = target_of(engine, rec)
    backdrop = composite_cases.unit(80, 60, seed=5)
    color = (0.0, 0.6, 0.2, 0.9)
    target, scratch = Image(engine, backdrop), Image(engine, None, 64, 48)
    try:
        engine.outline(rec.target["id"], target.id, 2, color, scratch.id)
        got, grown = target.bits(), scratch.bits()
        assert np.array_equal(target_of(engine, rec), layer)
    finally:
        target.free()
        scratch.free()
    halo = morph_ref.morph(layer, morph_ref.DILATE, 2, morph_ref.ZERO)
    assert morph_ref.same_bits(grown, halo), _differences(grown, halo)
    want = composite_ref.composite(layer, composite_ref.composite(halo, backdrop, tint=color))
    assert composite_ref.same_bits(got, want), _differences(got, want)
    assert (want != composite_ref.composite(layer, backdrop)).any()  # (the outline shows)


def test_drop_shadow_with_spread_and_without(engine):
    """spread=3: the layer dilated into the scratch, the scratch blurred in place, then the two composites -- against morph_ref,
    blur_ref and composite_ref.  The default spread: the bytes of the three calls drop_shadow has always made."""
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    layer = target_of(engine, rec)
    backdrop = composite_cases.unit(80, 60, seed=5)
    sigma, offset, color = (2.0, 3.5), (7, 5), (0.05, 0.0, 0.1, 0.6)
    got = {}
    for spread in (3, 0, None):
        target, scratch = Image(engine, backdrop), Image(engine, None, 64, 48)
        try:
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
        finally:
            target.free()
            scratch.free()
    assert np.array_equal(got[0][0], got[None][0]) and np.array_equal(got[0][1], got[None][1])
    plain_shadow = blur_ref.blur(layer, sigma, blur_ref.ZERO)
    assert blur_ref.same_bits(got[0][1], plain_shadow)
    shadow = blur_ref.blur(morph_ref.morph(layer, morph_ref.DILATE, 3, morph_ref.ZERO), sigma, blur_ref.ZERO)
    assert blur_ref.same_bits(got[3][1], shadow), _differences(got[3][1], shadow)
    want = composite_ref.composite(layer, composite_ref.composite(shadow, backdrop, tint=color, offset=offset))
    assert composite_ref.same_bits(got[3][0], want), _differences(got[3][0], want)
    assert (shadow != plain_shadow).any()


def test_captured_with_the_frame(engine):
    """capture(morphology=..., surface=...): render, dilate in place, blit -- replayed twice, the bytes of the eager calls, and
    MORPH_LAUNCHES + 1 more kernel nodes than the plain capture."""
    s, p = _scene()
    fmt, what = Surface.RGBA8_SRGB, dict(op=MorphOp.DILATE, radius=(3, 5), edge=MorphEdge.CLAMP, rect=(8, 4, 50, 40))
    rec = jello_amd.Host().record(s, p)
    surf = DevBuf(engine, 64 * 48 * 4)
    g = None
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        t = rec.target
        plain = target_of(engine, rec)
        engine.morphology(t["id"], **what)
        engine.blit(t["id"], 64, 48, fmt, out_device_ptr=surf.ptr)
        eager = surf.bytes().reshape(48, 64, 4)
        grown = morph_ref.morph(plain, morph_ref.DILATE, (3, 5), morph_ref.CLAMP, 0, what["rect"], plain)
        assert morph_ref.same_bits(target_of(engine, rec), grown), _differences(target_of(engine, rec), grown)
        assert np.array_equal(eager, surface_ref.convert(grown, int(fmt)))
        g0 = engine.capture(rec)
        g = engine.capture(rec, morphology=what, surface=(surf.ptr, 64 * 4, fmt))
        (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
        engine.graph_destroy(g0)
        assert (k1, o1) == (k0 + MORPH_LAUNCHES + 1, o0)
        for _ in range(2):
            engine.clear(surf.id)
            engine.replay(g)
            engine.sync()
            assert np.array_equal(surf.bytes().reshape(48, 64, 4), eager)
    finally:
        if g is not None:
            engine.graph_destroy(g)
        surf.free()


def test_capture_without_scratch_is_refused_with_advice(engine):
    hip, ctx = engine.hip, engine.ctx
    bits = morph_cases.content("unit", 64, 48, seed=1)
    img = Image(engine, bits)
    d = CMorphDesc(1, 0, 1, 2, 2, 0, 0, 0, 0)
    g = None
    try:
        engine.trim_scratch()  # the planes have to be allocated again
        engine._check(hip.jh_graph_begin(ctx), "graph_begin")
        try:
            rc = hip.jh_morphology(ctx, img.id, img.id, ctypes.byref(d))
            msg = hip.jh_last_error(ctx).decode()
        finally:
            h = ctypes.c_void_p()
            engine._check(hip.jh_graph_end(ctx, ctypes.byref(h)), "graph_end")
            engine.graph_destroy(h)
        assert rc == JH_ERR_OOM and msg.startswith("jh_morphology: ") and "once eagerly first" in msg, (rc, msg)
        assert np.array_equal(img.bits(), bits)
        # ... the context stays usable, and after that eager call the same capture works
        engine.morphology(img.id, radius=2, premultiplied=False)
        once = img.bits()
        assert np.array_equal(once, morph_ref.morph(bits, morph_ref.DILATE, 2, morph_ref.ZERO, morph_ref.STRAIGHT))
        engine._check(hip.jh_graph_begin(ctx), "graph_begin")
        try:
            rc = hip.jh_morphology(ctx, img.id, img.id, ctypes.byref(d))
        finally:
            g = ctypes.c_void_p()
            engine._check(hip.jh_graph_end(ctx, ctypes.byref(g)), "graph_end")
        assert rc == 0
        assert np.array_equal(img.bits(), once)  # a capture runs nothing
        engine.replay(g)
        assert np.array_equal(img.bits(), morph_ref.morph(once, morph_ref.DILATE, 2, morph_ref.ZERO, morph_ref.STRAIGHT))
    finally:
        if g is not None:
            engine.graph_destroy(g)
        img.free()


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_morphology: ", no texel of any image touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = np.full((H, W, 4), CANARY | (CANARY << 8), np.uint16)
    src, dst = Image(engine, canary), Image(engine, canary)
    wider = Image(engine, np.full((H, W + 1, 4), CANARY | (CANARY << 8), np.uint16))
    rgba8 = Image(engine, np.full((H, W, 2), 0x1111, np.uint16), fmt=ImageFormat.RGBA8)  # (W x H texels of 4 bytes)
    ok = (1, 0, 0, 1, 1, 0, 0, 0, 0)

    def call(s=None, d=None, desc=ok):
        return hip.jh_morphology(ctx, src.id if s is None else s, dst.id if d is None else d, None if desc is None else ctypes.byref(CMorphDesc(*desc)))

    refused = {
        "null descriptor": lambda: call(desc=None),
        "unknown source": lambda: call(s=_id()),
        "unknown destination": lambda: call(d=_id()),
        "source not RGBA16F": lambda: call(s=rgba8.id),
        "destination not RGBA16F": lambda: call(d=rgba8.id),
        "sizes differ": lambda: call(d=wider.id),
        "op 2": lambda: call(desc=(2, 0, 0, 1, 1, 0, 0, 0, 0)),
        "op -1": lambda: call(desc=(-1, 0, 0, 1, 1, 0, 0, 0, 0)),
        "edge 2": lambda: call(desc=(1, 2, 0, 1, 1, 0, 0, 0, 0)),
        "edge -1": lambda: call(desc=(1, -1, 0, 1, 1, 0, 0, 0, 0)),
        "flag bit 1": lambda: call(desc=(1, 0, 2, 1, 1, 0, 0, 0, 0)),
        "flag bit 31": lambda: call(desc=(1, 0, 0x80000001, 1, 1, 0, 0, 0, 0)),
        "radius_x 256": lambda: call(desc=(1, 0, 0, 256, 1, 0, 0, 0, 0)),
        "radius_y 256": lambda: call(desc=(1, 0, 0, 1, 256, 0, 0, 0, 0)),
        "radius_x 2^32 - 1": lambda: call(desc=(1, 0, 0, 0xFFFFFFFF, 1, 0, 0, 0, 0)),
        "rectangle beyond the right edge": lambda: call(desc=(1, 0, 0, 1, 1, 8, 0, 9, 4)),
        "rectangle beyond the bottom edge": lambda: call(desc=(1, 0, 0, 1, 1, 0, 9, 4, 4)),
        "rectangle whose end wraps": lambda: call(desc=(1, 0, 0, 1, 1, 0xFFFFFFFF, 0, 2, 2)),
        "empty in x only": lambda: call(desc=(1, 0, 0, 1, 1, 2, 2, 0, 4)),
        "empty in y only": lambda: call(desc=(1, 0, 0, 1, 1, 2, 2, 4, 0)),
    }
    try:
        for what, f in refused.items():
            assert f() == JH_ERR_INVALID, what
            assert hip.jh_last_error(ctx).startswith(b"jh_morphology: "), (what, hip.jh_last_error(ctx))
        engine.set_band(0, 1)
        try:
            assert call() == JH_ERR_INVALID
            assert hip.jh_last_error(ctx).startswith(b"jh_morphology: ") and b"band" in hip.jh_last_error(ctx)
        finally:
            engine.set_band()
        with pytest.raises(ValueError, match="jh_morphology: "):
            engine.morphology(src.id, dst.id, radius=256)
        with pytest.raises(ValueError, match="jh_morphology: "):
            engine.morphology(src.id, dst.id, rect=(8, 0, 9, 4))
        for im, want in ((src, canary), (dst, canary), (wider, np.full((H, W + 1, 4), CANARY | (CANARY << 8), np.uint16))):
            assert np.array_equal(im.bits(), want)
        assert call() == 0  # (and the same call with nothing wrong is accepted)
    finally:
        for im in (src, dst, wider, rgba8):
            im.free()


def test_the_call_is_one_query_of_the_tree(engine):
    bits = morph_cases.content("unit", 48, 33, seed=2)
    img = Image(engine, bits)
    try:
        engine.profile(True)
        try:
            with engine.profile_group("post"):
                engine.morphology(img.id, radius=(2, 1), premultiplied=False)
            tree = engine.profile_collect_tree()
            engine.morphology(img.id, radius=(2, 1), premultiplied=False)
            flat = engine.profile_collect()
        finally:
            engine.profile(False)
        got = img.bits()
    finally:
        img.free()
    assert [(n["kind"], n["label"], n["parent"], n["stage"]) for n in tree] == [("group", "post", -1, -1), ("query", "morphology", 0, -1)]
    assert tree[1]["gpu_end_ms"] >= tree[1]["gpu_start_ms"]
    assert flat == []
    once = morph_ref.morph(bits, morph_ref.DILATE, (2, 1), morph_ref.ZERO, morph_ref.STRAIGHT)
    assert np.array_equal(got, morph_ref.morph(once, morph_ref.DILATE, (2, 1), morph_ref.ZERO, morph_ref.STRAIGHT))
