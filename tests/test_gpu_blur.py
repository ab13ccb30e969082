"""-m gpu: jh_blur against the rule of DESIGN.md 5.7 (tests/blur_ref.py) byte for byte -- the battery of tests/blur_cases.py, a
rendered frame, a captured frame -- and the call's frame: its refusals, its profile query, the held-back commands in front of it."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import BlurEdge, Brush, Cap, Fill, ImageFormat, Join, Path, RenderParams, Scene, Stroke, Surface
from jello_amd._lib import CBlurDesc
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS

import blur_cases
import blur_ref
import surface_ref
from devmem import CANARY, DevBuf, Image, _id, target_of

pytestmark = pytest.mark.gpu

JH_ERR_OOM = -5


@pytest.mark.parametrize("name", [c["name"] for c in blur_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.blur: dst is poisoned first (or is the source), the whole of dst is compared -- the rectangle with
    the reference, the texels outside it with what they held."""
    c = blur_cases.BY_NAME[name]
    src_bits = blur_cases.source(c)
    src = Image(engine, None, c["w"], c["h"]) if c["kind"] == "never" else Image(engine, src_bits)
    dst = src if c["in_place"] else Image(engine, np.full_like(src_bits, blur_cases.POISON))
    try:
        engine.blur(src.id, c["w"], c["h"], c["sigma"], dst_image_id=None if c["in_place"] else dst.id, edge=BlurEdge(c["edge"]), rect=c["rect"])
        got = dst.bits()
        if not c["in_place"] and c["kind"] != "never":  # (a never-written image reads as zero; its memory holds anything)
            assert np.array_equal(src.bits(), src_bits)  # the source is only read
    finally:
        src.free()
        if dst is not src:
            dst.free()
    want = blur_cases.expected(name)
    if not blur_ref.same_bits(got, want):
        bad = np.argwhere(got != want)
        pytest.fail("%s: %d of %d values differ, first at (y, x, ch) = %s: got %#06x, want %#06x" % (
            name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def test_a_never_written_destination_is_cleared_outside_the_rectangle(engine):
    bits = blur_cases.content("unit", 33, 21, seed=3)
    src, dst = Image(engine, bits), Image(engine, None, 33, 21)
    rect = (5, 4, 20, 9)
    try:
        engine.blur(src.id, 33, 21, (1.0, 2.5), dst_image_id=dst.id, rect=rect)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    assert np.array_equal(got, blur_ref.blur(bits, (1.0, 2.5), blur_ref.ZERO, rect, None))


def _scene():
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid((0.9, 0.4, 0.1, 1.0)), None, Path.circle(24, 20, 13))
    curve = Path().move_to(6, 40).cubic_to(20, 2, 44, 46, 58, 8)
    s.stroke(Stroke(3, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None, curve)
    return s, RenderParams(64, 48)


@pytest.mark.parametrize("edge", list(BlurEdge))
def test_rendered_scene_in_place(engine, edge):
    """A rendered 64 x 48 frame (a circle and a stroked curve) blurred in place = the reference on the download of the same render."""
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    t = rec.target
    plain = target_of(engine, rec)
    assert plain.any()
    engine.blur(t["id"], 64, 48, (2.0, 3.5), edge=edge)
    assert blur_ref.same_bits(target_of(engine, rec), blur_ref.blur(plain, (2.0, 3.5), int(edge)))


def test_captured_with_the_frame(engine):
    """capture(blur=..., surface=...): render, blur in place, blit -- replayed twice, the bytes of the eager calls."""
    s, p = _scene()
    fmt, sigma, rect = Surface.RGBA8_SRGB, (3.0, 1.5), (8, 4, 50, 40)
    rec = jello_amd.Host().record(s, p)
    surf = DevBuf(engine, 64 * 48 * 4)
    g = None
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        t = rec.target
        plain = target_of(engine, rec)
        engine.blur(t["id"], 64, 48, sigma, edge=BlurEdge.CLAMP, rect=rect)
        engine.blit(t["id"], 64, 48, fmt, out_device_ptr=surf.ptr)
        eager = surf.bytes().reshape(48, 64, 4)
        blurred = blur_ref.blur(plain, sigma, blur_ref.CLAMP, rect, plain)
        assert blur_ref.same_bits(target_of(engine, rec), blurred)
        assert np.array_equal(eager, surface_ref.convert(blurred, int(fmt)))
        g0 = engine.capture(rec)
        g = engine.capture(rec, blur=dict(sigma=sigma, edge=BlurEdge.CLAMP, rect=rect), surface=(surf.ptr, 64 * 4, fmt))
        (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
        engine.graph_destroy(g0)
        assert (k1, o1) == (k0 + 3, o0)  # rows, columns, blit
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
    bits = blur_cases.content("unit", 64, 48, seed=1)
    img, other = Image(engine, bits), DevBuf(engine, 64)
    d = CBlurDesc(2.0, 2.0, 0, 0, 0, 0, 0)
    g = None
    try:
        engine.trim_scratch()  # the intermediate has to be allocated again
        engine._check(hip.jh_graph_begin(ctx), "graph_begin")
        try:
            engine.clear(other.id)
            rc = hip.jh_blur(ctx, img.id, img.id, 64, 48, ctypes.byref(d))
            msg = hip.jh_last_error(ctx).decode()
        finally:
            h = ctypes.c_void_p()
            engine._check(hip.jh_graph_end(ctx, ctypes.byref(h)), "graph_end")
            engine.graph_destroy(h)
        assert rc == JH_ERR_OOM and msg.startswith("jh_blur: ") and "blur a rectangle of this size once eagerly first" in msg, (rc, msg)
        assert np.array_equal(img.bits(), bits)
        # ... and after that eager call the same capture works
        engine.blur(img.id, 64, 48, 2.0)
        once = img.bits()
        assert blur_ref.same_bits(once, blur_ref.blur(bits, 2.0))
        engine._check(hip.jh_graph_begin(ctx), "graph_begin")
        try:
            rc = hip.jh_blur(ctx, img.id, img.id, 64, 48, ctypes.byref(d))
        finally:
            g = ctypes.c_void_p()
            engine._check(hip.jh_graph_end(ctx, ctypes.byref(g)), "graph_end")
        assert rc == 0
        assert np.array_equal(img.bits(), once)  # a capture runs nothing
        engine.replay(g)
        assert blur_ref.same_bits(img.bits(), blur_ref.blur(once, 2.0))
    finally:
        if g is not None:
            engine.graph_destroy(g)
        img.free()
        other.free()


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_blur: ", no texel of either image touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = np.full((H, W, 4), CANARY | (CANARY << 8), np.uint16)
    src, dst = Image(engine, canary), Image(engine, canary)
    rgba8 = Image(engine, np.full((H, W, 2), 0x1111, np.uint16), fmt=ImageFormat.RGBA8)  # (W x H texels of 4 bytes)
    nan, inf = float("nan"), float("inf")

    def call(s=None, d=None, w=W, h=H, desc=(1.0, 1.0, 0, 0, 0, 0, 0)):
        return hip.jh_blur(ctx, src.id if s is None else s, dst.id if d is None else d, w, h, None if desc is None else ctypes.byref(CBlurDesc(*desc)))

    refused = {
        "null descriptor": lambda: call(desc=None),
        "unknown source": lambda: call(s=_id()),
        "unknown destination": lambda: call(d=_id()),
        "source not RGBA16F": lambda: call(s=rgba8.id),
        "destination not RGBA16F": lambda: call(d=rgba8.id),
        "width differs": lambda: call(w=W + 1),
        "height differs": lambda: call(h=H - 1),
        "sigma_x negative": lambda: call(desc=(-0.5, 1.0, 0, 0, 0, 0, 0)),
        "sigma_y negative": lambda: call(desc=(1.0, -1e-20, 0, 0, 0, 0, 0)),
        "sigma_x above 64": lambda: call(desc=(64.5, 1.0, 0, 0, 0, 0, 0)),
        "sigma_y infinite": lambda: call(desc=(1.0, inf, 0, 0, 0, 0, 0)),
        "sigma_x NaN": lambda: call(desc=(nan, 1.0, 0, 0, 0, 0, 0)),
        "sigma_y NaN": lambda: call(desc=(1.0, nan, 0, 0, 0, 0, 0)),
        "edge mode 2": lambda: call(desc=(1.0, 1.0, 2, 0, 0, 0, 0)),
        "edge mode -1": lambda: call(desc=(1.0, 1.0, -1, 0, 0, 0, 0)),
        "rectangle beyond the right edge": lambda: call(desc=(1.0, 1.0, 0, 8, 0, 9, 4)),
        "rectangle beyond the bottom edge": lambda: call(desc=(1.0, 1.0, 0, 0, 9, 4, 4)),
        "rectangle whose end wraps": lambda: call(desc=(1.0, 1.0, 0, 0xFFFFFFFF, 0, 2, 2)),
        "empty in x only": lambda: call(desc=(1.0, 1.0, 0, 2, 2, 0, 4)),
        "empty in y only": lambda: call(desc=(1.0, 1.0, 0, 2, 2, 4, 0)),
    }
    try:
        for what, f in refused.items():
            assert f() == JH_ERR_INVALID, what
            assert hip.jh_last_error(ctx).startswith(b"jh_blur: "), (what, hip.jh_last_error(ctx))
        engine.set_band(0, 1)
        try:
            assert call() == JH_ERR_INVALID
            assert hip.jh_last_error(ctx).startswith(b"jh_blur: ") and b"band" in hip.jh_last_error(ctx)
        finally:
            engine.set_band()
        with pytest.raises(ValueError, match="jh_blur: "):
            engine.blur(src.id, W, H, 65.0)
        assert np.array_equal(src.bits(), canary) and np.array_equal(dst.bits(), canary)
        assert call() == 0  # (and the same call with nothing wrong is accepted)
    finally:
        for im in (src, dst, rgba8):
            im.free()


def test_the_call_is_one_query_of_the_tree(engine):
    bits = blur_cases.content("unit", 48, 33, seed=2)
    img = Image(engine, bits)
    try:
        engine.profile(True)
        try:
            with engine.profile_group("post"):
                engine.blur(img.id, 48, 33, (2.0, 1.0))
            tree = engine.profile_collect_tree()
            engine.blur(img.id, 48, 33, (2.0, 1.0))
            flat = engine.profile_collect()
        finally:
            engine.profile(False)
        got = img.bits()
    finally:
        img.free()
    assert [(n["kind"], n["label"], n["parent"], n["stage"]) for n in tree] == [("group", "post", -1, -1), ("query", "blur", 0, -1)]
    assert tree[1]["gpu_end_ms"] >= tree[1]["gpu_start_ms"]
    assert flat == []
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
