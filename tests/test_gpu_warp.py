"""-m gpu: jh_warp against the rule of DESIGN.md 5.12 (tests/warp_ref.py) byte for byte -- the battery of tests/warp_cases.py, a warp
in quadrants, a rendered frame, Engine.place_layer, a captured frame -- and the call's frame: its refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, Fill, ImageFormat, Join, Path, RenderParams, ResampleFilter, Scene, Stroke, Surface, WarpEdge, WarpFilter
from jello_amd._lib import CWarpDesc
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS

import composite_ref
import surface_ref
import warp_cases
import warp_ref
from devmem import CANARY, DevBuf, Image, _id, target_of

pytestmark = pytest.mark.gpu


def _differences(name, got, want):
    bad = np.argwhere(got != want)
    return "%s: %d of %d values differ, first at (y, x, ch) = %s: got %#06x, want %#06x" % (
        name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", [c["name"] for c in warp_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.warp: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle with
    the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = warp_cases.BY_NAME[name]
    src_bits, prior = warp_cases.source(c), warp_cases.before(c)
    src = Image(engine, None, *c["src_size"]) if c["kind"] == "never" else Image(engine, src_bits)
    dst = Image(engine, None, *c["dst_size"]) if prior is None else Image(engine, prior)
    try:
        engine.warp(src.id, dst.id, c["matrix"], WarpFilter(c["filter"]), WarpEdge(c["edge"]), c["src_rect"], c["dst_rect"], premultiplied=not c["flags"])
        got = dst.bits()
        if c["kind"] != "never":  # (a never-written image reads as zero; its memory holds anything)
            assert np.array_equal(src.bits(), src_bits)  # the source is only read
    finally:
        src.free()
        dst.free()
    want = warp_cases.expected(name)
    if not warp_ref.same_bits(got, want):
        pytest.fail(_differences(name, got, want))


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_four_quadrants_are_the_whole_image(engine, filt):
    bits = warp_cases.content("unit", 45, 37, seed=3)
    m = warp_cases.rotate(30, (45, 37), (51, 35), 1.2)
    src, whole, parts = Image(engine, bits), Image(engine, None, 51, 35), Image(engine, None, 51, 35)
    try:
        engine.warp(src.id, whole.id, m, filt, WarpEdge.MIRROR)
        for rect in ((0, 0, 25, 17), (25, 0, 26, 17), (0, 17, 25, 18), (25, 17, 26, 18)):
            engine.warp(src.id, parts.id, m, filt, WarpEdge.MIRROR, dst_rect=rect)
        a, b = whole.bits(), parts.bits()
    finally:
        for im in (src, whole, parts):
            im.free()
    assert np.array_equal(a, b)
    assert warp_ref.same_bits(a, warp_ref.warp(bits, (35, 51), m, int(filt), warp_ref.MIRROR))


def test_a_never_written_source_and_a_never_written_destination(engine):
    """A never-written source gives transparent black inside the rectangle under every edge mode and leaves the rest of dst alone; a
    never-written destination is cleared around the rectangle."""
    src, dst = Image(engine, None, 40, 30), Image(engine, np.full((20, 25, 4), warp_cases.POISON, np.uint16))
    bits = warp_cases.content("unit", 9, 7, seed=4)
    real, fresh = Image(engine, bits), Image(engine, None, 25, 20)
    m = warp_cases.rotate(45, (40, 30), (25, 20))
    try:
        for edge, premultiplied, rect in ((WarpEdge.REPEAT, True, (1, 1, 11, 9)), (WarpEdge.CLAMP, False, (13, 10, 12, 10))):
            engine.warp(src.id, dst.id, m, WarpFilter.BICUBIC, edge, dst_rect=rect, premultiplied=premultiplied)
        got = dst.bits()
        engine.warp(real.id, fresh.id, warp_cases.translate(3, 2), WarpFilter.BILINEAR, WarpEdge.CLAMP, dst_rect=(5, 3, 7, 9))
        cleared = fresh.bits()
    finally:
        for im in (src, dst, real, fresh):
            im.free()
    want = np.full((20, 25, 4), warp_cases.POISON, np.uint16)
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    assert np.array_equal(got, want)
    assert warp_ref.same_bits(cleared, warp_ref.warp(bits, (20, 25), warp_cases.translate(3, 2), warp_ref.BILINEAR, warp_ref.CLAMP, dst_rect=(5, 3, 7, 9)))


def _scene():
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid((0.9, 0.4, 0.1, 1.0)), None, Path.circle(50, 44, 30))
    curve = Path().move_to(10, 100).cubic_to(40, 4, 90, 120, 120, 16)
    s.stroke(Stroke(5, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None, curve)
    return s, RenderParams(128, 128)


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_rendered_scene(engine, filt):
    """A rendered 128 x 128 frame (a circle and a stroked curve, translucent edges) rotated by 30 degrees into 96 x 80 = the
    reference on the download of the same render."""
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    plain = target_of(engine, rec)
    assert plain.any()
    m = warp_cases.rotate(30, (128, 128), (96, 80), 0.7)
    dst = Image(engine, None, 96, 80)
    try:
        engine.warp(rec.target["id"], dst.id, m, filt)
        got = dst.bits()
    finally:
        dst.free()
    want = warp_ref.warp(plain, (80, 96), m, int(filt))
    assert warp_ref.same_bits(got, want), _differences(filt.name, got, want)
    assert np.array_equal(target_of(engine, rec), plain)


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_place_layer(engine, filt):
    """Engine.place_layer = warp_ref.warp into the scratch's bounds rectangle, then composite_ref.composite of that rectangle."""
    layer_bits = warp_cases.content("alpha01", 29, 21, seed=6)
    target_bits = warp_cases.content("unit", 61, 47, seed=7)
    target_bits[..., 3] = 0x3C00
    m = warp_cases.rotate(30, (29, 21), (61, 47), 0.9)
    layer, target, scratch = Image(engine, layer_bits), Image(engine, target_bits), Image(engine, None, 61, 47)
    try:
        rect = engine.place_layer(layer.id, target.id, m, scratch.id, (29, 21), (61, 47), filter=filt, opacity=0.75)
        got, got_scratch = target.bits(), scratch.bits()
        gone = engine.place_layer(layer.id, target.id, warp_cases.translate(500, 0), scratch.id, (29, 21), (61, 47), filter=filt)
        assert gone == (0, 0, 0, 0) and np.array_equal(target.bits(), got)
    finally:
        for im in (layer, target, scratch):
            im.free()
    assert rect == warp_ref.bounds(m, (29, 21), int(filt), (61, 47)) and 0 < rect[2] < 61 and 0 < rect[3] < 47
    warped = warp_ref.warp(layer_bits, (47, 61), m, int(filt), warp_ref.ZERO, dst_rect=rect)
    assert warp_ref.same_bits(got_scratch, warped)
    assert warp_ref.same_bits(warped, warp_ref.warp(layer_bits, (47, 61), m, int(filt), warp_ref.ZERO))  # outside the bounds: transparent black
    want = composite_ref.composite(warped, target_bits, opacity=0.75, src_rect=rect, offset=(rect[0], rect[1]))
    assert composite_ref.same_bits(got, want), _differences(filt.name, got, want)


def test_captured_with_the_frame(engine):
    """capture(warp=..., surface=...): render, rotate into a second image, blit that image at its size -- one launch more than with
    the blit alone, replayed twice, the bytes of the eager calls; resample= together with warp= is refused before anything is
    captured."""
    s, p = _scene()
    fmt, filt = Surface.RGBA8_SRGB, WarpFilter.BICUBIC
    m = warp_cases.rotate(30, (128, 128), (48, 40), 0.4)
    rec = jello_amd.Host().record(s, p)
    small, surf, full = Image(engine, None, 48, 40), DevBuf(engine, 48 * 40 * 4), DevBuf(engine, 128 * 128 * 4)
    g = None
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        t = rec.target
        plain = target_of(engine, rec)
        engine.warp(t["id"], small.id, m, filt, WarpEdge.CLAMP)
        engine.blit(small.id, 48, 40, fmt, out_device_ptr=surf.ptr)
        eager = surf.bytes()[:48 * 40 * 4].reshape(40, 48, 4)
        turned = warp_ref.warp(plain, (40, 48), m, int(filt), warp_ref.CLAMP)
        assert warp_ref.same_bits(small.bits(), turned)
        assert np.array_equal(eager, surface_ref.convert(turned, int(fmt)))
        with pytest.raises(ValueError, match="exclusive"):
            engine.capture(rec, resample=dict(dst=small.id, width=48, height=40, filter=ResampleFilter.BOX),
                           warp=dict(dst=small.id, width=48, height=40, matrix=m))
        g0 = engine.capture(rec, surface=(full.ptr, 128 * 4, fmt))  # (the frame and the blit of its own target)
        g = engine.capture(rec, warp=dict(dst=small.id, width=48, height=40, matrix=m, filter=filt, edge=WarpEdge.CLAMP), surface=(surf.ptr, 48 * 4, fmt))
        (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
        engine.graph_destroy(g0)
        assert (k1, o1) == (k0 + 1, o0)  # one launch, no scratch, no tables
        for _ in range(2):
            engine.clear(surf.id)
            engine.replay(g)
            engine.sync()
            assert np.array_equal(surf.bytes()[:48 * 40 * 4].reshape(40, 48, 4), eager)
        assert np.array_equal(target_of(engine, rec), plain)
    finally:
        if g is not None:
            engine.graph_destroy(g)
        small.free()
        surf.free()
        full.free()


IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_warp: ", no texel of either image and no byte
    of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = np.full((H, W, 4), CANARY | (CANARY << 8), np.uint16)
    src, dst = Image(engine, canary), Image(engine, canary)
    rgba8 = Image(engine, np.full((H, W, 2), 0x1111, np.uint16), fmt=ImageFormat.RGBA8)  # (W x H texels of 4 bytes)
    long_ = Image(engine, None, 32769, 1)
    guard = DevBuf(engine, 256)

    def call(s=None, d=None, m=IDENT, tail=(1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), null=False):
        desc = CWarpDesc((ctypes.c_double * 6)(*m), *tail)
        return hip.jh_warp(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

    refused = {
        "null descriptor": (lambda: call(null=True), b""),
        "unknown source": (lambda: call(s=_id()), b"unknown source"),
        "unknown destination": (lambda: call(d=_id()), b"unknown destination"),
        "source not RGBA16F": (lambda: call(s=rgba8.id), b"RGBA16F"),
        "destination not RGBA16F": (lambda: call(d=rgba8.id), b"RGBA16F"),
        "filter 3": (lambda: call(tail=(3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), b"filter"),
        "filter -1": (lambda: call(tail=(-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), b"filter"),
        "edge 4": (lambda: call(tail=(1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0)), b"edge"),
        "edge -1": (lambda: call(tail=(1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0)), b"edge"),
        "flag bit 1": (lambda: call(tail=(1, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0)), b"flag"),
        "flag bit 31": (lambda: call(tail=(1, 0, 0x80000001, 0, 0, 0, 0, 0, 0, 0, 0)), b"flag"),
        "a NaN entry": (lambda: call(m=(1.0, math.nan, 0.0, 1.0, 0.0, 0.0)), b"not finite"),
        "an infinite entry": (lambda: call(m=(1.0, 0.0, 0.0, 1.0, 0.0, math.inf)), b"not finite"),
        "determinant 0": (lambda: call(m=(1.0, 2.0, 2.0, 4.0, 0.0, 0.0)), b"determinant is 0"),
        "determinant overflows": (lambda: call(m=(1e200, 0.0, 0.0, 1e200, 0.0, 0.0)), b"determinant is not finite"),
        "65:1": (lambda: call(m=(1.0 / 65.0, 0.0, 0.0, 1.0, 0.0, 0.0)), b"above 64"),
        "offset beyond 2^22": (lambda: call(m=(1.0, 0.0, 0.0, 1.0, 5e6, 0.0)), b"above 2^22"),
        "a side above 32768": (lambda: call(s=long_.id), b"32768"),
        "source rectangle beyond the right edge": (lambda: call(tail=(1, 0, 0, 8, 0, 9, 4, 0, 0, 0, 0)), b"source rectangle"),
        "source rectangle beyond the bottom edge": (lambda: call(tail=(1, 0, 0, 0, 9, 4, 4, 0, 0, 0, 0)), b"source rectangle"),
        "source rectangle whose end wraps": (lambda: call(tail=(1, 0, 0, 0xFFFFFFFF, 0, 2, 2, 0, 0, 0, 0)), b"source rectangle"),
        "source rectangle empty in x only": (lambda: call(tail=(1, 0, 0, 2, 2, 0, 4, 0, 0, 0, 0)), b"source rectangle"),
        "source rectangle empty in y only": (lambda: call(tail=(1, 0, 0, 2, 2, 4, 0, 0, 0, 0, 0)), b"source rectangle"),
        "destination rectangle beyond the right edge": (lambda: call(tail=(1, 0, 0, 0, 0, 0, 0, 8, 0, 9, 4)), b"destination rectangle"),
        "destination rectangle beyond the bottom edge": (lambda: call(tail=(1, 0, 0, 0, 0, 0, 0, 0, 9, 4, 4)), b"destination rectangle"),
        "destination rectangle whose end wraps": (lambda: call(tail=(1, 0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 2, 2)), b"destination rectangle"),
        "destination rectangle empty in x only": (lambda: call(tail=(1, 0, 0, 0, 0, 0, 0, 2, 2, 0, 4)), b"destination rectangle"),
        "destination rectangle empty in y only": (lambda: call(tail=(1, 0, 0, 0, 0, 0, 0, 2, 2, 4, 0)), b"destination rectangle"),
        "source is the destination": (lambda: call(d=src.id), b"source is the destination"),
    }
    try:
        for what, (f, word) in refused.items():
            assert f() == JH_ERR_INVALID, what
            msg = hip.jh_last_error(ctx)
            assert msg.startswith(b"jh_warp: ") and word in msg, (what, msg)
        engine.set_band(0, 1)
        try:
            assert call() == JH_ERR_INVALID
            assert hip.jh_last_error(ctx).startswith(b"jh_warp: ") and b"band" in hip.jh_last_error(ctx)
        finally:
            engine.set_band()
        with pytest.raises(ValueError, match="jh_warp: "):
            engine.warp(src.id, src.id, IDENT)
        with pytest.raises(ValueError, match="jh_warp: "):
            engine.warp(src.id, dst.id, (0.0,) * 6)
        with pytest.raises(ValueError, match="jh_warp: "):
            engine.warp(src.id, dst.id, IDENT[:5])
        assert np.array_equal(src.bits(), canary) and np.array_equal(dst.bits(), canary)
        assert np.all(guard.bytes() == CANARY)
        assert call(m=(1.0 / 64.0, 0.0, 0.0, 1.0 / 64.0, 0.0, 0.0)) == 0  # (64:1 is accepted, and so is the plain call)
        assert call() == 0
        assert np.all(guard.bytes() == CANARY)
    finally:
        for im in (src, dst, rgba8, long_, guard):
            im.free()


def test_the_call_is_one_query_of_the_tree(engine):
    bits = warp_cases.content("unit", 48, 33, seed=2)
    m = warp_cases.rotate(45, (48, 33), (20, 40))
    src, dst = Image(engine, bits), Image(engine, None, 20, 40)
    try:
        engine.profile(True)
        try:
            with engine.profile_group("post"):
                engine.warp(src.id, dst.id, m, WarpFilter.BICUBIC, WarpEdge.MIRROR)
            tree = engine.profile_collect_tree()
            engine.warp(src.id, dst.id, m, WarpFilter.BICUBIC, WarpEdge.MIRROR)
            flat = engine.profile_collect()
        finally:
            engine.profile(False)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    assert [(n["kind"], n["label"], n["parent"], n["stage"]) for n in tree] == [("group", "post", -1, -1), ("query", "warp", 0, -1)]
    assert tree[1]["gpu_end_ms"] >= tree[1]["gpu_start_ms"]
    assert flat == []
    assert warp_ref.same_bits(got, warp_ref.warp(bits, (40, 20), m, warp_ref.BICUBIC, warp_ref.MIRROR))
