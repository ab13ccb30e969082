"""-m gpu: jh_resample against the rule of DESIGN.md 5.9 (tests/resample_ref.py) byte for byte -- the battery of
tests/resample_cases.py, a rendered frame, a captured frame -- and the call's frame: its tap tables and captures, its refusals, its
profile query."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, Fill, ImageFormat, Join, Path, RenderParams, ResampleFilter, Scene, Stroke, Surface
from jello_amd._lib import CResampleDesc
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS

import resample_cases
import resample_ref
import surface_ref
from devmem import CANARY, DevBuf, Image, _id, target_of

pytestmark = pytest.mark.gpu

JH_ERR_OOM = -5


def _differences(name, got, want):
    bad = np.argwhere(got != want)
    return "%s: %d of %d values differ, first at (y, x, ch) = %s: got %#06x, want %#06x" % (
        name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", [c["name"] for c in resample_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.resample: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = resample_cases.BY_NAME[name]
    src_bits, prior = resample_cases.source(c), resample_cases.before(c)
    src = Image(engine, None, *c["src_size"]) if c["kind"] == "never" else Image(engine, src_bits)
    dst = Image(engine, None, *c["dst_size"]) if prior is None else Image(engine, prior)
    try:
        engine.resample(src.id, dst.id, ResampleFilter(c["filter"]), c["src_rect"], c["dst_rect"], premultiplied=not c["flags"])
        got = dst.bits()
        if c["kind"] != "never":  # (a never-written image reads as zero; its memory holds anything)
            assert np.array_equal(src.bits(), src_bits)  # the source is only read
    finally:
        src.free()
        dst.free()
    want = resample_cases.expected(name)
    if not resample_ref.same_bits(got, want):
        pytest.fail(_differences(name, got, want))


def test_a_never_written_source_gives_transparent_black(engine):
    """... inside the rectangle (under both flag settings: 0 / max(0, 1e-6) is 0), and leaves the rest of dst alone."""
    src, dst = Image(engine, None, 40, 30), Image(engine, np.full((20, 25, 4), resample_cases.POISON, np.uint16))
    try:
        for premultiplied, rect in ((True, (1, 1, 11, 9)), (False, (13, 10, 12, 10))):
            engine.resample(src.id, dst.id, ResampleFilter.LANCZOS3, dst_rect=rect, premultiplied=premultiplied)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    want = np.full((20, 25, 4), resample_cases.POISON, np.uint16)
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    assert np.array_equal(got, want)


def _scene():
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid((0.9, 0.4, 0.1, 1.0)), None, Path.circle(50, 44, 30))
    curve = Path().move_to(10, 100).cubic_to(40, 4, 90, 120, 120, 16)
    s.stroke(Stroke(5, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None, curve)
    return s, RenderParams(128, 128)


@pytest.mark.parametrize("filt", list(ResampleFilter))
def test_rendered_scene(engine, filt):
    """A rendered 128 x 128 frame (a circle and a stroked curve, translucent edges) resized to 48 x 40 = the reference on the download
    of the same render."""
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    plain = target_of(engine, rec)
    assert plain.any()
    dst = Image(engine, None, 48, 40)
    try:
        engine.resample(rec.target["id"], dst.id, filt)
        got = dst.bits()
    finally:
        dst.free()
    want = resample_ref.resample(plain, (40, 48), int(filt))
    assert resample_ref.same_bits(got, want), _differences(filt.name, got, want)
    assert np.array_equal(target_of(engine, rec), plain)


def test_captured_with_the_frame(engine):
    """capture(resample=..., surface=...): render, resize into a second image, blit that image at its size -- replayed twice, the
    bytes of the eager calls."""
    s, p = _scene()
    fmt, filt = Surface.RGBA8_SRGB, ResampleFilter.CATMULL_ROM
    rec = jello_amd.Host().record(s, p)
    small, surf = Image(engine, None, 48, 40), DevBuf(engine, 48 * 40 * 4)
    g = None
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        t = rec.target
        plain = target_of(engine, rec)
        engine.resample(t["id"], small.id, filt)
        engine.blit(small.id, 48, 40, fmt, out_device_ptr=surf.ptr)
        eager = surf.bytes()[:48 * 40 * 4].reshape(40, 48, 4)
        resized = resample_ref.resample(plain, (40, 48), int(filt))
        assert resample_ref.same_bits(small.bits(), resized)
        assert np.array_equal(eager, surface_ref.convert(resized, int(fmt)))
        g0 = engine.capture(rec)
        g = engine.capture(rec, resample=dict(dst=small.id, width=48, height=40, filter=filt), surface=(surf.ptr, 48 * 4, fmt))
        (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
        engine.graph_destroy(g0)
        assert (k1, o1) == (k0 + 3, o0)  # rows, columns, blit: the tables are resident, nothing is uploaded
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


def _captured_call(engine, src, dst, desc, clear_first=None):
    """jh_resample between jh_graph_begin and jh_graph_end (after the clear of a buffer, if one is given): (rc, message, graph)."""
    hip, ctx = engine.hip, engine.ctx
    engine._check(hip.jh_graph_begin(ctx), "graph_begin")
    try:
        if clear_first is not None:
            engine.clear(clear_first)
        rc = hip.jh_resample(ctx, src.id, dst.id, ctypes.byref(desc))
        msg = hip.jh_last_error(ctx).decode()
    finally:
        g = ctypes.c_void_p()
        engine._check(hip.jh_graph_end(ctx, ctypes.byref(g)), "graph_end")
    return rc, msg, g


def test_captures_and_the_resident_geometry(engine):
    """A capture whose geometry is not the resident one is refused with the advice and touches nothing; after one eager call it is
    recorded (and runs nothing); an eager call with another geometry then makes that graph stale."""
    hip, ctx = engine.hip, engine.ctx
    bits = resample_cases.content("unit", 60, 44, seed=1)
    poison = np.full((17, 23, 4), resample_cases.POISON, np.uint16)
    src, dst, other, buf = Image(engine, bits), Image(engine, poison), Image(engine, None, 30, 22), DevBuf(engine, 64)
    d = CResampleDesc(int(ResampleFilter.TRIANGLE), 0, 0, 0, 0, 0, 0, 0, 0, 0)
    g = None
    try:
        engine.resample(src.id, other.id, ResampleFilter.TRIANGLE)  # (another geometry is resident)
        rc, msg, refused = _captured_call(engine, src, dst, d, clear_first=buf.id)
        engine.graph_destroy(refused)
        assert rc == JH_ERR_OOM and msg.startswith("jh_resample: ") and "resample this geometry once eagerly first" in msg, (rc, msg)
        assert np.array_equal(dst.bits(), poison) and np.array_equal(src.bits(), bits)
        engine.resample(src.id, dst.id, ResampleFilter.TRIANGLE)
        want = resample_ref.resample(bits, (17, 23), resample_ref.TRIANGLE)
        assert resample_ref.same_bits(dst.bits(), want)
        engine.upload_image(dst.id, poison)
        rc, msg, g = _captured_call(engine, src, dst, d)
        assert rc == 0, msg
        assert np.array_equal(dst.bits(), poison)  # a capture runs nothing
        engine.replay(g)
        assert resample_ref.same_bits(dst.bits(), want)
        # the same geometry again, eagerly: nothing is uploaded, the graph stays valid
        engine.resample(src.id, dst.id, ResampleFilter.TRIANGLE, premultiplied=False)
        engine.replay(g)
        assert resample_ref.same_bits(dst.bits(), want)
        # another filter is another geometry: its tables replace the ones the graph reads
        engine.resample(src.id, dst.id, ResampleFilter.BOX)
        assert hip.jh_graph_launch(ctx, g) == JH_ERR_INVALID
        assert b"stale" in hip.jh_last_error(ctx)
        assert resample_ref.same_bits(dst.bits(), resample_ref.resample(bits, (17, 23), resample_ref.BOX))
    finally:
        if g is not None:
            engine.graph_destroy(g)
        for im in (src, dst, other, buf):
            im.free()


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_resample: ", no texel of either image and no
    byte of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = np.full((H, W, 4), CANARY | (CANARY << 8), np.uint16)
    src, dst = Image(engine, canary), Image(engine, canary)
    wide = Image(engine, np.full((2, 40, 4), CANARY | (CANARY << 8), np.uint16))  # 40 x 2 and 2 x 40: 34 texels onto 2 are 17:1
    tall = Image(engine, np.full((40, 2, 4), CANARY | (CANARY << 8), np.uint16))
    rgba8 = Image(engine, np.full((H, W, 2), 0x1111, np.uint16), fmt=ImageFormat.RGBA8)  # (W x H texels of 4 bytes)
    guard = DevBuf(engine, 256)

    def call(s=None, d=None, desc=(2, 0, 0, 0, 0, 0, 0, 0, 0, 0)):
        return hip.jh_resample(ctx, src.id if s is None else s, dst.id if d is None else d, None if desc is None else ctypes.byref(CResampleDesc(*desc)))

    refused = {
        "null descriptor": lambda: call(desc=None),
        "unknown source": lambda: call(s=_id()),
        "unknown destination": lambda: call(d=_id()),
        "source not RGBA16F": lambda: call(s=rgba8.id),
        "destination not RGBA16F": lambda: call(d=rgba8.id),
        "filter 4": lambda: call(desc=(4, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
        "filter -1": lambda: call(desc=(-1, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
        "flag bit 1": lambda: call(desc=(2, 2, 0, 0, 0, 0, 0, 0, 0, 0)),
        "flag bit 31": lambda: call(desc=(2, 0x80000001, 0, 0, 0, 0, 0, 0, 0, 0)),
        "source rectangle beyond the right edge": lambda: call(desc=(2, 0, 8, 0, 9, 4, 0, 0, 0, 0)),
        "source rectangle beyond the bottom edge": lambda: call(desc=(2, 0, 0, 9, 4, 4, 0, 0, 0, 0)),
        "source rectangle whose end wraps": lambda: call(desc=(2, 0, 0xFFFFFFFF, 0, 2, 2, 0, 0, 0, 0)),
        "source rectangle empty in x only": lambda: call(desc=(2, 0, 2, 2, 0, 4, 0, 0, 0, 0)),
        "source rectangle empty in y only": lambda: call(desc=(2, 0, 2, 2, 4, 0, 0, 0, 0, 0)),
        "destination rectangle beyond the right edge": lambda: call(desc=(2, 0, 0, 0, 0, 0, 8, 0, 9, 4)),
        "destination rectangle beyond the bottom edge": lambda: call(desc=(2, 0, 0, 0, 0, 0, 0, 9, 4, 4)),
        "destination rectangle whose end wraps": lambda: call(desc=(2, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 2, 2)),
        "destination rectangle empty in x only": lambda: call(desc=(2, 0, 0, 0, 0, 0, 2, 2, 0, 4)),
        "destination rectangle empty in y only": lambda: call(desc=(2, 0, 0, 0, 0, 0, 2, 2, 4, 0)),
        "17:1 on x": lambda: call(s=wide.id, desc=(2, 0, 0, 0, 34, 2, 0, 0, 2, 2)),
        "17:1 on y": lambda: call(s=tall.id, desc=(2, 0, 0, 0, 2, 34, 0, 0, 2, 2)),
        "source is the destination": lambda: call(d=src.id),
    }
    try:
        for what, f in refused.items():
            assert f() == JH_ERR_INVALID, what
            assert hip.jh_last_error(ctx).startswith(b"jh_resample: "), (what, hip.jh_last_error(ctx))
        engine.set_band(0, 1)
        try:
            assert call() == JH_ERR_INVALID
            assert hip.jh_last_error(ctx).startswith(b"jh_resample: ") and b"band" in hip.jh_last_error(ctx)
        finally:
            engine.set_band()
        with pytest.raises(ValueError, match="jh_resample: "):
            engine.resample(src.id, src.id)
        with pytest.raises(ValueError, match="jh_resample: "):
            engine.resample(wide.id, dst.id, src_rect=(0, 0, 34, 2), dst_rect=(0, 0, 2, 2))
        assert np.array_equal(src.bits(), canary) and np.array_equal(dst.bits(), canary)
        assert np.all(guard.bytes() == CANARY)
        assert call(s=wide.id, desc=(2, 0, 0, 0, 32, 2, 0, 0, 2, 2)) == 0  # (16:1 is accepted, and so is the plain call)
        assert call() == 0
        assert np.all(guard.bytes() == CANARY)
    finally:
        for im in (src, dst, wide, tall, rgba8, guard):
            im.free()


def test_the_call_is_one_query_of_the_tree(engine):
    bits = resample_cases.content("unit", 48, 33, seed=2)
    src, dst = Image(engine, bits), Image(engine, None, 20, 40)
    try:
        engine.profile(True)
        try:
            with engine.profile_group("post"):
                engine.resample(src.id, dst.id, ResampleFilter.LANCZOS3)  # (a new geometry: the upload is inside the query)
            tree = engine.profile_collect_tree()
            engine.resample(src.id, dst.id, ResampleFilter.LANCZOS3)
            flat = engine.profile_collect()
        finally:
            engine.profile(False)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    assert [(n["kind"], n["label"], n["parent"], n["stage"]) for n in tree] == [("group", "post", -1, -1), ("query", "resample", 0, -1)]
    assert tree[1]["gpu_end_ms"] >= tree[1]["gpu_start_ms"]
    assert flat == []
    assert resample_ref.same_bits(got, resample_ref.resample(bits, (40, 20), resample_ref.LANCZOS3))
