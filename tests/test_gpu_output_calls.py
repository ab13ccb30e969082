"""-m gpu: what the post-render calls -- jh_blit, jh_blit_yuv, jh_pack_tiles, jh_unpack_tiles, jh_dash -- share: each is one
query of the profile tree (stage -1, no flat record), each launches the held-back commands before its own work, and each
refused call answers JH_ERR_INVALID with a message that starts with the entry point's own name -- which the Engine method raises
as the exception it documents."""
import ctypes

import numpy as np
import pytest

from jello_amd import Path, Surface, YuvLayout, tilepack
from jello_amd._lib import CDashPath
from jello_amd.engine import JH_ERR_INVALID

import surface_ref
import tilepack_ref
import yuv_ref
from devmem import CANARY, DevBuf, Image, _id

pytestmark = pytest.mark.gpu

W, H = 48, 33  # not tile-aligned; the odd height has a chroma row with one luma row above it


def test_the_five_calls_are_queries_of_one_tree(engine):
    bits = np.random.default_rng(7).random((H, W, 4), dtype=np.float32).astype(np.float16).view(np.uint16)
    img = Image(engine, bits)
    bound = tilepack.bound(W, H, 4)
    surf, pack, back = DevBuf(engine, 4 * W * H), DevBuf(engine, bound), DevBuf(engine, 4 * W * H)
    two_lines, no_segment = Path().move_to(0, 0).line_to(10, 0).line_to(10, 10), Path().move_to(5, 5)
    got = {}

    def calls():
        engine.blit(img.id, W, H, Surface.RGBA8_UNORM, out_device_ptr=surf.ptr)
        got["yuv"] = engine.blit_yuv(img.id, W, H, YuvLayout.NV12)
        engine.pack_tiles(surf.ptr, 4 * W, W, H, 4, out_device_ptr=pack.ptr)
        engine.unpack_tiles((pack.ptr, bound), back.ptr, 4 * W, W, H, 4)
        got["dash"] = engine.dash_paths([two_lines], [[3, 2]], [0.0], raw=True)
        got["empty"] = engine.dash_paths([no_segment], [[3, 2]], [0.0], raw=True)

    try:
        engine.profile(True)
        try:
            with engine.profile_group("post"):
                calls()
            tree = engine.profile_collect_tree()
            calls()
            flat = engine.profile_collect()
        finally:
            engine.profile(False)
        calls()
        engine.profile(True)
        try:
            tree_off = engine.profile_collect_tree()
        finally:
            engine.profile(False)
        surface = surf.bytes().reshape(H, W, 4)
        unpacked = back.bytes().reshape(H, W, 4)
    finally:
        img.free()
        for b in (surf, pack, back):
            b.free()
    groups = [i for i, n in enumerate(tree) if n["kind"] == "group"]
    assert len(groups) == 1 and tree[groups[0]]["label"] == "post" and tree[groups[0]]["parent"] == -1
    queries = [n for n in tree if n["kind"] == "query"]
    assert sorted(n["label"] for n in queries) == ["blit", "blit_yuv", "dash", "dash", "pack", "unpack"]
    assert len(tree) == 7
    for n in queries:
        assert n["stage"] == -1 and n["parent"] == groups[0] and n["gpu_end_ms"] >= n["gpu_start_ms"], n
    assert flat == []
    assert tree_off == []
    # and the calls did their work on a frame of this shape
    want = surface_ref.convert(bits, int(Surface.RGBA8_UNORM))
    assert np.array_equal(surface, want) and np.array_equal(unpacked, want)
    for g, w in zip(got["yuv"], yuv_ref.convert(bits, 0, 1, 0, 0)):  # NV12, BT.709, limited range, no transfer: blit_yuv's defaults
        assert np.array_equal(g, w)
    els, index = got["dash"]
    assert list(index) == [0, len(els)] and len(els) > 0
    assert len(got["empty"][0]) == 0 and list(got["empty"][1]) == [0, 0]


def test_a_post_render_call_launches_what_is_held_back_first(engine):
    """A whole-buffer clear of a buffer of a JlBump's size is held back; the call that reads or writes the buffer next has to
    launch it first."""
    zero = np.zeros((1, 8, 4), np.uint8)
    solid = np.full((1, 8, 4), 0x11, np.uint8)
    bufs = [DevBuf(engine, 32) for _ in range(3)]
    packs = [DevBuf(engine, data=tilepack_ref.pack(zero, zero)), DevBuf(engine, data=tilepack_ref.pack(solid))]
    try:
        assert np.all(bufs[0].bytes() == CANARY)
        engine.clear(bufs[0].id)
        assert engine.pack_tiles(bufs[0].ptr, 32, 8, 1, 4) == tilepack_ref.pack(zero)  # without the flush: 0xA7 texels
        # unpack as the consumer: a pack whose single tile is skipped writes nothing ...
        engine.clear(bufs[1].id)
        engine.unpack_tiles((packs[0].ptr, packs[0].n), bufs[1].ptr, 32, 8, 1, 4)
        assert np.all(bufs[1].bytes() == 0)
        # ... and a solid tile must land after the clear (without the flush the clear would run later and wipe it)
        engine.clear(bufs[2].id)
        engine.unpack_tiles((packs[1].ptr, packs[1].n), bufs[2].ptr, 32, 8, 1, 4)
        assert np.array_equal(bufs[2].bytes(), solid.reshape(-1))
    finally:
        for b in bufs + packs:
            b.free()


def test_messages_keep_their_prefixes(engine):
    """One refused call per entry point on a 16 x 16 frame: JH_ERR_INVALID, the entry point's name in front, nothing written."""
    hip, ctx = engine.hip, engine.ctx
    img = Image(engine, np.full((16, 16, 4), 0x3C00, np.uint16))
    mem = DevBuf(engine, 4096)
    bound = tilepack.bound(16, 16, 4)
    line = Path().move_to(0, 0).line_to(12, 0)
    desc = (CDashPath * 1)()
    desc[0].first_el, desc[0].n_els, desc[0].first_dash, desc[0].n_dash, desc[0].offset = 0, 2, 0, 2, 0.0
    d, _ = engine._yuv_desc(16, 16, YuvLayout.NV12, 1, 0, 0, [(mem.ptr, 15), (mem.ptr + 256, None)])
    refused = {
        "jh_blit": lambda: hip.jh_blit(ctx, _id(), mem.ptr, 64, 16, 16, int(Surface.RGBA8_UNORM)),
        "jh_blit_yuv": lambda: hip.jh_blit_yuv(ctx, img.id, 16, 16, ctypes.byref(d)),
        "jh_pack_tiles": lambda: hip.jh_pack_tiles(ctx, mem.ptr, 64, None, 0, 16, 16, 4, mem.ptr + 1024, bound - 1),
        "jh_unpack_tiles": lambda: hip.jh_unpack_tiles(ctx, mem.ptr, 31, mem.ptr + 1024, 64, 16, 16, 4),
        "jh_dash": lambda: hip.jh_dash(ctx, line._c(), 2, desc, 1, (ctypes.c_double * 2)(4.0, -1.0), 2, mem.ptr, 64, mem.ptr + 2048),
    }
    try:
        for name, call in refused.items():
            assert call() == JH_ERR_INVALID, name
            assert hip.jh_last_error(ctx).startswith(name.encode() + b": "), (name, hip.jh_last_error(ctx))
        assert np.all(mem.bytes() == CANARY)
    finally:
        img.free()
        mem.free()


def test_the_way_out_and_the_way_in_refuse_the_same_frame_faults_in_the_same_words(engine):
    """include/jello_frame.h from both sides, on a 5 x 3 image with the planes in one canary buffer: a null pointer or a pitch one
    below the row's bytes at every plane index the layout uses, given to jh_blit_yuv and -- the same planes as a jh_load_yuv_desc -- to
    jh_load_yuv; a pitch one below 4 * width and the formats -1 and 4, given to jh_blit and jh_load_surface.  Every one is
    JH_ERR_INVALID with the same words behind the call's own prefix, and nothing is written.  Only after that, the pitches that
    are exactly the rows' bytes are accepted (the only launches of this test) and write nothing outside the planes' rows."""
    from jello_amd.engine import _load_surface_desc, _load_yuv_desc
    hip, ctx = engine.hip, engine.ctx
    w, h = 5, 3
    bits = np.random.default_rng(53).random((h, w, 4), dtype=np.float32).astype(np.float16).view(np.uint16)
    src, dst, mem = Image(engine, bits), Image(engine, bits), DevBuf(engine, 1024)

    def both_yuv(layout, planes):
        out, _ = engine._yuv_desc(w, h, layout, 1, 0, 0, planes)
        into = _load_yuv_desc(layout, 1, 0, 0, 1, planes, None)
        return [("jh_blit_yuv", hip.jh_blit_yuv(ctx, src.id, w, h, ctypes.byref(out)), hip.jh_last_error(ctx)),
                ("jh_load_yuv", hip.jh_load_yuv(ctx, dst.id, ctypes.byref(into)), hip.jh_last_error(ctx))]

    def both_surface(fmt, pitch):
        into = _load_surface_desc(fmt, 0, mem.ptr, pitch, None)
        return [("jh_blit", hip.jh_blit(ctx, src.id, mem.ptr, pitch, w, h, fmt), hip.jh_last_error(ctx)),
                ("jh_load_surface", hip.jh_load_surface(ctx, dst.id, ctypes.byref(into)), hip.jh_last_error(ctx))]

    def refused(answers, words):
        for name, rc, message in answers:
            assert rc == JH_ERR_INVALID and message == name.encode() + b": " + words, (name, rc, message, words)

    try:
        legal = {}
        for layout in (YuvLayout.NV12, YuvLayout.I420):
            shapes = engine.yuv_plane_shapes(w, h, layout)
            assert [rb for _, rb in shapes] == ([5, 6] if layout == YuvLayout.NV12 else [5, 3, 3])
            legal[layout] = [(mem.ptr + 256 * i, rb) for i, (_, rb) in enumerate(shapes)]
            for i, (ptr, rb) in enumerate(legal[layout]):
                refused(both_yuv(layout, legal[layout][:i] + [(None, rb)] + legal[layout][i + 1:]), b"null plane")
                refused(both_yuv(layout, legal[layout][:i] + [(ptr, rb - 1)] + legal[layout][i + 1:]), b"pitch below the row's bytes")
        refused(both_surface(int(Surface.BGRA8_SRGB), 4 * w - 1), b"pitch below 4 * width")
        for fmt in (-1, 4):
            refused(both_surface(fmt, 4 * w), b"unknown surface format")
        assert np.all(mem.bytes() == CANARY) and np.array_equal(src.bits(), bits) and np.array_equal(dst.bits(), bits)
        # the boundary's other side: exactly the rows' bytes (NV12 without a third plane)
        outside = np.ones(mem.n, bool)  # (of the rows written so far; I420 first: its chroma rows lie inside NV12's, so each is checked exactly)
        for layout in (YuvLayout.I420, YuvLayout.NV12):
            assert [rc for _, rc, _ in both_yuv(layout, legal[layout])] == [0, 0], layout
            for (rows, rb), i in zip(engine.yuv_plane_shapes(w, h, layout), range(3)):
                outside[256 * i:256 * i + rows * rb] = False
            assert np.all(mem.bytes()[outside] == CANARY), layout
        assert [rc for _, rc, _ in both_surface(int(Surface.BGRA8_SRGB), 4 * w)] == [0, 0]
        after = mem.bytes()  # (the surface's 4 w h bytes lie inside plane 0's 256; the chroma planes still hold I420's bytes)
        assert np.all(after[4 * w * h:256] == CANARY) and np.all(after[256 * 2 + 2 * 3:] == CANARY) and np.array_equal(src.bits(), bits)
    finally:
        src.free()
        dst.free()
        mem.free()


def test_engine_methods_raise_for_a_refused_call(engine):
    """One refused call per Engine method on a 16 x 16 image (one tile): the exception class the method documents -- ValueError
    for what the rule of blur and composite refuses, RuntimeError elsewhere -- with the entry point's own text in it, and the
    image's bits are what was uploaded."""
    bits = np.random.default_rng(16).random((16, 16, 4), dtype=np.float32).astype(np.float16).view(np.uint16)
    img = Image(engine, bits)
    mem = DevBuf(engine, 4096)
    refused = [
        (RuntimeError, "jh_blit: pitch below", lambda: engine.blit(img.id, 16, 16, Surface.RGBA8_UNORM, out_device_ptr=mem.ptr, pitch=4 * 16 - 4)),
        (RuntimeError, "jh_blit_yuv: pitch below", lambda: engine.blit_yuv(img.id, 16, 16, planes=[(mem.ptr, 15), (mem.ptr + 256, None)])),
        (RuntimeError, "jh_pack_tiles: source: texel_bytes", lambda: engine.pack_tiles(mem.ptr, 64, 16, 16, 3, out_device_ptr=mem.ptr + 1024)),
        (RuntimeError, "jh_unpack_tiles: pack_bytes below", lambda: engine.unpack_tiles((mem.ptr, 16), mem.ptr + 1024, 64, 16, 16, 4)),
        (ValueError, "jh_blur: ", lambda: engine.blur(img.id, 16, 16, 65.0)),
        (ValueError, "jh_composite: ", lambda: engine.composite(img.id, img.id)),
    ]
    try:
        for exc, text, call in refused:
            with pytest.raises(exc, match=text) as info:
                call()
            assert info.type is exc, (text, info.type)  # (not a subclass: ValueError is not RuntimeError, and the reverse)
        assert np.array_equal(engine.download_image(img.id, 16, 16), bits)
        assert np.all(mem.bytes() == CANARY)
    finally:
        img.free()
        mem.free()
