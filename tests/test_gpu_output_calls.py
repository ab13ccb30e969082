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
