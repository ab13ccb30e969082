"""-m gpu: jh_color_filter against the rule of DESIGN.md 5.10 (tests/color_ref.py) byte for byte -- the battery of
tests/color_cases.py, rendered frames, a captured frame -- and the call's frame: its tables and captures, its refusals, its profile
query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, ColorSpace, Compose, Fill, ImageFormat, Join, Path, RenderParams, Scene, Stroke, Surface
from jello_amd import colorfilter as cf
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS, _color_desc

import color_cases
import color_ref
import composite_ref
import surface_ref
from devmem import CANARY, DevBuf, Image, _id, target_of

pytestmark = pytest.mark.gpu

JH_ERR_OOM = -5
_EXPECTED = {}


def _expected(name):
    """The reference on a value case, computed once for the tests of this file."""
    if name not in _EXPECTED:
        _EXPECTED[name] = color_ref.texels(color_cases.VALUES, **color_cases.VALUE_CASES[name])
    return _EXPECTED[name]


def _differences(name, got, want):
    bad = np.argwhere(got != want)
    return "%s: %d of %d values differ, first at (y, x, ch) = %s: got %#06x, want %#06x" % (
        name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _kw(case):
    return dict(case, space=ColorSpace(case["space"]))


@pytest.mark.parametrize("name", sorted(color_cases.VALUE_CASES))
def test_values(engine, name):
    """Every value case on the image of every f16 bit pattern, into a second image: every byte is the reference's (a NaN is
    0x7e00 on both sides), and the source is only read."""
    src, dst = Image(engine, color_cases.VALUES), Image(engine, None, 256, color_cases.VALUES.shape[0])
    try:
        engine.color_filter(src.id, dst.id, **_kw(color_cases.VALUE_CASES[name]))
        got = dst.bits()
        assert np.array_equal(src.bits(), color_cases.VALUES)
    finally:
        src.free()
        dst.free()
    want = _expected(name)
    if not np.array_equal(got, want):
        pytest.fail(_differences(name, got, want))


@pytest.mark.parametrize("in_place", (False, True), ids=("second_image", "in_place"))
@pytest.mark.parametrize("width", color_cases.WIDTHS)
def test_geometry(engine, width, in_place):
    """The rectangle widths at the kernel's seams, by heights, offsets and image widths of both parities, with and without tables:
    NaN around the source's rectangle, poison around the destination's; the rectangle is the reference's and no byte outside it
    changes."""
    for n, g in enumerate(color_cases.geometry(width)):
        kw = color_cases.geometry_filter(g["tables"])
        content = color_cases.geometry_source(g["size"], seed=width * 100 + n)
        src_bits = color_cases.surround(content, g["rect"], color_cases.NAN_BITS)
        if in_place:
            src = dst = Image(engine, src_bits)
            prior = src_bits
        else:
            prior = np.full_like(src_bits, color_cases.POISON)
            src, dst = Image(engine, src_bits), Image(engine, prior)
        try:
            engine.color_filter(src.id, None if in_place else dst.id, rect=g["rect"], **_kw(kw))
            got = dst.bits()
            if not in_place:
                assert np.array_equal(src.bits(), src_bits)
        finally:
            src.free()
            if not in_place:
                dst.free()
        want = color_ref.apply(src_bits, rect=g["rect"], dst_bits=prior, **kw)
        if not np.array_equal(got, want):
            pytest.fail(_differences(str(g), got, want))


def test_never_written_images(engine):
    """A never-written source reads as transparent black, so the rectangle takes what the rule makes of zeros (the offsets); a
    never-written destination is cleared outside the rectangle; both at once, in place."""
    kw = dict(matrix=color_cases.DENSE, funcs=(cf.linear(0.5, 0.25), None, None, cf.gamma(1.0, 2.0, 0.5)), space=color_ref.SRGB, clamp=True)
    zeros = np.zeros((9, 21, 4), np.uint16)
    content = color_cases.geometry_source((21, 9), seed=3)
    poison = np.full((9, 21, 4), color_cases.POISON, np.uint16)
    rect = (3, 2, 11, 5)
    empty, poisoned, full, fresh, alone = Image(engine, None, 21, 9), Image(engine, poison), Image(engine, content), Image(engine, None, 21, 9), Image(engine, None, 21, 9)
    try:
        engine.color_filter(empty.id, poisoned.id, rect=rect, **_kw(kw))
        assert np.array_equal(poisoned.bits(), color_ref.apply(zeros, rect=rect, dst_bits=poison, **kw))
        engine.color_filter(full.id, fresh.id, rect=rect, **_kw(kw))
        want = color_ref.apply(content, rect=rect, dst_bits=None, **kw)
        assert np.all(want[0] == 0) and want[2:7, 3:14].any()
        assert np.array_equal(fresh.bits(), want)
        engine.color_filter(alone.id, rect=rect, **_kw(kw))
        assert np.array_equal(alone.bits(), color_ref.apply(zeros, rect=rect, dst_bits=None, **kw))
    finally:
        for im in (empty, poisoned, full, fresh, alone):
            im.free()


def _scene(color=(0.9, 0.4, 0.1, 1.0)):
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid(color), None, Path.circle(50, 44, 30))
    curve = Path().move_to(10, 100).cubic_to(40, 4, 90, 120, 120, 16)
    s.stroke(Stroke(5, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None, curve)
    return s, RenderParams(128, 128)


def test_rendered_scene_through_grayscale(engine):
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    plain = target_of(engine, rec)
    assert plain.any()
    kw = cf.grayscale(1.0)
    engine.color_filter(rec.target["id"], **kw)
    got = target_of(engine, rec)
    want = color_ref.apply(plain, dst_bits=plain, **dict(kw, space=color_ref.SRGB))
    assert np.array_equal(got, want), _differences("grayscale", got, want)
    inside = got[44, 50].view(np.float16)
    assert inside[0] == inside[1] == inside[2] and inside[3] == 1.0  # grey, opaque


def test_luminance_mask(engine):
    """Engine.luminance_mask on two rendered layers: the mask's luminance into the scratch's alpha, the layer kept where it is."""
    layer_scene, p = _scene()
    mask_scene = Scene()
    mask_scene.fill(Fill.NonZero, None, Brush.solid((1.0, 1.0, 1.0, 1.0)), None, Path.circle(64, 64, 40))
    mask_scene.fill(Fill.NonZero, None, Brush.solid((0.2, 0.6, 0.1, 0.7)), None, Path.circle(40, 50, 25))
    scratch = Image(engine, None, 128, 128)
    mask = None
    try:
        mrec, _, _ = engine.render(mask_scene, p)
        mask_bits = target_of(engine, mrec)
        mask = Image(engine, mask_bits)
        rec, _, _ = engine.render(layer_scene, p)
        layer_bits = target_of(engine, rec)
        assert mask_bits.any() and layer_bits.any() and not np.array_equal(mask_bits, layer_bits)
        engine.luminance_mask(rec.target["id"], mask.id, scratch.id)
        got = target_of(engine, rec)
        lum = color_ref.apply(mask_bits, **dict(cf.luminance_to_alpha(), space=color_ref.LINEAR))
        assert np.array_equal(scratch.bits(), lum)
        want = composite_ref.composite(lum, layer_bits, compose=int(Compose.DestIn))
        assert composite_ref.same_bits(got, want), _differences("luminance mask", got, want)
        assert got[44, 50, 3] != 0 and got[100, 120, 3] == 0  # kept under the mask's white disc, gone outside it
    finally:
        scratch.free()
        if mask is not None:
            mask.free()


def test_captured_with_the_frame(engine):
    """capture(color=..., surface=...): render, filter the target in place, blit it -- replayed twice, the bytes of the eager calls."""
    s, p = _scene()
    fmt, kw = Surface.RGBA8_SRGB, cf.sepia(1.0)
    rec = jello_amd.Host().record(s, p)
    surf = DevBuf(engine, 128 * 128 * 4)
    g = None
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        t = rec.target
        plain = target_of(engine, rec)
        engine.color_filter(t["id"], **kw)
        engine.blit(t["id"], 128, 128, fmt, out_device_ptr=surf.ptr)
        eager = surf.bytes()[:128 * 128 * 4].reshape(128, 128, 4)
        toned = color_ref.apply(plain, dst_bits=plain, **dict(kw, space=color_ref.SRGB))
        assert np.array_equal(target_of(engine, rec), toned)
        assert np.array_equal(eager, surface_ref.convert(toned, int(fmt)))
        g0 = engine.capture(rec)
        g = engine.capture(rec, color=kw, surface=(surf.ptr, 128 * 4, fmt))
        (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
        engine.graph_destroy(g0)
        assert (k1, o1) == (k0 + 2, o0)  # the filter and the blit: the tables are resident, nothing is uploaded
        for _ in range(2):
            engine.clear(surf.id)
            engine.replay(g)
            engine.sync()
            assert np.array_equal(surf.bytes()[:128 * 128 * 4].reshape(128, 128, 4), eager)
            assert np.array_equal(target_of(engine, rec), toned)
    finally:
        if g is not None:
            engine.graph_destroy(g)
        surf.free()


def _captured_call(engine, src, dst, desc, clear_first=None):
    """jh_color_filter between jh_graph_begin and jh_graph_end (after the clear of a buffer, if one is given): (rc, message, graph)."""
    hip, ctx = engine.hip, engine.ctx
    engine._check(hip.jh_graph_begin(ctx), "graph_begin")
    try:
        if clear_first is not None:
            engine.clear(clear_first)
        rc = hip.jh_color_filter(ctx, src.id, dst.id, ctypes.byref(desc))
        msg = hip.jh_last_error(ctx).decode()
    finally:
        g = ctypes.c_void_p()
        engine._check(hip.jh_graph_end(ctx, ctypes.byref(g)), "graph_end")
    return rc, msg, g


def test_captures_and_the_resident_key():
    """On a fresh context: a call that needs no tables is capturable at once and takes no scratch; a capture whose key is not
    resident is refused with the advice and touches nothing; after one eager call it is recorded (and runs nothing); the same key
    again, with another matrix, uploads nothing and leaves the graph valid; another key makes it stale; jh_scratch_trim forgets
    the key."""
    engine = jello_amd.Engine(0)
    hip, ctx = engine.hip, engine.ctx
    bits = color_cases.geometry_source((37, 19), seed=8)
    poison = np.full((19, 37, 4), color_cases.POISON, np.uint16)
    src, dst, buf = Image(engine, bits), Image(engine, poison), DevBuf(engine, 64)
    gray, sepia, lum = cf.grayscale(1.0), cf.sepia(1.0), cf.luminance_to_alpha()
    ref = lambda kw, **more: color_ref.apply(bits, dst_bits=poison, **dict(kw, space=int(kw["space"]), **more))  # noqa: E731
    slot = 17  # JH_SCR_COLOR_TABLES
    graphs = []
    try:
        # no tables: capturable on a fresh context, and the slot stays empty
        rc, msg, g = _captured_call(engine, src, dst, _color_desc(rect=None, **lum))
        graphs.append(g)
        assert rc == 0, msg
        assert np.array_equal(dst.bits(), poison)  # a capture runs nothing
        engine.replay(g)
        assert np.array_equal(dst.bits(), ref(lum))
        assert hip.jh_debug_scratch_bytes(ctx, slot) == 0
        engine.upload_image(dst.id, poison)
        # a key that is not resident
        rc, msg, refused = _captured_call(engine, src, dst, _color_desc(rect=None, **gray), clear_first=buf.id)
        engine.graph_destroy(refused)
        assert rc == JH_ERR_OOM and msg.startswith("jh_color_filter: ") and "run this filter once eagerly first" in msg, (rc, msg)
        assert np.array_equal(dst.bits(), poison) and np.array_equal(src.bits(), bits)
        engine.color_filter(src.id, dst.id, **gray)
        assert np.array_equal(dst.bits(), ref(gray))
        assert hip.jh_debug_scratch_bytes(ctx, slot) >= 3 * 65536 * 4 + 4 * 65536 * 2
        engine.upload_image(dst.id, poison)
        rc, msg, g = _captured_call(engine, src, dst, _color_desc(rect=None, **gray))
        graphs.append(g)
        assert rc == 0, msg
        assert np.array_equal(dst.bits(), poison)
        engine.replay(g)
        assert np.array_equal(dst.bits(), ref(gray))
        # the same key with another matrix (sepia differs from grayscale in the matrix alone), and a call without tables: nothing
        # is uploaded, the graph stays valid
        engine.color_filter(src.id, dst.id, **sepia)
        assert np.array_equal(dst.bits(), ref(sepia))
        engine.color_filter(src.id, dst.id, **lum)
        engine.replay(g)
        assert np.array_equal(dst.bits(), ref(gray))
        # another key: its tables replace the ones the graph reads
        engine.color_filter(src.id, dst.id, **cf.invert(1.0))
        assert hip.jh_graph_launch(ctx, g) == JH_ERR_INVALID
        assert b"stale" in hip.jh_last_error(ctx)
        assert np.array_equal(dst.bits(), ref(cf.invert(1.0)))
        # a trim forgets the key: the same filter is no longer capturable until it has run again
        engine._check(hip.jh_scratch_trim(ctx), "scratch_trim")
        rc, msg, refused = _captured_call(engine, src, dst, _color_desc(rect=None, **cf.invert(1.0)))
        engine.graph_destroy(refused)
        assert rc == JH_ERR_OOM and "run this filter once eagerly first" in msg
        engine.color_filter(src.id, dst.id, **cf.invert(1.0))
        assert np.array_equal(dst.bits(), ref(cf.invert(1.0)))
    finally:
        for g in graphs:
            engine.graph_destroy(g)
        for im in (src, dst, buf):
            im.free()
        engine.close()


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_color_filter: ", no texel of either image and
    no byte of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = np.full((H, W, 4), CANARY | (CANARY << 8), np.uint16)
    src, dst = Image(engine, canary), Image(engine, canary)
    small = Image(engine, np.full((6, 8, 4), CANARY | (CANARY << 8), np.uint16))
    rgba8 = Image(engine, np.full((H, W, 2), 0x1111, np.uint16), fmt=ImageFormat.RGBA8)  # (W x H texels of 4 bytes)
    guard = DevBuf(engine, 256)
    inf, nan = math.inf, math.nan

    def call(s=None, d=None, null=False, rect=None, flags=None, **kw):
        args = dict(matrix=None, funcs=None, space=0, clamp=True)
        args.update(kw)
        desc = _color_desc(rect=rect, **args)
        if flags is not None:
            desc.flags = flags
        return hip.jh_color_filter(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

    def matrix_with(k, v):
        m = list(color_ref.IDENTITY)
        m[k] = v
        return m

    refused = {
        "null descriptor": lambda: call(null=True),
        "unknown source": lambda: call(s=_id()),
        "unknown destination": lambda: call(d=_id()),
        "source not RGBA16F": lambda: call(s=rgba8.id),
        "destination not RGBA16F": lambda: call(d=rgba8.id),
        "rectangle beyond the right edge": lambda: call(rect=(8, 0, 9, 4)),
        "rectangle beyond the bottom edge": lambda: call(rect=(0, 9, 4, 4)),
        "rectangle whose end wraps": lambda: call(rect=(0xFFFFFFFF, 0, 2, 2)),
        "rectangle empty in x only": lambda: call(rect=(2, 2, 0, 4)),
        "rectangle empty in y only": lambda: call(rect=(2, 2, 4, 0)),
        "rectangle outside the destination only": lambda: call(d=small.id, rect=(4, 2, 6, 3)),
        "rectangle outside the source only": lambda: call(s=small.id, rect=(4, 2, 6, 3)),
        "the whole source does not fit the destination": lambda: call(d=small.id),
        "space 2": lambda: call(space=2),
        "space -1": lambda: call(space=-1),
        "flag bit 1": lambda: call(flags=2),
        "flag bit 31": lambda: call(flags=0x80000001),
        "func type 5": lambda: call(funcs=(None, (5,), None, None)),
        "func type -1": lambda: call(funcs=(None, None, None, (-1,))),
        "matrix entry NaN": lambda: call(matrix=matrix_with(7, nan)),
        "matrix offset Inf": lambda: call(matrix=matrix_with(19, inf)),
        "slope Inf": lambda: call(funcs=(cf.linear(inf, 0.0), None, None, None)),
        "exponent NaN": lambda: call(funcs=(None, cf.gamma(1.0, nan, 0.0), None, None)),
        "a table value -Inf": lambda: call(funcs=(None, None, cf.table([0.0, -inf]), None)),
        "table of 0": lambda: call(funcs=(cf.table([]), None, None, None)),
        "discrete of 65": lambda: call(funcs=(None, None, None, cf.discrete([0.5] * 65))),
    }
    try:
        for what, f in refused.items():
            assert f() == JH_ERR_INVALID, what
            assert hip.jh_last_error(ctx).startswith(b"jh_color_filter: "), (what, hip.jh_last_error(ctx))
        engine.set_band(0, 1)
        try:
            assert call() == JH_ERR_INVALID
            assert hip.jh_last_error(ctx).startswith(b"jh_color_filter: ") and b"band" in hip.jh_last_error(ctx)
        finally:
            engine.set_band()
        with pytest.raises(ValueError, match="jh_color_filter: "):
            engine.color_filter(src.id, dst.id, rect=(8, 0, 9, 4))
        with pytest.raises(ValueError, match="jh_color_filter: "):
            engine.color_filter(src.id, funcs=(cf.table([]), None, None, None))
        assert np.array_equal(src.bits(), canary) and np.array_equal(dst.bits(), canary) and np.all(small.bits() == (CANARY | (CANARY << 8)))
        assert np.all(guard.bytes() == CANARY)
        assert call(s=small.id) == 0  # (the whole of a smaller source fits, and so does the plain call in place)
        assert call(d=src.id) == 0
        assert np.all(guard.bytes() == CANARY)
    finally:
        for im in (src, dst, small, rgba8, guard):
            im.free()


def test_the_call_is_one_query_of_the_tree(engine):
    bits = color_cases.geometry_source((48, 33), seed=2)
    src, dst = Image(engine, bits), Image(engine, None, 48, 33)
    kw = cf.contrast(1.7)
    try:
        engine.profile(True)
        try:
            with engine.profile_group("post"):
                engine.color_filter(src.id, dst.id, **kw)  # (a new key: the upload is inside the query)
            tree = engine.profile_collect_tree()
            engine.color_filter(src.id, dst.id, **kw)
            flat = engine.profile_collect()
        finally:
            engine.profile(False)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    assert [(n["kind"], n["label"], n["parent"], n["stage"]) for n in tree] == [("group", "post", -1, -1), ("query", "color", 0, -1)]
    assert tree[1]["gpu_end_ms"] >= tree[1]["gpu_start_ms"]
    assert flat == []
    assert np.array_equal(got, color_ref.apply(bits, **dict(kw, space=color_ref.SRGB)))
