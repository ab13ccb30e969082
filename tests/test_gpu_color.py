"""-m gpu: jh_color_filter against the rule of DESIGN.md 5.10 (tests/color_ref.py) byte for byte -- the battery of
tests/color_cases.py, rendered frames, a captured frame -- and the call's frame: its tables and captures, its refusals, its profile
query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, ColorSpace, Compose, Fill, ImageFormat, Path, Scene
from jello_amd import colorfilter as cf
from jello_amd.engine import JH_ERR_INVALID, _color_desc

import color_cases
import color_ref
import composite_ref
from devmem import target_of
from image_call import (JH_ERR_OOM, assert_equal_bits, assert_same_bits, canary_bits, captured_call, captured_with_the_frame, check_refusals,
                        common_refusals, images, one_query, scene)

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def _expected(name):
    """The reference on a value case, computed once for the tests of this file."""
    if name not in _EXPECTED:
        _EXPECTED[name] = color_ref.texels(color_cases.VALUES, **color_cases.VALUE_CASES[name])
    return _EXPECTED[name]


def _kw(case):
    return dict(case, space=ColorSpace(case["space"]))


@pytest.mark.parametrize("name", sorted(color_cases.VALUE_CASES))
def test_values(engine, name):
    """Every value case on the image of every f16 bit pattern, into a second image: every byte is the reference's (a NaN is
    0x7e00 on both sides), and the source is only read."""
    with images(engine, color_cases.VALUES, (256, color_cases.VALUES.shape[0])) as (src, dst):
        engine.color_filter(src.id, dst.id, **_kw(color_cases.VALUE_CASES[name]))
        got = dst.bits()
        assert np.array_equal(src.bits(), color_cases.VALUES)
    assert_equal_bits(got, _expected(name), name)


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
        prior = src_bits if in_place else np.full_like(src_bits, color_cases.POISON)
        with images(engine, src_bits, *([] if in_place else [prior])) as made:
            src, dst = made[0], made[-1]
            engine.color_filter(src.id, None if in_place else dst.id, rect=g["rect"], **_kw(kw))
            got = dst.bits()
            if not in_place:
                assert np.array_equal(src.bits(), src_bits)
        assert_equal_bits(got, color_ref.apply(src_bits, rect=g["rect"], dst_bits=prior, **kw), str(g))


def test_never_written_images(engine):
    """A never-written source reads as transparent black, so the rectangle takes what the rule makes of zeros (the offsets); a
    never-written destination is cleared outside the rectangle; both at once, in place."""
    kw = dict(matrix=color_cases.DENSE, funcs=(cf.linear(0.5, 0.25), None, None, cf.gamma(1.0, 2.0, 0.5)), space=color_ref.SRGB, clamp=True)
    zeros = np.zeros((9, 21, 4), np.uint16)
    content = color_cases.geometry_source((21, 9), seed=3)
    poison = np.full((9, 21, 4), color_cases.POISON, np.uint16)
    rect = (3, 2, 11, 5)
    with images(engine, (21, 9), poison, content, (21, 9), (21, 9)) as (empty, poisoned, full, fresh, alone):
        engine.color_filter(empty.id, poisoned.id, rect=rect, **_kw(kw))
        assert np.array_equal(poisoned.bits(), color_ref.apply(zeros, rect=rect, dst_bits=poison, **kw))
        engine.color_filter(full.id, fresh.id, rect=rect, **_kw(kw))
        want = color_ref.apply(content, rect=rect, dst_bits=None, **kw)
        assert np.all(want[0] == 0) and want[2:7, 3:14].any()
        assert np.array_equal(fresh.bits(), want)
        engine.color_filter(alone.id, rect=rect, **_kw(kw))
        assert np.array_equal(alone.bits(), color_ref.apply(zeros, rect=rect, dst_bits=None, **kw))


def test_rendered_scene_through_grayscale(engine):
    rec, _, _ = engine.render(*scene())
    plain = target_of(engine, rec)
    assert plain.any()
    kw = cf.grayscale(1.0)
    engine.color_filter(rec.target["id"], **kw)
    got = target_of(engine, rec)
    assert_equal_bits(got, color_ref.apply(plain, dst_bits=plain, **dict(kw, space=color_ref.SRGB)), "grayscale")
    inside = got[44, 50].view(np.float16)
    assert inside[0] == inside[1] == inside[2] and inside[3] == 1.0  # grey, opaque


def test_luminance_mask(engine):
    """Engine.luminance_mask on two rendered layers: the mask's luminance into the scratch's alpha, the layer kept where it is."""
    layer_scene, p = scene()
    mask_scene = Scene()
    mask_scene.fill(Fill.NonZero, None, Brush.solid((1.0, 1.0, 1.0, 1.0)), None, Path.circle(64, 64, 40))
    mask_scene.fill(Fill.NonZero, None, Brush.solid((0.2, 0.6, 0.1, 0.7)), None, Path.circle(40, 50, 25))
    mrec, _, _ = engine.render(mask_scene, p)
    mask_bits = target_of(engine, mrec)
    with images(engine, (128, 128), mask_bits) as (scratch, mask):
        rec, _, _ = engine.render(layer_scene, p)
        layer_bits = target_of(engine, rec)
        assert mask_bits.any() and layer_bits.any() and not np.array_equal(mask_bits, layer_bits)
        engine.luminance_mask(rec.target["id"], mask.id, scratch.id)
        got = target_of(engine, rec)
        lum = color_ref.apply(mask_bits, **dict(cf.luminance_to_alpha(), space=color_ref.LINEAR))
        assert np.array_equal(scratch.bits(), lum)
        assert_same_bits(got, composite_ref.composite(lum, layer_bits, compose=int(Compose.DestIn)), "luminance mask")
        assert got[44, 50, 3] != 0 and got[100, 120, 3] == 0  # kept under the mask's white disc, gone outside it


def test_captured_with_the_frame(engine):
    """capture(color=..., surface=...): render, filter the target in place, blit it -- two launches more than the frame alone (the
    filter and the blit: the tables are resident, nothing is uploaded), replayed twice, the bytes of the eager calls."""
    kw = cf.sepia(1.0)
    captured_with_the_frame(engine, scene(), lambda target, _: engine.color_filter(target, **kw), lambda _: dict(color=kw),
                            lambda plain: color_ref.apply(plain, dst_bits=plain, **dict(kw, space=color_ref.SRGB)), extra_launches=2,
                            same=assert_equal_bits)


def test_captures_and_the_resident_key():
    """On a fresh context: a call that needs no tables is capturable at once and takes no scratch; a capture whose key is not
    resident is refused with the advice and touches nothing; after one eager call it is recorded (and runs nothing); the same key
    again, with another matrix, uploads nothing and leaves the graph valid; another key makes it stale; jh_scratch_trim forgets
    the key."""
    engine = jello_amd.Engine(0)
    hip, ctx = engine.hip, engine.ctx
    bits = color_cases.geometry_source((37, 19), seed=8)
    poison = np.full((19, 37, 4), color_cases.POISON, np.uint16)
    gray, sepia, lum = cf.grayscale(1.0), cf.sepia(1.0), cf.luminance_to_alpha()
    ref = lambda kw, **more: color_ref.apply(bits, dst_bits=poison, **dict(kw, space=int(kw["space"]), **more))  # noqa: E731
    captured = lambda kw, **more: captured_call(  # noqa: E731
        engine, lambda: hip.jh_color_filter(ctx, src.id, dst.id, ctypes.byref(_color_desc(rect=None, **kw))), **more)
    slot = 17  # JH_SCR_COLOR_TABLES
    graphs = []
    try:
        with images(engine, bits, poison, 64) as (src, dst, buf):
            try:
                # no tables: capturable on a fresh context, and the slot stays empty
                rc, msg, g = captured(lum)
                graphs.append(g)
                assert rc == 0, msg
                assert np.array_equal(dst.bits(), poison)  # a capture runs nothing
                engine.replay(g)
                assert np.array_equal(dst.bits(), ref(lum))
                assert hip.jh_debug_scratch_bytes(ctx, slot) == 0
                engine.upload_image(dst.id, poison)
                # a key that is not resident
                rc, msg, refused = captured(gray, clear_first=buf.id)
                engine.graph_destroy(refused)
                assert rc == JH_ERR_OOM and msg.startswith("jh_color_filter: ") and "run this filter once eagerly first" in msg, (rc, msg)
                assert np.array_equal(dst.bits(), poison) and np.array_equal(src.bits(), bits)
                engine.color_filter(src.id, dst.id, **gray)
                assert np.array_equal(dst.bits(), ref(gray))
                assert hip.jh_debug_scratch_bytes(ctx, slot) >= 3 * 65536 * 4 + 4 * 65536 * 2
                engine.upload_image(dst.id, poison)
                rc, msg, g = captured(gray)
                graphs.append(g)
                assert rc == 0, msg
                assert np.array_equal(dst.bits(), poison)
                engine.replay(g)
                assert np.array_equal(dst.bits(), ref(gray))
                # the same key with another matrix (sepia differs from grayscale in the matrix alone), and a call without tables:
                # nothing is uploaded, the graph stays valid
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
                rc, msg, refused = captured(cf.invert(1.0))
                engine.graph_destroy(refused)
                assert rc == JH_ERR_OOM and "run this filter once eagerly first" in msg
                engine.color_filter(src.id, dst.id, **cf.invert(1.0))
                assert np.array_equal(dst.bits(), ref(cf.invert(1.0)))
            finally:
                for g in graphs:
                    engine.graph_destroy(g)
    finally:
        engine.close()


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_color_filter: ", no texel of either image and
    no byte of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    inf, nan = math.inf, math.nan

    def matrix_with(k, v):
        m = list(color_ref.IDENTITY)
        m[k] = v
        return m

    with images(engine, canary, canary, canary_bits(8, 6), (W, H, ImageFormat.RGBA8)) as (src, dst, small, rgba8):
        def call(s=None, d=None, null=False, rect=None, flags=None, **kw):
            args = dict(matrix=None, funcs=None, space=0, clamp=True)
            args.update(kw)
            desc = _color_desc(rect=rect, **args)
            if flags is not None:
                desc.flags = flags
            return hip.jh_color_filter(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

        outside_dst = (b"the destination rectangle is ", b"not inside the destination image")
        refused = dict(common_refusals(call, rgba8, rects=(("", "source ", "rect"),)), **{
            "rectangle outside the destination only": (lambda: call(d=small.id, rect=(4, 2, 6, 3)), outside_dst),
            "rectangle outside the source only": (lambda: call(s=small.id, rect=(4, 2, 6, 3)), (b"the source rectangle is ", b"not inside the source image")),
            "the whole source does not fit the destination": (lambda: call(d=small.id), outside_dst),
            "space 2": (lambda: call(space=2), b""),
            "space -1": (lambda: call(space=-1), b""),
            "flag bit 1": (lambda: call(flags=2), b""),
            "flag bit 31": (lambda: call(flags=0x80000001), b""),
            "func type 5": (lambda: call(funcs=(None, (5,), None, None)), b""),
            "func type -1": (lambda: call(funcs=(None, None, None, (-1,))), b""),
            "matrix entry NaN": (lambda: call(matrix=matrix_with(7, nan)), b""),
            "matrix offset Inf": (lambda: call(matrix=matrix_with(19, inf)), b""),
            "slope Inf": (lambda: call(funcs=(cf.linear(inf, 0.0), None, None, None)), b""),
            "exponent NaN": (lambda: call(funcs=(None, cf.gamma(1.0, nan, 0.0), None, None)), b""),
            "a table value -Inf": (lambda: call(funcs=(None, None, cf.table([0.0, -inf]), None)), b""),
            "table of 0": (lambda: call(funcs=(cf.table([]), None, None, None)), b""),
            "discrete of 65": (lambda: call(funcs=(None, None, None, cf.discrete([0.5] * 65))), b""),
        })
        check_refusals(engine, "jh_color_filter", call, refused, untouched=((src, canary), (dst, canary), (small, canary_bits(8, 6))),
                       raises=(lambda: engine.color_filter(src.id, dst.id, rect=(8, 0, 9, 4)),
                               lambda: engine.color_filter(src.id, funcs=(cf.table([]), None, None, None))),
                       accepted=(lambda: call(s=small.id), lambda: call(d=src.id)))  # (the whole of a smaller source fits, and so does the plain call in place)


def test_the_call_is_one_query_of_the_tree(engine):
    bits = color_cases.geometry_source((48, 33), seed=2)
    kw = cf.contrast(1.7)
    with images(engine, bits, (48, 33)) as (src, dst):
        one_query(engine, "color", lambda: engine.color_filter(src.id, dst.id, **kw))  # (a new key: the upload is inside the query)
        got = dst.bits()
    assert np.array_equal(got, color_ref.apply(bits, **dict(kw, space=color_ref.SRGB)))
