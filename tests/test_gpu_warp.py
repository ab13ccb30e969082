"""-m gpu: jh_warp against the rule of DESIGN.md 5.12 (tests/warp_ref.py) byte for byte -- the battery of tests/warp_cases.py, a warp
in quadrants, a rendered frame, Engine.place_layer, a captured frame -- and the call's frame: its refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import ImageFormat, ResampleFilter, WarpEdge, WarpFilter
from jello_amd._lib import CWarpDesc

import composite_ref
import warp_cases
import warp_ref
from devmem import target_of
from image_call import (assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query,
                        run_case, scene)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in warp_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.warp: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle with
    the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = warp_cases.BY_NAME[name]
    call = lambda src, dst: engine.warp(src.id, dst.id, c["matrix"], WarpFilter(c["filter"]), WarpEdge(c["edge"]), c["src_rect"], c["dst_rect"],  # noqa: E731
                                        premultiplied=not c["flags"])
    got = run_case(engine, c, call, warp_cases.source(c), warp_cases.before(c), dst_size=c["dst_size"])
    assert_same_bits(got, warp_cases.expected(name), name)


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_four_quadrants_are_the_whole_image(engine, filt):
    bits = warp_cases.content("unit", 45, 37, seed=3)
    m = warp_cases.rotate(30, (45, 37), (51, 35), 1.2)
    with images(engine, bits, (51, 35), (51, 35)) as (src, whole, parts):
        engine.warp(src.id, whole.id, m, filt, WarpEdge.MIRROR)
        for rect in ((0, 0, 25, 17), (25, 0, 26, 17), (0, 17, 25, 18), (25, 17, 26, 18)):
            engine.warp(src.id, parts.id, m, filt, WarpEdge.MIRROR, dst_rect=rect)
        a, b = whole.bits(), parts.bits()
    assert np.array_equal(a, b)
    assert warp_ref.same_bits(a, warp_ref.warp(bits, (35, 51), m, int(filt), warp_ref.MIRROR))


def test_a_never_written_source_and_a_never_written_destination(engine):
    """A never-written source gives transparent black inside the rectangle under every edge mode and leaves the rest of dst alone; a
    never-written destination is cleared around the rectangle."""
    bits = warp_cases.content("unit", 9, 7, seed=4)
    m = warp_cases.rotate(45, (40, 30), (25, 20))
    with images(engine, (40, 30), np.full((20, 25, 4), warp_cases.POISON, np.uint16), bits, (25, 20)) as (src, dst, real, fresh):
        for edge, premultiplied, rect in ((WarpEdge.REPEAT, True, (1, 1, 11, 9)), (WarpEdge.CLAMP, False, (13, 10, 12, 10))):
            engine.warp(src.id, dst.id, m, WarpFilter.BICUBIC, edge, dst_rect=rect, premultiplied=premultiplied)
        got = dst.bits()
        engine.warp(real.id, fresh.id, warp_cases.translate(3, 2), WarpFilter.BILINEAR, WarpEdge.CLAMP, dst_rect=(5, 3, 7, 9))
        cleared = fresh.bits()
    want = np.full((20, 25, 4), warp_cases.POISON, np.uint16)
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    assert np.array_equal(got, want)
    assert warp_ref.same_bits(cleared, warp_ref.warp(bits, (20, 25), warp_cases.translate(3, 2), warp_ref.BILINEAR, warp_ref.CLAMP, dst_rect=(5, 3, 7, 9)))


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_rendered_scene(engine, filt):
    """A rendered 128 x 128 frame (a circle and a stroked curve, translucent edges) rotated by 30 degrees into 96 x 80 = the
    reference on the download of the same render."""
    rec, _, _ = engine.render(*scene())
    plain = target_of(engine, rec)
    assert plain.any()
    m = warp_cases.rotate(30, (128, 128), (96, 80), 0.7)
    with images(engine, (96, 80)) as (dst,):
        engine.warp(rec.target["id"], dst.id, m, filt)
        got = dst.bits()
    assert_same_bits(got, warp_ref.warp(plain, (80, 96), m, int(filt)), filt.name)
    assert np.array_equal(target_of(engine, rec), plain)


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_place_layer(engine, filt):
    """Engine.place_layer = warp_ref.warp into the scratch's bounds rectangle, then composite_ref.composite of that rectangle."""
    layer_bits = warp_cases.content("alpha01", 29, 21, seed=6)
    target_bits = warp_cases.content("unit", 61, 47, seed=7)
    target_bits[..., 3] = 0x3C00
    m = warp_cases.rotate(30, (29, 21), (61, 47), 0.9)
    with images(engine, layer_bits, target_bits, (61, 47)) as (layer, target, scratch):
        rect = engine.place_layer(layer.id, target.id, m, scratch.id, (29, 21), (61, 47), filter=filt, opacity=0.75)
        got, got_scratch = target.bits(), scratch.bits()
        gone = engine.place_layer(layer.id, target.id, warp_cases.translate(500, 0), scratch.id, (29, 21), (61, 47), filter=filt)
        assert gone == (0, 0, 0, 0) and np.array_equal(target.bits(), got)
    assert rect == warp_ref.bounds(m, (29, 21), int(filt), (61, 47)) and 0 < rect[2] < 61 and 0 < rect[3] < 47
    warped = warp_ref.warp(layer_bits, (47, 61), m, int(filt), warp_ref.ZERO, dst_rect=rect)
    assert warp_ref.same_bits(got_scratch, warped)
    assert warp_ref.same_bits(warped, warp_ref.warp(layer_bits, (47, 61), m, int(filt), warp_ref.ZERO))  # outside the bounds: transparent black
    want = composite_ref.composite(warped, target_bits, opacity=0.75, src_rect=rect, offset=(rect[0], rect[1]))
    assert_same_bits(got, want, filt.name)


def test_captured_with_the_frame(engine):
    """capture(warp=..., surface=...): render, rotate into a second image, blit that image at its size -- one launch more than with
    the blit alone (no scratch, no tables), replayed twice, the bytes of the eager calls; resample= together with warp= is refused
    before anything is captured."""
    filt = WarpFilter.BICUBIC
    m = warp_cases.rotate(30, (128, 128), (48, 40), 0.4)
    with images(engine, (48, 40)) as (small,):
        with pytest.raises(ValueError, match="exclusive"):
            engine.capture(jello_amd.Host().record(*scene()), resample=dict(dst=small.id, width=48, height=40, filter=ResampleFilter.BOX),
                           warp=dict(dst=small.id, width=48, height=40, matrix=m))
    captured_with_the_frame(engine, scene(), lambda target, dst: engine.warp(target, dst, m, filt, WarpEdge.CLAMP),
                            lambda dst: dict(warp=dict(dst=dst, width=48, height=40, matrix=m, filter=filt, edge=WarpEdge.CLAMP)),
                            lambda plain: warp_ref.warp(plain, (40, 48), m, int(filt), warp_ref.CLAMP), extra_launches=1, out_size=(48, 40),
                            baseline_surface=True)


IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_warp: ", no texel of either image and no byte
    of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    with images(engine, canary, canary, (W, H, ImageFormat.RGBA8), (32769, 1)) as (src, dst, rgba8, long_):
        def call(s=None, d=None, m=IDENT, head=(1, 0, 0), src_rect=(0, 0, 0, 0), dst_rect=(0, 0, 0, 0), null=False):
            desc = CWarpDesc((ctypes.c_double * 6)(*m), *head, *src_rect, *dst_rect)
            return hip.jh_warp(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, rects=(("source ", "source ", "src_rect"), ("destination ", "destination ", "dst_rect"))), **{
            "filter 3": (lambda: call(head=(3, 0, 0)), b"filter"),
            "filter -1": (lambda: call(head=(-1, 0, 0)), b"filter"),
            "edge 4": (lambda: call(head=(1, 4, 0)), b"edge"),
            "edge -1": (lambda: call(head=(1, -1, 0)), b"edge"),
            "flag bit 1": (lambda: call(head=(1, 0, 2)), b"flag"),
            "flag bit 31": (lambda: call(head=(1, 0, 0x80000001)), b"flag"),
            "a NaN entry": (lambda: call(m=(1.0, math.nan, 0.0, 1.0, 0.0, 0.0)), b"not finite"),
            "an infinite entry": (lambda: call(m=(1.0, 0.0, 0.0, 1.0, 0.0, math.inf)), b"not finite"),
            "determinant 0": (lambda: call(m=(1.0, 2.0, 2.0, 4.0, 0.0, 0.0)), b"determinant is 0"),
            "determinant overflows": (lambda: call(m=(1e200, 0.0, 0.0, 1e200, 0.0, 0.0)), b"determinant is not finite"),
            "65:1": (lambda: call(m=(1.0 / 65.0, 0.0, 0.0, 1.0, 0.0, 0.0)), b"above 64"),
            "offset beyond 2^22": (lambda: call(m=(1.0, 0.0, 0.0, 1.0, 5e6, 0.0)), b"above 2^22"),
            "a side above 32768": (lambda: call(s=long_.id), b"32768"),
            "source is the destination": (lambda: call(d=src.id), b"source is the destination"),
        })
        check_refusals(engine, "jh_warp", call, refused, untouched=((src, canary), (dst, canary)),
                       raises=(lambda: engine.warp(src.id, src.id, IDENT), lambda: engine.warp(src.id, dst.id, (0.0,) * 6),
                               lambda: engine.warp(src.id, dst.id, IDENT[:5])),
                       accepted=(lambda: call(m=(1.0 / 64.0, 0.0, 0.0, 1.0 / 64.0, 0.0, 0.0)), call))  # (64:1 is accepted, and so is the plain call)


def test_the_call_is_one_query_of_the_tree(engine):
    bits = warp_cases.content("unit", 48, 33, seed=2)
    m = warp_cases.rotate(45, (48, 33), (20, 40))
    with images(engine, bits, (20, 40)) as (src, dst):
        one_query(engine, "warp", lambda: engine.warp(src.id, dst.id, m, WarpFilter.BICUBIC, WarpEdge.MIRROR))
        got = dst.bits()
    assert warp_ref.same_bits(got, warp_ref.warp(bits, (40, 20), m, warp_ref.BICUBIC, warp_ref.MIRROR))
