"""-m gpu: jh_perspective against the rule of DESIGN.md 5.19 (tests/perspective_ref.py) byte for byte -- the battery of
tests/perspective_cases.py (every instantiation of the kernel), the call against jh_warp on the device where the rule says they
agree, a call in quadrants, never-written images, Engine.project_layer against the composed references, a captured frame -- and the
call's frame: its refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import ImageFormat, ResampleFilter, WarpEdge, WarpFilter
from jello_amd import perspective as persp
from jello_amd._lib import CPerspectiveDesc

import composite_ref
import perspective_cases
import perspective_ref
import warp_cases
from image_call import (assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query,
                        run_case, scene)

pytestmark = pytest.mark.gpu

IDENT = perspective_ref.IDENTITY
KEYSTONE = perspective_cases.KEYSTONE


def _call(engine, c):
    return lambda src, dst: engine.perspective(src.id, dst.id, c["matrix"], WarpFilter(c["filter"]), WarpEdge(c["edge"]), c["src_rect"], c["dst_rect"],
                                               premultiplied=not c["flags"])


INSTANTIATIONS = sorted({c["inst"] for c in perspective_cases.CASES})


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: "%s_%s_%s" % (WarpFilter(i[0]).name, WarpEdge(i[1]).name, "straight" if i[2] else "premul"))
def test_battery(engine, inst):
    """Every case of one instantiation of jh_perspective's kernel through Engine.perspective: dst is poisoned first (or never written), the
    whole of dst is compared -- the rectangle with the reference, the texels outside it with what they held (a never-written dst:
    transparent black).  A failure names the case."""
    names = [c["name"] for c in perspective_cases.CASES if c["inst"] == inst]
    assert names
    for name in names:
        c = perspective_cases.BY_NAME[name]
        got = run_case(engine, c, _call(engine, c), perspective_cases.source(c), perspective_cases.before(c), dst_size=c["dst_size"])
        assert_same_bits(got, perspective_cases.expected(name), name)


def test_the_battery_runs_every_instantiation():
    assert len(INSTANTIATIONS) == 24 and sum(len([c for c in perspective_cases.CASES if c["inst"] == i]) for i in INSTANTIATIONS) == len(perspective_cases.CASES)


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_a_dyadic_affine_matrix_is_the_warp_on_the_device(engine, filt):
    """The affine cases whose inverse is dyadic (the identity, integer and half-texel translations, the flips and quarter turns, a
    scale by 2), every one of this filter: the bits of Engine.warp, on the device."""
    names = [n for n in perspective_cases.AFFINE if perspective_cases.BY_NAME[n]["filter"] == int(filt)]
    assert len(names) >= 20
    for name in names:
        c = perspective_cases.BY_NAME[name]
        src_bits, prior = perspective_cases.source(c), perspective_cases.before(c)
        with images(engine, src_bits, prior, prior) as (src, projected, warped):
            _call(engine, c)(src, projected)
            engine.warp(src.id, warped.id, c["affine"], WarpFilter(c["filter"]), WarpEdge(c["edge"]), c["src_rect"], c["dst_rect"], premultiplied=not c["flags"])
            a, b = projected.bits(), warped.bits()
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_four_quadrants_are_the_whole_image(engine, filt):
    bits = warp_cases.content("unit", 45, 37, seed=3)
    with images(engine, bits, (51, 35), (51, 35)) as (src, whole, parts):
        engine.perspective(src.id, whole.id, KEYSTONE, filt, WarpEdge.MIRROR)
        for rect in ((0, 0, 25, 17), (25, 0, 26, 17), (0, 17, 25, 18), (25, 17, 26, 18)):
            engine.perspective(src.id, parts.id, KEYSTONE, filt, WarpEdge.MIRROR, dst_rect=rect)
        a, b = whole.bits(), parts.bits()
    assert np.array_equal(a, b)
    assert perspective_ref.same_bits(a, perspective_ref.perspective(bits, (35, 51), KEYSTONE, int(filt), perspective_ref.MIRROR))


def test_a_never_written_source_and_a_never_written_destination(engine):
    """A never-written source gives transparent black inside the rectangle under every edge mode and leaves the rest of dst alone; a
    never-written destination is cleared around the rectangle."""
    bits = warp_cases.content("unit", 9, 7, seed=4)
    with images(engine, (40, 30), np.full((20, 25, 4), warp_cases.POISON, np.uint16), bits, (25, 20)) as (src, dst, real, fresh):
        for edge, premultiplied, rect in ((WarpEdge.REPEAT, True, (1, 1, 11, 9)), (WarpEdge.CLAMP, False, (13, 10, 12, 10))):
            engine.perspective(src.id, dst.id, KEYSTONE, WarpFilter.BICUBIC, edge, dst_rect=rect, premultiplied=premultiplied)
        got = dst.bits()
        engine.perspective(real.id, fresh.id, KEYSTONE, WarpFilter.BILINEAR, WarpEdge.CLAMP, dst_rect=(5, 3, 7, 9))
        cleared = fresh.bits()
    want = np.full((20, 25, 4), warp_cases.POISON, np.uint16)
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    assert np.array_equal(got, want)
    ref = perspective_ref.perspective(bits, (20, 25), KEYSTONE, perspective_ref.BILINEAR, perspective_ref.CLAMP, dst_rect=(5, 3, 7, 9))
    assert perspective_ref.same_bits(cleared, ref) and ref[3:12, 5:12].any() and not ref[:3].any()


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_project_layer(engine, filt):
    """Engine.project_layer = perspective_ref.perspective into the scratch's bounds rectangle, then composite_ref.composite of that
    rectangle; a matrix that takes the layer behind the viewer writes the whole target's rectangle."""
    layer_bits = warp_cases.content("alpha01", 29, 21, seed=6)
    target_bits = warp_cases.content("unit", 61, 47, seed=7)
    target_bits[..., 3] = 0x3C00
    m = persp.rotate_y(math.radians(35), 90.0, (14.5, 10.5))["matrix"]
    m = persp.compose(persp.affine(warp_cases.translate(12, 9)), m)["matrix"]
    with images(engine, layer_bits, target_bits, (61, 47)) as (layer, target, scratch):
        rect = engine.project_layer(layer.id, target.id, m, scratch.id, (29, 21), (61, 47), filter=filt, opacity=0.75)
        got, got_scratch = target.bits(), scratch.bits()
        gone = engine.project_layer(layer.id, target.id, persp.compose(persp.affine(warp_cases.translate(500, 0)), m)["matrix"], scratch.id, (29, 21),
                                    (61, 47), filter=filt)
        assert gone == (0, 0, 0, 0) and np.array_equal(target.bits(), got)
    assert rect == perspective_ref.bounds(m, (29, 21), int(filt), (61, 47)) and 0 < rect[2] < 61 and 0 < rect[3] < 47
    projected = perspective_ref.perspective(layer_bits, (47, 61), m, int(filt), perspective_ref.ZERO, dst_rect=rect)
    assert perspective_ref.same_bits(got_scratch, projected)
    assert perspective_ref.same_bits(projected, perspective_ref.perspective(layer_bits, (47, 61), m, int(filt), perspective_ref.ZERO))  # outside the bounds: transparent black
    want = composite_ref.composite(projected, target_bits, opacity=0.75, src_rect=rect, offset=(rect[0], rect[1]))
    assert_same_bits(got, want, filt.name)


def test_captured_with_the_frame(engine):
    """capture(perspective=..., surface=...): render, project into a second image, blit that image at its size -- one launch more than
    with the blit alone (no scratch, no tables), replayed twice, the bytes of the eager calls; perspective= together with resample= or
    warp= is refused before anything is captured."""
    filt = WarpFilter.BICUBIC
    m = persp.compose(persp.affine(warp_cases.rotate(30, (128, 128), (48, 40), 0.4)), persp.rotate_x(math.radians(25), 300.0, (64, 64)))["matrix"]
    with images(engine, (48, 40)) as (small,):
        rec = jello_amd.Host().record(*scene())
        d = dict(dst=small.id, width=48, height=40, matrix=m)
        with pytest.raises(ValueError, match="exclusive"):
            engine.capture(rec, resample=dict(dst=small.id, width=48, height=40, filter=ResampleFilter.BOX), perspective=d)
        with pytest.raises(ValueError, match="exclusive"):
            engine.capture(rec, warp=dict(dst=small.id, width=48, height=40, matrix=warp_cases.translate(0, 0)), perspective=d)
    captured_with_the_frame(engine, scene(), lambda target, dst: engine.perspective(target, dst, m, filt, WarpEdge.CLAMP),
                            lambda dst: dict(perspective=dict(dst=dst, width=48, height=40, matrix=m, filter=filt, edge=WarpEdge.CLAMP)),
                            lambda plain: perspective_ref.perspective(plain, (40, 48), m, int(filt), perspective_ref.CLAMP), extra_launches=1,
                            out_size=(48, 40), baseline_surface=True)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_perspective: ", no texel of either image and no
    byte of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    nan, inf = math.nan, math.inf
    with images(engine, canary, canary, (W, H, ImageFormat.RGBA8), (32769, 1)) as (src, dst, rgba8, long_):
        def call(s=None, d=None, m=IDENT, head=(1, 0, 0), src_rect=(0, 0, 0, 0), dst_rect=(0, 0, 0, 0), null=False):
            desc = CPerspectiveDesc((ctypes.c_double * 9)(*m), *head, *src_rect, *dst_rect)
            return hip.jh_perspective(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, rects=(("source ", "source ", "src_rect"), ("destination ", "destination ", "dst_rect"))), **{
            "filter 3": (lambda: call(head=(3, 0, 0)), b"filter"),
            "filter -1": (lambda: call(head=(-1, 0, 0)), b"filter"),
            "edge 4": (lambda: call(head=(1, 4, 0)), b"edge"),
            "edge -1": (lambda: call(head=(1, -1, 0)), b"edge"),
            "flag bit 1": (lambda: call(head=(1, 0, 2)), b"flag"),
            "flag bit 31": (lambda: call(head=(1, 0, 0x80000001)), b"flag"),
            "a NaN entry": (lambda: call(m=(1.0, nan, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)), b"matrix entry is not finite"),
            "an infinite entry": (lambda: call(m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, inf)), b"matrix entry is not finite"),
            "determinant 0": (lambda: call(m=(1.0, 2.0, 0.0, 2.0, 4.0, 0.0, 0.0, 0.0, 1.0)), b"determinant is 0"),
            "a row of zeros": (lambda: call(m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)), b"determinant is 0"),
            "an adjugate entry overflows": (lambda: call(m=(1e200, 0.0, 0.0, 0.0, 1e200, 0.0, 0.0, 0.0, 1.0)), b"adjugate entry is not finite"),
            "determinant overflows": (lambda: call(m=(1e120, 0.0, 0.0, 0.0, 1e120, 0.0, 0.0, 0.0, 1e120)), b"determinant is not finite"),
            "a side above 32768": (lambda: call(s=long_.id), b"32768"),
            "source is the destination": (lambda: call(d=src.id), b"source is the destination"),
        })
        check_refusals(engine, "jh_perspective", call, refused, untouched=((src, canary), (dst, canary)),
                       raises=(lambda: engine.perspective(src.id, src.id, IDENT), lambda: engine.perspective(src.id, dst.id, (0.0,) * 9),
                               lambda: engine.perspective(src.id, dst.id, IDENT[:6])),
                       accepted=(lambda: call(m=(1e-150, 0.0, 0.0, 0.0, 1e-150, 0.0, 0.0, 0.0, 1.0)), call))  # (no limit on the scale; the plain call)


def test_the_call_is_one_query_of_the_tree(engine):
    bits = warp_cases.content("unit", 48, 33, seed=2)
    with images(engine, bits, (20, 40)) as (src, dst):
        one_query(engine, "perspective", lambda: engine.perspective(src.id, dst.id, KEYSTONE, WarpFilter.BICUBIC, WarpEdge.MIRROR))
        got = dst.bits()
    assert perspective_ref.same_bits(got, perspective_ref.perspective(bits, (40, 20), KEYSTONE, perspective_ref.BICUBIC, perspective_ref.MIRROR))
