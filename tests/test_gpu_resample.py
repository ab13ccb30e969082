"""-m gpu: jh_resample against the rule of DESIGN.md 5.9 (tests/resample_ref.py) byte for byte -- the battery of
tests/resample_cases.py, a rendered frame, a captured frame -- and the call's frame: its tap tables and captures, its refusals, its
profile query."""
import ctypes

import numpy as np
import pytest

from jello_amd import ImageFormat, ResampleFilter
from jello_amd._lib import CResampleDesc
from jello_amd.engine import JH_ERR_INVALID

import resample_cases
import resample_ref
from devmem import target_of
from image_call import (JH_ERR_OOM, assert_same_bits, canary_bits, captured_call, captured_with_the_frame, check_refusals, common_refusals, images,
                        one_query, run_case, scene)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in resample_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.resample: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = resample_cases.BY_NAME[name]
    call = lambda src, dst: engine.resample(src.id, dst.id, ResampleFilter(c["filter"]), c["src_rect"], c["dst_rect"], premultiplied=not c["flags"])  # noqa: E731
    got = run_case(engine, c, call, resample_cases.source(c), resample_cases.before(c), dst_size=c["dst_size"])
    assert_same_bits(got, resample_cases.expected(name), name)


def test_a_never_written_source_gives_transparent_black(engine):
    """... inside the rectangle (under both flag settings: 0 / max(0, 1e-6) is 0), and leaves the rest of dst alone."""
    with images(engine, (40, 30), np.full((20, 25, 4), resample_cases.POISON, np.uint16)) as (src, dst):
        for premultiplied, rect in ((True, (1, 1, 11, 9)), (False, (13, 10, 12, 10))):
            engine.resample(src.id, dst.id, ResampleFilter.LANCZOS3, dst_rect=rect, premultiplied=premultiplied)
        got = dst.bits()
    want = np.full((20, 25, 4), resample_cases.POISON, np.uint16)
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("filt", list(ResampleFilter))
def test_rendered_scene(engine, filt):
    """A rendered 128 x 128 frame (a circle and a stroked curve, translucent edges) resized to 48 x 40 = the reference on the download
    of the same render."""
    rec, _, _ = engine.render(*scene())
    plain = target_of(engine, rec)
    assert plain.any()
    with images(engine, (48, 40)) as (dst,):
        engine.resample(rec.target["id"], dst.id, filt)
        got = dst.bits()
    assert_same_bits(got, resample_ref.resample(plain, (40, 48), int(filt)), filt.name)
    assert np.array_equal(target_of(engine, rec), plain)


def test_captured_with_the_frame(engine):
    """capture(resample=..., surface=...): render, resize into a second image, blit that image at its size -- three launches more
    than the frame alone (rows, columns, blit: the tables are resident, nothing is uploaded), replayed twice, the bytes of the eager
    calls."""
    filt = ResampleFilter.CATMULL_ROM
    captured_with_the_frame(engine, scene(), lambda target, dst: engine.resample(target, dst, filt),
                            lambda dst: dict(resample=dict(dst=dst, width=48, height=40, filter=filt)),
                            lambda plain: resample_ref.resample(plain, (40, 48), int(filt)), extra_launches=3, out_size=(48, 40))


def test_captures_and_the_resident_geometry(engine):
    """A capture whose geometry is not the resident one is refused with the advice and touches nothing; after one eager call it is
    recorded (and runs nothing); an eager call with another geometry then makes that graph stale."""
    hip, ctx = engine.hip, engine.ctx
    bits = resample_cases.content("unit", 60, 44, seed=1)
    poison = np.full((17, 23, 4), resample_cases.POISON, np.uint16)
    d = CResampleDesc(int(ResampleFilter.TRIANGLE), 0, 0, 0, 0, 0, 0, 0, 0, 0)
    enqueue = lambda: hip.jh_resample(ctx, src.id, dst.id, ctypes.byref(d))  # noqa: E731
    g = None
    with images(engine, bits, poison, (30, 22), 64) as (src, dst, other, buf):
        try:
            engine.resample(src.id, other.id, ResampleFilter.TRIANGLE)  # (another geometry is resident)
            rc, msg, refused = captured_call(engine, enqueue, clear_first=buf.id)
            engine.graph_destroy(refused)
            assert rc == JH_ERR_OOM and msg.startswith("jh_resample: ") and "resample this geometry once eagerly first" in msg, (rc, msg)
            assert np.array_equal(dst.bits(), poison) and np.array_equal(src.bits(), bits)
            engine.resample(src.id, dst.id, ResampleFilter.TRIANGLE)
            want = resample_ref.resample(bits, (17, 23), resample_ref.TRIANGLE)
            assert resample_ref.same_bits(dst.bits(), want)
            engine.upload_image(dst.id, poison)
            rc, msg, g = captured_call(engine, enqueue)
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


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_resample: ", no texel of either image and no
    byte of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    # 40 x 2 and 2 x 40: 34 texels onto 2 are 17:1
    with images(engine, canary, canary, canary_bits(40, 2), canary_bits(2, 40), (W, H, ImageFormat.RGBA8)) as (src, dst, wide, tall, rgba8):
        def call(s=None, d=None, filt=2, flags=0, src_rect=(0, 0, 0, 0), dst_rect=(0, 0, 0, 0), null=False):
            return hip.jh_resample(ctx, src.id if s is None else s, dst.id if d is None else d,
                                   None if null else ctypes.byref(CResampleDesc(filt, flags, *src_rect, *dst_rect)))

        refused = dict(common_refusals(call, rgba8, rects=(("source ", "source ", "src_rect"), ("destination ", "destination ", "dst_rect"))), **{
            "filter 4": (lambda: call(filt=4), b""),
            "filter -1": (lambda: call(filt=-1), b""),
            "flag bit 1": (lambda: call(flags=2), b""),
            "flag bit 31": (lambda: call(flags=0x80000001), b""),
            "17:1 on x": (lambda: call(s=wide.id, src_rect=(0, 0, 34, 2), dst_rect=(0, 0, 2, 2)), b""),
            "17:1 on y": (lambda: call(s=tall.id, src_rect=(0, 0, 2, 34), dst_rect=(0, 0, 2, 2)), b""),
            "source is the destination": (lambda: call(d=src.id), b""),
        })
        check_refusals(engine, "jh_resample", call, refused, untouched=((src, canary), (dst, canary)),
                       raises=(lambda: engine.resample(src.id, src.id),
                               lambda: engine.resample(wide.id, dst.id, src_rect=(0, 0, 34, 2), dst_rect=(0, 0, 2, 2))),
                       accepted=(lambda: call(s=wide.id, src_rect=(0, 0, 32, 2), dst_rect=(0, 0, 2, 2)), call))  # (16:1 is accepted, and so is the plain call)


def test_the_call_is_one_query_of_the_tree(engine):
    bits = resample_cases.content("unit", 48, 33, seed=2)
    with images(engine, bits, (20, 40)) as (src, dst):
        one_query(engine, "resample", lambda: engine.resample(src.id, dst.id, ResampleFilter.LANCZOS3))  # (a new geometry: the upload is inside the query)
        got = dst.bits()
    assert resample_ref.same_bits(got, resample_ref.resample(bits, (40, 20), resample_ref.LANCZOS3))
