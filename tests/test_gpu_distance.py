"""-m gpu: jh_distance against the rule of DESIGN.md 5.20 (tests/distance_ref.py) byte for byte -- the battery of
tests/distance_cases.py, never-written images, quadrants, a captured frame, jh_morphology on images one texel high or wide,
Engine.round_outline and Engine.glow -- and the call's frame: its refusals, its captures, its profile query."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import Compose, DistanceEdge, DistanceWhich, ImageFormat, MorphEdge, MorphOp
from jello_amd import distance as ramps
from jello_amd._lib import CDistanceDesc

import composite_cases
import composite_ref
import distance_cases
import distance_ref
from devmem import target_of
from image_call import (JH_ERR_OOM, assert_same_bits, canary_bits, captured_call, captured_with_the_frame, check_refusals, common_refusals, images,
                        one_query, run_case, scene)

pytestmark = pytest.mark.gpu

DISTANCE_LAUNCHES = 2  # columns, rows + store (include/jello_hip.h)
ONE = 0x3C00


def _call(engine, src_id, dst_id, c, rect="case"):
    engine.distance(src_id, dst_id, channel=c["channel"], threshold=c["threshold"], which=DistanceWhich(c["which"]), edge=DistanceEdge(c["edge"]),
                    max_distance=c["R"], scale=c["scale"], offset=c["offset"], color=c["color"], rect=c["rect"] if rect == "case" else rect,
                    straight=bool(c["flags"]))


INSTANTIATIONS = sorted({c["inst"] for c in distance_cases.CASES})


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: i.replace("k_dist_rows<", "straight_").replace(", ", "_signed_").replace(">", ""))
def test_battery(engine, inst):
    """Every case of one instantiation of k_dist_rows through Engine.distance: dst is poisoned first (or is the source), the whole of
    dst is compared -- the rectangle with the reference, the texels outside it with what they held -- and the source of a call into a
    second image is only read.  A failure names the case."""
    names = [c["name"] for c in distance_cases.CASES if c["inst"] == inst]
    assert names
    for name in names:
        c = distance_cases.BY_NAME[name]
        src_bits = distance_cases.source(c)
        got = run_case(engine, c, lambda src, dst: _call(engine, src.id, None if c["in_place"] else dst.id, c), src_bits,
                       np.full_like(src_bits, distance_cases.POISON), in_place=c["in_place"])
        assert_same_bits(got, distance_cases.expected(name), "%s (%s)" % (name, inst))


def test_the_battery_runs_every_instantiation():
    assert len(INSTANTIATIONS) == 4 and sum(len([c for c in distance_cases.CASES if c["inst"] == i]) for i in INSTANTIATIONS) == len(distance_cases.CASES)


def _mask(w, h, at):
    """(h, w, 4) uint16: a 0 / 1 mask of a line, 1 at the positions `at`, the same in all four channels."""
    m = np.zeros(w * h, bool)
    m[list(at)] = True
    return np.repeat(np.where(m.reshape(h, w), ONE, 0).astype(np.uint16)[..., None], 4, axis=-1)


def test_a_never_written_destination_is_cleared_outside_the_rectangle(engine):
    bits = distance_cases.content("blob", None, 33, 21, 3, seed=3)
    rect = (5, 4, 20, 9)
    kw = dict(which=distance_ref.SIGNED, edge=distance_ref.CLAMP, R=3, scale=0.125, offset=0.5, color=(0.5, 0.25, 0.125, 1.0))
    with images(engine, bits, (33, 21)) as (src, dst):
        engine.distance(src.id, dst.id, which=DistanceWhich.SIGNED, edge=DistanceEdge.CLAMP, max_distance=3, scale=0.125, offset=0.5,
                        color=(0.5, 0.25, 0.125, 1.0), rect=rect)
        got = dst.bits()
    want = distance_ref.distance(bits, rect=rect, dst_bits=None, **kw)
    assert_same_bits(got, want, "a never-written destination")
    assert want[4:13, 5:25].any() and not want[:4].any()


def test_a_never_written_source_reads_as_transparent_black(engine):
    """No texel is a seed under threshold 0.5, every texel is one under threshold 0."""
    with images(engine, (33, 21), np.full((21, 33, 4), distance_cases.POISON, np.uint16)) as (src, dst):
        engine.distance(src.id, dst.id, max_distance=3, scale=0.25, straight=True)  # OUTER: s = 4 everywhere
        far = dst.bits()
        engine.distance(src.id, dst.id, threshold=0.0, max_distance=3, scale=0.25, straight=True)  # s = 0 everywhere
        near = dst.bits()
    assert np.all(far == ONE) and not near.any()


def test_four_quadrant_calls_equal_one(engine):
    bits = distance_cases.content("blob", None, 67, 41, 3, seed=7)
    kw = dict(which=DistanceWhich.SIGNED, max_distance=9, scale=0.05, offset=0.5, color=(0.25, 0.5, 0.75, 1.0))
    with images(engine, bits, (67, 41), (67, 41)) as (src, whole, parts):
        engine.distance(src.id, whole.id, **kw)
        for rect in ((0, 0, 31, 19), (31, 0, 36, 19), (0, 19, 31, 22), (31, 19, 36, 22)):
            engine.distance(src.id, parts.id, rect=rect, **kw)
        a, b = whole.bits(), parts.bits()
    assert np.array_equal(a, b) and len(np.unique(a[..., 3])) > 4


def test_on_a_line_the_disc_is_the_box_of_morphology(engine):
    """On an image one texel high or wide, at R = 1, 4 and 17: OUTER with the step ramp (scale -1, offset R + 1) on a 0 / 1 mask = the
    STRAIGHT DILATE of the mask by R; INNER with the step ramp (scale 1, offset -R) = the STRAIGHT ERODE, under ZERO (where both eat
    everything: the rows or columns next to the line are outside the image) and under CLAMP.  Device against device, bit for bit."""
    one = (1.0, 1.0, 1.0, 1.0)
    for (w, h) in ((97, 1), (1, 97)):
        mask = _mask(w, h, (10, 11, 60, 96))  # (at R = 17 the dilate leaves 28 .. 42 and 78, the erode of the inverse keeps them)
        inverse = mask ^ ONE  # (few non-seeds, so that an erode leaves something)
        with images(engine, mask, inverse, (w, h), (w, h)) as (src, inv, a, b):
            for R in (1, 4, 17):
                what = (w, h, R)
                engine.distance(src.id, a.id, which=DistanceWhich.OUTER, max_distance=R, scale=-1.0, offset=R + 1.0, color=one, straight=True)
                engine.morphology(src.id, b.id, op=MorphOp.DILATE, radius=R, edge=MorphEdge.ZERO, premultiplied=False)
                assert np.array_equal(a.bits(), b.bits()) and a.bits().any() and not a.bits().all(), what
                for edge, medge in ((DistanceEdge.ZERO, MorphEdge.ZERO), (DistanceEdge.CLAMP, MorphEdge.CLAMP)):
                    engine.distance(inv.id, a.id, which=DistanceWhich.INNER, edge=edge, max_distance=R, scale=1.0, offset=-float(R), color=one, straight=True)
                    engine.morphology(inv.id, b.id, op=MorphOp.ERODE, radius=R, edge=medge, premultiplied=False)
                    assert np.array_equal(a.bits(), b.bits()), (what, edge)
                    assert a.bits().any() == (edge == DistanceEdge.CLAMP), (what, edge)


def test_round_outline_and_glow_of_a_rendered_frame(engine):
    """Engine.round_outline onto an 80 x 60 target = distance_ref (OUTER, the outline ramp, the colour premultiplied), composite_ref of
    the halo, composite_ref of the layer; Engine.glow = distance_ref with the glow ramp, composite_ref with Plus (inner: SrcAtop)."""
    rec, _, _ = engine.render(*scene((64, 48), 3))
    layer = target_of(engine, rec)
    backdrop = composite_cases.unit(80, 60, seed=5)
    color = (0.0, 0.6, 0.2, 0.9)
    pre = tuple(c * color[3] for c in color[:3]) + (color[3],)

    def ref(ramp):
        return distance_ref.distance(layer, which=int(ramp["which"]), R=ramp["max_distance"], scale=ramp["scale"], offset=ramp["offset"], color=pre)

    with images(engine, backdrop, (64, 48)) as (target, scratch):
        engine.round_outline(rec.target["id"], target.id, 2.5, color, scratch.id)
        got, halo = target.bits(), scratch.bits()
        assert np.array_equal(target_of(engine, rec), layer)
    want_halo = ref(ramps.outline(2.5))
    assert_same_bits(halo, want_halo, "the halo")
    want = composite_ref.composite(layer, composite_ref.composite(want_halo, backdrop))
    assert_same_bits(got, want, "the round outline")
    assert (want != composite_ref.composite(layer, backdrop)).any()  # (the outline shows)
    for inner in (False, True):
        with images(engine, backdrop, (64, 48)) as (target, scratch):
            engine.glow(rec.target["id"], target.id, 5.5, color, scratch.id, inner=inner)
            got, field = target.bits(), scratch.bits()
        want_field = ref(ramps.glow(5.5, inner))
        assert_same_bits(field, want_field, "the glow's field")
        want = composite_ref.composite(want_field, backdrop, compose=int(Compose.SrcAtop if inner else Compose.Plus))
        assert_same_bits(got, want, "the glow, inner=%s" % inner)
        assert (want != backdrop).any()


def test_captured_with_the_frame(engine):
    """capture(distance=..., surface=...): render, the distance field in place, blit -- replayed twice, the bytes of the eager calls,
    and DISTANCE_LAUNCHES + 1 more kernel nodes than the plain capture."""
    what = dict(which=DistanceWhich.SIGNED, edge=DistanceEdge.CLAMP, max_distance=6, scale=1.0 / 12, offset=0.5, color=(0.5, 0.25, 0.75, 1.0), rect=(8, 4, 50, 40))
    captured_with_the_frame(engine, scene((64, 48), 3), lambda target, _: engine.distance(target, **what), lambda _: dict(distance=what),
                            lambda plain: distance_ref.distance(plain, which=distance_ref.SIGNED, edge=distance_ref.CLAMP, R=6, scale=1.0 / 12, offset=0.5,
                                                                color=what["color"], rect=what["rect"], dst_bits=plain),
                            extra_launches=DISTANCE_LAUNCHES + 1)


def test_capture_without_scratch_is_refused_with_advice(engine):
    """A capture that would grow the planes' slot: JH_ERR_OOM and the advice, nothing touched; after one eager call of the plan's size
    the same capture is accepted, and one that needs less as well."""
    hip, ctx = engine.hip, engine.ctx
    bits = distance_cases.content("blob", None, 64, 48, 3, seed=1)
    d = CDistanceDesc(3, 0.5, 0, 0, 5, -1.0, 6.0)
    d.color[:] = (1.0, 1.0, 1.0, 1.0)
    d.flags = 1
    small = CDistanceDesc(3, 0.5, 0, 0, 2, -1.0, 3.0)
    small.color[:] = (1.0, 1.0, 1.0, 1.0)
    small.flags = 1
    ref = lambda b, R: distance_ref.distance(b, R=R, scale=-1.0, offset=R + 1.0, flags=distance_ref.STRAIGHT)  # noqa: E731
    assert jello_amd.distance_plan((64, 48), max_distance=5)["scratch_bytes"] > jello_amd.distance_plan((64, 48), max_distance=2)["scratch_bytes"]
    g = g2 = None
    with images(engine, bits) as (img,):
        enqueue = lambda: hip.jh_distance(ctx, img.id, img.id, ctypes.byref(d))  # noqa: E731
        try:
            engine.trim_scratch()  # the planes have to be allocated again
            rc, msg, refused = captured_call(engine, enqueue)
            engine.graph_destroy(refused)
            assert rc == JH_ERR_OOM and msg.startswith("jh_distance: ") and "once eagerly first" in msg, (rc, msg)
            assert np.array_equal(img.bits(), bits)
            # ... the context stays usable, and after that eager call the same capture works
            engine.distance(img.id, max_distance=5, scale=-1.0, offset=6.0, straight=True)
            once = img.bits()
            assert np.array_equal(once, ref(bits, 5))
            rc, msg, g = captured_call(engine, enqueue)
            assert rc == 0, msg
            assert np.array_equal(img.bits(), once)  # a capture runs nothing
            engine.replay(g)
            twice = img.bits()
            assert np.array_equal(twice, ref(once, 5))
            rc, msg, g2 = captured_call(engine, lambda: hip.jh_distance(ctx, img.id, img.id, ctypes.byref(small)))
            assert rc == 0, msg
            engine.replay(g2)
            assert np.array_equal(img.bits(), ref(twice, 2))
        finally:
            for graph in (g, g2):
                if graph is not None:
                    engine.graph_destroy(graph)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_distance: ", no texel of any image and no byte
    of a canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    inf, nan = float("inf"), float("nan")
    with images(engine, canary, canary, canary_bits(W + 1, H), (W, H, ImageFormat.RGBA8)) as (src, dst, wider, rgba8):
        def call(s=None, d=None, rect=(0, 0, 0, 0), null=False, **fields):
            desc = CDistanceDesc(3, 0.5, 0, 0, 2, 1.0, 0.0)
            desc.x, desc.y, desc.width, desc.height = rect
            for k, v in fields.items():
                setattr(desc, k, v)
            return hip.jh_distance(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8), **{
            "sizes differ": (lambda: call(d=wider.id), b"differ in size"),
            "channel 4": (lambda: call(channel=4), b"unknown channel"),
            "channel -1": (lambda: call(channel=-1), b"unknown channel"),
            "which 3": (lambda: call(which=3), b"unknown which"),
            "which -1": (lambda: call(which=-1), b"unknown which"),
            "edge 2": (lambda: call(edge=2), b"unknown edge mode"),
            "edge -1": (lambda: call(edge=-1), b"unknown edge mode"),
            "flag bit 1": (lambda: call(flags=2), b"unknown flag bits"),
            "flag bit 31": (lambda: call(flags=0x80000001), b"unknown flag bits"),
            "R 0": (lambda: call(max_distance=0), b"max_distance"),
            "R 256": (lambda: call(max_distance=256), b"max_distance"),
            "R 2^32 - 1": (lambda: call(max_distance=0xFFFFFFFF), b"max_distance"),
            "threshold Inf": (lambda: call(threshold=inf), b"threshold is not finite"),
            "threshold NaN": (lambda: call(threshold=nan), b"threshold is not finite"),
            "scale -Inf": (lambda: call(scale=-inf), b"scale or offset is not finite"),
            "scale NaN": (lambda: call(scale=nan), b"scale or offset is not finite"),
            "offset Inf": (lambda: call(offset=inf), b"scale or offset is not finite"),
            "offset NaN": (lambda: call(offset=nan), b"scale or offset is not finite"),
        })
        check_refusals(engine, "jh_distance", call, refused, untouched=((src, canary), (dst, canary), (wider, canary_bits(W + 1, H))),
                       raises=(lambda: engine.distance(src.id, dst.id, max_distance=256), lambda: engine.distance(src.id, dst.id, max_distance=0),
                               lambda: engine.distance(src.id, dst.id, scale=inf), lambda: engine.distance(src.id, dst.id, rect=(8, 0, 9, 4))),
                       accepted=(call, lambda: call(max_distance=255), lambda: call(max_distance=1, which=2, edge=1, flags=1, channel=0)))


def test_the_call_is_one_query_of_the_tree(engine):
    bits = distance_cases.content("blob", None, 48, 33, 3, seed=2)
    kw = dict(max_distance=4, scale=-1.0, offset=5.0, straight=True)
    with images(engine, bits) as (img,):
        one_query(engine, "distance", lambda: engine.distance(img.id, **kw))
        got = img.bits()
    ref = lambda b: distance_ref.distance(b, R=4, scale=-1.0, offset=5.0, flags=distance_ref.STRAIGHT)  # noqa: E731
    assert np.array_equal(got, ref(ref(bits)))
