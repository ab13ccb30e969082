"""-m gpu: jh_lighting against the rule of DESIGN.md 5.14 (tests/lighting_ref.py) byte for byte -- the battery of
tests/lighting_cases.py (every instantiation of the kernel), a rendered frame through Engine.bevel against the composed references, the
residency of the power tables, a captured frame -- and the call's frame: its refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import Compose, ImageFormat, LightKind, LightSource, lighting
from jello_amd._lib import CLightingDesc
from jello_amd.engine import JH_ERR_INVALID, _lighting_desc

import blur_ref
import composite_ref
import lighting_cases
import lighting_ref
from devmem import target_of
from image_call import (JH_ERR_OOM, assert_same_bits, canary_bits, captured_call, captured_with_the_frame, check_refusals, common_refusals, images,
                        one_query, run_case, scene)

pytestmark = pytest.mark.gpu

SLOT = 19  # JH_SCR_LIGHT_TABLES
TABLE_BYTES = 4097 * 4


def _ref_kw(k):
    return {n: (int(v) if n in ("kind", "light") else v) for n, v in k.items()}


@pytest.mark.parametrize("name", [c["name"] for c in lighting_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.lighting: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = lighting_cases.BY_NAME[name]
    call = lambda src, dst: engine.lighting(src.id, dst.id, rect=c["rect"], **c["desc"])  # noqa: E731
    got = run_case(engine, c, call, lighting_cases.source(c), lighting_cases.before(c), dst_size=c["size"])
    assert_same_bits(got, lighting_cases.expected(name), name)


def test_the_battery_runs_every_instantiation():
    assert {c["inst"] for c in lighting_cases.CASES} == {
        "diffuse/distant/0", "diffuse/point/0", "diffuse/spot/0", "diffuse/spot/2", "specular/distant/0", "specular/distant/1", "specular/point/0",
        "specular/point/1", "specular/spot/0", "specular/spot/1", "specular/spot/2", "specular/spot/3"}


@pytest.mark.parametrize("light", ["distant", "point", "spot"])
def test_bevel_of_a_rendered_frame(engine, light):
    """Engine.bevel on a rendered 128 x 128 frame (a disc and a stroked curve) = blur_ref, lighting_ref and composite_ref composed on
    the download of the same render; the layer itself is untouched and the highlight is there."""
    lt = {"distant": lighting.distant(225, 35), "point": lighting.point(-50, -100, 200), "spot": lighting.spot(20, 10, 60, (64, 64, 0), 8, 40)}[light]
    rec, _, _ = engine.render(*scene(stroke=9))
    layer = target_of(engine, rec)
    assert layer.any()
    back = np.zeros((128, 128, 4), np.float16)
    back[...] = (0.1, 0.15, 0.2, 1.0)
    back = back.view(np.uint16)
    with images(engine, back, (128, 128), (128, 128)) as (target, a, b):
        engine.bevel(rec.target["id"], target.id, a.id, b.id, 3.0, lt, (128, 128), surface_scale=5.0, ks=0.75, exponent=20.0)
        got, got_b = target.bits(), b.bits()
    blurred = blur_ref.blur(layer, 3.0)
    lit = lighting_ref.lighting(blurred, kind=lighting_ref.SPECULAR, surface_scale=5.0, constant=0.75, specular_exponent=20.0,
                                **{k: (int(v) if k == "light" else v) for k, v in lt.items()})
    inside = composite_ref.composite(layer, lit, compose=int(Compose.DestIn))
    want = composite_ref.composite(inside, composite_ref.composite(layer, back), compose=int(Compose.Plus))
    assert_same_bits(got_b, inside, light + " highlight")
    assert_same_bits(got, want, light)
    assert np.array_equal(target_of(engine, rec), layer)
    assert inside[..., 3].view(np.float16).max() > 0.05  # there is a highlight
    assert not np.array_equal(got, composite_ref.composite(layer, back))


def test_captures_and_the_resident_key():
    """On a fresh context: a call that needs no table is capturable at once and leaves the slot at 0 bytes; a capture whose tables
    are not resident is refused with the advice and touches nothing; after one eager call it is recorded (and runs nothing); the same
    key again -- another light position, another colour -- uploads nothing (the slot's size and the graph stay); another key replaces
    the tables and makes the graph stale; jh_scratch_trim forgets the key."""
    engine = jello_amd.Engine(0)
    hip, ctx = engine.hip, engine.ctx
    bits = lighting_cases.content("disc", 37, 19, 8)
    poison = np.full((19, 37, 4), lighting_cases.POISON, np.uint16)
    plain = dict(lighting.diffuse(4.0, 1.0), **lighting.point(10, 5, 20))
    plain_spot = dict(lighting.specular(4.0, 1.0, 1.0), **lighting.spot(10, 5, 20, (18, 9, 0), 1.0, 50))
    shiny = dict(lighting.specular(4.0, 1.0, 20.0), **lighting.point(10, 5, 20))
    shiny_moved = dict(lighting.specular(2.0, 0.5, 20.0, (1.0, 0.5, 0.25)), **lighting.distant(30, 60))
    both = dict(lighting.specular(4.0, 1.0, 20.0), **lighting.spot(10, 5, 20, (18, 9, 0), 8.0, 50))
    ref = lambda kw: lighting_ref.lighting(bits, None, poison, **_ref_kw(kw))  # noqa: E731
    captured = lambda kw, **more: captured_call(  # noqa: E731
        engine, lambda: hip.jh_lighting(ctx, src.id, dst.id, ctypes.byref(_lighting_desc(**kw))), **more)
    graphs = []
    try:
        with images(engine, bits, poison, 64) as (src, dst, buf):
            try:
                for kw in (plain, plain_spot):  # no tables: capturable on a fresh context, and the slot stays empty
                    rc, msg, g = captured(kw)
                    graphs.append(g)
                    assert rc == 0, msg
                    assert np.array_equal(dst.bits(), poison)  # a capture runs nothing
                    engine.replay(g)
                    assert lighting_ref.same_bits(dst.bits(), ref(kw))
                    assert hip.jh_debug_scratch_bytes(ctx, SLOT) == 0
                    engine.upload_image(dst.id, poison)
                # a key that is not resident
                rc, msg, refused = captured(shiny, clear_first=buf.id)
                engine.graph_destroy(refused)
                assert rc == JH_ERR_OOM and msg.startswith("jh_lighting: ") and "run this lighting once eagerly first" in msg, (rc, msg)
                assert np.array_equal(dst.bits(), poison) and np.array_equal(src.bits(), bits)
                engine.lighting(src.id, dst.id, **shiny)
                assert lighting_ref.same_bits(dst.bits(), ref(shiny))
                size = hip.jh_debug_scratch_bytes(ctx, SLOT)
                assert size >= 2 * TABLE_BYTES
                engine.upload_image(dst.id, poison)
                rc, msg, g = captured(shiny)
                graphs.append(g)
                assert rc == 0, msg
                assert np.array_equal(dst.bits(), poison)
                engine.replay(g)
                assert lighting_ref.same_bits(dst.bits(), ref(shiny))
                # the same key with another light, scale, constant and colour, and calls without tables: nothing is uploaded, the
                # graph stays valid
                engine.lighting(src.id, dst.id, **shiny_moved)
                assert lighting_ref.same_bits(dst.bits(), ref(shiny_moved))
                engine.lighting(src.id, dst.id, **plain)
                assert hip.jh_debug_scratch_bytes(ctx, SLOT) == size
                engine.replay(g)
                assert lighting_ref.same_bits(dst.bits(), ref(shiny))
                # another key: its tables replace the ones the graph reads
                engine.lighting(src.id, dst.id, **both)
                assert hip.jh_graph_launch(ctx, g) == JH_ERR_INVALID
                assert b"stale" in hip.jh_last_error(ctx)
                assert lighting_ref.same_bits(dst.bits(), ref(both))
                engine.lighting(src.id, dst.id, **shiny)  # (and back: the specular exponent alone is another key than both exponents)
                assert lighting_ref.same_bits(dst.bits(), ref(shiny))
                # a trim forgets the key: the same lighting is no longer capturable until it has run again
                engine._check(hip.jh_scratch_trim(ctx), "scratch_trim")
                rc, msg, refused = captured(shiny)
                engine.graph_destroy(refused)
                assert rc == JH_ERR_OOM and "run this lighting once eagerly first" in msg
                engine.lighting(src.id, dst.id, **shiny)
                assert lighting_ref.same_bits(dst.bits(), ref(shiny))
            finally:
                for g in graphs:
                    engine.graph_destroy(g)
    finally:
        engine.close()


def test_captured_with_the_frame(engine):
    """capture(lighting=..., surface=...): render, light the target's alpha into a second image, blit that image -- one launch more
    than with the blit alone (the tables are resident, nothing is uploaded), replayed twice, the bytes of the eager calls."""
    k = dict(lighting.specular(6.0, 1.0, 20.0, (1.0, 0.9, 0.8)), **lighting.point(30, 20, 50))
    captured_with_the_frame(engine, scene(stroke=9), lambda target, dst: engine.lighting(target, dst, **k), lambda dst: dict(lighting=dict(dst=dst, **k)),
                            lambda plain: lighting_ref.lighting(plain, **_ref_kw(k)), extra_launches=1, out_size=(128, 128), baseline_surface=True)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_lighting: ", no texel of either image and no byte
    of a canary buffer touched; a valid call works afterwards."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    nan, inf = math.nan, math.inf
    point = dict(light=1, position=(1.0, 2.0, 3.0))
    spot = dict(light=2, position=(1.0, 2.0, 3.0), points_at=(4.0, 5.0, 0.0))
    with images(engine, canary, canary, (W, H, ImageFormat.RGBA8), (W + 1, H), ((1 << 23) + 1, 1), ((1 << 23) + 1, 1)) as (src, dst, rgba8, other, wide_a, wide_b):
        def call(s=None, d=None, null=False, **kw):
            desc = _lighting_desc(**kw)
            return hip.jh_lighting(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8), **{
            "images of different size": (lambda: call(d=other.id), b"size"),
            "source is the destination": (lambda: call(d=src.id), b"source is the destination"),
            "an extent above 2^23": (lambda: call(s=wide_a.id, d=wide_b.id), b"2^23"),
            "kind 2": (lambda: call(kind=2), b"kind"),
            "kind -1": (lambda: call(kind=-1), b"kind"),
            "light 3": (lambda: call(light=3), b"light"),
            "light -1": (lambda: call(light=-1), b"light"),
            "a NaN surface_scale": (lambda: call(surface_scale=nan), b"surface_scale"),
            "an infinite surface_scale": (lambda: call(surface_scale=-inf), b"surface_scale"),
            "a negative constant": (lambda: call(constant=-1e-30), b"constant"),
            "a NaN constant": (lambda: call(constant=nan), b"constant"),
            "an infinite constant": (lambda: call(constant=inf), b"constant"),
            "specular_exponent below 1": (lambda: call(kind=1, specular_exponent=0.99999994), b"specular_exponent"),
            "specular_exponent above 128": (lambda: call(kind=1, specular_exponent=128.00002), b"specular_exponent"),
            "a NaN specular_exponent": (lambda: call(kind=1, specular_exponent=nan), b"specular_exponent"),
            "a negative color": (lambda: call(color=(1.0, -0.5, 1.0)), b"color"),
            "a NaN color": (lambda: call(color=(1.0, 1.0, nan)), b"color"),
            "an infinite color": (lambda: call(color=(inf, 1.0, 1.0)), b"color"),
            "a zero direction": (lambda: call(direction=(0.0, 0.0, -0.0)), b"direction"),
            "a NaN direction": (lambda: call(direction=(0.0, nan, 1.0)), b"direction"),
            "a direction whose length overflows": (lambda: call(direction=(1e200, 0.0, 1.0)), b"direction"),
            "a direction whose length underflows": (lambda: call(direction=(1e-200, 0.0, 0.0)), b"direction"),
            "an infinite position": (lambda: call(light=1, position=(inf, 0.0, 0.0)), b"position"),
            "a position beyond binary32": (lambda: call(light=1, position=(0.0, 1e39, 0.0)), b"position"),
            "a NaN spot position": (lambda: call(**dict(spot, position=(0.0, 0.0, nan))), b"position"),
            "points_at the position": (lambda: call(**dict(spot, points_at=(1.0, 2.0, 3.0))), b"points_at"),
            "a NaN points_at": (lambda: call(**dict(spot, points_at=(nan, 2.0, 3.0))), b"points_at"),
            "spot_exponent below 1": (lambda: call(spot_exponent=0.5, **spot), b"spot_exponent"),
            "spot_exponent above 128": (lambda: call(spot_exponent=129.0, **spot), b"spot_exponent"),
            "cone_cos above 1": (lambda: call(cone_cos=1.0000000000000002, **spot), b"cone_cos"),
            "cone_cos below -1": (lambda: call(cone_cos=-1.5, **spot), b"cone_cos"),
            "a NaN cone_cos": (lambda: call(cone_cos=nan, **spot), b"cone_cos"),
        })
        # (accepted: fields the kind and the light do not use are not looked at; the boundaries themselves are legal)
        check_refusals(engine, "jh_lighting", call, refused, untouched=((src, canary), (dst, canary)),
                       raises=(lambda: engine.lighting(src.id, src.id),
                               lambda: engine.lighting(src.id, dst.id, **dict(lighting.specular(exponent=200), **lighting.distant(0, 45))),
                               lambda: engine.lighting(src.id, dst.id, color=(1.0, 1.0))),
                       accepted=(lambda: call(specular_exponent=nan, spot_exponent=nan, position=(nan,) * 3, points_at=(nan,) * 3, cone_cos=nan, rect=(3, 3, 2, 2)),
                                 lambda: call(direction=(nan,) * 3, spot_exponent=0.0, rect=(3, 3, 2, 2), **point),
                                 lambda: call(specular_exponent=128.0, spot_exponent=1.0, cone_cos=1.0, rect=(3, 3, 2, 2), kind=1, **spot),
                                 lambda: call(specular_exponent=1.0, spot_exponent=128.0, cone_cos=-1.0, constant=0.0, rect=(3, 3, 2, 2), kind=1, **spot)))
        want = canary.copy()
        want[3:5, 3:5] = 0  # (the last call: a constant of 0 gives transparent black under SPECULAR)
        assert np.array_equal(dst.bits(), want)
        assert np.array_equal(src.bits(), canary)
        with images(engine, (0, 5), (0, 5)) as (empty_a, empty_b):
            assert hip.jh_lighting(ctx, empty_a.id, empty_b.id, ctypes.byref(CLightingDesc(0, 0, 1.0, 1.0, 1.0, 1.0, (ctypes.c_float * 3)(1, 1, 1), 0, 0, 0, 0,
                                                                                            (ctypes.c_double * 3)(0, 0, 1)))) == 0  # (an image without texels)
    assert point["light"] == int(LightSource.POINT) and int(LightKind.SPECULAR) == 1


def test_the_call_is_one_query_of_the_tree(engine):
    bits = lighting_cases.content("disc", 48, 33, 2)
    k = dict(lighting.diffuse(5.0, 1.2), **lighting.distant(45, 30))
    with images(engine, bits, (48, 33)) as (src, dst):
        one_query(engine, "lighting", lambda: engine.lighting(src.id, dst.id, **k))
        got = dst.bits()
    assert lighting_ref.same_bits(got, lighting_ref.lighting(bits, **_ref_kw(k)))
