"""-m gpu: jh_turbulence against the rule of DESIGN.md 5.15 (tests/turbulence_ref.py) byte for byte -- the battery of
tests/turbulence_cases.py (every instantiation of the kernel), a never-written destination, two images with adjoining origins,
Engine.lit_noise against the composed references, the residency of the tables, a captured frame -- and the call's frame: its refusals,
its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import ImageFormat, Surface, TurbulenceKind, lighting
from jello_amd._lib import CTurbulenceDesc
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS, _turbulence_desc

import lighting_ref
import surface_ref
import turbulence_cases
import turbulence_ref
from devmem import target_of
from image_call import (JH_ERR_OOM, assert_equal_bits, assert_same_bits, canary_bits, captured_call, check_refusals, common_refusals, images,
                        one_query, run_case, scene)

pytestmark = pytest.mark.gpu

SLOT = 20  # JH_SCR_TURB_TABLES
TABLE_BYTES = 2048 * 4 + 256


def _ref(size, rect=None, prior=None, **kw):
    return turbulence_ref.turbulence((size[1], size[0]), rect, prior, **{k: (int(v) if k == "kind" else v) for k, v in kw.items()})


@pytest.mark.parametrize("name", [c["name"] for c in turbulence_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.turbulence: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = turbulence_cases.BY_NAME[name]
    call = lambda _, dst: engine.turbulence(dst.id, rect=c["rect"], **c["desc"])  # noqa: E731
    got = run_case(engine, c, call, None, turbulence_cases.before(c), dst_size=c["size"])
    assert_equal_bits(got, turbulence_cases.expected(name), name)


def test_the_battery_runs_every_instantiation():
    assert {c["inst"] for c in turbulence_cases.CASES} == {"fractal/0", "fractal/1", "turbulence/0", "turbulence/1"}


def test_a_never_written_destination_and_the_texels_outside_the_rectangle(engine):
    """A rectangle of a never-written image: transparent black around it, and the image counts as written afterwards (a second
    rectangle keeps the first); on a written image every texel outside the rectangle keeps its bits."""
    kw = dict(base_frequency=(0.08, 0.05), octaves=3, seed=11, kind=TurbulenceKind.FRACTAL_NOISE, origin=(4.0, -2.5))
    rng = np.random.default_rng(5)
    held = rng.integers(0, 0x7C00, (23, 41, 4)).astype(np.uint16)
    with images(engine, (41, 23), held) as (fresh, written):
        engine.turbulence(fresh.id, rect=(3, 5, 17, 9), **kw)
        first = fresh.bits()
        want = _ref((41, 23), (3, 5, 17, 9), None, **kw)
        assert_equal_bits(first, want, "first rectangle")
        assert not first[:5].any() and not first[:, :3].any() and first[5:14, 3:20].any()
        engine.turbulence(fresh.id, rect=(25, 1, 9, 20), **kw)
        want = _ref((41, 23), (25, 1, 9, 20), want, **kw)
        assert np.array_equal(fresh.bits(), want)
        engine.turbulence(written.id, rect=(1, 1, 39, 21), **kw)
        got = written.bits()
        assert_equal_bits(got, _ref((41, 23), (1, 1, 39, 21), held, **kw), "written")
        assert np.array_equal(got[0], held[0]) and np.array_equal(got[:, 40], held[:, 40])


@pytest.mark.parametrize("kind", [TurbulenceKind.FRACTAL_NOISE, TurbulenceKind.TURBULENCE])
def test_two_images_with_adjoining_origins_equal_one_image_of_both(engine, kind):
    """Frequencies and origins whose products are exact (multiples of 2^-7), so that both halves sit on the one position grid."""
    kw = dict(base_frequency=(0.0625, 0.09375), octaves=4, seed=21, kind=kind)
    with images(engine, (70, 19), (33, 19), (37, 19)) as (whole, left, right):
        engine.turbulence(whole.id, origin=(-8.0, 3.0), **kw)
        engine.turbulence(left.id, origin=(-8.0, 3.0), **kw)
        engine.turbulence(right.id, origin=(25.0, 3.0), **kw)
        w, a, b = whole.bits(), left.bits(), right.bits()
    assert np.array_equal(w, _ref((70, 19), origin=(-8.0, 3.0), **kw))
    assert np.array_equal(w[:, :33], a) and np.array_equal(w[:, 33:], b)
    assert len(np.unique(w[..., 3])) > 50  # there is noise


@pytest.mark.parametrize("light", ["distant", "point"])
def test_lit_noise_equals_the_composed_references(engine, light):
    """Engine.lit_noise: turbulence into the scratch, feDiffuseLighting of the scratch's alpha into dst."""
    lt = {"distant": lighting.distant(225, 35), "point": lighting.point(20, 10, 60)}[light]
    noise = dict(base_frequency=(0.04, 0.06), octaves=4, seed=17)
    with images(engine, (96, 40), (96, 40)) as (dst, scratch):
        engine.lit_noise(dst.id, scratch.id, lt, surface_scale=6.0, kd=1.1, color=(1.0, 0.9, 0.7), **noise)
        got, got_noise = dst.bits(), scratch.bits()
    want_noise = _ref((96, 40), kind=turbulence_ref.TURBULENCE, **noise)
    want = lighting_ref.lighting(want_noise, kind=lighting_ref.DIFFUSE, surface_scale=6.0, constant=1.1, color=(1.0, 0.9, 0.7),
                                 **{k: (int(v) if k == "light" else v) for k, v in lt.items()})
    assert_equal_bits(got_noise, want_noise, "noise")
    assert_same_bits(got, want, light)
    assert len(np.unique(got[..., 0])) > 20 and np.all(got[..., 3] == 0x3C00)  # a lit, opaque surface


def test_captures_and_the_resident_key():
    """On a fresh context: the slot is empty and a capture is refused with the advice and touches nothing; after one eager call it is
    recorded (and runs nothing); the same seed again -- another kind, frequency, octave count, origin and stitch -- uploads nothing
    (the slot's size and the graph stay); seeds that setup_seed maps to the same key are the same key; another seed replaces the
    tables and makes the graph stale; jh_scratch_trim forgets the key."""
    engine = jello_amd.Engine(0)
    hip, ctx = engine.hip, engine.ctx
    poison = np.full((19, 37, 4), turbulence_cases.POISON, np.uint16)
    first = dict(base_frequency=(0.1, 0.07), octaves=3, seed=5)
    moved = dict(base_frequency=(0.3, 0.02), octaves=5, seed=5, kind=TurbulenceKind.FRACTAL_NOISE, origin=(-7.5, 2.0), stitch_tile=(0.0, 0.0, 20.0, 10.0))
    other = dict(base_frequency=(0.1, 0.07), octaves=3, seed=6)
    ref = lambda kw: _ref((37, 19), None, poison, **kw)  # noqa: E731
    captured = lambda kw, **more: captured_call(engine, lambda: hip.jh_turbulence(ctx, dst.id, ctypes.byref(_turbulence_desc(**kw))), **more)  # noqa: E731
    graphs = []
    try:
        with images(engine, poison, 64) as (dst, buf):
            try:
                assert hip.jh_debug_scratch_bytes(ctx, SLOT) == 0
                rc, msg, refused = captured(first, clear_first=buf.id)
                engine.graph_destroy(refused)
                assert rc == JH_ERR_OOM and msg.startswith("jh_turbulence: ") and "run this turbulence once eagerly first" in msg, (rc, msg)
                assert np.array_equal(dst.bits(), poison) and hip.jh_debug_scratch_bytes(ctx, SLOT) == 0
                engine.turbulence(dst.id, **first)
                assert np.array_equal(dst.bits(), ref(first))
                size = hip.jh_debug_scratch_bytes(ctx, SLOT)
                assert size >= TABLE_BYTES
                engine.upload_image(dst.id, poison)
                rc, msg, g = captured(first)
                graphs.append(g)
                assert rc == 0, msg
                assert np.array_equal(dst.bits(), poison)  # a capture runs nothing
                engine.replay(g)
                assert np.array_equal(dst.bits(), ref(first))
                # the same key with everything else changed: nothing is uploaded, the graph stays valid
                engine.turbulence(dst.id, **moved)
                assert np.array_equal(dst.bits(), ref(moved))
                assert hip.jh_debug_scratch_bytes(ctx, SLOT) == size
                engine.replay(g)
                assert np.array_equal(dst.bits(), ref(first))
                # seeds 0 and 1 are one key (setup_seed): the second uploads nothing and leaves a graph of the first valid
                engine.turbulence(dst.id, **dict(first, seed=0))
                rc, msg, g01 = captured(dict(first, seed=1))
                graphs.append(g01)
                assert rc == 0, msg
                assert hip.jh_graph_launch(ctx, g) == JH_ERR_INVALID and b"stale" in hip.jh_last_error(ctx)  # (seed 0 replaced seed 5's tables)
                engine.turbulence(dst.id, **dict(first, seed=1))
                engine.replay(g01)
                assert np.array_equal(dst.bits(), ref(dict(first, seed=0)))
                # another key: its tables replace the ones the graph reads
                engine.turbulence(dst.id, **other)
                assert hip.jh_graph_launch(ctx, g01) == JH_ERR_INVALID
                assert b"stale" in hip.jh_last_error(ctx)
                assert np.array_equal(dst.bits(), ref(other))
                # a trim forgets the key: the same turbulence is no longer capturable until it has run again
                engine._check(hip.jh_scratch_trim(ctx), "scratch_trim")
                rc, msg, refused = captured(other)
                engine.graph_destroy(refused)
                assert rc == JH_ERR_OOM and "run this turbulence once eagerly first" in msg
                engine.turbulence(dst.id, **other)
                assert np.array_equal(dst.bits(), ref(other))
            finally:
                for g in graphs:
                    engine.graph_destroy(g)
    finally:
        engine.close()


def test_captured_with_the_frame(engine):
    """capture(turbulence=..., surface=...): render, generate noise into a second image, blit the frame -- one launch more than
    with the blit alone (the tables are resident), replayed twice; the noise image holds the eager call's bytes, the frame is as
    without the noise.  (Written out, not image_call.captured_with_the_frame: the blit reads the frame, not what the call wrote, so
    what is compared after a replay is the baseline's surface and the noise image, and the image is overwritten before each replay.)"""
    s, p = scene(stroke=None)
    fmt = Surface.RGBA8_SRGB
    k = dict(base_frequency=(0.05, 0.05), octaves=4, seed=31, kind=TurbulenceKind.FRACTAL_NOISE)
    rec = jello_amd.Host().record(s, p)
    g = None
    with images(engine, (128, 128), 128 * 128 * 4, 128 * 128 * 4) as (noise, surf, full):
        try:
            engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
            plain = target_of(engine, rec)
            engine.turbulence(noise.id, **k)
            want = _ref((128, 128), **k)
            assert np.array_equal(noise.bits(), want)
            g0 = engine.capture(rec, surface=(full.ptr, 128 * 4, fmt))  # (the frame and the blit of its own target)
            g = engine.capture(rec, turbulence=dict(dst=noise.id, **k), surface=(surf.ptr, 128 * 4, fmt))
            (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
            engine.replay(g0)
            engine.sync()
            frame = full.bytes()[:128 * 128 * 4].reshape(128, 128, 4).copy()
            engine.graph_destroy(g0)
            assert (k1, o1) == (k0 + 1, o0)  # one launch; the tables are resident, nothing is uploaded
            assert np.array_equal(frame, surface_ref.convert(plain, int(fmt)))
            for _ in range(2):
                engine.clear(surf.id)
                engine.turbulence(noise.id, **dict(k, octaves=0))  # (other content, the same key: nothing is uploaded)
                engine.replay(g)
                engine.sync()
                assert np.array_equal(surf.bytes()[:128 * 128 * 4].reshape(128, 128, 4), frame)
                assert np.array_equal(noise.bits(), want)
            assert np.array_equal(target_of(engine, rec), plain)
        finally:
            if g is not None:
                engine.graph_destroy(g)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_turbulence: ", no texel of the image and no byte
    of a canary buffer touched; a valid call works afterwards."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    nan, inf = math.nan, math.inf
    with images(engine, canary, (W, H, ImageFormat.RGBA8), (769, 1)) as (dst, rgba8, wide):
        def call(d=None, null=False, stitch=None, **kw):
            desc = _turbulence_desc(**dict(dict(base_frequency=0.1), **kw))
            if stitch is not None:
                desc.stitch = stitch
            return hip.jh_turbulence(ctx, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, source=False), **{
            "kind 2": (lambda: call(kind=2), b"kind"),
            "kind -1": (lambda: call(kind=-1), b"kind"),
            "17 octaves": (lambda: call(octaves=17), b"octaves"),
            "stitch 2": (lambda: call(stitch=2), b"stitch"),
            "a negative base_frequency": (lambda: call(base_frequency=(0.1, -1e-300)), b"base_frequency"),
            "a NaN base_frequency": (lambda: call(base_frequency=(nan, 0.1)), b"base_frequency"),
            "an infinite base_frequency": (lambda: call(base_frequency=inf), b"base_frequency"),
            "a base_frequency of 2^30": (lambda: call(base_frequency=2.0 ** 30, origin=(-0.5, -0.5)), b"2^30"),
            "a NaN origin": (lambda: call(origin=(0.0, nan)), b"origin"),
            "an infinite origin": (lambda: call(origin=(-inf, 0.0)), b"origin"),
            "an origin beyond the range": (lambda: call(base_frequency=1.0, origin=(2.0 ** 30, 0.0)), b"position range"),
            "an origin beyond the range of 16 octaves": (lambda: call(base_frequency=1.0, octaves=16, origin=(0.0, -32769.0)), b"position range"),
            "an image beyond max_extent": (lambda: call(d=wide.id, base_frequency=(1.0, 0.0), octaves=16, origin=(32000.0, 0.0)), b"max_extent"),
            "an image beyond max_extent, whatever the rectangle": (  # (the IMAGE, not the rectangle)
                lambda: call(d=wide.id, base_frequency=(1.0, 0.0), octaves=16, origin=(32001.0, 0.0), rect=(766, 0, 1, 1)), b""),
            "a NaN stitch tile": (lambda: call(stitch_tile=(0.0, nan, 8.0, 8.0)), b"tile"),
            "an infinite stitch tile": (lambda: call(stitch_tile=(0.0, 0.0, inf, 8.0)), b"tile"),
            "an empty stitch tile": (lambda: call(stitch_tile=(0.0, 0.0, 8.0, 0.0)), b"tile is empty"),
            "a negative stitch tile": (lambda: call(stitch_tile=(0.0, 0.0, -8.0, 8.0)), b"tile is empty"),
            "a stitch tile beyond the lattice": (lambda: call(base_frequency=1.0, octaves=16, stitch_tile=(0.0, 0.0, 65536.0, 8.0)), b"lattice range"),
        })

        def without_stitch():  # the tile is not looked at without stitch
            desc = _turbulence_desc(base_frequency=0.1, rect=(3, 3, 2, 2))
            desc.tile[:] = (nan, nan, nan, nan)
            return hip.jh_turbulence(ctx, dst.id, ctypes.byref(desc))

        check_refusals(engine, "jh_turbulence", call, refused, untouched=((dst, canary),),
                       raises=(lambda: engine.turbulence(dst.id, 0.1, octaves=17), lambda: engine.turbulence(dst.id, (0.1, 0.2, 0.3)),
                               lambda: engine.turbulence(dst.id, 0.1, stitch_tile=(0.0, 0.0, 8.0))),
                       accepted=(without_stitch,  # ... and the boundaries themselves are legal
                                 lambda: call(base_frequency=1.0, octaves=16, origin=(32767.0 - W, -32768.0), rect=(3, 3, 2, 2)),
                                 lambda: call(base_frequency=1.0, octaves=16, stitch_tile=(0.0, 0.0, 65535.0, 8.0), rect=(3, 3, 2, 2)),
                                 lambda: call(octaves=0, kind=0, rect=(3, 3, 2, 2))))
        want = canary.copy()
        want[3:5, 3:5] = 0x3800  # (the last call: 0 octaves of FRACTAL_NOISE are 0.5 in all four channels)
        assert np.array_equal(dst.bits(), want)
        with images(engine, (0, 5)) as (empty,):
            assert hip.jh_turbulence(ctx, empty.id, ctypes.byref(CTurbulenceDesc(1, 1, 0, 0))) == 0  # (an image without texels)
    assert int(TurbulenceKind.TURBULENCE) == 1


def test_the_call_is_one_query_of_the_tree(engine):
    k = dict(base_frequency=0.05, octaves=2, seed=3)
    with images(engine, (48, 33)) as (dst,):
        engine.turbulence(dst.id, **k)  # (the tables are resident before the profile starts)
        one_query(engine, "turbulence", lambda: engine.turbulence(dst.id, **k))
        got = dst.bits()
    assert np.array_equal(got, _ref((48, 33), **k))
