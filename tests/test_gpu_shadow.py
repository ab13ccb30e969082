"""-m gpu: jh_shadow against the rule of DESIGN.md 5.18 (tests/shadow_ref.py) byte for byte -- the battery of tests/shadow_cases.py
(every instantiation of the kernel) --, OVER against STORE followed by Engine.composite on the device, the texels outside
shadow_bounds, Engine.box_shadow on a rendered scene, four quadrant calls against one, a captured frame -- and the call's frame: its
refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import ImageFormat, ShadowFlags
from jello_amd._lib import CShadowDesc
from jello_amd.engine import RUN_DISPATCHES, RUN_UPLOADS, _shadow_desc

import shadow_cases
import shadow_ref
from devmem import target_of
from image_call import (assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query, run_case, scene)
from shadow_ref import INVERT, OVER

pytestmark = pytest.mark.gpu


def _keywords(desc):
    """The keywords of Engine.shadow for a case's desc."""
    d = dict(shadow_ref.DEFAULTS, **desc)
    flags = d.pop("flags")
    return dict(d, over=bool(flags & OVER), invert=bool(flags & INVERT))


@pytest.mark.parametrize("name", [c["name"] for c in shadow_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.shadow: dst holds the case's prior content (or was never written), the whole of dst is compared -- the
    rectangle with the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = shadow_cases.BY_NAME[name]
    call = lambda _, dst: engine.shadow(dst.id, rect=c["rect"], **_keywords(c["desc"]))  # noqa: E731
    got = run_case(engine, c, call, None, shadow_cases.before(c), dst_size=c["size"])
    assert_same_bits(got, shadow_cases.expected(name), name)


def test_the_battery_runs_every_instantiation():
    assert {c["inst"] for c in shadow_cases.CASES} == {"round/store", "round/over", "sharp/store", "sharp/over"}


@pytest.mark.parametrize("radius, invert", [(0.0, False), (7.0, False), (7.0, True)])
def test_over_equals_store_then_composite_on_the_device(engine, radius, invert):
    """The two routes to the same bits, both on the device: shadow(over=True) onto a backdrop, and shadow() into a second image that
    Engine.composite (Normal + SrcOver) lays over the same backdrop."""
    kw = dict(box=(9.0, 5.0, 71.0, 30.0), radius=radius, sigma=2.5, color=(0.05, 0.1, 0.3, 0.8), invert=invert)
    rng = np.random.default_rng(11)
    backdrop = rng.uniform(0.0, 1.0, (37, 83, 4)).astype(np.float16).view(np.uint16)
    with images(engine, backdrop, backdrop, (83, 37)) as (direct, composed, layer):
        engine.shadow(direct.id, over=True, **kw)
        engine.shadow(layer.id, **kw)
        engine.composite(layer.id, composed.id)
        a, b = direct.bits(), composed.bits()
    assert np.array_equal(a, b)
    assert (a != backdrop).any()
    flags = OVER | (INVERT if invert else 0)
    assert_same_bits(a, shadow_ref.shadow((37, 83), None, backdrop, **dict({k: v for k, v in kw.items() if k != "invert"}, flags=flags)), "over")


@pytest.mark.parametrize("matrix", ["id", "rot30", "scale"])
def test_the_texels_outside_shadow_bounds_are_below_2_to_the_minus_12(engine, matrix):
    """A STORE of the whole image with colour (1, 1, 1, 1): alpha is S.  Outside jh_shadow_bounds' rectangle every alpha is below
    2^-12; inside it some are not (the rectangle is not everything)."""
    m = shadow_cases.MATRICES[matrix]
    kw = dict(box=(40.0, 30.0, 90.0, 60.0), radius=8.0, sigma=3.0, matrix=m)
    W, H = 190, 100
    x, y, w, h = jello_amd.shadow_bounds(kw["box"], kw["radius"], kw["sigma"], (W, H), m)
    assert 0 < w * h < W * H
    with images(engine, (W, H)) as (dst,):
        engine.shadow(dst.id, color=(1.0, 1.0, 1.0, 1.0), **kw)
        alpha = dst.bits()[..., 3].view(np.float16).astype(np.float32)
    inside = np.zeros((H, W), bool)
    inside[y:y + h, x:x + w] = True
    assert alpha[~inside].max() < 2.0 ** -12
    assert alpha[inside].max() > 0.9


def test_box_shadow_on_a_rendered_scene_equals_the_composed_references(engine):
    """Engine.box_shadow onto the frame's target: one call over shadow_bounds' rectangle, the texels outside it as rendered."""
    s, p = scene((128, 128))
    rec = jello_amd.Host().record(s, p)
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    plain = target_of(engine, rec)
    box, radius, sigma, offset, spread, color = (30.0, 40.0, 90.0, 80.0), 6.0, 3.0, (4.0, 6.0), 2.0, (0.0, 0.0, 0.0, 0.6)
    rect = engine.box_shadow(rec.target, box, radius, sigma, offset, spread, color)
    got = target_of(engine, rec)
    shape, r = jello_amd.box_shadow_geometry(box, radius, offset, spread)
    assert shape == (32.0, 44.0, 96.0, 88.0) and r == 8.0
    assert rect == shadow_ref.bounds(shape, r, sigma, shadow_ref.IDENTITY, (128, 128)) and 0 < rect[2] < 128
    want = shadow_ref.shadow((128, 128), rect, plain, box=shape, radius=r, sigma=sigma, color=color, flags=OVER)
    assert_same_bits(got, want, "box_shadow")
    assert (got != plain).any()


@pytest.mark.parametrize("over", [False, True])
def test_four_quadrant_calls_equal_one_call(engine, over):
    kw = dict(box=(8.0, 6.0, 62.0, 31.0), radius=9.0, sigma=2.0, color=(0.2, 0.1, 0.0, 0.7), matrix=shadow_cases.MATRICES["rot30"], over=over)
    rng = np.random.default_rng(3)
    held = rng.uniform(0.0, 1.0, (37, 71, 4)).astype(np.float16).view(np.uint16)
    with images(engine, held, held) as (whole, parts):
        engine.shadow(whole.id, **kw)
        for rect in ((0, 0, 33, 18), (33, 0, 38, 18), (0, 18, 33, 19), (33, 18, 38, 19)):
            engine.shadow(parts.id, rect=rect, **kw)
        a, b = whole.bits(), parts.bits()
    assert np.array_equal(a, b) and (a != held).any()


def test_captured_with_the_frame(engine):
    """capture(shadow=..., surface=...): one launch more than the frame with its blit, nothing to run eagerly first; replayed twice."""
    kw = dict(box=(20.0, 30.0, 100.0, 90.0), radius=10.0, sigma=4.0, color=(0.0, 0.0, 0.1, 0.5), over=True)
    ref = dict(box=kw["box"], radius=kw["radius"], sigma=kw["sigma"], color=kw["color"], flags=OVER)
    captured_with_the_frame(engine, scene((128, 128)), lambda t, _: engine.shadow(t, **kw), lambda _: dict(shadow=kw),
                            lambda plain: shadow_ref.shadow((128, 128), None, plain, **ref), extra_launches=1, baseline_surface=True)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_shadow: ", no texel of the image and no byte of a
    canary buffer touched; a valid call works afterwards."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    nan, inf = math.nan, math.inf
    with images(engine, canary, (W, H, ImageFormat.RGBA8)) as (dst, rgba8):
        def call(d=None, null=False, flags=None, rect=None, **kw):
            args = dict(box=(2.0, 2.0, 10.0, 8.0), radius=1.0, sigma=1.0, color=(0.0, 0.0, 0.0, 1.0))
            args.update(kw)
            with np.errstate(all="ignore"):
                desc = _shadow_desc(rect=rect, **args)
            if flags is not None:
                desc.flags = flags
            return hip.jh_shadow(ctx, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, source=False), **{
            "an infinite box": (lambda: call(box=(2.0, 2.0, inf, 8.0)), b"the box is not finite"),
            "a NaN box": (lambda: call(box=(nan, 2.0, 10.0, 8.0)), b"the box is not finite"),
            "x1 < x0": (lambda: call(box=(10.0, 2.0, 9.5, 8.0)), b"x1 < x0"),
            "y1 < y0": (lambda: call(box=(2.0, 8.0, 10.0, 7.0)), b"y1 < y0"),
            "a box beyond 2^22": (lambda: call(box=(2.0, 2.0, 2.0 ** 22 + 1.0, 8.0)), b"above 2^22"),
            "a negative radius": (lambda: call(radius=-1.0), b"radius"),
            "a NaN radius": (lambda: call(radius=nan), b"radius"),
            "an infinite radius": (lambda: call(radius=inf), b"radius"),
            "a negative sigma": (lambda: call(sigma=-0.5), b"sigma"),
            "a sigma above 2^16": (lambda: call(sigma=65537.0), b"sigma"),
            "a NaN sigma": (lambda: call(sigma=nan), b"sigma"),
            "an unknown flag": (lambda: call(flags=4), b"unknown flag bits"),
            "a singular matrix": (lambda: call(matrix=(1.0, 2.0, 2.0, 4.0, 0.0, 0.0)), (b"illegal matrix", b"determinant is 0")),
            "a NaN matrix": (lambda: call(matrix=(nan, 0.0, 0.0, 1.0, 0.0, 0.0)), (b"illegal matrix", b"not finite")),
            "a matrix that minifies beyond 64": (lambda: call(matrix=(1.0 / 65.0, 0.0, 0.0, 1.0, 0.0, 0.0)), b"above 64"),
        })
        check_refusals(engine, "jh_shadow", call, refused, untouched=((dst, canary),),
                       raises=(lambda: engine.shadow(dst.id, (2.0, 2.0, 1.0, 8.0), 1.0, 1.0, (0, 0, 0, 1)), lambda: engine.shadow(dst.id, (2.0, 2.0, 8.0), 1.0, 1.0, (0, 0, 0, 1))),
                       accepted=(lambda: call(box=(2.0, 2.0, 2.0, 8.0)),  # ... and the boundaries themselves are legal
                                 lambda: call(box=(-2.0 ** 22, -2.0 ** 22, 2.0 ** 22, 2.0 ** 22), radius=1e30, sigma=65536.0, rect=(3, 3, 2, 2)),
                                 lambda: call(sigma=0.0, radius=0.0, flags=3, rect=(3, 3, 2, 2)),
                                 lambda: call(box=(-100.0, -100.0, 100.0, 100.0), color=(0.5, 0.25, 0.125, 1.0), rect=(3, 3, 2, 2))))
        want = canary.copy()
        want[:] = 0  # (the first accepted call: a box empty in x over the whole image, transparent black)
        want[3:5, 3:5] = np.array([0.5, 0.25, 0.125, 1.0], np.float16).view(np.uint16)  # (the last: S = 1 under an opaque colour)
        assert np.array_equal(dst.bits(), want)
        with images(engine, (0, 5)) as (empty,):
            assert hip.jh_shadow(ctx, empty.id, ctypes.byref(CShadowDesc())) != 0  # (a zero matrix is refused before the empty image is looked at)
            assert hip.jh_shadow(ctx, empty.id, ctypes.byref(_shadow_desc((0.0, 0.0, 1.0, 1.0), 0.0, 1.0, (0, 0, 0, 1)))) == 0  # (an image without texels)
    assert int(ShadowFlags.OVER) == 1 and int(ShadowFlags.INVERT) == 2


def test_the_call_is_one_query_of_the_tree(engine):
    kw = dict(box=(5.0, 4.0, 40.0, 28.0), radius=5.0, sigma=2.0, color=(0.0, 0.0, 0.0, 0.5))
    with images(engine, (48, 33)) as (dst,):
        one_query(engine, "shadow", lambda: engine.shadow(dst.id, **kw))
        got = dst.bits()
    assert_same_bits(got, shadow_ref.shadow((33, 48), None, None, flags=0, **kw), "profiled")
