"""-m gpu: jh_load_surface and jh_load_yuv against the rule of DESIGN.md 5.21 (tests/load_ref.py) byte for byte -- the batteries of
tests/load_cases.py, one test per kernel instantiation; the sources only read; jh_load_yuv against jh_load_surface of the reference's
codes and the round trip through jh_blit on the device; a loaded frame composited onto a rendered one; a captured frame -- and the
calls' frame: their refusals and their profile queries."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import ChromaFilter, LoadAlpha, Surface, YuvLayout, YuvMatrix, YuvRange, YuvTransfer
from jello_amd._lib import CLoadSurfaceDesc, CLoadYuvDesc

import composite_ref
import load_cases
import load_ref
from devmem import CANARY, DevBuf, target_of
from image_call import assert_equal_bits, assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query, scene
from jello_amd import ImageFormat

pytestmark = pytest.mark.gpu


def _dst_spec(case):
    prior = load_cases.prior_bits(case)
    return prior[::-1] if isinstance(prior, tuple) else prior  # (images() takes (width, height))


def _run_yuv(engine, case):
    """The case through Engine.load_yuv with device planes: what dst holds afterwards, having asserted the planes unchanged."""
    planes = load_cases.planes_of(case["y"], case["cb"], case["cr"], case["layout"])
    laid = [load_cases.in_memory(p, e, o, CANARY) for p, e, o in zip(planes, case["pitch_extra"], case["ptr_off"])]
    bufs = [DevBuf(engine, data=b.tobytes()) for b, _ in laid]
    try:
        with images(engine, _dst_spec(case)) as (dst,):
            engine.load_yuv(dst.id, [(buf.ptr + off, pitch) for buf, (_, pitch), off in zip(bufs, laid, case["ptr_off"])], YuvLayout(case["layout"]),
                            YuvMatrix(case["matrix"]), YuvRange(case["rng"]), YuvTransfer(case["transfer"]), ChromaFilter(case["chroma"]), rect=case["rect"])
            got = dst.bits()
        for buf, (b, _) in zip(bufs, laid):
            assert np.array_equal(buf.bytes()[:b.size], b), case["name"]  # the planes are only read
    finally:
        for buf in bufs:
            buf.free()
    return got


def _run_surface(engine, case):
    px = case["pixels"]
    b, pitch = load_cases.in_memory(px.reshape(px.shape[0], -1), case["pitch_extra"], case["ptr_off"], CANARY)
    buf = DevBuf(engine, data=b.tobytes())
    try:
        with images(engine, _dst_spec(case)) as (dst,):
            rect = case["rect"] or (0, 0, px.shape[1], px.shape[0])
            engine.load_surface(dst.id, buf.ptr + case["ptr_off"], Surface(case["fmt"]), LoadAlpha(case["alpha"]), rect=rect, pitch=pitch)
            got = dst.bits()
        assert np.array_equal(buf.bytes()[:b.size], b), case["name"]  # the surface is only read
    finally:
        buf.free()
    return got


@pytest.mark.parametrize("instance", load_cases.YUV_INSTANCES, ids=lambda i: load_cases.yuv_instance_name(*i))
def test_yuv_battery(engine, instance):
    """Every case of one instantiation of k_load_yuv: the whole of dst is compared, bit for bit -- the rectangle with the reference,
    the texels outside it with what they held (zero for a never-written image).  A failure names the case."""
    cases = load_cases.yuv_cases(instance)
    assert len(cases) > 60
    for c in cases:
        assert_equal_bits(_run_yuv(engine, c), load_cases.yuv_expected(c), c["name"])


@pytest.mark.parametrize("instance", load_cases.SURFACE_INSTANCES, ids=lambda i: load_cases.surface_instance_name(*i))
def test_surface_battery(engine, instance):
    cases = load_cases.surface_cases(instance)
    assert len(cases) > 25
    for c in cases:
        assert_equal_bits(_run_surface(engine, c), load_cases.surface_expected(c), c["name"])


def test_arrays_go_through_the_engines_own_buffers(engine):
    """Engine.load_surface and Engine.load_yuv with host arrays, the planes as blit_yuv returns them, into a rectangle."""
    px = load_cases.random_pixels(21, 9, 40)
    y, cb, cr = load_cases.random_frame(21, 9, 41)
    prior = np.full((13, 30, 4), load_cases.POISON, np.uint16)
    with images(engine, prior, prior) as (a, b):
        engine.load_surface(a.id, px, Surface.BGRA8_SRGB, LoadAlpha.PREMULTIPLIED, rect=(3, 2, 21, 9))
        engine.load_yuv(b.id, (y, np.stack([cb, cr], axis=-1)), YuvLayout.NV12, YuvMatrix.BT601, YuvRange.FULL, YuvTransfer.SRGB, rect=(5, 4, 21, 9))
        got_a, got_b = a.bits(), b.bits()
        engine.load_yuv(b.id, (y, cb, cr), YuvLayout.I420, chroma=ChromaFilter.REPLICATE, rect=(5, 4, 21, 9))
        got_c = b.bits()
    assert_equal_bits(got_a, load_ref.load_surface(prior, px, load_ref.BGRA8_SRGB, load_ref.PREMULTIPLIED, (3, 2, 21, 9)), "load_surface of an array")
    assert_equal_bits(got_b, load_ref.load_yuv(prior, [y, np.stack([cb, cr], axis=-1)], load_ref.NV12, load_ref.BT601, load_ref.FULL, load_ref.SRGB,
                                               load_ref.BILINEAR, (5, 4, 21, 9)), "load_yuv of NV12 arrays")
    assert_equal_bits(got_c, load_ref.load_yuv(prior, [y, cb, cr], load_ref.I420, chroma=load_ref.REPLICATE, rect=(5, 4, 21, 9)), "load_yuv of I420 arrays")
    with pytest.raises(ValueError):
        engine.load_yuv(0, (y, cb), YuvLayout.I420)


def test_an_array_without_a_rectangle_fills_its_own_size_at_the_origin(engine):
    """rect=None with host arrays: the frame's own (0, 0, w, h) goes into the descriptor, never the image's size -- a frame as wide
    as the image with fewer rows (1920 x 1080 into 1920 x 1088, in small) fills its rows and nothing is read behind the upload; a
    frame with more rows or columns than the image is refused and no texel changes."""
    prior = np.full((13, 30, 4), load_cases.POISON, np.uint16)
    for w, h in ((30, 9), (21, 13), (21, 9)):
        px = load_cases.random_pixels(w, h, 45)
        y, cb, cr = load_cases.random_frame(w, h, 46)
        with images(engine, prior, prior) as (a, b):
            engine.load_surface(a.id, px, Surface.RGBA8_UNORM)
            engine.load_yuv(b.id, (y, cb, cr), YuvLayout.I420)
            assert_equal_bits(a.bits(), load_ref.load_surface(prior, px, load_ref.RGBA8_UNORM, rect=(0, 0, w, h)), "load_surface %d x %d" % (w, h))
            assert_equal_bits(b.bits(), load_ref.load_yuv(prior, [y, cb, cr], load_ref.I420, rect=(0, 0, w, h)), "load_yuv %d x %d" % (w, h))
    for w, h in ((30, 14), (31, 13)):
        y, cb, cr = load_cases.random_frame(w, h, 47)
        with images(engine, prior) as (a,):
            with pytest.raises(ValueError, match="jh_load_surface: .*not inside"):
                engine.load_surface(a.id, load_cases.random_pixels(w, h, 48), Surface.RGBA8_UNORM)
            with pytest.raises(ValueError, match="jh_load_yuv: .*not inside"):
                engine.load_yuv(a.id, (y, np.stack([cb, cr], axis=-1)))
            assert np.array_equal(a.bits(), prior)


def test_the_kernels_store_rule_is_the_host_querys(engine):
    """k_load_surface<., PREMULTIPLIED> calls texel_io.h's texel_unpremultiply; jh_load_texel compiles the host copy in
    include/jello_load.h.  Device against library, bit for bit, over every (code, alpha) pair in every channel, both transfers."""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    px = np.stack([c, 255 - c, c ^ 0x5A, a], axis=-1)
    for fmt in (Surface.RGBA8_UNORM, Surface.BGRA8_SRGB):
        with images(engine, (256, 256)) as (img,):
            engine.load_surface(img.id, px, fmt, LoadAlpha.PREMULTIPLIED)
            assert_equal_bits(img.bits(), jello_amd.load_texels(px, fmt=fmt, alpha=LoadAlpha.PREMULTIPLIED), "format %d" % fmt)


def test_load_yuv_is_load_surface_of_its_codes(engine):
    """Device against device, bit for bit: jh_load_yuv = jh_load_surface (OPAQUE) of the reference's R'G'B' codes, both transfers."""
    y, cb, cr = load_cases.random_frame(45, 11, 50)
    for chroma in load_ref.CHROMAS:
        for transfer, fmt in ((load_ref.NONE, Surface.RGBA8_UNORM), (load_ref.SRGB, Surface.RGBA8_SRGB)):
            rgb = load_ref.yuv_codes([y, cb, cr], load_ref.I420, load_ref.BT709, load_ref.LIMITED, chroma).astype(np.uint8)
            px = np.concatenate([rgb, np.full((11, 45, 1), 7, np.uint8)], axis=-1)  # (byte 3 is ignored)
            with images(engine, (45, 11), (45, 11)) as (a, b):
                engine.load_yuv(a.id, (y, cb, cr), YuvLayout.I420, transfer=YuvTransfer(transfer), chroma=ChromaFilter(chroma))
                engine.load_surface(b.id, px, fmt, LoadAlpha.OPAQUE)
                assert_equal_bits(a.bits(), b.bits(), "chroma %d transfer %d" % (chroma, transfer))


def test_an_opaque_surface_round_trips_through_the_blit(engine):
    """jh_blit(jh_load_surface(S)) = S for an opaque S holding every code in every channel, in the four formats (both transfers), under
    the three alpha modes (byte 3 is 255: they agree)."""
    c = np.arange(256, dtype=np.uint8)
    surface = np.stack([np.stack([np.roll(c, 85 * k) for k in range(3)] + [np.full(256, 255, np.uint8)], axis=-1) for _ in range(2)])
    for fmt in Surface:
        for alpha in (LoadAlpha.OPAQUE, LoadAlpha.STRAIGHT, LoadAlpha.PREMULTIPLIED):
            with images(engine, (256, 2)) as (img,):
                engine.load_surface(img.id, surface, fmt, alpha)
                back = engine.blit(img.id, 256, 2, fmt)
            assert np.array_equal(back, surface), (fmt, alpha)


def test_a_loaded_frame_composited_onto_a_rendered_one(engine):
    """A video frame loaded into a layer and laid over a rendered target at an offset, against the composed references."""
    rec, _, _ = engine.render(*scene((64, 48), 3))
    target = rec.target
    plain = target_of(engine, rec)
    y, cb, cr = load_cases.random_frame(31, 17, 60)
    with images(engine, (31, 17)) as (layer,):
        engine.load_yuv(layer.id, (y, cb, cr), YuvLayout.I420, YuvMatrix.BT601, YuvRange.LIMITED, YuvTransfer.SRGB)
        engine.composite(layer.id, target["id"], opacity=0.75, offset=(9, 5))
        got = target_of(engine, rec)
    frame = load_ref.load_yuv((17, 31), [y, cb, cr], load_ref.I420, load_ref.BT601, load_ref.LIMITED, load_ref.SRGB)
    want = composite_ref.composite(frame, plain, opacity=0.75, offset=(9, 5))
    assert_same_bits(got, want, "the loaded frame over the rendered one")
    assert (want != plain).any()


def test_captured_with_the_frame(engine):
    """capture(load_yuv=dict(dst=a second image, ...), composite=dict(src=that image), surface=...): render, the video frame into the
    layer (one more kernel node), the layer over the frame, blit -- replayed twice, the bytes of the eager calls."""
    y, cb, cr = load_cases.random_frame(40, 24, 70)
    planes = load_cases.planes_of(y, cb, cr, load_ref.NV12)
    bufs = [DevBuf(engine, data=p.tobytes()) for p in planes]
    try:
        what = dict(planes=[(b.ptr, p.shape[1]) for b, p in zip(bufs, planes)], layout=YuvLayout.NV12, matrix=YuvMatrix.BT709, range=YuvRange.LIMITED,
                    transfer=YuvTransfer.SRGB, chroma=ChromaFilter.BILINEAR)
        over = dict(opacity=0.5, offset=(11, 7))
        with images(engine, (40, 24)) as (layer,):
            def eager(target, _):
                engine.load_yuv(layer.id, **what)
                engine.composite(layer.id, target, **over)
            frame = load_ref.load_yuv((24, 40), planes, load_ref.NV12, load_ref.BT709, load_ref.LIMITED, load_ref.SRGB, load_ref.BILINEAR)
            captured_with_the_frame(engine, scene((64, 48), 3), eager, lambda _: dict(load_yuv=dict(dst=layer.id, **what), composite=dict(src=layer.id, **over)),
                                    lambda plain: composite_ref.composite(frame, plain, **over), extra_launches=3)
            assert_equal_bits(layer.bits(), frame, "the layer after the replays")
    finally:
        for b in bufs:
            b.free()


def test_captured_load_surface_lays_over_the_frame(engine):
    """capture(load_surface=..., composite=dict(src=dst)): the loaded picture over the rendered frame, two more kernel nodes; a replay
    converts what the surface holds then."""
    px = load_cases.random_pixels(64, 48, 80)
    px[..., 3] //= 2
    buf = DevBuf(engine, data=px.tobytes())
    try:
        what = dict(pixels=buf.ptr, fmt=Surface.RGBA8_UNORM, alpha=LoadAlpha.STRAIGHT, rect=(0, 0, 64, 48))
        with images(engine, (64, 48)) as (layer,):
            def eager(target, _):
                engine.load_surface(layer.id, **what)
                engine.composite(layer.id, target)
            captured_with_the_frame(engine, scene((64, 48), 3), eager, lambda _: dict(load_surface=dict(dst=layer.id, **what), composite=dict(src=layer.id)),
                                    lambda plain: composite_ref.composite(load_ref.load_surface((48, 64), px, load_ref.RGBA8_UNORM), plain), extra_launches=3)
    finally:
        buf.free()


def test_refusals_of_load_surface(engine):
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    with images(engine, canary, (W, H, ImageFormat.RGBA8), 4 * W * H) as (dst, rgba8, src):
        def call(d=None, rect=(0, 0, 0, 0), null=False, **fields):
            desc = CLoadSurfaceDesc(0, 0, src.ptr, 4 * W, *rect)
            if "pitch" not in fields and rect[2]:
                desc.pitch = 4 * rect[2]
            for k, v in fields.items():
                setattr(desc, k, v)
            return hip.jh_load_surface(ctx, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, source=False), **{
            "format 4": (lambda: call(format=4), b"unknown surface format"),
            "format -1": (lambda: call(format=-1), b"unknown surface format"),
            "alpha 3": (lambda: call(alpha=3), b"unknown alpha mode"),
            "alpha -1": (lambda: call(alpha=-1), b"unknown alpha mode"),
            "null src": (lambda: call(src=None), b"null src"),
            "pitch below the row": (lambda: call(pitch=4 * W - 1), b"pitch below 4 * width"),
            "pitch below the rectangle's row": (lambda: call(rect=(2, 2, 8, 4), pitch=31), b"pitch below 4 * width"),
        })
        check_refusals(engine, "jh_load_surface", call, refused, untouched=((dst, canary),),
                       raises=(lambda: engine.load_surface(dst.id, src.ptr, 4, rect=(0, 0, W, H)), lambda: engine.load_surface(dst.id, src.ptr, 0, rect=(8, 0, 9, 4))),
                       accepted=(call, lambda: call(rect=(2, 2, 8, 4), pitch=32), lambda: call(format=3, alpha=2)))


def test_refusals_of_load_yuv(engine):
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    with images(engine, canary, (W, H, ImageFormat.RGBA8), W * H, W * H, W * H) as (dst, rgba8, p0, p1, p2):
        def call(d=None, rect=(0, 0, 0, 0), null=False, planes=None, pitches=None, **fields):
            desc = CLoadYuvDesc(0, 1, 0, 0, 1, 0)
            desc.x, desc.y, desc.width, desc.height = rect
            for i, p in enumerate((p0.ptr, p1.ptr, p2.ptr) if planes is None else planes):
                desc.plane[i] = p
            for i, p in enumerate((W, W, W) if pitches is None else pitches):
                desc.pitch[i] = p
            for k, v in fields.items():
                setattr(desc, k, v)
            return hip.jh_load_yuv(ctx, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, source=False), **{
            "layout 2": (lambda: call(layout=2), b"unknown layout"),
            "layout -1": (lambda: call(layout=-1), b"unknown layout"),
            "matrix 2": (lambda: call(matrix=2), b"unknown matrix"),
            "range 2": (lambda: call(range=2), b"unknown range"),
            "transfer 2": (lambda: call(transfer=2), b"unknown transfer"),
            "chroma 2": (lambda: call(chroma=2), b"unknown chroma filter"),
            "chroma -1": (lambda: call(chroma=-1), b"unknown chroma filter"),
            "null luma plane": (lambda: call(planes=(None, p1.ptr, p2.ptr)), b"null plane"),
            "null chroma plane": (lambda: call(planes=(p0.ptr, None, p2.ptr)), b"null plane"),
            "null third plane of I420": (lambda: call(layout=1, planes=(p0.ptr, p1.ptr, None)), b"null plane"),
            "luma pitch below the row": (lambda: call(pitches=(W - 1, W, W)), b"pitch below the row's bytes"),
            "NV12 chroma pitch below the row": (lambda: call(pitches=(W, W - 1, W)), b"pitch below the row's bytes"),
            "I420 chroma pitch below the row": (lambda: call(layout=1, pitches=(W, W // 2, W // 2 - 1)), b"pitch below the row's bytes"),
        })
        check_refusals(engine, "jh_load_yuv", call, refused, untouched=((dst, canary),),
                       raises=(lambda: engine.load_yuv(dst.id, [(p0.ptr, W), (p1.ptr, W)], layout=2), lambda: engine.load_yuv(dst.id, [(p0.ptr, W), (p1.ptr, W - 1)])),
                       accepted=(call, lambda: call(planes=(p0.ptr, p1.ptr, None)), lambda: call(layout=1, pitches=(W, W // 2, W // 2)),
                                 lambda: call(rect=(3, 1, 7, 5), pitches=(7, 8, 0))))


def test_each_call_is_one_query_of_the_tree(engine):
    px = load_cases.random_pixels(33, 9, 90)
    y, cb, cr = load_cases.random_frame(33, 9, 91)
    with images(engine, (33, 9)) as (img,):
        one_query(engine, "load_surface", lambda: engine.load_surface(img.id, px, Surface.RGBA8_SRGB))
        assert_equal_bits(img.bits(), load_ref.load_surface((9, 33), px, load_ref.RGBA8_SRGB), "after the queries")
        one_query(engine, "load_yuv", lambda: engine.load_yuv(img.id, (y, cb, cr), YuvLayout.I420))
        assert_equal_bits(img.bits(), load_ref.load_yuv((9, 33), [y, cb, cr], load_ref.I420), "after the queries")
