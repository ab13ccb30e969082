"""-m gpu: jh_convolve against the rule of DESIGN.md 5.13 (tests/convolve_ref.py) byte for byte -- the battery of
tests/convolve_cases.py (every instantiation of the kernel), never-written images, a rendered frame sharpened, from_svg against the
specification's formula, a captured frame -- and the call's frame: its refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, ConvolveEdge, ConvolveMode, Fill, ImageFormat, Join, Path, RenderParams, Scene, Stroke, Surface, convolution
from jello_amd._lib import CConvolveDesc
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS

import convolve_cases
import convolve_ref
import surface_ref
from devmem import CANARY, DevBuf, Image, _id, target_of

pytestmark = pytest.mark.gpu


def _differences(name, got, want):
    bad = np.argwhere(got != want)
    return "%s: %d of %d values differ, first at (y, x, ch) = %s: got %#06x, want %#06x" % (
        name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", [c["name"] for c in convolve_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.convolve: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = convolve_cases.BY_NAME[name]
    src_bits, prior = convolve_cases.source(c), convolve_cases.before(c)
    src = Image(engine, None, *c["size"]) if c["kind"] == "never" else Image(engine, src_bits)
    dst = Image(engine, None, *c["size"]) if prior is None else Image(engine, prior)
    try:
        engine.convolve(src.id, dst.id, convolve_cases.weights(c), target=c["target"], edge=ConvolveEdge(c["edge"]), mode=ConvolveMode(c["mode"]),
                        bias=c["bias"], rect=c["rect"])
        got = dst.bits()
        if c["kind"] != "never":  # (a never-written image reads as zero; its memory holds anything)
            assert np.array_equal(src.bits(), src_bits)  # the source is only read
    finally:
        src.free()
        dst.free()
    want = convolve_cases.expected(name)
    if not convolve_ref.same_bits(got, want):
        pytest.fail(_differences(name, got, want))


def test_a_never_written_source_and_a_never_written_destination(engine):
    """A never-written source gives transparent black inside the rectangle under PREMULTIPLIED and PRESERVE_ALPHA, the bias under
    STRAIGHT, and leaves the rest of dst alone; a never-written destination is cleared around the rectangle."""
    src, dst = Image(engine, None, 40, 30), Image(engine, np.full((30, 40, 4), convolve_cases.POISON, np.uint16))
    bits = convolve_cases.content("unit", 25, 20, seed=4)
    real, fresh = Image(engine, bits), Image(engine, None, 25, 20)
    w = convolve_cases.kernel((5, 5), 8)
    try:
        engine.convolve(src.id, dst.id, w, edge=ConvolveEdge.REPEAT, rect=(1, 1, 11, 9))
        engine.convolve(src.id, dst.id, w, edge=ConvolveEdge.MIRROR, mode=ConvolveMode.PRESERVE_ALPHA, rect=(13, 10, 12, 10))
        engine.convolve(src.id, dst.id, w, edge=ConvolveEdge.ZERO, mode=ConvolveMode.STRAIGHT, bias=0.5, rect=(30, 1, 7, 5))
        got = dst.bits()
        engine.convolve(real.id, fresh.id, w, edge=ConvolveEdge.CLAMP, rect=(5, 3, 7, 9))
        cleared = fresh.bits()
    finally:
        for im in (src, dst, real, fresh):
            im.free()
    want = np.full((30, 40, 4), convolve_cases.POISON, np.uint16)
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    want[1:6, 30:37] = 0x3800
    assert np.array_equal(got, want)
    assert convolve_ref.same_bits(cleared, convolve_ref.convolve(bits, w, None, convolve_ref.CLAMP, rect=(5, 3, 7, 9)))


def _scene():
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid((0.9, 0.4, 0.1, 1.0)), None, Path.circle(50, 44, 30))
    curve = Path().move_to(10, 100).cubic_to(40, 4, 90, 120, 120, 16)
    s.stroke(Stroke(5, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None, curve)
    return s, RenderParams(128, 128)


@pytest.mark.parametrize("kernel", ["sharpen", "box", "emboss", "sobel_x", "laplacian8"])
def test_rendered_scene(engine, kernel):
    """A rendered 128 x 128 frame (a circle and a stroked curve, translucent edges) under the named kernels = the reference on the
    download of the same render; the frame itself is untouched."""
    k = {"sharpen": convolution.sharpen(1.5), "box": convolution.box(7), "emboss": convolution.emboss(), "sobel_x": convolution.sobel_x(),
         "laplacian8": convolution.laplacian(True)}[kernel]
    s, p = _scene()
    rec, _, _ = engine.render(s, p)
    plain = target_of(engine, rec)
    assert plain.any()
    dst = Image(engine, None, 128, 128)
    try:
        engine.convolve(rec.target["id"], dst.id, **k)
        got = dst.bits()
    finally:
        dst.free()
    want = convolve_ref.convolve(plain, k["weights"], k["target"], int(k["edge"]), int(k["mode"]), k["bias"])
    assert convolve_ref.same_bits(got, want), _differences(kernel, got, want)
    assert not np.array_equal(got, plain)
    assert np.array_equal(target_of(engine, rec), plain)


@pytest.mark.parametrize("edge_mode", ["none", "duplicate", "wrap"])
def test_from_svg_is_the_specifications_formula(engine, edge_mode):
    """feConvolveMatrix: RESULT(X, Y) = sum over I, J of SOURCE(X - targetX + J, Y - targetY + I) kernelMatrix(orderX - J - 1, orderY - I -
    1) / divisor + bias ALPHA(X, Y), with preserveAlpha, an asymmetric kernel of small integers, a divisor that is a power of two and
    an integer-valued opaque image: every product, sum and quotient is exact in binary32 and in f16, so float64 numpy gives the
    device's values exactly -- which proves the flip, the target and the edge modes."""
    order, target = (4, 3), (1, 2)
    km = [1, -2, 3, 0, 5, 6, -7, 8, 0, 10, 11, -12]
    rng = np.random.default_rng(5)
    img = rng.integers(-6, 7, (17, 23, 4)).astype(np.float64)
    img[..., 3] = 1.0
    H, W, _ = img.shape
    k = convolution.from_svg(order, km, divisor=4, bias=0.5, target=target, edge_mode=edge_mode, preserve_alpha=True)
    src, dst = Image(engine, img.astype(np.float16).view(np.uint16)), Image(engine, None, W, H)
    try:
        engine.convolve(src.id, dst.id, **k)
        got_bits = dst.bits()
    finally:
        src.free()
        dst.free()

    def source(x, y):  # SOURCE under the edge mode
        if edge_mode == "none":
            return img[y, x] if 0 <= x < W and 0 <= y < H else np.zeros(4)
        if edge_mode == "duplicate":
            return img[min(max(y, 0), H - 1), min(max(x, 0), W - 1)]
        return img[y % H, x % W]

    want = np.zeros_like(img)
    for Y in range(H):
        for X in range(W):
            acc = np.zeros(4)
            for I in range(order[1]):
                for J in range(order[0]):
                    acc += source(X - target[0] + J, Y - target[1] + I) * km[(order[1] - I - 1) * order[0] + (order[0] - J - 1)]
            want[Y, X] = np.append(acc[:3] / 4.0 + 0.5 * img[Y, X, 3], img[Y, X, 3])
    assert np.array_equal(got_bits.view(np.float16).astype(np.float64), want)
    assert np.array_equal(want.astype(np.float16).astype(np.float64), want) and len(np.unique(want)) > 100
    ref = convolve_ref.convolve(img.astype(np.float16).view(np.uint16), k["weights"], target, int(k["edge"]), int(k["mode"]), 0.5)
    assert np.array_equal(got_bits, ref)


def test_captured_with_the_frame(engine):
    """capture(convolve=..., surface=...): render, sharpen into a second image, blit that image -- one launch more than with the blit
    alone, replayed twice, the bytes of the eager calls."""
    s, p = _scene()
    fmt = Surface.RGBA8_SRGB
    k = convolution.sharpen(1.0)
    rec = jello_amd.Host().record(s, p)
    sharp, surf, full = Image(engine, None, 128, 128), DevBuf(engine, 128 * 128 * 4), DevBuf(engine, 128 * 128 * 4)
    g = None
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        t = rec.target
        plain = target_of(engine, rec)
        engine.convolve(t["id"], sharp.id, **k)
        engine.blit(sharp.id, 128, 128, fmt, out_device_ptr=surf.ptr)
        eager = surf.bytes()[:128 * 128 * 4].reshape(128, 128, 4)
        want = convolve_ref.convolve(plain, k["weights"], None, int(k["edge"]), int(k["mode"]), k["bias"])
        assert convolve_ref.same_bits(sharp.bits(), want)
        assert np.array_equal(eager, surface_ref.convert(want, int(fmt)))
        g0 = engine.capture(rec, surface=(full.ptr, 128 * 4, fmt))  # (the frame and the blit of its own target)
        g = engine.capture(rec, convolve=dict(dst=sharp.id, **k), surface=(surf.ptr, 128 * 4, fmt))
        (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
        engine.graph_destroy(g0)
        assert (k1, o1) == (k0 + 1, o0)  # one launch, no scratch, no tables
        for _ in range(2):
            engine.clear(surf.id)
            engine.replay(g)
            engine.sync()
            assert np.array_equal(surf.bytes()[:128 * 128 * 4].reshape(128, 128, 4), eager)
        assert np.array_equal(target_of(engine, rec), plain)
    finally:
        if g is not None:
            engine.graph_destroy(g)
        sharp.free()
        surf.free()
        full.free()


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_convolve: ", no texel of either image and no byte
    of a canary buffer touched; a valid call works afterwards."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = np.full((H, W, 4), CANARY | (CANARY << 8), np.uint16)
    src, dst = Image(engine, canary), Image(engine, canary)
    rgba8 = Image(engine, np.full((H, W, 2), 0x1111, np.uint16), fmt=ImageFormat.RGBA8)  # (W x H texels of 4 bytes)
    other = Image(engine, None, W + 1, H)
    guard = DevBuf(engine, 256)

    def call(s=None, d=None, head=(3, 3, 1, 1, 1, 0, 0.0), rect=(0, 0, 0, 0), weights=None, null=False):
        desc = CConvolveDesc(*head, *rect)
        w = [0.0] * 4 + [1.0] + [0.0] * 220 if weights is None else weights
        desc.weights[:len(w)] = w
        return hip.jh_convolve(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

    def weights_with(at, value):
        w = [0.5] * 225
        w[at] = value
        return w

    refused = {
        "null descriptor": (lambda: call(null=True), b""),
        "unknown source": (lambda: call(s=_id()), b"unknown source"),
        "unknown destination": (lambda: call(d=_id()), b"unknown destination"),
        "source not RGBA16F": (lambda: call(s=rgba8.id), b"RGBA16F"),
        "destination not RGBA16F": (lambda: call(d=rgba8.id), b"RGBA16F"),
        "images of different size": (lambda: call(d=other.id), b"size"),
        "source is the destination": (lambda: call(d=src.id), b"source is the destination"),
        "order_x 0": (lambda: call(head=(0, 3, 0, 1, 1, 0, 0.0)), b"order"),
        "order_y 0": (lambda: call(head=(3, 0, 1, 0, 1, 0, 0.0)), b"order"),
        "order_x 16": (lambda: call(head=(16, 3, 1, 1, 1, 0, 0.0)), b"order"),
        "order_y 16": (lambda: call(head=(3, 16, 1, 1, 1, 0, 0.0)), b"order"),
        "order 2^32 - 1": (lambda: call(head=(0xFFFFFFFF, 0xFFFFFFFF, 1, 1, 1, 0, 0.0)), b"order"),
        "target_x at the order": (lambda: call(head=(3, 3, 3, 1, 1, 0, 0.0)), b"target"),
        "target_y at the order": (lambda: call(head=(3, 3, 1, 3, 1, 0, 0.0)), b"target"),
        "target 2^32 - 1": (lambda: call(head=(3, 3, 0xFFFFFFFF, 1, 1, 0, 0.0)), b"target"),
        "edge 4": (lambda: call(head=(3, 3, 1, 1, 4, 0, 0.0)), b"edge"),
        "edge -1": (lambda: call(head=(3, 3, 1, 1, -1, 0, 0.0)), b"edge"),
        "mode 3": (lambda: call(head=(3, 3, 1, 1, 1, 3, 0.0)), b"mode"),
        "mode -1": (lambda: call(head=(3, 3, 1, 1, 1, -1, 0.0)), b"mode"),
        "a NaN weight": (lambda: call(weights=weights_with(0, math.nan)), b"weight"),
        "an infinite last weight": (lambda: call(weights=weights_with(8, math.inf)), b"weight"),
        "an infinite weight of 15 x 15": (lambda: call(head=(15, 15, 7, 7, 1, 0, 0.0), weights=weights_with(224, -math.inf)), b"weight"),
        "a NaN bias": (lambda: call(head=(3, 3, 1, 1, 1, 0, math.nan)), b"bias"),
        "an infinite bias": (lambda: call(head=(3, 3, 1, 1, 1, 0, math.inf)), b"bias"),
        "rectangle beyond the right edge": (lambda: call(rect=(8, 0, 9, 4)), b"rectangle is not inside"),
        "rectangle beyond the bottom edge": (lambda: call(rect=(0, 9, 4, 4)), b"rectangle is not inside"),
        "rectangle whose end wraps": (lambda: call(rect=(0xFFFFFFFF, 0, 2, 2)), b"rectangle is not inside"),
        "rectangle empty in x only": (lambda: call(rect=(2, 2, 0, 4)), b"empty in one dimension"),
        "rectangle empty in y only": (lambda: call(rect=(2, 2, 4, 0)), b"empty in one dimension"),
    }
    try:
        for what, (f, word) in refused.items():
            assert f() == JH_ERR_INVALID, what
            msg = hip.jh_last_error(ctx)
            assert msg.startswith(b"jh_convolve: ") and word in msg, (what, msg)
        engine.set_band(0, 1)
        try:
            assert call() == JH_ERR_INVALID
            assert hip.jh_last_error(ctx).startswith(b"jh_convolve: ") and b"band" in hip.jh_last_error(ctx)
        finally:
            engine.set_band()
        with pytest.raises(ValueError, match="jh_convolve: "):
            engine.convolve(src.id, src.id, np.ones((3, 3), np.float32))
        with pytest.raises(ValueError, match="jh_convolve: "):
            engine.convolve(src.id, dst.id, np.ones((3, 3), np.float32), target=(3, 0))
        with pytest.raises(ValueError, match="jh_convolve: "):
            engine.convolve(src.id, dst.id, np.full((2, 2), np.inf, np.float32))
        with pytest.raises(ValueError, match="jh_convolve: "):
            engine.convolve(src.id, dst.id, np.ones(9, np.float32), order=(4, 2))
        assert np.array_equal(src.bits(), canary) and np.array_equal(dst.bits(), canary)
        assert np.all(guard.bytes() == CANARY)
        assert call(weights=weights_with(9, math.nan)) == 0  # (a weight beyond the ones that are read is not looked at)
        assert call(head=(3, 3, 1, 1, 1, 1, 0.0)) == 0       # (the plain call, STRAIGHT: the kernel is the identity)
        assert np.array_equal(dst.bits(), canary) and np.array_equal(src.bits(), canary)
        assert np.all(guard.bytes() == CANARY)
        empty_a, empty_b = Image(engine, None, 0, 5), Image(engine, None, 0, 5)
        try:
            assert hip.jh_convolve(ctx, empty_a.id, empty_b.id, ctypes.byref(CConvolveDesc(1, 1, 0, 0, 1, 0, 0.0, 0, 0, 0, 0))) == 0  # (an image without texels)
        finally:
            empty_a.free()
            empty_b.free()
    finally:
        for im in (src, dst, rgba8, other, guard):
            im.free()


def test_the_call_is_one_query_of_the_tree(engine):
    bits = convolve_cases.content("unit", 48, 33, seed=2)
    k = convolution.box(5)
    src, dst = Image(engine, bits), Image(engine, None, 48, 33)
    try:
        engine.profile(True)
        try:
            with engine.profile_group("post"):
                engine.convolve(src.id, dst.id, **k)
            tree = engine.profile_collect_tree()
            engine.convolve(src.id, dst.id, **k)
            flat = engine.profile_collect()
        finally:
            engine.profile(False)
        got = dst.bits()
    finally:
        src.free()
        dst.free()
    assert [(n["kind"], n["label"], n["parent"], n["stage"]) for n in tree] == [("group", "post", -1, -1), ("query", "convolve", 0, -1)]
    assert tree[1]["gpu_end_ms"] >= tree[1]["gpu_start_ms"]
    assert flat == []
    assert convolve_ref.same_bits(got, convolve_ref.convolve(bits, k["weights"], None, convolve_ref.CLAMP))
