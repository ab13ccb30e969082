"""-m gpu: jh_convolve against the rule of DESIGN.md 5.13 (tests/convolve_ref.py) byte for byte -- the battery of
tests/convolve_cases.py (every instantiation of the kernel), never-written images, a rendered frame sharpened, from_svg against the
specification's formula, a captured frame -- and the call's frame: its refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

from jello_amd import ConvolveEdge, ConvolveMode, ImageFormat, convolution
from jello_amd._lib import CConvolveDesc

import convolve_cases
import convolve_ref
from devmem import target_of
from image_call import (assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query,
                        run_case, scene)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in convolve_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.convolve: dst is poisoned first (or never written), the whole of dst is compared -- the rectangle
    with the reference, the texels outside it with what they held (a never-written dst: transparent black)."""
    c = convolve_cases.BY_NAME[name]
    call = lambda src, dst: engine.convolve(src.id, dst.id, convolve_cases.weights(c), target=c["target"], edge=ConvolveEdge(c["edge"]),  # noqa: E731
                                            mode=ConvolveMode(c["mode"]), bias=c["bias"], rect=c["rect"])
    got = run_case(engine, c, call, convolve_cases.source(c), convolve_cases.before(c), dst_size=c["size"])
    assert_same_bits(got, convolve_cases.expected(name), name)


def test_a_never_written_source_and_a_never_written_destination(engine):
    """A never-written source gives transparent black inside the rectangle under PREMULTIPLIED and PRESERVE_ALPHA, the bias under
    STRAIGHT, and leaves the rest of dst alone; a never-written destination is cleared around the rectangle."""
    bits = convolve_cases.content("unit", 25, 20, seed=4)
    w = convolve_cases.kernel((5, 5), 8)
    with images(engine, (40, 30), np.full((30, 40, 4), convolve_cases.POISON, np.uint16), bits, (25, 20)) as (src, dst, real, fresh):
        engine.convolve(src.id, dst.id, w, edge=ConvolveEdge.REPEAT, rect=(1, 1, 11, 9))
        engine.convolve(src.id, dst.id, w, edge=ConvolveEdge.MIRROR, mode=ConvolveMode.PRESERVE_ALPHA, rect=(13, 10, 12, 10))
        engine.convolve(src.id, dst.id, w, edge=ConvolveEdge.ZERO, mode=ConvolveMode.STRAIGHT, bias=0.5, rect=(30, 1, 7, 5))
        got = dst.bits()
        engine.convolve(real.id, fresh.id, w, edge=ConvolveEdge.CLAMP, rect=(5, 3, 7, 9))
        cleared = fresh.bits()
    want = np.full((30, 40, 4), convolve_cases.POISON, np.uint16)
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    want[1:6, 30:37] = 0x3800
    assert np.array_equal(got, want)
    assert convolve_ref.same_bits(cleared, convolve_ref.convolve(bits, w, None, convolve_ref.CLAMP, rect=(5, 3, 7, 9)))


@pytest.mark.parametrize("kernel", ["sharpen", "box", "emboss", "sobel_x", "laplacian8"])
def test_rendered_scene(engine, kernel):
    """A rendered 128 x 128 frame (a circle and a stroked curve, translucent edges) under the named kernels = the reference on the
    download of the same render; the frame itself is untouched."""
    k = {"sharpen": convolution.sharpen(1.5), "box": convolution.box(7), "emboss": convolution.emboss(), "sobel_x": convolution.sobel_x(),
         "laplacian8": convolution.laplacian(True)}[kernel]
    rec, _, _ = engine.render(*scene())
    plain = target_of(engine, rec)
    assert plain.any()
    with images(engine, (128, 128)) as (dst,):
        engine.convolve(rec.target["id"], dst.id, **k)
        got = dst.bits()
    assert_same_bits(got, convolve_ref.convolve(plain, k["weights"], k["target"], int(k["edge"]), int(k["mode"]), k["bias"]), kernel)
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
    with images(engine, img.astype(np.float16).view(np.uint16), (W, H)) as (src, dst):
        engine.convolve(src.id, dst.id, **k)
        got_bits = dst.bits()

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
    alone (no scratch, no tables), replayed twice, the bytes of the eager calls."""
    k = convolution.sharpen(1.0)
    captured_with_the_frame(engine, scene(), lambda target, dst: engine.convolve(target, dst, **k), lambda dst: dict(convolve=dict(dst=dst, **k)),
                            lambda plain: convolve_ref.convolve(plain, k["weights"], None, int(k["edge"]), int(k["mode"]), k["bias"]),
                            extra_launches=1, out_size=(128, 128), baseline_surface=True)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_convolve: ", no texel of either image and no byte
    of a canary buffer touched; a valid call works afterwards."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)

    def weights_with(at, value):
        w = [0.5] * 225
        w[at] = value
        return w

    with images(engine, canary, canary, (W, H, ImageFormat.RGBA8), (W + 1, H)) as (src, dst, rgba8, other):
        def call(s=None, d=None, head=(3, 3, 1, 1, 1, 0, 0.0), rect=(0, 0, 0, 0), weights=None, null=False):
            desc = CConvolveDesc(*head, *rect)
            w = [0.0] * 4 + [1.0] + [0.0] * 220 if weights is None else weights
            desc.weights[:len(w)] = w
            return hip.jh_convolve(ctx, src.id if s is None else s, dst.id if d is None else d, None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8), **{
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
        })
        check_refusals(engine, "jh_convolve", call, refused, untouched=((src, canary), (dst, canary)),
                       raises=(lambda: engine.convolve(src.id, src.id, np.ones((3, 3), np.float32)),
                               lambda: engine.convolve(src.id, dst.id, np.ones((3, 3), np.float32), target=(3, 0)),
                               lambda: engine.convolve(src.id, dst.id, np.full((2, 2), np.inf, np.float32)),
                               lambda: engine.convolve(src.id, dst.id, np.ones(9, np.float32), order=(4, 2))),
                       accepted=(lambda: call(weights=weights_with(9, math.nan)),  # (a weight beyond the ones that are read is not looked at)
                                 lambda: call(head=(3, 3, 1, 1, 1, 1, 0.0))))      # (the plain call, STRAIGHT: the kernel is the identity)
        assert np.array_equal(dst.bits(), canary) and np.array_equal(src.bits(), canary)
        with images(engine, (0, 5), (0, 5)) as (empty_a, empty_b):
            assert hip.jh_convolve(ctx, empty_a.id, empty_b.id, ctypes.byref(CConvolveDesc(1, 1, 0, 0, 1, 0, 0.0, 0, 0, 0, 0))) == 0  # (an image without texels)


def test_the_call_is_one_query_of_the_tree(engine):
    bits = convolve_cases.content("unit", 48, 33, seed=2)
    k = convolution.box(5)
    with images(engine, bits, (48, 33)) as (src, dst):
        one_query(engine, "convolve", lambda: engine.convolve(src.id, dst.id, **k))
        got = dst.bits()
    assert convolve_ref.same_bits(got, convolve_ref.convolve(bits, k["weights"], None, convolve_ref.CLAMP))
