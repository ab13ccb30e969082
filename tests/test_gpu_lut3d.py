"""-m gpu: jh_lut3d against the rule of DESIGN.md 5.23 (tests/lut3d_ref.py) byte for byte -- the battery of tests/lut3d_cases.py, one
test per kernel instantiation -- and the call's frame: a captured frame, its refusals, its profile query, never-written images, baked
chains of colour calls, a .cube text, a loaded frame."""
import ctypes

import numpy as np
import pytest

from jello_amd import ColorSpace, ImageFormat, Surface
from jello_amd import colorfilter as cf
from jello_amd import lut3d
from jello_amd.imagecalls import _lut3d_desc

import color_ref
import load_ref
import lut3d_cases as C
import lut3d_ref
import surface_ref
from devmem import _id, target_of
from image_call import (assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query, scene)

pytestmark = pytest.mark.gpu

VARIANT = {"global": 1, "staged": 2}  # jh_debug_lut3d_variant


@pytest.fixture
def instantiation(engine):
    """set(name): the instantiation the engine's next jh_lut3d calls launch; the launcher's own choice again afterwards."""
    def set_(name):
        assert engine.hip.jh_debug_lut3d_variant(engine.ctx, VARIANT[name]) == 0
    yield set_
    assert engine.hip.jh_debug_lut3d_variant(engine.ctx, 0) == 0


def _random_source(size, seed):
    return C.geometry_source(size, seed)


@pytest.mark.parametrize("inst", C.INSTANTIATIONS)
def test_battery(engine, instantiation, inst):
    """Every case of the battery that names this instantiation: every byte of dst is the reference's (a NaN equal to any NaN), the
    texels outside the rectangle keep their bits, and a source of its own is only read.  The failure names the case."""
    instantiation(inst)
    ran = 0
    for case in C.CASES:
        if case["inst"] != inst:
            continue
        src_bits, lut_bits, prior, rect = C.inputs(case)
        in_place = case.get("in_place", False)
        with images(engine, src_bits, lut_bits, *([] if in_place else [prior])) as made:
            src, lut, dst = made[0], made[1], made[-1] if not in_place else made[0]
            engine.lut3d(src.id, lut.id, None if in_place else dst.id, rect=rect)
            got = dst.bits()
            if not in_place:
                assert np.array_equal(src.bits(), src_bits), case["name"]
            assert np.array_equal(lut.bits(), lut_bits), case["name"]
        assert_same_bits(got, C.expected(case), case["name"])
        ran += 1
    assert ran > 50


@pytest.mark.parametrize("n", (2, 3, 5, 9, 17, 33, 65))
def test_an_identity_table_returns_the_clamped_input(engine, n):
    """On the device: the identity table of an N with N - 1 a power of two returns every finite f16 in [0, 1] bit for bit; -0 becomes
    +0, values outside are clamped, NaN becomes 0; alpha never changes.  The expectation is written out here, not the reference's."""
    bits = C.VALUES
    h = bits[..., :3].view(np.float16).astype(np.float32)
    want = bits.copy()
    want[..., :3] = np.where(np.isnan(h) | (h <= 0), 0, np.where(h >= 1, 0x3C00, bits[..., :3]))
    with images(engine, bits, lut3d.as_image(lut3d.identity(n)), (256, 256)) as (src, lut, dst):
        engine.lut3d(src.id, lut.id, dst.id)
        got = dst.bits()
    assert np.array_equal(got, want)


def test_never_written_images(engine):
    """A never-written source reads as transparent black: the rectangle takes entry (0, 0, 0) and alpha 0; a never-written destination
    is cleared outside the rectangle; a never-written table reads as zeros: colour +0, alpha the source's."""
    n = 5
    lut_bits = C.lut_image("random", n)
    content = _random_source((21, 9), 4)
    zeros = np.zeros_like(content)
    poison = np.full_like(content, C.POISON)
    rect = (3, 2, 11, 5)
    with images(engine, (21, 9), poison, content, (21, 9), (21, 9), lut_bits, (n, n * n), np.array(poison)) as (empty, poisoned, full, fresh, alone, lut, no_lut, out):
        engine.lut3d(empty.id, lut.id, poisoned.id, rect=rect)
        want = lut3d_ref.apply(zeros, lut_bits, rect, poison)
        assert np.array_equal(want[2, 3, :3], lut_bits[0, 0, :3]) and want[2, 3, 3] == 0
        assert np.array_equal(poisoned.bits(), want)
        engine.lut3d(full.id, lut.id, fresh.id, rect=rect)
        want = lut3d_ref.apply(content, lut_bits, rect, None)
        assert np.all(want[0] == 0) and want[2:7, 3:14].any()
        assert np.array_equal(fresh.bits(), want)
        engine.lut3d(alone.id, lut.id, rect=rect)
        assert np.array_equal(alone.bits(), lut3d_ref.apply(zeros, lut_bits, rect, None))
        engine.lut3d(full.id, no_lut.id, out.id, rect=rect)
        want = lut3d_ref.apply(content, C.lut_image("zeros", n), rect, poison)
        assert np.all(want[2:7, 3:14, :3] == 0) and np.array_equal(want[2:7, 3:14, 3], content[2:7, 3:14, 3])
        assert np.array_equal(out.bits(), want)


@pytest.mark.parametrize("n", (4, 18))
def test_the_table_may_be_the_source(engine, n):
    lut_bits = C.lut_image("random", n)
    lut_bits[..., 3] = 0x3800
    with images(engine, lut_bits, (n, n * n)) as (lut, dst):
        engine.lut3d(lut.id, lut.id, dst.id)
        got = dst.bits()
        assert np.array_equal(lut.bits(), lut_bits)
    assert_same_bits(got, lut3d_ref.apply(lut_bits, lut_bits), "the table through itself")


def test_four_quadrant_calls_are_one_call(engine):
    bits = _random_source((37, 23), 9)
    lut_bits = C.lut_image("wild", 9)
    with images(engine, bits, lut_bits, (37, 23), (37, 23)) as (src, lut, whole, parts):
        engine.lut3d(src.id, lut.id, whole.id)
        for rect in ((0, 0, 19, 11), (19, 0, 18, 11), (0, 11, 19, 12), (19, 11, 18, 12)):
            engine.lut3d(src.id, lut.id, parts.id, rect=rect)
        one, four = whole.bits(), parts.bits()
    assert np.array_equal(one, four)
    assert_same_bits(one, lut3d_ref.apply(bits, lut_bits), "one call")


def test_captured_with_the_frame(engine):
    """capture(lut3d=..., surface=...): render, the table on the target in place, blit it -- two launches more than the frame alone
    (the call and the blit: nothing is uploaded, nothing had to run eagerly first), replayed twice, the bytes of the eager calls."""
    lut_bits = lut3d.as_image(lut3d.from_function(9, lambda c: c[..., ::-1] ** 2))
    with images(engine, lut_bits) as (lut,):
        captured_with_the_frame(engine, scene(), lambda target, _: engine.lut3d(target, lut.id), lambda _: dict(lut3d=dict(lut=lut.id)),
                                lambda plain: lut3d_ref.apply(plain, lut_bits, dst_bits=plain), extra_launches=2)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_lut3d: ", no texel of any image and no byte of a
    canary buffer touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    table = canary_bits(2, 4)
    with images(engine, canary, canary, canary_bits(8, 6), (W, H, ImageFormat.RGBA8), table, canary_bits(3, 9), canary_bits(2, 5), canary_bits(3, 4)) \
            as (src, dst, small, rgba8, lut, lut3, tall, wide):
        def call(s=None, d=None, l=None, null=False, rect=None, size=2, flags=0):  # noqa: E741
            desc = _lut3d_desc(size, rect)
            desc.flags = flags
            return hip.jh_lut3d(ctx, src.id if s is None else s, dst.id if d is None else d, lut.id if l is None else l, None if null else ctypes.byref(desc))

        outside_dst = (b"the destination rectangle is ", b"not inside the destination image")
        refused = dict(common_refusals(call, rgba8, rects=(("", "source ", "rect"),)), **{
            "unknown LUT": (lambda: call(l=_id()), b"unknown LUT image id"),
            "LUT not RGBA16F": (lambda: call(l=rgba8.id), b"the LUT is not an RGBA16F image"),
            "rectangle outside the destination only": (lambda: call(d=small.id, rect=(4, 2, 6, 3)), outside_dst),
            "rectangle outside the source only": (lambda: call(s=small.id, rect=(4, 2, 6, 3)), (b"the source rectangle is ", b"not inside the source image")),
            "the whole source does not fit the destination": (lambda: call(d=small.id), outside_dst),
            "size 1": (lambda: call(size=1), b"size outside 2..65"),
            "size 0": (lambda: call(size=0), b"size outside 2..65"),
            "size 66": (lambda: call(size=66), b"size outside 2..65"),
            "flag bit 0": (lambda: call(flags=1), b"unknown flag bits"),
            "flag bit 31": (lambda: call(flags=0x80000000), b"unknown flag bits"),
            "size 3 with the table of 2": (lambda: call(size=3), b"the LUT image is not size x size^2"),
            "size 2 with the table of 3": (lambda: call(l=lut3.id), b"the LUT image is not size x size^2"),
            "a table one row too tall": (lambda: call(l=tall.id), b"the LUT image is not size x size^2"),
            "a table one texel too wide": (lambda: call(l=wide.id), b"the LUT image is not size x size^2"),
            "the LUT is the destination": (lambda: call(s=lut.id, d=lut.id), b"the LUT is the destination"),
        })
        check_refusals(engine, "jh_lut3d", call, refused,
                       untouched=((src, canary), (dst, canary), (small, canary_bits(8, 6)), (lut, table), (lut3, canary_bits(3, 9))),
                       raises=(lambda: engine.lut3d(src.id, lut.id, dst.id, rect=(8, 0, 9, 4)), lambda: engine.lut3d(src.id, _id(), dst.id),
                               lambda: engine.lut3d(src.id, tall.id), lambda: engine.lut3d(lut.id, lut.id)),
                       accepted=(lambda: call(s=small.id), lambda: call(d=src.id), lambda: call(s=lut.id),  # a smaller source, in place, the table as the source
                                 lambda: call(l=lut3.id, size=3)))


def test_the_call_is_one_query_of_the_tree(engine):
    bits = _random_source((48, 33), 2)
    lut_bits = C.lut_image("random", 17)
    with images(engine, bits, lut_bits, (48, 33)) as (src, lut, dst):
        one_query(engine, "lut3d", lambda: engine.lut3d(src.id, lut.id, dst.id))
        got = dst.bits()
    assert_same_bits(got, lut3d_ref.apply(bits, lut_bits), "after the queries")


def _baked_reference(n, steps):
    """The table Engine.bake_lut leaves, by the references: color_ref on the identity image, step by step."""
    table = lut3d_ref.identity(n)
    for kw in steps:
        table = color_ref.apply(table, dst_bits=table, **dict(kw, space=int(kw.get("space", 0))))
    return table


@pytest.mark.parametrize("name", ("sepia", "linear_func", "chain"))
def test_a_baked_chain_is_the_composed_references(engine, name):
    """Engine.bake_lut: the identity table uploaded, the colour calls over it in place -- the table is color_ref's of the identity
    image bit for bit, and an image through it is lut3d_ref's through that table."""
    steps = {"sepia": [cf.sepia(1.0)],
             "linear_func": [dict(funcs=(cf.linear(0.5, 0.25), cf.linear(-1.0, 1.0), cf.linear(0.75, 0.0), None), space=ColorSpace.LINEAR)],
             "chain": [cf.saturate(1.6), cf.contrast(0.8), dict(funcs=(cf.gamma(1.0, 0.8, 0.0),) * 3 + (None,), space=ColorSpace.LINEAR)]}[name]
    n = 17
    bits = _random_source((61, 35), 12)
    with images(engine, (n, n * n), bits, (61, 35)) as (lut, src, dst):
        engine.bake_lut(lut.id, n, steps)
        table = lut.bits()
        engine.lut3d(src.id, lut.id, dst.id)
        got = dst.bits()
    want_table = _baked_reference(n, steps)
    assert np.array_equal(table, want_table)
    assert_same_bits(got, lut3d_ref.apply(bits, want_table), name)


def test_a_baked_matrix_against_the_filter_itself(engine):
    """Device against device: a LINEAR-space matrix without tables, baked into a table of 17 (the vertices i / 16 are exact f16),
    against jh_color_filter applied directly.  The matrix keeps [0, 1]^3 inside [0, 1] (no negative coefficient, every row sums to
    at most 1 with its offset), so the clamp never acts and the filter is one affine map A on the cube.  Tetrahedral interpolation
    of an affine map is exact in the reals: sum w_i A(V_i) = A(x), the weights being exact and summing to 1.  What is left:
      entries   E_i = f16(A(V_i) + d1), off by at most half an f16 ulp below 1, 2^-12, so |sum w_i E_i - A(x)| <= 2^-12 + d1
      the sum   four binary32 roundings of values <= 1: d2 <= 4 x 2^-24
      baked     one rounding to f16: <= 2^-12
      direct    f16(A(x) + d1), d1 <= 4 x 2^-24 x 2 (four fmaf, partial sums below 2): <= 2^-12 + d1
    |baked - direct| <= 3 x 2^-12 + 2^-20.  Alpha is copied by one and kept by the other (alpha in [0, 1], identity row)."""
    matrix = (0.41, 0.23, 0.17, 0.0, 0.05,  # (no dyadic coefficients: the entries do round)
              0.07, 0.61, 0.19, 0.0, 0.02,
              0.21, 0.27, 0.33, 0.0, 0.11,
              0.0, 0.0, 0.0, 1.0, 0.0)
    step = dict(matrix=matrix, space=ColorSpace.LINEAR, clamp=True)
    bound = 3 * 2.0 ** -12 + 2.0 ** -20
    rng = np.random.default_rng(77)
    bits = rng.uniform(0.0, 1.0, (64, 128, 4)).astype(np.float16).view(np.uint16)
    with images(engine, (17, 17 * 17), bits, (128, 64), (128, 64)) as (lut, src, baked, direct):
        engine.bake_lut(lut.id, 17, [step])
        engine.lut3d(src.id, lut.id, baked.id)
        engine.color_filter(src.id, direct.id, **step)
        a, b = baked.bits(), direct.bits()
    assert np.array_equal(a[..., 3], bits[..., 3]) and np.array_equal(b[..., 3], bits[..., 3])
    worst = float(np.abs(a[..., :3].view(np.float16).astype(np.float64) - b[..., :3].view(np.float16).astype(np.float64)).max())
    print("baked matrix against the filter: worst difference %.3g = %.1f %% of the bound %.3g" % (worst, 100 * worst / bound, bound))
    assert worst <= bound


CUBE = """# a grade written by hand: red and blue swapped, green squared
TITLE "swap"
LUT_3D_SIZE 3

DOMAIN_MIN 0.0 0.0 0.0
DOMAIN_MAX 1.0 1.0 1.0
""" + "\n".join("%g %g %g" % (b / 2, (g / 2) ** 2, r / 2) for b in range(3) for g in range(3) for r in range(3)) + "\n"


def test_a_rendered_scene_through_a_cube_text(engine):
    table = lut3d.from_cube(CUBE)
    lut_bits = lut3d.as_image(table)
    rec, _, _ = engine.render(*scene())
    plain = target_of(engine, rec)
    assert plain.any()
    with images(engine, lut_bits) as (lut,):
        engine.lut3d(rec.target["id"], lut.id)
        got = target_of(engine, rec)
    assert_same_bits(got, lut3d_ref.apply(plain, lut_bits, dst_bits=plain), "the scene through the .cube")
    inside, before = got[44, 50].view(np.float16), plain[44, 50].view(np.float16)
    assert inside[0] == before[2] and inside[2] == before[0] and inside[3] == before[3] == 1.0  # red and blue swapped (exact: a linear table), opaque


def test_a_loaded_frame_through_a_table_to_a_surface(engine):
    """load_surface -> lut3d -> blit: an 8-bit picture in, graded on the device, an 8-bit picture out."""
    rng = np.random.default_rng(31)
    px = rng.integers(0, 256, (19, 45, 4), dtype=np.uint8)
    lut_bits = lut3d.as_image(lut3d.from_function(33, lambda c: np.clip(1.1 * c ** 1.2 - 0.02, 0.0, 1.0)))
    with images(engine, (45, 19), lut_bits) as (img, lut):
        engine.load_surface(img.id, px, Surface.RGBA8_SRGB)
        engine.lut3d(img.id, lut.id)
        got = engine.blit(img.id, 45, 19, Surface.RGBA8_SRGB)
        texels = img.bits()
    want = lut3d_ref.apply(load_ref.load_surface((19, 45), px, load_ref.RGBA8_SRGB), lut_bits)
    assert_same_bits(texels, want, "the graded frame")
    assert np.array_equal(got, surface_ref.convert(want, int(Surface.RGBA8_SRGB)))
