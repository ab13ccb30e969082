"""-m gpu: jh_displace against the rule of DESIGN.md 5.17 (tests/displace_ref.py) byte for byte -- the battery of
tests/displace_cases.py (every instantiation of the kernel; the map a third image, the destination, the source, or never written), the
call against jh_warp on the device where the rule says they agree, a call in quadrants, never-written images, Engine.distort on a
rendered frame against the composed references, captured frames -- and the call's frame: its refusals, its profile query."""
import ctypes
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import DisplaceChannel, ImageFormat, ResampleFilter, TurbulenceKind, WarpEdge, WarpFilter
from jello_amd._lib import CDisplaceDesc

import displace_cases
import displace_ref
import turbulence_ref
import warp_cases
from devmem import _id, target_of
from image_call import (assert_same_bits, canary_bits, captured_with_the_frame, check_refusals, common_refusals, images, one_query, scene)

pytestmark = pytest.mark.gpu

IDENT = displace_ref.IDENTITY
QUADRANTS = ((0, 0, 25, 17), (25, 0, 26, 17), (0, 17, 25, 18), (25, 17, 26, 18))


@pytest.mark.parametrize("name", [c["name"] for c in displace_cases.CASES])
def test_battery(engine, name):
    """Every case through Engine.displace: dst holds POISON first (or the map, where the map is dst; or was never written), the whole
    of dst is compared -- the rectangle with the reference, the texels outside it with what they held -- and the source and a map of
    its own still hold their bits."""
    c = displace_cases.BY_NAME[name]
    src_bits, map_bits, prior = displace_cases.source(c), displace_cases.the_map(c), displace_cases.before(c)
    never = c["kind"] == "never"  # (a never-written image reads as zero; its memory holds anything)
    specs = [c["src_size"] if never else src_bits, c["dst_size"] if prior is None else prior]
    if c["map_is"] in ("own", "never"):
        specs.append(c["dst_size"] if map_bits is None else map_bits)
    with images(engine, *specs) as made:
        src, dst = made[0], made[1]
        dmap = {"own": made[-1], "never": made[-1], "dst": dst, "src": src}[c["map_is"]]
        engine.displace(src.id, dmap.id, dst.id, c["scale"], DisplaceChannel(c["channels"][0]), DisplaceChannel(c["channels"][1]), c["matrix"],
                        WarpFilter(c["filter"]), WarpEdge(c["edge"]), c["src_rect"], c["dst_rect"], premultiplied=not c["flags"])
        got = dst.bits()
        if not never:
            assert np.array_equal(src.bits(), src_bits)  # the source is only read
        if c["map_is"] == "own":
            assert np.array_equal(dmap.bits(), map_bits)  # and so is the map
    assert_same_bits(got, displace_cases.expected(name), name)


def test_the_battery_runs_every_instantiation():
    assert len({c["inst"] for c in displace_cases.CASES}) == 24


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_scale_zero_and_a_half_map_are_the_warp_on_the_device(engine, filt):
    """What the rule says of the two calls, held on the device: the bits of Engine.warp, whatever the map holds under scale 0 and
    whatever the scale under a map of 0.5."""
    bits = warp_cases.content("unit", 45, 37, seed=3)
    m = warp_cases.rotate(30, (45, 37), (51, 35), 1.2)
    any_map = displace_cases.map_bits("values", 51, 35, 1)
    half = np.full((35, 51, 4), 0x3800, np.uint16)
    with images(engine, bits, any_map, half, (51, 35), (51, 35)) as (src, noise, flat, warped, out):
        for edge in WarpEdge:
            for premultiplied in (True, False):
                kw = dict(filter=filt, edge=edge, premultiplied=premultiplied)
                engine.warp(src.id, warped.id, m, **kw)
                want = warped.bits()
                for dmap, scale, channels in ((noise, 0.0, (0, 1)), (noise, (-0.0, 0.0), (3, 3)), (flat, (1e30, -313.7), (2, 0))):
                    engine.upload_image(out.id, np.full((35, 51, 4), warp_cases.POISON, np.uint16))
                    engine.displace(src.id, dmap.id, out.id, scale, *channels, matrix=m, **kw)
                    assert np.array_equal(out.bits(), want), (edge, premultiplied, scale)


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_four_quadrants_are_the_whole_image(engine, filt):
    """... with a map of its own, and with the map being the destination: a quadrant reads only the map texels it overwrites."""
    bits = warp_cases.content("unit", 45, 37, seed=3)
    dmap_bits = displace_cases.map_bits("random", 51, 35, 4)
    m = warp_cases.rotate(30, (45, 37), (51, 35), 1.2)
    kw = dict(matrix=m, filter=filt, edge=WarpEdge.MIRROR)
    with images(engine, bits, dmap_bits, (51, 35), (51, 35), dmap_bits) as (src, dmap, whole, parts, inplace):
        engine.displace(src.id, dmap.id, whole.id, (6.0, -4.0), **kw)
        for rect in QUADRANTS:
            engine.displace(src.id, dmap.id, parts.id, (6.0, -4.0), dst_rect=rect, **kw)
            engine.displace(src.id, inplace.id, inplace.id, (6.0, -4.0), dst_rect=rect, **kw)
        a, b, c = whole.bits(), parts.bits(), inplace.bits()
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert displace_ref.same_bits(a, displace_ref.displace(bits, dmap_bits, (35, 51), (6.0, -4.0), matrix=m, filt=int(filt), edge=displace_ref.MIRROR))


def test_never_written_source_map_and_destination(engine):
    """A never-written source gives transparent black inside the rectangle under every edge mode and leaves the rest of dst alone; a
    never-written map reads 0 in every channel (t = -0.5); a never-written destination is cleared around the rectangle -- also when it
    is the map, which then reads 0 too."""
    bits = warp_cases.content("unit", 25, 20, seed=4)
    dmap_bits = displace_cases.map_bits("random", 25, 20, 5)
    poison = np.full((20, 25, 4), warp_cases.POISON, np.uint16)
    with images(engine, (40, 30), poison, dmap_bits, bits, (25, 20), (25, 20), (25, 20), (25, 20)) as (empty, dst, dmap, real, nomap, fresh, fresh2, both):
        for edge, premultiplied, rect in ((WarpEdge.REPEAT, True, (1, 1, 11, 9)), (WarpEdge.CLAMP, False, (13, 10, 12, 10))):
            engine.displace(empty.id, dmap.id, dst.id, 9.0, matrix=warp_cases.rotate(45, (40, 30), (25, 20)), filter=WarpFilter.BICUBIC, edge=edge, dst_rect=rect,
                            premultiplied=premultiplied)
        got = dst.bits()
        engine.displace(real.id, nomap.id, fresh.id, (8.0, -6.0), filter=WarpFilter.BILINEAR, edge=WarpEdge.CLAMP, dst_rect=(5, 3, 7, 9))
        cleared = fresh.bits()
        engine.displace(real.id, dmap.id, fresh2.id, (8.0, -6.0), filter=WarpFilter.BICUBIC, edge=WarpEdge.MIRROR, dst_rect=(2, 1, 20, 17))
        with_map = fresh2.bits()
        engine.displace(real.id, both.id, both.id, (8.0, -6.0), filter=WarpFilter.NEAREST, edge=WarpEdge.REPEAT, dst_rect=(5, 3, 7, 9))
        in_place = both.bits()
    want = poison.copy()
    want[1:10, 1:12] = 0
    want[10:20, 13:25] = 0
    assert np.array_equal(got, want)
    assert displace_ref.same_bits(cleared, displace_ref.displace(bits, None, (20, 25), (8.0, -6.0), filt=displace_ref.BILINEAR, edge=displace_ref.CLAMP,
                                                                 dst_rect=(5, 3, 7, 9)))
    assert displace_ref.same_bits(with_map, displace_ref.displace(bits, dmap_bits, (20, 25), (8.0, -6.0), filt=displace_ref.BICUBIC, edge=displace_ref.MIRROR,
                                                                  dst_rect=(2, 1, 20, 17)))
    assert not with_map[0].any() and not with_map[:, :2].any() and with_map[1:18, 2:22].any()
    assert displace_ref.same_bits(in_place, displace_ref.displace(bits, None, (20, 25), (8.0, -6.0), filt=displace_ref.NEAREST, edge=displace_ref.REPEAT,
                                                                  dst_rect=(5, 3, 7, 9)))


NOISE = dict(base_frequency=(0.03, 0.05), octaves=2, seed=7, kind=TurbulenceKind.FRACTAL_NOISE)


def _noise_ref(size, **kw):
    return turbulence_ref.turbulence((size[1], size[0]), **{k: (int(v) if k == "kind" else v) for k, v in kw.items()})


@pytest.mark.parametrize("filt", list(WarpFilter))
def test_distort_equals_the_composed_references(engine, filt):
    """Engine.distort on a rendered 128 x 128 frame: turbulence into dst, then displace with the map being dst = turbulence_ref, then
    displace_ref on the download of the same render."""
    rec, _, _ = engine.render(*scene())
    plain = target_of(engine, rec)
    assert plain.any()
    with images(engine, (128, 128)) as (dst,):
        engine.distort(rec.target["id"], dst.id, (20.0, 14.0), DisplaceChannel.A, DisplaceChannel.G, filter=filt, edge=WarpEdge.CLAMP, **NOISE)
        got = dst.bits()
    noise = _noise_ref((128, 128), **NOISE)
    want = displace_ref.displace(plain, noise, (128, 128), (20.0, 14.0), displace_ref.A, displace_ref.G, filt=int(filt), edge=displace_ref.CLAMP)
    assert_same_bits(got, want, filt.name)
    assert (got != plain).any() and np.array_equal(target_of(engine, rec), plain)
    offsets = displace_ref.offset(20.0, noise[..., 3])
    assert np.abs(offsets).max() > 1 << 32  # the noise moves texels by more than one


def test_captured_with_the_frame(engine):
    """capture(displace=..., surface=...): render, displace into a second image by a map of its own, blit that image -- one launch
    more than with the blit alone (no scratch, no tables), replayed twice, the bytes of the eager calls; displace= together with
    resample= or warp= is refused before anything is captured."""
    filt = WarpFilter.BICUBIC
    dmap_bits = displace_cases.map_bits("random", 128, 128, 12)
    with images(engine, dmap_bits, (48, 40)) as (dmap, small):
        rec = jello_amd.Host().record(*scene())
        d = dict(map=dmap.id, dst=small.id, width=48, height=40, scale=3.0)
        with pytest.raises(ValueError, match="exclusive"):
            engine.capture(rec, resample=dict(dst=small.id, width=48, height=40, filter=ResampleFilter.BOX), displace=d)
        with pytest.raises(ValueError, match="exclusive"):
            engine.capture(rec, warp=dict(dst=small.id, width=48, height=40, matrix=IDENT), displace=d)
        captured_with_the_frame(engine, scene(), lambda target, dst: engine.displace(target, dmap.id, dst, (11.0, -7.0), filter=filt, edge=WarpEdge.MIRROR),
                                lambda dst: dict(displace=dict(map=dmap.id, dst=dst, width=128, height=128, scale=(11.0, -7.0), filter=filt,
                                                               edge=WarpEdge.MIRROR)),
                                lambda plain: displace_ref.displace(plain, dmap_bits, (128, 128), (11.0, -7.0), filt=int(filt), edge=displace_ref.MIRROR),
                                extra_launches=1, out_size=(128, 128), baseline_surface=True)


def test_captured_with_the_frame_and_the_turbulence_that_makes_the_map(engine):
    """capture(turbulence=dict(dst=out), displace=dict(map=out, dst=out), surface=...): one capture makes the map and uses it, in place
    -- two launches more than the frame with its blit (the turbulence's tables are resident after the eager call)."""
    def eager(target, dst):
        engine.turbulence(dst, **NOISE)
        engine.displace(target, dst, dst, 16.0, DisplaceChannel.R, DisplaceChannel.B)

    captured_with_the_frame(engine, scene(), eager,
                            lambda dst: dict(turbulence=dict(dst=dst, **NOISE),
                                             displace=dict(map=dst, dst=dst, width=128, height=128, scale=16.0, x_channel=DisplaceChannel.R,
                                                           y_channel=DisplaceChannel.B)),
                            lambda plain: displace_ref.displace(plain, _noise_ref((128, 128), **NOISE), (128, 128), 16.0, displace_ref.R, displace_ref.B),
                            extra_launches=2, out_size=(128, 128), baseline_surface=True)


def test_refusals(engine):
    """Every refusal of the header's list: JH_ERR_INVALID, a message that starts "jh_displace: ", no texel of the three images and no
    byte of a canary buffer touched; src == map and map == dst are accepted."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    nan, inf = math.nan, math.inf
    with images(engine, canary, canary, canary, (W, H, ImageFormat.RGBA8), (32769, 1), (W + 1, H), (W, H - 1)) as (src, dmap, dst, rgba8, long_, wider, lower):
        def call(s=None, m=None, d=None, mat=IDENT, head=(1, 0, 0), src_rect=(0, 0, 0, 0), dst_rect=(0, 0, 0, 0), scale=(1.0, 1.0), channels=(0, 1), null=False):
            desc = CDisplaceDesc((ctypes.c_double * 6)(*mat), *head, *src_rect, *dst_rect, *scale, *channels)
            return hip.jh_displace(ctx, src.id if s is None else s, dmap.id if m is None else m, dst.id if d is None else d,
                                   None if null else ctypes.byref(desc))

        refused = dict(common_refusals(call, rgba8, rects=(("source ", "source ", "src_rect"), ("destination ", "destination ", "dst_rect"))), **{
            "filter 3": (lambda: call(head=(3, 0, 0)), b"filter"),
            "filter -1": (lambda: call(head=(-1, 0, 0)), b"filter"),
            "edge 4": (lambda: call(head=(1, 4, 0)), b"edge"),
            "edge -1": (lambda: call(head=(1, -1, 0)), b"edge"),
            "flag bit 1": (lambda: call(head=(1, 0, 2)), b"flag"),
            "flag bit 31": (lambda: call(head=(1, 0, 0x80000001)), b"flag"),
            "a NaN entry": (lambda: call(mat=(1.0, nan, 0.0, 1.0, 0.0, 0.0)), b"not finite"),
            "an infinite entry": (lambda: call(mat=(1.0, 0.0, 0.0, 1.0, 0.0, inf)), b"not finite"),
            "determinant 0": (lambda: call(mat=(1.0, 2.0, 2.0, 4.0, 0.0, 0.0)), b"determinant is 0"),
            "determinant overflows": (lambda: call(mat=(1e200, 0.0, 0.0, 1e200, 0.0, 0.0)), b"determinant is not finite"),
            "65:1": (lambda: call(mat=(1.0 / 65.0, 0.0, 0.0, 1.0, 0.0, 0.0)), b"above 64"),
            "offset beyond 2^22": (lambda: call(mat=(1.0, 0.0, 0.0, 1.0, 5e6, 0.0)), b"above 2^22"),
            "a side above 32768": (lambda: call(s=long_.id), b"32768"),
            "source is the destination": (lambda: call(d=src.id, m=src.id), b"source is the destination"),
            "unknown map": (lambda: call(m=_id()), b"unknown map image id"),
            "map not RGBA16F": (lambda: call(m=rgba8.id), b"the map is not an RGBA16F image"),
            "a wider map": (lambda: call(m=wider.id), b"the map's size is not the destination's"),
            "a lower map": (lambda: call(m=lower.id), b"the map's size is not the destination's"),
            "x channel 4": (lambda: call(channels=(4, 0)), b"channel"),
            "y channel -1": (lambda: call(channels=(0, -1)), b"channel"),
            "an infinite scale": (lambda: call(scale=(inf, 1.0)), b"scale is not finite"),
            "a negative infinite scale": (lambda: call(scale=(1.0, -inf)), b"scale is not finite"),
            "a NaN scale": (lambda: call(scale=(0.0, nan)), b"scale is not finite"),
        })
        check_refusals(engine, "jh_displace", call, refused, untouched=((src, canary), (dmap, canary), (dst, canary)),
                       raises=(lambda: engine.displace(src.id, dmap.id, src.id, 1.0), lambda: engine.displace(src.id, dmap.id, dst.id, inf),
                               lambda: engine.displace(src.id, wider.id, dst.id, 1.0), lambda: engine.displace(src.id, dmap.id, dst.id, 1.0, 4, 0)),
                       accepted=(call, lambda: call(m=src.id, scale=(3.4e38, -3.4e38), channels=(3, 3)),  # (the largest scales, src == map)
                                 lambda: call(m=dst.id, dst_rect=(3, 3, 2, 2)), lambda: call(mat=(1.0 / 64.0, 0.0, 0.0, 1.0 / 64.0, 0.0, 0.0))))
        with images(engine, (0, 5), (0, 5)) as (empty, empty_map):
            assert hip.jh_displace(ctx, src.id, empty_map.id, empty.id, ctypes.byref(CDisplaceDesc((ctypes.c_double * 6)(*IDENT), 1, 0, 0))) == 0  # (an image without texels)
    assert [int(c) for c in DisplaceChannel] == [0, 1, 2, 3]


def test_the_call_is_one_query_of_the_tree(engine):
    bits = warp_cases.content("unit", 48, 33, seed=2)
    dmap_bits = displace_cases.map_bits("wide", 20, 40, 3)
    m = warp_cases.rotate(45, (48, 33), (20, 40))
    with images(engine, bits, dmap_bits, (20, 40)) as (src, dmap, dst):
        one_query(engine, "displace", lambda: engine.displace(src.id, dmap.id, dst.id, 5.0, matrix=m, filter=WarpFilter.BICUBIC, edge=WarpEdge.MIRROR))
        got = dst.bits()
    assert displace_ref.same_bits(got, displace_ref.displace(bits, dmap_bits, (40, 20), 5.0, matrix=m, filt=displace_ref.BICUBIC, edge=displace_ref.MIRROR))
