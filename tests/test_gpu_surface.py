"""-m gpu: RenderToSurface / jh_blit (include/jello_hip.h, DESIGN.md "Surface blit") against tests/surface_ref.py, a numpy
statement of the conversion rule that shares nothing with the kernel or its threshold table: rendered scenes in all four
formats (and the oracle's image), every f16 bit pattern, pitch and alignment, band mode, a captured graph, refused calls,
the regrow loop and the profiler."""
import numpy as np
import pytest

import jello_amd
from jello_amd import BumpSizes, ImageFormat, Surface, scenes
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS
from oracle.oracle_engine import OracleEngine

import surface_ref as ref
from devmem import CANARY, SCENES, DevBuf, _id, _odd, target_of

pytestmark = pytest.mark.gpu

def assert_surface(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x, c = bad[0]
        raise AssertionError("%s: %d bytes differ; first at (x=%d, y=%d, byte %d): got %d want %d" %
                             (what, len(bad), x, y, c, got[y, x, c], want[y, x, c]))


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_in_every_format(engine, name):
    """render_to_surface in all four formats = surface_ref of the same frame's RGBA16F target = surface_ref of the oracle's
    image of the final recording."""
    oracle_img = None
    for fmt in Surface:
        s, p = SCENES[name]()
        surf, rec, bump, attempts = engine.render_to_surface(s, p, fmt)
        assert bump["failed"] == 0 and surf.shape == (p.height, p.width, 4) and surf.dtype == np.uint8
        target = target_of(engine, rec)
        assert_surface(surf, ref.convert(target, int(fmt)), "%s %s vs its target" % (name, fmt.name))
        if oracle_img is None:
            orc = OracleEngine()
            orc.run(rec)
            oracle_img = np.asarray(orc.target(rec)).copy()
        assert_surface(surf, ref.convert(oracle_img, int(fmt)), "%s %s vs the oracle" % (name, fmt.name))


def _blit_crafted(engine, img_bits, fmt):
    """Uploads an (H, W, 4) uint16 f16 image and blits it; returns the (H, W, 4) uint8 surface."""
    h, w, _ = img_bits.shape
    iid = _id()
    try:
        engine.upload_image(iid, np.asarray(img_bits, np.uint16))
        return engine.blit(iid, w, h, fmt)
    finally:
        engine.free_image(iid)


ALPHAS = [0x0000, 0x8000, 0x0001, 0x0002, 0x00FF, 0x03FF, 0x8001, 0x83FF, 0x0400, 0x1C00, 0x1E00, 0x2000, 0x2E66, 0x3000,
          0x3266, 0x3400, 0x3555, 0x3800, 0x3801, 0x399A, 0x3A00, 0x3B33, 0x3BFF, 0x3C00, 0x3C01, 0x3E00, 0x4000, 0x5BF8,
          0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0x7C01, 0xFE00, 0xB800, 0xBC00, 0xC000, 0x1A0C, 0x2C00, 0x3A8F]


@pytest.mark.parametrize("fmt", list(Surface))
def test_every_f16_colour_against_alphas(engine, fmt):
    """All 65 536 f16 bit patterns in every colour channel (in three different orders) against 40 alphas: +-0, subnormals,
    0.5, 1, > 1, inf, NaN, negatives.  Proves the kernel's sRGB estimate-and-correct exact where a colour value lands."""
    pat = np.arange(65536, dtype=np.uint32)
    w = 1024
    rows = 65536 // w
    img = np.empty((len(ALPHAS) * rows, w, 4), np.uint16)
    for i, a in enumerate(ALPHAS):
        blk = img[i * rows:(i + 1) * rows].reshape(-1, 4)
        blk[:, 0] = pat
        blk[:, 1] = pat[::-1]
        blk[:, 2] = (pat * 40503) & 0xFFFF  # (an odd multiplier: a permutation)
        blk[:, 3] = a
    assert_surface(_blit_crafted(engine, img, fmt), ref.convert(img, int(fmt)), "f16 colours " + fmt.name)


@pytest.mark.parametrize("fmt", list(Surface))
def test_every_f16_alpha_in_unit_interval(engine, fmt):
    """Every f16 alpha in [0, 1] (0x0000 .. 0x3C00) against fixed colours, in an odd-width image (8-B aligned source rows,
    one-pixel tails)."""
    alphas = np.arange(0x3C01, dtype=np.uint16)
    colours = [(0x3C00, 0x3800, 0x0000), (0x3266, 0x399A, 0x3BFF), (0x0001, 0x03FF, 0x2E66), (0x7C00, 0xFC00, 0x7E00),
               (0x3555, 0x3A00, 0x1E00), (0x3C01, 0x4000, 0xB800), (0x2000, 0x2C00, 0x3400), (0x3B33, 0x3E00, 0x8000)]
    img = np.empty((len(colours), alphas.size, 4), np.uint16)
    for i, c in enumerate(colours):
        img[i, :, 0], img[i, :, 1], img[i, :, 2] = c
        img[i, :, 3] = alphas
    assert_surface(_blit_crafted(engine, img, fmt), ref.convert(img, int(fmt)), "f16 alphas " + fmt.name)


def test_c3_full_size_captured_graph(engine):
    """C3 at full size (100k paths, 4096 x 4096, area): capture(surface=...) adds exactly one kernel launch to the frame;
    three replays give identical bytes, equal to the blit of the eager frame and to an eager render_to_surface."""
    s, p = scenes.scene_c3(100_000, 4096)
    p.bump = BumpSizes(lines=1 << 22, seg_counts=1 << 23, segments=1 << 23, tiles=1 << 21, ptcl=1 << 25, bin_data=1 << 20)
    fmt = Surface.BGRA8_SRGB
    rec = jello_amd.Host().record(s, p)
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    engine.sync()
    assert engine.download(rec.buffer("bumpBuf")[0], dtype=np.uint32)[0] == 0
    want = ref.convert(target_of(engine, rec), int(fmt))
    buf = DevBuf(engine, 4096 * 4096 * 4)
    g0 = g1 = None
    try:
        g0 = engine.capture(rec)
        g1 = engine.capture(rec, surface=(buf.ptr, 4096 * 4, fmt))
        k0, o0 = engine.graph_node_counts(g0)
        k1, o1 = engine.graph_node_counts(g1)
        assert k1 == k0 + 1 and o1 == o0, ((k0, o0), (k1, o1))
        outs = []
        for _ in range(3):
            engine.clear(buf.id)  # (every replay writes the whole surface again)
            engine.replay(g1)
            engine.sync()
            outs.append(buf.bytes().reshape(4096, 4096, 4))
        for o in outs:
            assert_surface(o, want, "replayed C3")
    finally:
        for g in (g0, g1):
            if g is not None:
                engine.graph_destroy(g)
        engine.release(rec)
        buf.free()
    surf, rec2, bump, attempts = engine.render_to_surface(s, p, fmt)
    assert bump["failed"] == 0
    assert_surface(surf, want, "eager render_to_surface C3")


@pytest.mark.parametrize("extra,offset", [(64, 0), (4, 4), (2, 1), (0, 8)])
def test_pitch_and_padding(engine, extra, offset):
    """pitch = 4 W + extra into a canary-filled buffer at dst + offset: the pixels are right and no other byte changes
    (16-B aligned rows, 4-B aligned rows, rows at odd addresses, 8-B aligned rows)."""
    s, p = _odd(203, 77, 21)
    w, h = p.width, p.height
    pitch = 4 * w + extra
    buf = DevBuf(engine, offset + pitch * h + 64)
    try:
        for fmt in Surface:
            _, rec, bump, _ = engine.render_to_surface(s, p, fmt, out_device_ptr=buf.ptr + offset, pitch=pitch)
            engine.sync()
            got = buf.bytes()
            want = ref.convert(target_of(engine, rec), int(fmt))
            rows = got[offset:offset + pitch * h].reshape(h, pitch)
            assert_surface(rows[:, :4 * w].reshape(h, w, 4), want, "pitch %d offset %d %s" % (pitch, offset, fmt.name))
            assert np.all(rows[:, 4 * w:] == CANARY)
            assert np.all(got[:offset] == CANARY) and np.all(got[offset + pitch * h:] == CANARY)
    finally:
        buf.free()


def test_band_mode_composes(engine):
    """Two bands of one frame blitted into one canary-filled surface: the band rows equal the whole frame's surface, the
    rows of the bin rows no band covers keep the canary."""
    s, p = scenes.scene_c3(3000, 1024)
    p.bump = BumpSizes(ptcl=1 << 23, blend_spill=1 << 20)
    fmt = Surface.RGBA8_SRGB
    full, _, _, _ = engine.render_to_surface(s, p, fmt)
    buf = DevBuf(engine, 1024 * 1024 * 4)
    bands = [(0, 1), (2, 3)]  # bin rows of 256 pixel rows: rows 256..511 and 768..1023 belong to no band
    try:
        for y0, y1 in bands:
            engine.set_band(y0, y1)
            _, _, bump, _ = engine.render_to_surface(s, p, fmt, out_device_ptr=buf.ptr)
            assert bump["failed"] == 0
        engine.sync()
    finally:
        engine.set_band()
    got = buf.bytes().reshape(1024, 1024, 4)
    buf.free()
    for y0, y1 in bands:
        assert_surface(got[y0 * 256:y1 * 256], full[y0 * 256:y1 * 256], "band %d..%d" % (y0, y1))
    assert np.all(got[256:512] == CANARY) and np.all(got[768:] == CANARY)


def test_refused_calls_touch_nothing(engine):
    """Every JH_ERR_INVALID case of jh_blit leaves the destination as it was, and a valid blit on the same context works
    after each one."""
    hip, ctx = engine.hip, engine.ctx
    w, h = 13, 5
    rng = np.random.default_rng(7)
    img = rng.integers(0, 0x3C01, size=(h, w, 4), dtype=np.uint16)
    src, rgba8 = _id(), _id()
    engine.upload_image(src, img)
    engine.create_image(rgba8, w, h, ImageFormat.RGBA8)
    canary = DevBuf(engine, 4 * w * h + 256)
    good = DevBuf(engine, 4 * w * h)
    want = ref.convert(img, 0)
    cases = [
        ("unknown source", (0xDEAD_BEEF_0001, canary.ptr, 4 * w, w, h, 0)),
        ("RGBA8 source", (rgba8, canary.ptr, 4 * w, w, h, 0)),
        ("width differs", (src, canary.ptr, 4 * w + 4, w + 1, h, 0)),
        ("height differs", (src, canary.ptr, 4 * w, w, h - 1, 0)),
        ("pitch below 4 W", (src, canary.ptr, 4 * w - 1, w, h, 0)),
        ("null dst", (src, None, 4 * w, w, h, 0)),
        ("format 4", (src, canary.ptr, 4 * w, w, h, 4)),
        ("format -1", (src, canary.ptr, 4 * w, w, h, -1)),
    ]
    try:
        for what, args in cases:
            assert hip.jh_blit(ctx, *args) == JH_ERR_INVALID, what
            engine.sync()
            assert np.all(canary.bytes() == CANARY), what
            assert hip.jh_blit(ctx, src, good.ptr, 4 * w, w, h, 0) == 0, what
            engine.sync()
            assert_surface(good.bytes().reshape(h, w, 4), want, "valid blit after " + what)
    finally:
        engine.free_image(src)
        engine.free_image(rgba8)
        canary.free()
        good.free()


def test_never_written_source_is_transparent_black(engine):
    iid = _id()
    engine.create_image(iid, 9, 4, ImageFormat.RGBA16_FLOAT)
    try:
        for fmt in Surface:
            assert not engine.blit(iid, 9, 4, fmt).any()
    finally:
        engine.free_image(iid)


def test_regrow_loop(engine):
    """Undersized BumpSizes: render_to_surface goes through the regrow loop and still gives the exact bytes."""
    s, p = scenes.scene_c3(800, 256)
    p.bump = BumpSizes(bin_data=256, tiles=512, lines=1024, seg_counts=1024, segments=1024, blend_spill=256, ptcl=1 << 14)
    surf, rec, bump, attempts = engine.render_to_surface(s, p, Surface.RGBA8_UNORM)
    assert bump["failed"] == 0 and attempts > 1
    s2, p2 = scenes.scene_c3(800, 256)
    p2.bump = BumpSizes(ptcl=1 << 22)
    host_rec = jello_amd.Host().record(s2, p2)
    orc = OracleEngine()
    orc.run(host_rec)
    assert_surface(surf, ref.convert(np.asarray(orc.target(host_rec)), 0), "regrown frame vs the oracle")


def test_profile_has_a_blit_query(engine):
    """With profiling on the blit is a query labelled "blit" (stage -1) under the RenderToSurface group, and no flat
    per-stage record."""
    s, p = scenes.scene_c1()
    engine.profile(True)
    try:
        engine.render_to_surface(s, p, Surface.RGBA8_UNORM)
        tree = engine.profile_collect_tree()
        engine.render_to_surface(s, p, Surface.RGBA8_UNORM)
        flat = engine.profile_collect()
    finally:
        engine.profile(False)
    blits = [n for n in tree if n["label"] == "blit"]
    assert len(blits) == 1 and blits[0]["kind"] == "query" and blits[0]["stage"] == -1
    parent = tree[blits[0]["parent"]]
    assert parent["kind"] == "group" and parent["label"] == "RenderToSurface"
    assert blits[0]["gpu_end_ms"] >= blits[0]["gpu_start_ms"]
    assert len(flat) > 10 and all(name in jello_amd.STAGE_NAMES for name, _ in flat)
