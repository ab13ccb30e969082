"""-m gpu: RenderToYUV / jh_blit_yuv (include/jello_hip.h "YUV blit") byte for byte against tests/yuv_ref.py, a
numpy statement of the rule that shares nothing with the kernel, the generator or the committed table: rendered scenes in
every layout, matrix, range and transfer (and the oracle's image), all 2^24 code triples, random f16 bit patterns, pitch and
alignment inside canary-filled buffers, band mode, a captured graph, refused calls, a never-written source, the profiler and
the regrow loop."""
import ctypes
import itertools

import numpy as np
import pytest

import jello_amd
from jello_amd import BumpSizes, ImageFormat, YuvLayout, YuvMatrix, YuvRange, YuvTransfer, scenes
from jello_amd._lib import CYuvDesc
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS
from oracle.oracle_engine import OracleEngine

import surface_ref
import yuv_ref as ref
from devmem import CANARY, SCENES, DevBuf, Image, _id, target_of

pytestmark = pytest.mark.gpu

COMBOS = list(itertools.product(YuvLayout, YuvMatrix, YuvRange, YuvTransfer))


def assert_planes(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.uint8, "%s: plane %d has shape %r, want %r" % (what, i, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            at = tuple(int(v) for v in bad[0])
            raise AssertionError("%s: plane %d: %d bytes differ; first at %r: got %d want %d" % (what, i, len(bad), at, g[at], w[at]))


def _name(layout, matrix, rng, transfer):
    return "%s %s %s %s" % (layout.name, matrix.name, rng.name, transfer.name)


ORACLE_SUBSET = ("c1_area", "images", "odd_3x7", "odd_1001x517", "fuzz0", "fuzz5")


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_in_every_combination(engine, name):
    """render_to_yuv in both layouts, matrices, ranges and transfers = yuv_ref of the same frame's RGBA16F target; for a
    subset also = yuv_ref of the oracle's image of the same scene."""
    oracle_img = None
    for layout, matrix, rng, transfer in COMBOS:
        s, p = SCENES[name]()
        planes, rec, bump, attempts = engine.render_to_yuv(s, p, layout, matrix, rng, transfer)
        assert bump["failed"] == 0
        target = target_of(engine, rec)
        what = "%s %s" % (name, _name(layout, matrix, rng, transfer))
        assert_planes(planes, ref.convert(target, int(layout), int(matrix), int(rng), int(transfer)), what + " vs its target")
        if name in ORACLE_SUBSET:
            if oracle_img is None:
                # a recording of its own: the engine's renderer keeps scene images by key across frames, so the recording of a
                # later frame in a session no longer carries their uploads and the oracle could not run it on its own
                host_rec = jello_amd.Host().record(*SCENES[name]())
                orc = OracleEngine()
                orc.run(host_rec)
                oracle_img = np.asarray(orc.target(host_rec)).copy()
            assert_planes(planes, ref.convert(oracle_img, int(layout), int(matrix), int(rng), int(transfer)), what + " vs the oracle")


def test_all_code_triples(engine):
    """A 4096 x 4096 image of all 2^24 (R, G, B): pixel i has R = i & 255, G = (i >> 8) & 255, B = i >> 16, stored as
    f16(k / 255) with alpha 1.  Transfer NONE, all four tables, both layouts, Y and chroma planes."""
    lut = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float16)
    # with the unorm rule f16(k / 255) yields exactly code k
    assert np.array_equal(surface_ref.unorm8(surface_ref.clamp01(lut.astype(np.float32))), np.arange(256, dtype=np.uint8))
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    codes = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1).astype(np.uint8)
    img = np.empty((4096, 4096, 4), np.uint16)
    img[..., :3] = lut.view(np.uint16)[codes]
    img[..., 3] = 0x3C00
    src = Image(engine, img)
    del img
    try:
        for matrix, rng in itertools.product(YuvMatrix, YuvRange):
            y, cb, cr = ref.from_codes(codes, int(matrix), int(rng))
            for layout in YuvLayout:
                got = engine.blit_yuv(src.id, 4096, 4096, layout, matrix, rng, YuvTransfer.NONE)
                want = (y, np.stack([cb, cr], axis=-1)) if layout == YuvLayout.NV12 else (y, cb, cr)
                assert_planes(got, want, "all triples " + _name(layout, matrix, rng, YuvTransfer.NONE))
    finally:
        src.free()


def test_random_f16_bit_patterns(engine):
    """512 x 512 seeded random f16 bit patterns in all four channels -- NaN, +-inf, values above 1, negative and > 1 alpha
    included -- in both transfers (and every layout, matrix and range)."""
    rng_ = np.random.default_rng(20261017)
    img = rng_.integers(0, 65536, size=(512, 512, 4), dtype=np.uint16)
    f = img.view(np.float16)
    assert np.isnan(f).any() and np.isinf(f).any() and (f[..., :3] > 1).any() and (f[..., 3] < 0).any() and (f[..., 3] > 1).any()
    src = Image(engine, img)
    try:
        for layout, matrix, rng, transfer in COMBOS:
            got = engine.blit_yuv(src.id, 512, 512, layout, matrix, rng, transfer)
            assert_planes(got, ref.convert(img, int(layout), int(matrix), int(rng), int(transfer)),
                          "random f16 " + _name(layout, matrix, rng, transfer))
    finally:
        src.free()


def _crafted_plausible(w, h, seed):
    """Random f16 values in [0, 1.25] with random alpha in [0, 1]."""
    r = np.random.default_rng(seed)
    img = np.empty((h, w, 4), np.float16)
    img[..., :3] = r.random((h, w, 3)) * 1.25
    img[..., 3] = r.random((h, w))
    return img.view(np.uint16)


class Planes:
    """The planes of a w x h frame, each inside a canary-filled buffer of its own at byte `offset`, rows row bytes + `extra`
    apart, with 64 guard bytes behind."""

    def __init__(self, engine, w, h, layout, extra, offset):
        self.shapes = engine.yuv_plane_shapes(w, h, layout)
        self.layout, self.offset = layout, offset
        self.pitches = [rb + extra for _, rb in self.shapes]
        self.bufs = [DevBuf(engine, offset + rows * pitch + 64) for (rows, _), pitch in zip(self.shapes, self.pitches)]
        self.args = [(b.ptr + offset, pitch) for b, pitch in zip(self.bufs, self.pitches)]

    def check(self, want, what, rows_written=None):
        """The plane rows equal `want`, every other byte is the canary.  rows_written: per plane, a boolean mask of the rows
        that must have been written (default: all); the others must be untouched."""
        for i, (b, (rows, rb), pitch) in enumerate(zip(self.bufs, self.shapes, self.pitches)):
            raw = b.bytes()
            o = self.offset
            assert np.all(raw[:o] == CANARY) and np.all(raw[o + rows * pitch:] == CANARY), "%s: plane %d: guard bytes changed" % (what, i)
            body = raw[o:o + rows * pitch].reshape(rows, pitch)
            assert np.all(body[:, rb:] == CANARY), "%s: plane %d: bytes between the row's end and the pitch changed" % (what, i)
            w_ = want[i].reshape(rows, rb)
            mask = np.ones(rows, bool) if rows_written is None else rows_written[i]
            assert_planes([body[mask, :rb]], [w_[mask]], "%s plane %d" % (what, i))
            assert np.all(body[~mask, :rb] == CANARY), "%s: plane %d: rows outside the band changed" % (what, i)

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("size", [(203, 77), (208, 78), (32, 3), (1, 1)])
@pytest.mark.parametrize("extra", [0, 1, 16, 17])
@pytest.mark.parametrize("offset", [0, 1, 4, 16])
def test_pitch_alignment_and_canaries(engine, size, extra, offset):
    """Planes inside canary-filled buffers at pointer offsets 0, 1, 4 and 16 with pitches of row bytes + 0, 1, 16 and 17: the
    planes' rows are right (the wide and the narrow path write the same bytes) and no other byte changes."""
    w, h = size
    img = _crafted_plausible(w, h, 100 * w + h)
    src = Image(engine, img)
    try:
        for layout, transfer in itertools.product(YuvLayout, YuvTransfer):
            pl = Planes(engine, w, h, layout, extra, offset)
            try:
                assert engine.blit_yuv(src.id, w, h, layout, YuvMatrix.BT709, YuvRange.LIMITED, transfer, planes=pl.args) is None
                engine.sync()
                pl.check(ref.convert(img, int(layout), ref.BT709, ref.LIMITED, int(transfer)),
                         "%dx%d extra %d offset %d %s %s" % (w, h, extra, offset, layout.name, transfer.name))
            finally:
                pl.free()
    finally:
        src.free()


def test_band_mode_composes(engine):
    """Two bands of one frame converted into one set of canary-filled planes: the luma rows of the bands and the chroma rows
    under them equal the whole frame's, the rows no band covers keep the canary."""
    s, p = scenes.scene_c3(3000, 1024)
    p.bump = BumpSizes(ptcl=1 << 23, blend_spill=1 << 20)
    bands = [(0, 1), (2, 3)]  # bin rows of 256 pixel rows: rows 256..511 and 768..1023 belong to no band
    luma_rows = np.zeros(1024, bool)
    for y0, y1 in bands:
        luma_rows[y0 * 256:y1 * 256] = True
    chroma_rows = luma_rows[::2]
    for layout in YuvLayout:
        full, _, _, _ = engine.render_to_yuv(s, p, layout, YuvMatrix.BT601, YuvRange.FULL, YuvTransfer.SRGB)
        pl = Planes(engine, 1024, 1024, layout, 0, 0)
        try:
            try:
                for y0, y1 in bands:
                    engine.set_band(y0, y1)
                    _, _, bump, _ = engine.render_to_yuv(s, p, layout, YuvMatrix.BT601, YuvRange.FULL, YuvTransfer.SRGB, planes=pl.args)
                    assert bump["failed"] == 0
                engine.sync()
            finally:
                engine.set_band()
            pl.check(full, "bands " + layout.name, rows_written=[luma_rows] + [chroma_rows] * (len(pl.shapes) - 1))
        finally:
            pl.free()


def test_captured_graph(engine):
    """capture(yuv=...) adds exactly one kernel node to the frame; three replays give identical planes, equal to the eager
    conversion of the eager frame."""
    s, p = scenes.scene_c3(3000, 1024)
    p.bump = BumpSizes(ptcl=1 << 23, blend_spill=1 << 20)
    combo = (YuvLayout.NV12, YuvMatrix.BT709, YuvRange.LIMITED, YuvTransfer.SRGB)
    rec = jello_amd.Host().record(s, p)
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    engine.sync()
    assert engine.download(rec.buffer("bumpBuf")[0], dtype=np.uint32)[0] == 0
    t = rec.target
    want = ref.convert(target_of(engine, rec), *(int(c) for c in combo))
    eager = engine.blit_yuv(t["id"], 1024, 1024, *combo)
    assert_planes(eager, want, "eager blit_yuv")
    pl = Planes(engine, 1024, 1024, combo[0], 0, 0)
    g0 = g1 = None
    try:
        g0 = engine.capture(rec)
        g1 = engine.capture(rec, yuv=(pl.args,) + combo)
        k0, o0 = engine.graph_node_counts(g0)
        k1, o1 = engine.graph_node_counts(g1)
        assert k1 == k0 + 1 and o1 == o0, ((k0, o0), (k1, o1))
        for _ in range(3):
            for b in pl.bufs:
                engine._check(engine.hip.jh_upload(engine.ctx, b.id, np.full(b.n, CANARY, np.uint8).ctypes.data, b.n), "upload")
            engine.replay(g1)
            engine.sync()
            pl.check(want, "replayed frame")
    finally:
        for g in (g0, g1):
            if g is not None:
                engine.graph_destroy(g)
        engine.release(rec)
        pl.free()


def _desc(layout, matrix, rng, transfer, planes):
    d = CYuvDesc(layout, matrix, rng, transfer)
    for i, (ptr, pitch) in enumerate(planes):
        d.plane[i] = ptr
        d.pitch[i] = pitch
    return d


def test_refused_calls_touch_nothing(engine):
    """Every JH_ERR_INVALID case of jh_blit_yuv leaves the planes as they were, and a valid call on the same context works
    after each one."""
    hip, ctx = engine.hip, engine.ctx
    w, h = 13, 5
    cw, ch = 7, 3
    img = _crafted_plausible(w, h, 7)
    src, rgba8 = Image(engine, img), _id()
    engine.create_image(rgba8, w, h, ImageFormat.RGBA8)
    canary = [DevBuf(engine, 512) for _ in range(3)]
    nv12 = [(canary[0].ptr, w), (canary[1].ptr, 2 * cw), (None, 0)]
    i420 = [(canary[0].ptr, w), (canary[1].ptr, cw), (canary[2].ptr, cw)]

    def repl(planes, i, ptr=..., pitch=...):
        out = list(planes)
        out[i] = (out[i][0] if ptr is ... else ptr, out[i][1] if pitch is ... else pitch)
        return out

    cases = [
        ("unknown source", (0xDEAD_BEEF_0001, w, h, _desc(0, 1, 0, 0, nv12))),
        ("RGBA8 source", (rgba8, w, h, _desc(0, 1, 0, 0, nv12))),
        ("width differs", (src.id, w - 1, h, _desc(0, 1, 0, 0, nv12))),
        ("height differs", (src.id, w, h + 1, _desc(0, 1, 0, 0, nv12))),
        ("null Y plane", (src.id, w, h, _desc(0, 1, 0, 0, repl(nv12, 0, ptr=None)))),
        ("null CbCr plane", (src.id, w, h, _desc(0, 1, 0, 0, repl(nv12, 1, ptr=None)))),
        ("null Cb plane", (src.id, w, h, _desc(1, 1, 0, 0, repl(i420, 1, ptr=None)))),
        ("null Cr plane", (src.id, w, h, _desc(1, 1, 0, 0, repl(i420, 2, ptr=None)))),
        ("Y pitch below W", (src.id, w, h, _desc(0, 1, 0, 0, repl(nv12, 0, pitch=w - 1)))),
        ("CbCr pitch below 2 ceil(W/2)", (src.id, w, h, _desc(0, 1, 0, 0, repl(nv12, 1, pitch=2 * cw - 1)))),
        ("Cb pitch below ceil(W/2)", (src.id, w, h, _desc(1, 1, 0, 0, repl(i420, 1, pitch=cw - 1)))),
        ("Cr pitch below ceil(W/2)", (src.id, w, h, _desc(1, 1, 0, 0, repl(i420, 2, pitch=cw - 1)))),
        ("layout 2", (src.id, w, h, _desc(2, 1, 0, 0, i420))), ("layout -1", (src.id, w, h, _desc(-1, 1, 0, 0, i420))),
        ("matrix 2", (src.id, w, h, _desc(1, 2, 0, 0, i420))), ("matrix -1", (src.id, w, h, _desc(1, -1, 0, 0, i420))),
        ("range 2", (src.id, w, h, _desc(1, 1, 2, 0, i420))), ("range -1", (src.id, w, h, _desc(1, 1, -1, 0, i420))),
        ("transfer 2", (src.id, w, h, _desc(1, 1, 0, 2, i420))), ("transfer -1", (src.id, w, h, _desc(1, 1, 0, -1, i420))),
        ("null descriptor", (src.id, w, h, None)),
    ]
    want = ref.convert(img, ref.NV12, ref.BT709, ref.LIMITED, ref.NONE)
    good = Planes(engine, w, h, YuvLayout.NV12, 0, 0)
    try:
        for what, (sid, ww, hh, d) in cases:
            assert hip.jh_blit_yuv(ctx, sid, ww, hh, None if d is None else ctypes.byref(d)) == JH_ERR_INVALID, what
            engine.sync()
            for c in canary:
                assert np.all(c.bytes() == CANARY), what
            # (the third plane of NV12 is ignored: a null pointer there is a valid call)
            gd = _desc(0, 1, 0, 0, good.args + [(None, 0)])
            assert hip.jh_blit_yuv(ctx, src.id, w, h, ctypes.byref(gd)) == 0, what
            engine.sync()
            good.check(want, "valid call after " + what)
    finally:
        src.free()
        engine.free_image(rgba8)
        good.free()
        for c in canary:
            c.free()
    assert (ch, cw) == engine.yuv_plane_shapes(w, h, YuvLayout.I420)[1]


def test_never_written_source_is_black(engine):
    iid = _id()
    engine.create_image(iid, 9, 5, ImageFormat.RGBA16_FLOAT)
    try:
        for layout, matrix, rng, transfer in COMBOS:
            planes = engine.blit_yuv(iid, 9, 5, layout, matrix, rng, transfer)
            assert planes[0].shape == (5, 9) and np.all(planes[0] == (16 if rng == YuvRange.LIMITED else 0))
            for c in planes[1:]:
                assert c.shape[:2] == (3, 5) and np.all(c == 128)
    finally:
        engine.free_image(iid)


def test_regrow_loop(engine):
    """Undersized BumpSizes: render_to_yuv goes through the regrow loop and still gives the exact bytes."""
    s, p = scenes.scene_c3(800, 256)
    p.bump = BumpSizes(bin_data=256, tiles=512, lines=1024, seg_counts=1024, segments=1024, blend_spill=256, ptcl=1 << 14)
    planes, rec, bump, attempts = engine.render_to_yuv(s, p, YuvLayout.I420, YuvMatrix.BT601, YuvRange.LIMITED, YuvTransfer.NONE)
    assert bump["failed"] == 0 and attempts > 1
    s2, p2 = scenes.scene_c3(800, 256)
    p2.bump = BumpSizes(ptcl=1 << 22)
    host_rec = jello_amd.Host().record(s2, p2)
    orc = OracleEngine()
    orc.run(host_rec)
    assert_planes(planes, ref.convert(np.asarray(orc.target(host_rec)), ref.I420, ref.BT601, ref.LIMITED, ref.NONE),
                  "regrown frame vs the oracle")


def test_profile_has_a_blit_yuv_query(engine):
    """With profiling on the conversion is a query labelled "blit_yuv" (stage -1) under the RenderToYUV group, and no flat
    per-stage record."""
    s, p = scenes.scene_c1()
    engine.profile(True)
    try:
        engine.render_to_yuv(s, p)
        tree = engine.profile_collect_tree()
        engine.render_to_yuv(s, p)
        flat = engine.profile_collect()
    finally:
        engine.profile(False)
    q = [n for n in tree if n["label"] == "blit_yuv"]
    assert len(q) == 1 and q[0]["kind"] == "query" and q[0]["stage"] == -1
    parent = tree[q[0]["parent"]]
    assert parent["kind"] == "group" and parent["label"] == "RenderToYUV"
    assert q[0]["gpu_end_ms"] >= q[0]["gpu_start_ms"]
    assert len(flat) > 10 and all(name in jello_amd.STAGE_NAMES for name, _ in flat)
