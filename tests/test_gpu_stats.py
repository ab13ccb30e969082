"""-m gpu: jh_stats against the rule of DESIGN.md 5.22 (tests/stats_ref.py), every comparison byte for byte on the whole record, the
record in caller-owned memory with a canary on both sides -- the battery of tests/stats_cases.py, never-written images, quadrants
merged, two runs and a poisoned scratch, Engine.content_bounds and Engine.auto_levels on a rendered frame -- and the call's frame:
its refusals, its captures, its profile query."""
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import ImageFormat, StatsPopulation, StatsTransfer, StatsWhat
from jello_amd import stats as jstats
from jello_amd._lib import CStatsDesc
from jello_amd.engine import RUN_DISPATCHES, RUN_UPLOADS, STATS_RECORD_BYTES

import color_ref
import stats_cases
import stats_ref
from devmem import CANARY, DevBuf, target_of
from image_call import JH_ERR_OOM, canary_bits, captured_call, check_refusals, common_refusals, images, one_query, scene

pytestmark = pytest.mark.gpu

STATS_LAUNCHES = 2  # the partials, the finish (include/jello_hip.h)
GUARD = 64  # canary bytes on either side of the record
ONE = 0x3C00


class Record:
    """sizeof(jh_stats_record) bytes of caller-owned device memory between two canaries."""

    def __init__(self, engine):
        self.buf = DevBuf(engine, GUARD + STATS_RECORD_BYTES + GUARD)
        self.ptr = self.buf.ptr + GUARD
        assert self.ptr % 8 == 0

    def bytes(self):
        """The record's bytes, having seen both canaries whole."""
        b = self.buf.bytes()
        assert np.all(b[:GUARD] == CANARY) and np.all(b[GUARD + STATS_RECORD_BYTES:] == CANARY), "a byte outside the record was written"
        return b[GUARD:GUARD + STATS_RECORD_BYTES].tobytes()

    def free(self):
        self.buf.free()


def _keywords(c, rect="case"):
    return dict(what=StatsWhat(c["what"]), channel=c["channel"], threshold=c["threshold"], population=StatsPopulation(c["population"]),
                transfer=StatsTransfer(c["transfer"]), rect=c["rect"] if rect == "case" else rect)


def _first_difference(got, want):
    g, w = np.frombuffer(got, "<u4"), np.frombuffer(want, "<u4")
    bad = np.flatnonzero(g != w)
    return "equal" if len(bad) == 0 else "%d of %d words differ, first word %d: got %#x, want %#x" % (len(bad), len(g), bad[0], g[bad[0]], w[bad[0]])


def _run(engine, c, record):
    """The record of one case: the source uploaded (a case of kind "never": only created), the call, and the source only read."""
    bits = stats_cases.source(c)
    with images(engine, (c["w"], c["h"]) if c["kind"] == "never" else bits) as (src,):
        assert engine.stats(src.id, out_device_ptr=record.ptr, **_keywords(c)) is None
        got = record.bytes()
        if c["kind"] != "never":
            assert np.array_equal(src.bits(), bits), c["name"]  # the source is only read
    return got


@pytest.mark.parametrize("inst", stats_cases.INSTANTIATIONS, ids=lambda i: i.replace("k_stats<", "box_").replace(", ", "_").replace(">", ""))
def test_battery(engine, inst):
    """Every case of one instantiation of k_stats through Engine.stats into a record between canaries: the whole record is compared
    with the reference's bytes, and the source still holds its bits.  A failure names the case."""
    names = [c["name"] for c in stats_cases.CASES if c["inst"] == inst]
    assert names
    record = Record(engine)
    try:
        for name in names:
            got, want = _run(engine, stats_cases.BY_NAME[name], record), stats_cases.expected(name)
            assert got == want, "%s (%s): %s" % (name, inst, _first_difference(got, want))
    finally:
        record.free()


def test_the_battery_runs_every_instantiation():
    assert len(stats_cases.INSTANTIATIONS) == 5
    assert sum(len([c for c in stats_cases.CASES if c["inst"] == i]) for i in stats_cases.INSTANTIATIONS) == len(stats_cases.CASES)


def test_two_runs_and_a_poisoned_scratch_give_equal_bytes(engine):
    """Nothing relies on what a partial held before: the same cases again, and again after every scratch array of the context was
    filled with 0xEE and with 0x00, give the bytes of the first run."""
    names = ["1x1030_values_inst_w7_content_srgb_ch3", "513x3_values_inst_w3_content_linear_ch3", "3x3_values_inst_w4_content_srgb_ch3",
             "256x256_patterns_w7_content_srgb_ch3"]
    record = Record(engine)
    try:
        first = {n: _run(engine, stats_cases.BY_NAME[n], record) for n in names}
        for n in names:
            assert first[n] == stats_cases.expected(n), n
            assert _run(engine, stats_cases.BY_NAME[n], record) == first[n], n
        for byte in (0xEE, 0x00):
            for n in names:
                engine.debug_poison_scratch(byte)
                got = _run(engine, stats_cases.BY_NAME[n], record)
                assert got == first[n], "%s after poison %#x: %s" % (n, byte, _first_difference(got, first[n]))
    finally:
        record.free()


def test_four_quadrant_calls_merged_equal_one(engine):
    bits = stats_cases.content("values", None, 67, 41, 3, None, seed=7)
    kw = dict(threshold=0.5, population=StatsPopulation.CONTENT, transfer=StatsTransfer.SRGB, channel=1)
    record = Record(engine)
    try:
        with images(engine, bits) as (src,):
            engine.stats(src.id, out_device_ptr=record.ptr, **kw)
            whole = jstats.Stats(record.bytes())
            parts = []
            for rect in ((0, 0, 31, 19), (31, 0, 36, 19), (0, 19, 31, 22), (31, 19, 36, 22)):
                engine.stats(src.id, rect=rect, out_device_ptr=record.ptr, **kw)
                parts.append(jstats.Stats(record.bytes()))
    finally:
        record.free()
    merged = jstats.merge(jstats.merge(parts[0], parts[1]), jstats.merge(parts[2], parts[3]))
    assert merged == whole and whole.content_count > 100 and whole.tobytes() == stats_ref.record_bytes(bits, population=1, transfer=1, channel=1, threshold=0.5)


def test_a_never_written_source_reads_as_transparent_black_and_stays_never_written(engine):
    """No texel is content under threshold 0.5, every texel is under threshold 0 -- through the engine's own buffer, which returns a
    Stats -- and the call leaves the image never written: a rectangle written afterwards still clears the rest."""
    zeros = np.zeros((21, 33, 4), np.uint16)
    with images(engine, (33, 21)) as (src,):
        a = engine.stats(src.id, threshold=0.5)
        b = engine.stats(src.id, threshold=0.0, population=StatsPopulation.CONTENT, transfer=StatsTransfer.SRGB, rect=(3, 5, 20, 9))
        assert isinstance(a, jstats.Stats) and a.tobytes() == stats_ref.record_bytes(zeros, threshold=0.5)
        assert b.tobytes() == stats_ref.record_bytes(zeros, threshold=0.0, population=1, transfer=1, rect=(3, 5, 20, 9))
        assert a.content_count == 0 and a.bounds is None and b.bounds == (3, 5, 20, 9) and a.histogram[0][0] == 33 * 21
        # (had the call marked the image as written, this shadow into a rectangle would leave the rest of the memory as it was)
        engine.shadow(src.id, box=(4, 4, 10, 10), radius=1, sigma=1.0, color=(1, 1, 1, 1), rect=(2, 2, 12, 12))
        after = src.bits()
        outside = np.ones((21, 33), bool)
        outside[2:14, 2:14] = False
        assert not after[outside].any() and after[2:14, 2:14].any()


def test_an_image_without_texels_writes_the_header_and_zeros(engine):
    record = Record(engine)
    try:
        with images(engine, (0, 0)) as (src,):
            engine.stats(src.id, population=StatsPopulation.CONTENT, transfer=StatsTransfer.SRGB, out_device_ptr=record.ptr)
            got = record.bytes()
    finally:
        record.free()
    assert got == stats_ref.record_bytes(np.zeros((0, 0, 4), np.uint16), population=1, transfer=1)
    assert got == np.array([0, 0, 0, 0, 7, 1, 1, 0], "<u4").tobytes() + bytes(STATS_RECORD_BYTES - 32)


def test_content_bounds_of_a_rendered_frame(engine):
    """A glyph-like drawing rendered on the device: Engine.content_bounds against the box of the reference, whole and inside a
    rectangle at odd offsets, and the full record of the frame."""
    rec, _, _ = engine.render(*scene((128, 128), 5))
    frame = target_of(engine, rec)
    tid = rec.target["id"]
    s = jstats.Stats(stats_ref.record_bytes(frame))
    box = engine.content_bounds(tid)
    assert box == s.bounds and box is not None and box[2] < 128 and box[3] < 128
    at = np.argwhere(frame[..., 3] != 0)
    assert box == (at[:, 1].min(), at[:, 0].min(), at[:, 1].max() - at[:, 1].min() + 1, at[:, 0].max() - at[:, 0].min() + 1)
    for rect, kw in (((33, 21, 55, 41), {}), ((1, 1, 9, 9), {}), ((33, 21, 55, 41), dict(channel=0, threshold=0.5))):
        want = jstats.Stats(stats_ref.record_bytes(frame, what=1, rect=rect, **kw)).bounds
        assert engine.content_bounds(tid, rect=rect, **kw) == want, (rect, kw)
    got = engine.stats(tid, population=StatsPopulation.CONTENT, transfer=StatsTransfer.SRGB)
    assert got.tobytes() == stats_ref.record_bytes(frame, population=1, transfer=1)
    assert np.array_equal(target_of(engine, rec), frame)


@pytest.mark.parametrize("transfer", [StatsTransfer.LINEAR, StatsTransfer.SRGB])
def test_auto_levels_of_a_rendered_frame(engine, transfer):
    """Engine.auto_levels = stats_ref's histogram over the content, jello_amd.stats.levels of it, color_ref with those functions."""
    rec, _, _ = engine.render(*scene((64, 48), 3, color=(0.6, 0.3, 0.2, 1.0)))
    frame = target_of(engine, rec)
    with images(engine, (64, 48)) as (dst,):
        record = engine.auto_levels(rec.target["id"], dst.id, clip=(0.01, 0.02), transfer=transfer)
        got = dst.bits()
    want_record = jstats.Stats(stats_ref.record_bytes(frame, what=4, population=1, transfer=int(transfer)))
    assert record == want_record
    funcs = jstats.levels(want_record, (0.01, 0.02))[:3] + [None]
    assert any(f[1] != 1.0 for f in funcs[:3])
    want = color_ref.apply(frame, funcs=funcs, space=color_ref.SRGB if transfer == StatsTransfer.SRGB else color_ref.LINEAR, clamp=True)
    assert np.array_equal(got, want) and (want != frame).any()
    assert np.array_equal(target_of(engine, rec), frame)


def test_captured_with_the_frame(engine):
    """capture(stats=dict(out=...)): the frame and the record of its target, replayed twice into a cleared record -- the bytes of the
    eager call and of the reference -- with STATS_LAUNCHES more kernel nodes than the plain capture and no other node more."""
    s, p = scene((64, 48), 3)
    rec = jello_amd.Host().record(s, p)
    what = dict(threshold=0.5, population=StatsPopulation.CONTENT, transfer=StatsTransfer.SRGB, rect=(8, 4, 50, 40))
    record = Record(engine)
    g = g0 = None
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        frame = target_of(engine, rec)
        engine.stats(rec.target["id"], out_device_ptr=record.ptr, **what)
        eager = record.bytes()
        assert eager == stats_ref.record_bytes(frame, threshold=0.5, population=1, transfer=1, rect=(8, 4, 50, 40))
        g0 = engine.capture(rec)
        g = engine.capture(rec, stats=dict(out=record.ptr, **what))
        (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
        assert (k1, o1) == (k0 + STATS_LAUNCHES, o0)
        for _ in range(2):
            engine._check(engine.hip.jh_clear(engine.ctx, record.buf.id, GUARD, STATS_RECORD_BYTES), "clear")
            engine.replay(g)
            engine.sync()
            assert record.bytes() == eager
        assert np.array_equal(target_of(engine, rec), frame)
        with pytest.raises(ValueError, match="capture: stats= needs out="):
            engine.capture(rec, stats=dict(threshold=0.5))
    finally:
        for graph in (g, g0):
            if graph is not None:
                engine.graph_destroy(graph)
        record.free()


def test_capture_without_scratch_is_refused_with_advice(engine):
    """A capture that would have to allocate the partials' slot: JH_ERR_OOM and the advice, nothing written; after one eager call --
    of any image -- the capture is accepted, for a larger image too, and its replay writes the record."""
    hip, ctx = engine.hip, engine.ctx
    small, large = stats_cases.content("values", None, 9, 7, 3, None, seed=1), stats_cases.content("values", None, 515, 40, 3, None, seed=2)
    d = CStatsDesc(7, 3, 0.5, 0, 0)
    record = Record(engine)
    g = None
    try:
        with images(engine, small, large) as (a, b):
            engine.trim_scratch()  # the partials have to be allocated again
            rc, msg, refused = captured_call(engine, lambda: hip.jh_stats(ctx, b.id, ctypes.byref(d), record.ptr))
            engine.graph_destroy(refused)
            assert rc == JH_ERR_OOM and msg.startswith("jh_stats: ") and "once eagerly first" in msg, (rc, msg)
            assert np.all(np.frombuffer(record.bytes(), np.uint8) == CANARY)
            engine.stats(a.id, out_device_ptr=record.ptr, threshold=0.5)
            assert record.bytes() == stats_ref.record_bytes(small, threshold=0.5)
            rc, msg, g = captured_call(engine, lambda: hip.jh_stats(ctx, b.id, ctypes.byref(d), record.ptr))
            assert rc == 0, msg
            assert record.bytes() == stats_ref.record_bytes(small, threshold=0.5)  # a capture runs nothing
            engine.replay(g)
            engine.sync()
            assert record.bytes() == stats_ref.record_bytes(large, threshold=0.5)
    finally:
        if g is not None:
            engine.graph_destroy(g)
        record.free()


def test_refusals(engine):
    """Every refusal of the header's list that a device can hold (a rectangle of more than 2^31 texels: tests/test_stats_spec.py, on the
    plan): JH_ERR_INVALID, a message that starts "jh_stats: ", no texel of any image and no byte of the record or a canary touched."""
    hip, ctx = engine.hip, engine.ctx
    W, H = 16, 12
    canary = canary_bits(W, H)
    inf, nan = float("inf"), float("nan")
    record = Record(engine)
    try:
        with images(engine, canary, (W, H, ImageFormat.RGBA8)) as (src, rgba8):
            def call(s=None, rect=(0, 0, 0, 0), null=False, out="record", **fields):
                desc = CStatsDesc(7, 3, 0.5, 0, 0)
                desc.x, desc.y, desc.width, desc.height = rect
                for k, v in fields.items():
                    setattr(desc, k, v)
                return hip.jh_stats(ctx, src.id if s is None else s, None if null else ctypes.byref(desc), record.ptr if out == "record" else out)

            rows = common_refusals(lambda d=None, **kw: call(**kw), rgba8, source=True)
            refused = {k: v for k, v in rows.items() if "destination" not in k}
            refused.update({
                "null out pointer": (lambda: call(out=None), b"null out pointer"),
                "out pointer off by 4": (lambda: call(out=record.ptr + 4), b"not 8-byte aligned"),
                "out pointer off by 1": (lambda: call(out=record.ptr + 1), b"not 8-byte aligned"),
                "what 0": (lambda: call(what=0), b"what names no part"),
                "what 8": (lambda: call(what=8), b"unknown bits in what"),
                "what bit 31": (lambda: call(what=0x80000001), b"unknown bits in what"),
                "channel 4": (lambda: call(channel=4), b"unknown channel"),
                "channel -1": (lambda: call(channel=-1), b"unknown channel"),
                "population 2": (lambda: call(population=2), b"unknown population"),
                "population -1": (lambda: call(population=-1), b"unknown population"),
                "transfer 2": (lambda: call(transfer=2), b"unknown transfer"),
                "transfer -1": (lambda: call(transfer=-1), b"unknown transfer"),
                "threshold Inf": (lambda: call(threshold=inf), b"threshold is not finite"),
                "threshold -Inf": (lambda: call(threshold=-inf), b"threshold is not finite"),
                "threshold NaN": (lambda: call(threshold=nan), b"threshold is not finite"),
            })
            check_refusals(engine, "jh_stats", call, refused, untouched=((src, canary),),
                           raises=(lambda: engine.stats(src.id, what=0), lambda: engine.stats(src.id, what=8), lambda: engine.stats(src.id, channel=4),
                                   lambda: engine.stats(src.id, threshold=inf), lambda: engine.stats(src.id, rect=(8, 0, 9, 4)),
                                   lambda: engine.content_bounds(src.id, channel=-1), lambda: engine.auto_levels(src.id, transfer=2)))
            assert np.all(np.frombuffer(record.bytes(), np.uint8) == CANARY)  # no refusal wrote a byte of the record
            for accepted in (call, lambda: call(what=1, channel=0, population=1, transfer=1), lambda: call(rect=(15, 11, 1, 1)), lambda: call(threshold=-3.0e38)):
                assert accepted() == 0, hip.jh_last_error(ctx)
                engine.sync()
                record.bytes()
            assert np.array_equal(src.bits(), canary)
    finally:
        record.free()


def test_the_call_is_one_query_of_the_tree(engine):
    bits = stats_cases.content("values", None, 48, 33, 3, None, seed=2)
    record = Record(engine)
    try:
        with images(engine, bits) as (img,):
            one_query(engine, "stats", lambda: engine.stats(img.id, threshold=0.5, out_device_ptr=record.ptr))
            engine.sync()
            assert record.bytes() == stats_ref.record_bytes(bits, threshold=0.5)
    finally:
        record.free()
