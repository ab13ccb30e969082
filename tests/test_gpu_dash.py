"""-m gpu: the device stage of the dash rule (jh_dash) against tests/dash_ref.py, byte for byte, on the battery of
tests/dash_cases.py -- as one batch and path by path, elements and index words -- plus the contract of the call: a buffer that
is too small reports the need and nothing is written beyond its capacity, two calls and a call over poisoned scratch give the
same bytes, a rejected input is JH_ERR_INVALID and leaves the next call alone.  And the host route end to end on the HIP
pipeline: a dashed scene bit for bit against the oracle, and the closed-form coverage of a dashed line on the HIP image."""
import ctypes

import numpy as np
import pytest

from jello_amd import Aa, Brush, Cap, Host, Join, Path, RenderParams, Scene, Stroke
from jello_amd.engine import DASH_EL, RUN_DISPATCHES, RUN_UPLOADS

import coverage_scenes as C
import dash_cases
import dash_ref
from test_dash_spec import as_path, check_dashed_line, dashed_line_scene

pytestmark = pytest.mark.gpu

CASES = dash_cases.cases()
GUARD_BUFFER_ID = 0x4441534854455354


@pytest.fixture(scope="module")
def reference():
    """dash_ref on every job, computed once: {case name: bytes}, and the batch's list of bytes."""
    single = {name: dash_ref.to_bytes(dash_ref.dash(path, pattern, offset)) for name, path, pattern, offset in CASES}
    batch = [dash_ref.to_bytes(dash_ref.dash(path, pattern, offset)) for path, pattern, offset in dash_cases.batch_cases()]
    return single, batch


def job_of(cases):
    return [as_path(p) for p, _, _ in cases], [pat for _, pat, _ in cases], [off for _, _, off in cases]


def expect(blobs):
    index = np.concatenate([[0], np.cumsum([len(b) // DASH_EL.itemsize for b in blobs])]).astype(np.uint32)
    return b"".join(blobs), index


def test_battery_as_one_batch(engine, reference):
    single, _ = reference
    els, index = engine.dash_paths(*job_of([c[1:] for c in CASES]), raw=True)
    want, want_index = expect([single[c[0]] for c in CASES])
    assert np.array_equal(index, want_index)
    for i, c in enumerate(CASES):
        assert els[index[i]:index[i + 1]].tobytes() == single[c[0]], c[0]
    assert els.tobytes() == want


def test_battery_path_by_path(engine, reference):
    single, _ = reference
    for name, path, pattern, offset in CASES:
        els, index = engine.dash_paths([as_path(path)], [pattern], [offset], raw=True)
        assert list(index) == [0, len(single[name]) // DASH_EL.itemsize], name
        assert els.tobytes() == single[name], name


def test_300_paths_in_one_batch(engine, reference):
    _, batch = reference
    els, index = engine.dash_paths(*job_of(dash_cases.batch_cases()), raw=True)
    want, want_index = expect(batch)
    assert np.array_equal(index, want_index)
    assert els.tobytes() == want


def test_dash_paths_returns_paths(engine, reference):
    name, path, pattern, offset = [c for c in CASES if c[0] == "mixed_kinds"][0]
    out = engine.dash_paths([as_path(path), as_path(path)], [pattern, [5, 0]], [offset, 0.0])
    assert dash_ref.to_bytes(out[0].els) == reference[0][name]
    assert dash_ref.to_bytes(out[1].els) == dash_ref.to_bytes(dash_ref.dash(path, [5, 0], 0.0))
    assert engine.dash_paths([], [], []) == []


def test_a_buffer_one_element_short(engine, reference):
    """The need is reported, nothing at or beyond the capacity is written, and the regrown call succeeds."""
    single, _ = reference
    names = ["closed_merged", "seg_1100_dashes", "mixed_kinds"]  # (a relocated piece among them: it is written out of order)
    cases = [c for n in names for c in CASES if c[0] == n]
    want, want_index = expect([single[n] for n in names])
    total = int(want_index[-1])
    size = DASH_EL.itemsize
    hip, ctx = engine.hip, engine.ctx
    guard = np.full((total + 64) * size, 0xC5, dtype=np.uint8)
    engine._check(hip.jh_upload(ctx, GUARD_BUFFER_ID, guard.ctypes.data, guard.nbytes), "upload")
    engine._check(hip.jh_buffer_create(ctx, GUARD_BUFFER_ID + 1, 4 * (len(names) + 1)), "buffer_create")
    els_ptr, index_ptr = hip.jh_buffer_device_ptr(ctx, GUARD_BUFFER_ID), hip.jh_buffer_device_ptr(ctx, GUARD_BUFFER_ID + 1)
    try:
        for capacity in (total - 1, total):
            engine.dash_into(*job_of([c[1:] for c in cases]), els_ptr, capacity, index_ptr)
            index = engine.download(GUARD_BUFFER_ID + 1, dtype=np.uint32)[:len(names) + 1]
            got = engine.download(GUARD_BUFFER_ID, dtype=np.uint8)[:guard.nbytes]
            assert np.array_equal(index, want_index), capacity          # the need, whatever the capacity
            assert got[:capacity * size].tobytes() == want[:capacity * size]
            assert (got[capacity * size:] == 0xC5).all(), "bytes beyond the capacity were written"
        # and through the convenience call, which regrows once
        els, index = engine.dash_paths(*job_of([c[1:] for c in cases]), capacity=total - 1, raw=True)
        assert els.tobytes() == want and np.array_equal(index, want_index)
    finally:
        hip.jh_free(ctx, GUARD_BUFFER_ID)
        hip.jh_free(ctx, GUARD_BUFFER_ID + 1)


def test_repeatable_and_independent_of_scratch_contents(engine, reference):
    _, batch = reference
    job = job_of(dash_cases.batch_cases()[:80])
    a = engine.dash_paths(*job, raw=True)
    b = engine.dash_paths(*job, raw=True)
    engine.debug_poison_scratch()
    c = engine.dash_paths(*job, raw=True)
    want, want_index = expect(batch[:80])
    for els, index in (a, b, c):
        assert els.tobytes() == want and np.array_equal(index, want_index)


def test_a_rejected_input_is_invalid_and_harmless(engine, reference):
    single, _ = reference
    good = [c for c in CASES if c[0] == "sub_300_segments"][0]
    line = as_path(dash_cases.polyline([(0, 0), (12, 0)]))
    nan_path = as_path([dash_cases.M(0, 0), dash_cases.L(float("nan"), 1)])
    for paths, patterns, offsets in [([line], [[4, -1]], [0.0]), ([line], [[0, 0]], [0.0]), ([line], [[]], [0.0]), ([line], [[1.0] * 65], [0.0]),
                                     ([line], [[4, 2]], [float("inf")]), ([line, nan_path], [[4, 2], [4, 2]], [0.0, 0.0])]:
        with pytest.raises(ValueError):
            engine.dash_paths(paths, patterns, offsets)
        els, index = engine.dash_paths([as_path(good[1])], [good[2]], [good[3]], raw=True)
        assert els.tobytes() == single[good[0]]
    # the C ABI's own answer
    L = engine._L
    from jello_amd._lib import CDashPath, PathEl
    els = line._c()
    desc = (CDashPath * 1)()
    desc[0].first_el, desc[0].n_els, desc[0].first_dash, desc[0].n_dash, desc[0].offset = 0, 2, 0, 2, 0.0
    bad = (ctypes.c_double * 2)(4.0, float("nan"))
    engine._check(engine.hip.jh_buffer_create(engine.ctx, GUARD_BUFFER_ID, 4096), "buffer_create")
    try:
        ptr = engine.hip.jh_buffer_device_ptr(engine.ctx, GUARD_BUFFER_ID)
        assert engine.hip.jh_dash(engine.ctx, els, 2, desc, 1, bad, 2, ptr, 64, ptr) == -1  # JH_ERR_INVALID
        assert b"jh_dash" in engine.hip.jh_last_error(engine.ctx)
    finally:
        engine.hip.jh_free(engine.ctx, GUARD_BUFFER_ID)


def test_the_call_is_a_profile_query(engine):
    engine.profile(True)
    try:
        engine.dash_paths([as_path(dash_cases.polyline([(0, 0), (12, 0)]))], [[4, 2]], [0.0])
        tree = engine.profile_collect_tree()
    finally:
        engine.profile(False)

    assert any(n["kind"] == "query" and n["label"] == "dash" and n["stage"] == -1 for n in tree)


def dashed_scene():
    s = Scene()
    white = Brush.solid(C.WHITE)
    caps = [Cap.Butt, Cap.Square, Cap.Round]
    for i, cap in enumerate(caps):
        style = Stroke(3.0 + i, Join.Round if i == 2 else Join.Miter, 4.0, cap, caps[(i + 1) % 3], dash_pattern=[9.0 + i, 4.5, 2.0, 4.5], dash_offset=1.25 * i)
        y = 20.0 + 40.0 * i
        s.stroke(style, None, white, None, Path().move_to(10, y).line_to(120, y + 8).line_to(200, y - 6).line_to(246, y))
        s.stroke(style, (1.0, 0.1, -0.1, 1.0, 0.0, 120.0), white, None,
                 Path().move_to(10, y).cubic_to(80, y - 30, 150, y + 40, 240, y).quad_to(200, y + 20, 180, y + 4))
    s.stroke(Stroke(2.0, Join.Bevel, 4.0, Cap.Butt, Cap.Butt, dash_pattern=[6, 3]), None, white, None, Path.circle(128, 128, 100))
    return s


def test_a_dashed_scene_is_bit_identical_to_the_oracle(engine):
    from parity import compare
    scene = dashed_scene()
    out = compare(engine, scene, RenderParams(256, 256, aa=Aa.Area, bump=scene.bump_sizes(256, 256)))
    assert out["image"].any()


@pytest.mark.parametrize("offset", [0.0, 0.5])
def test_dashed_line_coverage_on_the_hip_image(engine, offset):
    rec = Host().record(dashed_line_scene(offset), RenderParams(64, 32, aa=Aa.Area))
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    engine.sync()
    try:
        assert int(engine.download(rec.buffer("bumpBuf")[0], dtype=np.uint32)[0]) == 0
        t = rec.target
        img = engine.download_image(t["id"], t["width"], t["height"])
    finally:
        engine.release(rec)
    check_dashed_line(img.view(np.float16).astype(np.float64)[..., 3], offset)
