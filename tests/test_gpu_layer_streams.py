"""-m gpu: the fine stage ALONE on the hand-written command lists of tests/ptcl_streams.py -- what tests/test_gpu_fine_stage.py
does for segments, for the layer machinery: lazy BEGIN_CLIP, the empty-layer shortcut and each reason to refuse it, the memo of a
run, the lane-parallel counting loop at every phase of its window, and the three tiers of the stack.  A small carrier scene runs
through the whole pipeline on both sides; the PTCL, segment and blend-spill buffers are then overwritten with the same bytes and
only fine is dispatched again.  The device's f16 bits must be the oracle's at every pixel and, on every finite stream, the eager
interpreter's (in the multisampled modes on the streams without a FILL: those modes differ in a FILL's coverage alone).
Instantiations: Area, Msaa8, Msaa16, Area with a ramp bound (the one with the paint code) and Area over poisoned scratch memory.
tests/test_layer_streams_spec.py holds the same battery on the CPU and must pass first.

Last, one scene through the whole pipeline: every (mix mode, Porter-Duff operator) pair as a 16 x 16 cell, bit for bit against
the oracle in every buffer and against the W3C formulas at the cells' centres."""
import ctypes

import numpy as np
import pytest

import jello_amd
import ptcl_streams as P
from jello_amd.engine import RUN_DISPATCHES, RUN_ONLY_FINE, RUN_UPLOADS
from parity import compare

pytestmark = pytest.mark.gpu

# (name, aa, ramp bound, byte the scratch arrays are poisoned with)
INSTANCES = [("area", 0, False, None), ("msaa8", 1, False, None), ("msaa16", 2, False, None), ("area_ramp", 0, True, None),
             ("area_poisoned", 0, False, 0xFF)]


def _overflows(engine, reset):
    n = ctypes.c_uint32(99)
    assert engine.hip.jh_debug_clip_hint_overflows(engine.ctx, ctypes.byref(n), reset) == 0
    return n.value


@pytest.mark.parametrize("group", ["A", "B", "C", "D"])
@pytest.mark.parametrize("inst", INSTANCES, ids=[i[0] for i in INSTANCES])
def test_fine_alone_on_layer_streams(engine, inst, group):
    _, aa, ramp, poison = inst
    oracle = P.OracleFine(aa, ramp)  # (the carrier through the whole oracle pipeline)
    rec = oracle.rec
    assert rec.config["n_clip"] != 0
    engine.hip.jh_upload.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    engine.sync()
    _overflows(engine, 1)
    t = rec.target
    problems, held = [], 0
    try:
        for frame in P.frames(group):
            want = oracle.run(frame)
            for bid, raw in P.images(frame, rec).items():  # (validated against the buffers' real sizes in there)
                assert engine.hip.jh_upload(engine.ctx, bid, raw.ctypes.data, raw.nbytes) == 0
            if poison is not None:
                engine.debug_poison_scratch(poison)
            engine.run(rec, RUN_DISPATCHES | RUN_ONLY_FINE)
            engine.sync()
            got = P.tiles_of(engine.download_image(t["id"], t["width"], t["height"]).view(np.uint16).reshape(t["height"], t["width"], 4).copy())
            for s, g, w in zip(frame.streams, got, want):
                ref = P.expected(s) if s.finite and (aa == 0 or not s.has_fill) else None
                m = P.mismatch(s, g, w, "gpu", "oracle", ref, "interpreter")
                if m is None and ref is not None:
                    held += 1
                    m = P.mismatch(s, g, ref, "gpu", "interpreter", w, "oracle")
                if m:
                    problems.append(m)
        assert _overflows(engine, 0) == 0  # the carrier's clip nest made the hint cover the deepest stream
    finally:
        engine.release(rec)
    assert held == sum(1 for s in P.battery()[group] if s.finite and (aa == 0 or not s.has_fill)) or problems
    assert not problems, "%d streams differ:\n%s" % (len(problems), "\n".join(problems[:12]))


@pytest.mark.parametrize("aa", [0, 1], ids=["area", "msaa8"])
def test_blend_grid_through_the_whole_pipeline(engine, aa):
    s, p, cells = P.blend_grid(aa)
    assert len(cells) == 16 * 13
    out = compare(engine, s, p)  # every buffer and the image, bit for bit
    bad = P.check_grid(out["image"].view(np.uint16).reshape(p.height, p.width, 4), cells)
    assert not bad, bad
