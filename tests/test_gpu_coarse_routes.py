"""-m gpu: the two routes of coarse for a scene with clip layers give the same frame.

Such a scene normally takes the one walk + relocation (k_coarse_walk, k_coarse_bases, k_coarse_relocate).  The launcher falls back
to the two passes with clip state, k_coarse_pass<., true>, only when the PTCL binding has no words -- nothing to relocate into --
and no other test binds one.  Engine::run_recording creates a bound buffer only if the context has none under its id, so a
PTCL created with zero bytes before the run stays: every PTCL store is dropped by its bounds check (Buf::wr, ptcl_wr4, the `room`
test of the walk), and what coarse leaves besides the PTCL -- the bump totals and ~seg_ix in the Tiles, from which
path_tiling places the segments -- must not depend on the route.  Fine is skipped: nothing here reads a PTCL."""
import numpy as np
import pytest

import jello_amd
from jello_amd import scenes
from jello_amd.engine import RUN_DISPATCHES, RUN_SKIP_FINE, RUN_UPLOADS
from jello_amd.scene import Aa, BumpSizes

pytestmark = pytest.mark.gpu
BUMP = ["failed", "binning", "ptcl", "tile", "seg_counts", "segments", "blend", "lines"]


def coarse_outputs(eng, kind, empty_ptcl):
    """(bump, Tiles, segments) of scenes.scene_clip_torture(kind): 256 x 256, one bin shared by 16 strip workgroups."""
    s, p = scenes.scene_clip_torture(kind)
    p.aa, p.bump = Aa.Area, BumpSizes(ptcl=1 << 24, blend_spill=1 << 23)
    rec = jello_amd.Host().record(s, p)
    ptcl_id = rec.buffer("ptclBuf")[0]
    try:
        if empty_ptcl:
            eng._check(eng.hip.jh_buffer_create(eng.ctx, ptcl_id, 0), "buffer_create")
        eng.run(rec, RUN_UPLOADS | RUN_DISPATCHES | RUN_SKIP_FINE)
        eng.sync()
        assert (eng.hip.jh_buffer_size(eng.ctx, ptcl_id) == 0) == empty_ptcl, "the run replaced the PTCL binding"
        bump = eng.download(rec.buffer("bumpBuf")[0], 32, dtype=np.uint32).copy()
        n_tile, n_seg = int(bump[3]), int(bump[5])
        tiles = eng.download(rec.buffer("tileBuf")[0], 8 * n_tile, dtype=np.uint32).copy()
        segments = eng.download(rec.buffer("segmentsBuf")[0], 24 * n_seg, dtype=np.uint32).reshape(n_seg, 6)[:, :5].copy()  # 5 live words of 6
    finally:
        eng.release(rec)
    return bump, tiles, segments


@pytest.mark.parametrize("kind", ["deep", "mixed"])
def test_clip_scene_without_ptcl_takes_the_two_passes(engine, kind):
    want = coarse_outputs(engine, kind, empty_ptcl=False)
    fresh = jello_amd.Engine(0)
    try:
        got = coarse_outputs(fresh, kind, empty_ptcl=True)
    finally:
        fresh.close()
    for (b, t, s), route in ((want, "one walk + relocation"), (got, "two passes")):
        assert b[0] == 0, "%s: bump.failed = %d" % (route, b[0])
        assert b[3] > 0 and b[5] > 0, "%s: an empty frame checks nothing: %s" % (route, dict(zip(BUMP, b)))
    assert list(got[0]) == list(want[0]), "bump differs: two passes %s, one walk %s" % (dict(zip(BUMP, got[0])), dict(zip(BUMP, want[0])))
    for name, g, w in (("tileBuf", got[1], want[1]), ("segmentsBuf", got[2], want[2])):
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert bad.size == 0, "%s differs at %d word(s), first at %d: two passes 0x%x, one walk 0x%x" % (
            name, bad.size, bad[0], g.ravel()[bad[0]], w.ravel()[bad[0]])


def test_clip_scene_reports_a_seg_counts_overflow(engine):
    """bump.seg_counts beyond its buffer is found by coarse alone (coarse.wgsl:161-176): the one walk gives up and has to
    raise JL_STAGE_PATH_COUNT (8) in bump.failed as the write pass of the two-pass route does, or the regrow loop takes the
    empty frame for a finished one."""
    s, p = scenes.scene_clip_torture("deep")
    p.aa, p.bump = Aa.Area, BumpSizes(seg_counts=64, ptcl=1 << 24, blend_spill=1 << 23)
    rec = jello_amd.Host().record(s, p)
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES | RUN_SKIP_FINE)
        engine.sync()
        bump = engine.download(rec.buffer("bumpBuf")[0], 32, dtype=np.uint32).copy()
    finally:
        engine.release(rec)
    assert bump[4] > 64, "the scene fits 64 segment counts: %s" % dict(zip(BUMP, bump))
    assert bump[0] & 8, "no JL_STAGE_PATH_COUNT in bump.failed: %s" % dict(zip(BUMP, bump))
