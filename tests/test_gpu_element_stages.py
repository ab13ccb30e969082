"""-m gpu: the element stages in front of path_count as stages of their own -- the path-tag scan on both of its routes and on both
sides of every threshold, draw_reduce / draw_leaf across the block split, binning, tile_alloc, and the single-launch u32 scan -- through
jh_dispatch (jh_debug_scan_u32 for the scan) on buffers built by hand, against the definitions of tests/element_streams.py, which
test_element_spec.py holds against the oracle on the same cases.  Every comparison is exact; outputs are poisoned first and the words the
definition does not name must come back as poison."""
import ctypes
import time

import numpy as np
import pytest

import jello_amd
import element_streams as E
from devmem import _id
from parity import compare
from test_gpu_clip import Binding

pytestmark = pytest.mark.gpu
PT_ABSORB_MAX = 16  # kcommon.h: the largest pathtag_scan1 grid that redoes a held-back pathtag_reduce2 in passing
PATHTAG = E.pathtag_streams()
BINNING = E.binning_cases()
TILES = E.tile_alloc_cases()


class Job:
    """The buffers of a hand-built dispatch list as context buffers: uploaded on entry, freed on exit."""

    def __init__(self, engine, bufs):
        self.e, self.bufs = engine, {k: np.ascontiguousarray(v) for k, v in bufs.items()}
        self.ids = {k: _id() for k in bufs}
        engine.hip.jh_dispatch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Binding),
                                           ctypes.c_int]

    def __enter__(self):
        for k in self.bufs:
            self.upload(k)
        return self

    def __exit__(self, *a):
        for i in self.ids.values():
            self.e.hip.jh_free(self.e.ctx, i)

    def upload(self, k, array=None):
        a = self.bufs[k] if array is None else np.ascontiguousarray(array)
        self.e._check(self.e.hip.jh_upload(self.e.ctx, self.ids[k], a.ctypes.data, a.nbytes), "upload")

    def dispatch_rc(self, stage, gx, names):
        b = (Binding * len(names))(*[Binding(1, 0, self.ids[k], None) for k in names])
        return self.e.hip.jh_dispatch(self.e.ctx, E.STAGE[stage], gx, 1, 1, b, len(names))

    def dispatch(self, dispatches):
        for stage, gx, names in dispatches:
            self.e._check(self.dispatch_rc(stage, gx, names), stage)

    def download(self, names=None):
        return {k: self.e.download(self.ids[k], dtype=np.uint32).copy().reshape(self.bufs[k].shape) for k in (names or self.bufs)}

    def run(self, dispatches):
        self.dispatch(dispatches)
        self.e.sync()  # (launches what is still held back, as recorded)
        return self.download()


def kernel_launches(engine, job, dispatches):
    """Kernel launches of the dispatch list, counted on a captured graph (which is not replayed)."""
    engine._check(engine.hip.jh_graph_begin(engine.ctx), "graph_begin")
    try:
        job.dispatch(dispatches)
    finally:
        g = ctypes.c_void_p()
        rc = engine.hip.jh_graph_end(engine.ctx, ctypes.byref(g))
    engine._check(rc, "graph_end")
    kernels, others = engine.graph_node_counts(g)
    engine.graph_destroy(g)
    assert others == 0
    return kernels


# ---- pathtag ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wgs,kind", PATHTAG, ids=[s[0] for s in PATHTAG])
def test_pathtag_scan_on_tag_streams(engine, name, wgs, kind):
    """Random tag bytes (every bit pattern reaches reduce_tag), all-ones and all-zero words, at 1, 2, 255, 256 tag-word workgroups
    (pathtag_scan_small) and 257, 511, 512, 513, 3840, 3841, 4096, 4097 (the three-level route; pathtag_scan1 grids of 2, 2, 2, 3, 15,
    16, 16, 17: both sides of PT_ABSORB_MAX and of a `reduced` length that is a multiple of 256), with the workgroup counts and buffer
    sizes of a recording of that tag count.  Twice: as the engine runs it -- pathtag_reduce2 held back and, up to PT_ABSORB_MAX
    workgroups, redone by k_pathtag_scan1<true>, the last scan held back and launched as recorded by the sync -- and with the profiler
    on, every command as recorded.  Which route ran is asserted: by the launches of a captured graph (3 when reduce2 was absorbed,
    4 when not, 2 on the small route) and by the profile's labels.  reduced, all 256 entries of reduced2 (the tail of `reduced` is
    uploaded as poison, so each has a definite value -- the entries behind scan1's grid included, which workgroup 0 writes on the
    absorbed route), reducedScan and every tag monoid against the definition; the two routes against each other word for word.
    random_4097 (4 MB of tags, 21 MB of monoids; the largest case): 0.34 s on the MI355X machine, inputs, both routes and the
    definition included."""
    t0 = time.perf_counter()
    counts = E.host_counts(wgs)
    scene = E.pathtag_scene(wgs, kind)
    want = E.pathtag_by_definition(scene, counts)
    bufs, dispatches = E.pathtag_job(scene, counts)
    outputs = [k for k in bufs if k not in ("cfg", "scene")]
    with Job(engine, bufs) as job:
        held = job.run(dispatches)
        E.check_pathtag(held, want, counts, "held back")
        launches = kernel_launches(engine, job, dispatches)
        absorbed = counts["large"] and counts["scan1"] <= PT_ABSORB_MAX
        assert launches == (2 if not counts["large"] else 3 if absorbed else 4), (launches, counts["scan1"])
        for k in outputs:
            job.upload(k)  # poison again
        engine.profile(True)
        try:
            recorded = job.run(dispatches)
            labels = [nd["label"] for nd in engine.profile_collect_tree() if nd["kind"] == "query"]
        finally:
            engine.profile(False)
        assert labels == [d[0] for d in dispatches], labels
        E.check_pathtag(recorded, want, counts, "as recorded")
        for k in outputs:
            assert np.array_equal(held[k], recorded[k]), "the two routes differ in " + k
    print("%s: %.2f s" % (name, time.perf_counter() - t0))


@pytest.mark.parametrize("wgs", (256, 257))
def test_last_scan_in_flatten_on_both_sides_of_the_route_switch(engine, wgs):
    """The last scan as flatten absorbs it (k_flatten_classify<SCAN>) needs a real recording: one filled polygon of straight
    segments whose padded tag words make exactly 256 workgroups (pathtag_scan_small, the last size that takes it) and 257 (the first on
    the three-level route), asserted on the recording.  Each against the oracle buffer by buffer and pixel by pixel on the engine's
    own route and once more as recorded (profiler on), the two frames equal.  The oracle takes 0.4 s for either scene."""
    s, p = E.scene_of_tag_wgs(wgs)
    p.bump = s.bump_sizes(p.width, p.height)
    rec = jello_amd.Host().record(s, p)
    wg = rec.workgroup_counts()
    assert wg["path_reduce"][0] == wgs and wg["use_large_path_scan"] == (wgs == 257) and rec.config["n_path"] == 1
    held = compare(engine, s, p)
    engine.profile(True)
    try:
        recorded = compare(engine, s, p)
        labels = [nd["label"] for nd in engine.profile_collect_tree() if nd["kind"] == "query"]
    finally:
        engine.profile(False)
    assert ("pathtag_scan_large" if wgs == 257 else "pathtag_scan_small") in labels and ("pathtag_reduce2" in labels) == (wgs == 257)
    assert held["bump"] == recorded["bump"] and np.array_equal(held["image"], recorded["image"])


# ---- draw_reduce / draw_leaf -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.DRAW_COUNTS)
def test_draw_stages_on_tag_streams(engine, n):
    """Random 32-bit draw tags (every field pattern of map_draw_tag; draw_leaf writes no info for them) with nop, solid colour,
    begin-clip and end-clip mixed in at known positions, at object counts on both sides of one block, of 256 blocks (each workgroup
    walks one block, then several: base 0, 1, 2 and 3 with remainders 0, 1, 255 and 14).  draw_reduced, every draw monoid, the clip_inp
    records and the info words of the 0x50 objects -- and the poison between them -- against the definition and the oracle.
    n = 200 000: 0.04 s on the MI355X machine, the oracle included."""
    t0 = time.perf_counter()
    n_wgs = E.host_draw_counts(n)["draw_reduce"]
    bufs, dispatches, tags = E.draw_job(n, n_wgs)
    want = E.draw_by_definition(tags, bufs["path_bbox"], n_wgs, len(bufs["clip_inp"]), len(bufs["info"]))
    with Job(engine, bufs) as job:
        got = job.run(dispatches)
    E.check_draw(got, want, "gpu")
    E.check_draw(got, E.run_oracle(bufs, dispatches), "gpu against the oracle")
    print("draw %d: %.2f s" % (n, time.perf_counter() - t0))


# ---- binning / tile_alloc ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BINNING, ids=[c.name for c in BINNING])
def test_binning_on_hand_built_boxes(engine, case):
    """The rules of element_streams.binning_by_definition case by case: boxes on, inside and past a bin line, empty, inverted and
    cleared boxes, boxes outside the target, +-1e9, clip_ix 0 / n_clip / past it, 512 bins (those from 256 on are dropped), one element
    in every bin next to 255 in none, 1 .. 65 537 elements (257 workgroups: the loop over the workgroup totals), a bin_data one word
    too small for the last chunk, and flatten's failure on entry.  Intersected boxes bit for bit, all headers, the chunk lists,
    bump.binning and bump.failed.

    bins_512: the dispatcher refuses a binning dispatch whose config -- known to it from the upload of exactly sizeof(JlConfig) bytes
    -- has more than 256 bins (asserted here); the kernel's own rule is reached with the same config in a longer buffer."""
    bufs, dispatches = E.binning_job(case)
    if case.name == "bins_512":
        with Job(engine, bufs) as job:
            assert job.dispatch_rc(*dispatches[0]) == jello_amd.engine.JH_ERR_INVALID
            assert b"bins" in engine.hip.jh_last_error(engine.ctx)
        bufs["cfg"] = np.concatenate([bufs["cfg"], np.zeros(3, np.uint32)])
    want = E.binning_by_definition(case)
    with Job(engine, bufs) as job:
        got = job.run(dispatches)
    E.check_binning(got, want, case, "gpu")
    oracle = E.run_oracle(bufs, dispatches)
    for k in ("boxes", "headers", "bump"):
        assert np.array_equal(got[k], oracle[k]), "gpu against the oracle: " + k


@pytest.mark.parametrize("case", TILES, ids=[c.name for c in TILES])
def test_tile_alloc_on_hand_built_boxes(engine, case):
    """Both kernels of tile_alloc by the rules of element_streams.tile_alloc_by_definition: boxes on tile lines, a target that is no
    multiple of 16 px, nop and end-clip objects, 1 .. 65 537 objects, an even and an odd tile total (the clear stores two tiles at a
    time), tiles_size one tile too small and far too small, each failed bit on entry.  Path.bbox, Path.tiles, bump, and the tile
    buffer: exactly [0, min(total, tiles_size)) zero, poison from there on."""
    bufs, dispatches = E.tile_alloc_job(case)
    want = E.tile_alloc_by_definition(case)
    with Job(engine, bufs) as job:
        got = job.run(dispatches)
    E.check_tile_alloc(got, want, case, "gpu")


# ---- the look-back scan --------------------------------------------------------------------------------------------------------------------
COUNT_WORD, TOTAL_WORD = 3, 5


class Scan:
    """in / out / a buffer of eight words for the device-side count and the total, for scans of up to n_max elements."""

    def __init__(self, engine, n_max, stride):
        self.n_max, self.stride = n_max, stride
        self.job = Job(engine, {"in": np.zeros(max(n_max * stride, 4), np.uint32), "out": E.poisoned(n_max + 64), "misc": E.poisoned(8)})

    def __enter__(self):
        self.job.__enter__()
        return self

    def __exit__(self, *a):
        self.job.__exit__(*a)

    def load(self, values, count):
        self.values, self.count = values, count
        misc = E.poisoned(8)
        if count is not None:
            misc[COUNT_WORD] = count
        self.job.upload("in", values)
        self.job.upload("out")
        self.job.upload("misc", misc)

    def launch(self, n_max=None, total=True):
        e, ids = self.job.e, self.job.ids
        self.launched = (self.n_max if n_max is None else n_max, total)
        e._check(e.hip.jh_debug_scan_u32(e.ctx, ids["in"], ids["out"], self.stride, self.launched[0], ids["misc"] if self.count is not None else 0,
                                         COUNT_WORD, ids["misc"] if total else 0, TOTAL_WORD), "debug_scan_u32")

    def check(self, what):
        n_max, total = self.launched
        n = n_max if self.count is None else min(self.count, n_max)
        want, want_total = E.scan_u32(self.values, self.stride, n)
        self.job.e.sync()
        got = self.job.download(["out", "misc"])
        bad = np.flatnonzero(got["out"][:n] != want)
        assert bad.size == 0, "%s: %d of %d prefixes differ, first at %d: 0x%x want 0x%x" % (what, bad.size, n, bad[0], got["out"][bad[0]], want[bad[0]])
        assert np.all(got["out"][n:] == E.POISON), what + ": out was written from word n on"
        misc = E.poisoned(8)
        if self.count is not None:
            misc[COUNT_WORD] = self.count
        if total:
            misc[TOTAL_WORD] = want_total
        assert np.array_equal(got["misc"], misc), "%s: count / total words %s want %s" % (what, got["misc"], misc)


@pytest.mark.parametrize("n", E.SCAN_N)
def test_lookback_scan_at_tile_edges(engine, n):
    """jh_scan_u32 (k_scan_lookback) at 0, 1, a wave +-1, a tile of 16 384 +-1, two tiles +-1, and 64 * 16384 + 1 and 65 * 16384 +
    16385 elements -- more than 64 tiles, so a workgroup whose predecessors have not published an inclusive prefix yet looks back a
    second round of 64 descriptors; whether one does depends on the order the hardware runs the workgroups in and cannot be forced.
    Stride 1 (the vectorised path for full threads, the guarded one for the tail) and stride 2; random values of the full u32 range,
    so the sums wrap; the count on the device absent, 0, smaller than n_max by more than two tiles, equal to it and larger; the total
    asked for or not; all-ones and all-zero runs.  `out` is poisoned and must be untouched from word n on."""
    for stride in (1, 2):
        with Scan(engine, n, stride) as s:
            values = E.scan_values(n, stride, "random")
            counts = [None, 0, n, n + 1000] + ([n - 2 * E.LB_TILE - 77] if n > 3 * E.LB_TILE else []) + ([n - 1, n // 2] if 1 < n < 70000 else [])
            for count in counts:
                for total in ((True, False) if count in (None, 0) or count < n else (True,)):
                    s.load(values, count)
                    s.launch(total=total)
                    s.check("n_max %d stride %d count %s total %s" % (n, stride, count, total))
            for kind in ("ones", "zeros"):
                s.load(E.scan_values(n, stride, kind), None)
                s.launch()
                s.check("n_max %d stride %d %s" % (n, stride, kind))


def test_lookback_scan_leaves_its_state_clean(engine):
    """The kernel's last workgroup puts the descriptors and both counters back to zero, and the next launch on the same scratch slot
    relies on it: a large scan, a small one, a large one with another tile count, then one scan captured in a hipGraph and replayed
    three times on new inputs -- on one context, nothing reset in between, every result exact."""
    big, other = 65 * E.LB_TILE + 16385, 64 * E.LB_TILE + 1
    with Scan(engine, big, 1) as s:
        for k, (n, count) in enumerate(((big, None), (65, None), (other, None), (big, 40 * E.LB_TILE + 3), (1, None), (big, None))):
            s.load(E.scan_values(big, 1, "random") + np.uint32(k), count)
            s.launch(n_max=n)
            s.check("eager launch %d" % k)
        s.load(E.scan_values(big, 1, "random"), 50 * E.LB_TILE)
        engine._check(engine.hip.jh_graph_begin(engine.ctx), "graph_begin")
        try:
            s.launch()
        finally:
            g = ctypes.c_void_p()
            rc = engine.hip.jh_graph_end(engine.ctx, ctypes.byref(g))
        engine._check(rc, "graph_end")
        assert engine.graph_node_counts(g) == (1, 0)
        try:
            for k, count in enumerate((50 * E.LB_TILE, 3, big + 5)):
                s.load(E.scan_values(big, 1, "random") * np.uint32(2 * k + 3), count)
                engine.replay(g)
                s.check("replay %d" % k)
        finally:
            engine.graph_destroy(g)
        s.load(E.scan_values(big, 1, "random"), None)
        s.launch(n_max=other)
        s.check("eager launch after the replays")
