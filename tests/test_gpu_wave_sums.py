"""-m gpu: path_count's crossing bases from ONE sum per wave of 64 lines (k_pc_count -> the u32 scan over the wave sums -> k_pc_emit,
which adds the prefix inside the wave from the counts it derives itself), against the oracle through parity.compare: every buffer of
the frame, bump first.

The scenes are closed polylines of straight lines, so the line count is exact: a filled polygon of k vertices is k lines in canonical
order, v0->v1, ..., v(k-1)->v0 (the encoder closes every filled subpath), and the paths' lines follow each other in path order.  Every
case asserts bump.lines against the count it aims at.

The counts sit on both sides of a wave (64 lines), of a workgroup (256 lines = 4 wave sums) and of 16 384 lines (64 workgroups, 256
wave sums).  What they do NOT reach: the kernels' grids are sized by the line buffer's capacity, 8 workgroups per CU at the most for
k_pc_count and 32 for k_pc_emit, so a wave strides to a second batch of lines only above 524 288 resp. 2 097 152 lines on a 256-CU
device; and the wave sums of these frames fit one tile of the look-back scan (16 384 sums = 1 048 576 lines).  Both are the full-size C3
frame of test_gpu_parity.py (3.3 M lines: 52 K wave sums, 4 tiles, every wave of both kernels strides).

The counts asked for were 0, 1, 63, ...; COUNTS has 2 where that list has 1.  A frame of one line cannot be had from a scene: the
encoder drops zero-length segments and closes every filled subpath, so the smallest one is the out-and-back pair A->B, B->A (two lines),
and a stroked segment is at least four.  The case of one line is therefore NOT covered here."""
import numpy as np
import pytest

import jello_amd
from jello_amd import BumpSizes
from jello_amd.engine import RUN_DISPATCHES, RUN_UPLOADS
from element_streams import ArrayPath
from oracle.oracle_engine import OracleEngine
from parity import BUMP, compare

pytestmark = pytest.mark.gpu
SIZE = 512
PC_LONG_LINE, PC_BIG_PATH = 32, 64  # kernels_tile.hip


def saw(k, x0, y0, step=1.5, h=5.0):
    """k vertices of a sawtooth: a closed polygon of k lines, each about one tile crossing, the closing line a few."""
    i = np.arange(k)
    return np.stack([x0 + i * step, y0 + (i % 2) * h], axis=1).astype(np.float64)


def scene_of(polygons, size=SIZE):
    s = jello_amd.Scene()
    for j, pts in enumerate(polygons):
        s.fill(jello_amd.Fill.NonZero if j % 2 else jello_amd.Fill.EvenOdd, None,
               jello_amd.Brush.solid((0.2 + 0.1 * (j % 7), 0.9 - 0.1 * (j % 5), 0.5, 0.7)), None, ArrayPath(pts, close=True))
    p = jello_amd.RenderParams(size, size, base_color=(0.1, 0.1, 0.1, 1.0))
    p.bump = BumpSizes(lines=1 << 16, seg_counts=1 << 18, segments=1 << 18, ptcl=1 << 20)
    return s, p


def split(n, per=37):
    """n lines as paths of `per` lines (the last one takes the rest; no path has fewer than two)."""
    sizes = [per] * (n // per)
    rest = n - per * len(sizes)
    if rest >= 2 or not sizes:
        sizes += [rest] if rest else []
    else:
        sizes[-1] += rest
    assert sum(sizes) == n and all(k >= 2 for k in sizes), sizes
    return sizes


def grid_polygons(sizes, size=SIZE):
    """One sawtooth per entry, laid out left to right, top to bottom, rows 8 px apart (neighbours overlap: they are separate paths)."""
    out, x, y = [], 2.0, 2.0
    for k in sizes:
        w = k * 1.5
        if x + w > size - 2.0 and x > 2.0:
            x, y = 2.0, y + 8.0
        if x + w > size - 2.0:  # a path longer than a row: a smaller step
            out.append(saw(k, 2.0, y, step=(size - 4.0) / k))
            y += 8.0
            continue
        out.append(saw(k, x, y))
        x += w + 3.0
    assert y + 8.0 < size, "the polygons do not fit"
    return out


def run(engine, polygons, lines, **kw):
    s, p = scene_of(polygons)
    r = compare(engine, s, p, **kw)
    assert r["bump"]["lines"] == lines, (r["bump"], lines)
    return r


COUNTS = [0, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 16383, 16384, 16385]


@pytest.mark.parametrize("n", COUNTS)
def test_line_counts_at_wave_and_workgroup_edges(engine, n):
    """n lines in paths of 37 (so path boundaries fall on every lane in turn), the whole frame against the oracle."""
    polys = grid_polygons(split(n)) if n else []
    r = run(engine, polys, n)
    assert (r["bump"]["seg_counts"] > 0) == (n > 0)


@pytest.mark.parametrize("sizes", [[64, 64, 64, 64], [65, 64, 64, 63], [63, 64, 64, 65], [128, 2, 62, 64]], ids=lambda s: "-".join(map(str, s)))
def test_path_boundaries_on_lanes_0_and_63(engine, sizes):
    """A path whose first line is line 64 k and whose last is line 64 k + 63, and the same shifted by one line either way: the ranges
    k_pc_emit writes at a path's first and last line use the neighbour lane or the line next door."""
    run(engine, grid_polygons(sizes), sum(sizes))


def long_triangle():
    """3 lines: a diagonal of 32 + 18 tile crossings (> PC_LONG_LINE: handed to the whole wave), a short one, the long way back."""
    return np.array([[5.0, 5.0], [505.0, 300.0], [500.0, 306.0]])


@pytest.mark.parametrize("before", [64, 63, 128 + 63], ids=["lane0", "lane63", "lane63_wave2"])
def test_a_long_line_in_lane_0_and_in_lane_63(engine, before):
    """The long line's base is the wave sum in front plus the lanes below it; the lines behind it are shifted by its 50 crossings."""
    polys = grid_polygons(split(before, per=before)) + [long_triangle()] + [saw(40, 10.0, 400.0)]
    r = run(engine, polys, before + 3 + 40)
    assert r["bump"]["seg_counts"] > before + 2 * PC_LONG_LINE


def test_a_line_without_crossings_in_lane_63(engine):
    """Line 63 of the frame lies below the target: outside its path's tile box, no crossings, and its lane must add nothing to the
    prefix of the wave behind it."""
    pts = saw(100, 4.0, SIZE - 20.0, step=3.0)
    pts[63, 1], pts[64, 1] = SIZE + 60.0, SIZE + 70.0
    run(engine, [pts, saw(30, 10.0, 100.0)], 130)


def test_a_big_path_still_finds_its_bases(engine):
    """One path above PC_BIG_PATH crossings (the list route: arrival slots, list bases, k_pc_rank) between small ones."""
    polys = [saw(30, 10.0, 50.0), saw(200, 10.0, 100.0, step=2.0), saw(30, 10.0, 150.0)]
    r = run(engine, polys, 260)
    assert r["bump"]["seg_counts"] > PC_BIG_PATH + 60


def frame_bump(engine, rec):
    return engine.download(rec.buffer("bumpBuf")[0], dtype=np.uint32)[:8].copy()


def test_upstream_failure_counts_nothing(engine):
    """A line buffer too small for the scene: flatten raises its bit in bump.failed, path_count is dispatched with a count of 0 --
    no wave holds lines, the scan's total is 0 -- and bump is the oracle's, seg_counts == 0."""
    s, p = scene_of(grid_polygons(split(300)))
    p.bump = BumpSizes(lines=128, seg_counts=1 << 12, segments=1 << 12, ptcl=1 << 20)
    rec = jello_amd.Host().record(s, p)
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        engine.sync()
        got = frame_bump(engine, rec)
        orc = OracleEngine()
        orc.run(rec)
        want = orc.get(rec, "bumpBuf", np.uint32)[:8]
    finally:
        engine.release(rec)
    assert list(got) == list(want), (dict(zip(BUMP, got)), dict(zip(BUMP, want)))
    assert got[0] != 0 and got[7] == 300 and got[4] == 0, dict(zip(BUMP, got))


def test_captured_frame_replays_to_the_same_crossings(engine):
    """The wave sums, their count and their scan are written before they are read in every frame: three replays of a captured
    frame (with an eager frame of another size in between) give the eager frame's segCountsBuf, Tiles and bump."""
    s, p = scene_of(grid_polygons(split(1000)) + [long_triangle()])
    so, po = scene_of(grid_polygons(split(129)))
    host = jello_amd.Host()
    rec, other = host.record(s, p), host.record(so, po)

    def frame():
        b = frame_bump(engine, rec)
        segc = engine.download(rec.buffer("segCountsBuf")[0], dtype=np.uint32)[:2 * int(b[4])].copy()
        tiles = engine.download(rec.buffer("tileBuf")[0], dtype=np.uint32)[:2 * int(b[3])].copy()
        return b, segc, tiles
    try:
        engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
        engine.sync()
        want = frame()
        assert want[0][0] == 0 and want[0][7] == 1003 and want[0][4] > 1003
        g = engine.capture(rec)
        engine.run(other, RUN_UPLOADS | RUN_DISPATCHES)
        for _ in range(3):
            engine.replay(g)
            engine.sync()
            got = frame()
            for name, a, b in zip(("bump", "segCountsBuf", "tileBuf"), got, want):
                assert np.array_equal(a, b), name
            engine.run(other, RUN_DISPATCHES)
        engine.sync()
        engine.graph_destroy(g)
    finally:
        engine.release(rec)
        engine.release(other)
