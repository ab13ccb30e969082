"""k_flatten_items cuts its item list into units of 64 -- the heavy items (Euler jobs: curves) first, then the light ones (lines,
caps, joins), never both in one unit -- and groups of workgroups take the units one at a time from a counter they share
(kernels_flatten.hip, "Work distribution").  Which wave runs which unit is decided by the order the waves arrive in; the line
buffer must not depend on it.  The arithmetic has its edges where a count crosses a multiple of 64 or of what one round of waves
takes.  With the whole grid a round is 262 144 jobs; bit 3 of jh_debug_flatten_regions runs the kernel as ONE workgroup (four
waves on one counter, a round of 256 jobs), which puts the same edges at scene sizes the oracle renders in milliseconds.  Every
case: every buffer of the pipeline (the line buffer and the bump allocators among them) and the image, bit for bit against the
oracle, which knows nothing of batches."""
import math

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Fill, Path, RenderParams, Scene, scenes
from parity import compare

pytestmark = pytest.mark.gpu

ONE_WG = 8  # jh_debug_flatten_regions bit 3
REGIONS = 1 | 2 | 4  # every wave starts in region 0, eight regions, batches allocate job by job


def classify(rec):
    """(heavy, light) item counts of a recording by the rule of k_flatten_classify: a curved segment of a fill is one heavy item,
    a line of a fill one light item; a stroke's segment gives two offset curves (heavy) and a join (light), or three light
    items if it is a line; the marker segment that ends a stroked subpath gives a cap (light) if it is curved."""
    cfg = rec.config
    scene = np.frombuffer([c for c in rec.commands() if c["buf_name"] == "scene" and c["data"]][0]["data"], np.uint32)
    tags = scene[cfg["pathtag_base"]:cfg["pathdata_base"]].view(np.uint8).astype(np.uint32)
    styles_before = np.cumsum((tags & 0x40) != 0) - ((tags & 0x40) != 0)
    seg = tags & 3
    has_seg = seg != 0
    flags = np.zeros(tags.size, np.uint32)
    flags[has_seg] = scene[cfg["style_base"] + 2 * styles_before[has_seg] - 2]
    stroke = (flags & 0x80000000) != 0
    curved, end = has_seg & (seg != 1), (tags & 4) != 0
    line = has_seg & ~curved
    heavy = int(np.sum(curved & ~stroke)) + 2 * int(np.sum(curved & stroke & ~end))
    light = int(np.sum(line & ~stroke)) + int(np.sum(curved & stroke & end)) + int(np.sum(curved & stroke & ~end)) + 3 * int(np.sum(line & stroke & ~end))
    return heavy, light


def run(scene, params, flags, heavy=None, light=None):
    params.bump = scene.bump_sizes(params.width, params.height)
    got = classify(jello_amd.Host().record(scene, params))
    if heavy is not None:
        assert got[0] == heavy, got
    if light is not None:
        assert got[1] == light, got
    eng = jello_amd.Engine(0)  # (an engine of its own: the debug flags must not outlive the case)
    try:
        assert eng.hip.jh_debug_flatten_regions(eng.ctx, flags) == 0
        r = compare(eng, scene, params)
        assert r["bump"]["failed"] == 0 and r["bump"]["lines"] > 0
        return r
    finally:
        eng.close()


@pytest.mark.parametrize("flags", [ONE_WG, ONE_WG | REGIONS])
@pytest.mark.parametrize("n", [1, 4, 5, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 1025])
def test_boundary_counts_with_one_workgroup(n, flags):
    """Unstroked C3 shapes: one Euler job per shape and one light item (the line that closes the fill), so n_heavy = n_light = n.
    Four waves: less than one unit, exactly one, one item more; 1, 2, 3 and 5 rounds of 64-job batches, a last unit shorter than
    the rest, and counts that are an exact multiple of rounds * waves (256, 512).  With the region flags every allocation of
    the batches also takes the fallback routes."""
    s, p = scenes.scene_c3(n, 256, stroked=False)
    run(s, p, flags, heavy=n, light=n)


@pytest.mark.parametrize("n", [100, 171])
def test_stroked_shapes_with_one_workgroup(n):
    """Fill and stroke: three heavy items per shape (300 and 513) and their light items behind them -- the boundary between the
    last heavy unit and the first light chunk, which never share a batch."""
    s, p = scenes.scene_c3(n, 256)
    heavy, light = classify(jello_amd.Host().record(s, p))
    assert heavy == 3 * n and light >= n
    run(s, p, ONE_WG)


def polygon_scene():
    s = Scene()
    pts = [(128 + 100 * math.cos(2.4 * k + 0.1), 128 + 100 * math.sin(2.4 * k + 0.1)) for k in range(70)]
    path = Path().move_to(*pts[0])
    for x, y in pts[1:]:
        path.line_to(x, y)
    path.close()
    s.fill(Fill.NonZero, None, Brush.solid((0.2, 0.6, 0.9, 0.8)), None, path)
    return s, RenderParams(256, 256)


def closed_curves_scene():
    """Closed outlines of cubics only: the last curve returns to the start point, so no closing line is encoded."""
    s = Scene()
    for k in range(90):
        x, y = 20.0 + 24.0 * (k % 10), 20.0 + 24.0 * (k // 10)
        path = Path().move_to(x, y).cubic_to(x + 30, y - 12, x + 25, y + 31, x + 8, y + 18).cubic_to(x - 9, y + 22, x - 14, y + 3, x, y)
        s.fill(Fill.EvenOdd if k % 3 == 0 else Fill.NonZero, None, Brush.solid((k / 90.0, 0.5, 1.0 - k / 90.0, 0.7)), None, path)
    return s, RenderParams(256, 256)


@pytest.mark.parametrize("flags", [ONE_WG, 0])
@pytest.mark.parametrize("which", ["no_heavy", "no_light"])
def test_one_kind_of_item_only(which, flags):
    """A frame without a single Euler job (a polygon of straight segments: zero rounds, the light chunks start at unit 0) and one
    without a single light item (closed outlines of cubics only)."""
    if which == "no_heavy":
        s, p = polygon_scene()
        heavy, light = classify(jello_amd.Host().record(s, p))
        assert heavy == 0 and light >= 70
        run(s, p, flags)
    else:
        s, p = closed_curves_scene()
        run(s, p, flags, heavy=180, light=0)


def test_full_grid_below_one_round():
    """60 000 jobs on the whole grid: 938 heavy units and as many light ones, less than one per wave -- most waves find their
    group's counter past the end at once."""
    s, p = scenes.scene_c3(20000, 1024)
    run(s, p, 0, heavy=60000)
