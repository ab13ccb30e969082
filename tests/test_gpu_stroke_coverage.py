"""-m gpu: per-pixel coverage of stroked polylines on the HIP image against the float64 stroker of tests/exact_stroke.py,
on the stroke battery of tests/coverage_scenes.py (families 11-15), in all three AA modes, through the check and the
tolerance table of tests/test_gpu_coverage.py (classes "stroke" and "stroke-xform", and the "arc" row for the lines of
round caps and joins).  Strokes are filled non-zero; nothing here renders them even-odd.  Every new entry also goes
through parity.compare (every buffer and the image, bit for bit against the oracle), and the line buffer of the round
entries is held to the arc rule itself: the number of lines per arc, every vertex within the derived f32 distance of
its float64 position, consecutive lines connected bit for bit.  tests/test_stroke_coverage_spec.py runs the same
checks on the oracle, together with the sensitivity tests that keep the check honest."""
import numpy as np
import pytest

from jello_amd import Host
from jello_amd.engine import RUN_DISPATCHES, RUN_UPLOADS

import coverage_scenes as C
from test_gpu_coverage import AAS, arc_term, check, f32_term, record, render

pytestmark = pytest.mark.gpu

CASES = [(e.id, aa, "plain") for e in C.STROKE_BATTERY for aa in AAS]
CASES += [(eid, aa, v) for eid in C.STROKE_VARIANT_ENTRIES for v in ("clip", "paint") for aa in AAS]
ROUND = [e.id for e in C.STROKE_BATTERY if e.outline().arcs]
# bit-for-bit parity in the MSAA modes too: cr == 0, the miter flip, 100 joins in a tile, arcs of 1 and of 61 lines
PARITY_MSAA = ["f13-collinear-miter", "f13-angle-28.9", "f13-angle-29", "f14-100-joins-one-tile", "f14-w0.3-round-join",
               "f14-round-cap-60-lines"]
ZERO_LENGTH = ("f14-zero-length-segment", "f14-zero-length-segment-removed")


def check_arc_lines(entry, lines):
    """`lines`: the line buffer, (n, 6) uint32 (path_ix, pad, p0, p1 as f32 bits).  For every arc of the reference: its
    n lines lie in consecutive slots, start at the arc's begin point, pass through its n - 1 rotated vertices and end
    at its exact end point, each vertex within f32_term + arc_term (per coordinate) of the float64 one, and line k ends
    on the very bits line k + 1 starts on.  A flattening with one line more or fewer cannot pass: the vertices are a
    chord apart.  Returns the largest vertex error in units of its bound."""
    pts = lines[:, 2:].copy().view(np.float32).astype(np.float64).reshape(-1, 2, 2)
    worst = 0.0
    for arc in entry.outline().arcs:
        tol = f32_term(entry) + arc_term(arc)
        v = arc.device
        assert arc.n == 1 or np.abs(v[1:] - v[:-1]).max(axis=1).min() > 4 * tol, "the vertices of this arc cannot be told apart"
        first = np.flatnonzero((np.abs(pts[:, 0] - v[0]).max(axis=1) <= tol) & (np.abs(pts[:, 1] - v[1]).max(axis=1) <= tol))
        assert len(first) >= 1, "%s: no line from %s to %s" % (entry.id, v[0], v[1])
        ok = False
        for j in first:            # (two arcs may share their first line: a cap and a join of a short segment)
            if j + arc.n > len(pts):
                continue
            chain = pts[j:j + arc.n]
            err = max(np.abs(chain[:, 0] - v[:-1]).max(), np.abs(chain[:, 1] - v[1:]).max())
            if err <= tol:
                assert np.array_equal(lines[j:j + arc.n - 1, 4:6], lines[j + 1:j + arc.n, 2:4]), \
                    "%s: the lines of the arc at slot %d are not connected bit for bit" % (entry.id, j)
                ok = True
                worst = max(worst, err / tol)
                break
        assert ok, "%s: no run of %d lines follows the arc from %s to %s within %.3g" % (entry.id, arc.n, v[0], v[-1], tol)
    return worst


def gpu_lines(engine, entry):
    rec = Host().record(entry.scene(), entry.params(AAS["area"]))
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    engine.sync()
    try:
        bump = engine.download(rec.buffer("bumpBuf")[0], dtype=np.uint32)
        assert int(bump[0]) == 0
        return engine.download(rec.buffer("linesBuf")[0], dtype=np.uint32)[:int(bump[7]) * 6].reshape(-1, 6)
    finally:
        engine.release(rec)


@pytest.mark.parametrize("eid,aa,variant", CASES, ids=["-".join(c) for c in CASES])
def test_stroke_coverage(engine, request, eid, aa, variant):
    entry = C.BY_ID[eid]
    record(request, entry, aa, check(entry, "nonzero", aa, render(engine, entry, "nonzero", aa, variant)))


@pytest.mark.parametrize("aa", list(AAS))
def test_zero_length_segment_is_dropped(engine, aa):
    """The encoder drops a zero-length line between two real ones: the image is the one of the path without it."""
    a, b = (render(engine, C.BY_ID[eid], "nonzero", aa, "plain") for eid in ZERO_LENGTH)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("eid", [e.id for e in C.STROKE_BATTERY])
def test_stroke_parity(engine, eid):
    """Every buffer (the line buffer included) and the image bit for bit against the oracle, area AA."""
    from parity import compare
    entry = C.BY_ID[eid]
    compare(engine, entry.scene(), entry.params(AAS["area"]))


@pytest.mark.parametrize("eid", PARITY_MSAA)
@pytest.mark.parametrize("aa", ["msaa8", "msaa16"])
def test_stroke_parity_msaa(engine, eid, aa):
    from parity import compare
    entry = C.BY_ID[eid]
    compare(engine, entry.scene(), entry.params(AAS[aa]))


@pytest.mark.parametrize("eid", ROUND)
def test_arc_lines_follow_the_arc_rule(engine, request, eid):
    entry = C.BY_ID[eid]
    worst = check_arc_lines(entry, gpu_lines(engine, entry))
    request.node.user_properties.append(("arc_vertex_max_share_of_bound", "%.3g" % worst))
