"""CPU: the oracle's fill coverage against the exact float64 reference of tests/exact_coverage.py, per pixel, on the
battery of tests/coverage_scenes.py in all three AA modes -- the checks and tolerances of tests/test_gpu_coverage.py
(see the table there), run on the oracle.  This pins more than test_invariants.test_coverage_matches_supersampling,
which stays as it is."""
import numpy as np
import pytest

from jello_amd import Host
from oracle.oracle_engine import OracleEngine

import coverage_scenes as C
from test_gpu_coverage import AAS, check, record

CASES = [(e.id, rule, aa, "plain") for e in C.BATTERY for rule in C.RULES for aa in AAS]
CASES += [(eid, rule, "area", v) for eid in C.VARIANT_ENTRIES for v in ("clip", "paint") for rule in C.RULES]


def oracle_alpha(entry, rule, aa, variant="plain"):
    rec = Host().record(entry.scene(rule, variant), entry.params(AAS[aa]))
    o = OracleEngine()
    o.run(rec)
    assert int(o.get(rec, "bumpBuf", np.uint32)[0]) == 0
    return o.target(rec).view(np.float16).astype(np.float64)[..., 3]


@pytest.mark.parametrize("eid,rule,aa,variant", CASES, ids=["-".join(c) for c in CASES])
def test_oracle_coverage(built, request, eid, rule, aa, variant):
    entry = C.BY_ID[eid]
    record(request, entry, aa, check(entry, rule, aa, oracle_alpha(entry, rule, aa, variant)))


def _fine_area_a(xmin0, xmax0):
    """fine.wgsl:847-856 for one pixel (i = 0), one binary32 operation at a time."""
    f = np.float32
    xmin = f(min(f(xmin0), f(1.0)) - f(1e-6))
    xmax = f(xmax0)
    b = min(xmax, f(1.0))
    c = max(b, f(0.0))
    d = max(xmin, f(0.0))
    return float(f(f(f(b + f(f(0.5) * f(f(d * d) - f(c * c)))) - xmin) / f(xmax - xmin)))


def test_fine_area_formula_is_exact_beside_and_on_pixel_aligned_edges():
    """The cancellation term of test_gpu_coverage is 0 for an edge on a pixel line and for the pixels beside a piece:
    a vertical edge at tile-relative k is at k - 1e-6 after path_tiling.wgsl:159-164 (1e-6 for k = 0), and fine's
    formula gives every pixel of the tile the exact fraction right of it, up to that 1e-6.  Left of any piece
    (xmin0 >= 1) the operands are constants and a is exactly 0; right of it (xmax0 <= 0) a is exactly 1."""
    f = np.float32
    for k in range(17):
        x = f(1e-6) if k == 0 else f(f(k) - f(1e-6))
        for px in range(16):
            u = f(x - f(px))
            assert abs(_fine_area_a(u, u) - min(max(px + 1 - float(x), 0.0), 1.0)) <= 1.1e-6, (k, px)
    rng = np.random.default_rng(3)
    for lo, span in zip(rng.uniform(1.0, 15.0, 200), rng.uniform(0.0, 3.0, 200)):
        assert _fine_area_a(f(lo), f(lo + span)) == 0.0
        assert _fine_area_a(f(-lo - span), f(-lo)) == 1.0


@pytest.mark.parametrize("eid", ["f1-pixel-lines", "f1-tile-lines"])
def test_errors_beside_pixel_aligned_edges_are_caught(built, eid):
    """The bound is tight beside edges on pixel and tile lines: 0.15 added to or taken from every pixel on either side
    of a vertical edge, in the rows it spans, fails the check."""
    entry = C.BY_ID[eid]
    alpha = oracle_alpha(entry, "nonzero", "area")
    check(entry, "nonzero", "area", alpha)
    (x0, y0), _, (x1, y1), _ = entry.contours[0]
    for x in (int(x0), int(x1)):
        for col, sign in ((x - 1, 1.0), (x, -1.0), (x - 1, -1.0), (x, 1.0)):
            if not 0 <= col < entry.width:
                continue
            bad = alpha.copy()
            bad[int(y0):int(y1), col] = np.clip(bad[int(y0):int(y1), col] + sign * 0.15, 0.0, 1.0)
            if np.array_equal(bad, alpha):
                continue
            with pytest.raises(AssertionError):
                check(entry, "nonzero", "area", bad)
