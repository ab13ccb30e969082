"""The battery of dash jobs shared by tests/test_dash_spec.py (host route against tests/dash_ref.py, no GPU) and
tests/test_gpu_dash.py (device stage against the same): the smallest shapes at which something can go wrong.

A case is (name, path, pattern, offset); a path is a list of (kind, (six floats)) as jello_amd.Path.els holds it."""
import math
import random

MOVE, LINE, QUAD, CUBIC, CLOSE = 0, 1, 2, 3, 4
Z = (0.0,) * 6


def M(x, y): return (MOVE, (float(x), float(y), 0.0, 0.0, 0.0, 0.0))
def L(x, y): return (LINE, (float(x), float(y), 0.0, 0.0, 0.0, 0.0))
def Q(x1, y1, x2, y2): return (QUAD, (float(x1), float(y1), float(x2), float(y2), 0.0, 0.0))
def C(x1, y1, x2, y2, x3, y3): return (CUBIC, (float(x1), float(y1), float(x2), float(y2), float(x3), float(y3)))
CL = (CLOSE, Z)


def polyline(points, closed=False):
    p = [M(*points[0])] + [L(*q) for q in points[1:]]
    return p + [CL] if closed else p


def square(x, y, s):
    return polyline([(x, y), (x + s, y), (x + s, y + s), (x, y + s)], closed=True)


# ---- curve families (seeded; also the accuracy test's) ----
def _cusp(size, sigma, rng):
    """A cubic with an exact cusp at t = 1/2, inside [0, size]^2, every coordinate perturbed by N(0, sigma) and clamped."""
    s = size
    pts = [(0.1 * s, 0.1 * s), (0.9 * s, 0.9 * s), (0.1 * s, 0.9 * s), (0.9 * s, 0.1 * s)]
    # B'(1/2) = 3/4 (d0 + 2 d1 + d2) = 3/4 ((p3 - p0) + (p2 - p1)): zero for these four points
    return [(min(max(x + rng.gauss(0.0, sigma), 0.0), size), min(max(y + rng.gauss(0.0, sigma), 0.0), size)) for x, y in pts]


def family(name, n, seed=1):
    """n curves of a family as (kind, [p0 .. pk]) with control points in [0, 4096]^2."""
    rng = random.Random(sum(map(ord, name)) + seed)
    out = []
    for i in range(n):
        if name == "cubic":
            out.append((CUBIC, [(rng.uniform(0, 4096), rng.uniform(0, 4096)) for _ in range(4)]))
        elif name == "quad":
            out.append((QUAD, [(rng.uniform(0, 4096), rng.uniform(0, 4096)) for _ in range(3)]))
        elif name == "arc":  # a circle arc of up to a quarter turn as one cubic
            r = rng.uniform(1.0, 2000.0)
            cx, cy = rng.uniform(r, 4096 - r), rng.uniform(r, 4096 - r)
            a0, da = rng.uniform(0, 2 * math.pi), rng.uniform(0.1, math.pi / 2)
            k = 4.0 / 3.0 * math.tan(da / 4)
            c0, s0, c1, s1 = math.cos(a0), math.sin(a0), math.cos(a0 + da), math.sin(a0 + da)
            out.append((CUBIC, [(cx + r * c0, cy + r * s0), (cx + r * (c0 - k * s0), cy + r * (s0 + k * c0)),
                                (cx + r * (c1 + k * s1), cy + r * (s1 - k * c1)), (cx + r * c1, cy + r * s1)]))
        elif name == "loop":  # the control polygon crosses itself: the curve has a loop
            x, y, s = rng.uniform(0, 2000), rng.uniform(0, 2000), rng.uniform(50, 2000)
            out.append((CUBIC, [(x, y), (x + s, y + s), (x, y + s), (x + s, y + rng.uniform(0, 0.3) * s)]))
        elif name == "nearline":
            x0, y0, x1, y1 = (rng.uniform(0, 4096) for _ in range(4))
            e = rng.choice([1e-9, 1e-3, 0.5])
            out.append((CUBIC, [(x0, y0), (min(x0 + (x1 - x0) / 3 + e, 4096.0), y0 + (y1 - y0) / 3),
                                (x0 + 2 * (x1 - x0) / 3, min(y0 + 2 * (y1 - y0) / 3 + e, 4096.0)), (x1, y1)]))
        elif name.startswith("cusp"):  # "cusp:<size>:<sigma>"
            _, size, sigma = name.split(":")
            out.append((CUBIC, _cusp(float(size), float(sigma), rng)))
        else:
            raise KeyError(name)
    return out


FAMILIES = ["cubic", "quad", "arc", "loop", "nearline"] + ["cusp:%s:%s" % (size, sigma) for size in ("4096", "40") for sigma in ("0.001", "1", "30")]


def curve_path(kind, pts):
    flat = [v for p in pts[1:] for v in p]
    return [M(*pts[0]), (kind, tuple(flat + [0.0] * (6 - len(flat))))]


def cases():
    out = []
    add = lambda name, path, pattern, offset=0.0: out.append((name, path, list(pattern), float(offset)))
    line12 = polyline([(0, 0), (12, 0)])
    add("line12_boundary_on_end", line12, [4, 2])
    # 3-4-5 triangle legs: every vertex sits exactly on a dash boundary
    add("345_vertices_on_boundaries", polyline([(0, 0), (3, 0), (3, 4), (0, 0)]), [3, 4, 5, 0.5])
    add("345_vertex_on_dash_start", polyline([(0, 0), (3, 0), (3, 4), (0, 0)]), [2, 1])
    add("345_vertex_on_dash_end", polyline([(0, 0), (3, 0), (3, 4), (0, 0)]), [3, 1])
    for n in (3, 65, 257):  # one dash spanning n short segments
        add("span_%d" % n, polyline([(0.25 * i, (i % 2) * 0.25) for i in range(n + 3)]), [0.3 * (n + 1), 1000.0], 0.0)
    add("seg_1100_dashes", polyline([(1, 1), (1 + 1100 * 0.75, 1)]), [0.5, 0.25])
    add("cubic_1100_dashes", curve_path(CUBIC, [(0, 0), (400, 300), (800, -200), (1100, 100)]), [0.7, 0.4])
    add("sub_300_segments", polyline([(3.0 * i, 10.0 * math.sin(i)) for i in range(301)]), [7, 3, 1, 3], 2.5)
    many = []
    for i in range(70):
        many += polyline([(10 * i, 0), (10 * i + 5, 7), (10 * i + 9, 0)], closed=(i % 3 == 0))
    add("70_subpaths", many, [2.5, 1.5], 0.75)
    # closed subpaths, perimeter 16
    add("closed_merged", square(0, 0, 4), [3, 2], 1.0)             # on at 0 and reaching the end
    add("closed_merged_touching", square(0, 0, 4), [4, 4])         # the last dash ends exactly on the end, the first starts at 0
    add("closed_start_in_gap", square(0, 0, 4), [3, 2], 3.5)        # position 0 lies in a gap
    add("closed_merged_clipped_last", square(0, 0, 4), [3, 2])      # [0,3) ... [15,18) clipped to [15,16)
    add("closed_merged_last_ends_on_end", square(0, 0, 4), [5, 6])  # [0,5) [11,16)
    add("closed_end_in_gap", square(0, 0, 4), [5, 5.5])             # [0,5) [10.5,15.5): the end lies in a gap
    add("closed_run_starts_on_end", square(0, 0, 4), [4, 2, 4, 6])  # [0,4) [6,10): a run starts at 16 exactly, nothing reaches it
    add("closed_whole", square(0, 0, 4), [20, 3], 2.0)
    add("closed_whole_exact", square(0, 0, 4), [16, 3])
    add("closed_solid", square(0, 0, 4), [5, 0])
    add("closed_curve_merged", [M(10, 0), C(10, 5.5, 5.5, 10, 0, 10), C(-5.5, 10, -10, 5.5, -10, 0), C(-10, -5.5, -5.5, -10, 0, -10),
                                C(5.5, -10, 10, -5.5, 10, 0), CL], [4, 3], 2.0)
    add("closed_needs_closing_line", polyline([(0, 0), (4, 0), (4, 3)], closed=True), [2, 1], 0.5)
    add("draw_after_close", square(0, 0, 4) + [L(9, 9), L(9, 0)], [3, 1])
    # offsets
    add("offset_negative", line12, [4, 2], -1.0)
    add("offset_above_period", line12, [4, 2], 6 * 1000 + 1.5)
    add("offset_on_boundary", line12, [4, 2], 4.0)
    add("offset_on_dash_start", line12, [4, 2], 6.0)
    # patterns
    add("pattern_solid", line12 + [L(12, 5)], [5, 0])
    add("pattern_nothing", line12, [0, 5])
    add("pattern_odd_single", line12, [3])
    add("pattern_odd_three", polyline([(0, 0), (30, 0)]), [1, 2, 3])
    add("pattern_zero_off_inside", polyline([(0, 0), (30, 0)]), [1, 0, 2, 3])
    add("pattern_zero_on_inside", polyline([(0, 0), (30, 0)]), [1, 1, 0, 1])
    add("pattern_wraps_on", polyline([(0, 0), (30, 0)]), [2, 3, 1, 0], 0.5)  # the last on and the first on are one run across the period
    add("pattern_64", polyline([(0, 0), (300, 40)]), [0.5 + 0.125 * (i % 7) for i in range(64)], 3.0)
    add("pattern_63", polyline([(0, 0), (300, 40)]), [0.5 + 0.125 * (i % 5) for i in range(63)], 1.0)
    add("pattern_below_grid", line12, [2.0 ** -22, 1, 2])  # an entry that quantises to 0
    # degenerate input
    add("zero_length_segments", [M(1, 1), L(1, 1), L(5, 1), L(5, 1), Q(5, 1, 5, 1), L(5, 4), C(5, 4, 5, 4, 5, 4)], [1.5, 1])
    add("tiny_segment_vanishes", [M(0, 0), L(2.0 ** -22, 0), L(4, 0)], [1, 1])
    add("lone_moveto", [M(3, 3)], [1, 1])
    add("double_moveto", [M(3, 3), M(4, 4), L(9, 4), M(1, 1), M(2, 2)], [1, 1])
    add("empty_path", [], [1, 1])
    add("only_zero_length", [M(1, 1), L(1, 1), CL], [1, 1])
    add("no_moveto", [L(5, 5), L(9, 9)], [1, 1])
    add("mixed_kinds", [M(0, 0), L(10, 0), Q(15, 0, 15, 5), C(15, 10, 10, 15, 5, 15), L(0, 15), CL, M(20, 20), Q(30, 40, 40, 20)], [2.5, 1.25, 0.5, 1.25], 0.3)
    for fam in FAMILIES:
        size = float(fam.split(":")[1]) if fam.startswith("cusp") else 4096.0
        for i, (kind, pts) in enumerate(family(fam, 2)):
            add("%s_%d" % (fam, i), curve_path(kind, pts), [size / 37.0, size / 91.0], size / 300.0)
    return out


def batch_cases():
    """300 paths for one call, element counts around 64 and 256 among them: [(path, pattern, offset)]."""
    rng = random.Random(5)
    out = []
    counts = [63, 64, 65, 255, 256, 257]
    for i in range(300):
        n = counts[i] if i < len(counts) else rng.randint(1, 9)
        pts = [(rng.uniform(0, 64), rng.uniform(0, 64)) for _ in range(n)]
        path = [M(*pts[0])]
        for j, p in enumerate(pts[1:]):
            if i % 4 == 1 and j % 3 == 0:
                path.append(Q(rng.uniform(0, 64), rng.uniform(0, 64), *p))
            elif i % 4 == 2 and j % 3 == 0:
                path.append(C(rng.uniform(0, 64), rng.uniform(0, 64), rng.uniform(0, 64), rng.uniform(0, 64), *p))
            else:
                path.append(L(*p))
        if i % 5 == 4 and n > 2:
            path.append(CL)
        assert len(path) == n + (1 if (i % 5 == 4 and n > 2) else 0)
        pattern = [rng.choice([0.5, 1.0, 2.5, 4.0]) for _ in range(rng.randint(1, 4))]
        out.append((path, pattern, rng.uniform(-5, 20)))
    return out
