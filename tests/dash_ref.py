"""The dash rule of DESIGN.md 5.6 restated on the CPU, dash by dash, with no GPU and none of the project's native code.

The host route (jello_amd.dash) and the device stage (Engine.dash_paths) must equal `dash` byte for byte.  Arithmetic: Python
floats are IEEE binary64 and `+ - * /` and math.sqrt are correctly rounded, so every expression below is the fixed sequence the
rule names, written in the same order; numpy supplies the one rounding to binary32.  Integers are Python's (exact).

A path is a list of (kind, (six floats)) as jello_amd.Path.els holds it; so is the result.

`merge=False` and `closed_left=False` are deliberately wrong variants for the sensitivity tests (the merge of a closed subpath's
last and first dash removed; "on" intervals closed at their end instead of their start)."""
import bisect
import math

import numpy as np

MOVE, LINE, QUAD, CUBIC, CLOSE = 0, 1, 2, 3, 4
N_POINTS = {MOVE: 1, LINE: 1, QUAD: 2, CUBIC: 3, CLOSE: 0}
MAX_PANELS = 4096
SOLVE_ITERATIONS = 8
COORD_LIMIT, ENTRY_LIMIT, OFFSET_LIMIT = 2.0 ** 20, 2.0 ** 30, 2.0 ** 40
X = (0.06943184420297371, 0.33000947820757187, 0.6699905217924281, 0.9305681557970262)
W0, W1 = 0.17392742256872692, 0.3260725774312731


class Rejected(ValueError):
    pass


def q20(x):
    return round(x * 1048576.0)  # exact product, then ties-to-even


def f32(x):
    return float(np.float32(x))


# ---- one segment ----
class Seg:
    def __init__(self, kind, pts):
        self.kind, self.p = kind, [float(v) for v in pts] + [0.0] * (8 - len(pts))
        self.panels = panels(self)
        if self.panels == 0:
            dx, dy = self.p[2] - self.p[0], self.p[3] - self.p[1]
            self.cum = [0, round(math.sqrt(dx * dx + dy * dy) * 4294967296.0)]
        else:
            h = 1.0 / float(self.panels)
            self.cum = [0]
            for k in range(self.panels):
                self.cum.append(self.cum[-1] + round(panel_length(self, float(k) * h, h, 1.0) * 4294967296.0))
        self.q = (self.cum[-1] + 2048) >> 12


def panels(g):
    if g.kind == LINE:
        return 0
    p = g.p
    d2 = abs((p[0] - 2.0 * p[2]) + p[4]) + abs((p[1] - 2.0 * p[3]) + p[5])
    if g.kind == CUBIC:
        e = abs((p[2] - 2.0 * p[4]) + p[6]) + abs((p[3] - 2.0 * p[5]) + p[7])
        d2 = 6.0 * (e if e > d2 else d2)
    else:
        d2 = 2.0 * d2
    k = math.ceil(math.sqrt(64.0 * d2))
    return min(max(int(k), 1), MAX_PANELS)


def speed(g, t):
    p = g.p
    mt = 1.0 - t
    if g.kind == CUBIC:
        a, b, c = mt * mt, (mt * t) * 2.0, t * t
        dx = (a * (p[2] - p[0]) + b * (p[4] - p[2])) + c * (p[6] - p[4])
        dy = (a * (p[3] - p[1]) + b * (p[5] - p[3])) + c * (p[7] - p[5])
        return 3.0 * math.sqrt(dx * dx + dy * dy)
    dx = mt * (p[2] - p[0]) + t * (p[4] - p[2])
    dy = mt * (p[3] - p[1]) + t * (p[5] - p[3])
    return 2.0 * math.sqrt(dx * dx + dy * dy)


def panel_length(g, t0, h, u):
    hu = u * h
    s = [speed(g, t0 + hu * x) for x in X]
    return hu * (((W0 * s[0] + W1 * s[1]) + W1 * s[2]) + W0 * s[3])


def nominal_length(g, t):
    """L(t) as the rule evaluates it (user units): whole panels from the integer table, the rest of t's panel by the 4 points."""
    if g.panels == 0:
        return t * g.cum[-1] / 4294967296.0
    k = min(int(t * g.panels), g.panels - 1)
    h = 1.0 / float(g.panels)
    return g.cum[k] / 4294967296.0 + panel_length(g, float(k) * h, h, (t - float(k) * h) / h)


def inverse(g, s):
    """The parameter at which the segment has run s of its q units (2^-20), 0 < s < q."""
    if g.panels == 0:
        return float(s) / float(g.q)
    target = s << 12
    k = bisect.bisect_right(g.cum, target) - 1
    h = 1.0 / float(g.panels)
    t0 = float(k) * h
    tau = float(target - g.cum[k]) / 4294967296.0
    lo, hi = 0.0, 1.0
    u = tau / panel_length(g, t0, h, 1.0)
    for _ in range(SOLVE_ITERATIONS):
        if not (lo <= u <= hi):
            u = 0.5 * (lo + hi)
        r = panel_length(g, t0, h, u) - tau
        if r > 0.0:
            hi = u
        else:
            lo = u
        sp = speed(g, t0 + u * h) * h
        u = u - r / sp if sp > 0.0 else 2.0
    if not (lo <= u <= hi):
        u = 0.5 * (lo + hi)
    t = t0 + u * h
    return t if t < 1.0 else 1.0


def lerp(a, b, t):
    return b if t == 1.0 else a + (b - a) * t


def blossom(g, t1, t2, t3):
    out = []
    p = g.p
    for d in (0, 1):
        if g.kind == CUBIC:
            a, b, c = lerp(p[d], p[2 + d], t1), lerp(p[2 + d], p[4 + d], t1), lerp(p[4 + d], p[6 + d], t1)
            out.append(lerp(lerp(a, b, t2), lerp(b, c, t2), t3))
        elif g.kind == QUAD:
            out.append(lerp(lerp(p[d], p[2 + d], t1), lerp(p[2 + d], p[4 + d], t1), t2))
        else:
            out.append(lerp(p[d], p[2 + d], t1))
    return out


def el(kind, pts=()):
    pts = [f32(v) for v in pts]
    return (kind, tuple(pts + [0.0] * (6 - len(pts))))


def piece(g, ta, tb):
    if g.kind == CUBIC:
        return el(CUBIC, blossom(g, ta, ta, tb) + blossom(g, ta, tb, tb) + blossom(g, tb, tb, tb))
    if g.kind == QUAD:
        return el(QUAD, blossom(g, ta, tb, tb) + blossom(g, tb, tb, tb))
    return el(LINE, blossom(g, tb, tb, tb))


# ---- subpaths ----
def subpaths(path):
    """[(segments, closed)] -- MoveTo begins a subpath; drawing before the first MoveTo and a ClosePath with nothing open are
    ignored; after a ClosePath drawing goes on from the closed subpath's start."""
    subs, cur, start, segs = [], None, None, None
    for kind, pts in path:
        if kind not in N_POINTS:
            raise Rejected("unknown element kind")
        for v in pts[:2 * N_POINTS[kind]]:
            if not math.isfinite(v) or abs(v) > COORD_LIMIT:
                raise Rejected("coordinate")
        if kind == MOVE:
            if segs:
                subs.append((segs, False))
            cur = start = (float(pts[0]), float(pts[1]))
            segs = []
        elif kind == CLOSE:
            if segs:
                if cur != start:
                    segs.append(Seg(LINE, cur + start))
                subs.append((segs, True))
            segs = [] if cur is not None else None
            cur = start
        elif cur is not None:
            if not segs:
                start = cur
            n = 2 * N_POINTS[kind]
            segs.append(Seg(kind, cur + tuple(pts[:n])))
            cur = (float(pts[n - 2]), float(pts[n - 1]))
    if segs:
        subs.append((segs, False))
    return subs


def on_intervals(entries, phase, total, closed_left=True):
    """The dashes of a subpath of length `total` as integer intervals (a, b), clipped, ascending, adjacent ones joined."""
    period = sum(entries)
    out = []
    pos = -phase
    while pos < total or (not closed_left and pos == total):
        a = pos
        for i in range(0, len(entries), 2):
            b = a + entries[i]
            if closed_left:
                exists = b > a and a < total and b > 0          # [a, b) meets [0, total)
            else:
                exists = b > a and a < total and b >= 0         # (a, b] meets [0, total]  (the wrong variant)
            if exists:
                ca, cb = max(a, 0), min(b, total)
                if out and out[-1][1] == ca:
                    out[-1] = (out[-1][0], cb)
                else:
                    out.append((ca, cb))
            a = b + entries[i + 1]
        pos += period
    return out


def dash_subpath(segs, closed, entries, phase, merge=True, closed_left=True, trace=None):
    segs = [g for g in segs if g.q > 0]  # segments of quantised length 0 vanish
    starts, pos = [], 0
    for g in segs:
        starts.append(pos)
        pos += g.q
    total = pos
    if total == 0:
        return []
    dashes = on_intervals(entries, phase, total, closed_left)
    if not dashes:
        return []

    def pieces(a, b):
        out = []
        for g, s in zip(segs, starts):
            e = s + g.q
            if s < b and e > a:
                ta = 0.0 if a <= s else inverse(g, a - s)
                tb = 1.0 if b >= e else inverse(g, b - s)
                out.append((g, ta, tb))
                if trace is not None:  # (segment, its two parameters, the piece's nominal length in user units)
                    trace.append((g, ta, tb, (min(b, e) - max(a, s)) / 1048576.0))
        if not out:  # only the wrong variant gets here: an empty dash at the very start
            out.append((segs[0], 0.0, 0.0))
        return out

    def emit(parts, with_move=True):
        g, ta, _ = parts[0]
        out = [el(MOVE, blossom(g, ta, ta, ta))] if with_move else []
        return out + [piece(g, ta, tb) for g, ta, tb in parts]

    whole = closed and len(dashes) == 1 and dashes[0] == (0, total)
    if whole:
        return emit(pieces(0, total)) + [el(CLOSE)]
    merged = merge and closed and len(dashes) >= 2 and dashes[0][0] == 0 and dashes[-1][1] == total
    out = []
    for a, b in (dashes[1:] if merged else dashes):
        out += emit(pieces(a, b))
    if merged:
        out += emit(pieces(*dashes[0]), with_move=False)
    return out


def quantise_pattern(pattern, offset):
    pattern = [float(d) for d in pattern]
    if not 1 <= len(pattern) <= 64:
        raise Rejected("pattern length")
    if not math.isfinite(offset) or abs(offset) > OFFSET_LIMIT:
        raise Rejected("offset")
    for d in pattern:
        if not math.isfinite(d) or d < 0.0 or d > ENTRY_LIMIT:
            raise Rejected("pattern entry")
    entries = [q20(d) for d in pattern]
    if len(entries) & 1:
        entries = entries + entries
    period = sum(entries)
    if period == 0:
        raise Rejected("period")
    return entries, q20(float(offset)) % period


def dash(path, pattern, offset=0.0, merge=True, closed_left=True, trace=None):
    entries, phase = quantise_pattern(pattern, offset)
    out = []
    for segs, closed in subpaths(path):
        out += dash_subpath(segs, closed, entries, phase, merge, closed_left, trace)
    return out


def to_bytes(els):
    """The device's element format: {u32 kind, f32 p[6]}, 28 bytes each."""
    a = np.zeros(len(els), dtype=np.dtype([("kind", "<u4"), ("p", "<f4", 6)]))
    for i, (k, pts) in enumerate(els):
        a[i] = (k, pts)
    return a.tobytes()
