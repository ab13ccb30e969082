"""Hand-written per-tile command lists (PTCL) for the fine stage's layer machinery: a builder, an eager reference interpreter and
the battery the stage tests send through fine alone (tests/test_layer_streams_spec.py on the oracle,
tests/test_gpu_layer_streams.py on the device).

The kernel does not execute layers the way fine.wgsl does: BEGIN_CLIP only counts, a layer closed while still pending takes a
shortcut, a run of empty layers carries a memo and is counted on the register window, and the stack has three tiers.  The
interpreter here knows none of that.  It is fine.wgsl:938-973 as written: BEGIN_CLIP pushes the colour so far and starts from
zero, END_CLIP pops and blends `rgba * area * alpha` into what was saved.  Every IEEE operation is one numpy float32 operation;
the blend is composite_ref.blend_mix_compose, a FILL's area fine_by_hand.fill_area per pixel, COLOR fine_by_hand.over and the
store fine_by_hand.store_rgba16f (the two scalar functions are evaluated once per distinct pixel state of the tile).  Nothing is
shared with oracle/oracle.cpp or the kernel, and no constant of the kernel (window length, trip length, tier sizes) is used:
the battery reaches the phases and tiers by sweeping.

Commands are tuples: ("solid",) ("color", r, g, b, a) ("fill", segments, backdrop, even_odd) ("begin",) ("end", word, alpha)
("jump",) ("END",).  Colour channels and alpha are floats or U(bits): raw binary32 patterns, premultiplied.  Segments are
(p0x, p0y, p1x, p1y, y_edge) in tile-relative coordinates.  ("jump",) continues the list in a fresh chunk behind the heads; the
builder also jumps by itself wherever a head or a chunk is full, as coarse does.

Backdrops the command set can and cannot produce (group B):
  * a colour channel of -0 IS reachable: COLOR(-0, -0, -0, 2) over the transparent base gives +0 * (1 - 2) + -0 = -0 + -0 = -0;
  * an ALPHA of -0 is not reachable through COLOR: fg.a = -0 makes k = 1 - (-0) = 1 and +0 * 1 + -0 = +0, and any other fg.a is
    not -0; it is not reachable through END_CLIP with source-over either (src.a + bg.a * (1 - src.a) has a +0 term whenever the
    layer started from zero).  It needs a base colour of -0, which a command list cannot set;
  * a backdrop whose bit pattern is exactly 0x41800000 / 0x41800001, negative channels, colour above alpha and alpha 0 under a
    colour are all reachable as COLOR words over the transparent base (+0 * k + c = c for finite k), in single pixels through a
    FILL of two vertical segments on pixel edges, whose area is exactly 1 in one pixel and exactly 0 elsewhere;
  * NaN or inf in ALL pixels is a COLOR word; in ONE pixel it is not (fg * area is NaN wherever the area is 0), so the one-pixel
    cases are made from finite words: 3e38 in the pixel, a COLOR of alpha 3 (k = -2) makes it -inf there alone, a COLOR of alpha
    1 (k = 0) makes that NaN;
  * an ALPHA of inf is not reachable: COLOR with fg.a = inf has k = -inf, and +0 * -inf is NaN in every channel.  The NaN
    backdrops cover what it turns into.
"""
import functools

import numpy as np

import composite_ref
import fine_by_hand

F = np.float32
HEAD_WORDS = 64      # JL_PTCL_INITIAL_ALLOC (include/jello_formats.h): a tile's head is at tile_ix * 64
CHUNK_WORDS = 256    # JL_PTCL_INCREMENT: what coarse allocates per continuation
STACK_SPLIT = 4      # JL_BLEND_STACK_SPLIT: levels from here on live in blend_spill
TILE_PIXELS = 256
TILES_X = TILES_Y = 8
TILES = TILES_X * TILES_Y
TAG = {"END": 0, "fill": 1, "solid": 3, "color": 5, "begin": 10, "end": 11, "jump": 12}
WORDS = {"END": 1, "fill": 4, "solid": 1, "color": 5, "begin": 1, "end": 3, "jump": 2}


class U(int):
    """A raw binary32 bit pattern where a command takes a float."""


def bits(x):
    if isinstance(x, U):
        return int(x) & 0xffffffff
    return int(np.float32(x).view(np.uint32))


def f32_of(x):
    return np.uint32(bits(x)).view(np.float32)


class Stream:
    def __init__(self, name, group, cmds, finite=True):
        self.name, self.group, self.cmds, self.finite = name, group, tuple(cmds), finite

    @property
    def has_fill(self):
        return any(c[0] == "fill" for c in self.cmds)

    @property
    def depth(self):
        d = top = 0
        for c in self.cmds:
            if c[0] == "begin":
                d += 1
                top = max(top, d)
            elif c[0] == "end":
                d -= 1
        return top

    def __repr__(self):
        return "Stream(%s)" % self.name


# ---- builder ------------------------------------------------------------------------------------------------------------------
def spill_entries(stream):
    return max(stream.depth - STACK_SPLIT, 0) * TILE_PIXELS


class Frame:
    """Up to 64 streams laid out as the three buffers fine reads: ptcl (uint32 words), segments (float32 [n, 6]) and the
    blend_offset of every tile; `spill_entries` is what blend_spill has to hold."""

    def __init__(self, streams):
        assert 0 < len(streams) <= TILES
        self.streams = list(streams)
        words = [0] * (TILES * HEAD_WORDS)
        segs = []
        spill = 0
        self.blend_offsets = []
        for t in range(TILES):
            base = t * HEAD_WORDS
            if t >= len(self.streams):
                words[base] = spill
                words[base + 1] = TAG["END"]
                spill += 1
                continue
            st = self.streams[t]
            # (distinct per tile, (depth - 4) * 256 entries each, and one entry of distance even between tiles that need none)
            words[base] = spill
            self.blend_offsets.append(spill)
            spill += spill_entries(st) + 1
            pos, limit = base + 1, base + HEAD_WORDS
            for c in st.cmds:
                kind = c[0]
                if kind == "jump" or pos + WORDS[kind] + WORDS["jump"] > limit:
                    new = len(words)
                    words += [0] * CHUNK_WORDS
                    words[pos], words[pos + 1] = TAG["jump"], new
                    pos, limit = new, new + CHUNK_WORDS
                    if kind == "jump":
                        continue
                if kind == "fill":
                    words[pos:pos + 4] = [TAG["fill"], (len(c[1]) << 1) | (1 if c[3] else 0), len(segs), c[2] & 0xffffffff]
                    segs += [tuple(s) for s in c[1]]
                elif kind == "color":
                    words[pos:pos + 5] = [TAG["color"]] + [bits(v) for v in c[1:5]]
                elif kind == "end":
                    words[pos:pos + 3] = [TAG["end"], int(c[1]), bits(c[2])]
                else:
                    words[pos] = TAG[kind]
                pos += WORDS[kind]
        self.ptcl = np.array(words, np.uint32)
        self.segments = np.zeros((max(len(segs), 1), 6), np.float32)
        for i, s in enumerate(segs):
            self.segments[i, :5] = s
        self.spill_entries = spill


def validate(frame, ptcl_words=None, spill_capacity=None, segment_capacity=None):
    """What a stream must satisfy before it goes anywhere near a GPU: every jump forward and inside the buffer, every list ends
    in END, every END_CLIP closes an open layer, every spill index and every segment inside the sized buffers, every tag known.
    Walks the placed words, not the tuples: it checks what fine will read.  Raises AssertionError."""
    ptcl = frame.ptcl
    n = len(ptcl) if ptcl_words is None else ptcl_words
    assert len(ptcl) <= n, "the PTCL image does not fit the buffer"
    cap = frame.spill_entries if spill_capacity is None else spill_capacity
    seg_cap = frame.segments.shape[0] if segment_capacity is None else segment_capacity
    assert frame.segments.shape[0] <= seg_cap
    size = {v: WORDS[k] for k, v in TAG.items()}
    claimed = []
    for st in frame.streams:  # (the placed words end in END anyway where the padding is zero: the list itself has to say it)
        assert st.cmds and st.cmds[-1] == ("END",) and ("END",) not in st.cmds[:-1], "%s: no END at the end" % st.name
    for t in range(TILES):
        name = frame.streams[t].name if t < len(frame.streams) else "(idle tile %d)" % t
        pos = t * HEAD_WORDS
        blend_offset = int(ptcl[pos])
        pos += 1
        depth = top = 0
        for _ in range(1 << 16):
            assert 0 <= pos < len(ptcl), "%s: reads outside the PTCL at %d" % (name, pos)
            tag = int(ptcl[pos])
            assert tag in size, "%s: unknown tag %d at %d" % (name, tag, pos)
            assert pos + size[tag] <= len(ptcl), "%s: a command straddles the buffer's end" % name
            if tag == TAG["END"]:
                break
            if tag == TAG["jump"]:
                to = int(ptcl[pos + 1])
                assert pos < to < len(ptcl), "%s: jump from %d to %d" % (name, pos, to)
                pos = to
                continue
            if tag == TAG["begin"]:
                depth += 1
                top = max(top, depth)
            elif tag == TAG["end"]:
                assert depth > 0, "%s: END_CLIP at depth 0" % name
                depth -= 1
            elif tag == TAG["fill"]:
                n_segs, first = int(ptcl[pos + 1]) >> 1, int(ptcl[pos + 2])
                assert first + n_segs <= frame.segments.shape[0], "%s: segments outside the buffer" % name
            pos += size[tag]
        else:
            raise AssertionError("%s: no END" % name)
        need = max(top - STACK_SPLIT, 0) * TILE_PIXELS
        assert blend_offset + need <= cap, "%s: spill index %d outside %d" % (name, blend_offset + need, cap)
        claimed.append((blend_offset, blend_offset + need, name))
    claimed.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(claimed, claimed[1:]):
        assert a0 != b0 and a1 <= b0, "blend_offset of %s and %s overlap" % (an, bn)
    return True


# ---- reference interpreter ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fill_areas(segments, backdrop, even_odd):
    out = np.zeros(TILE_PIXELS, np.float32)
    with np.errstate(all="ignore"):
        for py in range(16):
            for px in range(16):
                out[py * 16 + px] = fine_by_hand.fill_area(segments, backdrop, px, py, even_odd)[0]
    out.setflags(write=False)
    return out


def _per_distinct(rows, fn, width, dtype):
    """fn on every distinct row of the (256, k) float32 array (compared as bit patterns), scattered back."""
    u = np.ascontiguousarray(rows, np.float32).view(np.uint32)
    distinct, inverse = np.unique(u, axis=0, return_inverse=True)
    vals = np.zeros((distinct.shape[0], width), dtype)
    with np.errstate(all="ignore"):
        for i, row in enumerate(distinct):
            vals[i] = fn(row.view(np.float32))
    return vals[np.asarray(inverse).reshape(-1)]


def _over(rgba, fg, area):
    rows = np.concatenate([rgba, area[:, None]], axis=1)
    return _per_distinct(rows, lambda r: fine_by_hand.over(r[:4], fg, r[4])[0], 4, np.float32)


def _store(rgba):
    return _per_distinct(rgba, lambda r: fine_by_hand.store_rgba16f(r)[0], 4, np.uint16)


VARIANTS = ("no_range_test", "no_lum_test", "memo_across_plus", "luminosity_shortcut", "compose_ignored", "fa_fb_swapped",
            "tier_off_by_one", "inner_saves_not_zero", "end_clip_area_one", "alpha3_is_solid", "neg_zero_alpha")


def _lum_ok(bg):
    """What the shortcut tests for hue / saturation / color: lum(cb) <= 1 in every pixel, with the full formula's operations."""
    with np.errstate(all="ignore"):
        inv = F(1.0) / composite_ref.fmax(bg[:, 3], composite_ref.EPSILON)
        lum = composite_ref._lum([bg[:, k] * inv for k in range(3)])
    return bool(np.all(lum.view(np.uint32) <= 0x3f800000))


def _range_ok(bg):
    return bool(np.all(bg.view(np.uint32) <= 0x41800000))


def _blend_factors_swapped(bg, src, word):
    """composite_ref.blend_mix_compose with the Porter-Duff factors Fa and Fb exchanged (a near miss)."""
    rule = composite_ref._FACTORS
    composite_ref._FACTORS = {k: (fb, fa) for k, (fa, fb) in rule.items()}
    try:
        return composite_ref.blend_mix_compose(bg, src, word)
    finally:
        composite_ref._FACTORS = rule


def run_tile(stream, variant=None, raw_before_last_end=False):
    """(16, 16, 4) uint16: the f16 bits fine stores for the tile, over a transparent base colour.  `variant`: one of VARIANTS, a
    near miss of the kernel's layer machinery expressed on this eager model (tests/test_layer_streams_spec.py says which stream
    tells each from the rule).  raw_before_last_end: instead, the (256, 4) float32 colour in front of the list's last END_CLIP
    (None if it has none) -- what that layer's backdrop really is."""
    assert variant is None or variant in VARIANTS
    rgba = np.zeros((TILE_PIXELS, 4), np.float32)
    area = np.zeros(TILE_PIXELS, np.float32)
    stack = []        # saved backdrops
    drawn = []        # per open layer: something was composited inside it (the variants' notion of "not empty")
    memo_lum = False  # (memo_across_plus) an empty hue / saturation / color layer passed its test earlier in the list
    last_end = max([i for i, c in enumerate(stream.cmds) if c[0] == "end"], default=None)
    with np.errstate(all="ignore"):
        for ci, c in enumerate(stream.cmds):
            kind = c[0]
            if kind == "solid":
                area = np.ones(TILE_PIXELS, np.float32)
            elif kind == "fill":
                area = _fill_areas(tuple(tuple(float(v) for v in s) for s in c[1]), int(c[2]), bool(c[3]))
            elif kind == "color":
                rgba = _over(rgba, [f32_of(v) for v in c[1:5]], area)
                drawn = [True] * len(drawn)
            elif kind == "begin":
                if variant == "inner_saves_not_zero" and drawn and not drawn[-1]:
                    stack.append(stack[-1].copy())  # (the pending inner level gets the colour, not the zeros it starts from)
                else:
                    stack.append(rgba)
                rgba = np.zeros((TILE_PIXELS, 4), np.float32)
                drawn.append(False)
            elif kind == "end":
                if raw_before_last_end and ci == last_end:
                    return stack[-1].copy()
                word, alpha = int(c[1]), f32_of(c[2])
                level = len(stack) - 1
                bg = stack.pop()
                empty = not drawn.pop()
                if variant == "tier_off_by_one" and level >= STACK_SPLIT + 1:
                    bg = stack[-1]  # (the slot of the level below)
                if variant == "neg_zero_alpha" and bits(alpha) == 0x80000000:
                    alpha = F(0.0)
                a_src = np.ones(TILE_PIXELS, np.float32) if variant == "end_clip_area_one" else area
                src = (rgba * a_src[:, None]) * alpha
                if variant == "compose_ignored":
                    word &= ~0xff
                mixm, srcover = (word >> 8) & 0xff, (word & 0xff) == 0
                alpha_ok = bits(alpha) < 0x7f800000
                shortcut = False
                if empty and srcover and alpha_ok:
                    if variant == "no_range_test" and 1 <= mixm <= 14:
                        shortcut = mixm < 12 or _lum_ok(bg)
                    if variant == "no_lum_test" and 12 <= mixm <= 14:
                        shortcut = _range_ok(bg)
                    if variant == "luminosity_shortcut" and mixm == 15:
                        shortcut = _range_ok(bg) and _lum_ok(bg)
                    if variant == "memo_across_plus" and 12 <= mixm <= 14:
                        if memo_lum:
                            shortcut = True
                        elif _range_ok(bg) and _lum_ok(bg):
                            memo_lum = True
                if shortcut:
                    rgba = bg
                elif variant == "fa_fb_swapped":
                    rgba = _blend_factors_swapped(bg, src, word)
                else:
                    rgba = composite_ref.blend_mix_compose(bg, src, word)
                if not empty or not shortcut:
                    drawn = [True] * len(drawn)
                if variant == "alpha3_is_solid" and bits(c[2]) == 3:
                    area = np.ones(TILE_PIXELS, np.float32)  # (the alpha word taken for a tag of its own)
            elif kind == "END":
                break
        if raw_before_last_end:
            return None
        return _store(rgba).reshape(16, 16, 4)


@functools.lru_cache(maxsize=None)
def _expected_cached(stream):
    out = run_tile(stream)
    out.setflags(write=False)
    return out


def expected(stream):
    """run_tile(stream), computed once per stream and shared (read-only)."""
    return _expected_cached(stream)


def canon(x):
    """f16 bits with every NaN made one NaN (0/0 is -NaN on x86 and +NaN on gfx950: DESIGN 5)."""
    x = np.array(x, np.uint16)
    x[(x & 0x7fff) > 0x7c00] = 0x7e00
    return x


# ---- battery ------------------------------------------------------------------------------------------------------------------
SOLID, BEGIN, END = ("solid",), ("begin",), ("END",)
DIAGONAL = ((0.5, 0.0, 13.25, 16.0, 1.0e9),)   # one segment across the tile: areas 0, 1 and every fraction in between
BACK = (0.15, 0.3, 0.2, 0.6)                   # translucent, premultiplied
SRC = (0.35, 0.1, 0.25, 0.5)
TRAIL = (0.05, 0.02, 0.1, 0.25)


def color(c):
    return ("color",) + tuple(c)


def fill(segments, backdrop=0, even_odd=False):
    return ("fill", tuple(tuple(s) for s in segments), backdrop, even_odd)


def end_clip(word, alpha=1.0):
    return ("end", word, alpha)


def one_pixel(px, py):
    """Two vertical segments on the pixel's edges: area exactly 1 in (px, py), exactly 0 everywhere else."""
    return ((px, py, px, py + 1, 1.0e9), (px + 1, py + 1, px + 1, py, 1.0e9))


def word_name(w):
    return "%04x" % w


def group_a():
    out = []
    words = [(m << 8) | c for m in range(16) for c in range(14)] + [0x8000, 0x8100]
    for w in words:
        for alpha in (1.0, 0.625):
            out.append(Stream("A_%s_a%g" % (word_name(w), alpha), "A",
                              [SOLID, color(BACK), BEGIN, SOLID, color(SRC), fill(DIAGONAL), end_clip(w, alpha), END]))
    return out


B_WORDS = [0x0000, 0x8000, 0x0100, 0x0600, 0x0900, 0x0c00, 0x0d00, 0x0e00, 0x0f00, 0x8100] + list(range(1, 14))
NAN, INF = U(0x7fc00000), U(0x7f800000)
SIXTEEN, SIXTEEN_UP = U(0x41800000), U(0x41800001)


def _backdrops():
    """(name, commands, finite).  "one": the odd value sits in pixel (9, 6) alone -- one lane has to turn the wave's ballot."""
    def whole(c):
        return [SOLID, color(c)]

    def one(c):  # the pixel first, over the transparent base (+0 * k + c = c); then BACK on every pixel but that one
        return [fill(one_pixel(9, 6)), color(c), fill(one_pixel(9, 6), backdrop=1), color(BACK)]
    def blown(last):
        """Finite words only: 3e38 in one pixel, times (1 - 3) = -inf there alone; then `last` over it."""
        return [fill(one_pixel(9, 6)), color((3.0e38, 0.5, 0.25, 1.0)), SOLID, color((0.0, 0.0, 0.0, 3.0))] + last
    grey = np.float32(0.35) * np.float32(0.5)
    back = [
        ("inrange", whole(BACK), True),
        ("sixteen_all", whole((SIXTEEN, 1.0, 0.5, 1.0)), True),
        ("sixteen_one", one((0.25, SIXTEEN, 0.5, 1.0)), True),
        ("sixteen_alpha_one", one((0.25, 0.5, 0.125, SIXTEEN)), True),
        ("sixteenup_all", whole((SIXTEEN_UP, 1.0, 0.5, 1.0)), True),
        ("sixteenup_one", one((0.25, 0.5, SIXTEEN_UP, 1.0)), True),
        ("far_all", whole((3.0e5, 1.0e5, 2.0e5, 0.0)), False),   # cb = 1e20: the mix modes overflow, cs' * 0 is NaN
        ("lum_one", one((1.0000002, 1.0000002, 1.0000002, 1.0)), False),  # lum(cb) just above 1: clip_color divides 0 by 0
        ("lum_grey_all", whole((0.5, 0.5, 0.5, 0.25)), False),
        ("grey_all", whole((grey, grey, grey, 0.5)), True),      # (luminosity over this grey: lum(c) - min(c) vanishes)
        ("alpha0_all", whole((0.015625, 0.0078125, 0.03125, 0.0)), True),   # (small: the store divides by 1e-6)
        ("negative_all", whole((-0.25, 0.5, 0.125, 0.75)), True),
        ("negative_one", one((0.25, -0.5, 0.125, 1.0)), True),
        ("negzero_all", whole((U(0x80000000), U(0x80000000), 0.5, 2.0)), True),
        ("nan_one", blown([SOLID, color((0.15, 0.3, 0.2, 1.0))]), False),      # -inf * (1 - 1) there alone
        ("nan_alpha_all", whole((0.5, 0.25, 0.125, NAN)), False),
        ("inf_all", whole((INF, 0.5, 0.25, 1.0)), False),
        ("inf_one", blown([fill(one_pixel(9, 6), backdrop=1), color(BACK)]), False),
    ]
    # (a backdrop with lum(cb) outside [0, 1] gives NaN under hue / saturation / color: clip_color divides 0 by 0; so does the one
    # grey under luminosity)
    lum_over = ("sixteen_all", "sixteen_one", "sixteenup_all", "sixteenup_one", "far_all", "lum_one", "lum_grey_all", "alpha0_all", "negative_one")
    return [(n, c, f, n not in lum_over) for n, c, f in back]


B_ALPHAS = [("0", 0.0, True), ("neg0", U(0x80000000), True), ("half", 0.5, True), ("1", 1.0, True), ("fltmax", U(0x7f7fffff), True),
            ("inf", INF, False), ("nan", NAN, False), ("pat3", U(3), True), ("pat10", U(10), True), ("pat11", U(11), True)]


def group_b():
    """<backdrop> BEGIN_CLIP (SOLID | FILL) END_CLIP(word, alpha), then -- behind a FILL -- one COLOR that shows what the area is
    afterwards.  Every word against every backdrop (alpha 1 behind SOLID, 0.5 behind FILL), every word against every alpha on the
    in-range backdrop, and the alphas against the backdrops that refuse the shortcut on three words."""
    out = []

    def add(bname, bcmds, bfin, lum_ok, w, aname, alpha, afin, inner):
        bfin = bfin and (lum_ok or not 0x0c <= (w >> 8) <= 0x0e) and not (bname == "grey_all" and (w >> 8) == 0x0f)
        body = [BEGIN, SOLID] if inner == "solid" else [BEGIN, fill(DIAGONAL)]
        tail = [] if inner == "solid" else [color(TRAIL)]
        out.append(Stream("B_%s_%s_%s_%s" % (bname, word_name(w), aname, inner), "B", bcmds + body + [end_clip(w, alpha)] + tail + [END],
                          finite=bfin and afin))
    backs = _backdrops()
    for bname, bcmds, bfin, lum_ok in backs:
        for w in B_WORDS:
            add(bname, bcmds, bfin, lum_ok, w, "1", 1.0, True, "solid")
            add(bname, bcmds, bfin, lum_ok, w, "half", 0.5, True, "fill")
    for w in B_WORDS:
        for aname, alpha, afin in B_ALPHAS:
            if aname != "1":
                add("inrange", backs[0][1], True, True, w, aname, alpha, afin, "solid")
            if aname != "half":
                add("inrange", backs[0][1], True, True, w, aname, alpha, afin, "fill")
    for bname, bcmds, bfin, lum_ok in backs:
        if bname in ("sixteenup_one", "negzero_all", "lum_one", "nan_one"):
            for w in (0x0000, 0x0100, 0x0c00):
                for aname, alpha, afin in B_ALPHAS:
                    if aname not in ("1", "half"):
                        add(bname, bcmds, bfin, lum_ok, w, aname, alpha, afin, "solid")
    return out


def _layer(word=0x0000, alpha=1.0):
    return [BEGIN, SOLID, end_clip(word, alpha)]


def _run(n, word=0x0000, alpha=1.0):
    return _layer(word, alpha) * n


C_TAIL = [fill(DIAGONAL), color(TRAIL), END]


def memo_prefix(w):
    low, lift = (0.125, 0.125, 0.125, 0.25), (0.875, 0.875, 0.875, 0.25)
    return [SOLID, color(low)] + _layer(w, 1.0) + [BEGIN, SOLID, color(lift), end_clip(0x000c, 1.0)] + _layer(w, 1.0)


def group_c():
    out = []
    head = [SOLID, color(BACK)]

    def add(name, cmds, finite=True):
        out.append(Stream("C_" + name, "C", cmds, finite))
    # every command boundary and every payload word at every phase of whatever window the kernel reads through: the run moves one
    # word at a time; words alternate between plain and a separable mode so that blend words of both kinds land everywhere
    mixed_run = (_layer(0x0000, 1.0) + _layer(0x0200, 0.5) + _layer(0x8000, 0.75)) * 10
    for k in range(67):
        add("phase_%02d" % k, head + [SOLID] * k + mixed_run + C_TAIL)
    for n in (1, 2, 21, 22, 64, 213):
        add("run_%d" % n, head + _run(n) + C_TAIL)
        add("run_hue_%d" % n, head + _run(n, 0x0c00, 0.5) + C_TAIL)
    for n in (4, 5):
        add("begin_x%d_empty" % n, head + [BEGIN] * n + [SOLID] + [end_clip(0x0000, 1.0)] * n + C_TAIL)
        add("begin_x%d_drawn" % n, head + [BEGIN] * n + [SOLID, color(SRC)] + [end_clip(w, 0.75) for w in (0x0300, 0x0904, 0x0b00, 0x0509, 0x020c)[:n]] + C_TAIL)
    add("open_at_end_empty", head + _run(3) + [BEGIN, BEGIN, SOLID, END])
    add("open_at_end_drawn", head + _run(3) + [BEGIN, SOLID, color(SRC), BEGIN, fill(DIAGONAL), color(TRAIL), END])
    add("open_at_end_after_run", head + [BEGIN, SOLID, color(SRC)] + _run(30) + [END])
    interrupts = [
        ("plus", lambda: _layer(0x000c, 1.0), True),
        ("destout", lambda: _layer(0x0008, 0.5), True),
        ("xor_multiply", lambda: _layer(0x010b, 1.0), True),
        ("multiply", lambda: _layer(0x0100, 1.0), True),           # after plain layers only: needs the range, not yet in the memo
        ("luminosity", lambda: _layer(0x0f00, 1.0), True),
        ("clip_mix", lambda: _layer(0x8100, 1.0), True),
        ("pat3", lambda: _layer(0x0000, U(3)), True),
        ("pat10", lambda: _layer(0x0000, U(10)), True),
        ("pat11", lambda: _layer(0x0000, U(11)), True),
        ("neg0", lambda: _layer(0x0000, U(0x80000000)), True),
        ("inf", lambda: _layer(0x0000, INF), False),
        ("jump", lambda: [("jump",)], True),
        ("materialised", lambda: [BEGIN, color(SRC), BEGIN, SOLID, end_clip(0x0000, 1.0), end_clip(0x0400, 0.5)], True),
        ("fill_layer", lambda: [BEGIN, fill(DIAGONAL), end_clip(0x0000, 1.0), SOLID], True),
    ]
    for iname, make, fin in interrupts:
        for at in (0, 1, 15, 29):
            add("cut_%s_at%02d" % (iname, at), head + _run(at) + make() + _run(30 - at) + C_TAIL, fin)
    # hue needs more than multiply established: a run of multiply layers, one hue layer at the position, multiply again
    for at in (0, 1, 15, 29):
        add("cut_hue_in_multiply_at%02d" % at, head + _run(at, 0x0100) + _layer(0x0c00, 1.0) + _run(30 - at, 0x0100) + C_TAIL)
        add("cut_jump_in_hue_at%02d" % at, head + _run(at, 0x0e00, 0.5) + [("jump",)] + _run(30 - at, 0x0d00, 0.5) + C_TAIL)
    # the memo must not survive a layer that changes the backdrop: colour 0.125 / alpha 0.25 (cb = 0.5), a Plus layer lifts it to
    # 1.0 / 0.5 (cb = 2: lum > 1), and the hue layer behind it must not be closed on what the first one established
    for w in (0x0c00, 0x0d00, 0x0e00):
        add("memo_plus_%s" % word_name(w), memo_prefix(w) + _run(3, w) + C_TAIL, finite=False)
    # ... nor a backdrop that leaves the range between two separable layers (DestOver is no SrcOver: the run stops there anyway;
    # Plus again, from 12 to 24)
    add("memo_plus_range", [SOLID, color((12.0, 0.5, 0.25, 1.0))] + _layer(0x0100, 1.0)
        + [BEGIN, SOLID, color((12.0, 0.0, 0.0, 0.0)), end_clip(0x000c, 1.0)] + _layer(0x0100, 1.0) + _run(3, 0x0900) + C_TAIL)
    return out


D_WORDS = [0x0100, 0x0904, 0x0c00, 0x0209, 0x0f00, 0x050c, 0x0a0b]   # per level: mix and operator both varied
D_ALPHAS = [1.0, 0.75, 0.5, 0.875, 0.625, 0.9375, 0.8125]
D_COLORS = [(0.3, 0.1, 0.2, 0.5), (0.1, 0.35, 0.15, 0.45), (0.2, 0.2, 0.05, 0.4), (0.05, 0.15, 0.3, 0.55), (0.25, 0.05, 0.1, 0.35),
            (0.1, 0.3, 0.3, 0.6), (0.15, 0.1, 0.05, 0.3)]


def _level_fill(i):
    """Per-pixel-varying content of level i: a diagonal of its own."""
    return fill(((0.25 + 1.5 * i, 0.0, 15.5 - 1.25 * i, 16.0, 1.0e9),), 0, i % 2 == 1)


def group_d():
    out = []
    head = [SOLID, color(BACK)]
    for depth in range(1, 8):
        every = list(head)
        for i in range(depth):
            every += [BEGIN, _level_fill(i), color(D_COLORS[i])]
        for i in reversed(range(depth)):
            every += [_level_fill(i + 1), end_clip(D_WORDS[i], D_ALPHAS[i])]
        out.append(Stream("D_every_level_%d" % depth, "D", every + C_TAIL))
        inner = list(head) + [BEGIN] * depth + [_level_fill(depth), color(D_COLORS[depth - 1])]
        for i in reversed(range(depth)):
            inner += [_level_fill(i), end_clip(D_WORDS[i], D_ALPHAS[i])]
        out.append(Stream("D_innermost_only_%d" % depth, "D", inner + C_TAIL))
    # depth 7, the second-innermost layer (level 5) closed empty: its only content is the innermost layer, which is empty too
    cmds = list(head)
    for i in range(5):
        cmds += [BEGIN, _level_fill(i), color(D_COLORS[i])]
    cmds += [BEGIN, BEGIN, SOLID, end_clip(0x0000, 1.0), end_clip(0x0100, 0.5)]
    for i in reversed(range(5)):
        cmds += [_level_fill(i + 1), end_clip(D_WORDS[i], D_ALPHAS[i])]
    out.append(Stream("D_depth7_level5_empty", "D", cmds + C_TAIL))
    cmds = list(head)
    for i in range(5):
        cmds += [BEGIN, _level_fill(i), color(D_COLORS[i])]
    cmds += [BEGIN, BEGIN, _level_fill(6), color(D_COLORS[6]), _level_fill(2), end_clip(D_WORDS[6], D_ALPHAS[6]), SOLID, end_clip(0x0c00, 0.5)]
    for i in reversed(range(5)):
        cmds += [_level_fill(i + 1), end_clip(D_WORDS[i], D_ALPHAS[i])]
    out.append(Stream("D_depth7_level5_only_inner", "D", cmds + C_TAIL))
    return out


@functools.lru_cache(maxsize=None)
def battery():
    """{"A": [...], "B": [...], "C": [...], "D": [...]}: every stream is one tile."""
    groups = {"A": group_a(), "B": group_b(), "C": group_c(), "D": group_d()}
    names = [s.name for g in groups.values() for s in g]
    assert len(names) == len(set(names))
    return groups


def frames(group):
    """The group's streams, 64 per frame."""
    ss = battery()[group]
    return [Frame(ss[i:i + TILES]) for i in range(0, len(ss), TILES)]


MAX_DEPTH = 7


# ---- running a frame through fine alone -------------------------------------------------------------------------------------
FINE_STAGE = {0: "fine_area", 1: "fine_msaa8", 2: "fine_msaa16"}
BUFFERS = ("ptclBuf", "segmentsBuf", "blend_spill")


def carrier(aa, ramp=False):
    """(scene, params): 128 x 128 with a clip nest MAX_DEPTH deep -- n_clip != 0 selects the instantiations with the layer
    machinery and the engine's clip-depth hint covers the deepest stream -- and, with `ramp`, a gradient, which binds a ramp image
    and so selects the instantiation with the paint code.  The bump sizes hold the largest frame of the battery."""
    import jello_amd
    from jello_amd import Brush, ColorStop, Compose, Fill, Mix, Path, RenderParams, Scene
    size = 16 * TILES_X
    s = Scene()
    for k in range(MAX_DEPTH):
        s.push_layer(Mix.Clip if k % 2 else Mix.Normal, Compose.SrcOver, 1.0, None, Path.rect(4 + 2 * k, 4 + 2 * k, size - 4 - 2 * k, size - 4 - 2 * k))
    s.fill(Fill.NonZero, None, Brush.solid((0.2, 0.4, 0.6, 0.8)), None, Path.circle(size / 2, size / 2, size / 3))
    for _ in range(MAX_DEPTH):
        s.pop_layer()
    if ramp:
        stops = [ColorStop(0.0, (1.0, 0.0, 0.0, 1.0)), ColorStop(1.0, (0.0, 0.0, 1.0, 0.5))]
        s.fill(Fill.NonZero, None, Brush.linear((0.0, 0.0), (float(size), 0.0), stops), None, Path.rect(0, 0, size, 8))
    p = RenderParams(size, size, aa=jello_amd.Aa(aa))
    p.bump = s.bump_sizes(size, size)
    all_frames = [f for g in "ABCD" for f in frames(g)]
    p.bump.ptcl = max(p.bump.ptcl, max(len(f.ptcl) for f in all_frames))
    p.bump.segments = max(p.bump.segments, max(f.segments.shape[0] for f in all_frames))
    p.bump.blend_spill = max(p.bump.blend_spill, max(f.spill_entries for f in all_frames))
    return s, p


def images(frame, rec):
    """{buffer id: uint8 array of exactly the buffer's size}: the frame's PTCL (behind it END words), its segments (zeros) and a
    blend_spill of 0xCD bytes.  Validates the frame against the real sizes first."""
    sizes = {n: rec.buffer(n) for n in BUFFERS}
    validate(frame, ptcl_words=sizes["ptclBuf"][1] // 4, spill_capacity=sizes["blend_spill"][1] // 16, segment_capacity=sizes["segmentsBuf"][1] // 24)
    out = {}
    for name, src, pad in (("ptclBuf", frame.ptcl, 0), ("segmentsBuf", frame.segments, 0), ("blend_spill", np.zeros(0, np.uint8), 0xCD)):
        bid, size = sizes[name]
        raw = np.full(size, pad, np.uint8)
        b = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        raw[:b.size] = b
        out[bid] = raw
    return out


def tiles_of(image):
    """(128, 128, 4) -> [64] x (16, 16, 4), tile_ix = ty * 8 + tx."""
    return [image[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] for ty in range(TILES_Y) for tx in range(TILES_X)]


class OracleFine:
    """The carrier through the whole oracle pipeline once; then frames through its fine stage alone."""

    def __init__(self, aa=0, ramp=False):
        import jello_amd
        from oracle.oracle_engine import OracleEngine
        self.aa = int(aa)
        s, p = carrier(aa, ramp)
        self.rec = jello_amd.Host().record(s, p)
        self.o = OracleEngine()
        self.o.run(self.rec)

    def run(self, frame):
        for bid, raw in images(frame, self.rec).items():
            self.o.bufs[bid] = raw
        self.o.run(self.rec, only=FINE_STAGE[self.aa])
        return tiles_of(self.o.target(self.rec).copy())


def mismatch(stream, got, want, got_name, want_name, third=None, third_name=None):
    """None, or the message for the first pixel of the tile whose f16 bits differ (NaNs made one)."""
    bad = np.argwhere((canon(got) != canon(want)).any(axis=2))
    if bad.shape[0] == 0:
        return None
    y, x = (int(v) for v in bad[0])
    text = "%s: %d pixels differ, first at (x, y) = (%d, %d): %s %s %s %s" % (
        stream.name, bad.shape[0], x, y, got_name, ["0x%04x" % v for v in got[y, x]], want_name, ["0x%04x" % v for v in want[y, x]])
    if third is not None:
        text += " %s %s" % (third_name, ["0x%04x" % v for v in third[y, x]])
    return text


# ---- one scene through the whole pipeline: every (mix, operator) pair as a 16 x 16 cell ---------------------------------------
def blend_grid(aa=0):
    """(scene, params, cells): cells = [(mix, compose, backdrop, source, layer_alpha, (cx, cy))] with the cell's centre pixel."""
    import jello_amd
    from jello_amd import Brush, Compose, Fill, Mix, Path, RenderParams, Scene
    from test_blend_spec import PAIRS
    backdrop, source = PAIRS[1]
    mixes = [m for m in Mix if m != Mix.Clip]
    operators = [c for c in Compose if c != Compose.PlusLighter]
    s = Scene()
    cells = []
    for row, op in enumerate(operators):
        for col, mix in enumerate(mixes):
            x0, y0 = 16 * col, 16 * row
            cell = Path.rect(x0, y0, x0 + 16, y0 + 16)
            s.fill(Fill.NonZero, None, Brush.solid(backdrop), None, cell)
            s.push_layer(mix, op, 0.8, None, cell)
            s.fill(Fill.NonZero, None, Brush.solid(source), None, cell)
            s.pop_layer()
            cells.append((mix, op, backdrop, source, 0.8, (x0 + 8, y0 + 8)))
    return s, RenderParams(16 * len(mixes), 16 * len(operators), aa=jello_amd.Aa(aa)), cells


def check_grid(image_bits, cells):
    """Every cell's centre pixel against test_blend_spec.expected at its tolerance (the RGBA16F store's 2.5e-3); alpha alone where
    the result is transparent.  Returns the list of failures."""
    from test_blend_spec import expected as w3c
    px = np.ascontiguousarray(image_bits).view(np.float16).astype(np.float64)
    bad = []
    for mix, op, backdrop, source, alpha, (cx, cy) in cells:
        got, want = px[cy, cx], w3c(mix, op, backdrop, source, alpha)
        ok = abs(got[3]) < 1e-3 if want[3] < 1e-3 else np.allclose(got, want, atol=2.5e-3)
        if not ok:
            bad.append((mix.name, op.name, [float(v) for v in got], [float(v) for v in want]))
    return bad
