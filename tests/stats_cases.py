"""The battery jh_stats is held to (tests/test_gpu_stats.py) and the reference's sensitivity is measured on
(tests/test_stats_spec.py).  A case: name, w, h, content (kind and its argument), what, channel, threshold, population, transfer, rect
(or None) and `inst`, the instantiation of k_stats it runs (jello_amd/csrc/kernels_stats.hip: <BOX, HIST, SRGB>; BOX: bounds or
extremes are asked for).  The expected value of a case is the whole record, byte for byte.

Sizes: 1x1, 1x5, 5x1, 2x2, 3x3, and one on each side of every boundary of the kernel:
  an item of 2 x 256 texels          widths 511, 512, 513, 514 with heights 1, 2, 3 (511: one item with the phase's spare pair, 512: a
                                     second item for the last texel of an odd-phase row, 513 and 514: two)
  the 16-byte grid                   odd image widths (511, 513, 37, 67) alternate the phase by row; rectangles at odd x
  the grid cap, 4 workgroups x CUs   1 x 1024: exactly 1024 items on 256 CUs; 1 x 1030 and 3 x 1100: more, the grid stride
  the finish's 16 groups             1 .. 1024 partials: 1x1 (one), 1x5 (five), 3x3, 1x1030 (all)"""
import functools
import itertools

import numpy as np

import stats_ref
from stats_ref import ALL, BOUNDS, CONTENT, EVERYTHING, EXTREMES, HISTOGRAM, LINEAR, SRGB, SUBNORMAL

ONE, ZERO, NEG0, HALF, INF, NINF, NAN, NNAN, SUB, NSUB, TWO, QUARTER = 0x3C00, 0x0000, 0x8000, 0x3800, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x0001, 0x8001, 0x4000, 0x3400
# 0x3BFF .. 0x3C01 straddle 1; 0x1C04 is f16(1 / 255) (code 1), 0x1804 half of it (255 q just below 0.5: code 0); 0x37FF .. 0x3801 straddle the one tie, 127.5
VALUES = [ZERO, NEG0, SUB, NSUB, HALF, ONE, TWO, INF, NINF, NAN, NNAN, QUARTER, 0x3BFF, 0x3C01, 0x1C04, 0x1804, 0x37FF, 0x3801, 0xBC00, 0x2E66, 0x7BFF, 0xFBFF]
ABOVE_FINITE = 7.0e4  # a finite binary32 above every finite f16: only +Inf is content
COMBOS = [(what, pop, transfer) for what in range(1, 8) for pop in (ALL, CONTENT) for transfer in (LINEAR, SRGB)]
INSTANTIATIONS = ["k_stats<true, false, false>", "k_stats<false, true, false>", "k_stats<false, true, true>", "k_stats<true, true, false>",
                  "k_stats<true, true, true>"]


def inst(what, transfer):
    box, hist = bool(what & (BOUNDS | EXTREMES)), bool(what & HISTOGRAM)
    return "k_stats<%s, %s, %s>" % tuple("true" if f else "false" for f in (box or not hist, hist, hist and transfer == SRGB))


def blob(w, h):
    """A glyph-like shape: a ring with a bar through it."""
    Y, X = np.mgrid[0:h, 0:w]
    cx, cy, r = (w - 1) / 2.0, (h - 1) / 2.0, max(1.0, min(w, h) / 2.0 - 1.5)
    d = np.hypot(X - cx, Y - cy)
    return ((d <= r) & (d >= r * 0.55)) | ((np.abs(Y - cy) <= max(1, h // 8)) & (np.abs(X - cx) <= r))


def all_patterns():
    """256 x 256: every f16 bit pattern once per channel, each channel in another order (odd multipliers permute 2^16)."""
    i = np.arange(65536, dtype=np.uint32)
    return np.stack([((i * m + a) & 0xFFFF).astype(np.uint16) for m, a in ((1, 0), (40503, 7), (3, 0x8000), (25173, 13849))], axis=-1).reshape(256, 256, 4)


def content(kind, arg, w, h, channel, rect, seed):
    """(h, w, 4) uint16.  'values': every channel drawn from VALUES; 'unit': random values in [0, 1]; 'patterns': all_patterns;
    'constant': the texel `arg` everywhere; 'alternate': the texels arg[0], arg[1] in a chessboard; 'set': every channel drawn from
    the patterns `arg`; 'nan_channel': unit, channel 1 all NaN; 'mask': unit colour, and in `channel` 1 at the positions `arg` -- (x, y)
    relative to the rectangle, which may lie just outside it -- and 0 elsewhere; 'blob'; 'diagonal'; 'never': zeros (the source is
    only created).  'mask', 'blob' and 'diagonal' with a rectangle: the image around the rectangle holds NaN colour and content."""
    rng = np.random.default_rng(seed)
    if kind == "never":
        return np.zeros((h, w, 4), np.uint16)
    if kind == "patterns":
        return all_patterns()
    if kind == "values":
        return rng.choice(np.array(VALUES, np.uint16), (h, w, 4))
    if kind == "set":
        return rng.choice(np.array(arg, np.uint16), (h, w, 4))
    if kind == "constant":
        return np.broadcast_to(np.array(arg, np.uint16), (h, w, 4)).copy()
    if kind == "alternate":
        Y, X = np.mgrid[0:h, 0:w]
        return np.where(((X + Y) & 1)[..., None] == 0, np.array(arg[0], np.uint16), np.array(arg[1], np.uint16)).astype(np.uint16)
    bits = rng.random((h, w, 4)).astype(np.float16).view(np.uint16)
    if kind == "unit":
        return bits
    if kind == "nan_channel":
        bits[..., 1] = np.where(rng.random((h, w)) < 0.5, NAN, NNAN)
        return bits
    x0, y0, rw, rh = rect or (0, 0, w, h)
    m = np.zeros((h, w), bool)
    if kind == "mask":
        for (px, py) in arg:
            m[y0 + py, x0 + px] = True
    elif kind == "blob":
        m[y0:y0 + rh, x0:x0 + rw] = blob(rw, rh)
    elif kind == "diagonal":
        for i in range(min(rw, rh)):
            m[y0 + i, x0 + i] = True
    else:
        raise ValueError(kind)
    bits[..., channel] = np.where(m, ONE, ZERO)
    if rect is not None and arg != "plain":
        outside = np.ones((h, w), bool)
        outside[y0:y0 + rh, x0:x0 + rw] = False
        keep = m & outside  # (a mask position just outside the rectangle stays what it is: content)
        fill = np.array([NAN, INF, NNAN, ONE], np.uint16)
        fill[channel] = ONE  # content everywhere around the rectangle, NaN and Inf colour
        bits[outside & ~keep] = fill
    return bits


CASES = []


def _case(w, h, kind, arg=None, what=EVERYTHING, channel=3, threshold=SUBNORMAL, population=ALL, transfer=LINEAR, rect=None, tag=""):
    name = "%dx%d_%s%s_w%d_%s_%s_ch%d" % (w, h, kind, tag, what, "content" if population == CONTENT else "all", "srgb" if transfer == SRGB else "linear", channel)
    if rect:
        name += "_r%d_%d_%d_%d" % rect
    assert not any(c["name"] == name for c in CASES), name
    CASES.append(dict(name=name, w=w, h=h, kind=kind, arg=arg, what=what, channel=channel, threshold=threshold, population=population, transfer=transfer,
                      rect=rect, inst=inst(what, transfer), seed=len(CASES) + 1))


_combo = itertools.cycle(COMBOS)
_channel = itertools.cycle((3, 0, 1, 2))
# sizes on both sides of every boundary, each under the next combination of (what, population, transfer) and the next content channel
for (_w, _h) in [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3)] + [(w, h) for w in (511, 512, 513, 514) for h in (1, 2, 3)] + \
        [(1, 1024), (1, 1030), (3, 1100), (37, 21), (1023, 2), (1025, 3), (67, 41)]:
    for _ in range(2 if _w * _h < 2000 else 1):
        _what, _pop, _tr = next(_combo)
        _case(_w, _h, "values", what=_what, population=_pop, transfer=_tr, channel=next(_channel), threshold=0.5)
# every instantiation on the small and the boundary sizes
for _what, _tr in ((BOUNDS | EXTREMES, LINEAR), (HISTOGRAM, LINEAR), (HISTOGRAM, SRGB), (EVERYTHING, LINEAR), (EVERYTHING, SRGB)):
    for (_w, _h) in ((1, 1), (2, 2), (3, 3), (513, 3), (1, 1030)):
        _case(_w, _h, "values", what=_what, transfer=_tr, population=CONTENT, threshold=0.0, tag="_inst")
# every f16 pattern once per channel: both transfers, both populations, every subset of what
for _what, _pop, _tr in COMBOS:
    _case(256, 256, "patterns", what=_what, population=_pop, transfer=_tr, threshold=0.5, channel=_what % 4)
# rectangles at odd offsets inside NaN and content
for _rect in ((11, 7, 45, 27), (1, 1, 65, 39), (33, 17, 1, 1), (0, 0, 67, 41), (66, 40, 1, 1), (3, 5, 2, 30)):
    _what, _pop, _tr = next(_combo)
    _case(67, 41, "blob", rect=_rect, what=EVERYTHING, population=_pop, transfer=_tr, threshold=0.5)
    _case(67, 41, "diagonal", rect=_rect, what=_what, population=CONTENT, transfer=_tr, threshold=0.5, channel=1)
_R = (11, 7, 45, 27)
for _tag, _at in (("_none", ()), ("_tl", ((0, 0),)), ("_tr", ((44, 0),)), ("_bl", ((0, 26),)), ("_br", ((44, 26),)),
                  ("_corners", ((0, 0), (44, 0), (0, 26), (44, 26))), ("_left_of", ((-1, 13),)), ("_right_of", ((45, 13),)), ("_above", ((20, -1),)),
                  ("_below", ((20, 27),)), ("_one", ((20, 13),))):
    _case(67, 41, "mask", _at, rect=_R, what=EVERYTHING, population=CONTENT, threshold=0.5, tag=_tag)
    _case(67, 41, "mask", _at, rect=_R, what=BOUNDS, threshold=0.5, channel=2, tag=_tag)
_case(67, 41, "mask", tuple((x, y) for x in range(45) for y in range(27)), rect=_R, what=EVERYTHING, population=CONTENT, threshold=0.5, tag="_every")
# values: constants (every lane of every wave on one bin), two alternating values, the special sets
for _tag, _texel in (("_transparent", (ZERO, ZERO, ZERO, ZERO)), ("_colour", (0x3666, HALF, 0x2E66, ONE)), ("_nan", (NAN, NAN, NAN, NAN))):
    for _what, _tr in ((BOUNDS | EXTREMES, LINEAR), (HISTOGRAM, LINEAR), (HISTOGRAM, SRGB), (EVERYTHING, LINEAR), (EVERYTHING, SRGB)):
        _case(515, 5, "constant", _texel, what=_what, transfer=_tr, tag=_tag)
    _case(515, 5, "constant", _texel, population=CONTENT, transfer=SRGB, tag=_tag)
_case(515, 5, "alternate", ((0x3666, HALF, 0x2E66, ONE), (ONE, QUARTER, ZERO, HALF)), transfer=SRGB)
_case(515, 5, "alternate", ((ZERO, ZERO, ZERO, ZERO), (ONE, ONE, ONE, ONE)), population=CONTENT)
for _tag, _set in (("_zeros", (ZERO, NEG0)), ("_infs", (INF, NINF)), ("_subnormals", (SUB, NSUB, 0x03FF, 0x83FF, ZERO)), ("_neg0", (NEG0,)), ("_pos0", (ZERO,))):
    _case(37, 21, "set", _set, threshold=0.0, transfer=SRGB, tag=_tag)
    _case(37, 21, "set", _set, threshold=-0.0, population=CONTENT, tag=_tag + "_t-0")
_case(37, 21, "nan_channel", threshold=0.5, transfer=SRGB)
_case(37, 21, "nan_channel", threshold=0.5, population=CONTENT, channel=1)  # (no content: a NaN is none)
for _t, _tag in ((0.0, "_t0"), (-0.0, "_t-0"), (0.5, "_thalf"), (SUBNORMAL, "_tsub"), (ABOVE_FINITE, "_tabove")):
    for _ch in range(4):
        _case(37, 21, "values", threshold=_t, channel=_ch, population=CONTENT, transfer=SRGB if _ch & 1 else LINEAR, tag=_tag)
# a never-written source
_case(33, 21, "never", threshold=0.5)
_case(33, 21, "never", threshold=0.0, population=CONTENT, transfer=SRGB, rect=(3, 5, 20, 9))

BY_NAME = {c["name"]: c for c in CASES}


def source(c):
    return content(c["kind"], c["arg"], c["w"], c["h"], c["channel"], c["rect"], c["seed"])


def keywords(c):
    return dict(what=c["what"], channel=c["channel"], threshold=c["threshold"], population=c["population"], transfer=c["transfer"], rect=c["rect"])


@functools.lru_cache(maxsize=None)
def _expected(name, variant):
    c = BY_NAME[name]
    return stats_ref.record_bytes(source(c), **keywords(c), **dict(variant))


def expected(name, **variant):
    """The record's bytes of a case (computed once and shared), or of a near miss of the rule."""
    return _expected(name, tuple(sorted(variant.items())))
