"""The battery jh_composite is held to (tests/test_gpu_composite.py) and the reference's consequences and sensitivity are checked on
(tests/test_composite_spec.py).  A case: name, the source image (size and content), the destination (size; its content is POISON
outside the placed rectangle and real texels inside it), src_rect, offset, mix, compose, opacity, tint.

Geometry (GEOMETRY): Normal + SrcOver and Multiply over dst widths 1, 2, 3, 511, 512, 513, 1025 x heights 1 and 3 -- one on each side
of the kernel's seams (jello_amd/csrc/kernels_composite.hip): a work item is a row segment of 512 texels on the 16-byte grid of the
dst row, so 511 / 512 / 513 are one item, one item and one-or-two items depending on the row's phase, 1025 three; an odd dst width
puts every other row on the other phase -- with placements that make dx and sx - dx even and odd, the source width odd, dx and dy
negative and past each of the four edges, the placement fully outside, a sub-rectangle of a larger source, a source larger than dst.
Values (VALUES): a 64 x 9 image pair under all 224 modes; TINTED: opacity and tint on the same pair; RANDOM: a 257 x 33 layer of
random texels on a 300 x 40 destination with opacity 0.3, where a reordered or contracted binary32 operation reaches the f16 result."""
import functools

import numpy as np

import composite_ref

POISON = 0x5A5A  # what dst holds outside the placed rectangle (a finite f16)


def _h(v):
    return int(np.array(v, np.float16).view(np.uint16))


SUB = 0x0001  # the smallest f16 subnormal
COLOURS = [0x0000, 0x8000, SUB, 0x0400, _h(0.25), _h(0.5), _h(1.0), _h(1.5), 0x7BFF, _h(-0.5), 0x7C00, 0x7E00]  # .. 65504, -0.5, Inf, NaN
ALPHAS = [0x0000, 0x8000, SUB, 0x0400, _h(0.25), _h(0.5), _h(1.0), _h(1.5), 0x7E00]
# (source rgb, source a, backdrop rgb, backdrop a): +-0 ties between the two colours and inside one, and equal channels (the
# orderings set_sat and the min / max of sat and clip_color have to break)
Z, N, Q, H_, O = 0x0000, 0x8000, _h(0.25), _h(0.5), _h(1.0)
TIES = [((Z, N, H_), O, (N, Z, H_), O), ((N, N, N), O, (Z, Z, Z), O), ((Z, Z, Z), H_, (N, N, N), H_),
        ((H_, H_, H_), O, (Q, Q, Q), O), ((Q, Q, O), H_, (O, Q, Q), O), ((Q, O, Q), O, (H_, H_, Q), H_),
        ((O, Q, Q), O, (Q, H_, H_), O), ((N, Z, O), H_, (Z, N, O), H_), ((H_, Q, H_), O, (Q, Q, H_), H_)]
VW, VH = 64, 9


def value_pair():
    """(src, dst) of the value battery, (9, 64, 4) uint16 each: texel t = y * 64 + x takes the alpha pair t % 81 of ALPHAS x ALPHAS
    (every pair seven times) with colours that walk COLOURS at different strides per image and channel; the last nine texels are TIES."""
    src = np.zeros((VH, VW, 4), np.uint16)
    dst = np.zeros((VH, VW, 4), np.uint16)
    n = len(COLOURS)
    for t in range(VW * VH):
        y, x = divmod(t, VW)
        p, rep = t % 81, t // 81
        for ch in range(3):
            src[y, x, ch] = COLOURS[(p + 5 * rep + 3 * ch) % n]
            dst[y, x, ch] = COLOURS[(7 * p + rep + 4 * ch + 1) % n]
        src[y, x, 3] = ALPHAS[p // 9]
        dst[y, x, 3] = ALPHAS[p % 9]
    for i, (sc, sa, dc, da) in enumerate(TIES):
        y, x = divmod(VW * VH - len(TIES) + i, VW)
        src[y, x] = list(sc) + [sa]
        dst[y, x] = list(dc) + [da]
    return src, dst


def unit(w, h, seed):
    """(h, w, 4) uint16: colours in [-0.25, 1.25) and alphas in [0, 1], a tenth of the alphas exactly 0 and a tenth exactly 1."""
    rng = np.random.default_rng(seed)
    f = rng.random((h, w, 4), dtype=np.float32)
    f[..., :3] = f[..., :3] * 1.5 - 0.25
    pick = rng.random((h, w))
    f[..., 3][pick < 0.1] = 0.0
    f[..., 3][pick > 0.9] = 1.0
    return f.astype(np.float16).view(np.uint16)


def _case(name, src_size, dst_size, src_rect=None, offset=(0, 0), mix=0, compose=0, opacity=1.0, tint=None, content="unit"):
    return {"name": name, "src_size": src_size, "dst_size": dst_size, "src_rect": src_rect, "offset": offset, "mix": mix, "compose": compose,
            "opacity": opacity, "tint": tint, "content": content}


def _geometry():
    out = []
    for mix in (0, 1):
        m = composite_ref.MIX_NAMES[mix]
        for W in (1, 2, 3, 511, 512, 513, 1025):
            for H in (1, 3):
                down = 1 if H > 1 else 0
                tag = "%s_%dx%d_" % (m, W, H)
                out.append(_case(tag + "whole", (W, H), (W, H), mix=mix))
                # sx - dx odd, and a source width of the other parity: the source pair of a row is aligned where dst's is not
                out.append(_case(tag + "sx1", (W + 1, H), (W, H), (1, 0, W, H), (0, 0), mix=mix))
                out.append(_case(tag + "up_left", (W, H), (W, H), None, (-1, -down), mix=mix))      # over the left and top edges
                out.append(_case(tag + "down_right", (W, H), (W, H), None, (1, down), mix=mix))     # odd dx; over the right and bottom edges
                out.append(_case(tag + "larger_source", (W + 5, H + 4), (W, H), None, (-2, -1), mix=mix))
                if W >= 3:
                    out.append(_case(tag + "inner", (W - 2, H), (W, H), None, (1, 0), mix=mix))     # odd dx, dst's edges untouched
                    out.append(_case(tag + "inner_even", (W - 2, H), (W, H), None, (2, 0), mix=mix) if W > 3 else
                               _case(tag + "inner_even", (1, H), (W, H), None, (2, 0), mix=mix))
        # a 23 x 7 source (odd width) on a 37 x 5 destination (odd width): offsets on both sides of every edge, fully outside included
        for dx in (-23, -22, -3, -2, 0, 1, 2, 3, 30, 36, 37, 40):
            for dy in ((-7, 0, 4) if dx % 2 else (-6, -2, 1, 5)):
                out.append(_case("%s_37x5_at_%d_%d" % (m, dx, dy), (23, 7), (37, 5), None, (dx, dy), mix=mix))
        # sub-rectangles of a larger source, sx - dx even and odd, even and odd dx
        for rect in ((1, 2, 20, 3), (2, 1, 21, 5), (22, 6, 1, 1), (3, 0, 19, 7)):
            for dx in (0, 1, 4, 17, 30):
                out.append(_case("%s_37x5_rect_%d_%d_%d_%d_at_%d" % ((m,) + rect + (dx,)), (23, 7), (37, 5), rect, (dx, 1), mix=mix))
    return out


GEOMETRY = _geometry()
VALUES = [_case("values_%s_%s" % (composite_ref.MIX_NAMES[mix], composite_ref.COMPOSE_NAMES[compose]), (VW, VH), (VW, VH), mix=mix, compose=compose,
                content="values") for mix in range(composite_ref.N_MIX) for compose in range(composite_ref.N_COMPOSE)]
TINTS = {"plain": None, "tint": (0.125, 0.3, 0.7, 0.5), "tint_above_1": (1.5, 0.2, 2.25, 1.0)}
TINTED = [_case("tinted_%s_%s_op%g_%s" % (composite_ref.MIX_NAMES[mix], composite_ref.COMPOSE_NAMES[compose], opacity, tname), (VW, VH), (VW, VH),
                mix=mix, compose=compose, opacity=opacity, tint=tint, content="values")
          for (mix, compose) in ((0, 0), (1, 0), (0, 5), (12, 11)) for opacity in (0.0, 0.5, 1.0) for tname, tint in TINTS.items()]
# random content, an opacity that is no power of two: where the order and the fusing of the binary32 operations show in the f16 result
RANDOM = [_case("random_%s_op%g_%s" % (composite_ref.MIX_NAMES[mix], opacity, tname), (257, 33), (300, 40), None, (21, 3), mix=mix, opacity=opacity, tint=tint)
          for mix in (0, 1) for opacity in (0.3, 1.0) for tname, tint in TINTS.items() if tname != "tint_above_1"]
CASES = GEOMETRY + VALUES + TINTED + RANDOM
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _seed(case):
    (sw, sh), (dw, dh) = case["src_size"], case["dst_size"]
    return sw * 100003 + sh * 9176 + dw * 131 + dh * 17 + (case["offset"][0] & 0xFF) * 7 + case["mix"]


@functools.lru_cache(maxsize=None)
def _images(name):
    c = BY_NAME[name]
    if c["content"] == "values":
        src, content = value_pair()
    else:
        src = unit(c["src_size"][0], c["src_size"][1], _seed(c))
        content = unit(c["dst_size"][0], c["dst_size"][1], _seed(c) + 1)
    dst = np.full_like(content, POISON)
    _, _, dx, dy, w, h = composite_ref.clip(c["src_size"], c["dst_size"], c["src_rect"], c["offset"])
    dst[dy:dy + h, dx:dx + w] = content[dy:dy + h, dx:dx + w]
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


def source(case):
    """(h, w, 4) uint16, read-only."""
    return _images(case["name"])[0]


def destination(case):
    """What dst holds before the call: (H, W, 4) uint16, read-only -- POISON outside the placed rectangle."""
    return _images(case["name"])[1]


@functools.lru_cache(maxsize=None)
def expected(name, **variant):
    """What dst holds after the case's call, by tests/composite_ref.py (computed once per case and variant; do not modify the result)."""
    c = BY_NAME[name]
    out = composite_ref.composite(source(c), destination(c), c["mix"], c["compose"], c["opacity"], c["tint"], c["src_rect"], c["offset"], **variant)
    out.setflags(write=False)
    return out
