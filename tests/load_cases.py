"""The batteries of jh_load_yuv and jh_load_surface: every case names the kernel instantiation it runs, and
tests/test_gpu_load.py runs one GPU test per instantiation.  A case is a dict of plain data -- the frame, how it lies in memory
(pointer offsets, pitches) and where it goes (image size, rectangle, what dst held) -- that load_ref turns into the expected image.

The kernels walk row segments of SEG = 512 texels laid on the destination's 16-byte grid (a rectangle at an odd x starts its grid one
texel early), so the widths sit on each side of 512 and 1024 and of the 16-byte chunks of the luma (16), NV12 chroma (16) and I420
chroma (32) strings; the launcher's grid is at most 8 workgroups per CU."""
import functools

import numpy as np

import load_ref as R

SEG = 512
POISON = 0x7BCD  # an f16 pattern no case produces in every channel: what a poisoned dst holds
YUV_INSTANCES = [(layout, chroma) for chroma in R.CHROMAS for layout in R.LAYOUTS]
SURFACE_INSTANCES = [(srgb, alpha) for srgb in (False, True) for alpha in R.ALPHAS]


def yuv_instance_name(layout, chroma):
    return "k_load_yuv<%s, %s>" % ("NV12" if layout == R.NV12 else "I420", "BILINEAR" if chroma == R.BILINEAR else "REPLICATE")


def surface_instance_name(srgb, alpha):
    return "k_load_surface<%s, %s>" % ("SRGB" if srgb else "UNORM", ("STRAIGHT", "PREMULTIPLIED", "OPAQUE")[alpha])


def _rng(*key):
    return np.random.default_rng([20261021] + [int(k) for k in key])


def random_frame(w, h, *key):
    """(Y (h, w), Cb, Cr (ceil(h/2), ceil(w/2))) uint8, every code possible."""
    g = _rng(w, h, *key)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return g.integers(0, 256, (h, w), np.uint8), g.integers(0, 256, (ch, cw), np.uint8), g.integers(0, 256, (ch, cw), np.uint8)


def planes_of(y, cb, cr, layout):
    """The planes as jh_blit_yuv lays them out, each a 2-D uint8 array (rows, bytes per row)."""
    if layout == R.NV12:
        return [y, np.stack([cb, cr], axis=-1).reshape(cb.shape[0], -1)]
    return [y, cb, cr]


def _yuv(name, layout, chroma, frame, matrix=R.BT709, rng=R.LIMITED, transfer=R.NONE, at=None, image=None, prior="poison", ptr_off=(0, 0, 0),
         pitch_extra=(0, 0, 0)):
    y, cb, cr = frame
    h, w = y.shape
    return dict(name="%s %s" % (yuv_instance_name(layout, chroma), name), instance=(layout, chroma), y=y, cb=cb, cr=cr, layout=layout, chroma=chroma,
                matrix=matrix, rng=rng, transfer=transfer, rect=None if at is None else (at[0], at[1], w, h), image=image or (w, h), prior=prior,
                ptr_off=ptr_off, pitch_extra=pitch_extra)


def all_luma_frame():
    """Every Y (across x) with Cb and Cr at 0, 16, 128, 240 and 255 (one pair of rows per combination): the clamp acts at both ends."""
    levels = (0, 16, 128, 240, 255)
    combos = [(b, r) for b in levels for r in levels]
    y = np.tile(np.arange(256, dtype=np.uint8), (2 * len(combos), 1))
    cb = np.repeat(np.array([c[0] for c in combos], np.uint8)[:, None], 128, axis=1)
    cr = np.repeat(np.array([c[1] for c in combos], np.uint8)[:, None], 128, axis=1)
    return y, cb, cr


@functools.lru_cache(maxsize=None)
def tie_frame(matrix, rng):
    """A frame of constant chroma (the two modes then agree) and every Y in a row whose sums include exact ties -- a sum + 2^19 that is
    a multiple of 2^20 with the code inside [1, 255] -- so that the rounding constant shows: the (Cb, Cr) with the most ties under Y."""
    k, off = R.table(matrix, rng)
    y = np.arange(256, dtype=np.int64)[:, None, None] - off
    cb, cr = np.arange(256, dtype=np.int64)[None, :, None], np.arange(256, dtype=np.int64)[None, None, :]
    luma, u, v = 16 * k[0] * y, 16 * cb - 2048, 16 * cr - 2048
    ties = np.zeros((256, 256), np.int64)
    for s in (luma + k[1] * v + 0 * u, luma + k[2] * u + k[3] * v, luma + k[4] * u + 0 * v):
        ties += ((((s + (1 << 19)) & ((1 << 20) - 1)) == 0) & (s > 0) & (s < (255 << 20))).sum(axis=0)
    b, r = np.unravel_index(int(ties.argmax()), ties.shape)
    assert ties[b, r] > 0
    return np.tile(np.arange(256, dtype=np.uint8), (2, 1)), np.full((1, 128), b, np.uint8), np.full((1, 128), r, np.uint8)


@functools.lru_cache(maxsize=None)
def yuv_cases(instance):
    layout, chroma = instance
    out = []
    add = lambda name, frame, **kw: out.append(_yuv(name, layout, chroma, frame, **kw))  # noqa: E731
    for w, h in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (4, 5), (7, 6)):
        add("frame %dx%d" % (w, h), random_frame(w, h, 1))
    for w in (15, 16, 17, 31, 32, 33, SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1):
        for h in (1, 2, 3):
            add("width %d height %d" % (w, h), random_frame(w, h, 2))
    add("width %d at an odd offset" % SEG, random_frame(SEG, 2, 3), at=(1, 1), image=(SEG + 3, 4))
    add("width %d at an odd offset" % (SEG - 1), random_frame(SEG - 1, 3, 3), at=(1, 0), image=(SEG + 2, 3))
    for off in (1, 2, 8):
        add("plane pointers offset by %d" % off, random_frame(37, 5, 4, off), ptr_off=(off, off, off))
    add("plane pointers offset by 1, 2, 8", random_frame(37, 5, 4, 9), ptr_off=(1, 2, 8))
    frame = random_frame(48, 6, 5)
    add("all-aligned pitches", frame, pitch_extra=(16, 16, 16))  # (48, 48 or 24 + 16: multiples of 16 under NV12, and the same frame below)
    add("odd pitches", frame, pitch_extra=(1, 3, 5))
    frame = random_frame(13, 7, 6)
    for matrix in R.MATRICES:
        for rng in R.RANGES:
            for transfer in R.TRANSFERS:
                add("matrix %d range %d transfer %d" % (matrix, rng, transfer), frame, matrix=matrix, rng=rng, transfer=transfer)
    for matrix in R.MATRICES:
        for rng in R.RANGES:
            add("every Y x extreme chroma, matrix %d range %d" % (matrix, rng), all_luma_frame(), matrix=matrix, rng=rng)
            if rng == R.LIMITED:  # (in full range Ky = 2^16 and no sum of replicated chroma lands on a tie)
                add("sums on an exact tie, matrix %d range %d" % (matrix, rng), tie_frame(matrix, rng), matrix=matrix, rng=rng)
    y = random_frame(9, 7, 7)[0]
    add("constant chroma", (y, np.full((4, 5), 90, np.uint8), np.full((4, 5), 200, np.uint8)))
    board = ((np.arange(4)[:, None] + np.arange(5)[None, :]) & 1).astype(np.uint8)
    add("chroma checkerboard", (y, 16 + 224 * board, 240 - 224 * board))
    for at in ((1, 1), (3, 2), (2, 3)):
        add("rectangle at %s in a poisoned image" % (at,), random_frame(11, 5, 8, *at), at=at, image=(17, 9))
    add("never-written destination", random_frame(6, 4, 9), prior="never")
    add("never-written destination, rectangle", random_frame(6, 4, 10), at=(1, 1), image=(9, 7), prior="never")
    add("more segments than the grid", random_frame(2, 2200, 11))
    return out


def code_frame(alphas=(0, 1, 127, 128, 254, 255)):
    """(3 * len(alphas), 256, 4) uint8: per row a channel k and an alpha a; the pixel's channel k holds every code c across x, the other
    two 255 - c and (7 c + 3) mod 256 -- so colour above alpha and alpha 0 under colour both occur."""
    c = np.arange(256)
    rows = []
    for a in alphas:
        for k in range(3):
            px = np.zeros((256, 4), np.uint8)
            px[:, k], px[:, (k + 1) % 3], px[:, (k + 2) % 3], px[:, 3] = c, 255 - c, (7 * c + 3) % 256, a
            rows.append(px)
    return np.stack(rows)


def random_pixels(w, h, *key):
    return _rng(w, h, 77, *key).integers(0, 256, (h, w, 4), np.uint8)


def _surface(name, fmt, alpha, pixels, at=None, image=None, prior="poison", ptr_off=0, pitch_extra=0):
    h, w = pixels.shape[:2]
    srgb = fmt in (R.RGBA8_SRGB, R.BGRA8_SRGB)
    return dict(name="%s %s" % (surface_instance_name(srgb, alpha), name), instance=(srgb, alpha), pixels=pixels, fmt=fmt, alpha=alpha,
                rect=None if at is None else (at[0], at[1], w, h), image=image or (w, h), prior=prior, ptr_off=ptr_off, pitch_extra=pitch_extra)


@functools.lru_cache(maxsize=None)
def surface_cases(instance):
    srgb, alpha = instance
    rgba, bgra = (R.RGBA8_SRGB, R.BGRA8_SRGB) if srgb else (R.RGBA8_UNORM, R.BGRA8_UNORM)
    out = []
    add = lambda name, fmt, px, **kw: out.append(_surface(name, fmt, alpha, px, **kw))  # noqa: E731
    for fmt in (rgba, bgra):
        add("every code x six alphas, format %d" % fmt, fmt, code_frame())
    if alpha == R.PREMULTIPLIED:  # (every quotient of two codes)
        add("every code x every alpha", rgba, code_frame(range(256))[0::3])
    for w in (1, 2, 3, SEG - 1, SEG, SEG + 1, 2 * SEG + 1):
        for h in (1, 2):
            add("width %d height %d" % (w, h), rgba, random_pixels(w, h, 1))
    add("pitch above 4 * width", bgra, random_pixels(9, 5, 2), pitch_extra=12)
    add("odd pitch", rgba, random_pixels(9, 5, 3), pitch_extra=3)  # (rows at every alignment: the byte route)
    add("pointer offset by 4", rgba, random_pixels(9, 5, 4), ptr_off=4)
    add("pointer offset by 1", bgra, random_pixels(9, 5, 5), ptr_off=1)
    for at in ((1, 1), (2, 1), (3, 2)):
        add("rectangle at %s in a poisoned image" % (at,), rgba, random_pixels(10, 4, 6, *at), at=at, image=(15, 7))  # (an odd image width: both phases)
    add("width %d at an odd offset" % SEG, bgra, random_pixels(SEG, 2, 7), at=(1, 0), image=(SEG + 2, 2))
    add("never-written destination", rgba, random_pixels(6, 4, 8), prior="never")
    add("never-written destination, rectangle", rgba, random_pixels(6, 4, 9), at=(1, 1), image=(9, 7), prior="never")
    add("more segments than the grid", rgba, random_pixels(2, 2200, 10))
    return out


def prior_bits(case):
    """What dst holds before the call: (H, W, 4) uint16 of POISON, or the (H, W) of an image that is only created."""
    W, H = case["image"]
    return (H, W) if case["prior"] == "never" else np.full((H, W, 4), POISON, np.uint16)


def yuv_expected(case, **variant):
    return R.load_yuv(prior_bits(case), planes_of(case["y"], case["cb"], case["cr"], case["layout"]), case["layout"], case["matrix"], case["rng"],
                      case["transfer"], case["chroma"], case["rect"], **variant)


def surface_expected(case, **variant):
    return R.load_surface(prior_bits(case), case["pixels"], case["fmt"], case["alpha"], case["rect"], **variant)


def in_memory(rows, pitch_extra, ptr_off, canary):
    """(bytes, pitch): the 2-D uint8 array `rows` laid out with `pitch_extra` bytes of `canary` after every row but the last and
    `ptr_off` bytes in front."""
    r, rb = rows.shape
    pitch = rb + pitch_extra
    buf = np.full(ptr_off + (r - 1) * pitch + rb, canary, np.uint8)
    for i in range(r):
        buf[ptr_off + i * pitch:ptr_off + i * pitch + rb] = rows[i]
    return buf, pitch
