"""Device time of jh_lut3d from one 4096^2 RGBA16F image into another: the whole image and a 1024^2 rectangle at an odd
offset, for tables of N = 17 -- in both instantiations: gathered from memory and copied into LDS, chosen through
jh_debug_lut3d_variant, the product library as it is -- 33 and 65, on three contents side by side -- constant (every lane of a wave
on one tetrahedron), a smooth gradient (a wave inside one or two cells) and random values (a tetrahedron per texel) -- next to a
device-to-device copy of the same rectangle (torch's copy_, 8 B read + 8 B written per texel), jh_color_filter without tables (a
LINEAR matrix: the same stream and no gather) and jh_color_filter with four GAMMA funcs (four 2-byte gathers), all from the same
run.  hipEvents (torch's, on the stream the context is switched to) around blocks of back-to-back calls, median of the blocks.
Every jh_lut3d result carries the estimate of DESIGN 5.23, written before the first run, and the ratio of the time to it.  Writes a
JSON file (default profiles/lut3d_kernel_times.json).  Run on the GPU box.

    python tools/time_lut3d.py [--blocks 5] [--per-block 5] [--out profiles/lut3d_kernel_times.json]
"""
import numpy as np

from timing import Timer

from jello_amd import ColorSpace, lut3d  # noqa: E402 (timing puts the root on sys.path)
from jello_amd import colorfilter as cf  # noqa: E402

SIZE = 4096
# DESIGN 5.23, before the first run.  Gathered from memory: 4 gathers a texel at 5.10's 15-19 us per gather and texel at 4096^2 on
# random content (17 taken), an eighth of it where a wave's lanes share their entries.  From LDS: a wave trip (128 texels) issues 8
# reads of 64 lanes, about 8 clocks each with the conflicts of random addresses and 2 without, on 256 CUs at 2.4 GHz; the copy of the
# table into LDS by 1 024 workgroups is 40 MB from the L2, taken as 10 us whatever the rectangle.
GATHER_US = 17.0
SHARED = {"constant": 0.125, "smooth": 0.125, "random": 1.0}
LDS_CLOCKS = {"constant": 2.0, "smooth": 2.0, "random": 8.0}
FILL_US = 10.0
CUS, CLOCK_GHZ = 256, 2.4
DENSE = (0.5, 0.25, 0.125, 0.0, 0.0625, 0.0, 0.75, 0.125, 0.0, 0.0, 0.25, 0.25, 0.25, 0.0, 0.125, 0.0, 0.0, 0.0, 1.0, 0.0)


def contents(size):
    rng = np.random.default_rng(1)
    X = np.mgrid[0:size, 0:size][1]
    ramp = (X / float(size)).astype(np.float16).view(np.uint16)
    smooth = np.stack([ramp, ramp[::-1], ramp.T, np.full((size, size), 0x3C00, np.uint16)], axis=-1)
    constant = np.empty((size, size, 4), np.uint16)
    constant[...] = np.array((0.3, 0.6, 0.45, 1.0), np.float16).view(np.uint16)
    return (("constant", constant), ("smooth", np.ascontiguousarray(smooth)), ("random", rng.random((size, size, 4)).astype(np.float16).view(np.uint16)))


def estimate_us(stream_us, rect, staged, content):
    """the stream (the table-free colour filter of the same rectangle and run) plus the gathers."""
    texels = rect[2] * rect[3]
    if staged:
        return stream_us + texels / 128.0 * 8.0 * LDS_CLOCKS[content] / (CUS * CLOCK_GHZ * 1e3) + FILL_US
    return stream_us + 4.0 * GATHER_US * SHARED[content] * texels / float(SIZE * SIZE)


def main():
    t = Timer("tools/time_lut3d.py", 5, 5, "lut3d_kernel_times.json")
    eng = t.eng
    src, dst = 0x7200_0000, 0x7200_0001
    tables = {n: 0x7201_0000 + n for n in (17, 33, 65)}
    for n, image in tables.items():
        t.upload(lut3d.as_image(lut3d.from_function(n, lambda c: c ** 0.9)), image)
    t.tensors(SIZE, SIZE)
    gamma = dict(funcs=(cf.gamma(1.0, 0.9, 0.0),) * 4, space=ColorSpace.LINEAR)
    variants = (("N = 17, from memory", 17, 1), ("N = 17, in LDS", 17, 2), ("N = 33", 33, 0), ("N = 65", 65, 0))
    t.upload(np.zeros((SIZE, SIZE, 4), np.uint16), dst)
    for content, bits in contents(SIZE):
        t.upload(bits, src)
        for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", (1531, 1537, 1024, 1024))):
            call_rect = None if label == "whole" else rect
            floor = t.record({"content": content, "rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * rect[2] * rect[3]}, t.timed(t.copy(rect)))
            stream = t.record({"content": content, "rect": label, "call": "jh_color_filter", "filter": "LINEAR matrix, no tables"},
                              t.timed(lambda: eng.color_filter(src, dst, matrix=DENSE, rect=call_rect)), floor)
            t.record({"content": content, "rect": label, "call": "jh_color_filter", "filter": "four GAMMA funcs"},
                     t.timed(lambda: eng.color_filter(src, dst, rect=call_rect, **gamma)), floor)
            for name, n, variant in variants:
                assert eng.hip.jh_debug_lut3d_variant(eng.ctx, variant) == 0
                est = estimate_us(stream, rect, variant == 2, content)
                t.record({"content": content, "rect": label, "call": "jh_lut3d", "table": name, "estimate_us": round(est, 1)},
                         t.timed(lambda n=n: eng.lut3d(src, tables[n], dst, rect=call_rect)), floor,
                         more=lambda med, est=est, stream=stream: {"ratio_to_estimate": round(med / est, 2), "ratio_to_plain_filter": round(med / stream, 2)})
            assert eng.hip.jh_debug_lut3d_variant(eng.ctx, 0) == 0
    t.finish("hipEvents around back-to-back calls from one 4096^2 image into another; the copy is torch's copy_ of the same rectangle between two tensors "
             "of the image's shape; estimate_us = the table-free jh_color_filter of the same rectangle and run + 4 gathers x 17 us x texels / 4096^2 (an "
             "eighth of it on the constant and the smooth image) from memory, or + wave trips x 8 LDS reads x 8 clocks (2 on the constant and the smooth "
             "image) over 256 CUs at 2.4 GHz + 10 us for the copies of the table, written into DESIGN 5.23 before the first run", SIZE)


if __name__ == "__main__":
    main()
