"""Device time of jh_distance on a 4096^2 RGBA16F image: the whole image and a 1024^2 rectangle at an odd offset, OUTER and
SIGNED, max_distance 4, 16, 64 and 255, edge ZERO, from one image into a second one, on four contents -- a glyph-like layer of
strokes (rings and bars 3 to 9 texels thick on a 96-texel grid), an empty image (no seed: every wave of the row pass skips its walk)
a single seed in a corner (only the waves whose staged segment holds the seed's column walk) and a seed every 512 texels both ways
(the longest walks: at R = 255 every wave finds a G <= R and most of its lanes walk all R columns) -- next to a device-to-device
copy of the same rectangle from the same run (torch's copy_ of the rectangle's view, on the same stream), which is the byte floor (8 B
read + 8 B written per texel), and next to jh_morphology STRAIGHT DILATE of the same radius.  Then Engine.round_outline (width 3.5)
next to Engine.outline (radius 4) on the strokes, onto a third image.  hipEvents (torch's, on the stream the context is switched to)
around blocks of back-to-back calls, median of the blocks; a call is two kernels.  Every result carries the estimate of DESIGN 5.20,
written before the first run -- the bytes of the two passes against the copy's rate plus the walk's steps at 56 clocks a wave step --
and the ratio of the time to it.  Writes a JSON file (default profiles/distance_kernel_times.json).  Run on the GPU box; for the
kernels' own times run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_distance.py --blocks 2`.

    python tools/time_distance.py [--blocks 5] [--per-block 5] [--out profiles/distance_kernel_times.json]
"""
import numpy as np

from timing import Timer

from jello_amd import DistanceEdge, DistanceWhich, MorphEdge, MorphOp  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
RADII = (4, 16, 64, 255)
CLOCK_GHZ, SIMDS, STEP_CLOCKS = 2.4, 256 * 4, 56.0  # the estimate's machine: 256 CUs x 4 SIMDs, 14 instructions x 4 clocks a wave step


def strokes(size):
    """(size, size) bool: rings and bars on a 96-texel grid, 3 to 9 texels thick -- a page of glyph-like strokes."""
    Y, X = np.mgrid[0:size, 0:size]
    cx, cy = X % 96 - 48, Y % 96 - 48
    thick = 3 + ((X // 96 + Y // 96) % 4) * 2
    ring = np.abs(np.hypot(cx, cy) - 30) * 2 <= thick
    bar = (np.abs(cy) * 2 <= thick) & (np.abs(cx) <= 36)
    return ring | bar


def image(mask):
    bits = np.zeros(mask.shape + (4,), np.uint16)
    bits[mask] = (0x3A00, 0x3800, 0x3400, 0x3C00)  # a colour, alpha 1
    return bits


def mean_steps(content, rect, R):
    """The walk's steps per wave step slot that the estimate takes, a number fixed before the first run.  A wave walks only where its
    staged segment (256 + 2 R columns of one row) holds a G <= R, and then for as long as its farthest lane: empty: 0.  The corner seed:
    R steps in the R + 1 rows below the seed, in the segments within R columns of it, and nowhere in a rectangle away from the corner.
    The lattice (a seed every 512 texels both ways): R steps in the rows within R of a seed row, in the segments whose staged columns
    hold a seed column.  The strokes: every wave walks, to the farthest of its 256 texels from a stroke, about 20 on the 96-texel grid."""
    w, h = rect[2], rect[3]
    if content == "empty":
        return 0.0
    if content == "corner seed":
        return 0.0 if rect[0] + rect[1] > 0 else R * (R + 1.0) * 256.0 * (1 + R // 256) / (w * h)
    if content == "lattice512":
        return R * min(1.0, (2 * R + 1) / 512.0) * min(1.0, (256 + 2 * R) / 512.0)
    return float(min(R, 20))


def estimate_us(copy_us, rect, R, which, steps):
    """bytes per texel of the two passes over the copy's 16, times the copy, plus the walk."""
    w, h = rect[2], rect[3]
    planes = 2 if which == DistanceWhich.SIGNED else 1
    seg = max(64, 2 * R)
    cols = 8.0 * (1.0 + 2.0 * R / seg) + planes * 6.0 * (w + 2.0 * R) / w
    rows = planes * 2.0 * (1.0 + 2.0 * R / 256.0) + 8.0
    walk = (w * h / 64.0) / SIMDS * steps * STEP_CLOCKS / (CLOCK_GHZ * 1e3)
    return copy_us * (cols + rows) / 16.0 + walk, cols + rows


def main():
    t = Timer("tools/time_distance.py", 5, 5, "distance_kernel_times.json")
    eng = t.eng
    src, dst, third = 0x71E0_0000, 0x71E1_0000, 0x71E2_0000
    corner = np.zeros((SIZE, SIZE), bool)
    corner[0, 0] = True
    lattice = np.zeros((SIZE, SIZE), bool)
    lattice[::512, ::512] = True
    contents = (("strokes", strokes(SIZE)), ("empty", np.zeros((SIZE, SIZE), bool)), ("corner seed", corner), ("lattice512", lattice))
    t.tensors(SIZE, SIZE)
    first = True
    for content, mask in contents:
        t.upload(image(mask), src)
        if first:
            t.upload(image(mask), dst, third)
            first = False
        for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", (1531, 1537, 1024, 1024))):
            texels = rect[2] * rect[3]
            call_rect = None if label == "whole" else rect
            floor = t.record({"content": content, "rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * texels}, t.timed(t.copy(rect)))
            for R in RADII:
                launch = lambda: eng.morphology(src, dst, op=MorphOp.DILATE, radius=R, edge=MorphEdge.ZERO, rect=call_rect, premultiplied=False)  # noqa: E731
                t.record({"content": content, "rect": label, "call": "jh_morphology", "op": "DILATE", "radius": R}, t.timed(launch), floor)
                for which in (DistanceWhich.OUTER, DistanceWhich.SIGNED):
                    scale, offset = (1.0 / (2 * R), 0.5) if which == DistanceWhich.SIGNED else (-1.0, R + 0.5)
                    launch = lambda: eng.distance(src, dst, which=which, edge=DistanceEdge.ZERO, max_distance=R, scale=scale, offset=offset,  # noqa: E731
                                                  color=(0.25, 0.5, 0.75, 1.0), rect=call_rect)
                    steps = mean_steps(content, rect, R)
                    est, bytes_per_texel = estimate_us(floor, rect, R, which, steps)
                    t.record({"content": content, "rect": label, "call": "jh_distance", "which": which.name, "max_distance": R,
                              "estimate_bytes_per_texel": round(bytes_per_texel, 2), "estimate_steps": round(steps, 1), "estimate_us": round(est, 1)},
                             t.timed(launch), floor, more=lambda med, est=est: {"ratio_to_estimate": round(med / est, 2)})
    t.upload(image(contents[0][1]), src)
    color = (0.0, 0.6, 0.2, 0.9)
    floor = t.record({"content": "strokes", "rect": "whole", "call": "device-to-device copy", "algorithmic_bytes": 16 * SIZE * SIZE}, t.timed(t.copy(None)))
    t.record({"content": "strokes", "rect": "whole", "call": "Engine.outline", "radius": 4}, t.timed(lambda: eng.outline(src, third, 4, color, dst)), floor)
    t.record({"content": "strokes", "rect": "whole", "call": "Engine.round_outline", "width": 3.5}, t.timed(lambda: eng.round_outline(src, third, 3.5, color, dst)), floor)
    t.finish("hipEvents around back-to-back jh_distance calls (two kernels each) from one 4096^2 image into another, edge ZERO; the copy is "
             "torch's copy_ of the same rectangle between two tensors of the image's shape, and jh_morphology (three kernels, STRAIGHT DILATE, the "
             "same radius) is timed in the same run; estimate_us = copy x (the passes' bytes per texel / 16) + wave steps x 56 clocks at 2.4 GHz over "
             "1024 SIMDs, written into DESIGN 5.20 before the first run; Engine.outline and Engine.round_outline are three calls each", SIZE)


if __name__ == "__main__":
    main()
