"""Device time of jh_stats on a 4096^2 RGBA16F image: the whole image and a 1024^2 rectangle at an odd offset, for the
parts BOUNDS | EXTREMES, HISTOGRAM (LINEAR and SRGB) and everything (SRGB), population ALL, on five contents side by side -- constant
(transparent black: every lane of every wave on one bin per channel), a mask (a disc of alpha 1 on transparent black: constant waves
but for those across its edge), two values alternating texel by texel, a smooth gradient (16 texels to a code: about eight codes to a
wave) and random values (about fifty codes to a wave) -- next to a device-to-device copy of the same rectangle from the same run
(torch's copy_, 8 B read + 8 B written per texel; the call reads 8 B per texel and writes 4 KB).  hipEvents (torch's, on the stream the
context is switched to) around blocks of back-to-back calls, median of the blocks; a call is two kernels.  Every result carries the
estimate of DESIGN 5.22, written before the first run, and the ratio of the time to it.  Writes a JSON file (default
profiles/stats_kernel_times.json).  Run on the GPU box; for the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_stats.py --blocks 2`.

    python tools/time_stats.py [--blocks 5] [--per-block 5] [--out profiles/stats_kernel_times.json]
"""
import numpy as np

from timing import Timer

from jello_amd import StatsTransfer, StatsWhat  # noqa: E402 (timing puts the root on sys.path)
from jello_amd.engine import STATS_RECORD_BYTES  # noqa: E402

SIZE = 4096
CLOCK_GHZ, SIMDS, CUS = 2.4, 256 * 4, 256  # the estimate's machine
# DESIGN 5.22, before the first run: instructions of a wave trip (128 texels) at 4 clocks each, and LDS clocks of its 8 bin adds
TRIP_INSTRUCTIONS = {"box": 60.0, "hist": 140.0, "hist_srgb": 200.0, "all_srgb": 240.0}
ADD_CLOCKS = {"constant": 2.0, "mask": 2.0, "alternate": 4.0, "smooth": 16.0, "random": 16.0}  # per wave instruction; the extra round costs 12 instructions
FINISH_US = 6.0


def contents(size):
    rng = np.random.default_rng(1)
    Y, X = np.mgrid[0:size, 0:size]
    disc = np.hypot(X - size / 2, Y - size / 2) <= size * 0.3
    mask = np.zeros((size, size, 4), np.uint16)
    mask[disc] = (0x3A00, 0x3800, 0x3400, 0x3C00)
    alt = np.where(((X + Y) & 1)[..., None] == 0, np.array((0x3A00, 0x3800, 0x3400, 0x3C00), np.uint16), np.array((0, 0, 0, 0), np.uint16)).astype(np.uint16)
    ramp = (X / float(size)).astype(np.float16).view(np.uint16)
    smooth = np.stack([ramp, ramp[::-1], ramp.T, np.full((size, size), 0x3C00, np.uint16)], axis=-1)
    return (("constant", np.zeros((size, size, 4), np.uint16)), ("mask", mask), ("alternate", alt), ("smooth", np.ascontiguousarray(smooth)),
            ("random", rng.random((size, size, 4)).astype(np.float16).view(np.uint16)))


def estimate_us(copy_us, rect, part, content):
    """the larger of the bytes (8 of the copy's 16 per texel), the instructions and the LDS adds of the first launch, plus
    the finish."""
    trips = rect[2] * rect[3] / 128.0
    instructions = TRIP_INSTRUCTIONS[part] + (0.0 if part == "box" or content in ("constant", "mask") else 8 * 12.0)
    valu = trips / SIMDS * instructions * 4.0 / (CLOCK_GHZ * 1e3)
    lds = 0.0 if part == "box" else trips / CUS * 8.0 * ADD_CLOCKS[content] / (CLOCK_GHZ * 1e3)
    return max(copy_us * 0.5, valu, lds) + FINISH_US


def main():
    t = Timer("tools/time_stats.py", 5, 5, "stats_kernel_times.json")
    eng = t.eng
    src = 0x71F0_0000
    out = eng._own_buffer(0x71F1_0000, STATS_RECORD_BYTES)
    t.tensors(SIZE, SIZE)
    parts = (("box", StatsWhat.BOUNDS | StatsWhat.EXTREMES, StatsTransfer.LINEAR), ("hist", StatsWhat.HISTOGRAM, StatsTransfer.LINEAR),
             ("hist_srgb", StatsWhat.HISTOGRAM, StatsTransfer.SRGB), ("all_srgb", StatsWhat.ALL, StatsTransfer.SRGB))
    for content, bits in contents(SIZE):
        t.upload(bits, src)
        for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", (1531, 1537, 1024, 1024))):
            call_rect = None if label == "whole" else rect
            floor = t.record({"content": content, "rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * rect[2] * rect[3]}, t.timed(t.copy(rect)))
            for part, what, transfer in parts:
                launch = lambda: eng.stats(src, rect=call_rect, what=what, threshold=2.0 ** -24, transfer=transfer, out_device_ptr=out)  # noqa: E731
                est = estimate_us(floor, rect, part, content)
                t.record({"content": content, "rect": label, "call": "jh_stats", "parts": part, "estimate_us": round(est, 1)}, t.timed(launch), floor,
                         more=lambda med, est=est: {"ratio_to_estimate": round(med / est, 2)})
    eng.hip.jh_free(eng.ctx, 0x71F1_0000)
    t.finish("hipEvents around back-to-back jh_stats calls (two kernels each) on one 4096^2 image, population ALL, content = alpha >= 2^-24; the copy "
             "is torch's copy_ of the same rectangle between two tensors of the image's shape; estimate_us = max(copy / 2, wave trips x instructions x 4 "
             "clocks over 1024 SIMDs, wave trips x 8 adds x LDS clocks over 256 CUs) at 2.4 GHz + 6 us for the finish, written into DESIGN 5.22 before the "
             "first run", SIZE)


if __name__ == "__main__":
    main()
