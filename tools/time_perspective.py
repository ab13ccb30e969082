"""Device time of jh_perspective into a 4096^2 RGBA16F image from a 4096^2 source: NEAREST, BILINEAR and BICUBIC,
premultiplied, edge ZERO; the whole image and a 1024^2 destination rectangle at an odd offset; under three matrices -- "identity" as a
3 x 3 matrix, "keystone": perspective.rotate_y(30 degrees, distance 8192) about the centre, "horizon": perspective.rotate_x(60 degrees,
distance 2048) about the centre, whose horizon crosses the image at row 866 (the rows above it are void: no loads) -- next to jh_warp
under the identity with the same filter and next to a device-to-device copy of the same rectangle, both from the same run (torch's
copy_ of the rectangle's view, on the same stream: 8 B read + 8 B written per texel).  hipEvents (torch's, on the stream the context
is switched to) around blocks of back-to-back calls, median of the blocks; each call is one kernel.  Writes a JSON file (default
profiles/perspective_kernel_times.json) with, per entry, the ratio to the estimate DESIGN 5.19 wrote down before the first run
(estimate() below) first, then the times and the ratio to the copy.  Run on the GPU box.

    python tools/time_perspective.py [--blocks 5] [--per-block 5] [--out profiles/perspective_kernel_times.json]
"""
import math

import numpy as np

from timing import Timer, median

from jello_amd import WarpEdge, WarpFilter, perspective, perspective_plan  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
RECT = (1531, 1537, 1024, 1024)
IDENTITY6 = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
TAPS = (1, 2, 4)  # per axis
CENTRE = (SIZE / 2.0, SIZE / 2.0)
MATRICES = (("identity", perspective.affine(IDENTITY6)["matrix"]),
            ("keystone", perspective.rotate_y(math.radians(30.0), 8192.0, CENTRE)["matrix"]),
            ("horizon", perspective.rotate_x(math.radians(60.0), 2048.0, CENTRE)["matrix"]))
# us per 4096^2 texels, written into DESIGN 5.19 before the first timing run: the position's 52 binary64-rate instructions at 4.3
# cycles and one v_rcp_f64 at 16 per wave and SIMD, 262 144 waves over 1 024 SIMDs at 2.4 GHz, not overlapped with anything
POSITION_US = 25.6


def live_share(matrix, rect):
    """The share of the rectangle's texels that are in front (den > 0): the others store zeros and load nothing."""
    G = perspective_plan(matrix)
    x, y, w, h = rect
    xs, ys = (np.arange(x, x + w) + 0.5)[None, :], (np.arange(y, y + h) + 0.5)[:, None]
    return float(np.mean(((G[6] * xs) + (G[7] * ys)) + G[8] > 0.0))


def estimate(warp_us, texels, live):
    """The same run's jh_warp time for the texels that load, plus the position's arithmetic for all of them."""
    return warp_us * live + POSITION_US * texels / float(SIZE * SIZE)


def main():
    t = Timer("tools/time_perspective.py", 5, 5, "perspective_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # colours and alphas spread over [0, 1.25), as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    src, dst = 0x7E00_0000, 0x7E01_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", RECT)):
        x, y, w, h = rect
        call_rect = None if label == "whole" else rect
        floor = t.record({"rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * w * h}, t.timed(t.copy(rect)))
        for filt in WarpFilter:
            launch = lambda: eng.warp(src, dst, IDENTITY6, filter=filt, edge=WarpEdge.ZERO, dst_rect=call_rect)  # noqa: E731
            warp_us = t.record({"rect": label, "call": "jh_warp", "case": "identity", "filter": filt.name, "taps": TAPS[int(filt)] ** 2}, t.timed(launch), floor)
            for name, matrix in MATRICES:
                launch = lambda: eng.perspective(src, dst, matrix, filter=filt, edge=WarpEdge.ZERO, dst_rect=call_rect)  # noqa: E731
                times = t.timed(launch)
                live = live_share(matrix, rect)
                est = estimate(warp_us, w * h, live)
                r = {"rect": label, "call": "jh_perspective", "case": name, "filter": filt.name, "taps": TAPS[int(filt)] ** 2,
                     "measured_over_estimate": round(median(times) / est, 2), "estimate_us": round(est, 1), "live_share": round(live, 4),
                     "over_warp": round(median(times) / warp_us, 2)}
                t.record(r, times, floor)
    t.finish("hipEvents around back-to-back jh_perspective calls (one kernel each) into a 4096^2 image from a 4096^2 source, premultiplied, "
             "edge ZERO; matrices: the identity as 3 x 3, rotate_y(30 degrees, distance 8192) and rotate_x(60 degrees, distance 2048, horizon at "
             "row 866) about the centre; jh_warp under the identity with the same filter and torch's copy_ of the same rectangle are timed in "
             "the same run; estimate_us is that jh_warp time times the share of texels in front plus what DESIGN 5.19 wrote down for the "
             "position before the first timing run", SIZE)


if __name__ == "__main__":
    main()
