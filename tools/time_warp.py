"""Device time of jh_warp into a 4096^2 RGBA16F image: the identity, a 30 degree rotation about the centre (both from a
4096^2 source) and a 2048^2 source scaled up 2 x; each with NEAREST, BILINEAR and BICUBIC, premultiplied, edge ZERO; the whole image
and a 1024^2 destination rectangle at an odd offset -- next to a device-to-device copy of the same rectangle from the same run
(torch's copy_ of the rectangle's view, on the same stream), which is the byte floor (8 B read + 8 B written per texel), and, for the
axis-aligned cases, next to jh_resample TRIANGLE / CATMULL_ROM at the same shape.  hipEvents (torch's, on the stream the context is
switched to) around blocks of back-to-back calls, median of the blocks; a warp is one kernel, a resample two.  Writes a JSON file
(default profiles/warp_kernel_times.json) with the times and the ratio to the copy.  Run on the GPU box; for the kernels' own times
run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_warp.py --blocks 2`.

    python tools/time_warp.py [--blocks 5] [--per-block 5] [--out profiles/warp_kernel_times.json]
"""
import math

import numpy as np

from timing import Timer

from jello_amd import ResampleFilter, WarpEdge, WarpFilter  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
HALF = SIZE // 2
RECT = (1531, 1537, 1024, 1024)


def rotation(deg, size):
    t, c = math.radians(deg), size / 2.0
    a, b = math.cos(t), math.sin(t)
    return (a, b, -b, a, c - (a * c - b * c), c - (b * c + a * c))


def main():
    t = Timer("tools/time_warp.py", 5, 5, "warp_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # colours and alphas spread over [0, 1.25), as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    src, small, dst = 0x71E0_0000, 0x71E1_0000, 0x71E2_0000
    t.upload(img, src, dst)
    t.upload(img[:HALF, :HALF], small)
    t.tensors(SIZE, SIZE)
    cases = (("identity", src, (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), None), ("rotate30", src, rotation(30, SIZE), None),
             ("up2", small, (2.0, 0.0, 0.0, 2.0, 0.0, 0.0), HALF))
    resample_of = {WarpFilter.BILINEAR: ResampleFilter.TRIANGLE, WarpFilter.BICUBIC: ResampleFilter.CATMULL_ROM}
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", RECT)):
        x, y, w, h = rect
        call_rect = None if label == "whole" else rect
        floor = t.record({"rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * w * h}, t.timed(t.copy(rect)))
        for name, source, matrix, up_from in cases:
            for filt in WarpFilter:
                launch = lambda: eng.warp(source, dst, matrix, filter=filt, edge=WarpEdge.ZERO, dst_rect=call_rect)  # noqa: E731
                t.record({"rect": label, "call": "jh_warp", "case": name, "filter": filt.name, "taps": (1, 4, 16)[int(filt)]}, t.timed(launch), floor)
            if name == "rotate30":
                continue
            # the same shape through jh_resample: the source rectangle the destination rectangle is the image of
            k = 1 if up_from is None else 2
            src_rect = None if label == "whole" else (x // k, y // k, w // k, h // k)
            for filt, rfilt in resample_of.items():
                launch = lambda: eng.resample(source, dst, rfilt, src_rect=src_rect, dst_rect=call_rect)  # noqa: E731
                t.record({"rect": label, "call": "jh_resample", "case": name, "filter": rfilt.name, "beside": filt.name}, t.timed(launch), floor)
    t.finish("hipEvents around back-to-back jh_warp calls (one kernel each) into a 4096^2 image, premultiplied, edge ZERO; the copy is "
             "torch's copy_ of the same rectangle between two tensors of the image's shape, and jh_resample (two kernels) at the same "
             "shape is timed in the same run for the axis-aligned cases (its source rectangle is the destination rectangle's preimage, "
             "rounded down at the odd offset)", SIZE)


if __name__ == "__main__":
    main()
