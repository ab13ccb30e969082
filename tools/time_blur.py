"""Device time of jh_blur on a 4096^2 RGBA16F image: the whole image and a 1024^2 rectangle in its middle, sigma = 2, 8
and 32 on both axes, both edge modes, from one image into a second one -- next to a device-to-device copy of the same rectangle
from the same run (torch's copy_ of the rectangle's view, on the same stream), which is the byte floor: 8 B read + 8 B written per
texel.  hipEvents (torch's, on the stream the context is switched to) around blocks of back-to-back launches, median of the
blocks.  Algorithmic work per texel and pass: (2 R + 1) x 4 fused multiply-adds.  Writes a JSON file (default
profiles/blur_kernel_times.json) with the times, the ratio to the copy and the fmaf rate.  Run on the GPU box; for the two kernels'
own times run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_blur.py --blocks 2`.

    python tools/time_blur.py [--blocks 7] [--per-block 10] [--out profiles/blur_kernel_times.json]
"""
import math

import numpy as np

from timing import Timer

from jello_amd import BlurEdge  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096


def main():
    t = Timer("tools/time_blur.py", 7, 10, "blur_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # colours and alphas spread over [0, 1.25), as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    src, dst = 0x71C0_0000, 0x71C1_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", (1536, 1536, 1024, 1024))):
        texels = rect[2] * rect[3]
        floor = t.record({"rect": label, "call": "device-to-device copy"}, t.timed(t.copy(rect)), more=lambda med: {
            "algorithmic_bytes": 16 * texels, "tb_per_s": round(16 * texels / (med * 1e-6) / 1e12, 3)})
        for sigma in (2.0, 8.0, 32.0):
            for edge in BlurEdge:
                launch = lambda: eng.blur(src, SIZE, SIZE, sigma, dst_image_id=dst, edge=edge, rect=None if label == "whole" else rect)  # noqa: E731
                radius = math.ceil(3 * sigma)
                fmas = 2 * (2 * radius + 1) * 4 * texels  # (the rows of the intermediate above and below a rectangle not counted)
                t.record({"rect": label, "call": "jh_blur", "sigma": sigma, "radius": radius, "edge": edge.name}, t.timed(launch), floor, lambda med: {
                    "fmaf": fmas, "tfmaf_per_s": round(fmas / (med * 1e-6) / 1e12, 2),
                    "traffic_bytes": (8 + 16 + 16 + 8) * texels, "traffic_tb_per_s": round(48 * texels / (med * 1e-6) / 1e12, 3)})
    t.finish("hipEvents around back-to-back jh_blur calls (two kernels each) from one 4096^2 image into another; the copy is torch's "
             "copy_ of the same rectangle between two tensors of the image's shape in the same run; traffic_bytes = f16 in, "
             "binary32 intermediate out and in, f16 out", SIZE)


if __name__ == "__main__":
    main()
