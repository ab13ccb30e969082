"""Device time of jh_blur on a 4096^2 RGBA16F image: the whole image and a 1024^2 rectangle in its middle, sigma = 2, 8
and 32 on both axes, both edge modes, from one image into a second one -- next to a device-to-device copy of the same rectangle
from the same run (torch's copy_ of the rectangle's view, on the same stream), which is the byte floor: 8 B read + 8 B written per
texel.  hipEvents (torch's, on the stream the context is switched to) around blocks of back-to-back launches, median of the
blocks.  Algorithmic work per texel and pass: (2 R + 1) x 4 fused multiply-adds.  Writes a JSON file (default
profiles/blur_kernel_times.json) with the times, the ratio to the copy and the fmaf rate.  Run on the GPU box; for the two kernels'
own times run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_blur.py --blocks 2`.

    python tools/time_blur.py [--blocks 7] [--per-block 10] [--out profiles/blur_kernel_times.json]
"""
import argparse
import json
import math
import os
import statistics

import numpy as np

from timing import ROOT, open_engine_on_stream, timed as timed_blocks, write_json

from jello_amd import BlurEdge  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blur_kernel_times.json"))
    a = ap.parse_args()
    import torch
    eng, stream = open_engine_on_stream()
    hip, ctx = eng.hip, eng.ctx
    rng = np.random.default_rng(1)
    # colours and alphas spread over [0, 1.25), as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    src, dst = 0x71C0_0000, 0x71C1_0000
    eng.upload_image(src, img)
    eng.upload_image(dst, img)
    with torch.cuda.stream(stream):
        ta = torch.zeros((SIZE, SIZE, 4), dtype=torch.float16, device="cuda")
        tb = torch.ones((SIZE, SIZE, 4), dtype=torch.float16, device="cuda")
    results = []
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", (1536, 1536, 1024, 1024))):
        x, y, w, h = rect
        texels = w * h

        def copy():
            with torch.cuda.stream(stream):
                tb[y:y + h, x:x + w].copy_(ta[y:y + h, x:x + w])

        times = timed_blocks(stream, copy, a.blocks, a.per_block)
        floor = statistics.median(times)
        r = {"rect": label, "call": "device-to-device copy", "us_median": round(floor, 3), "us_blocks": [round(t, 3) for t in times],
             "us_spread": round(max(times) - min(times), 3), "algorithmic_bytes": 16 * texels,
             "tb_per_s": round(16 * texels / (floor * 1e-6) / 1e12, 3)}
        results.append(r)
        print(json.dumps(r), flush=True)
        for sigma in (2.0, 8.0, 32.0):
            for edge in BlurEdge:
                launch = lambda: eng.blur(src, SIZE, SIZE, sigma, dst_image_id=dst, edge=edge, rect=None if label == "whole" else rect)  # noqa: E731
                times = timed_blocks(stream, launch, a.blocks, a.per_block)
                med = statistics.median(times)
                radius = math.ceil(3 * sigma)
                fmas = 2 * (2 * radius + 1) * 4 * texels  # (the rows of the intermediate above and below a rectangle not counted)
                r = {"rect": label, "call": "jh_blur", "sigma": sigma, "radius": radius, "edge": edge.name, "us_median": round(med, 3),
                     "us_blocks": [round(t, 3) for t in times], "us_spread": round(max(times) - min(times), 3), "copy_us_median": round(floor, 3),
                     "ratio_to_copy": round(med / floor, 2), "fmaf": fmas, "tfmaf_per_s": round(fmas / (med * 1e-6) / 1e12, 2),
                     "traffic_bytes": (8 + 16 + 16 + 8) * texels, "traffic_tb_per_s": round(48 * texels / (med * 1e-6) / 1e12, 3)}
                results.append(r)
                print(json.dumps(r), flush=True)
    eng.free_image(src)
    eng.free_image(dst)
    eng.sync()
    eng.set_stream(None)
    eng.close()
    out = {"tool": "tools/time_blur.py", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "per_block": a.per_block, "size": SIZE,
           "note": "hipEvents around back-to-back jh_blur calls (two kernels each) from one 4096^2 image into another; the copy is torch's "
                   "copy_ of the same rectangle between two tensors of the image's shape in the same run; traffic_bytes = f16 in, "
                   "binary32 intermediate out and in, f16 out",
           "results": results}
    write_json(a.out, out)


if __name__ == "__main__":
    main()
