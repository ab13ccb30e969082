"""Device time of jh_composite at 4096^2 RGBA16F: one image onto a second one, the whole image and a 1024^2 rectangle
placed at an odd offset (1537, 1535; once with the source's pairs 16-byte aligned, once 8-byte aligned only), for Normal + SrcOver, Normal + SrcOver with a
tint, Multiply and Hue -- next to a device-to-device copy of the same rectangle (torch's copy_ of the rectangle's view, on the same
stream: 8 B read + 8 B written per texel, where the composite reads 16 and writes 8) and next to jh_blit of the whole image (8 B
read, 4 B written), all from the same run.  hipEvents (torch's, on the stream the context is switched to) around blocks of
back-to-back launches, median of the blocks.  Writes a JSON file (default profiles/composite_kernel_times.json) with the times,
the ratio to the copy and the traffic rate.  Run on the GPU box.

    python tools/time_composite.py [--blocks 7] [--per-block 10] [--out profiles/composite_kernel_times.json]
"""
import argparse
import json
import os
import statistics

import numpy as np

from timing import ROOT, open_engine_on_stream, timed as timed_blocks, write_json

from jello_amd import Compose, Mix, Surface  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
MODES = [("Normal+SrcOver", Mix.Normal, None), ("Normal+SrcOver, tint", Mix.Normal, (0.0, 0.0, 0.0, 0.5)), ("Multiply+SrcOver", Mix.Multiply, None),
         ("Hue+SrcOver", Mix.Hue, None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_kernel_times.json"))
    a = ap.parse_args()
    import torch
    eng, stream = open_engine_on_stream()
    hip, ctx = eng.hip, eng.ctx
    rng = np.random.default_rng(1)
    # colours spread over [0, 1.25) and alphas over [0, 1], as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * np.array([1.25, 1.25, 1.25, 1.0], np.float32)).astype(np.float16).view(np.uint16)
    src, dst = 0x71C2_0000, 0x71C3_0000
    eng.upload_image(src, img)
    eng.upload_image(dst, img)
    with torch.cuda.stream(stream):
        ta = torch.zeros((SIZE, SIZE, 4), dtype=torch.float16, device="cuda")
        tb = torch.ones((SIZE, SIZE, 4), dtype=torch.float16, device="cuda")
        surface = torch.zeros((SIZE, SIZE, 4), dtype=torch.uint8, device="cuda")
    results = []

    def record(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    def blit():
        eng.blit(src, SIZE, SIZE, Surface.RGBA8_UNORM, out_device_ptr=surface.data_ptr())

    times = timed_blocks(stream, blit, a.blocks, a.per_block)
    med = statistics.median(times)
    record({"rect": "whole", "call": "jh_blit RGBA8_UNORM", "us_median": round(med, 3), "us_blocks": [round(t, 3) for t in times],
            "us_spread": round(max(times) - min(times), 3), "algorithmic_bytes": 12 * SIZE * SIZE, "tb_per_s": round(12 * SIZE * SIZE / (med * 1e-6) / 1e12, 3)})
    # dx is odd: dst's pairs start at the rectangle's second texel.  Read from sx = 1 the source's pairs are 16-byte aligned there
    # too (sx - dx even), read from sx = 2 they are not and load as two 8-byte halves.
    for label, src_rect, offset, (x, y, w, h) in (("whole", None, (0, 0), (0, 0, SIZE, SIZE)),
                                                  ("rect1024_odd", (1, 2, 1024, 1024), (1537, 1535), (1537, 1535, 1024, 1024)),
                                                  ("rect1024_odd_src_unaligned", (2, 2, 1024, 1024), (1537, 1535), (1537, 1535, 1024, 1024))):
        texels = w * h

        def copy():
            with torch.cuda.stream(stream):
                tb[y:y + h, x:x + w].copy_(ta[y:y + h, x:x + w])

        times = timed_blocks(stream, copy, a.blocks, a.per_block)
        floor = statistics.median(times)
        record({"rect": label, "call": "device-to-device copy", "us_median": round(floor, 3), "us_blocks": [round(t, 3) for t in times],
                "us_spread": round(max(times) - min(times), 3), "algorithmic_bytes": 16 * texels, "tb_per_s": round(16 * texels / (floor * 1e-6) / 1e12, 3)})
        for name, mix, tint in MODES:
            launch = lambda: eng.composite(src, dst, mix, Compose.SrcOver, 1.0, tint, src_rect, offset)  # noqa: E731
            times = timed_blocks(stream, launch, a.blocks, a.per_block)
            med = statistics.median(times)
            record({"rect": label, "call": "jh_composite", "mode": name, "us_median": round(med, 3), "us_blocks": [round(t, 3) for t in times],
                    "us_spread": round(max(times) - min(times), 3), "copy_us_median": round(floor, 3), "ratio_to_copy": round(med / floor, 2),
                    "algorithmic_bytes": 24 * texels, "tb_per_s": round(24 * texels / (med * 1e-6) / 1e12, 3)})
    eng.free_image(src)
    eng.free_image(dst)
    eng.sync()
    eng.set_stream(None)
    eng.close()
    out = {"tool": "tools/time_composite.py", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "per_block": a.per_block, "size": SIZE,
           "note": "hipEvents around back-to-back jh_composite calls (one kernel each) from one 4096^2 image onto another, which is blended "
                   "over and over (the values drift towards the blend's fixed point; the bytes moved do not change); the copy is torch's copy_ "
                   "of the same rectangle between two tensors of the image's shape in the same run; algorithmic_bytes = 8 source + 8 backdrop "
                   "in, 8 out per texel",
           "results": results}
    write_json(a.out, out)


if __name__ == "__main__":
    main()
