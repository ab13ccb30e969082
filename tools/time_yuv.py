"""Device time of jh_blit_yuv (the YUV blit) per layout and transfer at 4096^2 and 2048^2 and, in the same run on
the same source image, of jh_blit in RGBA8_UNORM and RGBA8_SRGB -- the yardstick: the blit of the same transfer.  hipEvents
(torch's, on the stream the context is switched to) around blocks of back-to-back launches, median of the blocks.  Matrix
and range are kernel arguments: one case each (BT.601 full next to the BT.709 limited every other case uses).  Algorithmic
bytes: 8 read + 1.5 written per pixel, against the blit's 8 + 4.  Writes a JSON file (default
profiles/yuv_kernel_times.json) with both sets of numbers and, per YUV case, whether it is no slower than its yardstick
within the yardstick's own block-to-block spread (max - min of its blocks).  Run on the GPU box.

    python tools/time_yuv.py [--blocks 7] [--per-block 20] [--out profiles/yuv_kernel_times.json]
"""
import argparse
import ctypes
import json
import os
import statistics

import numpy as np

from timing import ROOT, open_engine_on_stream, timed as timed_blocks, write_json

from jello_amd import Surface, YuvLayout, YuvMatrix, YuvRange, YuvTransfer  # noqa: E402 (timing puts the root on sys.path)



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_kernel_times.json"))
    a = ap.parse_args()
    import torch
    eng, stream = open_engine_on_stream()
    hip, ctx = eng.hip, eng.ctx
    rng = np.random.default_rng(1)

    def timed(launch):
        return timed_blocks(stream, launch, a.blocks, a.per_block)

    blits, yuvs = [], []
    for size in (4096, 2048):
        n = size * size
        # colours and alphas spread over [0, 1.25) (some values above 1 clamp), as a fine stage leaves them
        img = (rng.random((size, size, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
        src, dst = 0x71BE_0000 + size, 0x71BF_0000 + size
        eng.upload_image(src, img)
        eng._check(hip.jh_buffer_create(ctx, dst, 4 * n), "buffer_create")  # the surface; the YUV planes use its first 1.5 n bytes
        ptr = hip.jh_buffer_device_ptr(ctx, dst)
        yard = {}
        for fmt, transfer in ((Surface.RGBA8_UNORM, YuvTransfer.NONE), (Surface.RGBA8_SRGB, YuvTransfer.SRGB)):
            times = timed(lambda: eng._check(hip.jh_blit(ctx, src, ptr, 4 * size, size, size, int(fmt)), "blit"))
            med = statistics.median(times)
            r = {"size": size, "call": "jh_blit", "format": fmt.name, "us_median": round(med, 3), "us_blocks": [round(t, 3) for t in times],
                 "us_spread": round(max(times) - min(times), 3), "algorithmic_bytes": 12 * n,
                 "tb_per_s": round(12 * n / (med * 1e-6) / 1e12, 3)}
            yard[transfer] = r
            blits.append(r)
            print(json.dumps(r), flush=True)
        cases = [(layout, YuvMatrix.BT709, YuvRange.LIMITED, transfer) for layout in YuvLayout for transfer in YuvTransfer]
        cases.append((YuvLayout.NV12, YuvMatrix.BT601, YuvRange.FULL, YuvTransfer.NONE))
        for layout, matrix, rng_, transfer in cases:
            d, _ = eng._yuv_desc(size, size, layout, matrix, rng_, transfer,
                                 [(ptr, None), (ptr + n, None)] if layout == YuvLayout.NV12 else [(ptr, None), (ptr + n, None), (ptr + n + n // 4, None)])
            times = timed(lambda: eng._check(hip.jh_blit_yuv(ctx, src, size, size, ctypes.byref(d)), "blit_yuv"))
            med = statistics.median(times)
            y = yard[transfer]
            r = {"size": size, "call": "jh_blit_yuv", "layout": layout.name, "matrix": matrix.name, "range": rng_.name,
                 "transfer": transfer.name, "us_median": round(med, 3), "us_blocks": [round(t, 3) for t in times],
                 "us_spread": round(max(times) - min(times), 3), "algorithmic_bytes": 19 * n // 2,
                 "tb_per_s": round(9.5 * n / (med * 1e-6) / 1e12, 3), "yardstick": "jh_blit " + y["format"],
                 "yardstick_us_median": y["us_median"], "yardstick_us_spread": y["us_spread"],
                 "no_slower_than_yardstick": bool(med <= y["us_median"] + y["us_spread"])}
            yuvs.append(r)
            print(json.dumps(r), flush=True)
        hip.jh_free(ctx, dst)
        eng.free_image(src)
    eng.sync()
    eng.set_stream(None)
    eng.close()
    out = {"tool": "tools/time_yuv.py", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "per_block": a.per_block,
           "note": "hipEvents around back-to-back launches of one source into one destination (both stay in the Infinity Cache); "
                   "the yardstick of a jh_blit_yuv case is the jh_blit of the same transfer from this run, the margin that "
                   "blit's own max - min over its blocks",
           "blit": blits, "blit_yuv": yuvs}
    write_json(a.out, out)


if __name__ == "__main__":
    main()
