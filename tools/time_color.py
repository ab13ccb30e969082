"""Device time of jh_color_filter at 4096^2 RGBA16F: one image into a second one, the whole image and a 1024^2
rectangle at an odd offset (1537, 1535), for four filters -- a linear-space matrix alone (no tables: the TABLES = false kernel),
grayscale (SRGB space: three PRE and three POST tables), brightness (SRGB space, identity matrix, the same six tables plus LINEAR
funcs in them) and GAMMA on all four channels in LINEAR space (four POST tables) -- next to a device-to-device copy of the same
rectangle (torch's copy_ of the rectangle's view on the same stream: 8 B read + 8 B written per texel, what the filter moves too)
and next to jh_composite Normal + SrcOver of the same rectangle (16 B read, 8 B written), all from the same run.  Each filter runs
once before it is timed, so the timed calls find their tables resident.  hipEvents (torch's, on the stream the context is switched
to) around blocks of back-to-back launches, median of the blocks.  Writes a JSON file (default profiles/color_kernel_times.json) with
the times, the ratios to the copy and to the composite, and the traffic rate.  Run on the GPU box.

    python tools/time_color.py [--blocks 7] [--per-block 10] [--out profiles/color_kernel_times.json]
"""
import argparse
import json
import os
import statistics

import numpy as np

from timing import ROOT, open_engine_on_stream, timed as timed_blocks, write_json

from jello_amd import ColorSpace, colorfilter as cf  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
MATRIX = (0.9, 0.1, -0.05, 0.0, 0.02, 0.05, 0.85, 0.1, 0.0, 0.0, -0.1, 0.2, 0.9, 0.0, 0.01, 0.0, 0.0, 0.0, 0.8, 0.1)
FILTERS = [("linear matrix (no tables)", dict(matrix=MATRIX, funcs=None, space=ColorSpace.LINEAR, clamp=True)),
           ("grayscale (SRGB: 3 PRE + 3 POST)", cf.grayscale(1.0)),
           ("brightness (SRGB, identity matrix)", cf.brightness(1.5)),
           ("four GAMMA funcs (LINEAR: 4 POST)", dict(matrix=None, funcs=(cf.gamma(1.0, 2.2, 0.0),) * 4, space=ColorSpace.LINEAR, clamp=True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_kernel_times.json"))
    a = ap.parse_args()
    import torch
    eng, stream = open_engine_on_stream()
    rng = np.random.default_rng(1)
    # colours spread over [0, 1.25) and alphas over [0, 1], as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * np.array([1.25, 1.25, 1.25, 1.0], np.float32)).astype(np.float16).view(np.uint16)
    src, dst = 0x71C4_0000, 0x71C5_0000
    eng.upload_image(src, img)
    eng.upload_image(dst, img)
    with torch.cuda.stream(stream):
        ta = torch.zeros((SIZE, SIZE, 4), dtype=torch.float16, device="cuda")
        tb = torch.ones((SIZE, SIZE, 4), dtype=torch.float16, device="cuda")
    results = []

    def record(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    def entry(times):
        return {"us_median": round(statistics.median(times), 3), "us_blocks": [round(t, 3) for t in times], "us_spread": round(max(times) - min(times), 3)}

    for label, rect, (x, y, w, h) in (("whole", None, (0, 0, SIZE, SIZE)), ("rect1024_odd", (1537, 1535, 1024, 1024), (1537, 1535, 1024, 1024))):
        texels = w * h

        def copy():
            with torch.cuda.stream(stream):
                tb[y:y + h, x:x + w].copy_(ta[y:y + h, x:x + w])

        times = timed_blocks(stream, copy, a.blocks, a.per_block)
        floor = statistics.median(times)
        record(dict({"rect": label, "call": "device-to-device copy"}, **entry(times), algorithmic_bytes=16 * texels,
                    tb_per_s=round(16 * texels / (floor * 1e-6) / 1e12, 3)))
        over = lambda: eng.composite(src, dst, src_rect=rect, offset=(x, y))  # noqa: E731
        times = timed_blocks(stream, over, a.blocks, a.per_block)
        comp = statistics.median(times)
        record(dict({"rect": label, "call": "jh_composite", "mode": "Normal+SrcOver"}, **entry(times), copy_us_median=round(floor, 3),
                    ratio_to_copy=round(comp / floor, 2), algorithmic_bytes=24 * texels, tb_per_s=round(24 * texels / (comp * 1e-6) / 1e12, 3)))
        for name, kw in FILTERS:
            launch = lambda: eng.color_filter(src, dst, rect=rect, **kw)  # noqa: E731
            launch()  # (the filter's tables become resident: the timed calls upload nothing)
            times = timed_blocks(stream, launch, a.blocks, a.per_block)
            med = statistics.median(times)
            record(dict({"rect": label, "call": "jh_color_filter", "filter": name}, **entry(times), copy_us_median=round(floor, 3),
                        ratio_to_copy=round(med / floor, 2), composite_us_median=round(comp, 3), ratio_to_composite=round(med / comp, 2),
                        algorithmic_bytes=16 * texels, tb_per_s=round(16 * texels / (med * 1e-6) / 1e12, 3)))
    eng.free_image(src)
    eng.free_image(dst)
    eng.sync()
    eng.set_stream(None)
    eng.close()
    out = {"tool": "tools/time_color.py", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "per_block": a.per_block, "size": SIZE,
           "note": "hipEvents around back-to-back jh_color_filter calls (one kernel each, tables resident) from one 4096^2 image into another; "
                   "the copy is torch's copy_ of the same rectangle between two tensors of the image's shape and jh_composite blends the same "
                   "rectangle of the same two images, in the same run; algorithmic_bytes = 8 in, 8 out per texel (the tables, 1.25 MB at most, "
                   "are not counted)",
           "results": results}
    write_json(a.out, out)


if __name__ == "__main__":
    main()
