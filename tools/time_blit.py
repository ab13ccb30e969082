"""Device time of jh_blit (the RenderToSurface blit pass) per surface format at 4096^2 and 2048^2: hipEvents (torch's, on the
stream the context is switched to) around blocks of back-to-back blits, median of the blocks.  Algorithmic bytes: 8 read +
4 written per pixel.  Writes a JSON file (default profiles/blit_timing.json).  Run on the GPU box; for kernel times run it
under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_blit.py --blocks 2`.

    python tools/time_blit.py [--blocks 7] [--per-block 20] [--out profiles/blit_timing.json]
"""
import argparse
import json
import os
import statistics

import numpy as np

from timing import ROOT, open_engine_on_stream, timed, write_json

from jello_amd import Surface  # noqa: E402 (timing puts the root on sys.path)



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blit_timing.json"))
    a = ap.parse_args()
    import torch
    eng, stream = open_engine_on_stream()
    hip, ctx = eng.hip, eng.ctx
    rng = np.random.default_rng(1)
    results = []
    for size in (4096, 2048):
        n = size * size
        # colours and alphas spread over [0, 1.25) (some values above 1 clamp), as a fine stage leaves them
        img = (rng.random((size, size, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
        src, dst = 0x71BE_0000 + size, 0x71BF_0000 + size
        eng.upload_image(src, img)
        eng._check(hip.jh_buffer_create(ctx, dst, 4 * n), "buffer_create")
        ptr = hip.jh_buffer_device_ptr(ctx, dst)
        for fmt in Surface:
            times = timed(stream, lambda: eng._check(hip.jh_blit(ctx, src, ptr, 4 * size, size, size, int(fmt)), "blit"), a.blocks, a.per_block)
            med = statistics.median(times)
            r = {"size": size, "format": fmt.name, "us_median": round(med, 3), "us_blocks": [round(t, 3) for t in times],
                 "algorithmic_bytes": 12 * n, "tb_per_s": round(12 * n / (med * 1e-6) / 1e12, 3)}
            results.append(r)
            print(json.dumps(r), flush=True)
        hip.jh_free(ctx, dst)
        eng.free_image(src)
    eng.sync()
    eng.set_stream(None)
    eng.close()
    out = {"tool": "tools/time_blit.py", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "per_block": a.per_block,
           "note": "hipEvents around back-to-back blits of one source into one surface (both stay in the 256 MiB Infinity "
                   "Cache at 4096^2: 201 MB); kernel times: the rocprofv3 stats file next to this one",
           "results": results}
    write_json(a.out, out)


if __name__ == "__main__":
    main()
