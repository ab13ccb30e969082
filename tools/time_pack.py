"""Device time of jh_pack_tiles / jh_unpack_tiles next to a device-to-device copy of the same frame's bytes measured in the
same run (the yardstick), and the host time of pack + read_pack next to jh_download of the whole frame (what the feature is
for).  4096^2 and 2048^2, 4- and 8-byte texels; frames: all RAW (noise), all SOLID (flat), all SKIP (noise against itself),
and the rendered C3 / C4 frames (the 8-bit sRGB surface, the RGBA16F target), packed without a reference.

hipEvents (torch's, on the stream the context is switched to) around blocks of back-to-back calls, median of the blocks;
host times are perf_counter around calls that end in the download's synchronise, median of the repetitions.  Algorithmic
bytes of a pack: the frame read once per pass that needs it plus the pack written.  Writes a JSON file
(default profiles/pack_kernel_times.json).  Run on the GPU box; for kernel times run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_pack.py --blocks 3 --out DIR/times.json`.

    python tools/time_pack.py [--blocks 21] [--per-block 10] [--host-reps 21] [--sizes 4096 2048] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import time

import numpy as np

from timing import ROOT, open_engine_on_stream, timed, write_json

import jello_amd  # noqa: E402 (timing puts the root on sys.path)
from jello_amd import Surface, scenes, tilepack  # noqa: E402

_ids = [0x71C0_0000_0000]


def new_buffer(eng, nbytes, data=None):
    _ids[0] += 1
    bid = _ids[0]
    if data is None:
        eng._check(eng.hip.jh_buffer_create(eng.ctx, bid, nbytes), "buffer_create")
    else:
        eng._check(eng.hip.jh_upload(eng.ctx, bid, data.ctypes.data, data.nbytes), "upload")
    return bid, eng.hip.jh_buffer_device_ptr(eng.ctx, bid)


def rendered(eng, name, size, tb):
    """(buffer id, pointer) of a rendered frame in device memory: the sRGB surface (tb 4) or the RGBA16F target (tb 8)."""
    if name == "c3":  # the benchmark's density: 100 k paths at 4096^2
        s, p = scenes.scene_c3(100_000 * size * size // (4096 * 4096), size)
    else:  # 30 k paths under clips, gradients and blends, whatever the size
        s, p = scenes.scene_c4(30_000, size)
    p.bump = jello_amd.BumpSizes(lines=1 << 23, seg_counts=1 << 24, segments=1 << 24, tiles=1 << 23, ptcl=1 << 27, bin_data=1 << 22,
                                 blend_spill=1 << 26)
    bid, ptr = new_buffer(eng, size * size * tb)
    if tb == 4:
        _, _, bump, _ = eng.render_to_surface(s, p, Surface.RGBA8_SRGB, out_device_ptr=ptr)
    else:
        _, bump, _ = eng.render(s, p, out_device_ptr=ptr)
    assert bump["failed"] == 0, (name, size, bump)
    eng.sync()
    return bid, ptr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=21)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 2048])
    ap.add_argument("--frames", nargs="+", default=["all_raw", "all_solid", "all_skip", "c3", "c4"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_kernel_times.json"))
    a = ap.parse_args()
    import torch
    eng, stream = open_engine_on_stream()
    hip, ctx = eng.hip, eng.ctx
    rt = ctypes.CDLL("libamdhip64.so")
    rt.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    rng = np.random.default_rng(1)

    def device_us(fn):
        times = timed(stream, fn, a.blocks, a.per_block)
        return round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)

    def host_us(fn):
        for _ in range(2):
            fn()
        times = []
        for _ in range(a.host_reps):
            eng.sync()
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e6)
        return round(statistics.median(times), 1), round(min(times), 1), round(max(times), 1)

    results = []
    for size in a.sizes:
        for tb in (4, 8):
            frame_bytes = size * size * tb
            cap = tilepack.bound(size, size, tb)
            pack_id, pack_ptr = new_buffer(eng, cap)
            out_id, out_ptr = new_buffer(eng, frame_bytes)
            host_frame = np.empty(frame_bytes, np.uint8)
            for name in a.frames:
                ref_id = ref_ptr = None
                if name in ("c3", "c4"):
                    src_id, src_ptr = rendered(eng, name, size, tb)
                else:
                    if name == "all_solid":
                        data = np.full(frame_bytes, 0x5C, np.uint8)
                    else:
                        data = rng.integers(0, 256, size=frame_bytes, dtype=np.uint8)
                    src_id, src_ptr = new_buffer(eng, frame_bytes, data)
                    if name == "all_skip":
                        ref_id, ref_ptr = new_buffer(eng, frame_bytes, data)
                pitch = size * tb

                def do_pack():
                    eng._check(hip.jh_pack_tiles(ctx, src_ptr, pitch, ref_ptr, pitch if ref_ptr else 0, size, size, tb, pack_ptr, cap), "pack")

                def do_copy():
                    assert rt.hipMemcpyDtoDAsync(out_ptr, src_ptr, frame_bytes, stream.cuda_stream) == 0

                do_pack()
                pack = eng.read_pack(pack_ptr, cap)
                hdr = tilepack.parse_header(pack)

                def do_unpack():
                    eng._check(hip.jh_unpack_tiles(ctx, pack_ptr, len(pack), out_ptr, pitch, size, size, tb), "unpack")

                def do_pack_and_read():
                    do_pack()
                    eng.read_pack(pack_ptr, cap)

                def do_download():
                    eng._check(hip.jh_download(ctx, src_id, host_frame.ctypes.data, 0, frame_bytes), "download")

                copy_us = device_us(do_copy)
                pack_us = device_us(do_pack)
                unpack_us = device_us(do_unpack)
                copy_us2 = device_us(do_copy)  # the yardstick once more: its own spread within the run
                n_pass1 = 2 if ref_ptr else 1
                raw_bytes = 256 * tb * hdr["n_raw"]
                r = {"size": size, "texel_bytes": tb, "frame": name, "frame_bytes": frame_bytes, "pack_bytes": len(pack),
                     "packed_over_full": round(len(pack) / frame_bytes, 4),
                     "n_solid": hdr["n_solid"], "n_raw": hdr["n_raw"], "n_skip": (size // 16) ** 2 - hdr["n_entries"],
                     "copy_us": copy_us[0], "copy_us_min_max": copy_us[1:], "copy_again_us": copy_us2[0],
                     "pack_us": pack_us[0], "pack_us_min_max": pack_us[1:], "unpack_us": unpack_us[0], "unpack_us_min_max": unpack_us[1:],
                     "pack_over_copy": round(pack_us[0] / copy_us[0], 3), "unpack_over_copy": round(unpack_us[0] / copy_us[0], 3),
                     "pack_algorithmic_bytes": n_pass1 * frame_bytes + raw_bytes + len(pack),
                     "pack_tb_per_s": round((n_pass1 * frame_bytes + raw_bytes + len(pack)) / (pack_us[0] * 1e-6) / 1e12, 3),
                     "copy_tb_per_s": round(2 * frame_bytes / (copy_us[0] * 1e-6) / 1e12, 3)}
                hp, hd = host_us(do_pack_and_read), host_us(do_download)
                r.update({"host_pack_and_read_us": hp[0], "host_pack_and_read_us_min_max": hp[1:], "host_download_us": hd[0],
                          "host_download_us_min_max": hd[1:], "download_over_pack_and_read": round(hd[0] / hp[0], 2)})
                results.append(r)
                print(json.dumps(r), flush=True)
                hip.jh_free(ctx, src_id)
                if ref_id is not None:
                    hip.jh_free(ctx, ref_id)
            hip.jh_free(ctx, pack_id)
            hip.jh_free(ctx, out_id)
    eng.sync()
    eng.set_stream(None)
    eng.close()
    out = {"tool": "tools/time_pack.py", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "per_block": a.per_block,
           "host_reps": a.host_reps,
           "note": "device times: hipEvents around blocks of back-to-back calls on one stream, median of the blocks, us per call; "
                   "copy = hipMemcpyDtoDAsync of frame_bytes in the same run (source, pack and destination of a 4096^2 RGBA8 "
                   "frame fit the 256 MiB Infinity Cache together, the 8-byte frames do not); host times: perf_counter around "
                   "pack + read_pack (two synchronising downloads into pageable memory) and around jh_download of the whole "
                   "frame (one), median of the repetitions",
           "results": results}
    write_json(a.out, out)


if __name__ == "__main__":
    main()
