"""Device time of jh_resample between RGBA16F images: 4096^2 -> 2048^2, 4096^2 -> 1920 x 1080 and 2048^2 -> 4096^2, every
filter, premultiplied (the default) -- next to a device-to-device copy of the destination's bytes from the same run (torch's copy_
between two tensors of the destination's shape, on the same stream), which is the floor of the write side alone: 8 B read + 8 B
written per destination texel.  hipEvents (torch's, on the stream the context is switched to) around blocks of back-to-back
launches, median of the blocks; the tap tables of a geometry are uploaded by the first warm-up call and resident afterwards.
Algorithmic work: 4 fused multiply-adds per tap, (source rows x destination width) windows of the x axis and (destination texels)
windows of the y axis.  Writes a JSON file (default profiles/resample_kernel_times.json) with the times, the ratio to the copy, the
fmaf rate and the traffic rate.  Run on the GPU box; for the two kernels' own times run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_resample.py --blocks 2`.

    python tools/time_resample.py [--blocks 7] [--per-block 10] [--out profiles/resample_kernel_times.json]
"""
import numpy as np

from timing import Timer

from jello_amd import ResampleFilter, resample_taps  # noqa: E402 (timing puts the root on sys.path)

GEOMETRIES = [((4096, 4096), (2048, 2048)), ((4096, 4096), (1920, 1080)), ((2048, 2048), (4096, 4096))]


def main():
    t = Timer("tools/time_resample.py", 7, 10, "resample_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    src, dst = 0x71C2_0000, 0x71C3_0000
    for (sw, sh), (dw, dh) in GEOMETRIES:
        # colours and alphas spread over [0, 1.25), as a fine stage leaves them
        t.upload((rng.random((sh, sw, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16), src)
        t.upload(np.zeros((dh, dw, 4), np.uint16), dst)
        t.tensors(dw, dh)
        label = "%dx%d->%dx%d" % (sw, sh, dw, dh)
        floor = t.record({"geometry": label, "call": "device-to-device copy of dst"}, t.timed(t.copy()), more=lambda med: {
            "algorithmic_bytes": 16 * dw * dh, "tb_per_s": round(16 * dw * dh / (med * 1e-6) / 1e12, 3)})
        for filt in ResampleFilter:
            wins_y = resample_taps(filt, sh, dh)
            taps_x = sum(len(w) for _, w in resample_taps(filt, sw, dw))
            taps_y = sum(len(w) for _, w in wins_y)
            # the column pass loads a row of the intermediate once per item of four output rows whose windows hold it
            rows_in = sum(max(f + len(w) for f, w in wins_y[g:g + 4]) - min(f for f, _ in wins_y[g:g + 4]) for g in range(0, dh, 4))
            fmas = 4 * (taps_x * sh + taps_y * dw)
            traffic = 8 * sw * sh + 16 * dw * sh + 16 * dw * rows_in + 8 * dw * dh  # f16 in, binary32 rows out, rows in per item, f16 out
            t.record({"geometry": label, "call": "jh_resample", "filter": filt.name, "taps_per_output_x": round(taps_x / dw, 2),
                      "taps_per_output_y": round(taps_y / dh, 2)}, t.timed(lambda: eng.resample(src, dst, filt)), floor, lambda med: {
                "fmaf": fmas, "tfmaf_per_s": round(fmas / (med * 1e-6) / 1e12, 2), "traffic_bytes": traffic,
                "traffic_tb_per_s": round(traffic / (med * 1e-6) / 1e12, 3)})
    t.finish("hipEvents around back-to-back jh_resample calls (two kernels each, tables resident) from one image into another; the copy is "
             "torch's copy_ between two tensors of the destination's shape in the same run; traffic_bytes = f16 source in, binary32 "
             "intermediate out, the intermediate in once per column item of four output rows (what the column pass asks of the caches), f16 out")


if __name__ == "__main__":
    main()
