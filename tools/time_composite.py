"""Device time of jh_composite at 4096^2 RGBA16F: one image onto a second one, the whole image and a 1024^2 rectangle
placed at an odd offset (1537, 1535; once with the source's pairs 16-byte aligned, once 8-byte aligned only), for Normal + SrcOver, Normal + SrcOver with a
tint, Multiply and Hue -- next to a device-to-device copy of the same rectangle (torch's copy_ of the rectangle's view, on the same
stream: 8 B read + 8 B written per texel, where the composite reads 16 and writes 8) and next to jh_blit of the whole image (8 B
read, 4 B written), all from the same run.  hipEvents (torch's, on the stream the context is switched to) around blocks of
back-to-back launches, median of the blocks.  Writes a JSON file (default profiles/composite_kernel_times.json) with the times,
the ratio to the copy and the traffic rate.  Run on the GPU box.

    python tools/time_composite.py [--blocks 7] [--per-block 10] [--out profiles/composite_kernel_times.json]
"""
import numpy as np

from timing import Timer

from jello_amd import Compose, Mix, Surface  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
MODES = [("Normal+SrcOver", Mix.Normal, None), ("Normal+SrcOver, tint", Mix.Normal, (0.0, 0.0, 0.0, 0.5)), ("Multiply+SrcOver", Mix.Multiply, None),
         ("Hue+SrcOver", Mix.Hue, None)]


def main():
    t = Timer("tools/time_composite.py", 7, 10, "composite_kernel_times.json")
    eng = t.eng
    import torch
    rng = np.random.default_rng(1)
    # colours spread over [0, 1.25) and alphas over [0, 1], as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * np.array([1.25, 1.25, 1.25, 1.0], np.float32)).astype(np.float16).view(np.uint16)
    src, dst = 0x71C2_0000, 0x71C3_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)
    with torch.cuda.stream(t.stream):
        surface = torch.zeros(SIZE, SIZE, 4, dtype=torch.uint8, device="cuda")  # what the blit writes

    def traffic(bytes_):
        return lambda med: {"algorithmic_bytes": bytes_, "tb_per_s": round(bytes_ / (med * 1e-6) / 1e12, 3)}

    t.record({"rect": "whole", "call": "jh_blit RGBA8_UNORM"},
             t.timed(lambda: eng.blit(src, SIZE, SIZE, Surface.RGBA8_UNORM, out_device_ptr=surface.data_ptr())), more=traffic(12 * SIZE * SIZE))
    # dx is odd: dst's pairs start at the rectangle's second texel.  Read from sx = 1 the source's pairs are 16-byte aligned there
    # too (sx - dx even), read from sx = 2 they are not and load as two 8-byte halves.
    for label, src_rect, offset, rect in (("whole", None, (0, 0), (0, 0, SIZE, SIZE)),
                                          ("rect1024_odd", (1, 2, 1024, 1024), (1537, 1535), (1537, 1535, 1024, 1024)),
                                          ("rect1024_odd_src_unaligned", (2, 2, 1024, 1024), (1537, 1535), (1537, 1535, 1024, 1024))):
        texels = rect[2] * rect[3]
        floor = t.record({"rect": label, "call": "device-to-device copy"}, t.timed(t.copy(rect)), more=traffic(16 * texels))
        for name, mix, tint in MODES:
            launch = lambda: eng.composite(src, dst, mix, Compose.SrcOver, 1.0, tint, src_rect, offset)  # noqa: E731
            t.record({"rect": label, "call": "jh_composite", "mode": name}, t.timed(launch), floor, traffic(24 * texels))
    t.finish("hipEvents around back-to-back jh_composite calls (one kernel each) from one 4096^2 image onto another, which is blended "
             "over and over (the values drift towards the blend's fixed point; the bytes moved do not change); the copy is torch's copy_ "
             "of the same rectangle between two tensors of the image's shape in the same run; algorithmic_bytes = 8 source + 8 backdrop "
             "in, 8 out per texel", SIZE)


if __name__ == "__main__":
    main()
