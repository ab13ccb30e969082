"""Device time of jh_load_yuv and jh_load_surface into RGBA16F images of 4096^2 and 2048^2: the whole image and a
1024^2 rectangle at an odd offset.  jh_load_yuv: NV12 and I420, REPLICATE and BILINEAR, both transfers, BT.709 limited, from planes
with tightly packed rows at 16-byte aligned pointers; jh_load_surface: the six instantiations (UNORM / SRGB x STRAIGHT / PREMULTIPLIED /
OPAQUE) from an RGBA8 surface of random bytes.  Next to each, from the same run and with max - min over their blocks: a
device-to-device copy of the destination rectangle (8 B read + 8 B written per texel), jh_blit_yuv NV12 / NONE of an image of the
frame's size (the same 9.5 B per texel in the other direction) and jh_blit RGBA8_UNORM of it (the same 12 B per texel).  hipEvents
(torch's, on the stream the context is switched to) around blocks of back-to-back calls, median of the blocks; a call is one kernel.
Every descriptor is built once, outside the blocks, and a launch is one call of the C ABI, so that a block holds as little host work
as the ABI allows; the 1024^2 configurations, whose kernels take about 5 us, run RECT_CALLS times as many calls per block.  Even so
a kernel of that length is close to what a launch costs to submit: those figures are upper bounds of the device time, and their
ratios are not resolved by this method.  Every result carries the estimate of DESIGN 5.21, written before the first run -- the
yardstick of equal bytes, BILINEAR the same as REPLICATE -- and the ratio of the time to it.  Writes a JSON file (default
profiles/load_kernel_times.json).  Run on the GPU box.

    python tools/time_load.py [--blocks 5] [--per-block 5] [--out profiles/load_kernel_times.json]
"""
import ctypes

import numpy as np

from timing import Timer, timed

from jello_amd import ChromaFilter, LoadAlpha, Surface, YuvLayout, YuvMatrix, YuvRange, YuvTransfer  # noqa: E402 (timing puts the root on sys.path)
from jello_amd.engine import _load_surface_desc, _load_yuv_desc  # noqa: E402

SIZES = (4096, 2048)
RECT = 1024
RECT_CALLS = 8  # calls per block of a 1024^2 configuration, as a multiple of --per-block
SRC_SURFACE, SRC_YUV, OUT_SURFACE, OUT_YUV = 0x10AD_0001, 0x10AD_0002, 0x10AD_0003, 0x10AD_0004


def device_bytes(eng, buffer_id, host):
    eng._check(eng.hip.jh_upload(eng.ctx, buffer_id, host.ctypes.data, host.size), "upload")
    return eng.hip.jh_buffer_device_ptr(eng.ctx, buffer_id)


def planes(base, w, h, layout):
    """[(pointer, pitch)] of a tightly packed w x h frame at `base` (w even here: every plane starts at a multiple of 16)."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if layout == YuvLayout.NV12:
        return [(base, w), (base + w * h, 2 * cw)]
    return [(base, w), (base + w * h, cw), (base + w * h + cw * ch, cw)]


def checked(eng, what, call):
    """`call` -- one call of the C ABI returning its code -- made once and checked; then the launch a block repeats."""
    eng._check(call(), what)
    return call


def main():
    t = Timer("tools/time_load.py", 5, 5, "load_kernel_times.json")
    eng, hip = t.eng, t.eng.hip
    g = np.random.default_rng(1)
    big = max(SIZES)
    surface = device_bytes(eng, SRC_SURFACE, g.integers(0, 256, big * big * 4, np.uint8))
    yuv = device_bytes(eng, SRC_YUV, g.integers(0, 256, big * big * 3 // 2, np.uint8))
    out_surface = eng._own_buffer(OUT_SURFACE, big * big * 4)
    out_yuv = eng._own_buffer(OUT_YUV, big * big * 3 // 2)
    dst, frame_image = 0x10AE_0000, 0x10AF_0000
    for size in SIZES:
        t.tensors(size, size)
        t.upload(np.zeros((size, size, 4), np.uint16), dst)
        for label, rect in (("whole", (0, 0, size, size)), ("rect1024", (size // 4 + 7, size // 4 + 13, RECT, RECT))):
            w, h = rect[2], rect[3]
            per_block = t.args.per_block * (1 if label == "whole" else RECT_CALLS)
            run = lambda launch: timed(t.stream, launch, t.args.blocks, per_block)  # noqa: E731
            base = {"size": size, "rect": label, "calls_per_block": per_block}
            # the yardsticks of this configuration: the copy, and the two blits of an image of the frame's size
            t.upload(g.integers(0, 0x3C00, (h, w, 4)).astype(np.uint16), frame_image)
            copy_us = t.record(dict(base, call="device-to-device copy", algorithmic_bytes=16 * w * h), run(t.copy(None if label == "whole" else rect)))
            yd, _ = eng._yuv_desc(w, h, YuvLayout.NV12, YuvMatrix.BT709, YuvRange.LIMITED, YuvTransfer.NONE, planes(out_yuv, w, h, YuvLayout.NV12))
            blit_yuv_us = t.record(dict(base, call="jh_blit_yuv", layout="NV12", transfer="NONE", algorithmic_bytes=w * h * 19 // 2),
                                   run(checked(eng, "blit_yuv", lambda: hip.jh_blit_yuv(eng.ctx, frame_image, w, h, ctypes.byref(yd)))), copy_us)
            blit_us = t.record(dict(base, call="jh_blit", format="RGBA8_UNORM", algorithmic_bytes=12 * w * h),
                               run(checked(eng, "blit", lambda: hip.jh_blit(eng.ctx, frame_image, out_surface, 4 * w, w, h, int(Surface.RGBA8_UNORM)))), copy_us)
            ratio = lambda est: (lambda med: {"ratio_to_estimate": round(med / est, 2)})  # noqa: E731
            for layout in YuvLayout:
                for chroma in ChromaFilter:
                    for transfer in YuvTransfer:
                        d = _load_yuv_desc(layout, YuvMatrix.BT709, YuvRange.LIMITED, transfer, chroma, planes(yuv, w, h, layout), rect)
                        launch = checked(eng, "load_yuv", lambda d=d: hip.jh_load_yuv(eng.ctx, dst, ctypes.byref(d)))
                        t.record(dict(base, call="jh_load_yuv", layout=layout.name, chroma=chroma.name, transfer=transfer.name, algorithmic_bytes=w * h * 19 // 2,
                                      estimate="jh_blit_yuv of equal bytes", estimate_us=round(blit_yuv_us, 1)), run(launch), copy_us, more=ratio(blit_yuv_us))
            for fmt in (Surface.RGBA8_UNORM, Surface.RGBA8_SRGB):
                for alpha in LoadAlpha:
                    d = _load_surface_desc(fmt, alpha, surface, 4 * w, rect)
                    launch = checked(eng, "load_surface", lambda d=d: hip.jh_load_surface(eng.ctx, dst, ctypes.byref(d)))
                    t.record(dict(base, call="jh_load_surface", format=fmt.name, alpha=alpha.name, algorithmic_bytes=12 * w * h,
                                  estimate="jh_blit of equal bytes", estimate_us=round(blit_us, 1)), run(launch), copy_us, more=ratio(blit_us))
    for b in (SRC_SURFACE, SRC_YUV, OUT_SURFACE, OUT_YUV):
        hip.jh_free(eng.ctx, b)
    t.finish("hipEvents around back-to-back jh_load_yuv / jh_load_surface calls (one kernel each, descriptors built outside the blocks) into an "
             "RGBA16F image; the copy is torch's copy_ of the destination rectangle between two tensors of the image's shape; jh_blit_yuv (NV12, "
             "NONE) and jh_blit (RGBA8_UNORM) of an image of the frame's size are the yardsticks of equal bytes from the same run, their us_spread "
             "the max - min over the blocks; estimate_us = the yardstick of equal bytes, written into DESIGN 5.21 before the first run; the "
             "rect1024 kernels take about as long as a launch takes to submit: upper bounds, ratios not resolved", SIZES[0], sizes=list(SIZES))


if __name__ == "__main__":
    main()
