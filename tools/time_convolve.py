"""Device time of jh_convolve between two 4096^2 RGBA16F images: orders 3 x 3, 5 x 5 (the compile-time instantiations),
7 x 7 and 15 x 15 (the general one), PREMULTIPLIED and STRAIGHT, edge ZERO and REPEAT; the whole image and a 1024^2 rectangle at an
odd offset -- next to a device-to-device copy of the same rectangle from the same run (torch's copy_ of the rectangle's view, on the
same stream), which is the byte floor (8 B read + 8 B written per texel), and next to jh_blur at sigma = 1 and jh_warp BICUBIC under
the identity at the same rectangle.  hipEvents (torch's, on the stream the context is switched to) around blocks of back-to-back
calls, median of the blocks; a convolution and a warp are one kernel, a blur two.  Writes a JSON file (default
profiles/convolve_kernel_times.json) with the times, the ratio to the copy and ns per tap and texel.  Run on the GPU box; for the
kernels' own times run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_convolve.py --blocks 2`.

    python tools/time_convolve.py [--blocks 5] [--per-block 5] [--out profiles/convolve_kernel_times.json]
"""
import numpy as np

from timing import Timer

from jello_amd import BlurEdge, ConvolveEdge, ConvolveMode, WarpEdge, WarpFilter  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
RECT = (1531, 1537, 1024, 1024)
ORDERS = (3, 5, 7, 15)


def main():
    t = Timer("tools/time_convolve.py", 5, 5, "convolve_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # colours and alphas spread over [0, 1.25), as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    src, dst = 0x71E0_0000, 0x71E2_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", RECT)):
        x, y, w, h = rect
        call_rect = None if label == "whole" else rect
        floor = t.record({"rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * w * h}, t.timed(t.copy(rect)))
        t.record({"rect": label, "call": "jh_blur", "sigma": 1.0, "taps": "7 + 7"},
                 t.timed(lambda: eng.blur(dst, SIZE, SIZE, 1.0, edge=BlurEdge.ZERO, rect=call_rect)), floor)
        t.record({"rect": label, "call": "jh_warp", "case": "identity", "filter": "BICUBIC", "taps": 16},
                 t.timed(lambda: eng.warp(src, dst, (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), filter=WarpFilter.BICUBIC, edge=WarpEdge.ZERO, dst_rect=call_rect)), floor)
        for order in ORDERS:
            weights = (rng.random((order, order), dtype=np.float32) - 0.4) / np.float32(order * order)
            for mode in (ConvolveMode.PREMULTIPLIED, ConvolveMode.STRAIGHT):
                for edge in (ConvolveEdge.ZERO, ConvolveEdge.REPEAT):
                    launch = lambda: eng.convolve(src, dst, weights, edge=edge, mode=mode, rect=call_rect)  # noqa: E731
                    r = {"rect": label, "call": "jh_convolve", "order": order, "taps": order * order, "mode": mode.name, "edge": edge.name,
                         "instantiation": "%dx%d" % (order, order) if order in (3, 5) else "general"}
                    t.record(r, t.timed(launch), floor, lambda med: {"ps_per_tap_and_texel": round(med * 1e6 / (order * order * w * h), 3)})
    t.finish("hipEvents around back-to-back jh_convolve calls (one kernel each) between two 4096^2 images; the copy is torch's copy_ of "
             "the same rectangle between two tensors of the image's shape; jh_blur at sigma 1 (two kernels, in place on the destination) "
             "and jh_warp BICUBIC under the identity (one kernel) at the same rectangle are timed in the same run", SIZE)


if __name__ == "__main__":
    main()
