"""Device time of jh_morphology on a 4096^2 RGBA16F image: the whole image and a 1024^2 rectangle at an odd offset, both
ops, premultiplied and straight, radius 1, 4, 16, 64 and 255 on both axes, on x only and on y only, edge ZERO, from one image into a
second one -- next to a device-to-device copy of the same rectangle from the same run (torch's copy_ of the rectangle's view, on the
same stream), which is the byte floor (8 B read + 8 B written per texel), and next to jh_blur at sigma = r / 3 (so R = r) for the
radii the blur allows.  hipEvents (torch's, on the stream the context is switched to) around blocks of back-to-back calls, median
of the blocks; a call is three kernels.  Writes a JSON file (default profiles/morph_kernel_times.json) with the times, the ratio to
the copy, and the ratio of the r = 255 time to the r = 4 time of every (rectangle, op, operands) -- the evidence that the work per
output does not grow with the window.  Run on the GPU box; for the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_morph.py --blocks 2`.

    python tools/time_morph.py [--blocks 5] [--per-block 5] [--out profiles/morph_kernel_times.json]
"""
import json

import numpy as np

from timing import Timer

from jello_amd import BlurEdge, MorphEdge, MorphOp  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
RADII = (1, 4, 16, 64, 255)
BLUR_MAX_RADIUS = 192


def main():
    t = Timer("tools/time_morph.py", 5, 5, "morph_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # colours and alphas spread over [0, 1.25), as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    src, dst = 0x71D0_0000, 0x71D1_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)
    ratios = []
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", (1531, 1537, 1024, 1024))):
        texels = rect[2] * rect[3]
        call_rect = None if label == "whole" else rect
        floor = t.record({"rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * texels}, t.timed(t.copy(rect)))
        for r in RADII:
            if r > BLUR_MAX_RADIUS:
                continue
            sigma = r / 3.0
            launch = lambda: eng.blur(src, SIZE, SIZE, sigma, dst_image_id=dst, edge=BlurEdge.ZERO, rect=call_rect)  # noqa: E731
            t.record({"rect": label, "call": "jh_blur", "sigma": round(sigma, 4), "radius": r}, t.timed(launch), floor)
        for op in MorphOp:
            for premultiplied in (True, False):
                both = {}
                for r in RADII:
                    for axes, radius in (("both", (r, r)), ("x", (r, 0)), ("y", (0, r))):
                        launch = lambda: eng.morphology(src, dst, op=op, radius=radius, edge=MorphEdge.ZERO, rect=call_rect,  # noqa: E731
                                                        premultiplied=premultiplied)
                        # f16 in, plane H out; H in, plane P out; H and P in, f16 out (the rows above and below a rectangle, and
                        # the padding rows of P, not counted)
                        med = t.record({"rect": label, "call": "jh_morphology", "op": op.name, "operands": "premultiplied" if premultiplied else "straight",
                                        "radius": r, "axes": axes, "traffic_bytes": (8 + 16 + 16 + 16 + 32 + 8) * texels}, t.timed(launch), floor)
                        if axes == "both":
                            both[r] = med
                ratio = {"rect": label, "op": op.name, "operands": "premultiplied" if premultiplied else "straight",
                         "r255_over_r4": round(both[255] / both[4], 2), "r255_us": round(both[255], 3), "r4_us": round(both[4], 3)}
                ratios.append(ratio)
                print(json.dumps(ratio), flush=True)
    t.finish("hipEvents around back-to-back jh_morphology calls (three kernels each) from one 4096^2 image into another, edge ZERO; the "
             "copy is torch's copy_ of the same rectangle between two tensors of the image's shape, and jh_blur (two kernels, "
             "sigma = r / 3) is timed in the same run; traffic_bytes = f16 in, keys out; keys in, prefix out; keys and prefix in, f16 out",
             SIZE, r255_over_r4=ratios)


if __name__ == "__main__":
    main()
