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
import numpy as np

from timing import Timer

from jello_amd import ColorSpace, colorfilter as cf  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
MATRIX = (0.9, 0.1, -0.05, 0.0, 0.02, 0.05, 0.85, 0.1, 0.0, 0.0, -0.1, 0.2, 0.9, 0.0, 0.01, 0.0, 0.0, 0.0, 0.8, 0.1)
FILTERS = [("linear matrix (no tables)", dict(matrix=MATRIX, funcs=None, space=ColorSpace.LINEAR, clamp=True)),
           ("grayscale (SRGB: 3 PRE + 3 POST)", cf.grayscale(1.0)),
           ("brightness (SRGB, identity matrix)", cf.brightness(1.5)),
           ("four GAMMA funcs (LINEAR: 4 POST)", dict(matrix=None, funcs=(cf.gamma(1.0, 2.2, 0.0),) * 4, space=ColorSpace.LINEAR, clamp=True))]


def main():
    t = Timer("tools/time_color.py", 7, 10, "color_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # colours spread over [0, 1.25) and alphas over [0, 1], as a fine stage leaves them
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * np.array([1.25, 1.25, 1.25, 1.0], np.float32)).astype(np.float16).view(np.uint16)
    src, dst = 0x71C4_0000, 0x71C5_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)

    def traffic(bytes_):
        return lambda med: {"algorithmic_bytes": bytes_, "tb_per_s": round(bytes_ / (med * 1e-6) / 1e12, 3)}

    for label, rect, (x, y, w, h) in (("whole", None, (0, 0, SIZE, SIZE)), ("rect1024_odd", (1537, 1535, 1024, 1024), (1537, 1535, 1024, 1024))):
        texels = w * h
        floor = t.record({"rect": label, "call": "device-to-device copy"}, t.timed(t.copy((x, y, w, h))), more=traffic(16 * texels))
        comp = t.record({"rect": label, "call": "jh_composite", "mode": "Normal+SrcOver"},
                        t.timed(lambda: eng.composite(src, dst, src_rect=rect, offset=(x, y))), floor, traffic(24 * texels))
        for name, kw in FILTERS:
            launch = lambda: eng.color_filter(src, dst, rect=rect, **kw)  # noqa: E731
            launch()  # (the filter's tables become resident: the timed calls upload nothing)
            t.record({"rect": label, "call": "jh_color_filter", "filter": name}, t.timed(launch), floor, lambda med: dict(
                {"composite_us_median": round(comp, 3), "ratio_to_composite": round(med / comp, 2)}, **traffic(16 * texels)(med)))
    t.finish("hipEvents around back-to-back jh_color_filter calls (one kernel each, tables resident) from one 4096^2 image into another; "
             "the copy is torch's copy_ of the same rectangle between two tensors of the image's shape and jh_composite blends the same "
             "rectangle of the same two images, in the same run; algorithmic_bytes = 8 in, 8 out per texel (the tables, 1.25 MB at most, "
             "are not counted)", SIZE)


if __name__ == "__main__":
    main()
