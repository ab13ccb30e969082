"""Device time of jh_lighting between two 4096^2 RGBA16F images: DIFFUSE and SPECULAR x DISTANT, POINT and SPOT, the
exponents in use 1 (no table) and 20 (the specular exponent's table, the spot exponent's, or both) -- every one of the kernel's 12
instantiations; the whole image and a 1024^2 rectangle at an odd offset -- next to a device-to-device copy of the same rectangle from
the same run (torch's copy_ of the rectangle's view, on the same stream), which is the byte floor (8 B read + 8 B written per texel),
and next to jh_color_filter without tables (a matrix alone) and jh_convolve 3 x 3 at the same rectangle.  hipEvents (torch's, on the
stream the context is switched to) around blocks of back-to-back calls, median of the blocks; each call is one kernel.  Writes a JSON
file (default profiles/lighting_kernel_times.json) with the times, the ratio to the copy and the ratio to the estimate DESIGN 5.14
wrote down before the first run (ESTIMATE_US below, whole image).  Run on the GPU box.

    python tools/time_lighting.py [--blocks 5] [--per-block 5] [--out profiles/lighting_kernel_times.json]
"""
import numpy as np

from timing import Timer

from jello_amd import colorfilter, convolution, lighting  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
RECT = (1531, 1537, 1024, 1024)
# us at 4096^2, by instantiation kind/light/tables: written into DESIGN 5.14 before the first timing run
ESTIMATE_US = {"diffuse/distant/0": 53, "diffuse/point/0": 76, "diffuse/spot/0": 81, "diffuse/spot/2": 90, "specular/distant/0": 62, "specular/distant/1": 70,
               "specular/point/0": 91, "specular/point/1": 100, "specular/spot/0": 96, "specular/spot/1": 105, "specular/spot/2": 105, "specular/spot/3": 112}


def configurations():
    lights = {"distant": lighting.distant(35, 40), "point": lighting.point(0.4 * SIZE, 0.6 * SIZE, 300.0)}
    for kind in ("diffuse", "specular"):
        for name in ("distant", "point", "spot"):
            for e in ((1.0,) if kind == "diffuse" else (1.0, 20.0)):
                for es in ((1.0, 20.0) if name == "spot" else (1.0,)):
                    lt = lighting.spot(0.4 * SIZE, 0.6 * SIZE, 300.0, (0.5 * SIZE, 0.5 * SIZE, 0.0), es, 60) if name == "spot" else lights[name]
                    flt = lighting.diffuse(5.0, 1.0) if kind == "diffuse" else lighting.specular(5.0, 1.0, e)
                    tables = (1 if kind == "specular" and e != 1.0 else 0) | (2 if es != 1.0 else 0)
                    yield "%s/%s/%d" % (kind, name, tables), dict(flt, **lt)


def main():
    t = Timer("tools/time_lighting.py", 5, 5, "lighting_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # a height map with structure at every scale: random alpha in [0, 1), random colour
    img = rng.random((SIZE, SIZE, 4), dtype=np.float32).astype(np.float16).view(np.uint16)
    src, dst = 0x71E0_0000, 0x71E2_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)
    box = convolution.box(3)
    sepia = dict(matrix=colorfilter.sepia(1.0)["matrix"])  # (the matrix alone, in LINEAR space: no tables)
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", RECT)):
        x, y, w, h = rect
        call_rect = None if label == "whole" else rect
        floor = t.record({"rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * w * h}, t.timed(t.copy(rect)))
        t.record({"rect": label, "call": "jh_color_filter", "case": "sepia's matrix in LINEAR space: no tables"},
                 t.timed(lambda: eng.color_filter(src, dst, rect=call_rect, **sepia)), floor)
        t.record({"rect": label, "call": "jh_convolve", "order": 3, "mode": "PREMULTIPLIED", "edge": "CLAMP"},
                 t.timed(lambda: eng.convolve(src, dst, rect=call_rect, **box)), floor)
        for inst, kw in configurations():
            eng.lighting(src, dst, rect=call_rect, **kw)  # (uploads the key's tables outside the timed blocks)
            r = {"rect": label, "call": "jh_lighting", "instantiation": inst, "specular_exponent": kw.get("specular_exponent", 1.0), "spot_exponent": kw.get("spot_exponent", 1.0)}
            t.record(r, t.timed(lambda: eng.lighting(src, dst, rect=call_rect, **kw)), floor, lambda med: {} if label != "whole" else {
                "estimate_us": ESTIMATE_US[inst], "measured_over_estimate": round(med / ESTIMATE_US[inst], 2)})
    t.finish("hipEvents around back-to-back jh_lighting calls (one kernel each) between two 4096^2 images of random alpha; the copy is torch's "
             "copy_ of the same rectangle between two tensors of the image's shape; jh_color_filter (a matrix, no tables) and jh_convolve 3 x 3 "
             "at the same rectangle are timed in the same run; estimate_us is what DESIGN 5.14 wrote down before the first timing run", SIZE)


if __name__ == "__main__":
    main()
