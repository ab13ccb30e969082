"""Device time of jh_turbulence into a 4096^2 RGBA16F image: FRACTAL_NOISE and TURBULENCE, stitch off and on, 1, 4 and 8
octaves -- every one of the kernel's 4 instantiations; the whole image and a 1024^2 rectangle at an odd offset -- at a base frequency of
0.02 cells per texel (cells of 50 texels: the lanes of a wave share a cell in the first octaves and scatter over the lattice in the
last ones), next to a device-to-device copy of the same rectangle from the same run (torch's copy_ of the rectangle's view, on the same
stream; the kernel itself only writes, 8 B per texel) and next to jh_lighting DIFFUSE DISTANT at the same rectangle.  hipEvents
(torch's, on the stream the context is switched to) around blocks of back-to-back calls, median of the blocks; each call is one kernel.
Writes a JSON file (default profiles/turbulence_kernel_times.json) with, per entry, the ratio to the estimate DESIGN 5.15 wrote down
before the first run (ESTIMATE_US below, whole image) first, then the times and the ratio to the copy.  Run on the GPU box.

    python tools/time_turbulence.py [--blocks 5] [--per-block 5] [--out profiles/turbulence_kernel_times.json]
"""
import numpy as np

from timing import Timer, median

from jello_amd import TurbulenceKind, lighting  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
RECT = (1531, 1537, 1024, 1024)
FREQUENCY = 0.02
TILE = (0.0, 0.0, 1024.0, 1024.0)
# us at 4096^2, by instantiation kind/stitch and octaves: written into DESIGN 5.15 before the first timing run
ESTIMATE_US = {("fractal/0", 1): 40, ("fractal/1", 1): 43, ("turbulence/0", 1): 41, ("turbulence/1", 1): 44,
               ("fractal/0", 4): 119, ("fractal/1", 4): 131, ("turbulence/0", 4): 123, ("turbulence/1", 4): 135,
               ("fractal/0", 8): 325, ("fractal/1", 8): 338, ("turbulence/0", 8): 329, ("turbulence/1", 8): 341}


def configurations():
    for kind in (TurbulenceKind.FRACTAL_NOISE, TurbulenceKind.TURBULENCE):
        for stitch in (0, 1):
            for octaves in (1, 4, 8):
                yield "%s/%d" % (("fractal", "turbulence")[int(kind)], stitch), octaves, dict(
                    base_frequency=FREQUENCY, octaves=octaves, seed=1, kind=kind, stitch_tile=TILE if stitch else None)


def main():
    t = Timer("tools/time_turbulence.py", 5, 5, "turbulence_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    img = rng.random((SIZE, SIZE, 4), dtype=np.float32).astype(np.float16).view(np.uint16)
    src, dst = 0x7B00_0000, 0x7B02_0000
    t.upload(img, src, dst)
    t.tensors(SIZE, SIZE)
    diffuse = dict(lighting.diffuse(5.0, 1.0), **lighting.distant(35, 40))
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", RECT)):
        x, y, w, h = rect
        call_rect = None if label == "whole" else rect
        floor = t.record({"rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * w * h}, t.timed(t.copy(rect)))
        t.record({"rect": label, "call": "jh_lighting", "instantiation": "diffuse/distant/0"},
                 t.timed(lambda: eng.lighting(src, dst, rect=call_rect, **diffuse)), floor)
        for inst, octaves, kw in configurations():
            eng.turbulence(dst, rect=call_rect, **kw)  # (uploads the seed's tables outside the timed blocks)
            times = t.timed(lambda: eng.turbulence(dst, rect=call_rect, **kw))
            r = {"rect": label, "call": "jh_turbulence", "instantiation": inst, "octaves": octaves, "base_frequency": FREQUENCY}
            if label == "whole":  # (in front of the times, where the committed profile has them: not record()'s more=, which comes behind)
                est = ESTIMATE_US[(inst, octaves)]
                r.update({"measured_over_estimate": round(median(times) / est, 2), "estimate_us": est})
            t.record(r, times, floor)
    t.finish("hipEvents around back-to-back jh_turbulence calls (one kernel each) into a 4096^2 image at 0.02 cells per texel; the copy is "
             "torch's copy_ of the same rectangle between two tensors of the image's shape; jh_lighting DIFFUSE DISTANT at the same rectangle "
             "is timed in the same run; estimate_us is what DESIGN 5.15 wrote down before the first timing run", SIZE)


if __name__ == "__main__":
    main()
