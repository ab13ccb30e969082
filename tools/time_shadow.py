"""Device time of jh_shadow into a 4096^2 RGBA16F image under the identity: a box of half the image (2048 x 2048 about the
middle) with r = 0, 16 and 256 at sigma = 2, 8 and 32, as STORE and as OVER, over the whole image; the same for a 512 x 320 box over
jh_shadow_bounds' rectangle only; next to a device-to-device copy of the same rectangle, to jh_turbulence at 1 octave over the whole
image, and to the route this call replaces for a box: Engine.drop_shadow of a layer that holds the same box (blur, composite with a
tint, composite of the layer: three calls, two images more).  hipEvents (torch's, on the stream the context is switched to) around
blocks of back-to-back calls, median of the blocks.  Writes a JSON file (default profiles/shadow_kernel_times.json) with, per entry,
the ratio to the estimate DESIGN 5.18 wrote down before the first run (estimate() below) first.  Run on the GPU box.

    python tools/time_shadow.py [--blocks 5] [--per-block 5] [--out profiles/shadow_kernel_times.json]
"""
import numpy as np

from timing import Timer, median

from jello_amd import shadow_bounds, shadow_plan  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
BIG = (1024.0, 1024.0, 3072.0, 3072.0)
CARD = (1800.0, 1900.0, 2312.0, 2220.0)
COLOR = (0.0, 0.0, 0.0, 0.5)
# Written into DESIGN 5.18 before the first timing run, from instruction counts at the issue prices of a loaded SIMD (2 cycles a simple
# vector instruction, 8 a reciprocal; 1024 SIMDs at 2.4 GHz): G is 62 cycles (27 simple instructions, the division's ten among them, and
# one reciprocal); a texel's frame (two int64 positions, the products, the un-premultiplying store) 100, the blend of OVER 80 more; a
# texel outside every cap window 2.5 G under an axis-aligned matrix, one inside a window 3 N + 1 more per cap.  Bytes: 8 per texel
# stored, 8 more loaded under OVER, at the copy's 16.5 us per 4096^2 x 8 B.  The estimate is the larger of the two, not their sum.
G_CYCLES, FRAME_CYCLES, OVER_CYCLES, SIMD_HZ = 62.0, 100.0, 80.0, 1024 * 2.4e9
BYTES_US = 16.5


def estimate(box, radius, sigma, rect, over):
    x, y, w, h = rect
    pl = shadow_plan(box, radius, sigma)
    r, n, window = float(pl["radius"]), pl["n"], float(pl["window"])
    rows = np.arange(y, y + h) + 0.5 - 0.5 * (box[1] + box[3])
    caps = np.zeros(h)
    if r > 0:
        for sign in (1.0, -1.0):
            q = sign * rows - float(pl["straight"])
            caps += (np.minimum(q + window, r) > np.maximum(q - window, 0.0)) * (3 * n + 1)
    cycles = float(np.sum(2.5 * G_CYCLES + FRAME_CYCLES + (OVER_CYCLES if over else 0.0) + caps * G_CYCLES)) * w / 64.0
    return max(cycles / SIMD_HZ * 1e6, BYTES_US * (2 if over else 1) * w * h / float(SIZE * SIZE))


def main():
    t = Timer("tools/time_shadow.py", 5, 5, "shadow_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    dst, layer, scratch = 0x7E00_0000, 0x7E01_0000, 0x7E02_0000
    t.upload(img, dst, scratch)
    t.tensors(SIZE, SIZE)
    whole = (0, 0, SIZE, SIZE)
    floor = t.record({"rect": "whole", "call": "device-to-device copy", "algorithmic_bytes": 16 * SIZE * SIZE}, t.timed(t.copy(whole)))
    t.record({"rect": "whole", "call": "jh_turbulence", "octaves": 1}, t.timed(lambda: eng.turbulence(dst, 0.05, octaves=1, seed=1)), floor)
    t.upload(img, dst)
    for label, box in (("whole", BIG), ("bounds", CARD)):
        for radius in (0.0, 16.0, 256.0):
            for sigma in (2.0, 8.0, 32.0):
                rect = whole if label == "whole" else shadow_bounds(box, radius, sigma, (SIZE, SIZE))
                rect_floor = floor if label == "whole" else median(t.timed(t.copy(rect)))
                for over in (False, True):
                    launch = lambda: eng.shadow(dst, box, radius, sigma, COLOR, rect=rect, over=over)  # noqa: E731
                    times = t.timed(launch)
                    est = estimate(box, radius, sigma, rect, over)
                    t.record({"rect": label, "rect_texels": rect[2] * rect[3], "call": "jh_shadow", "box": list(box), "radius": radius, "sigma": sigma,
                              "mode": "OVER" if over else "STORE", "measured_over_estimate": round(median(times) / est, 2), "estimate_us": round(est, 1)}, times, rect_floor)
    # the route this replaces: a layer that holds the box, blurred, tinted and laid under the layer (sigma at most 64: jh_blur's limit)
    box_bits = np.zeros((SIZE, SIZE, 4), np.uint16)
    box_bits[1024:3072, 1024:3072] = np.array([0.9, 0.4, 0.1, 1.0], np.float16).view(np.uint16)
    t.upload(box_bits, layer)
    for sigma in (2.0, 8.0, 32.0):
        launch = lambda: eng.drop_shadow(layer, dst, SIZE, SIZE, sigma, (6, 8), COLOR, scratch)  # noqa: E731
        shadow_us = next(r["us_median"] for r in t.results if r.get("call") == "jh_shadow" and r["rect"] == "whole" and r["radius"] == 0.0 and
                         r["sigma"] == sigma and r["mode"] == "OVER")
        t.record({"rect": "whole", "call": "Engine.drop_shadow", "calls": 3, "sigma": sigma}, t.timed(launch), floor,
                 more=lambda med: {"over_jh_shadow_over_r0": round(med / shadow_us, 2)})
    t.finish("hipEvents around back-to-back jh_shadow calls (one kernel each) into a 4096^2 image under the identity; a 2048^2 box over the "
             "whole image and a 512 x 320 box over jh_shadow_bounds' rectangle; torch's copy_ of the same rectangle, jh_turbulence at 1 octave "
             "and Engine.drop_shadow (blur + two composites; it also draws the layer) of a layer holding the 2048^2 box are timed in the same "
             "run; estimate_us is what DESIGN 5.18 wrote down before the first timing run", SIZE)


if __name__ == "__main__":
    main()
