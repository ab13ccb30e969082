"""Device time of jh_displace into a 4096^2 RGBA16F image under the identity, from a 4096^2 source: NEAREST, BILINEAR and
BICUBIC, premultiplied, edge ZERO; the whole image and a 1024^2 destination rectangle at an odd offset; with three maps -- "half": 0.5
in every channel (jh_warp's identity plus the map's load), "noise": jh_turbulence fractal noise at 0.02 cells per texel, 2 octaves,
under scale 20 (the usual smooth map), "random": uniform values under scale 256 (scattered taps, the worst case) -- next to jh_warp under
the identity with the same filter and next to a device-to-device copy of the same rectangle, both from the same run (torch's copy_ of
the rectangle's view, on the same stream: 8 B read + 8 B written per texel).  hipEvents (torch's, on the stream the context is
switched to) around blocks of back-to-back calls, median of the blocks; each call is one kernel.  Writes a JSON file (default
profiles/displace_kernel_times.json) with, per entry, the ratio to the estimate DESIGN 5.17 wrote down before the first run (estimate()
below: the same run's jh_warp time plus the model's addition) first, then the times and the ratio to the copy.  Run on the GPU box.

    python tools/time_displace.py [--blocks 5] [--per-block 5] [--out profiles/displace_kernel_times.json]
"""
import numpy as np

from timing import Timer, median

from jello_amd import TurbulenceKind, WarpEdge, WarpFilter  # noqa: E402 (timing puts the root on sys.path)

SIZE = 4096
RECT = (1531, 1537, 1024, 1024)
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
TAPS = (1, 2, 4)  # per axis
MAPS = (("half", 20.0), ("noise", 20.0), ("random", 256.0))
# us per 4096^2 texels, written into DESIGN 5.17 before the first timing run: the map's 8 B per texel at the copy's rate, the offset's
# arithmetic at the vector rate, a smooth map's wider footprint, and for scattered taps the larger of the 128-byte lines they move
# through L2 (N per texel) and the line addresses the texture path takes (N^2 loads of 64 lines per wave)
MAP_BYTES_US, OFFSET_US, SMOOTH_FACTOR = 16.5, 5.3, 1.2
LINES_US, ADDRESS_US = 62.0, 27.0


def estimate(map_name, filt, warp_us, texels):
    share = texels / float(SIZE * SIZE)
    half = warp_us + (MAP_BYTES_US + OFFSET_US) * share
    if map_name == "half":
        return half
    if map_name == "noise":
        return half * SMOOTH_FACTOR
    n = TAPS[int(filt)]
    return half + max(n * LINES_US, n * n * ADDRESS_US) * share


def main():
    t = Timer("tools/time_displace.py", 5, 5, "displace_kernel_times.json")
    eng = t.eng
    rng = np.random.default_rng(1)
    # colours and alphas spread over [0, 1.25), as a fine stage leaves them; the random map uniform in [0, 1)
    img = (rng.random((SIZE, SIZE, 4), dtype=np.float32) * 1.25).astype(np.float16).view(np.uint16)
    src, dst, half, noise, scattered = 0x7D00_0000, 0x7D01_0000, 0x7D02_0000, 0x7D03_0000, 0x7D04_0000
    t.upload(img, src, dst)
    t.upload(np.full((SIZE, SIZE, 4), 0x3800, np.uint16), half)
    t.upload(rng.random((SIZE, SIZE, 4), dtype=np.float32).astype(np.float16).view(np.uint16), scattered)
    t.upload(img, noise)
    eng.turbulence(noise, base_frequency=0.02, octaves=2, seed=1, kind=TurbulenceKind.FRACTAL_NOISE)
    maps = {"half": half, "noise": noise, "random": scattered}
    t.tensors(SIZE, SIZE)
    for label, rect in (("whole", (0, 0, SIZE, SIZE)), ("rect1024", RECT)):
        x, y, w, h = rect
        call_rect = None if label == "whole" else rect
        floor = t.record({"rect": label, "call": "device-to-device copy", "algorithmic_bytes": 16 * w * h}, t.timed(t.copy(rect)))
        for filt in WarpFilter:
            launch = lambda: eng.warp(src, dst, IDENTITY, filter=filt, edge=WarpEdge.ZERO, dst_rect=call_rect)  # noqa: E731
            warp_us = t.record({"rect": label, "call": "jh_warp", "case": "identity", "filter": filt.name, "taps": TAPS[int(filt)] ** 2}, t.timed(launch), floor)
            for name, scale in MAPS:
                launch = lambda: eng.displace(src, maps[name], dst, scale, filter=filt, edge=WarpEdge.ZERO, dst_rect=call_rect)  # noqa: E731
                times = t.timed(launch)
                est = estimate(name, filt, warp_us, w * h)
                r = {"rect": label, "call": "jh_displace", "map": name, "scale": scale, "filter": filt.name, "taps": TAPS[int(filt)] ** 2,
                     "measured_over_estimate": round(median(times) / est, 2), "estimate_us": round(est, 1),
                     "over_warp": round(median(times) / warp_us, 2)}
                t.record(r, times, floor)
    t.finish("hipEvents around back-to-back jh_displace calls (one kernel each) into a 4096^2 image under the identity, premultiplied, edge "
             "ZERO; maps: 0.5 everywhere, jh_turbulence fractal noise (0.02 cells per texel, 2 octaves) under scale 20, uniform random under "
             "scale 256; jh_warp under the identity with the same filter and torch's copy_ of the same rectangle are timed in the same run; "
             "estimate_us is that jh_warp time plus what DESIGN 5.17 wrote down before the first timing run", SIZE)


if __name__ == "__main__":
    main()
