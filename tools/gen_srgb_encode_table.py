"""Writes jello_amd/csrc/srgb_encode_lut.h: the 255 f32 thresholds of the linear -> sRGB 8-bit encoding that jh_blit's
sRGB surface formats use ("Surface blit").

The rule (evaluated on a clamped f32 value v in [0, 1]):
    enc(v) = 12.92 v                      for v <= 0.0031308
           = 1.055 v^(1/2.4) - 0.055      otherwise
    code(v) = rint(255 * enc(v))          (binary64 throughout, ties to even)
t[k] (k = 1..255) is the smallest f32 v with code(v) >= k, found by bisection on the f32 bit patterns; the kernel's code
for v is then #{k : t[k] <= v}.

    python tools/gen_srgb_encode_table.py            # rewrite the header
    python tools/gen_srgb_encode_table.py --verify   # also check the table against code() on every f32 in [0, 1] (~1 min)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "jello_amd", "csrc", "srgb_encode_lut.h")
ONE_BITS = 0x3F800000


def code(v):
    """The binary64 rule on an array of f32 values in [0, 1] -> int64 codes 0..255."""
    d = np.asarray(v, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d <= 0.0031308, 12.92 * d, 1.055 * np.power(d, 1.0 / 2.4) - 0.055)
    return np.rint(255.0 * e).astype(np.int64)


def thresholds():
    """t[k - 1] for k = 1..255: the smallest f32 in [0, 1] whose code is >= k (np.float32 array of 255)."""
    out = np.empty(255, dtype=np.float32)
    for k in range(1, 256):
        lo, hi = 0, ONE_BITS  # code(f32(lo)) < k <= code(f32(hi))
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if code(np.array([mid], np.uint32).view(np.float32))[0] >= k:
                hi = mid
            else:
                lo = mid
        out[k - 1] = np.array([hi], np.uint32).view(np.float32)[0]
    return out


def render(t):
    lines = [
        "// Linear -> sRGB 8-bit encoding thresholds for jh_blit's *_SRGB surface formats (include/jello_hip.h, DESIGN.md).",
        "// Rule, on the clamped premultiplied f32 value v: enc(v) = 12.92 v for v <= 0.0031308, 1.055 v^(1/2.4) - 0.055",
        "// otherwise; code = rint(255 enc(v)), all in binary64, ties to even.  kSrgbEncodeThreshold[k - 1] is the smallest f32",
        "// whose code is >= k (k = 1..255), so code(v) = #{k : threshold[k - 1] <= v}.  Generated -- do not edit:",
        "//     python tools/gen_srgb_encode_table.py",
        "// JSRGB_ENCODE_TABLE is the including file's storage for the table: a device constant unless it says otherwise (the host",
        "// half of the stats rule, include/jello_queries.h and tools/stats_check.cpp, reads the same numbers as a host constant).",
        "#pragma once",
        "#ifndef JSRGB_ENCODE_TABLE",
        "#define JSRGB_ENCODE_TABLE static __device__ __constant__ const",
        "#endif",
        "JSRGB_ENCODE_TABLE float kSrgbEncodeThreshold[255] = {",
    ]
    vals = [float(x).hex() + "f" for x in t]
    for i in range(0, len(vals), 4):
        lines.append("    " + ", ".join(vals[i:i + 4]) + ",")
    lines.append("};")
    return "\n".join(lines) + "\n"


def parse(text):
    """The values of a header written by render() (np.float32 array)."""
    body = text[text.index("= {") + 3:text.rindex("}")]
    return np.array([float.fromhex(s.strip().rstrip("f")) for s in body.split(",") if s.strip()], dtype=np.float32)


def verify(t, chunk=1 << 24):
    """Every f32 bit pattern in [0, 1]: the table lookup equals code().  Returns the number of mismatches."""
    bad = 0
    for b0 in range(0, ONE_BITS + 1, chunk):
        v = np.arange(b0, min(b0 + chunk, ONE_BITS + 1), dtype=np.uint32).view(np.float32)
        bad += int(np.count_nonzero(np.searchsorted(t, v, side="right") != code(v)))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--verify", action="store_true", help="check every f32 in [0, 1] against the binary64 rule")
    ap.add_argument("--out", default=HEADER)
    a = ap.parse_args()
    t = thresholds()
    with open(a.out, "w") as f:
        f.write(render(t))
    print("wrote", a.out)
    if a.verify:
        bad = verify(t)
        print("f32 values in [0, 1] whose table lookup differs from the rule:", bad)
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
