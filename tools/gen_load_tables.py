"""Writes jello_amd/csrc/load_decode_lut.h: the tables of jh_load_surface and jh_load_yuv (include/jello_load.h, DESIGN.md 5.21
"Load rule").

Decode tables, one entry per 8-bit code c:
    U(c) = the binary32 nearest to c / 255 (the IEEE quotient (float)c / 255.0f);  kLoadUnormF16[c] = f16(U(c))
    L(c) = kSrgbToLinear[c] of jello_amd/csrc/srgb_lut.h, read from that header;   kLoadSrgbF16[c] = f16(L(c)),
                                                                                  kLoadSrgbF32[c] = the bits of L(c)
f16() rounds to nearest even.  The host has no copy of kSrgbToLinear (it is a device constant), hence kLoadSrgbF32.

Y'CbCr -> R'G'B' coefficients, 16.16 fixed point, per matrix and range, from exact fractions: Kr, Kb (BT.601: 299/1000, 114/1000;
BT.709: 2126/10000, 722/10000), Kg = 1 - Kr - Kb, sy = 255/219 or 1, s = 255/224 or 1:
    Ky = sy    Krv = 2 (1 - Kr) s    Kgu = -2 Kb (1 - Kb) / Kg s    Kgv = -2 Kr (1 - Kr) / Kg s    Kbu = 2 (1 - Kb) s
each round-half-even(exact * 2^16), no adjustment: one Ky serves the three rows, so a grey gives R = G = B.

    python tools/gen_load_tables.py            # rewrite the header
    python tools/gen_load_tables.py --verify   # also check the tables against their definitions, and the committed header
"""
import argparse
import math
import os
import struct
import sys
from fractions import Fraction as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "jello_amd", "csrc", "load_decode_lut.h")
SRGB_HEADER = os.path.join(ROOT, "jello_amd", "csrc", "srgb_lut.h")
MATRICES = (("BT601", F(299, 1000), F(114, 1000)), ("BT709", F(2126, 10000), F(722, 10000)))
RANGES = (("LIMITED", F(255, 219), F(255, 224), 16), ("FULL", F(1), F(1), 0))
ONE = 1 << 16


def rne(q):
    """round-half-even of a Fraction."""
    return round(q)


def nearest(q, bits, emin):
    """The value of the binary format with a `bits`-bit significand and least normal exponent `emin` nearest to the Fraction q >= 0,
    ties to even, as a Fraction (no overflow for the arguments of this file)."""
    if q == 0:
        return F(0)
    e = max(math.floor(math.log2(q)), emin)
    while F(2) ** e > q and e > emin:
        e -= 1
    while F(2) ** (e + 1) <= q:
        e += 1
    ulp = F(2) ** (e - bits + 1)
    return rne(q / ulp) * ulp


def f32_bits(q):
    return struct.unpack("<I", struct.pack("<f", float(q)))[0]  # (q is a binary32 value: the conversions are exact)


def f16_bits(q):
    return struct.unpack("<H", struct.pack("<e", float(q)))[0]  # (q is a binary16 value)


def srgb_to_linear():
    """kSrgbToLinear of srgb_lut.h, as 256 Fractions."""
    text = open(SRGB_HEADER).read()
    body = text[text.index("{") + 1:text.index("}")]
    vals = [F(float.fromhex(t.strip().rstrip("f"))) for t in body.split(",") if t.strip()]
    assert len(vals) == 256
    return vals


def decode_tables():
    """(f16(U), f16(L), bits of L): three lists of 256 ints."""
    u = [nearest(F(c, 255), 24, -126) for c in range(256)]
    lin = srgb_to_linear()
    return ([f16_bits(nearest(v, 11, -14)) for v in u], [f16_bits(nearest(v, 11, -14)) for v in lin], [f32_bits(v) for v in lin])


def exact_coefficients(kr, kb, sy, s):
    kg = 1 - kr - kb
    return [sy, 2 * (1 - kr) * s, -2 * kb * (1 - kb) / kg * s, -2 * kr * (1 - kr) / kg * s, 2 * (1 - kb) * s]


def yuv_tables():
    """[(matrix name, range name, offset, [Ky, Krv, Kgu, Kgv, Kbu])], matrix major, range minor."""
    return [(mname, rname, off, [rne(c * ONE) for c in exact_coefficients(kr, kb, sy, s)])
            for mname, kr, kb in MATRICES for rname, sy, s, off in RANGES]


def _rows(vals, fmt, per_line):
    return ["    " + ", ".join(fmt % v for v in vals[i:i + per_line]) + "," for i in range(0, len(vals), per_line)]


def render():
    uf16, lf16, lf32 = decode_tables()
    t = yuv_tables()
    lines = [
        "// The tables of jh_load_surface and jh_load_yuv (include/jello_load.h, DESIGN.md 5.21).  For an 8-bit code c:",
        "//   kLoadUnormF16[c] = f16(U(c)), U(c) = the binary32 nearest to c / 255;  kLoadSrgbF16[c] = f16(L(c)) and kLoadSrgbF32[c] =",
        "//   the bits of L(c), L = kSrgbToLinear of srgb_lut.h (a device constant: this is the copy the host reads).",
        "// kLoadYuv[jh_yuv_matrix][jh_yuv_range] = {Ky, Krv, Kgu, Kgv, Kbu}: round-half-even(exact * 2^16) of 255/219 or 1, 2 (1 - Kr) s,",
        "// -2 Kb (1 - Kb) / Kg s, -2 Kr (1 - Kr) / Kg s, 2 (1 - Kb) s with s = 255/224 or 1.  kLoadYuvOffset[jh_yuv_range]: the luma offset.",
        "// JLOAD_TABLE is the including file's storage for them (jello_load.h: a constant of both sides under hipcc).",
        "// Generated -- do not edit:",
        "//     python tools/gen_load_tables.py",
        "#pragma once",
        "#include <stdint.h>",
        "#ifndef JLOAD_TABLE",
        "#define JLOAD_TABLE static const",
        "#endif",
        "JLOAD_TABLE uint16_t kLoadUnormF16[256] = {",
    ]
    lines += _rows(uf16, "0x%04x", 16) + ["};", "JLOAD_TABLE uint16_t kLoadSrgbF16[256] = {"]
    lines += _rows(lf16, "0x%04x", 16) + ["};", "JLOAD_TABLE uint32_t kLoadSrgbF32[256] = {"]
    lines += _rows(lf32, "0x%08xu", 8) + ["};", "JLOAD_TABLE int32_t kLoadYuv[2][2][5] = {"]
    for i in range(0, len(t), 2):
        lines.append("    {")
        for mname, rname, off, k in t[i:i + 2]:
            lines.append("        {" + ", ".join("%d" % c for c in k) + "},  // %s %s" % (mname, rname))
        lines.append("    },")
    lines.append("};")
    lines.append("JLOAD_TABLE int32_t kLoadYuvOffset[2] = {%s};" % ", ".join("%d" % off for _, _, off, _ in t[:2]))
    return "\n".join(lines) + "\n"


def parse(text):
    """The tables of a header written by render(): {name: flat list of ints}."""
    body = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    out = {}
    for chunk in body.split("JLOAD_TABLE")[3:]:  # ([1], [2]: the #ifndef's and the #define's)
        name = chunk.split("[")[0].split()[-1]
        vals = chunk[chunk.index("=") + 1:chunk.index(";")]
        out[name] = [int(s.rstrip("u"), 0) for s in vals.replace("{", " ").replace("}", " ").replace(",", " ").split()]
    return out


def verify(path):
    """The committed header is what render() writes; U is the nearest binary32 and the IEEE quotient; L is the formula in binary64
    rounded once; every f16 entry is within half an ulp; the coefficients are within 1/2 of exact * 2^16 and every grey gives R = G = B."""
    bad = 0
    if not os.path.exists(path) or open(path).read() != render():
        print("the header differs from the generator's output")
        bad += 1
    got = parse(render())
    for c in range(256):
        u = nearest(F(c, 255), 24, -126)
        if f32_bits(u) != struct.unpack("<I", struct.pack("<f", c / 255.0))[0]:  # (binary64 quotient rounded to binary32: checked against U)
            bad += 1
        lo, hi = F(struct.unpack("<f", struct.pack("<I", f32_bits(u) - 1 if c else 0))[0]), F(struct.unpack("<f", struct.pack("<I", f32_bits(u) + 1))[0])
        if not (abs(u - F(c, 255)) <= abs(lo - F(c, 255)) and abs(u - F(c, 255)) <= abs(hi - F(c, 255))):
            bad += 1
        x = c / 255.0
        want = x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4
        if struct.unpack("<I", struct.pack("<f", want))[0] != got["kLoadSrgbF32"][c]:
            bad += 1
        for name, v in (("kLoadUnormF16", u), ("kLoadSrgbF16", F(struct.unpack("<f", struct.pack("<I", got["kLoadSrgbF32"][c]))[0]))):
            h = F(struct.unpack("<e", struct.pack("<H", got[name][c]))[0])
            ulp = F(2) ** (max(math.floor(math.log2(v)) if v else -14, -14) - 10)
            if abs(h - v) > ulp / 2:
                bad += 1
    for (mname, kr, kb), (rname, sy, s, off) in ((m, r) for m in MATRICES for r in RANGES):
        k = next(x[3] for x in yuv_tables() if x[0] == mname and x[1] == rname)
        if any(abs(a - b * ONE) > F(1, 2) for a, b in zip(k, exact_coefficients(kr, kb, sy, s))):
            bad += 1
        print("%s %s: %s" % (mname, rname, k))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--verify", action="store_true", help="check the tables against their definitions and the header against the generator")
    ap.add_argument("--out", default=HEADER)
    a = ap.parse_args()
    if a.verify:
        bad = verify(a.out)
        print("failed checks:", bad)
        return 1 if bad else 0
    with open(a.out, "w") as f:
        f.write(render())
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
