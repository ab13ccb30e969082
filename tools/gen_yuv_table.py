"""Writes jello_amd/csrc/yuv_matrix_lut.h: the 16.16 fixed-point R'G'B' -> Y'CbCr coefficient tables of jh_blit_yuv
(include/jello_hip.h, DESIGN.md 5.5 "YUV blit").

For Kr, Kb (BT.601: 299/1000, 114/1000; BT.709: 2126/10000, 722/10000), Kg = 1 - Kr - Kb, a luma scale sy (219/255 limited,
1 full) and a chroma scale sc (224/255 limited, 1 full), as exact fractions:
    Y  row = sy * (Kr, Kg, Kb)
    Cb row = sc * (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb))
    Cr row = sc * (1 - Kr, -Kg, -Kb) / (2 (1 - Kr))
Every coefficient is round-half-even(exact * 2^16); the green coefficient of a row is then adjusted so that the Y row sums to
round-half-even(sy * 2^16) and each chroma row to 0 (a grey has Cb = Cr = 128 exactly).

    python tools/gen_yuv_table.py            # rewrite the header
    python tools/gen_yuv_table.py --verify   # also check row sums, the grey property and the distance to the exact formula
"""
import argparse
import os
import sys
from fractions import Fraction as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "jello_amd", "csrc", "yuv_matrix_lut.h")
MATRICES = (("BT601", F(299, 1000), F(114, 1000)), ("BT709", F(2126, 10000), F(722, 10000)))
RANGES = (("LIMITED", F(219, 255), F(224, 255), 16), ("FULL", F(1), F(1), 0))
ONE = 1 << 16


def rne(q):
    """round-half-even of a Fraction."""
    return round(q)  # (Fraction.__round__ rounds ties to even)


def exact_rows(kr, kb, sy, sc):
    kg = 1 - kr - kb
    return ([sy * kr, sy * kg, sy * kb],
            [sc * -kr / (2 * (1 - kb)), sc * -kg / (2 * (1 - kb)), sc * F(1, 2)],
            [sc * F(1, 2), sc * -kg / (2 * (1 - kr)), sc * -kb / (2 * (1 - kr))])


def tables():
    """[(matrix name, range name, offset, [Y row, Cb row, Cr row])] in the order of the header: matrix major, range minor."""
    out = []
    for mname, kr, kb in MATRICES:
        for rname, sy, sc, off in RANGES:
            rows = [[rne(c * ONE) for c in row] for row in exact_rows(kr, kb, sy, sc)]
            for row, want in zip(rows, (rne(sy * ONE), 0, 0)):
                row[1] += want - sum(row)
            out.append((mname, rname, off, rows))
    return out


def render(t):
    lines = [
        "// 16.16 fixed-point R'G'B' -> Y'CbCr coefficients of jh_blit_yuv (include/jello_hip.h, DESIGN.md 5.5).",
        "// kYuvMatrix[jh_yuv_matrix][jh_yuv_range] = {Y row, Cb row, Cr row}: round-half-even(exact * 2^16) of the BT.601 / BT.709",
        "// coefficients scaled by 219/255 (luma) and 224/255 (chroma) in limited range, the green coefficient adjusted so that",
        "// the Y row sums to rne(scale * 2^16) and each chroma row to 0.  kYuvOffset[jh_yuv_range] is the luma offset.",
        "// Generated -- do not edit:",
        "//     python tools/gen_yuv_table.py",
        "#pragma once",
        "static const int kYuvMatrix[2][2][9] = {",
    ]
    for i in range(0, len(t), 2):
        lines.append("    {")
        for mname, rname, off, rows in t[i:i + 2]:
            lines.append("        {" + ",  ".join(", ".join("%d" % c for c in row) for row in rows) + "},  // %s %s" % (mname, rname))
        lines.append("    },")
    lines.append("};")
    lines.append("static const int kYuvOffset[2] = {%s};" % ", ".join("%d" % off for _, _, off, _ in t[:2]))
    return "\n".join(lines) + "\n"


def parse(text):
    """The tables of a header written by render(): ([[9 ints] x 4] in header order, [2 offsets])."""
    body = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    m = body[body.index("kYuvMatrix"):body.index("kYuvOffset")]
    nums = [int(s) for s in m[m.index("=") + 1:].replace("{", " ").replace("}", " ").replace(";", " ").replace(",", " ").split()
            if s.lstrip("-").isdigit()]
    o = body[body.index("kYuvOffset"):]
    offs = [int(s) for s in o[o.index("=") + 1:].replace("{", " ").replace("}", " ").replace(";", " ").replace(",", " ").split()]
    return [nums[i:i + 9] for i in range(0, len(nums), 9)], offs


def verify(t):
    """Row sums, greys, and the largest |fixed - exact| over a 52^3 grid of codes (uniform blocks for chroma)."""
    bad = 0
    grid = sorted(set(list(range(0, 256, 5)) + [255]))
    for (mname, kr, kb), (rname, sy, sc, off) in ((m, r) for m in MATRICES for r in RANGES):
        rows = next(x[3] for x in t if x[0] == mname and x[1] == rname)
        ex = exact_rows(kr, kb, sy, sc)
        if sum(rows[0]) != rne(sy * ONE) or sum(rows[1]) or sum(rows[2]):
            bad += 1
        for g in range(256):
            if ((rows[1][0] + rows[1][1] + rows[1][2]) * 4 * g + (1 << 17)) >> 18 != 0:
                bad += 1
        worst = F(0)
        for r in grid:
            for g in grid:
                for b in grid:
                    y = off + ((rows[0][0] * r + rows[0][1] * g + rows[0][2] * b + (1 << 15)) >> 16)
                    worst = max(worst, abs(y - (off + ex[0][0] * r + ex[0][1] * g + ex[0][2] * b)))
                    for k in (1, 2):
                        c = 128 + ((4 * (rows[k][0] * r + rows[k][1] * g + rows[k][2] * b) + (1 << 17)) >> 18)
                        worst = max(worst, abs(c - (128 + ex[k][0] * r + ex[k][1] * g + ex[k][2] * b)))
        print("%s %s: largest |fixed - exact| on the grid: %.4f" % (mname, rname, float(worst)))
        if worst >= F(51, 100):
            bad += 1
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--verify", action="store_true", help="check row sums, greys and the distance to the exact formula")
    ap.add_argument("--out", default=HEADER)
    a = ap.parse_args()
    t = tables()
    with open(a.out, "w") as f:
        f.write(render(t))
    print("wrote", a.out)
    if a.verify:
        bad = verify(t)
        print("failed checks:", bad)
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
