"""No GPU: the LUT rule of DESIGN.md 5.23 -- the exactness it claims, its queries (library and host twin) against tests/lut3d_ref.py,
texels worked by hand, the reference against binary64, the .cube text, the ctypes mirror, the stand-alone check under the
sanitizers, and the battery's sensitivity to near misses."""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import jello_amd
from jello_amd import _lib, lut3d

import lut3d_cases as C
import lut3d_ref as R
from abi_text import INCLUDE, ROOT, c_values
from image_ref import same_bits

F = np.float32
ALL16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)


# ---- the header's constants, the mirror ----

def test_the_headers_constants_and_the_mirrors_layout():
    assert c_values(["JH_LUT3D_MIN_SIZE", "JH_LUT3D_MAX_SIZE"]) == [2, 65]
    assert (jello_amd.LUT3D_MIN_SIZE, jello_amd.LUT3D_MAX_SIZE) == (2, 65) == (lut3d.MIN_SIZE, lut3d.MAX_SIZE) == (R.MIN_SIZE, R.MAX_SIZE)
    fields = [name for name, _ in _lib.CLut3dDesc._fields_]
    want = c_values(["sizeof(jh_lut3d_desc)"] + ["offsetof(jh_lut3d_desc, %s)" % f for f in fields])
    assert [ctypes.sizeof(_lib.CLut3dDesc)] + [getattr(_lib.CLut3dDesc, f).offset for f in fields] == want
    d = jello_amd.imagecalls._lut3d_desc(17, (1, 2, 3, 4))
    assert (d.size, d.flags, d.x, d.y, d.width, d.height) == (17, 0, 1, 2, 3, 4)
    d = jello_amd.imagecalls._lut3d_desc(33, None)
    assert (d.size, d.flags, d.x, d.y, d.width, d.height) == (33, 0, 0, 0, 0, 0)


# ---- step 2 is exact ----

def test_the_position_is_exact_for_every_f16_and_every_size():
    """p = c (N - 1), f = p - k, 1 - f and the differences of two fractions are representable in binary32: the binary32 results are
    the binary64 ones (which are exact: 11 + 7 bits), every fraction is a multiple of 2^-24 in [0, 1] -- so any difference of two is a
    multiple of 2^-24 of magnitude at most 1, a binary32 -- and the four weights sum to exactly 1."""
    h64 = ALL16.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        c64 = np.where(h64 > 0, h64, 0.0)
        c64 = np.where(c64 < 1, c64, 1.0)
    for n in range(R.MIN_SIZE, R.MAX_SIZE + 1):
        k, f = R.position(ALL16, n)
        p64 = c64 * (n - 1)
        assert k.min() >= 0 and k.max() == n - 2
        assert np.array_equal(k, np.minimum(p64.astype(np.int64), n - 2))
        assert np.array_equal(f.astype(np.float64), p64 - k)  # f is exact
        assert f.min() >= 0 and f.max() <= 1
        scaled = f.astype(np.float64) * 2.0 ** 24
        assert np.array_equal(scaled, np.floor(scaled))  # multiples of 2^-24
        assert np.array_equal((F(1) - f).astype(np.float64), 1.0 - f.astype(np.float64))  # 1 - f is exact
    # the weights of all pairs of a sample of fractions, as differences in binary32 against binary64
    k, f = R.position(ALL16[::37], 65)
    a, b = np.meshgrid(f, f)
    assert np.array_equal((a - b).astype(np.float64), a.astype(np.float64) - b.astype(np.float64))
    f3 = np.stack([f, np.roll(f, 5), np.roll(f, 11)], axis=-1)
    _, w = R.walk(f3)
    assert np.all(w.astype(np.float64).sum(axis=-1) == 1.0) and w.min() >= 0


def test_the_vectorised_walk_is_the_explicit_sort():
    rng = np.random.default_rng(5)
    f = rng.integers(0, 5, (400, 3)).astype(F) / F(4)  # many ties
    for ties_g_first in (False, True):
        o1, w1 = R.walk(f, "ties_g_first" if ties_g_first else None)
        o2, w2 = R._walk_fast(f, ties_g_first)
        assert np.array_equal(o1, o2) and np.array_equal(w1, w2)


# ---- the queries against the reference ----

@pytest.mark.parametrize("twin", (False, True), ids=("library", "twin"))
def test_the_identity_query_is_the_references(built, twin):
    for n in range(R.MIN_SIZE, R.MAX_SIZE + 1):
        got = jello_amd.lut3d_identity(n, twin=twin)
        assert np.array_equal(got, R.identity(n)), n
        assert np.array_equal(got, lut3d.as_image(lut3d.identity(n))), n
    t = R.identity(5).reshape(5, 5, 5, 4).view(np.float16)
    assert tuple(t[4, 2, 1]) == (0.25, 0.5, 1.0, 1.0)  # [b, g, r]: red varies fastest


@pytest.mark.parametrize("twin", (False, True), ids=("library", "twin"))
def test_the_texel_query_is_the_reference_on_the_whole_battery(built, twin):
    for case in C.CASES:
        if case["inst"] != "global":  # (the host has one instantiation; the staged cases repeat these inputs)
            continue
        src, lut, prior, rect = C.inputs(case)
        x, y, w, h = R.resolve(src.shape, rect)
        got = jello_amd.lut3d_texels(lut, src[y:y + h, x:x + w], twin=twin)
        assert same_bits(got, C.expected(case)[y:y + h, x:x + w]), case["name"]


def test_legality_and_null_arguments(built):
    table, texels = R.identity(3), np.zeros((2, 4), np.uint16)
    for twin in (False, True):
        qi, qt = jello_amd.imagecalls._query("lut3d_identity", twin), jello_amd.imagecalls._query("lut3d_texels", twin)
        out = np.full((2, 4), 0x1234, np.uint16)
        big = np.full((65 ** 3, 4), 0x1234, np.uint16)
        for n in (2, 3, 65):
            assert qi(n, big.ctypes.data) == 0
        assert qt(3, table.ctypes.data, texels.ctypes.data, 2, out.ctypes.data) == 0 and not np.any(out == 0x1234)
        assert qt(3, table.ctypes.data, None, 0, None) == 0
        out[:] = 0x1234
        big[:] = 0x1234
        for n in (0, 1, 66, 0xFFFFFFFF):
            assert qi(n, big.ctypes.data) != 0 and qt(n, table.ctypes.data, texels.ctypes.data, 2, out.ctypes.data) != 0
        assert qi(3, None) != 0
        assert qt(3, None, texels.ctypes.data, 2, out.ctypes.data) != 0 and qt(3, table.ctypes.data, None, 2, out.ctypes.data) != 0
        assert qt(3, table.ctypes.data, texels.ctypes.data, 2, None) != 0
        assert np.all(out == 0x1234) and np.all(big == 0x1234)
        if twin:
            L = jello_amd.load_host()
            assert qi(1, big.ctypes.data) != 0 and L.jl_last_error().startswith(b"lut3d_identity: size outside 2..65")
            assert qt(3, None, None, 0, None) != 0 and L.jl_last_error().startswith(b"lut3d_texels: null argument")
        for n in (1, 66):
            with pytest.raises(ValueError, match="jh_lut3d_identity: "):
                jello_amd.lut3d_identity(n, twin=twin)
        with pytest.raises(ValueError, match="jh_lut3d_texels: "):
            jello_amd.lut3d_texels(np.zeros((5, 2, 4), np.uint16), texels, twin=twin)
        with pytest.raises(ValueError, match="jh_lut3d_texels: "):
            jello_amd.lut3d_texels(table, np.zeros((2, 3), np.uint16), twin=twin)


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    assert hip.jh_lut3d(None, 1, 2, 3, ctypes.byref(_lib.CLut3dDesc())) == -1 and hip.jh_lut3d(None, 1, 2, 3, None) == -1
    assert hip.jh_debug_lut3d_variant(None, 0) == -1


# ---- texels by hand ----

def _power_table():
    """N = 2: the red of vertex (i, j, k) is 2^-(1 + i + 2 j + 4 k), green 1 - that, blue the vertex number / 8: nothing affine."""
    t = np.empty((2, 2, 2, 4), np.float64)  # [k, j, i]
    for k in range(2):
        for j in range(2):
            for i in range(2):
                v = i + 2 * j + 4 * k
                t[k, j, i] = (2.0 ** -(1 + v), 1.0 - 2.0 ** -(1 + v), v / 8.0, 0.0)
    return t


HAND = [  # (r, g, b), the order of the axes, the vertices (i, j, k) and the weights -- worked on paper for N = 2, where f = the value
    ((0.5, 0.25, 0.125), "rgb", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)], (0.5, 0.25, 0.125, 0.125)),
    ((0.5, 0.125, 0.25), "rbg", [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1)], (0.5, 0.25, 0.125, 0.125)),
    ((0.25, 0.5, 0.125), "grb", [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1)], (0.5, 0.25, 0.125, 0.125)),
    ((0.125, 0.5, 0.25), "gbr", [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 1)], (0.5, 0.25, 0.125, 0.125)),
    ((0.25, 0.125, 0.5), "brg", [(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1)], (0.5, 0.25, 0.125, 0.125)),
    ((0.125, 0.25, 0.5), "bgr", [(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)], (0.5, 0.25, 0.125, 0.125)),
    ((0.5, 0.5, 0.25), "rgb", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)], (0.5, 0.0, 0.25, 0.25)),    # r == g above b: r first
    ((0.25, 0.25, 0.5), "brg", [(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1)], (0.5, 0.25, 0.0, 0.25)),   # r == g below b
    ((0.25, 0.5, 0.5), "gbr", [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 1)], (0.5, 0.0, 0.25, 0.25)),    # g == b above r: g first
    ((0.5, 0.25, 0.25), "rgb", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)], (0.5, 0.25, 0.0, 0.25)),   # g == b below r
    ((0.5, 0.25, 0.5), "rbg", [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1)], (0.5, 0.0, 0.25, 0.25)),    # r == b above g: r first
    ((0.25, 0.5, 0.25), "grb", [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1)], (0.5, 0.25, 0.0, 0.25)),   # r == b below g
    ((0.75, 0.75, 0.75), "rgb", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)], (0.25, 0.0, 0.0, 0.75)),  # all three equal
    ((0.0, 0.0, 0.0), "rgb", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)], (1.0, 0.0, 0.0, 0.0)),
    ((1.0, 1.0, 1.0), "rgb", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)], (0.0, 0.0, 0.0, 1.0)),       # k stays N - 2, f = 1
    ((2.0, -1.0, 0.5), "rbg", [(0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1)], (0.0, 0.5, 0.5, 0.0)),      # clamped to (1, 0, 0.5)
]


@pytest.mark.parametrize("twin", (False, True), ids=("library", "twin"))
def test_texels_by_hand(built, twin):
    table = _power_table()
    image = lut3d.as_image(table[..., :3])
    for (rgb, axes, verts, weights) in HAND:
        texel = np.array([rgb + (0.3,)], np.float16).view(np.uint16)
        k, f = R.position(texel[..., :3], 2)
        order, w = R.walk(f)
        assert ["rgb"[a] for a in order[0]] == list(axes), rgb
        assert [tuple(v) for v in R.vertices(k, order)[0]] == verts, rgb
        assert tuple(float(x) for x in w[0]) == weights, rgb
        want = [sum(Fraction(wi) * Fraction(float(np.float16(table[v[2], v[1], v[0], c]))) for wi, v in zip(weights, verts)) for c in range(3)]
        want_bits = np.array([float(x) for x in want], np.float64).astype(np.float16).view(np.uint16)  # (exact sums of a few bits: one rounding)
        for got in (R.texels(texel, image), jello_amd.lut3d_texels(image, texel, twin=twin)):
            assert np.array_equal(got[0, :3], want_bits), rgb
            assert got[0, 3] == texel[0, 3]


def test_consequences_of_the_rule():
    """An identity table of a power-of-two N - 1 returns the clamped input bit for bit; a constant table of powers of two returns
    its colour exactly (every partial sum c (1 - f) is exact); alpha never changes, whatever the table's alpha."""
    bits = C.VALUES
    h = bits[..., :3].view(np.float16).astype(np.float32)
    clamped = bits.copy()
    with np.errstate(invalid="ignore"):
        clamped[..., :3] = np.where(np.isnan(h) | (h <= 0), 0, np.where(h >= 1, 0x3C00, bits[..., :3]))
    for n in (2, 3, 5, 9, 17, 33, 65):
        assert np.array_equal(R.texels(bits, R.identity(n)), clamped), n
    for n in (2, 7, 65):
        got = R.texels(bits, C.lut_image("constant", n))
        assert np.all(got[..., :3].view(np.float16) == np.array(C.CONSTANT, np.float16)) and np.array_equal(got[..., 3], bits[..., 3])
    assert np.array_equal(R.texels(bits, C.lut_image("nonfinite", 4))[..., 3], bits[..., 3])


# ---- the reference against binary64 ----

def test_the_reference_is_within_its_roundings_of_the_binary64_interpolation():
    """The position and the weights are exact, so what separates the rule from the real tetrahedral interpolation S is four binary32
    roundings and one to f16.  With entries of magnitude at most E = 1 every partial sum is a part of a convex combination, at most
    E in magnitude, so each binary32 rounding adds at most 2^-24 E (1 + 2^-22): |m - S| <= e = 4 x 2^-24 x (1 + 2^-22).  Then f16(m)
    is within half an f16 ulp of m: max(2^-11 |m|, 2^-25) <= max(2^-11 (|S| + e), 2^-25).  The test reports the largest fraction of
    that bound any value uses."""
    rng = np.random.default_rng(23)
    texels = rng.uniform(-0.05, 1.05, (96, 96, 4)).astype(np.float16).view(np.uint16)
    worst = 0.0
    for n in (2, 5, 17, 64):
        table = C.lut_image("random", n)
        S = R.definition(texels, table)
        got = R.texels(texels, table)[..., :3].view(np.float16).astype(np.float64)
        e = 4 * 2.0 ** -24 * (1 + 2.0 ** -22)
        bound = e + np.maximum(2.0 ** -11 * (np.abs(S) + e), 2.0 ** -25)
        used = np.abs(got - S) / bound
        worst = max(worst, float(used.max()))
        assert used.max() <= 1.0, n
    print("reference against binary64: %.1f %% of the bound used" % (100 * worst))
    assert worst > 0.5  # (the bound is not slack by more than a factor of two: the f16 rounding alone reaches half an ulp)


def test_affine_tables_agree_with_trilinear_interpolation():
    """On a table that samples an affine function both interpolations give that function, exactly in the reals: with entries
    (a i + b j + c k + d) / 64 on N = 17 (exact f16) the binary64 sums are exact too (a few bits each)."""
    n = 17
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    table = np.stack([(3 * i + j + 0 * k + 2) / 128.0, (i + 2 * j + k) / 64.0, (48 - i - j - k) / 64.0], axis=-1)
    image = lut3d.as_image(table)
    assert np.array_equal(lut3d.from_image(image), table)  # exact f16
    rng = np.random.default_rng(29)
    texels = rng.integers(0, 1025, (64, 64, 4)).astype(np.float64) / 1024.0  # multiples of 2^-10: the products stay within binary64
    bits = texels.astype(np.float16).view(np.uint16)
    tetra, tri = R.definition(bits, image), R.trilinear64(bits, image)
    x = bits[..., :3].view(np.float16).astype(np.float64) * 16
    want = np.stack([(3 * x[..., 0] + x[..., 1] + 2) / 128.0, (x[..., 0] + 2 * x[..., 1] + x[..., 2]) / 64.0, (48 - x.sum(axis=-1)) / 64.0], axis=-1)
    assert np.array_equal(tetra, want) and np.array_equal(tri, want)


# ---- jello_amd.lut3d ----

def test_tables_images_and_the_cube_text():
    t = lut3d.from_function(4, lambda c: np.stack([c[..., 2], c[..., 0] * c[..., 1], 1 - c[..., 0]], axis=-1))
    assert t.shape == (4, 4, 4, 3) and tuple(t[3, 2, 1]) == (1.0, (1 / 3) * (2 / 3), 1 - 1 / 3)  # [b, g, r]
    assert np.array_equal(lut3d.from_cube(lut3d.to_cube(t, title="a name # with a hash")), t)  # 17 digits: the float64 back
    image = lut3d.as_image(t)
    assert image.shape == (16, 4, 4) and np.all(image[..., 3] == 0x3C00)
    assert np.array_equal(image[2 + 4 * 3, 1, :3], np.array(t[3, 2, 1], np.float16).view(np.uint16))  # (x = r, y = g + N b)
    back = lut3d.from_image(image)
    assert np.array_equal(back, t.astype(np.float16).astype(np.float64)) and np.array_equal(lut3d.as_image(back), image)
    text = "# comment\nTITLE \"t\"\n\nLUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1.0 1.0 1.0\n" + "".join(
        "%d %d.5 %d # entry\n" % (i & 1, i >> 1 & 1, i >> 2) for i in range(8))
    got = lut3d.from_cube(text)
    assert got.shape == (2, 2, 2, 3) and tuple(got[1, 0, 1]) == (1.0, 0.5, 1.0) and tuple(got[0, 1, 0]) == (0.0, 1.5, 0.0)
    body = "".join("0 0 0\n" for _ in range(8))
    for bad in ("LUT_1D_SIZE 8\n" + body, "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0.1\n" + body, "LUT_3D_SIZE 2\nDOMAIN_MAX 1 1 2\n" + body, body,
                "LUT_3D_SIZE 2\n" + body + "0 0 0\n", "LUT_3D_SIZE 2\n" + body[:-6], "LUT_3D_SIZE 1\n0 0 0\n", "LUT_3D_SIZE 66\n", "LUT_3D_SIZE 2\n0 0\n" + body,
                "LUT_3D_SIZE 2\nLUT_3D_SIZE 2\n" + body, "LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0 1\n" + body, "LUT_3D_SIZE 2.5\n" + body):
        with pytest.raises(ValueError, match="lut3d: "):
            lut3d.from_cube(bad)
    for bad in (np.zeros((2, 2, 3, 3)), np.zeros((2, 2, 2, 4)), np.zeros((1, 1, 1, 3)), np.zeros((66, 66, 66, 3))):
        with pytest.raises(ValueError, match="lut3d: "):
            lut3d.as_image(bad)
    for bad in (np.zeros((4, 2, 3), np.uint16), np.zeros((5, 2, 4), np.uint16), np.zeros((1, 1, 4), np.uint16)):
        with pytest.raises(ValueError, match="lut3d: "):
            lut3d.from_image(bad)
    with pytest.raises(ValueError, match="lut3d: "):
        lut3d.identity(1)
    with pytest.raises(ValueError, match="lut3d: "):
        lut3d.from_function(3, lambda c: c[..., :2])


# ---- the stand-alone program ----

@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/lut3d_check.cpp, a program with a main of its own, built with ASan and UBSan as its header says."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("lut3d_check") / "lut3d_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wno-comment", "-I", INCLUDE, os.path.join(ROOT, "tools", "lut3d_check.cpp"), "-o", exe])
    return exe


def test_the_stand_alone_check_passes_under_the_sanitizers(check_program):
    out = subprocess.check_output([check_program]).decode()
    assert out.startswith("ok: 4194304 positions, 320388 walks, "), out  # (64 sizes x 65 536 patterns; the lattices of N = 2..5)


@pytest.mark.parametrize("n,kind", [(2, "nonfinite"), (3, "ties_all"), (4, "wild"), (5, "random")])
def test_the_programs_texels_are_the_references(check_program, n, kind):
    table = C.lut_image(kind, n)
    texels = np.concatenate([C.TIES[0], C.VALUES[::16, ::16].reshape(-1, 4)])
    text = subprocess.check_output([check_program, str(n), "".join("%04x" % v for v in table.reshape(-1)), "".join("%04x" % v for v in texels.reshape(-1))]).decode()
    got = np.array([[int(v, 16) for v in line.split()] for line in text.splitlines()], np.uint16)
    assert same_bits(got, R.texels(texels, table))


# ---- the battery ----

SENSITIVE_CASES = ["ties_rg_n3_global", "ties_all_n3_global", "values_nonfinite_n3_global", "values_wild_n3_global", "values_random_n33_global"]


@pytest.mark.parametrize("miss", R.VARIANTS)
def test_the_battery_tells_the_rule_from_a_near_miss(miss):
    """Each wrong rule -- trilinear; ties g before r; (int)(p + 0.5); k clamped to N - 1 with a wrap; V0 + f (V1 - V0); multiply and
    add unfused; zero weights skipped; a min / max clamp that hands NaN on; alpha put through the table -- changes bytes of the
    battery's expected output."""
    changed = {}
    for name in SENSITIVE_CASES:
        case = C.BY_NAME[name]
        changed[name] = int(np.sum(C.expected(case) != C.expected(case, miss)))
    print(miss, changed)
    assert any(changed.values())


def test_the_battery_covers_what_it_claims():
    sizes = {inst: {c["n"] for c in C.CASES if c["inst"] == inst} for inst in C.INSTANTIATIONS}
    assert sizes["staged"] >= {2, 3, 4, 16, 17} and max(sizes["staged"]) == C.STAGED_MAX == 17
    assert sizes["global"] >= set(C.SIZES)
    with open(os.path.join(INCLUDE, "jello_lut3d.h")) as f:
        assert re.search(r"#define JLUT_STAGED_MAX_SIZE (\d+)u", f.read()).group(1) == str(C.STAGED_MAX)
    geo = [c for c in C.CASES if "values" not in c]
    for inst in C.INSTANTIATIONS:
        mine = [c for c in geo if c["inst"] == inst]
        shapes = {c["src_size"] for c in mine}
        assert {(1, 1), (1, 5), (5, 1)} <= shapes
        widths = {(c["rect"][2] if c["rect"] else c["src_size"][0]) for c in mine}
        assert {511, 512, 513, 1023, 1024, 1025} <= widths
        assert any(c["rect"] and c["rect"][0] % 2 and c["rect"][2] % 2 for c in mine)  # odd x and odd width
        assert any(c["src_size"] != c["dst_size"] for c in mine) and any(c["in_place"] for c in mine) and any(not c["in_place"] for c in mine)
        assert any((c["rect"][3] if c["rect"] else c["src_size"][1]) > 8 * 256 for c in mine)  # more items than 8 workgroups on each of 256 CUs
    for c in C.CASES:
        src, _, prior, _ = C.inputs(c)
        assert src.shape[0] * src.shape[1] <= 2 ** 17 and prior.shape[0] * prior.shape[1] <= 2 ** 17, c["name"]
    # every f16 pattern in every channel; every tie among the hand-made texels
    for ch in range(4):
        assert len(np.unique(C.VALUES[..., ch])) == 65536
    _, f = R.position(C.TIES[0, :, :3], 3)
    ties = {(bool(a == b), bool(b == c), bool(a == c)) for a, b, c in f}
    assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, False, False)} <= ties
