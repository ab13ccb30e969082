"""The load rule of DESIGN.md 5.21 without a GPU: the tables, the batch queries of the library and of its host twin against
tests/load_ref.py over every input that matters, the rule's properties with their derived bounds, hand values, legality, the ctypes
mirrors, the stand-alone check under the sanitizers, and the battery's sensitivity to near misses."""
import ctypes
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import jello_amd
from jello_amd import ChromaFilter, LoadAlpha, Surface, YuvTransfer, _lib

import load_cases
import load_ref as R
import surface_ref
import yuv_ref
from abi_text import INCLUDE, ROOT, c_values

F = np.float32
sys.path.append(os.path.join(ROOT, "tools"))  # (gen_load_tables; appended, so that it shadows nothing)


@pytest.fixture(scope="module")
def triples():
    """All 2^24 (Y, Cb, Cr) as three flat uint8 arrays, and the sums of a replicated chroma."""
    y, cb, cr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return y.reshape(-1), cb.reshape(-1), cr.reshape(-1)


# ---- the header, the mirrors, the tables ----

def test_the_headers_constants_and_the_mirrors_layout():
    names = ["JH_LOAD_ALPHA_STRAIGHT", "JH_LOAD_ALPHA_PREMULTIPLIED", "JH_LOAD_ALPHA_OPAQUE", "JH_CHROMA_REPLICATE", "JH_CHROMA_BILINEAR"]
    assert c_values(names) == [0, 1, 2, 0, 1]
    assert [int(v) for v in LoadAlpha] == list(R.ALPHAS) and [int(v) for v in ChromaFilter] == list(R.CHROMAS)
    assert [int(v) for v in Surface] == list(R.FORMATS) and [int(v) for v in YuvTransfer] == list(R.TRANSFERS)
    for struct, ctype in (("jh_load_surface_desc", _lib.CLoadSurfaceDesc), ("jh_load_yuv_desc", _lib.CLoadYuvDesc)):
        fields = [name for name, _ in ctype._fields_]
        want = c_values(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, f) for f in fields])
        assert [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields] == want, struct


def test_the_descriptors_python_builds():
    d = jello_amd.engine._load_surface_desc(Surface.BGRA8_SRGB, LoadAlpha.OPAQUE, 0x1000, 64, (1, 2, 3, 4))
    assert (d.format, d.alpha, d.src, d.pitch, d.x, d.y, d.width, d.height) == (3, 2, 0x1000, 64, 1, 2, 3, 4)
    d = jello_amd.engine._load_yuv_desc(1, 0, 1, 1, ChromaFilter.BILINEAR, [(0x10, 7), (0x20, 4), (0x30, 5)], None)
    assert (d.layout, d.matrix, d.range, d.transfer, d.chroma, d.reserved, d.width, d.height) == (1, 0, 1, 1, 1, 0, 0, 0)
    assert list(d.plane) == [0x10, 0x20, 0x30] and list(d.pitch) == [7, 4, 5]


def test_host_arrays_are_described_by_their_own_size():
    """What Engine.load_surface and Engine.load_yuv upload and put into the descriptor for host arrays: without a rectangle it is
    (0, 0, w, h) of the ARRAY -- never 0 x 0, which names the whole image and would have the kernel read an image's worth of rows
    from an upload of the array's -- the pitches are the array's rows, and the bytes are all that is uploaded."""
    src = jello_amd.imagecalls._surface_array_source
    px = np.arange(9 * 21 * 4, dtype=np.uint8).reshape(9, 21, 4)
    host, pitch, rect = src(px, None)
    assert rect == (0, 0, 21, 9) and pitch == 84 and host.size == 9 * 84 and np.array_equal(host, px.reshape(-1))
    assert src(px, (3, 2, 21, 9))[2] == (3, 2, 21, 9)
    d = jello_amd.engine._load_surface_desc(0, 0, 0x1000, pitch, rect)
    assert (d.width, d.height) == (21, 9)  # (what the library takes as the frame's size)
    assert src(np.zeros((0, 5, 4), np.uint8), None) is None
    for bad_px, bad_rect in ((px, (0, 0, 21, 13)), (px, (0, 0, 0, 0)), (px, (0, 0, 20, 9)), (px[..., :3], None), (px[0], None)):
        with pytest.raises(ValueError, match="jh_load_surface: "):
            src(bad_px, bad_rect)
    yuv = jello_amd.imagecalls._yuv_array_source
    y, cb, cr = load_cases.random_frame(21, 9, 1)
    for layout, planes, pitches in ((0, (y, np.stack([cb, cr], axis=-1)), [21, 22]), (0, (y, np.stack([cb, cr], axis=-1).reshape(5, 22)), [21, 22]),
                                    (1, (y, cb, cr), [21, 11, 11])):
        host, placed, rect = yuv(planes, layout, None)
        assert rect == (0, 0, 21, 9) and [p for _, p in placed] == pitches and all(o % 16 == 0 for o, _ in placed)
        assert host.size >= placed[-1][0] + 5 * pitches[-1] and np.array_equal(host[:189], y.reshape(-1))
        assert yuv(planes, layout, (4, 4, 21, 9))[2] == (4, 4, 21, 9)
    assert yuv((np.zeros((0, 4), np.uint8), np.zeros((0, 2, 2), np.uint8)), 0, None) is None
    for planes, layout, bad_rect in (((y, cb, cr), 1, (0, 0, 21, 13)), ((y, cb, cr), 1, (0, 0, 0, 0)), ((y, cb), 1, None), ((y, cb, cr), 0, None),
                                     ((y[:8], cb, cr), 1, None), ((y.reshape(-1), cb, cr), 1, None), ((y, cb, cr), 2, None), ((), 1, None),
                                     ((y, (0x1000, 11), cr), 1, None)):
        with pytest.raises(ValueError, match="jh_load_yuv: "):
            yuv(planes, layout, bad_rect)


def test_the_tables_of_the_rule_from_the_reference_the_generator_and_the_header():
    import gen_load_tables
    want = {(R.BT601, R.LIMITED): [76309, 104597, -25675, -53279, 132201], (R.BT601, R.FULL): [65536, 91881, -22553, -46802, 116130],
            (R.BT709, R.LIMITED): [76309, 117489, -13975, -34925, 138438], (R.BT709, R.FULL): [65536, 103206, -12276, -30679, 121609]}
    header = gen_load_tables.parse(open(gen_load_tables.HEADER).read())
    generated = {(m, r): k for (m, r), (_, _, _, k) in zip(((m, r) for m in R.MATRICES for r in R.RANGES), gen_load_tables.yuv_tables())}
    for i, ((m, r), k) in enumerate(want.items()):
        assert R.table(m, r) == (k, 16 if r == R.LIMITED else 0) and generated[(m, r)] == k and header["kLoadYuv"][5 * i:5 * i + 5] == k
    assert header["kLoadYuvOffset"] == [16, 0]
    codes = np.arange(256, dtype=np.uint8)
    assert header["kLoadUnormF16"] == [int(v) for v in R.unorm_table().astype(np.float16).view(np.uint16)]
    assert header["kLoadSrgbF16"] == [int(v) for v in R.linear_table().astype(np.float16).view(np.uint16)]
    assert header["kLoadSrgbF32"] == [int(v) for v in R.linear_table().view(np.uint32)]
    assert list(gen_load_tables.srgb_to_linear()) == [Fraction(float(v)) for v in R.linear_table()]  # the table fine uses is the reference's L
    px = np.stack([codes, codes, codes, codes], axis=-1)
    for twin in (False, True):
        assert [int(v) for v in jello_amd.load_texels(px, fmt=Surface.RGBA8_UNORM, twin=twin)[:, 3]] == header["kLoadUnormF16"]
        assert [int(v) for v in jello_amd.load_texels(px, fmt=Surface.RGBA8_SRGB, twin=twin)[:, 0]] == header["kLoadSrgbF16"]


def test_the_generators_verify_passes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_load_tables.py"), "--verify"], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and "failed checks: 0" in out.stdout, out.stdout


def test_u_is_the_nearest_binary32_and_the_ieee_quotient():
    U = R.unorm_table()
    for c in range(256):
        q, u = Fraction(c, 255), Fraction(float(U[c]))
        for other in (np.nextafter(U[c], F(2.0)), np.nextafter(U[c], F(-1.0))):
            assert abs(u - q) <= abs(Fraction(float(other)) - q), c
    assert not np.array_equal(U, R.unorm_table(reciprocal=True))  # (c * (1 / 255) is another table)


# ---- the queries against the reference ----

@pytest.mark.parametrize("matrix", R.MATRICES)
@pytest.mark.parametrize("rng", R.RANGES)
def test_the_codes_of_all_triples_and_their_distance_to_the_real_formula(built, triples, matrix, rng):
    """jh_load_yuv_codes and jl_load_yuv_codes = the reference over all 2^24 triples; every code within 0.51 of the real-valued inverse
    matrix, clamped: 0.5 of rounding and (239 + 2 * 128) * 0.5 / 65536 of coefficient error."""
    y, cb, cr = triples
    want = R.codes(y, 16 * cb.astype(np.int64), 16 * cr.astype(np.int64), matrix, rng)
    s_cb, s_cr = (16 * cb.astype(np.uint16)), (16 * cr.astype(np.uint16))
    for twin in (False, True):
        assert np.array_equal(jello_amd.load_yuv_codes(y, s_cb, s_cr, matrix, rng, twin=twin), want), twin
    worst = float(np.abs(want - R.exact_codes(y, cb, cr, matrix, rng)).max())
    print("matrix %d range %d: largest |codes - real| = %.4f" % (matrix, rng, worst))
    assert worst <= 0.51


def test_the_codes_of_bilinear_sums(built):
    """Sums that are no multiple of 16, the extremes among them, on every table."""
    g = np.random.default_rng(5)
    y = g.integers(0, 256, 200000).astype(np.uint8)
    s_cb, s_cr = g.integers(0, 4081, 200000).astype(np.uint16), g.integers(0, 4081, 200000).astype(np.uint16)
    y[:4], s_cb[:4], s_cr[:4] = (0, 255, 0, 255), (0, 4080, 4080, 0), (0, 4080, 0, 4080)
    for m in R.MATRICES:
        for r in R.RANGES:
            for twin in (False, True):
                assert np.array_equal(jello_amd.load_yuv_codes(y, s_cb, s_cr, m, r, twin=twin), R.codes(y, s_cb, s_cr, m, r))


@pytest.mark.parametrize("srgb,alpha", load_cases.SURFACE_INSTANCES, ids=lambda v: str(int(v)))
def test_the_texels_of_all_code_alpha_pairs(built, srgb, alpha):
    """A channel depends on its code and on alpha only: all 256 x 256 pairs per transfer and alpha mode, in every channel position and
    both byte orders."""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for k in range(3):
        px = np.zeros((256, 256, 4), np.uint8)
        px[..., k], px[..., (k + 1) % 3], px[..., (k + 2) % 3], px[..., 3] = c, 255 - c, c ^ 0x5A, a
        for fmt in ((R.RGBA8_SRGB, R.BGRA8_SRGB) if srgb else (R.RGBA8_UNORM, R.BGRA8_UNORM)):
            want = R.texels(px, fmt=fmt, alpha=alpha)
            for twin in (False, True):
                assert np.array_equal(jello_amd.load_texels(px, fmt=fmt, alpha=alpha, twin=twin), want), (k, fmt, twin)
    rgba = R.texels(px, fmt=R.RGBA8_SRGB if srgb else R.RGBA8_UNORM, alpha=alpha)
    assert np.array_equal(jello_amd.load_texels(px, transfer=int(srgb), alpha=alpha), rgba)  # (a transfer names RGBA codes)


# ---- the properties ----

def test_every_grey_goes_back_to_its_luma():
    for m in R.MATRICES:
        for r in R.RANGES:
            y = np.arange(16, 236) if r == R.LIMITED else np.arange(256)
            rgb = R.codes(y, np.full_like(y, 2048), np.full_like(y, 2048), m, r)
            assert np.all(rgb[:, 0] == rgb[:, 1]) and np.all(rgb[:, 1] == rgb[:, 2])
            assert np.array_equal(yuv_ref.luma(rgb, m, r), y), (m, r)


def test_an_opaque_surface_round_trips_through_the_blit():
    """jh_blit(jh_load_surface(S)) = S on the references, for all 256 codes in both transfers: f16 keeps enough of U and L."""
    c = np.arange(256, dtype=np.uint8)
    s = np.stack([c, c[::-1], np.roll(c, 100), np.full(256, 255, np.uint8)], axis=-1)[None]
    for fmt in R.FORMATS:
        for alpha in R.ALPHAS:
            assert np.array_equal(surface_ref.convert(R.texels(s, fmt=fmt, alpha=alpha), fmt), s), (fmt, alpha)


def test_codes_through_444_and_back():
    """R'G'B' codes -> yuv_ref as 4:4:4 (S = 4 x code) -> the load rule: each channel within floor(0.5015 (Ky + sum |chroma coefficients
    of its row|) / 65536 + 0.504) codes, computed from the exact coefficients (their quotient by 65536 already taken): 2 for B and 1 for
    R and G in limited range (R: 1.89 for BT.601 and 1.99 for BT.709, below 2), 1 in full range.  A run over 2 000 000 codes reached
    exactly these."""
    g = np.random.default_rng(9)
    rgb = g.integers(0, 256, (200000, 3))
    rgb[:8] = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    for m in R.MATRICES:
        for r in R.RANGES:
            k, _ = R.exact_coefficients(m, r)
            bound = [int(Fraction(5015, 10000) * (k[0] + sum(abs(c) for c in row)) + Fraction(504, 1000)) for row in ((k[1],), (k[2], k[3]), (k[4],))]
            assert bound == ([1, 1, 2] if r == R.LIMITED else [1, 1, 1])
            y = yuv_ref.luma(rgb, m, r)
            cb, cr = yuv_ref.chroma_of_sums(4 * rgb, m, r)
            back = R.codes(y, 16 * cb, 16 * cr, m, r)
            worst = np.abs(back - rgb).max(axis=0)
            print("matrix %d range %d: largest |back - codes| = %s, bound %s" % (m, r, worst, bound))
            assert np.all(worst <= bound), (m, r, worst)


def test_constant_chroma_gives_the_same_sums_under_both_modes():
    for w, h in ((1, 1), (2, 3), (5, 4), (7, 7)):
        plane = np.full(((h + 1) // 2, (w + 1) // 2), 77)
        assert np.array_equal(R.chroma_sums(plane, w, h, R.REPLICATE), R.chroma_sums(plane, w, h, R.BILINEAR))


# ---- by hand ----

def test_the_hand_values(built):
    rows = [((235, 128, 128), (255, 255, 255)), ((63, 102, 240), (255, 1, 0)), ((173, 42, 26), (0, 255, 1)), ((32, 240, 118), (1, 0, 255)),
            ((16, 128, 128), (0, 0, 0))]
    for (y, cb, cr), rgb in rows:
        assert tuple(R.codes(y, 16 * cb, 16 * cr, R.BT709, R.LIMITED)) == rgb
        for twin in (False, True):
            assert tuple(jello_amd.load_yuv_codes([y], [16 * cb], [16 * cr], R.BT709, R.LIMITED, twin=twin)[0]) == rgb


def test_the_chroma_weights_by_hand():
    """A 4 x 4 frame, chroma (2, 2) = [[0, 16], [32, 48]]: texel (1, 1) blends 9 x 0 + 3 x 16 + 3 x 32 + 48; the corner repeats its sample."""
    plane = np.array([[0, 16], [32, 48]])
    s = R.chroma_sums(plane, 4, 4, R.BILINEAR)
    assert s[1, 1] == 9 * 0 + 3 * 16 + 3 * 32 + 48 and s[0, 0] == 0 and s[3, 3] == 16 * 48
    assert s[0, 1] == 9 * 0 + 3 * 16 + 3 * 0 + 16 and s[2, 2] == 9 * 48 + 3 * 32 + 3 * 16 + 0
    assert np.array_equal(R.chroma_sums(plane, 4, 4, R.REPLICATE), 16 * np.repeat(np.repeat(plane, 2, axis=0), 2, axis=1))
    one = R.chroma_sums(np.array([[200]]), 1, 1, R.BILINEAR)
    assert one.shape == (1, 1) and one[0, 0] == 3200


def test_texels_by_hand(built):
    """Straight: (255, 0, 51, 128) -> 1.0, 0, f16(0.2), f16(128 / 255).  Premultiplied (51, 102, 0, 102): the colour over alpha.  Alpha 0
    under a colour: the floor of the store rule, Inf in f16.  OPAQUE ignores byte 3.  BGRA swaps."""
    f16 = lambda v: int(np.float16(F(v)).view(np.uint16))  # noqa: E731
    for twin in (False, True):
        t = lambda px, **kw: [int(v) for v in jello_amd.load_texels(np.array(px, np.uint8), twin=twin, **kw)]  # noqa: E731
        assert t((255, 0, 51, 128), fmt=0) == [0x3C00, 0, f16(F(51) / F(255)), f16(F(128) / F(255))]
        a = F(102) / F(255)
        assert t((51, 102, 0, 102), fmt=0, alpha=1) == [f16(F(51) / F(255) * (F(1) / a)), f16(a * (F(1) / a)), 0, f16(a)]
        assert t((255, 0, 0, 0), fmt=0, alpha=1) == [0x7C00, 0, 0, 0]  # 1.0 / 1e-6 is beyond f16
        assert t((0, 0, 0, 0), fmt=0, alpha=1) == [0, 0, 0, 0]
        assert t((10, 20, 30, 9), fmt=0, alpha=2) == t((10, 20, 30, 200), fmt=0, alpha=2) and t((10, 20, 30, 9), fmt=0, alpha=2)[3] == 0x3C00
        assert t((10, 20, 30, 40), fmt=1) == t((30, 20, 10, 40), fmt=0)
        assert t((255, 128, 0, 255), fmt=2)[:3] == [0x3C00, f16(R.linear_table()[128]), 0]
        assert t((255, 128, 0, 255), fmt=2)[3] == 0x3C00 and t((1, 1, 1, 1), fmt=2)[3] == f16(F(1) / F(255))  # alpha is never decoded


# ---- legality, null arguments ----

def test_legality_and_null_arguments(built):
    px, out = np.zeros((2, 4), np.uint8), np.full((2, 4), 0x1234, np.uint16)
    y, s, rgb = np.zeros(2, np.uint8), np.zeros(2, np.uint16), np.full((2, 3), 7, np.uint8)
    for twin in (False, True):
        q, qc = jello_amd.imagecalls._query("load_texel", twin), jello_amd.imagecalls._query("load_yuv_codes", twin)
        for fmt in range(6):
            for alpha in range(3):
                assert q(fmt, alpha, 2, px.ctypes.data, out.ctypes.data) == 0
        out[:] = 0x1234
        for fmt, alpha in ((-1, 0), (6, 0), (0, -1), (0, 3)):
            assert q(fmt, alpha, 2, px.ctypes.data, out.ctypes.data) != 0
        assert q(0, 0, 2, None, out.ctypes.data) != 0 and q(0, 0, 2, px.ctypes.data, None) != 0 and q(0, 0, 0, None, None) == 0
        assert np.all(out == 0x1234)
        for m, r in ((-1, 0), (2, 0), (0, -1), (0, 2)):
            assert qc(m, r, 2, y.ctypes.data, s.ctypes.data, s.ctypes.data, rgb.ctypes.data) != 0
        assert qc(0, 0, 2, None, s.ctypes.data, s.ctypes.data, rgb.ctypes.data) != 0 and qc(0, 0, 2, y.ctypes.data, s.ctypes.data, s.ctypes.data, None) != 0
        big = np.array([0, 4081], np.uint16)
        assert qc(0, 0, 2, y.ctypes.data, s.ctypes.data, big.ctypes.data, rgb.ctypes.data) != 0
        assert np.all(rgb == 7)
        most = np.array([0, 4080], np.uint16)
        assert qc(0, 0, 2, y.ctypes.data, s.ctypes.data, most.ctypes.data, rgb.ctypes.data) == 0
        rgb[:] = 7
        with pytest.raises(ValueError, match="jh_load_texel: "):
            jello_amd.load_texels(px, fmt=4, twin=twin)
        with pytest.raises(ValueError, match="jh_load_yuv_codes: "):
            jello_amd.load_yuv_codes(y, s, s, 2, 0, twin=twin)


def test_a_null_context_is_refused_without_a_device(built):
    hip = jello_amd.load_host().hip
    assert hip.jh_load_surface(None, 1, ctypes.byref(_lib.CLoadSurfaceDesc())) == -1 and hip.jh_load_yuv(None, 1, ctypes.byref(_lib.CLoadYuvDesc())) == -1
    assert hip.jh_load_surface(None, 1, None) == -1 and hip.jh_load_yuv(None, 1, None) == -1


# ---- the stand-alone program ----

@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/load_check.cpp, a program with a main of its own, built with ASan and UBSan as its header says."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("load_check") / "load_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wno-comment", "-I", INCLUDE, os.path.join(ROOT, "tools", "load_check.cpp"), "-o", exe])
    return exe


def test_the_stand_alone_check_passes_under_the_sanitizers(check_program):
    out = subprocess.check_output([check_program]).decode()
    assert out.startswith("ok: 4 tables, 16777216 triples, 25 frames, 18 layout widths"), out  # (both layouts x widths 1..9: jello_frame.h)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (5, 4), (4, 5)])
def test_the_programs_frame_is_the_references(check_program, w, h):
    y, cb, cr = load_cases.random_frame(w, h, 30)
    hexes = "".join("%02x" % b for p in (y, cb, cr) for b in p.reshape(-1))
    for layout, chroma, matrix, rng, transfer in ((0, 1, 1, 0, 1), (1, 0, 0, 1, 0), (0, 1, 0, 0, 0)):
        text = subprocess.check_output([check_program] + [str(v) for v in (w, h, layout, chroma, matrix, rng, transfer)] + [hexes]).decode()
        got = np.array([[[int(v, 16) for v in texel.split()] for texel in line.split(" | ")] for line in text.splitlines()], np.uint16)
        assert np.array_equal(got, R.load_yuv((h, w), [y, cb, cr], R.I420, matrix, rng, transfer, chroma))


# ---- the battery ----

YUV_MISSES = [dict(bias=(1 << 19) - 1), dict(truncate=True), dict(clamp_first=True), dict(swap_weights=True), dict(cosited=True), dict(mirror_edge=True)]


@pytest.mark.parametrize("miss", YUV_MISSES, ids=lambda m: next(iter(m)))
def test_the_yuv_battery_tells_the_rule_from_a_near_miss(miss):
    """A wrong variant of the reference differs from the rule on some case of the battery.  (The chroma variants only exist under
    BILINEAR; the others show under every instantiation.)  `clamp_first` is a SUBSTITUTE for the near miss "the clamp before the
    shift": read literally -- the sum clamped to [0, 255 << 20], then rounded and shifted -- that variant gives the rule's codes for
    every input (a sum below 0 still ends at 0, one above 255 << 20 at 255), so no battery can fail it; what is run in its place is
    Y' clamped at 0 before the products, the nearest clamp-too-early that changes a code."""
    chroma_only = next(iter(miss)) in ("swap_weights", "cosited", "mirror_edge")
    for instance in load_cases.YUV_INSTANCES:
        if chroma_only and instance[1] != R.BILINEAR:
            continue
        assert any(not np.array_equal(load_cases.yuv_expected(c), load_cases.yuv_expected(c, **miss)) for c in load_cases.yuv_cases(instance)), instance


def test_the_surface_battery_tells_a_premultiplied_colour_decoded_after_the_division():
    """The near miss only exists under <SRGB, PREMULTIPLIED>, and shows there."""
    for instance in load_cases.SURFACE_INSTANCES:
        differs = any(not np.array_equal(load_cases.surface_expected(c), load_cases.surface_expected(c, decode_after=True))
                      for c in load_cases.surface_cases(instance))
        assert differs == (instance == (True, R.PREMULTIPLIED)), instance


def test_u_as_a_product_with_the_reciprocal_is_another_table_but_no_texel_shows_it():
    """U as c * (1 / 255) differs from the rule's U in binary32 for 126 of the 256 codes, which is why the rule names the quotient.  No
    battery can tell the two apart at the texels, though: over ALL 256 x 256 (code, alpha) pairs, in the three alpha modes and both
    transfers, the f16 results are the same -- the f16 tables agree entry for entry, and under PREMULTIPLIED no product lands on the other
    side of an f16 rounding boundary.  The test states that, so that a change of the store rule or of the formats that makes the
    difference visible is noticed, and the binary32 table is held by test_u_is_the_nearest_binary32_and_the_ieee_quotient."""
    assert int((R.unorm_table() != R.unorm_table(reciprocal=True)).sum()) == 126
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    px = np.stack([c, 255 - c, c ^ 0x5A, a], axis=-1)
    for fmt in (R.RGBA8_UNORM, R.RGBA8_SRGB):
        for alpha in R.ALPHAS:
            assert np.array_equal(R.texels(px, fmt=fmt, alpha=alpha), R.texels(px, fmt=fmt, alpha=alpha, reciprocal=True)), (fmt, alpha)


def test_the_battery_covers_what_it_claims():
    assert len(load_cases.YUV_INSTANCES) == 4 and len(load_cases.SURFACE_INSTANCES) == 6
    for instance in load_cases.YUV_INSTANCES:
        cases = load_cases.yuv_cases(instance)
        assert all(c["instance"] == instance and c["name"].startswith(load_cases.yuv_instance_name(*instance)) for c in cases)
        assert len({c["name"] for c in cases}) == len(cases)
        sizes = {c["y"].shape[::-1] for c in cases}
        assert {(1, 1), (1, 5), (5, 1), (2, 2), (3, 3)} <= sizes and {(w, h) for w in (511, 512, 513, 15, 16, 17, 31, 32, 33) for h in (1, 2, 3)} <= sizes
        assert {(c["matrix"], c["rng"], c["transfer"]) for c in cases} == {(m, r, t) for m in R.MATRICES for r in R.RANGES for t in R.TRANSFERS}
        assert any(c["prior"] == "never" for c in cases) and any(c["rect"] and c["rect"][0] & 1 for c in cases)
        assert any(c["y"].shape[0] > 256 * 8 for c in cases)  # more segments than 8 workgroups on each of 256 CUs
        assert {c["ptr_off"] for c in cases} >= {(0, 0, 0), (1, 1, 1), (2, 2, 2), (8, 8, 8)} and any(any(e & 1 for e in c["pitch_extra"]) for c in cases)
        clamp = [c for c in cases if "extreme chroma" in c["name"]]
        rgb = np.concatenate([R.yuv_codes(load_cases.planes_of(c["y"], c["cb"], c["cr"], c["layout"]), c["layout"], c["matrix"], c["rng"], c["chroma"],
                                          clamp8=False).reshape(-1) for c in clamp])
        assert rgb.min() < 0 and rgb.max() > 255  # (the rule's shifted sums before clamp8: it acts at both ends)
    for instance in load_cases.SURFACE_INSTANCES:
        cases = load_cases.surface_cases(instance)
        assert all(c["instance"] == instance for c in cases) and len({c["name"] for c in cases}) == len(cases)
        assert {c["fmt"] for c in cases} == ({R.RGBA8_SRGB, R.BGRA8_SRGB} if instance[0] else {R.RGBA8_UNORM, R.BGRA8_UNORM})
        assert {c["pixels"].shape[1] for c in cases} >= {1, 2, 3, 511, 512, 513}
        assert any(c["pitch_extra"] for c in cases) and any(c["rect"] and c["rect"][0] & 1 for c in cases) and any(c["rect"] and not c["rect"][0] & 1 for c in cases)
    frame = load_cases.code_frame()
    assert {tuple(p) for p in frame[..., [0, 3]].reshape(-1, 2)} >= {(c, a) for c in range(256) for a in (0, 1, 127, 128, 254, 255)}
    assert (frame[..., :3].max(axis=-1) > frame[..., 3]).any() and ((frame[..., 3] == 0) & (frame[..., :3].max(axis=-1) > 0)).any()
