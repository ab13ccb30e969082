"""CPU: the tile pack's format (include/jello_hip.h "tile-packed frame transport").  tests/tilepack_ref.py is
written from that text alone; here it is checked against itself (pack -> unpack), against the product's host-side consumer
jello_amd/tilepack.py (which shares no code with it), against hand-built packs, against malformed packs, and against the
tile statistics of two oracle frames.  The answer is exact everywhere: no tolerance."""
import os
import re
import struct

import numpy as np
import pytest

from jello_amd import tilepack

import tilepack_ref as ref
from abi_text import GO, JH, go_calls, header_arity
from tilepack_cases import CASES, DTYPES, SIZES, case_frames, make_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POISON = 0xA7


def test_every_class_occurs_in_the_battery():
    seen = set()
    for w, h, tb, kind in CASES:
        f, r = case_frames(w, h, tb, kind)
        seen |= {(tb, c) for c in ref.classify(f, r)}
    assert seen == {(tb, c) for tb in (4, 8) for c in (ref.SKIP, ref.SOLID, ref.RAW)}


@pytest.mark.parametrize("w,h,tb,kind", CASES)
def test_roundtrip_reference_and_product(w, h, tb, kind):
    """reference pack -> reference unpack and reference pack -> tilepack.apply both reproduce the frame when they start from
    the reference frame (or from poison when there is none), with no rejects; sizes, alignment and padding are as stated."""
    f, r = case_frames(w, h, tb, kind)
    p = ref.pack(f, r)
    classes = ref.classify(f, r)
    n_solid, n_raw = classes.count(ref.SOLID), classes.count(ref.RAW)
    hdr = struct.unpack_from("<8I", p, 0)
    assert hdr == (0x3150544A, w, h, tb, n_solid + n_raw, n_solid, n_raw, 0 if r is None else 1)
    off_solid = 32 + (8 * (n_solid + n_raw) + 15) // 16 * 16
    off_raw = off_solid + (tb * n_solid + 15) // 16 * 16
    assert off_solid % 16 == 0 and off_raw % 16 == 0
    assert len(p) == off_raw + 256 * tb * n_raw == ref.total_size(p)
    assert len(p) <= tilepack.bound(w, h, tb)
    assert not any(p[32 + 8 * (n_solid + n_raw):off_solid]) and not any(p[off_solid + tb * n_solid:off_raw])  # zero padding
    ph = tilepack.parse_header(p)
    assert ph is not None and ph["total_bytes"] == len(p) and ph["solid_offset"] == off_solid and ph["raw_offset"] == off_raw
    assert (ph["n_entries"], ph["n_solid"], ph["n_raw"], ph["flags"]) == hdr[4:]
    # entries ascend, payload indices count up per section
    ks, kr, last = 0, 0, -1
    for e in range(n_solid + n_raw):
        w0, w1 = struct.unpack_from("<II", p, 32 + 8 * e)
        t = w0 & 0x7FFFFFFF
        assert t > last and classes[t] == (ref.RAW if w0 >> 31 else ref.SOLID)
        last = t
        if w0 >> 31:
            assert w1 == kr
            kr += 1
        else:
            assert w1 == ks
            ks += 1
    for apply in (ref.unpack, tilepack.apply):
        out = np.full_like(f, POISON) if r is None else r.copy()
        assert apply(p, out) == 0
        assert np.array_equal(out, f)
    if kind == "equal":
        assert n_solid + n_raw == 0 and len(p) == 32
    if kind == "different":
        assert ref.SKIP not in classes


def test_raw_block_pads_with_zero_outside_the_frame():
    f = np.arange(17 * 3 * 4, dtype=np.uint8).reshape(3, 17, 4) | 1  # 2 tiles: 16 x 3 and 1 x 3 texels in the frame
    p = ref.pack(f)
    assert struct.unpack_from("<8I", p, 0)[4:7] == (2, 0, 2)
    blocks = np.frombuffer(p, np.uint8, offset=32 + 16).reshape(2, 16, 16, 4)
    assert np.array_equal(blocks[0, :3], f[:, :16]) and not blocks[0, 3:].any()
    assert np.array_equal(blocks[1, :3, :1], f[:, 16:]) and not blocks[1, :3, 1:].any() and not blocks[1, 3:].any()


def test_texels_are_bit_patterns():
    """-0 and +0, and two NaNs, are different texels; equal NaNs are equal."""
    f = np.zeros((16, 16, 4), np.uint16)
    f[...] = 0x7E00  # a NaN in every channel: one colour
    assert ref.classify(f) == [ref.SOLID]
    f[5, 5, 0] = 0x7E01  # another NaN
    assert ref.classify(f) == [ref.RAW]
    z = np.zeros((16, 16, 4), np.uint16)
    m = z.copy()
    m[0, 0, 2] = 0x8000  # -0
    assert ref.classify(m, z) == [ref.RAW] and ref.classify(z, z) == [ref.SKIP]


def test_bound():
    for (w, h) in SIZES + [(4096, 4096), (15, 4097)]:
        for tb in (4, 8):
            n = ((w + 15) // 16) * ((h + 15) // 16)
            assert tilepack.bound(w, h, tb) == 32 + (8 * n + 15) // 16 * 16 + 256 * tb * n
            noise = np.random.default_rng(3).integers(0, 256, size=(min(h, 64), min(w, 64), 4)).astype(DTYPES[tb])
            assert len(ref.pack(noise)) <= tilepack.bound(noise.shape[1], noise.shape[0], tb)
    assert tilepack.bound(16, 16, 3) == 0 and tilepack.bound(16, 16, 16) == 0
    # an all-RAW frame reaches the bound exactly
    noise = np.random.default_rng(4).integers(0, 256, size=(40, 250, 4), dtype=np.uint8)
    assert all(c == ref.RAW for c in ref.classify(noise)) and len(ref.pack(noise)) == tilepack.bound(250, 40, 4)


def _guarded(shape, dtype):
    """An array view with a guard band of POISON rows and columns around it."""
    h, w = shape
    big = np.full((h + 8, w + 8, 4), POISON, dtype)
    return big, big[4:4 + h, 4:4 + w]


def _set_entry(p, e, word0=None, word1=None):
    b = bytearray(p)
    w0, w1 = struct.unpack_from("<II", b, 32 + 8 * e)
    struct.pack_into("<II", b, 32 + 8 * e, w0 if word0 is None else word0, w1 if word1 is None else word1)
    return bytes(b)


@pytest.mark.parametrize("tb", [4, 8])
def test_malformed_packs_are_rejected_entry_by_entry(tb):
    w, h = 50, 40  # 4 x 3 tiles
    f = make_frame(w, h, tb, 99)
    p = ref.pack(f)
    n_entries, n_solid, n_raw = struct.unpack_from("<8I", p, 0)[4:7]
    assert n_entries == 12 and n_solid >= 2 and n_raw >= 2
    first_raw = next(e for e in range(12) if struct.unpack_from("<I", p, 32 + 8 * e)[0] >> 31)
    first_solid = next(e for e in range(12) if not struct.unpack_from("<I", p, 32 + 8 * e)[0] >> 31)
    raw_flag = 1 << 31
    entry_cases = {
        "tile index = tile count": _set_entry(p, first_solid, word0=12),
        "raw tile index far out of range": _set_entry(p, first_raw, word0=raw_flag | 0x7FFFFFFF),
        "solid payload index = n_solid": _set_entry(p, first_solid, word1=n_solid),
        "raw payload index = n_raw": _set_entry(p, first_raw, word1=n_raw),
        "raw payload index huge": _set_entry(p, first_raw, word1=0xFFFFFFFF),
    }
    for what, bad in entry_cases.items():
        e_bad = first_solid if "solid" in what or what.startswith("tile") else first_raw
        t_bad = struct.unpack_from("<I", p, 32 + 8 * e_bad)[0] & 0x7FFFFFFF
        for apply in (ref.unpack, tilepack.apply):
            big, view = _guarded((h, w), DTYPES[tb])
            assert apply(bad, view) == 1, what
            want = f.copy()
            want[16 * (t_bad // 4):16 * (t_bad // 4) + 16, 16 * (t_bad % 4):16 * (t_bad % 4) + 16] = POISON  # only that tile is missing
            assert np.array_equal(view, want), what
            view[...] = POISON
            assert (big == POISON).all(), what  # nothing outside the frame
    def hdr(i, v):
        b = bytearray(p)
        struct.pack_into("<I", b, 4 * i, v)
        return bytes(b)
    header_cases = {
        "truncated inside the raw section": p[:-1],
        "truncated to the header": p[:32],
        "shorter than a header": p[:31],
        "empty": b"",
        "magic": hdr(0, 0x3150544B),
        "width": hdr(1, w + 1),
        "height": hdr(2, h - 1),
        "texel size": hdr(3, 12 - tb),
        "n_entries != n_solid + n_raw": hdr(4, n_entries + 1),
        "n_raw beyond the bytes": hdr(6, n_raw + 1),
        "counts beyond the tile count": hdr(5, 0x7FFFFFF0),
    }
    for what, bad in header_cases.items():
        for apply in (ref.unpack, tilepack.apply):
            big, view = _guarded((h, w), DTYPES[tb])
            assert apply(bad, view) == 1, what
            assert (big == POISON).all(), what


def test_apply_refuses_arrays_it_cannot_address():
    with pytest.raises(ValueError):
        tilepack.apply(ref.pack(np.zeros((4, 4, 4), np.uint8)), np.zeros((4, 4, 4), np.float32))
    with pytest.raises(ValueError):
        tilepack.apply(ref.pack(np.zeros((4, 4, 4), np.uint8)), np.zeros((4, 4, 3), np.uint8))


def _oracle_rgba8(scene, params):
    import jello_amd
    from oracle.oracle_engine import OracleEngine
    import surface_ref
    rec = jello_amd.Host().record(scene, params)
    orc = OracleEngine()
    orc.run(rec)
    return surface_ref.convert(np.asarray(orc.target(rec)).copy(), 0)


def test_tile_statistics_of_oracle_frames(built):
    """The counts the format was designed on: scene_c1 at 512 x 512 has 928 one-colour tiles and 96 others; scene_large_shapes
    at 1536 x 1536 with 61 shapes against the frame with 60 has 146 changed tiles, none of them one colour, and 9 070 unchanged."""
    from jello_amd import scenes
    c1 = _oracle_rgba8(*scenes.scene_c1())
    cls = ref.classify(c1)
    assert (len(cls), cls.count(ref.SOLID), cls.count(ref.RAW)) == (1024, 928, 96)
    assert len(ref.pack(c1)) == 32 + 8 * 1024 + 4 * 928 + 1024 * 96
    a = _oracle_rgba8(*scenes.scene_large_shapes(1536, 60))
    b = _oracle_rgba8(*scenes.scene_large_shapes(1536, 61))
    cls = ref.classify(b, a)
    assert (len(cls), cls.count(ref.SOLID), cls.count(ref.RAW), cls.count(ref.SKIP)) == (9216, 0, 146, 9070)
    p = ref.pack(b, a)
    assert abs(len(p) / b.nbytes - 0.016) < 0.0005  # (the ratio the issue's table states, to its precision)
    out = a.copy()
    assert tilepack.apply(p, out) == 0 and np.array_equal(out, b)


# ---- the Go shim against the header ----
def test_go_shim_calls_pack_and_unpack_as_declared():
    decl = header_arity()
    assert decl.get("jh_pack_tiles") == 10 and decl.get("jh_unpack_tiles") == 8 and decl.get("jh_pack_bound") == 3
    calls = go_calls()
    by_name = {}
    for name, n in calls:
        by_name.setdefault(name, set()).add(n)
    assert by_name.get("jh_pack_tiles") == {10}
    assert by_name.get("jh_unpack_tiles") == {8}
    for name, n in calls:
        assert name in decl and decl[name] == n, (name, n)
    with open(GO) as f:
        text = f.read()
    for fn in ("PackTiles", "UnpackTiles", "ReadPack"):
        assert re.search(r"func \(e \*Engine\) %s\(" % fn, text), fn


def test_format_text_agrees_in_header_design_and_reference():
    """The three statements of the format name the same magic, tile size, section order and alignment."""
    with open(JH) as f:
        header = f.read()
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert "Tile pack: the format" in design
    for text in (header, design, ref.__doc__):
        flat = " ".join(text.replace(" * ", " ").split()).lower()
        for needle in ("0x3150544a", "16 x 16", "n_entries", "n_solid", "n_raw", "next multiple of 16", "word0", "word1"):
            assert needle in flat, needle
    assert ref.MAGIC == tilepack.MAGIC == 0x3150544A == struct.unpack("<I", b"JTP1")[0]
