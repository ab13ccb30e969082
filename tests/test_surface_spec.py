"""CPU: the surface blit's conversion rule (include/jello_hip.h, DESIGN.md "Surface blit") -- the committed sRGB threshold
table against its generator and the binary64 rule, hand values, the Python Surface enum against the header, and the Go
shim's C calls against the declarations of include/jello_hip.h."""
import importlib.util
import os

import numpy as np
import pytest

import surface_ref as ref
from abi_text import c_values, go_calls, header_arity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "jello_amd", "csrc", "srgb_encode_lut.h")
GEN = os.path.join(ROOT, "tools", "gen_srgb_encode_table.py")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_srgb_encode_table", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def table():
    with open(HEADER) as f:
        t = _gen().parse(f.read())
    assert t.shape == (255,) and t.dtype == np.float32
    return t


def lookup(t, v):
    return np.searchsorted(t, np.asarray(v, np.float32), side="right").astype(np.uint8)


def test_committed_table_is_the_generators_output(table):
    g = _gen()
    t = g.thresholds()
    assert np.array_equal(t.view(np.uint32), table.view(np.uint32))
    with open(HEADER) as f:
        assert f.read() == g.render(t)
    assert np.all(np.diff(table) > 0) and table[0] > 0 and table[-1] <= 1


def test_table_agrees_with_the_binary64_rule(table):
    """The 4096 f32 on either side of every threshold and 10^7 seeded random f32 in [0, 1]: the lookup equals the rule.
    (tools/gen_srgb_encode_table.py --verify sweeps every f32 in [0, 1].)"""
    bits = table.view(np.uint32).astype(np.int64)
    near = (bits[:, None] + np.arange(-4096, 4097)[None, :]).ravel()
    near = near[(near >= 0) & (near <= 0x3F800000)].astype(np.uint32).view(np.float32)
    rng = np.random.default_rng(20261016)
    rand = rng.integers(0, 0x3F800001, size=10_000_000, dtype=np.uint32).view(np.float32)
    for v in (near, rand):
        got = lookup(table, v)
        want = ref.srgb8(v)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "v=%r: table %d rule %d" % (float(v[bad[0]]), got[bad[0]], want[bad[0]])


HAND = [  # c, a, p, unorm, sRGB (c and a are f16 values)
    (1.0, 0.5, 0.5, 128, 188),
    (0.5, 0.5, 0.25, 64, 137),
    (1.0, 1.0, 1.0, 255, 255),
    (0.2, 0.7, 0.14000487, 36, 105),
]


@pytest.mark.parametrize("c,a,p,un,sr", HAND)
def test_hand_values(table, c, a, p, un, sr):
    c16, a16 = np.float32(np.float16(c)), np.float32(np.float16(a))
    prod = np.float32(c16 * a16)
    assert abs(float(prod) - p) < 1e-7
    for fmt, want in ((ref.RGBA8_UNORM, un), (ref.RGBA8_SRGB, sr)):
        px = ref.convert_f32(np.array([[c16, c16, c16]]), np.array([a16]), fmt)[0]
        assert list(px[:3]) == [want] * 3
        assert px[3] == ref.unorm8(a16)
    assert ref.unorm8(prod) == un
    assert lookup(table, prod) == sr


def test_specials(table):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for fmt in ref.FORMATS:
        px = ref.convert_f32(np.array([[nan, inf, -inf]], np.float32), np.array([1.0], np.float32), fmt)[0]
        assert list(px) == [0, 255, 0, 255]  # NaN -> 0, +inf -> 1, -inf -> 0 (the same bytes in BGRA order)
        px = ref.convert_f32(np.array([[inf, 0.5, 1.0]], np.float32), np.array([0.0], np.float32), fmt)[0]  # inf * 0 = NaN -> 0
        assert list(px) == [0, 0, 0, 0]
        px = ref.convert_f32(np.array([[1.0, 0.0, 0.25]], np.float32), np.array([nan], np.float32), fmt)[0]
        assert list(px) == [0, 0, 0, 0]
    assert lookup(table, ref.clamp01(nan)) == 0 and lookup(table, ref.clamp01(inf)) == 255
    bgra = ref.convert_f32(np.array([[1.0, 0.5, 0.0]], np.float32), np.array([1.0], np.float32), ref.BGRA8_UNORM)[0]
    assert list(bgra) == [0, 128, 255, 255]


def test_surface_enum_matches_header():
    from jello_amd import Surface
    vals = c_values(["JH_SURFACE_RGBA8_UNORM", "JH_SURFACE_BGRA8_UNORM", "JH_SURFACE_RGBA8_SRGB", "JH_SURFACE_BGRA8_SRGB"])
    assert vals == [Surface.RGBA8_UNORM, Surface.BGRA8_UNORM, Surface.RGBA8_SRGB, Surface.BGRA8_SRGB] == [0, 1, 2, 3]
    assert [s.name for s in Surface] == ["RGBA8_UNORM", "BGRA8_UNORM", "RGBA8_SRGB", "BGRA8_SRGB"]


def test_go_shim_calls_match_the_header():
    decl = header_arity()
    assert decl.get("jh_blit") == 7
    calls = go_calls()
    assert len(calls) > 20
    for name, n in calls:
        assert name in decl, "hip_engine.go calls %s, which include/jello_hip.h does not declare" % name
        assert decl[name] == n, "hip_engine.go calls %s with %d arguments, the header declares %d" % (name, n, decl[name])
    assert "jh_blit" in {n for n, _ in calls}
