"""The turbulence rule on the CPU: the generator's published check value, the tables and the plan of the library
(jh_turbulence_tables, jh_turbulence_plan) and of the host twin (jl_...) against the reference's bit for bit, the ctypes mirrors'
layout, the legality boundaries from both sides, lattice points, 0 octaves, texels worked by hand, the rule's host half
(include/jello_turbulence.h through tools/turbulence_check.cpp) against the reference bit for bit, the reference
(tests/turbulence_ref.py) against a binary64 transcription of the specification's algorithm within the bound DESIGN derives, the
stitch periodicity bound, the stand-alone check, and the sensitivity of the battery (tests/turbulence_cases.py) to every near miss of
the rule."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import TurbulenceKind, _lib

import turbulence_cases
import turbulence_ref
from abi_text import INCLUDE, ROOT, c_values
from turbulence_ref import FRACTAL_NOISE, TURBULENCE

F = np.float32
U = 2.0 ** -24  # the unit roundoff of binary32
LIPSCHITZ = 5.25  # |dn/dx| <= 1 + 1.5 * 2 sqrt 2


def as_f64(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def ulp16(v):
    """The spacing of f16 at |v| (float64 array), 2^-24 below the normal range."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 10)


# ---- the generator and the tables ----

def test_the_generators_published_check_value():
    s = 1
    for _ in range(10000):
        s = turbulence_ref.random(s)
    assert s == 1043618065
    assert [turbulence_ref.setup_seed(s) for s in (0, 1, -1, 5, 2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31, -(2 ** 31 - 2), -(2 ** 31 - 3))] == \
        [1, 1, 2, 5, 2 ** 31 - 2, 2 ** 31 - 2, 3, 1, 2 ** 31 - 2]


def _spec_tables(seed):
    """The specification's init transcribed: uLatticeSelector and fGradient with their duplicated upper halves, in binary64."""
    s = turbulence_ref.setup_seed(seed)
    lattice, gradient = [0] * 514, np.zeros((4, 514, 2))
    for k in range(4):
        for i in range(256):
            lattice[i] = i
            for j in range(2):
                s = turbulence_ref.random(s)
                gradient[k, i, j] = ((s % 512) - 256) / 256.0
            length = math.sqrt(gradient[k, i, 0] * gradient[k, i, 0] + gradient[k, i, 1] * gradient[k, i, 1])
            if length != 0.0:  # (0 / 0 in the specification's code; the rule keeps +0)
                gradient[k, i] /= length
    i = 256
    while True:
        i -= 1
        if not i:
            break
        s = turbulence_ref.random(s)
        j = s % 256
        lattice[i], lattice[j] = lattice[j], lattice[i]
    for i in range(258):
        lattice[256 + i] = lattice[i]
        gradient[:, 256 + i] = gradient[:, i]
    return lattice, gradient


SEEDS = turbulence_cases.SEEDS + (-2 ** 31, 7, 123456789)


@pytest.mark.parametrize("twin", [False, True], ids=["library", "host twin"])
def test_tables_equal_the_reference_bit_for_bit(built, twin):
    for seed in SEEDS:
        P, G = jello_amd.turbulence_tables(twin=twin, seed=seed)
        rp, rg, _ = turbulence_ref.tables(seed)
        assert np.array_equal(P, rp), seed
        assert np.array_equal(G.view(np.uint32), rg.view(np.uint32)), seed
        lattice, gradient = _spec_tables(seed)
        assert list(P) == lattice[:256] and np.array_equal(G, gradient[:, :256].astype(F))


def test_tables_are_a_permutation_and_unit_gradients():
    for seed in SEEDS:
        P, G, key = turbulence_ref.tables(seed)
        assert sorted(P) == list(range(256)) and key == turbulence_ref.setup_seed(seed)
        g = G.astype(np.float64)
        length = np.hypot(g[..., 0], g[..., 1])
        zero = (G.view(np.uint32) == 0).all(axis=2)  # (+0, +0)
        assert np.all(zero | (np.abs(length - 1.0) <= 2.0 ** -23)), seed
        assert zero.sum() == (1 if seed == turbulence_cases.SEED_WITH_A_ZERO_GRADIENT else 0)
    _, G, _ = turbulence_ref.tables(turbulence_cases.SEED_WITH_A_ZERO_GRADIENT)
    assert not G[1, 164].any()


def test_the_masked_lookup_is_the_duplicated_tables_lookup():
    lattice, gradient = _spec_tables(12)
    P = np.array(lattice[:256])
    for bx0 in range(0, 256, 3):
        by0 = np.arange(256)
        i, j = lattice[bx0], lattice[(bx0 + 1) & 255]
        for first in (i, j):
            for by in (by0, (by0 + 1) & 255):
                assert np.array_equal(np.array(lattice)[first + by], P[(first + by) & 255])


# ---- the plan ----

PLANS = [
    dict(base_frequency=(0.05, 0.03), octaves=4, seed=3),
    dict(base_frequency=(0.0, 7.3), octaves=1, seed=-5, origin=(-1000.25, 1e6)),
    dict(base_frequency=(0.1, 0.1), octaves=16, seed=0, origin=(0.1, -0.7)),
    dict(base_frequency=(0.047, 0.043), octaves=5, seed=1, stitch_tile=(10.0, -30.0, 100.0, 64.0)),
    dict(base_frequency=(0.004, 0.5), octaves=3, seed=1, stitch_tile=(0.0, -30.5, 100.0, 64.0), origin=(-3.0, 2.5)),
    dict(base_frequency=(1.5, 0.0), octaves=0, seed=2 ** 31 - 1, stitch_tile=(-7.0, 0.0, 3.0, 5.0)),
    dict(base_frequency=(1.0 / 3.0, 2.0 / 7.0), octaves=8, seed=9, origin=(1.0 / 3.0, -2.0 / 7.0)),
    dict(base_frequency=(0.3, 0.3), octaves=2, seed=9, origin=(0.5, 1.5)),  # (ties of the rounding are even)
]


@pytest.mark.parametrize("twin", [False, True], ids=["library", "host twin"])
def test_plan_equals_the_reference_bit_for_bit(built, twin):
    for d in PLANS:
        got, want = jello_amd.turbulence_plan(twin=twin, **d), turbulence_ref.plan(**d)
        for k in ("frequency", "step", "start", "wrap", "width", "max_extent"):
            assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, (d, k, got[k], want[k])
        assert (got["key"], got["stitched"]) == (want["key"], want["stitched"])
    p = turbulence_ref.plan(**PLANS[3])
    assert list(p["frequency"]) == [0.05, 0.046875] and list(p["width"]) == [5, 3] and list(p["wrap"]) == [5, -2 + 3]  # hi on both axes; floor(-30 x 0.046875) = -2
    p = turbulence_ref.plan(**PLANS[4])
    assert list(p["frequency"]) == [0.01, 0.5] and list(p["width"]) == [1, 32] and list(p["wrap"]) == [1, 16]  # a tile smaller than a cell
    p = turbulence_ref.plan(base_frequency=(2.0 ** -33, 3 * 2.0 ** -33))
    assert list(p["step"]) == [0, 2] and list(p["start"]) == [0, 1]  # ties to even: 0.5 -> 0, 1.5 -> 2; the starts are 0.25 and 0.75
    assert int(turbulence_ref.plan(base_frequency=(5 * 2.0 ** -33, 0.0))["step"][0]) == 2  # 2.5 -> 2


def _legal(twin, **d):
    """Whether the library (or the twin) and the reference accept the descriptor: they have to agree."""
    try:
        jello_amd.turbulence_plan(twin=twin, **d)
        lib = True
    except ValueError:
        lib = False
    try:
        turbulence_ref.plan(**{k: v for k, v in d.items() if k != "rect"})
        ref = True
    except ValueError:
        ref = False
    assert lib == ref, d
    return lib


@pytest.mark.parametrize("twin", [False, True], ids=["library", "host twin"])
def test_legality_boundaries(built, twin):
    nan, inf = math.nan, math.inf
    ok = lambda **d: _legal(twin, **d)  # noqa: E731
    assert ok(base_frequency=0.1) and ok(base_frequency=0.0) and ok(base_frequency=-0.0)
    assert not ok(base_frequency=(0.1, -5e-324)) and not ok(base_frequency=nan) and not ok(base_frequency=inf)
    assert ok(base_frequency=0.1, octaves=16) and not ok(base_frequency=0.1, octaves=17) and ok(base_frequency=0.1, octaves=0)
    assert ok(base_frequency=0.1, kind=0) and not ok(base_frequency=0.1, kind=2) and not ok(base_frequency=0.1, kind=-1)
    assert not ok(base_frequency=0.1, origin=(nan, 0.0)) and not ok(base_frequency=0.1, origin=(0.0, inf))
    # the frequency: f 2^32 below 2^62
    assert not ok(base_frequency=2.0 ** 30, origin=(-0.5, -0.5)) and ok(base_frequency=float(np.nextafter(2.0 ** 30, 0.0)), origin=(-0.5, -0.5))
    # the origin: |start| <= (2^62 - 1) >> (octaves - 1)
    for octaves, cells in ((0, 2.0 ** 30), (1, 2.0 ** 30), (2, 2.0 ** 29), (16, 2.0 ** 15)):
        assert not ok(base_frequency=1.0, octaves=octaves, origin=(cells - 0.5, 0.0))
        assert ok(base_frequency=1.0, octaves=octaves, origin=(cells - 0.75, 0.0))
        assert not ok(base_frequency=1.0, octaves=octaves, origin=(0.0, -cells - 0.5))
        assert ok(base_frequency=1.0, octaves=octaves, origin=(0.0, -cells - 0.25))
    # max_extent: the last extent inside the range
    p = jello_amd.turbulence_plan(twin=twin, base_frequency=(1.0, 0.0), octaves=16, origin=(32000.0, 0.0))
    assert list(p["max_extent"]) == [768, 0xFFFFFFFF]
    p = jello_amd.turbulence_plan(twin=twin, base_frequency=(0.5, 0.25), octaves=16, origin=(-40000.0, 100000.0))
    assert list(p["max_extent"]) == [40000 + 65536, 131072 - 100000]
    # the stitch tile
    tile = lambda *t: dict(base_frequency=1.0, stitch_tile=t)  # noqa: E731
    assert ok(**tile(0.0, 0.0, 8.0, 8.0)) and not ok(**tile(0.0, 0.0, 0.0, 8.0)) and not ok(**tile(0.0, 0.0, 8.0, -1.0)) and ok(**tile(0.0, 0.0, 8.0, 0.5))
    assert not ok(**tile(nan, 0.0, 8.0, 8.0)) and not ok(**tile(0.0, 0.0, inf, 8.0))
    assert ok(octaves=1, **tile(0.0, 0.0, 2147483647.0, 4.0)) and not ok(octaves=1, **tile(0.0, 0.0, 2147483648.0, 4.0))
    assert ok(octaves=16, **tile(0.0, 0.0, 65535.0, 4.0)) and not ok(octaves=16, **tile(0.0, 0.0, 65536.0, 4.0))
    assert ok(octaves=16, **tile(65000.0, 0.0, 535.0, 4.0)) and not ok(octaves=16, **tile(65000.0, 0.0, 536.0, 4.0))
    assert ok(octaves=16, **tile(-65539.0, 0.0, 4.0, 4.0)) and not ok(octaves=16, **tile(-65540.0, 0.0, 4.0, 4.0))
    assert not ok(octaves=1, **tile(2.0 ** 31, 0.0, 4.0, 4.0)) and not ok(octaves=1, **tile(-2.0 ** 31 - 1.0, 0.0, 4.0, 4.0))


# ---- the C ABI ----

def test_ctypes_mirrors_have_the_headers_layout():
    for mirror, struct in ((_lib.CTurbulenceDesc, "jh_turbulence_desc"), (_lib.CTurbPlan, "jh_turb_plan")):
        fields = [name for name, _ in mirror._fields_]
        want = c_values(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, f) for f in fields])
        assert [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, struct
    assert [n for n, _ in _lib.CTurbulenceDesc._fields_] == ["kind", "octaves", "seed", "stitch", "x", "y", "width", "height", "base_frequency", "tile", "origin"]
    assert [n for n, _ in _lib.CTurbPlan._fields_] == ["frequency", "step", "start", "wrap", "width", "max_extent", "key", "stitched"]


def test_enums_and_limits_match_the_header():
    assert c_values(["JH_TURBULENCE_" + k.name for k in TurbulenceKind]) == [int(k) for k in TurbulenceKind] == [0, 1]
    assert c_values(["JH_TURBULENCE_MAX_OCTAVES"]) == [16] == [jello_amd.engine.TURBULENCE_MAX_OCTAVES] == [turbulence_ref.MAX_OCTAVES]
    assert (FRACTAL_NOISE, TURBULENCE) == (0, 1)


# ---- consequences of the rule ----

def test_noise_is_exactly_zero_on_lattice_points():
    """origin -0.5 puts the texel centres on integers; with frequencies 1 and 0.25 every fourth (or every) texel is a lattice point
    in every octave: n = 0 there, so FRACTAL_NOISE stores 0.5 and TURBULENCE 0 -- whatever the seed, stitched or not."""
    for seed in (0, 5, turbulence_cases.SEED_WITH_A_ZERO_GRADIENT):
        for tile in (None, (0.0, 0.0, 8.0, 8.0)):
            for kind, bits in ((FRACTAL_NOISE, 0x3800), (TURBULENCE, 0)):
                kw = dict(kind=kind, octaves=5, seed=seed, origin=(-0.5, -0.5), stitch_tile=tile)
                assert np.all(turbulence_ref.turbulence((9, 13), base_frequency=(1.0, 1.0), **kw) == bits)
                quarter = turbulence_ref.turbulence((9, 13), base_frequency=(0.25, 0.25), **kw)
                assert np.all(quarter[::4, ::4] == bits) and np.any(quarter != bits)
                assert np.all(turbulence_ref.turbulence((9, 13), base_frequency=(0.25, 0.25), **dict(kw, origin=(-4.5, 7.5)))[::4, ::4] == bits)


def test_zero_octaves():
    assert np.all(turbulence_ref.turbulence((5, 7), kind=FRACTAL_NOISE, octaves=0, base_frequency=0.3) == 0x3800)
    assert not turbulence_ref.turbulence((5, 7), kind=TURBULENCE, octaves=0, base_frequency=0.3).any()
    held = np.full((5, 7, 4), 0x1234, np.uint16)
    out = turbulence_ref.turbulence((5, 7), (1, 1, 2, 3), held, kind=FRACTAL_NOISE, octaves=0, base_frequency=0.3)
    assert np.all(out[1:4, 1:3] == 0x3800) and (out == 0x1234).sum() == (35 - 6) * 4


def test_zero_frequency_is_constant_along_its_axis():
    out = turbulence_ref.turbulence((6, 9), base_frequency=(0.0, 0.13), octaves=3, seed=4)
    assert np.all(out == out[:, :1]) and len(np.unique(out[..., 0])) > 3
    both = turbulence_ref.turbulence((6, 9), base_frequency=(0.0, 0.0), octaves=3, seed=4, kind=FRACTAL_NOISE)
    assert np.all(both == 0x3800)  # position 0 is a lattice point


def _by_hand(P, G, X, Y, kind, seed_free_ratio=1.0):
    """One octave at frequency 1, origin 0: texel (X, Y) sits at (X + 0.5, Y + 0.5), so rx0 = ry0 = 0.5, sx = sy = (0.25)(2) = 0.5,
    and lerp(0.5, a, b) = fmaf(0.5, b - a, a).  Scalar binary32 arithmetic, written out."""
    P = [int(v) for v in P]
    i, j = P[X & 255], P[(X + 1) & 255]
    b00, b10, b01, b11 = P[(i + Y) & 255], P[(j + Y) & 255], P[(i + Y + 1) & 255], P[(j + Y + 1) & 255]
    h = F(0.5)
    out = []
    for c in range(4):
        dot = lambda rx, ry, g: F(F(ry * g[1]) + F(rx * g[0]))  # noqa: E731 (0.5 g is exact, so the fmaf is one rounded sum)
        u00, u10, u01, u11 = dot(h, h, G[c][b00]), dot(-h, h, G[c][b10]), dot(h, -h, G[c][b01]), dot(-h, -h, G[c][b11])
        lerp = lambda a, b: F(F(h * F(b - a)) + a)  # noqa: E731 (0.5 (b - a) is exact)
        n = lerp(lerp(u00, u10), lerp(u01, u11))
        v = F(n * h + h) if kind == FRACTAL_NOISE else abs(n)
        out.append(min(max(v, F(0.0)), F(1.0)))
    return np.array(out, F).astype(np.float16).view(np.uint16)


def test_texels_worked_by_hand():
    """(n + 1) / 2 = fmaf(n, 0.5, 0.5): 0.5 n is exact, so one rounded sum as well."""
    for seed in (1, 77):
        P, G, _ = turbulence_ref.tables(seed)
        for kind in (FRACTAL_NOISE, TURBULENCE):
            out = turbulence_ref.turbulence((4, 6), kind=kind, octaves=1, seed=seed, base_frequency=(1.0, 1.0))
            for (X, Y) in ((0, 0), (5, 3), (2, 1)):
                assert np.array_equal(out[Y, X], _by_hand(P, G, X, Y, kind)), (seed, kind, X, Y)
            far = turbulence_ref.turbulence((2, 2), kind=kind, octaves=1, seed=seed, base_frequency=(1.0, 1.0), origin=(-300.0, 515.0))
            assert np.array_equal(far[1, 1], _by_hand(P, G, -299, 516, kind))  # (negative cells floor; the lattice repeats every 256)


# ---- the rule's host half, through the stand-alone program ----

@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("turb") / "turbulence_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", INCLUDE, os.path.join(ROOT, "tools", "turbulence_check.cpp"), "-o", exe])
    return exe


def test_the_stand_alone_check_builds_and_passes(check_exe):
    """tools/turbulence_check.cpp is include/jello_turbulence.h with a main of its own: the generator against 64-bit arithmetic, P a
    permutation, the plan against __int128, legality from both sides, the masked lookup against the duplicated tables.  Its header has
    the command with the sanitizers; here it is built without them and run."""
    assert subprocess.check_output([check_exe]).decode() == "ok\n"


@pytest.mark.parametrize("kind", [FRACTAL_NOISE, TURBULENCE])
def test_the_headers_texels_equal_the_reference_bit_for_bit(check_exe, kind):
    """jturb_texel -- the split, the stitch step, the lattice walk, the s-curve, the dot and the lerp the kernel compiles too -- on the
    CPU, binary32 before the rounding to f16."""
    for f, tile, origin, octaves in (((0.05, 0.03), None, (0.0, 0.0), 4), ((0.25, 1.0), None, (-7.5, 3.25), 5), ((1.5, 7.3), None, (-100.0, 1e3), 16),
                                     ((0.047, 0.11), (3.0, -5.0, 40.0, 30.0), (-20.0, -11.5), 5), ((0.004, 0.3), (0.0, 0.0, 100.0, 64.0), (0.0, 0.0), 3)):
        for seed in (0, -2000000000, turbulence_cases.SEED_WITH_A_ZERO_GRADIENT):
            t = tile or (0.0, 0.0, 1.0, 1.0)
            args = [kind, octaves, seed, int(tile is not None), repr(f[0]), repr(f[1])] + [repr(c) for c in t] + [repr(origin[0]), repr(origin[1]), 3, 2, 41, 9]
            out = subprocess.check_output([check_exe, "texels"] + [str(a) for a in args]).decode().split()
            got = np.array([int(x, 16) for x in out], np.uint32).reshape(9, 41, 4)
            want = turbulence_ref.values(np.arange(3, 44), np.arange(2, 11), kind=kind, octaves=octaves, seed=seed, base_frequency=f, stitch_tile=tile, origin=origin)
            assert np.array_equal(got, want.view(np.uint32)), (f, tile, seed)


# ---- the reference against the specification in binary64 ----

def _spec64(X, Y, kind, octaves, seed, base_frequency, origin=(0.0, 0.0), stitch_tile=None):
    """The specification's turbulence() and noise2(), transcribed in binary64 with floating positions: the point is (origin + X + 0.5),
    vec = point * frequency, doubled per octave; floor for the cell (the specification adds 4096 and truncates); the stitch comparison
    before the mask; the duplicated tables, no mask after the first level."""
    lattice, gradient = _spec_tables(seed)
    lattice = np.array(lattice)
    fx, fy = base_frequency
    wrap = width = None
    if stitch_tile is not None:
        tx, ty, tw, th = stitch_tile
        f = []
        for freq, extent in ((fx, tw), (fy, th)):
            if freq != 0.0:
                lo, hi = math.floor(extent * freq) / extent, math.ceil(extent * freq) / extent
                freq = lo if (lo != 0.0 and freq / lo < hi / freq) else hi
            f.append(freq)
        fx, fy = f
        width = [int(tw * fx + 0.5), int(th * fy + 0.5)]
        wrap = [math.floor(tx * fx) + width[0], math.floor(ty * fy) + width[1]]
    vx, vy = (origin[0] + np.asarray(X, np.float64) + 0.5) * fx, (origin[1] + np.asarray(Y, np.float64) + 0.5) * fy
    total, ratio = np.zeros((len(Y), len(X), 4)), 1.0
    for _ in range(octaves):
        cx, cy = np.floor(vx), np.floor(vy)
        rx0, ry0 = (vx - cx)[None, :], (vy - cy)[:, None]
        bx0, by0 = cx.astype(np.int64), cy.astype(np.int64)
        bx1, by1 = bx0 + 1, by0 + 1
        if wrap is not None:
            bx0, bx1 = np.where(bx0 >= wrap[0], bx0 - width[0], bx0), np.where(bx1 >= wrap[0], bx1 - width[0], bx1)
            by0, by1 = np.where(by0 >= wrap[1], by0 - width[1], by0), np.where(by1 >= wrap[1], by1 - width[1], by1)
        bx0, bx1, by0, by1 = bx0 & 255, bx1 & 255, by0 & 255, by1 & 255
        i, j = lattice[bx0][None, :], lattice[bx1][None, :]
        b00, b10, b01, b11 = lattice[i + by0[:, None]], lattice[j + by0[:, None]], lattice[i + by1[:, None]], lattice[j + by1[:, None]]
        sx, sy = rx0 * rx0 * (3.0 - 2.0 * rx0), ry0 * ry0 * (3.0 - 2.0 * ry0)
        for c in range(4):
            g = gradient[c]
            u = rx0 * g[b00][..., 0] + ry0 * g[b00][..., 1]
            v = (rx0 - 1.0) * g[b10][..., 0] + ry0 * g[b10][..., 1]
            a = u + sx * (v - u)
            u = rx0 * g[b01][..., 0] + (ry0 - 1.0) * g[b01][..., 1]
            v = (rx0 - 1.0) * g[b11][..., 0] + (ry0 - 1.0) * g[b11][..., 1]
            b = u + sx * (v - u)
            n = a + sy * (b - a)
            total[..., c] += (np.abs(n) if kind == TURBULENCE else n) / ratio
        vx, vy, ratio = vx * 2.0, vy * 2.0, ratio * 2.0
        if wrap is not None:
            wrap, width = [2 * w for w in wrap], [2 * w for w in width]
    out = (total + 1.0) / 2.0 if kind == FRACTAL_NOISE else total
    return np.clip(out, 0.0, 1.0)


def rule_bound(extent, octaves):
    """DESIGN.md 5.15, "How far the rule is from the specification", for positions up to 2^20 cells: the f16 rounding, the position
    (the quantised step over `extent` texels, the start, the binary64 product: (extent + 2) 2^-33 cell, doubled per octave against
    the halved ratio; the 24-bit fraction: 2^-24 per octave) through the noise's Lipschitz constant on both axes, and the binary32
    operations."""
    return 2.0 ** -12 + 2.0 * LIPSCHITZ * (octaves * (extent + 2) * 2.0 ** -33 + 2.0 ** -23) + (40 + 2 * octaves) * U


@pytest.mark.parametrize("kind", [FRACTAL_NOISE, TURBULENCE])
@pytest.mark.parametrize("seed", [0, 31, -9])
def test_the_reference_is_the_specification_within_the_derived_bound(kind, seed):
    W, H = 97, 41
    X, Y = np.arange(W), np.arange(H)
    for f, origin, octaves, tile in (((0.013, 0.021), (0.0, 0.0), 8, None), ((0.31, 0.17), (-55.25, 1000.125), 5, None), ((1.5, 7.3), (12.0, -3.0), 3, None),
                                     ((0.01, 0.01), (0.0, 0.0), 16, None), ((0.047, 0.11), (-20.0, -11.5), 6, (3.0, -5.0, 40.0, 30.0)),
                                     ((0.25, 1.0), (-0.5, -0.5), 4, None)):
        kw = dict(kind=kind, octaves=octaves, seed=seed, base_frequency=f, origin=origin, stitch_tile=tile)
        got = as_f64(turbulence_ref.turbulence((H, W), **kw))
        want = _spec64(X, Y, **kw)
        err = np.abs(got - want).max()
        assert err <= rule_bound(max(W, H), octaves), (kw, err)
        # ... and the binary32 values before the store are far inside the f16 term
        raw = np.abs(turbulence_ref.values(X, Y, **kw).astype(np.float64) - want).max()
        assert raw <= rule_bound(max(W, H), octaves) - 2.0 ** -12, (kw, raw)
        assert want.std() > 0.01 or f == (0.25, 1.0)


def stitch_bound(tile_extent, octaves):
    """DESIGN.md 5.15, "Stitched tiles": what the values BEFORE the store at x and x + tile_w can differ by -- the step's rounding over
    the tile, tile_w 2^-33 cell, doubled per octave against the halved ratio, the 24-bit fraction, the binary32 operations of both
    evaluations; the stored values differ by that plus one f16 ULP."""
    return LIPSCHITZ * (octaves * (tile_extent + 1) * 2.0 ** -33 + 2.0 ** -23) + 2 * (40 + 2 * octaves) * U


@pytest.mark.parametrize("kind", [FRACTAL_NOISE, TURBULENCE])
def test_a_stitched_tile_meets_itself_at_its_edges(kind):
    """Texel centres on integers (origin -0.5): the columns tile_x .. tile_x + 3 against the columns one tile width further, on every
    row, and the rows likewise -- within the derived bound plus one f16 ULP; without stitch the same pairs differ by far more, so the
    test can fail."""
    tile = (16.0, 8.0, 100.0, 60.0)
    kw = dict(kind=kind, octaves=4, seed=6, base_frequency=(0.047, 0.06), origin=(-0.5, -0.5))
    X, Y = np.arange(0, 124), np.arange(0, 76)
    for stitched in (True, False):
        v = turbulence_ref.values(X, Y, stitch_tile=tile if stitched else None, **kw).astype(np.float64)
        stored = as_f64(turbulence_ref.turbulence((76, 124), stitch_tile=tile if stitched else None, **kw))
        dx, dy = np.abs(v[:, 16:20] - v[:, 116:120]), np.abs(v[8:12] - v[68:72])
        sx, sy = np.abs(stored[:, 16:20] - stored[:, 116:120]), np.abs(stored[8:12] - stored[68:72])
        ux, uy = np.maximum(ulp16(stored[:, 16:20]), ulp16(stored[:, 116:120])), np.maximum(ulp16(stored[8:12]), ulp16(stored[68:72]))
        bx, by = stitch_bound(100, 4), stitch_bound(60, 4)
        if stitched:
            assert dx.max() <= bx and dy.max() <= by, (dx.max(), dy.max(), bx, by)
            assert np.all(sx <= bx + ux) and np.all(sy <= by + uy)
        else:
            assert dx.max() > 100 * bx and dy.max() > 100 * by
            assert np.any(sx > bx + ux) and np.any(sy > by + uy)


def test_the_zero_gradient_of_the_searched_seed_is_used():
    """The battery's cases with SEED_WITH_A_ZERO_GRADIENT do read G[1][164]: with that entry replaced their green channel changes."""
    seed = turbulence_cases.SEED_WITH_A_ZERO_GRADIENT
    real = turbulence_ref.tables

    def patched(s):
        P, G, key = real(s)
        G = G.copy()
        G[1, 164] = (1.0, 0.0)
        return P, G, key

    cases = [c for c in turbulence_cases.CASES if c["desc"]["seed"] == seed and c["size"] == (40, 20)]
    assert len(cases) >= 4
    changed = 0
    for c in cases:
        want = turbulence_cases.expected(c["name"])
        turbulence_ref.tables = patched
        try:
            other = turbulence_ref.turbulence((20, 40), c["rect"], turbulence_cases.before(c), **c["desc"])
        finally:
            turbulence_ref.tables = real
        assert np.array_equal(other[..., [0, 2, 3]], want[..., [0, 2, 3]])
        changed += int(not np.array_equal(other[..., 1], want[..., 1]))
    assert changed >= 2


# ---- the battery ----

def test_battery_covers_what_it_names():
    cases = turbulence_cases.CASES
    assert len({c["name"] for c in cases}) == len(cases) >= 150
    assert {c["inst"] for c in cases} == {"fractal/0", "fractal/1", "turbulence/0", "turbulence/1"}
    assert all(any(c["rect"] for c in cases if c["inst"] == i) for i in ("fractal/0", "fractal/1", "turbulence/0", "turbulence/1"))
    assert {c["size"] for c in cases} >= set(turbulence_cases.TILE_SIZES) | set(turbulence_cases.GRID_SIZES)
    d = [dict(turbulence_ref.DEFAULTS, **c["desc"]) for c in cases]
    for kind in (FRACTAL_NOISE, TURBULENCE):
        assert {x["octaves"] for x in d if x["kind"] == kind} >= {0, 1, 2, 5, 16}
        assert {x["seed"] for x in d if x["kind"] == kind} >= set(turbulence_cases.SEEDS)
        assert {tuple(x["base_frequency"]) for x in d if x["kind"] == kind} >= set(turbulence_cases.FREQUENCIES)
    assert any(c["prior"] == "never" for c in cases)
    assert any(x["origin"][0] < 0 and x["origin"][0] != int(x["origin"][0]) for x in d) and any(abs(x["origin"][0]) >= 1e6 for x in d)
    # tile edges inside the image, a tile smaller than a cell, a wrap crossed in the first and in the last octave
    for c in cases:
        if c["name"].startswith("stitch_"):
            p = turbulence_ref.plan(**c["desc"])
            assert p["stitched"] == 1
    small = [turbulence_ref.plan(**c["desc"]) for c in cases if c["desc"].get("stitch_tile") == (0.0, 0.0, 30.0, 10.0)]
    assert small and all(list(p["width"]) == [1, 1] for p in small)


NEAR_MISSES = {
    "mask before stitch": dict(mask_first=True),
    "the single-level selector": dict(single_level=True),
    "the s-curve's operand order": dict(s_order=True),
    "lerp as a + t b - t a": dict(lerp_expanded=True),
    "ratio applied after the sum": dict(ratio_after=True),
    "|n| under FRACTAL_NOISE": dict(abs_fractal=True),
    "truncation instead of floor for negative cells": dict(trunc_cells=True),
    "the + 0.5 centre left out": dict(no_half=True),
}


@pytest.mark.parametrize("miss", sorted(NEAR_MISSES))
def test_the_battery_tells_every_near_miss_from_the_rule(miss):
    """Each near miss of the rule changes at least one byte of the battery's expected output (the big grid-stride cases left out: the
    smaller ones suffice).  A variant the range refuses where the rule does not (the centre left out moves the start) counts as told."""
    changed = 0
    for c in turbulence_cases.CASES:
        if c["size"][1] > 1000:
            continue
        try:
            other = turbulence_cases.expected(c["name"], **NEAR_MISSES[miss])
        except ValueError:
            continue
        if not np.array_equal(turbulence_cases.expected(c["name"]), other):
            changed += 1
    assert changed >= 3, (miss, changed)
