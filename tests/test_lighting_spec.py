"""The lighting rule on the CPU: the plan and the tables of the library (jh_lighting_plan, jh_lighting_tables) and of
the host twin (jl_lighting_plan, jl_lighting_tables) against the reference's bit for bit, the ctypes mirrors' layout, the legality
boundaries from both sides, the nine cases of the normal against the specification's formulas, texels worked by hand, the
consequences the header states, the reference (tests/lighting_ref.py) against the specification in binary64 within the bound DESIGN
derives, the stand-alone check (tools/lighting_check.cpp), and the sensitivity of the battery (tests/lighting_cases.py) to every near
miss of the rule."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import LightKind, LightSource, _lib, lighting

import lighting_cases
import lighting_ref
from abi_text import INCLUDE, ROOT, c_values
from lighting_ref import DIFFUSE, DISTANT, POINT, SPECULAR, SPOT

F = np.float32
U = 2.0 ** -24  # the unit roundoff of binary32


def f16(values):
    return np.asarray(values, np.float32).astype(np.float16).view(np.uint16)


def as_f64(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def image(alpha):
    """(H, W, 4) bits with this alpha and a colour that must not matter."""
    a = np.asarray(alpha, np.float64)
    img = np.full(a.shape + (4,), 0.75, np.float16)
    img[..., 3] = a
    return img.view(np.uint16)


# ---- the plan and the tables ----

DESCS = [
    dict(kind=DIFFUSE, light=DISTANT, surface_scale=3.0, direction=(0.3, -0.7, 0.2)),
    dict(kind=DIFFUSE, light=DISTANT, surface_scale=0.1, direction=(1e-3, 1e3, -1.0)),
    dict(kind=SPECULAR, light=DISTANT, surface_scale=-2.5, specular_exponent=20.0, direction=(1e150, 1e150, 0.0)),
    dict(kind=DIFFUSE, light=POINT, surface_scale=1000.0, position=(0.1, -1e30, 16777217.0)),
    dict(kind=SPECULAR, light=POINT, surface_scale=-0.0, specular_exponent=1.0, position=(12.25, 7.5, 3.0)),
    dict(kind=DIFFUSE, light=SPOT, surface_scale=1e-30, position=(1.0, 2.0, 3.0), points_at=(4.1, 5.2, 0.3), spot_exponent=1.5, cone_cos=0.30000000000000004),
    dict(kind=SPECULAR, light=SPOT, surface_scale=5.0, specular_exponent=128.0, position=(-20.0, 40.0, 15.0), points_at=(-20.0, 40.0, 14.999999), spot_exponent=128.0,
         cone_cos=-1.0),
    dict(kind=SPECULAR, light=SPOT, surface_scale=5.0, specular_exponent=1.5, position=(0.0, 0.0, 1e-3), points_at=(1e6, 1e6, 0.0), spot_exponent=1.0, cone_cos=1.0),
]


@pytest.mark.parametrize("twin", [False, True], ids=["library", "host twin"])
def test_plan_equals_the_reference_bit_for_bit(built, twin):
    for d in DESCS:
        got, want = jello_amd.lighting_plan(twin=twin, **d), lighting_ref.plan(**d)
        for k in ("s", "ldir", "p", "sdir"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (d, k, got[k], want[k])
        assert np.float32(got["cone"]).view(np.uint32) == np.float32(want["cone"]).view(np.uint32), d


@pytest.mark.parametrize("twin", [False, True], ids=["library", "host twin"])
def test_tables_equal_the_reference_bit_for_bit(built, twin):
    for d in DESCS:
        spec, spot, which = jello_amd.lighting_tables(twin=twin, **d)
        assert which == lighting_ref.which(**d)
        for got, e, bit in ((spec, d.get("specular_exponent", 1.0), 1), (spot, d.get("spot_exponent", 1.0), 2)):
            if which & bit:
                assert got.shape == (4097,) and np.array_equal(got.view(np.uint32), lighting_ref.table(e).view(np.uint32)), (d, bit)
            else:
                assert got is None
    for e in (1.5, 2.0, 20.0, 128.0):
        T = lighting_ref.table(e)
        assert T[0] == 0.0 and T[4096] == 1.0 and np.all(np.diff(T.astype(np.float64)) >= 0) and T[2048] == np.float32(0.5 ** e)


def test_which_tables_a_descriptor_needs():
    assert [lighting_ref.which(**d) for d in DESCS] == [0, 0, 1, 0, 0, 2, 3, 1]
    point = dict(light=POINT, position=(1.0, 1.0, 1.0))
    assert lighting_ref.which(kind=DIFFUSE, specular_exponent=20.0, spot_exponent=20.0, **point) == 0  # (neither exponent is in use)
    assert jello_amd.lighting_tables(kind=DIFFUSE, specular_exponent=20.0, spot_exponent=20.0, **point)[2] == 0


# ---- the C ABI ----

def test_ctypes_mirrors_have_the_headers_layout():
    for mirror, struct in ((_lib.CLightingDesc, "jh_lighting_desc"), (_lib.CLightPlan, "jh_light_plan")):
        fields = [name for name, _ in mirror._fields_]
        want = c_values(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, f) for f in fields])
        assert [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, struct
    assert [n for n, _ in _lib.CLightingDesc._fields_] == ["kind", "light", "surface_scale", "constant", "specular_exponent", "spot_exponent", "color", "x", "y",
                                                          "width", "height", "direction", "position", "points_at", "cone_cos"]
    assert [n for n, _ in _lib.CLightPlan._fields_] == ["s", "ldir", "p", "sdir", "cone"]


def test_enums_and_limits_match_the_header():
    names = ["JH_LIGHTING_" + k.name for k in LightKind] + ["JH_LIGHT_" + s.name for s in LightSource]
    assert c_values(names) == [int(k) for k in LightKind] + [int(s) for s in LightSource] == [0, 1, 0, 1, 2]
    assert c_values(["JH_LIGHTING_TABLE_ENTRIES", "JH_LIGHTING_TABLE_SPEC", "JH_LIGHTING_TABLE_SPOT", "JH_LIGHTING_MAX_EXTENT"]) == [4097, 1, 2, 1 << 23]
    from jello_amd import engine
    assert (engine.LIGHTING_TABLE_ENTRIES, engine.LIGHTING_TABLE_SPEC, engine.LIGHTING_TABLE_SPOT) == (4097, 1, 2)
    assert (lighting_ref.ENTRIES, lighting_ref.TABLE_SPEC, lighting_ref.TABLE_SPOT, lighting_ref.MAX_EXTENT) == (4097, 1, 2, 1 << 23)
    assert (lighting_ref.DIFFUSE, lighting_ref.SPECULAR, lighting_ref.DISTANT, lighting_ref.POINT, lighting_ref.SPOT) == (0, 1, 0, 1, 2)


def test_the_python_constructors():
    d = lighting.distant(90, 0)
    assert d["light"] == LightSource.DISTANT and np.allclose(d["direction"], (0.0, 1.0, 0.0), atol=1e-15)
    assert np.allclose(lighting.distant(0, 90)["direction"], (0.0, 0.0, 1.0), atol=1e-15)
    az, el = math.radians(30), math.radians(60)
    assert lighting.distant(30, 60)["direction"] == (math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el))
    assert lighting.point(1, 2, 3) == dict(light=LightSource.POINT, position=(1.0, 2.0, 3.0))
    s = lighting.spot(1, 2, 3, (4, 5, 6), 8, -30)
    assert s == dict(light=LightSource.SPOT, position=(1.0, 2.0, 3.0), points_at=(4.0, 5.0, 6.0), spot_exponent=8.0, cone_cos=math.cos(math.radians(30)))
    assert lighting.spot(0, 0, 1, (0, 0, 0))["cone_cos"] == -1.0 and lighting.spot(0, 0, 1, (0, 0, 0))["spot_exponent"] == 1.0
    assert lighting.diffuse() == dict(kind=LightKind.DIFFUSE, surface_scale=1.0, constant=1.0, color=(1.0, 1.0, 1.0))
    sp = lighting.specular(5, 0.75, 20, (1.0, 0.5, 0.0))
    assert (sp["kind"], sp["surface_scale"], sp["constant"], sp["specular_exponent"]) == (LightKind.SPECULAR, 5.0, 0.75, 20.0)
    assert sp["color"][0] == 1.0 and sp["color"][2] == 0.0 and abs(sp["color"][1] - 0.21404114048223255) < 1e-15  # the sRGB curve
    assert lighting.srgb_to_linear(0.04045) == 0.04045 / 12.92
    # a descriptor as Engine.lighting builds it
    c = jello_amd.engine._lighting_desc(rect=(1, 2, 3, 4), **sp, **s)
    assert (c.kind, c.light, c.surface_scale, c.constant, c.specular_exponent, c.spot_exponent, c.x, c.y, c.width, c.height) == (1, 2, 5.0, 0.75, 20.0, 8.0, 1, 2, 3, 4)
    assert list(c.position) == [1.0, 2.0, 3.0] and list(c.points_at) == [4.0, 5.0, 6.0] and c.cone_cos == s["cone_cos"]
    assert list(c.color) == [1.0, float(np.float32(sp["color"][1])), 0.0]
    with pytest.raises(ValueError, match="jh_lighting: "):
        jello_amd.engine._lighting_desc(direction=(1.0, 2.0))


# ---- legality, from both sides of every boundary ----

def _legal(**kw):
    try:
        lighting_ref.check(**kw)
        ref = True
    except ValueError:
        ref = False
    got = []
    for twin in (False, True):
        try:
            jello_amd.lighting_plan(twin=twin, **kw)
            got.append(True)
        except ValueError:
            got.append(False)
    assert got == [ref, ref], (kw, ref, got)
    return ref


def test_legality_boundaries(built):
    nan, inf = math.nan, math.inf
    spot = dict(light=SPOT, position=(1.0, 2.0, 3.0), points_at=(4.0, 5.0, 0.0))
    below1, above128 = float(np.nextafter(F(1), F(0))), float(np.nextafter(F(128), F(200)))
    assert _legal() and _legal(kind=SPECULAR, light=SPOT, points_at=(0.0, 0.0, 1.0))
    assert not _legal(kind=2) and not _legal(kind=-1) and not _legal(light=3) and not _legal(light=-1)
    assert _legal(surface_scale=-3.4e38) and not _legal(surface_scale=inf) and not _legal(surface_scale=nan)
    assert _legal(constant=0.0) and _legal(constant=3.4e38) and not _legal(constant=-1e-45) and not _legal(constant=inf) and not _legal(constant=nan)
    assert _legal(constant=-0.0)  # (-0 >= 0)
    for e, ok in ((1.0, True), (128.0, True), (below1, False), (above128, False), (nan, False), (0.0, False), (inf, False)):
        assert _legal(kind=SPECULAR, specular_exponent=e) == ok
        assert _legal(spot_exponent=e, **spot) == ok
        assert _legal(kind=DIFFUSE, specular_exponent=e)  # (not read)
        assert _legal(light=POINT, spot_exponent=e)
    assert _legal(color=(0.0, 0.0, 0.0)) and _legal(color=(3e38, 1.0, 1.0)) and not _legal(color=(1.0, -1e-45, 1.0)) and not _legal(color=(1.0, 1.0, inf))
    assert not _legal(color=(nan, 1.0, 1.0))
    assert _legal(direction=(0.0, 0.0, -1e-150)) and not _legal(direction=(0.0, 0.0, 0.0)) and not _legal(direction=(0.0, 1e-170, 0.0))
    assert _legal(direction=(1e150, 1e150, 1e150)) and not _legal(direction=(1e155, 0.0, 0.0)) and not _legal(direction=(nan, 0.0, 1.0))
    assert not _legal(direction=(inf, 0.0, 0.0))
    assert _legal(light=POINT, position=(3.4e38, -3.4e38, 0.0)) and not _legal(light=POINT, position=(3.5e38, 0.0, 0.0)) and not _legal(light=POINT, position=(0.0, nan, 0.0))
    assert _legal(light=POINT, direction=(0.0, 0.0, 0.0)) and _legal(light=DISTANT, position=(nan, nan, nan), points_at=(nan, nan, nan), cone_cos=nan)
    assert not _legal(**dict(spot, points_at=spot["position"])) and _legal(**dict(spot, points_at=(1.0, 2.0, 3.0000000000000004)))
    assert not _legal(**dict(spot, points_at=(inf, 0.0, 0.0))) and not _legal(**dict(spot, points_at=(1e200, 0.0, 0.0)))
    for c, ok in ((-1.0, True), (1.0, True), (0.0, True), (float(np.nextafter(1.0, 2.0)), False), (float(np.nextafter(-1.0, -2.0)), False), (nan, False)):
        assert _legal(cone_cos=c, **spot) == ok
    for f in (_lib.load_host().jl_lighting_plan, _lib.load_host().hip.jh_lighting_plan):
        assert f(None, ctypes.byref(_lib.CLightPlan())) != 0 and f(ctypes.byref(jello_amd.engine._lighting_desc()), None) != 0
    for f in (_lib.load_host().jl_lighting_tables, _lib.load_host().hip.jh_lighting_tables):
        assert f(None, None, None, None) != 0 and f(ctypes.byref(jello_amd.engine._lighting_desc()), None, None, None) == 0


# ---- the normal: nine cases against the specification's table ----

def _spec_normal(I, ss, x, y):
    """Filter Effects, 'Light source and surface normal calculations', in float64, on I[y][x]; for an image one texel wide or high the
    forms the rule leaves."""
    H, W = I.shape
    g = lambda i, j: float(I[j, i])  # noqa: E731
    l, r, t, b = x == 0, x == W - 1, y == 0, y == H - 1  # noqa: E741
    if W == 1 or H == 1:
        nx = ny = 0.0
        if W > 1:
            nx = -ss * (2 * g(x + 1, y) - 2 * g(x, y)) if l else -ss * (2 * g(x, y) - 2 * g(x - 1, y)) if r else -ss / 2 * (2 * g(x + 1, y) - 2 * g(x - 1, y))
        if H > 1:
            ny = -ss * (2 * g(x, y + 1) - 2 * g(x, y)) if t else -ss * (2 * g(x, y) - 2 * g(x, y - 1)) if b else -ss / 2 * (2 * g(x, y + 1) - 2 * g(x, y - 1))
        return nx, ny
    if t and l:
        return (-ss * 2 / 3 * ((2 * g(x + 1, y) + g(x + 1, y + 1)) - (2 * g(x, y) + g(x, y + 1))),
                -ss * 2 / 3 * ((2 * g(x, y + 1) + g(x + 1, y + 1)) - (2 * g(x, y) + g(x + 1, y))))
    if t and r:
        return (-ss * 2 / 3 * ((2 * g(x, y) + g(x, y + 1)) - (2 * g(x - 1, y) + g(x - 1, y + 1))),
                -ss * 2 / 3 * ((g(x - 1, y + 1) + 2 * g(x, y + 1)) - (g(x - 1, y) + 2 * g(x, y))))
    if b and l:
        return (-ss * 2 / 3 * ((g(x + 1, y - 1) + 2 * g(x + 1, y)) - (g(x, y - 1) + 2 * g(x, y))),
                -ss * 2 / 3 * ((2 * g(x, y) + g(x + 1, y)) - (2 * g(x, y - 1) + g(x + 1, y - 1))))
    if b and r:
        return (-ss * 2 / 3 * ((g(x, y - 1) + 2 * g(x, y)) - (g(x - 1, y - 1) + 2 * g(x - 1, y))),
                -ss * 2 / 3 * ((g(x - 1, y) + 2 * g(x, y)) - (g(x - 1, y - 1) + 2 * g(x, y - 1))))
    if t:
        return (-ss * 1 / 3 * ((2 * g(x + 1, y) + g(x + 1, y + 1)) - (2 * g(x - 1, y) + g(x - 1, y + 1))),
                -ss * 1 / 2 * ((g(x - 1, y + 1) + 2 * g(x, y + 1) + g(x + 1, y + 1)) - (g(x - 1, y) + 2 * g(x, y) + g(x + 1, y))))
    if b:
        return (-ss * 1 / 3 * ((g(x + 1, y - 1) + 2 * g(x + 1, y)) - (g(x - 1, y - 1) + 2 * g(x - 1, y))),
                -ss * 1 / 2 * ((g(x - 1, y) + 2 * g(x, y) + g(x + 1, y)) - (g(x - 1, y - 1) + 2 * g(x, y - 1) + g(x + 1, y - 1))))
    if l:
        return (-ss * 1 / 2 * ((g(x + 1, y - 1) + 2 * g(x + 1, y) + g(x + 1, y + 1)) - (g(x, y - 1) + 2 * g(x, y) + g(x, y + 1))),
                -ss * 1 / 3 * ((2 * g(x, y + 1) + g(x + 1, y + 1)) - (2 * g(x, y - 1) + g(x + 1, y - 1))))
    if r:
        return (-ss * 1 / 2 * ((g(x, y - 1) + 2 * g(x, y) + g(x, y + 1)) - (g(x - 1, y - 1) + 2 * g(x - 1, y) + g(x - 1, y + 1))),
                -ss * 1 / 3 * ((g(x - 1, y + 1) + 2 * g(x, y + 1)) - (g(x - 1, y - 1) + 2 * g(x, y - 1))))
    return (-ss * 1 / 4 * ((g(x + 1, y - 1) + 2 * g(x + 1, y) + g(x + 1, y + 1)) - (g(x - 1, y - 1) + 2 * g(x - 1, y) + g(x - 1, y + 1))),
            -ss * 1 / 4 * ((g(x - 1, y + 1) + 2 * g(x, y + 1) + g(x + 1, y + 1)) - (g(x - 1, y - 1) + 2 * g(x, y - 1) + g(x + 1, y - 1))))


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("H", [1, 2, 3, 4, 5])
def test_the_nine_cases_of_the_normal(W, H):
    """On small-integer alpha and surface_scale 3 every factor, sum and product is exact, so the reference's normal equals the
    specification's formula in float64 at every texel -- which proves the one-sided forms and their factors."""
    rng = np.random.default_rng(W * 16 + H)
    I = rng.integers(-8, 9, (H, W)).astype(np.float64)
    s = lighting_ref.plan(surface_scale=3.0)["s"]
    assert np.array_equal(s, np.array([[-3.0, -2.0, -1.5], [-1.5, -1.0, -0.75]], F))
    nx, ny = lighting_ref.normal(I.astype(F), np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64), s)
    for y in range(H):
        for x in range(W):
            assert (float(nx[y, x]), float(ny[y, x])) == _spec_normal(I, 3.0, x, y), (x, y)
    # and a rectangle of the image has the image's normals: the image is the edge
    if W >= 3 and H >= 3:
        nx1, ny1 = lighting_ref.normal(I.astype(F), np.arange(1, W - 1, dtype=np.int64), np.arange(1, H, dtype=np.int64), s)
        assert np.array_equal(nx1, nx[1:, 1:W - 1]) and np.array_equal(ny1, ny[1:, 1:W - 1])


# ---- texels worked by hand ----

def test_texels_worked_by_hand():
    """A 3 x 3 image whose alpha is x / 4 (exact in f16), surface_scale 2, kd 0.5, a white DISTANT light straight above and one at 45
    degrees in the x z plane.  Interior texel (1, 1): gx = (0.5 + 1 + 0.5) - 0 = 2, Nx = -2/4 * 2 = -1, Ny = 0, nlen = sqrt(2).
    Straight above: t = 1 / sqrt 2.  At 45 degrees from +x: l = (r, 0, r), r = (float)sqrt(0.5): t = (fmaf(-1, r, r)) / nlen = 0."""
    bits = image(np.tile(np.array([0.0, 0.25, 0.5]), (3, 1)))
    up = lighting_ref.lighting(bits, kind=DIFFUSE, light=DISTANT, surface_scale=2.0, constant=0.5, direction=(0.0, 0.0, 5.0))
    t = F(1.0) / np.sqrt(F(2.0))
    assert up[1, 1].tolist() == [int(f16(F(0.5) * t))] * 3 + [0x3C00]
    # left column (0, 1): span 1, wsum 4, s = -2 * 2 / 4 = -1, gx = (0.25 * 4) - 0 = 1, Nx = -1: the same normal
    assert np.array_equal(up[1, 0], up[1, 1]) and np.array_equal(up[1, 2], up[1, 1])
    # corner (0, 0): span 1, wsum 3, s = -4/3 rounded, gx = 0.25 * 3 = 0.75, Nx = (float)(-4/3) * 0.75
    nx = F(-4.0 / 3.0) * F(0.75)
    nlen = np.sqrt(lighting_ref.fmaf32(nx, nx, F(1.0))).astype(F)
    assert up[0, 0, 0] == int(f16(F(0.5) * (F(1.0) / nlen)))
    side = lighting_ref.lighting(bits, kind=DIFFUSE, light=DISTANT, surface_scale=2.0, constant=0.5, direction=(1.0, 0.0, 1.0))
    assert side[1, 1].tolist() == [0, 0, 0, 0x3C00]
    # SPECULAR, exponent 1, the light straight above: h = (0, 0, 2), hlen = 2, q = 2 / (sqrt 2 * 2); colour (1, 0.5, 0) and ks 1: V = q (1, 0.5,
    # 0), alpha = q, stored colour V / q
    spec = lighting_ref.lighting(bits, kind=SPECULAR, light=DISTANT, surface_scale=2.0, constant=1.0, color=(1.0, 0.5, 0.0), direction=(0.0, 0.0, 1.0))
    q = F(2.0) / (np.sqrt(F(2.0)) * F(2.0)).astype(F)
    a_inv = F(1.0) / q
    assert spec[1, 1].tolist() == [int(f16(q * a_inv)), int(f16(F(0.5) * q * a_inv)), 0, int(f16(q))]
    # a POINT light straight above texel (1, 1) at height 4.5: Z = 2 * 0.25 = 0.5, v = (0, 0, 4), l = (0, 0, 1): the DISTANT result
    pt = lighting_ref.lighting(bits, kind=DIFFUSE, light=POINT, surface_scale=2.0, constant=0.5, position=(1.5, 1.5, 4.5))
    assert np.array_equal(pt[1, 1], up[1, 1])
    # ... and without the half texel the light is not above the centre
    assert not np.array_equal(lighting_ref.lighting(bits, kind=DIFFUSE, light=POINT, surface_scale=2.0, constant=0.5, position=(1.5, 1.5, 4.5), half=False)[1, 1], up[1, 1])


# ---- the consequences the header states ----

def test_constant_alpha_is_a_flat_surface():
    for a in (0.0, 0.5, 1.0, 7.0, -2.0):
        bits = image(np.full((7, 9), a))
        for direction, kd, color in (((0.3, -0.7, 0.2), 1.0, (1.0, 0.5, 0.25)), ((0.0, 0.0, 1.0), 3.0, (0.2, 0.4, 0.6)), ((1.0, 1.0, 0.01), 0.5, (1.0, 1.0, 1.0))):
            got = lighting_ref.lighting(bits, kind=DIFFUSE, light=DISTANT, surface_scale=5.0, constant=kd, color=color, direction=direction)
            lz = lighting_ref.plan(direction=direction)["ldir"][2]
            want = [int(f16(min(F(F(kd) * lz) * F(c), F(1.0)))) for c in color] + [0x3C00]
            assert np.all(got == np.array(want, np.uint16)), (a, direction)


def test_a_light_below_the_surface_gives_black():
    bits = lighting_cases.content("disc", 21, 13, 3)
    for kw in (dict(light=DISTANT, direction=(0.3, 0.2, -0.5)), dict(light=POINT, position=(10.0, 6.0, -300.0))):
        got = lighting_ref.lighting(bits, kind=DIFFUSE, surface_scale=0.5, constant=2.0, **kw)
        assert np.all(got[..., :3] == 0) and np.all(got[..., 3] == 0x3C00)


def test_specular_alpha_is_the_maximum_of_the_premultiplied_colour():
    bits = lighting_cases.content("disc", 33, 17, 5)
    kw = dict(kind=SPECULAR, light=POINT, surface_scale=4.0, constant=0.9, specular_exponent=8.0, color=(0.5, 1.0, 0.25), position=(12.0, 8.0, 20.0))
    got = as_f64(lighting_ref.lighting(bits, **kw))
    V, a = lighting_ref.exact(bits, **kw)
    assert a.max() > 0.3
    lit = a > 1e-3
    assert np.allclose(got[..., 3][lit], V.max(axis=-1)[lit], rtol=2e-3)
    assert np.allclose(got[..., 1][lit], 1.0, rtol=1e-3)  # the largest channel is stored as 1: un-premultiplied
    assert np.allclose((got[..., :3] * got[..., 3:])[lit], V[lit], rtol=3e-3, atol=1e-4)


def test_the_alpha_outside_the_rectangle_shows_in_the_normals():
    bits = lighting_cases.content("random", 20, 12, 9)
    kw = dict(kind=DIFFUSE, light=DISTANT, surface_scale=3.0, direction=(0.5, 0.5, 0.7))
    rect = (4, 3, 9, 5)
    a = lighting_ref.lighting(bits, rect, **kw)
    other = bits.copy()
    other[2, 4:13, 3] ^= 0x0100  # the row above the rectangle
    b = lighting_ref.lighting(other, rect, **kw)
    assert not np.array_equal(a[3, 4:13], b[3, 4:13]) and np.array_equal(a[4:8], b[4:8])
    assert np.all(a[:3] == 0) and np.all(a[8:] == 0) and np.all(a[:, :4] == 0) and np.all(a[:, 13:] == 0)


# ---- the reference against the specification in binary64 ----

def table_bound(e):
    """|Pw(t, e) - t^e| on [0, 1] before any rounding: linear interpolation with h = 1 / 4096."""
    e = float(e)
    if e == 1.0:
        return 0.0
    return e * (e - 1.0) / (8.0 * 4096.0 ** 2) if e >= 2.0 else 4096.0 ** -e


def bound(kw, size, len_min):
    """The first-order bound of DESIGN.md 5.14 on |premultiplied colour of the reference - the specification in binary64|, per
    channel, for alpha in [0, 1], a light above the surface (l.z >= 0, so hlen >= 1) and no distance to the light below len_min: the
    arithmetic part (to which the f16 store is added by the caller).  Holds away from the cone's hard edge."""
    d = dict(lighting_ref.DEFAULTS, **kw)
    ss, k, cmax = abs(float(d["surface_scale"])), float(d["constant"]), float(max(d["color"]))
    E_N = 28.0 * ss * U                  # Nx, Ny: two sums of <= 4 (8u each), their difference, s rounded, the product
    M = 8.0 * ss + 1.0                   # |Nx| + |Ny| + 1
    if d["light"] == DISTANT:
        E_l = 2.0 * U
    else:
        R = max([abs(v) for v in d["position"]] + [float(size[0]), float(size[1]), ss])
        E_l = (1.0 + math.sqrt(3.0)) * 3.0 * U * R / len_min + 3.5 * U
    if d["kind"] == DIFFUSE:
        E_t = 3.5 * E_N + M * (E_l + 2.0 * U) + 3.0 * U
    else:
        E_q = 3.5 * E_N + (M + 2.0) * (E_l + 2.0 * U) + 7.0 * U
        e = float(d["specular_exponent"])
        E_t = e * E_q + table_bound(e) + 4.0 * U
    E_C = 0.0
    if d["light"] == SPOT:
        E_m = 3.0 * (E_l + U) + 3.0 * U
        es = float(d["spot_exponent"])
        E_C = cmax * (es * E_m + table_bound(es) + 5.0 * U)
    return 1.01 * k * (cmax * E_t + 1.0 * E_C + 3.0 * U * cmax)


def cone_margin(kw, size, len_min):
    d = dict(lighting_ref.DEFAULTS, **kw)
    R = max([abs(v) for v in d["position"]] + [float(size[0]), float(size[1]), abs(float(d["surface_scale"]))])
    E_l = (1.0 + math.sqrt(3.0)) * 3.0 * U * R / len_min + 3.5 * U
    return 2.0 * (3.0 * (E_l + U) + 3.0 * U)


SPEC_CASES = [(kind, light, e, es, content) for kind in (DIFFUSE, SPECULAR) for light in (DISTANT, POINT, SPOT)
              for e in ((1.0, 1.5, 2.0, 20.0, 128.0) if kind == SPECULAR else (1.0,)) for es in ((1.0, 1.5, 20.0, 128.0) if light == SPOT and e in (1.0, 20.0) else (1.0,))
              for content in ("disc", "random")]


@pytest.mark.parametrize("kind,light,e,es,content", SPEC_CASES)
def test_the_reference_is_the_specification_within_the_derived_bound(kind, light, e, es, content):
    """The stored texel, premultiplied again, against the specification evaluated in binary64 (real pow, no table, no rounding): within
    bound() plus the store -- half an f16 ULP on colour and on alpha for SPECULAR (2^-11 relative each, 2^-25 absolute below the
    normal range, and 2e-6 where alpha is under the store's floor of 1e-6), half an f16 ULP for DIFFUSE.  The table's term is e (e - 1) /
    (8 4096^2): 2.8e-6 at 20, 1.2e-4 at 128; the worst case of the roundings that reach the power's argument, e E_q, is a bound 25
    times that at 128 and surface_scale 3, and it is in bound() as derived, not trimmed to what the data show."""
    W, H = 45, 23
    bits = lighting_cases.content(content, W, H, 7)
    where = {DISTANT: dict(direction=(0.4, -0.3, 0.6)), POINT: dict(position=(17.3, 9.1, 12.0)),
             SPOT: dict(position=(17.3, 9.1, 12.0), points_at=(25.0, 14.0, 0.0), spot_exponent=es, cone_cos=0.8)}[light]
    kw = dict(kind=kind, light=light, surface_scale=3.0, constant=0.9, specular_exponent=e, color=(1.0, 0.6, 0.2), **where)
    got = as_f64(lighting_ref.lighting(bits, **kw))
    V, _ = lighting_ref.exact(bits, **kw)
    len_min = 12.0 - 3.0  # the light's height less the highest surface
    keep = np.ones((H, W), bool)
    if light == SPOT:  # away from the cone's hard edge
        A = lighting_ref.alpha_of(bits).astype(np.float64)
        yy, xx = np.mgrid[0:H, 0:W]
        v = np.stack([17.3 - (xx + 0.5), 9.1 - (yy + 0.5), 12.0 - 3.0 * A], -1)
        s = np.array([25.0 - 17.3, 14.0 - 9.1, -12.0])
        m = -(v @ s) / np.linalg.norm(v, axis=-1) / np.linalg.norm(s)
        keep = np.abs(m - 0.8) > cone_margin(kw, (W, H), len_min)
        assert keep.mean() > 0.95 and (m > 0.8).any() and (m < 0.8).any()
    arithmetic = bound(kw, (W, H), len_min)
    if kind == DIFFUSE:
        pre = got[..., :3]
        store = np.maximum(np.abs(V) * 2.0 ** -11, 2.0 ** -25)
        assert np.all(got[..., 3] == 1.0)
    else:
        pre = got[..., :3] * got[..., 3:]
        store = np.maximum(np.abs(V) * 2.1 * 2.0 ** -11, 2.0 ** -24) + 2e-6
    err = np.abs(pre - V)
    assert V.max() > (0.05 if (kind == SPECULAR and e >= 20) or es >= 20 else 0.2)  # (there is light to compare)
    assert np.all(err[keep] <= (arithmetic + store)[keep]), (float((err - store)[keep].max()), arithmetic)


def test_the_tables_interpolation_error_is_within_its_bound():
    """max |Pw(t, e) - t^e| over a fine grid of t, against the derived bound plus the binary32 roundings of the entries, the difference
    and the fmaf (4 u): 1.2e-4 at 128 as DESIGN states, and 1024 entries would be 16 times coarser."""
    t = np.linspace(0.0, 1.0, 200001).astype(F)
    for e in (1.5, 1.0 + 2.0 ** -10, 1.999, 2.0, 3.0, 20.0, 128.0):
        err = np.abs(lighting_ref.power(t, e).astype(np.float64) - t.astype(np.float64) ** float(F(e))).max()
        assert err <= table_bound(e) + 4.0 * U, (e, err)
    assert 1.1e-4 < table_bound(128.0) < 1.3e-4 and table_bound(128.0) < 2.0 ** -12  # below the f16 half ULP under 1
    coarse = np.abs(lighting_ref.power(t, 128.0, entries=1025).astype(np.float64) - t.astype(np.float64) ** 128.0).max()
    assert 1.5e-3 < coarse < 2.0e-3


# ---- the stand-alone check ----

def test_the_stand_alone_check_builds_and_passes(tmp_path):
    """tools/lighting_check.cpp is include/jello_lighting.h with a main of its own: legal and illegal descriptors, the plan against
    long double, the nine cases of the normal against the specification's table on images of 1..4 texels per side, the tables' ends
    and monotonicity.  Its header has the command with the sanitizers; here it is built without them and run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lighting_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-I", INCLUDE, os.path.join(ROOT, "tools", "lighting_check.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode() == "ok\n"


# ---- the battery ----

def test_battery_covers_what_it_names():
    cases = lighting_cases.CASES
    assert len({c["name"] for c in cases}) == len(cases) >= 200
    insts = {c["inst"] for c in cases}
    assert len(insts) == 12 and all(any(c["rect"] for c in cases if c["inst"].startswith(k)) for k in ("diffuse", "specular"))
    assert {c["size"] for c in cases} >= set(lighting_cases.TILE_SIZES) | {s for v in lighting_cases.GRID_SIZES.values() for s in v}
    assert {c["kind"] for c in cases} == set(lighting_cases.CONTENTS)
    d = [dict(lighting_ref.DEFAULTS, **c["desc"]) for c in cases]
    assert {x["specular_exponent"] for x in d if x["kind"] == SPECULAR} >= {1.0, 1.5, 20.0, 128.0}
    assert {x["spot_exponent"] for x in d if x["light"] == SPOT} >= {1.0, 1.5, 20.0, 128.0}
    assert {x["cone_cos"] for x in d if x["light"] == SPOT} >= {-1.0, 0.0, 1.0, 0.9}
    assert {x["surface_scale"] for x in d} >= {0.0, -2.5, 1000.0} and 0.0 in {x["constant"] for x in d}
    assert any(c["prior"] == "never" for c in cases)
    for c in cases:  # the len = 0 cases do have a texel at distance 0
        if "surface" in c["name"]:
            w, h = c["size"]
            assert c["desc"]["position"] == (w // 2 + 0.5, h // 2 + 0.5, 1.0) and c["kind"] == "const" and c["desc"]["surface_scale"] == 2.0


NEAR_MISSES = {
    "the interior factor at an edge": dict(interior_factor=True),
    "no + 0.5": dict(half=False),
    "N normalised before the dot product": dict(normal_first=True),
    "a reciprocal times v instead of three divisions": dict(reciprocal=True),
    "H normalised separately from the quotient": dict(h_first=True),
    "a table of 1024 steps": dict(entries=1025),
    "the table index rounded": dict(index_rounded=True),
    "specular alpha = 1": dict(alpha_one=True),
    "the clamp before the multiply by the colour": dict(clamp_first=True),
}


@pytest.mark.parametrize("miss", sorted(NEAR_MISSES))
def test_the_battery_tells_every_near_miss_from_the_rule(miss):
    """Each near miss of the rule changes at least one byte of the battery's expected output (the big grid-stride cases left out: the
    smaller ones suffice)."""
    changed = 0
    for c in lighting_cases.CASES:
        if c["size"][1] > 1000:
            continue
        if not np.array_equal(lighting_cases.expected(c["name"]), lighting_cases.expected(c["name"], **NEAR_MISSES[miss])):
            changed += 1
    assert changed >= 3, (miss, changed)
