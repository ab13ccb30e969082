"""The colour-filter rule on the CPU: the library's tables and its host twin's against the reference's
(tests/color_ref.py) bit for bit, the refusals of jh_color_tables, the reference against the binary64 definition it rounds, the
Filter Effects constructors against the specification's numbers, the consequences the rule states, texels worked by hand, the
ctypes mirrors, and that the battery (tests/color_cases.py) tells the rule from its near misses."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import jello_amd
from jello_amd import ColorFunc, ColorSpace, _lib
from jello_amd import colorfilter as cf

import color_cases
import color_ref
from abi_text import INCLUDE, ROOT, c_values
from color_ref import LINEAR, SRGB

# The largest deviation of the identity in SRGB space over every finite f16 in [0, 1], in f16 ULP, as the reference gives it
# (DESIGN.md 5.10 quotes it), how many of the 15 361 patterns change at all, and the same for invert(1) applied twice.
SRGB_IDENTITY_ULP, SRGB_IDENTITY_CHANGED = 2, 4694
INVERT_TWICE_ULP_UPPER_HALF = 1
INVERT_TWICE_ULP_ALL = 418


def _h(v):
    return int(np.float16(v).view(np.uint16))


FUNCS = {
    "identity": None,
    "linear": cf.linear(1.5, -0.25),
    "linear_invert": cf.linear(-1.0, 1.0),
    "gamma": cf.gamma(1.1, 2.2, -0.05),
    "gamma_root": cf.gamma(1.0, 1.0 / 2.2, 0.0),
    "gamma_negative_exponent": cf.gamma(0.9, -1.0, 0.1),
    "gamma_huge": cf.gamma(3.0e38, 3.0, 0.0),
    "table_1": cf.table([0.1]), "table_2": cf.table([0.0, 1.0]), "table_3": cf.table([1.0, 0.2, 0.7]),
    "table_64": cf.table(np.linspace(0.0, 1.0, 64) ** 2),
    "discrete_1": cf.discrete([0.3]), "discrete_2": cf.discrete([0.0, 1.0]), "discrete_3": cf.discrete([0.2, 0.9, 0.4]),
    "discrete_64": cf.discrete(np.linspace(1.0, 0.0, 64)),
}


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_tables_equal_the_references_bit_for_bit(built, name):
    """jh_color_tables (library) and jl_color_tables (host twin) against color_ref.tables on all 65 536 entries of every table,
    in both spaces under both clamp settings; `which` is the reference's, a channel whose composition is the identity (here
    channel 1, and every channel of "identity" in LINEAR space) has no table, and a table that does not exist is not written."""
    f = FUNCS[name]
    funcs = (f, None, f, f)
    for space in (LINEAR, SRGB):
        for clamp in (False, True):
            rpre, rpost, rwhich = color_ref.tables(funcs, space, clamp)
            want = (0x7 if space == SRGB else 0) | sum(1 << (4 + i) for i in range(4) if funcs[i] is not None or (space == SRGB and i < 3))
            assert rwhich == want
            for twin in (False, True):
                pre, post, which = jello_amd.color_tables(funcs, ColorSpace(space), clamp, twin=twin)
                assert which == rwhich and sorted(pre) == sorted(rpre) and sorted(post) == sorted(rpost), (name, space, clamp, twin)
                for c in pre:
                    assert np.array_equal(pre[c].view(np.uint32), rpre[c].view(np.uint32)), (name, space, clamp, twin, c)
                for i in post:
                    bad = np.argwhere(post[i] != rpost[i])
                    assert len(bad) == 0, (name, space, clamp, twin, i, len(bad), hex(int(bad[0][0])))


def test_tables_that_do_not_exist_are_left_alone(built):
    L = jello_amd.load_host()
    d = jello_amd.engine._color_desc(None, (None, cf.linear(2.0, 0.0), None, None), ColorSpace.LINEAR, True, None)
    for fn in (L.hip.jh_color_tables, L.jl_color_tables):
        pre, post = np.full((3, 65536), -7.0, np.float32), np.full((4, 65536), 0xDEAD, np.uint16)
        which = ctypes.c_uint32(99)
        assert fn(ctypes.byref(d), pre.ctypes.data, post.ctypes.data, ctypes.byref(which)) == 0
        assert which.value == 1 << 5
        assert np.all(pre == -7.0) and np.all(post[[0, 2, 3]] == 0xDEAD) and not np.any(post[1] == 0xDEAD)
        assert fn(ctypes.byref(d), None, None, ctypes.byref(which)) == 0 and which.value == 1 << 5  # (null pointers: `which` alone)
        assert fn(ctypes.byref(d), None, None, None) == 0


def test_bad_descriptors_are_refused(built):
    L = jello_amd.load_host()
    inf, nan = math.inf, math.nan
    bad = {
        "space 2": dict(space=2), "space -1": dict(space=-1),
        "type 5": dict(funcs=(None, (5, 1.0, 0.0), None, None)), "type -1": dict(funcs=(None, None, None, (-1,))),
        "table of 0": dict(funcs=(cf.table([]), None, None, None)), "discrete of 0": dict(funcs=(None, None, cf.discrete([]), None)),
        "table of 65": dict(funcs=(cf.table([0.5] * 65), None, None, None)), "discrete of 65": dict(funcs=(None, cf.discrete([0.5] * 65), None, None)),
        "slope inf": dict(funcs=(cf.linear(inf, 0.0), None, None, None)), "intercept nan": dict(funcs=(None, None, None, cf.linear(1.0, nan))),
        "amplitude nan": dict(funcs=(cf.gamma(nan, 1.0, 0.0), None, None, None)), "exponent -inf": dict(funcs=(None, cf.gamma(1.0, -inf, 0.0), None, None)),
        "offset inf": dict(funcs=(None, None, cf.gamma(1.0, 1.0, inf), None)), "a table value nan": dict(funcs=(cf.table([0.0, nan, 1.0]), None, None, None)),
        "a discrete value inf": dict(funcs=(None, None, None, cf.discrete([inf]))),
    }
    for what, kw in bad.items():
        d = jello_amd.engine._color_desc(None, kw.get("funcs"), kw.get("space", 0), True, None)
        for fn in (L.hip.jh_color_tables, L.jl_color_tables):
            which = ctypes.c_uint32(77)
            assert fn(ctypes.byref(d), None, None, ctypes.byref(which)) != 0, what
            assert which.value == 77, what
        with pytest.raises(ValueError, match="color_tables: "):
            jello_amd.color_tables(kw.get("funcs"), kw.get("space", 0), True)
    d = jello_amd.engine._color_desc(None, None, 0, True, None)
    d.flags = 2
    for fn in (L.hip.jh_color_tables, L.jl_color_tables):
        assert fn(ctypes.byref(d), None, None, None) != 0
        assert fn(None, None, None, None) != 0
    assert L.hip.jh_color_tables(None, None, None, None) == -1  # JH_ERR_INVALID
    # parameters a func's type does not use are not read
    d = jello_amd.engine._color_desc(None, (cf.linear(1.0, 0.0), None, None, None), 0, True, None)
    d.func[0].exponent, d.func[0].values[3], d.func[1].slope = nan, inf, nan
    assert L.hip.jh_color_tables(ctypes.byref(d), None, None, None) == 0 and L.jl_color_tables(ctypes.byref(d), None, None, None) == 0


def test_the_headers_constants_and_the_mirrors_layout():
    assert c_values(["JH_COLOR_LINEAR", "JH_COLOR_SRGB", "JH_COLOR_CLAMP", "JH_COLOR_MAX_VALUES", "JH_COLOR_TABLE_ENTRIES", "JH_COLOR_FUNC_IDENTITY",
                     "JH_COLOR_FUNC_LINEAR", "JH_COLOR_FUNC_GAMMA", "JH_COLOR_FUNC_TABLE", "JH_COLOR_FUNC_DISCRETE"]) == [0, 1, 1, 64, 65536, 0, 1, 2, 3, 4]
    assert [int(s) for s in ColorSpace] == [LINEAR, SRGB] and [int(f) for f in ColorFunc] == [0, 1, 2, 3, 4]
    assert (jello_amd.engine.COLOR_CLAMP, jello_amd.engine.COLOR_MAX_VALUES) == (1, 64)
    for struct, mirror, fields in (("jh_color_func", _lib.CColorFunc, ["type", "n", "slope", "intercept", "amplitude", "exponent", "offset", "values"]),
                                   ("jh_color_desc", _lib.CColorDesc, ["x", "y", "width", "height", "matrix", "space", "flags", "func"])):
        assert [name for name, _ in mirror._fields_] == fields
        want = c_values(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, f) for f in fields])
        assert [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, struct


def test_the_sanitizer_stand_in_compiles(tmp_path):
    """tools/color_tables_check.cpp is include/jello_color.h with a main of its own; it is run by hand (its header has the command
    with the sanitizers), here it only has to compile."""
    exe = str(tmp_path / "color_tables_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", INCLUDE, os.path.join(ROOT, "tools", "color_tables_check.cpp"),
                           "-o", exe])
    assert os.path.exists(exe)


# ---- the reference against the definition ----

_DEFINITION_CASES = {
    "dense linear": dict(matrix=color_cases.DENSE, funcs=None, space=LINEAR),
    "dense srgb": dict(matrix=color_cases.DENSE, funcs=None, space=SRGB),
    "grayscale": dict(cf.grayscale(1.0), space=SRGB),
    "sepia half": dict(cf.sepia(0.5), space=SRGB),
    "hue 90": dict(cf.hue_rotate(90.0), space=SRGB),
    "invert": dict(cf.invert(1.0), space=SRGB),
    "brightness 2": dict(cf.brightness(2.0), space=SRGB),
    "contrast half": dict(cf.contrast(0.5), space=SRGB),
    "contrast 2.7 linear": dict(matrix=None, funcs=(cf.linear(2.7, -0.85),) * 3 + (None,), space=LINEAR),
    "luminance to alpha": dict(cf.luminance_to_alpha(), space=LINEAR),
}


@pytest.mark.parametrize("name", sorted(_DEFINITION_CASES))
def test_reference_against_the_definition(name):
    """color_ref.texels against color_ref.definition (the rule's formulas wholly in binary64, nothing rounded on the way) on 20 000
    random texels in [0, 1] with the clamp on, IDENTITY and LINEAR funcs.  The bound, absolute, from the rule's roundings -- with
    A_i = |M[i][4]| + the sum of |M[i][k]|, which bounds every partial sum of row i because every t is in [0, 1]; S_i the |slope| of
    func_i (1 for IDENTITY); L the largest slope of dec on [0, 1], dec'(1) = 2.4 / 1.055 (1 in LINEAR space and for alpha):
      each PRE entry     one binary32 rounding of a value <= 1: 2^-25 each, 2^-25 A_i into row i                 (SRGB space only)
      four fused steps   each rounds a partial sum of magnitude <= A_i once: 4 x 2^-24 A_i
      the clamp          1-Lipschitz, adds nothing
      g = f16(m)         m in [0, 1]: half an f16 ULP below 1, 2^-12
      POST_i             func, clamp and dec are exact up to binary64 (allowed 2^-40) and carry the error e of their input to at most
                         L S_i e; the entry is rounded to f16 once: 2^-12                                         (where a table exists)
      bound_i = L S_i (A_i (2^-25 [SRGB] + 2^-22) + 2^-12) + 2^-12 [table] + 2^-40.
    The part of the bound that is used is printed; the bound was derived before the first run."""
    kw = _DEFINITION_CASES[name]
    rng = np.random.default_rng(77)
    bits = rng.uniform(0.0, 1.0, (20000, 4)).astype(np.float16).view(np.uint16)
    got = color_ref.texels(bits, kw["matrix"], kw["funcs"], kw["space"], True).view(np.float16).astype(np.float64)
    want = color_ref.definition(bits, kw["matrix"], kw["funcs"], kw["space"], True)
    M = np.asarray(color_ref.IDENTITY if kw["matrix"] is None else kw["matrix"], np.float32).astype(np.float64).reshape(4, 5)
    funcs = (None,) * 4 if kw["funcs"] is None else kw["funcs"]
    srgb = kw["space"] == SRGB
    used = 0.0
    for i in range(4):
        A = np.abs(M[i]).sum()
        S = 1.0 if funcs[i] is None else abs(float(np.float32(funcs[i][1])))
        L = 2.4 / 1.055 if srgb and i < 3 else 1.0
        table = funcs[i] is not None or (srgb and i < 3)
        bound = L * S * (A * ((2.0 ** -25 if srgb else 0.0) + 2.0 ** -22) + 2.0 ** -12) + (2.0 ** -12 if table else 0.0) + 2.0 ** -40
        err = np.abs(got[:, i] - want[:, i]).max()
        used = max(used, err / bound)
        assert err <= bound, (name, i, err, bound)
    print("%s: %.3f of the bound used" % (name, used))


# ---- the constructors against the specification's numbers ----

def _m(kw):
    return np.asarray(kw["matrix"], np.float32).reshape(4, 5)


def _f32(rows):
    return np.array(rows, np.float64).astype(np.float32)


def _within_one_ulp32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)))


def test_constructors_against_the_specifications_numbers():
    alpha_row = _f32([0, 0, 0, 1, 0])
    g = _m(cf.grayscale(1.0))
    assert np.array_equal(g[0], _f32([0.2126, 0.7152, 0.0722, 0, 0])) and np.array_equal(g[1], g[0]) and np.array_equal(g[2], g[0])
    assert np.array_equal(g[3], alpha_row)
    assert _within_one_ulp32(_m(cf.grayscale(0.0)), np.asarray(color_ref.IDENTITY, np.float32).reshape(4, 5))
    assert np.array_equal(_m(cf.grayscale(7.0)), g)  # (the amount is clamped to [0, 1])
    assert np.array_equal(_m(cf.sepia(1.0))[:3], _f32([[0.393, 0.769, 0.189, 0, 0], [0.349, 0.686, 0.168, 0, 0], [0.272, 0.534, 0.131, 0, 0]]))
    assert _within_one_ulp32(_m(cf.saturate(0.0)), g)
    assert _within_one_ulp32(_m(cf.saturate(1.0)), np.asarray(color_ref.IDENTITY, np.float32).reshape(4, 5))
    assert _within_one_ulp32(_m(cf.hue_rotate(0.0)), np.asarray(color_ref.IDENTITY, np.float32).reshape(4, 5))
    # hueRotate at 180 degrees, expanded by hand: cos = -1, sin = 0 (1.2e-16 in binary64: below a binary32 ULP of every entry) --
    # a00 = 0.213 - 0.787, a01 = 0.715 + 0.715, a02 = 0.072 + 0.072; a10 = 0.213 + 0.213, a11 = 0.715 - 0.285, a12 = 0.144;
    # a20 = 0.426, a21 = 1.430, a22 = 0.072 - 0.928
    assert _within_one_ulp32(_m(cf.hue_rotate(180.0))[:3, :3], _f32([[-0.574, 1.430, 0.144], [0.426, 0.430, 0.144], [0.426, 1.430, -0.856]]))
    assert np.all(_m(cf.hue_rotate(180.0))[:3, 3:] == 0.0)
    la = cf.luminance_to_alpha()
    assert np.array_equal(_m(la)[3], _f32([0.2125, 0.7154, 0.0721, 0, 0])) and np.all(_m(la)[:3] == 0.0)
    assert la["space"] == ColorSpace.LINEAR and la["funcs"] is None and la["clamp"] is True
    for kw in (cf.grayscale(1), cf.sepia(1), cf.saturate(2), cf.hue_rotate(30), cf.invert(1), cf.brightness(2), cf.contrast(2)):
        assert kw["space"] == ColorSpace.SRGB and kw["clamp"] is True
    lin, none = ColorFunc.LINEAR, None
    assert cf.invert(1.0)["funcs"] == ((lin, -1.0, 1.0),) * 3 + (none,) and cf.invert(1.0)["matrix"] is None
    assert cf.invert(0.25)["funcs"][0] == (lin, 0.5, 0.25)
    assert cf.opacity(0.4)["funcs"] == (none, none, none, (lin, 0.4, 0.0)) and cf.opacity(0.4)["space"] == ColorSpace.LINEAR
    assert cf.opacity(3.0)["funcs"][3] == (lin, 1.0, 0.0)
    assert cf.brightness(2.0)["funcs"] == ((lin, 2.0, 0.0),) * 3 + (none,)
    assert cf.contrast(0.5)["funcs"] == ((lin, 0.5, 0.25),) * 3 + (none,) and cf.contrast(2.0)["funcs"][0] == (lin, 2.0, -0.5)
    t = _m(cf.tint((0.1, 0.2, 0.9, 0.5)))
    assert np.array_equal(t, _f32([[0, 0, 0, 0, 0.1], [0, 0, 0, 0, 0.2], [0, 0, 0, 0, 0.9], [0, 0, 0, 0.5, 0]]))


# ---- consequences of the rule ----

def test_the_identity_in_linear_space():
    """The identity matrix, LINEAR space, IDENTITY funcs, no clamp, on every f16 bit pattern in one channel next to finite
    neighbours: no table exists, and the pattern comes back unchanged -- except that every NaN comes back as 0x7e00 and -0 as +0
    (m starts at the offset +0, and fmaf(1, -0, +0) is +0).  +-Inf come back themselves; the OTHER channels of that texel become
    NaN (0 x Inf in their rows), as they do beside a NaN."""
    assert color_ref.tables(None, LINEAR, False)[2] == 0 and color_ref.tables(None, LINEAR, True)[2] == 0
    h = color_ref.ALL16
    nan = (h & 0x7FFF) > 0x7C00
    for ch in range(4):
        tex = np.full((65536, 4), 0x3800, np.uint16)
        tex[:, ch] = h
        out = color_ref.texels(tex, None, None, LINEAR, False)
        want = np.where(nan, 0x7E00, np.where(h == 0x8000, 0, h)).astype(np.uint16)
        assert np.array_equal(out[:, ch], want)
        nonfinite = (h & 0x7C00) == 0x7C00
        others = [c for c in range(4) if c != ch]
        assert np.all(out[nonfinite][:, others] == 0x7E00) and np.all(out[~nonfinite][:, others] == 0x3800)


def _unit_patterns():
    hs = np.arange(0, 0x3C01, dtype=np.uint16)  # every finite f16 in [0, 1]
    return hs, np.stack([hs, hs, hs, np.full_like(hs, 0x3C00)], -1)


def test_the_identity_in_srgb_space_is_not_exact():
    """g = f16(enc(x)) and then f16(dec(g)): two roundings to f16 around a curve.  The largest deviation over every finite f16 in
    [0, 1], in f16 ULP (the difference of the bit patterns), is asserted to be what this file records -- DESIGN.md 5.10 quotes
    it -- and nothing else is claimed of it.  Alpha, which is never encoded, is exact."""
    hs, tex = _unit_patterns()
    out = color_ref.texels(tex, None, None, SRGB, True)
    dev = np.abs(out[:, :3].astype(np.int32) - tex[:, :3].astype(np.int32))
    print("identity in SRGB space: largest deviation %d ULP, %d of %d patterns change" % (dev.max(), (dev[:, 0] != 0).sum(), len(hs)))
    assert dev.max() == SRGB_IDENTITY_ULP and (dev[:, 0] != 0).sum() == SRGB_IDENTITY_CHANGED
    assert np.array_equal(out[:, 3], tex[:, 3])
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 0], out[:, 2])


def test_invert_twice():
    """invert(1) applied twice returns the input within the deviation recorded above -- on [0.5, 1], where it can: there the f16
    grid of the input (2^-11 wide) is the grid of the encoded values, so 1 - g is exact and each pass costs what the identity costs.
    FIGURES, for the sentence does not hold below that: a dark x becomes 1 - enc(x), close to 1, and is rounded on the 2^-11 grid
    there; brought back, that half-step of 2^-12 is hundreds of the ULPs of x (the f16 ULP of 0.001 is 2^-20).  Over every finite
    f16 in [0, 1] the reference's largest deviation is 418 ULP; it is asserted as measured, like the identity's, so that a change
    of the rule shows."""
    hs, tex = _unit_patterns()
    kw = dict(cf.invert(1.0), space=SRGB)
    out = color_ref.texels(color_ref.texels(tex, **kw), **kw)
    dev = np.abs(out[:, 0].astype(np.int32) - tex[:, 0].astype(np.int32))
    upper = hs >= 0x3800
    print("invert twice: largest deviation %d ULP on [0.5, 1], %d ULP on [0, 1] (at %#06x)" % (dev[upper].max(), dev.max(), hs[dev.argmax()]))
    assert dev[upper].max() <= SRGB_IDENTITY_ULP and dev[upper].max() == INVERT_TWICE_ULP_UPPER_HALF
    assert dev.max() == INVERT_TWICE_ULP_ALL
    assert np.array_equal(out[:, 3], tex[:, 3])


def test_the_clamp_sends_nan_to_zero():
    nans = np.array([[0x7E00, 0x7C01, 0xFFFF, 0xFE00]], np.uint16)
    assert np.array_equal(color_ref.texels(nans, None, None, LINEAR, True), [[0, 0, 0, 0]])
    assert np.array_equal(color_ref.texels(nans, None, None, LINEAR, False), [[0x7E00] * 4])
    # in SRGB space the POST tables see the clamped 0: dec(0) = 0
    assert np.array_equal(color_ref.texels(nans, None, None, SRGB, True), [[0, 0, 0, 0]])
    assert np.array_equal(color_ref.texels(nans, None, None, SRGB, False), [[0x7E00] * 4])
    # and -0: an offset of -0 under zero coefficients and a negative input is m = -0, which the clamp sends to +0
    m = (0.0,) * 4 + (-0.0,) + color_ref.IDENTITY[5:]
    tex = np.array([[0xBC00, 0xBC00, 0xBC00, 0xBC00]], np.uint16)
    assert color_ref.texels(tex, m, None, LINEAR, False)[0, 0] == 0x8000 and color_ref.texels(tex, m, None, LINEAR, True)[0, 0] == 0


def test_hand_values():
    """Texels worked by hand (f16 patterns: 0.5 = 0x3800, 1 = 0x3c00, 0.25 = 0x3400; the f16 grid is 2^-11 wide in [0.5, 1)).
    1. (0.5, 0.5, 0.5, 1) through grayscale(1), SRGB: enc(0.5) = 1.055 x 0.5^(1/2.4) - 0.055 = 0.73535698..., the same binary32 t
       in r, g, b; each row is 0.2126 t + 0.7152 t + 0.0722 t = t within a few binary32 ULP; t x 2048 = 1506.01, so g = 1506 / 2048 =
       0.73535156 = 0x39e2; POST: dec(g) = ((g + 0.055) / 1.055)^2.4 = 0.4999918, and the f16 grid below 0.5 is 2^-12 wide:
       x 4096 = 2047.97 -> 2048 -> 0.5 = 0x3800.  Alpha: 1 -> 0x3c00.  The texel comes back as it was.
    2. (1, 0.5, 0.25, 1) through luminance_to_alpha, LINEAR: colour rows are zero -> 0; alpha = 0.2125 + 0.7154 x 0.5 + 0.0721 x
       0.25 = 0.588225; x 2048 = 1204.68 -> 1205 -> 0x3800 + 181 = 0x38b5.
    3. (-0, 1, 2^-24, -2) through the identity, LINEAR, no clamp: (+0, 1, 2^-24, -2) = (0x0000, 0x3c00, 0x0001, 0xc000).
    4. (0, 1, 0.5, 1) through invert(1), SRGB: r: enc(0) = 0, g = 0, POST: 1 - 0 = 1, dec(1) = 1 -> 0x3c00.  g: enc(1) = 1 (as
       binary32), g = 1, POST: 1 - 1 = 0 -> 0.  b: g = 0x39e2 as in 1; 1 - 0.73535156 = 0.26464844; dec = ((0.26464844 + 0.055) /
       1.055)^2.4 = 0.0569388; the f16 grid in [2^-5, 2^-4) is 2^-15 wide: x 32768 = 1865.77 -> 1866 = 1024 + 842 -> exponent field 10,
       0x2800 + 0x34a = 0x2b4a.  Alpha 1.
    5. (Inf, 0, 0, 1) through the identity, LINEAR: row r is 1 x Inf = Inf; rows g, b and a hold 0 x Inf = NaN.  With the clamp:
       (1, 0, 0, 0) = (0x3c00, 0, 0, 0); without: (0x7c00, 0x7e00, 0x7e00, 0x7e00).
    6. (0.7, 0.7, 0.7, 0.5) through tint((0.1, 0.2, 0.9, 0.5)): colour = the offsets, f16(0.1f) = 0x2e66, f16(0.2f) = 0x3266,
       f16(0.9f) = 0x3b33; alpha = 0.5 x 0.5 = 0.25 = 0x3400.
    7. (0.25, 0.25, 0.25, 1) through brightness(2), SRGB: enc(0.25) = 0.5370987, g = 0x384c = 0.53710938; POST: 2 g = 1.0742 -> clamp
       1 -> dec(1) = 1 -> 0x3c00."""
    def run(texel, kw):
        return [int(v) for v in color_ref.texels(np.array([texel], np.uint16), kw["matrix"], kw["funcs"], int(kw["space"]), kw["clamp"])[0]]
    plain = dict(matrix=None, funcs=None, space=LINEAR)
    assert abs(color_ref.enc(0.5) - 0.73535698) < 1e-8 and abs(color_ref.dec(1506 / 2048) - 0.4999918) < 1e-7
    assert run([0x3800, 0x3800, 0x3800, 0x3C00], cf.grayscale(1.0)) == [0x3800, 0x3800, 0x3800, 0x3C00]
    assert run([0x3C00, 0x3800, 0x3400, 0x3C00], cf.luminance_to_alpha()) == [0, 0, 0, 0x38B5]
    assert run([0x8000, 0x3C00, 0x0001, 0xC000], dict(plain, clamp=False)) == [0x0000, 0x3C00, 0x0001, 0xC000]
    assert run([0x0000, 0x3C00, 0x3800, 0x3C00], cf.invert(1.0)) == [0x3C00, 0x0000, 0x2B4A, 0x3C00]
    assert run([0x7C00, 0, 0, 0x3C00], dict(plain, clamp=True)) == [0x3C00, 0, 0, 0]
    assert run([0x7C00, 0, 0, 0x3C00], dict(plain, clamp=False)) == [0x7C00, 0x7E00, 0x7E00, 0x7E00]
    assert run([_h(0.7)] * 3 + [0x3800], cf.tint((0.1, 0.2, 0.9, 0.5))) == [0x2E66, 0x3266, 0x3B33, 0x3400]
    assert run([0x3400, 0x3400, 0x3400, 0x3C00], cf.brightness(2.0)) == [0x3C00, 0x3C00, 0x3C00, 0x3C00]


# ---- the battery has teeth ----

_DISTINGUISHABLE = [v for v in color_ref.VARIANTS if v != "clamp_after_round"]
_EXPECTED = {}


def _expected(name):
    """The reference on a value case, computed once for the tests of this file."""
    if name not in _EXPECTED:
        _EXPECTED[name] = color_ref.texels(color_cases.VALUES, **color_cases.VALUE_CASES[name])
    return _EXPECTED[name]


@pytest.mark.parametrize("variant", _DISTINGUISHABLE)
def test_the_battery_tells_the_rule_from_a_near_miss(variant):
    """Each wrong variant -- the offset added last, multiply and add unfused, enc applied to alpha, the func applied after dec, a
    clamp of min and max that hand a NaN on -- differs from the reference in at least one texel of at least one value case of
    the battery."""
    telling = []
    for name, kw in color_cases.VALUE_CASES.items():
        want = color_ref.texels(color_cases.VALUES, **kw)
        got = color_ref.texels(color_cases.VALUES, variant=variant, **kw)
        if not np.array_equal(got, want):
            telling.append((name, int((got != want).sum())))
    print(variant, "told apart by", len(telling), "of", len(color_cases.VALUE_CASES), "cases; the first:", telling[:3])
    assert telling


def test_a_clamp_after_the_rounding_is_the_same_rule():
    """The sixth near miss of the list cannot be told from the rule, by any battery: 0 and 1 are f16 values and rounding to nearest
    is monotone, so f16(clamp(m)) = clamp(f16(m)) for every m that is not NaN (a tiny negative m gives +0 either way: the clamp
    of the rounded -0 is +0), and a NaN becomes +0 on both routes.  Asserted on the battery, so that the claim is checked."""
    for name, kw in color_cases.VALUE_CASES.items():
        assert np.array_equal(color_ref.texels(color_cases.VALUES, variant="clamp_after_round", **kw), _expected(name)), name


def test_the_battery_covers_what_it_claims():
    v = color_cases.VALUES
    assert v.shape == (352, 256, 4)
    for c in range(4):
        assert len(np.unique(v[:256, :, c])) == 65536
    assert not np.array_equal(v[:256, :, 0], v[:256, :, 1])
    names = set(color_cases.VALUE_CASES)
    assert {"identity_clamp", "identity_free", "dense_clamp", "hostile_free", "grayscale", "sepia", "hue_rotate_90", "invert", "brightness_2",
            "contrast_half", "luminance_to_alpha", "gamma_srgb_clamp", "table_linear_free", "discrete_srgb_free", "linear_linear_clamp"} <= names
    table_free = [n for n, kw in color_cases.VALUE_CASES.items() if color_ref.tables(kw["funcs"], kw["space"], kw["clamp"])[2] == 0]
    assert {"identity_clamp", "dense_free", "hostile_clamp", "luminance_to_alpha", "tint"} <= set(table_free) and len(table_free) < len(names) / 2
    # the hostile matrix reaches Inf, NaN and m = -0 on the image
    out = color_ref.texels(v, **color_cases.VALUE_CASES["hostile_free"])
    assert (out == 0x7C00).any() and (out == 0xFC00).any() and (out == 0x7E00).any() and (out == 0x8000).any()
    assert color_cases.WIDTHS == (1, 2, 3, 511, 512, 513, 1025) and color_cases.HEIGHTS == (1, 3)
    for w in color_cases.WIDTHS:
        g = color_cases.geometry(w)
        assert {c["rect"][0] % 2 for c in g} == {0, 1} and {c["size"][0] % 2 for c in g} == {0, 1} and {c["tables"] for c in g} == {False, True}
