"""The context-free queries of the image calls (include/jello_queries.h) on the CPU: the library's jh_<name> and the host twin's
jl_<name> against each other.  For every query one legal input and every class of refusal its body has -- a null for each pointer
argument, one illegal value per reason of the rule header's legality check -- and on each input: the two return the same code; on a
legal input they write the same bytes; on a refusal they leave every output as it was; and jl_last_error() is the twin's text.

The expected texts are those of the hand-written twins that host/capi.cpp held before the queries had one body ("<name>: " in
front of the rule header's reason), written out here and not derived from jello_queries.h.  resample_taps' second text, "a window
without taps", has no input: the rule has no window without taps."""
import ctypes
import math

import pytest

from jello_amd import _lib
from jello_amd._lib import CColorDesc, CLightingDesc, CLightPlan, CTurbPlan, CTurbulenceDesc

from abi_text import header_arity

FILL = 0xA5
u32, i64, f32, f64 = ctypes.c_uint32, ctypes.c_int64, ctypes.c_float, ctypes.c_double


def _out(ctype, n=1):
    """An output of exactly n entries, every byte FILL."""
    a = (ctype * n)()
    ctypes.memset(a, FILL, ctypes.sizeof(a))
    return a


def _untouched(a):
    return bytes(a) == bytes([FILL]) * ctypes.sizeof(a)


class Out:
    """Marks an argument as an output: a fresh buffer for each of the two libraries."""
    def __init__(self, ctype, n=1):
        self.ctype, self.n = ctype, n


# ---- the legal inputs ----

def _color(space=1, flags=1, funcs=((1, {"slope": 0.5, "intercept": 0.25}), None, None, (3, {"n": 2, "values": (0.0, 1.0)}))):
    d = CColorDesc()
    d.space, d.flags = space, flags
    for i, f in enumerate(funcs):
        if f is None:
            continue
        d.func[i].type = f[0]
        for k, v in f[1].items():
            if k == "values":
                d.func[i].values[:len(v)] = v
            else:
                setattr(d.func[i], k, v)
    return d


def _light(**fields):
    """A specular spot light with both exponents above 1: every field of the descriptor is looked at, both tables exist."""
    d = CLightingDesc()
    d.kind, d.light, d.surface_scale, d.constant, d.specular_exponent, d.spot_exponent = 1, 2, 2.0, 0.75, 3.0, 2.0
    d.color[:] = (1.0, 0.5, 0.25)
    d.direction[:] = (0.0, 0.0, 1.0)
    d.position[:] = (10.0, 20.0, 30.0)
    d.points_at[:] = (0.0, 0.0, 0.0)
    d.cone_cos = 0.5
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


def _turb(**fields):
    """Stitched turbulence of three octaves: the tile is looked at."""
    d = CTurbulenceDesc()
    d.kind, d.octaves, d.seed, d.stitch = 1, 3, 7, 1
    d.base_frequency[:] = (0.05, 0.03)
    d.tile[:] = (0.0, 0.0, 64.0, 48.0)
    d.origin[:] = (3.0, -2.0)
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


def _m(*m):
    return (f64 * 6)(*m)


# query -> (legal arguments, indices of the pointer arguments a null is legal for)
LEGAL = {
    "blur_taps": ([1.5, Out(f32, 11), Out(u32)], {1, 2}),  # (R = ceil(4.5) = 5: 11 taps)
    "resample_taps": ([3, 100, 37, 5, Out(f32, 96), Out(u32), Out(u32)], {4, 5, 6}),
    "color_tables": ([_color(), Out(f32, 3 * 65536), Out(ctypes.c_uint16, 4 * 65536), Out(u32)], {1, 2, 3}),
    "warp_plan": ([_m(2.0, 0.5, -0.25, 1.5, 3.0, -7.0), Out(i64, 6)], set()),
    "warp_bounds": ([_m(2.0, 0.5, -0.25, 1.5, 3.0, -7.0), 40, 30, 2, 100, 90, Out(u32, 4)], set()),
    "convolve_weights": ([3, 2, (f64 * 6)(1.0, 2.0, 3.0, 4.0, 5.0, 6.5), 0.0, Out(f32, 6)], set()),
    "lighting_plan": ([_light(), Out(CLightPlan)], set()),
    "lighting_tables": ([_light(), Out(f32, 4097), Out(f32, 4097), Out(u32)], {1, 2, 3}),
    "turbulence_plan": ([_turb(), Out(CTurbPlan)], set()),
    "turbulence_tables": ([_turb(), Out(ctypes.c_uint8, 256), Out(f32, 2048)], {1, 2}),
    "displace_offset": ([12.5, 0x3A00, Out(i64)], set()),
}
NULL_TEXT = {"color_tables": "null descriptor", "lighting_tables": "null descriptor", "turbulence_tables": "null descriptor"}

# ---- the refusals of the rule headers: (what replaces which legal argument, the reason) ----

MATRIX = [
    (_m(math.nan, 0.0, 0.0, 1.0, 0.0, 0.0), "a matrix entry is not finite"),
    (_m(1e200, 0.0, 0.0, 1e200, 0.0, 0.0), "the determinant is not finite"),
    (_m(1.0, 2.0, 2.0, 4.0, 0.0, 0.0), "the determinant is 0"),
    (_m(1.0, 0.0, 0.0, 1.0 / 65.0, 0.0, 0.0), "an inverse coefficient above 64 (a minification beyond 64:1)"),
    (_m(1.0, 0.0, 0.0, 1.0, 2.0 ** 22 + 1.0, 0.0), "an inverse offset above 2^22"),
]
COLOR = [
    (_color(space=2), "unknown colour space"),
    (_color(flags=2), "unknown flag bits"),
    (_color(funcs=(None, (5, {}), None, None)), "unknown func type"),
    (_color(funcs=(None, None, (3, {"n": 0}), None)), "a func has no values or more than 64"),
    (_color(funcs=(None, None, (4, {"n": 65}), None)), "a func has no values or more than 64"),
    (_color(funcs=((1, {"slope": math.nan, "intercept": 0.0}), None, None, None)), "a func parameter is not finite"),
    (_color(funcs=(None, (2, {"amplitude": 1.0, "exponent": math.inf, "offset": 0.0}), None, None)), "a func parameter is not finite"),
    (_color(funcs=(None, None, None, (3, {"n": 2, "values": (0.0, math.nan)}))), "a func parameter is not finite"),
]
LIGHT = [
    (_light(kind=2), "unknown kind"),
    (_light(light=3), "unknown light"),
    (_light(surface_scale=math.inf), "the surface_scale is not finite"),
    (_light(constant=-1.0), "the constant is negative or not finite"),
    (_light(specular_exponent=129.0), "the specular_exponent is outside [1, 128]"),
    (_light(color=(1.0, -0.5, 1.0)), "a color component is negative or not finite"),
    (_light(light=0, direction=(0.0, math.nan, 1.0)), "the direction is not finite"),
    (_light(light=0, direction=(0.0, 0.0, 0.0)), "the direction has no finite non-zero length"),
    (_light(position=(0.0, 1e39, 0.0)), "the position is not finite in binary32"),
    (_light(points_at=(math.inf, 0.0, 0.0)), "points_at is not finite"),
    (_light(points_at=(10.0, 20.0, 30.0)), "points_at is the position, or too far from it"),
    (_light(spot_exponent=0.5), "the spot_exponent is outside [1, 128]"),
    (_light(cone_cos=1.5), "the cone_cos is outside [-1, 1]"),
]
TURB_DESC = [
    (_turb(kind=2), "unknown kind"),
    (_turb(octaves=17), "more than 16 octaves"),
    (_turb(stitch=2), "stitch is neither 0 nor 1"),
    (_turb(base_frequency=(0.05, -0.03)), "a base_frequency is negative or not finite"),
    (_turb(origin=(math.inf, 0.0)), "the origin is not finite"),
    (_turb(tile=(0.0, math.nan, 64.0, 48.0)), "the stitch tile is not finite"),
    (_turb(tile=(0.0, 0.0, 64.0, 0.0)), "the stitch tile is empty"),
]
TURB_PLAN = [  # (refused by jturb_plan alone: turbulence_tables does not look at the position range)
    (_turb(base_frequency=(1.0, 1.0), tile=(0.0, 0.0, 1e-320, 48.0)), "the stitched frequency is not finite"),
    (_turb(stitch=0, base_frequency=(2.0 ** 30, 0.0)), "a base_frequency of 2^30 cells per texel or more"),
    (_turb(stitch=0, octaves=1, base_frequency=(1.0, 1.0), origin=(2.0 ** 31, 0.0)), "the origin is beyond the position range"),
    (_turb(stitch=0, octaves=16, base_frequency=(1.0, 1.0), origin=(2.0 ** 20, 0.0)), "the origin is beyond the position range of this many octaves"),
    (_turb(octaves=1, base_frequency=(1.0, 1.0), origin=(0.0, 0.0), tile=(0.0, 0.0, 2.0 ** 32, 48.0)), "the stitch tile is beyond the lattice range"),
    (_turb(octaves=16, base_frequency=(1.0, 1.0), origin=(0.0, 0.0), tile=(0.0, 0.0, 2.0 ** 17, 48.0)),
     "the stitch tile is beyond the lattice range of this many octaves"),
]
RESAMPLE_TEXT = "unknown filter, sizes outside 1 <= n_in <= 16 n_out, or an index outside the axis"
ILLEGAL = {
    # query -> [({index: value}, reason)]
    "blur_taps": [({0: v}, "sigma is negative, above 64 or NaN") for v in (-1.0, 64.5, math.nan)],
    "resample_taps": [({0: 4}, RESAMPLE_TEXT), ({0: -1}, RESAMPLE_TEXT), ({1: 0}, RESAMPLE_TEXT), ({1: 16 * 37 + 1}, RESAMPLE_TEXT), ({3: 37}, RESAMPLE_TEXT)],
    "color_tables": [({0: d}, why) for d, why in COLOR],
    "warp_plan": [({0: m}, why) for m, why in MATRIX],
    "warp_bounds": [({0: m}, why) for m, why in MATRIX] + [({3: 3}, "unknown filter"), ({3: -1}, "unknown filter")] +
                   [({i: 32769}, "an image side above 32768") for i in (1, 2, 4, 5)],
    "convolve_weights": [
        ({0: 0}, "an order outside 1..15"),
        ({1: 16}, "an order outside 1..15"),
        ({3: math.inf}, "the divisor is not finite"),
        ({2: (f64 * 6)(1.0, 2.0, math.nan, 4.0, 5.0, 6.0)}, "a kernelMatrix entry is not finite"),
        ({2: (f64 * 6)(1e308, 1e308, 0.0, 0.0, 0.0, 0.0)}, "the sum of kernelMatrix is not finite"),
        # (the weights are written in order, so only an overflow of the first one, the matrix's last entry, leaves them untouched)
        ({2: (f64 * 6)(0.0, 0.0, 0.0, 0.0, 0.0, 1e300), 3: 1.0}, "a weight does not come out finite"),
    ],
    "lighting_plan": [({0: d}, why) for d, why in LIGHT],
    "lighting_tables": [({0: d}, why) for d, why in LIGHT],
    "turbulence_plan": [({0: d}, why) for d, why in TURB_DESC + TURB_PLAN],
    "turbulence_tables": [({0: d}, why) for d, why in TURB_DESC],
    "displace_offset": [],  # (every scale and every bit pattern has an offset)
}


def _cases():
    out = []
    for name, (args, optional) in LEGAL.items():
        out.append(pytest.param(name, {}, None, id=name + "-legal"))
        for i, a in enumerate(args):
            if isinstance(a, (Out, ctypes.Array, ctypes.Structure)):
                why = None if i in optional else NULL_TEXT.get(name, "null argument")
                out.append(pytest.param(name, {i: None}, why, id="%s-null%d" % (name, i)))
        for k, (change, why) in enumerate(ILLEGAL[name]):
            out.append(pytest.param(name, change, why, id="%s-illegal%d" % (name, k)))
    return out


def _call(f, args):
    """f on args, every Out a fresh buffer: (code, the buffers)."""
    outs = [_out(a.ctype, a.n) for a in args if isinstance(a, Out)]
    it = iter(outs)
    return f(*[next(it) if isinstance(a, Out) else a for a in args]), outs


@pytest.mark.parametrize("name, change, why", _cases())
def test_the_library_and_the_twin_answer_alike(built, name, change, why):
    L = _lib.load_host()
    args = list(LEGAL[name][0])
    for i, v in change.items():
        args[i] = v
    inputs = [bytes(a) for a in args if isinstance(a, (ctypes.Array, ctypes.Structure))]
    jh_code, jh_outs = _call(getattr(L.hip, "jh_" + name), args)
    jl_code, jl_outs = _call(getattr(L, "jl_" + name), args)
    assert jh_code == jl_code == (0 if why is None else -1)
    assert [bytes(a) for a in jh_outs] == [bytes(a) for a in jl_outs]
    assert [bytes(a) for a in args if isinstance(a, (ctypes.Array, ctypes.Structure))] == inputs
    if why is None:
        assert jh_outs and not any(_untouched(a) for a in jh_outs)
    else:
        assert all(_untouched(a) for a in jh_outs)
        assert L.jl_last_error().decode() == "%s: %s" % (name, why)


def test_the_case_list_covers_every_query_of_the_table(built):
    assert set(LEGAL) == set(ILLEGAL) and len(LEGAL) == 11
    L = _lib.load_host()
    arity = header_arity()
    for name in LEGAL:
        assert getattr(L, "jl_" + name).argtypes == getattr(L.hip, "jh_" + name).argtypes
        assert len(getattr(L.hip, "jh_" + name).argtypes) == len(LEGAL[name][0]) == arity["jh_" + name]  # (jello_hip.h's declaration)
    assert not hasattr(L.hip, "jh_composite_clip")


# ---- composite_clip: the host library's alone ----

CLIP_TEXT = "composite_clip: the source rectangle is not inside the source image or is empty in one dimension"


@pytest.mark.parametrize("args, want", [
    ((40, 30, 4, 5, 20, 10, -3, 7, 64, 12), (7, 5, 0, 7, 17, 5)),
    ((40, 30, 0, 0, 0, 0, 100, 0, 64, 12), (0, 0, 0, 0, 0, 0)),  # (placed outside: legal, nothing left)
    ((40, 30, 30, 5, 20, 10, 0, 0, 64, 12), None),  # (not inside the source)
    ((40, 30, 4, 5, 0, 10, 0, 0, 64, 12), None),  # (empty in one dimension)
])
def test_composite_clip(built, args, want):
    L = _lib.load_host()
    out = _out(u32, 6)
    assert L.jl_composite_clip(*args, out) == (0 if want else -1)
    if want:
        assert tuple(out) == want
    else:
        assert _untouched(out) and L.jl_last_error().decode() == CLIP_TEXT
    assert L.jl_composite_clip(*args, None) == -1 and L.jl_last_error().decode() == CLIP_TEXT
