"""CPU: what a pixel is painted with -- gradient ramps, the gradient parameter of every kind and route, the extend modes,
images -- on the oracle's image against the float64 reference of tests/exact_paint.py, on the battery of
tests/paint_cases.py, with the bounds that tests/test_gpu_paint.py derives (its docstring holds the table) and holds on
the HIP image.  Also here: the ramps that make_ramp uploads against the rule bit for bit, consequences of the rule worked
by hand, the near misses of the rule that the battery must tell from it, and the ramp cache over several recordings of
one Host."""
import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, ColorStop, Fill, Host, Path, RenderParams, Scene
from oracle.oracle_engine import OracleEngine

import exact_paint as P
import kat_scenes as K
import paint_cases as C

_RENDERS = {}


def oracle_render(case):
    """(image, ramp rows) of a case on the oracle, rendered once per session and left unchanged."""
    if case.name not in _RENDERS:
        rec = Host().record(case.scene(), case.params())
        o = OracleEngine()
        o.run(rec)
        img = o.target(rec).copy()
        img.setflags(write=False)
        _RENDERS[case.name] = (img, K.ramp_rows(rec).copy() if case.ramps() else None)
    return _RENDERS[case.name]


def uploaded_ramp(stops):
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.linear((0, 0), (8, 0), [ColorStop(o, c) for o, c in stops]), None, Path.rect(0, 0, 8, 8))
    rows = K.ramp_rows(Host().record(s, RenderParams(8, 8)))
    assert rows.shape == (1, 512, 4)
    return rows[0]


def f16_bits(v):
    return int(np.float16(np.float32(v)).view(np.uint16))


@pytest.mark.parametrize("name", list(C.RAMPS))
def test_ramp_bit_for_bit(built, name):
    """make_ramp's upload against the numpy restatement of the rule: all 2048 f16 values.  libm's pow and numpy's agree
    on every texel of the battery (none had to be held to one ULP)."""
    got = uploaded_ramp(C.RAMPS[name])
    want = P.ramp(C.RAMPS[name])[1].view(np.uint16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("name", [c.name for c in C.BATTERY])
def test_case_on_oracle(built, request, name):
    case = C.BY_NAME[name]
    img, rows = oracle_render(case)
    C.record(request, case, C.check_case(case, img, rows))


def test_every_case_says_what_it_is_for():
    assert all(len(c.why) > 10 for c in C.BATTERY)
    assert all(c.width <= 64 and c.height <= 48 for c in C.BATTERY)
    assert any(c.width % 16 and c.height % 16 for c in C.BATTERY)
    kinds = {d.kind for c in C.BATTERY for d in c.draws}
    assert kinds == {"linear", "radial", "sweep", "image"}
    assert sorted({len(s) for s in C.RAMPS.values()}) == [2, 3, 4, 5, 6, 17]


# ---- the rule's consequences, worked by hand ---------------------------------------------------------------------------
def test_segment_counts_by_hand():
    """512 * 0.25 = 128; 512 * (0.5 + 257/1024 - 0.5) = 128.5, a tie, away from zero: 129; the last segment gets the rest."""
    assert P.segment_counts([o for o, _ in C.RAMPS["5-opaque"]]) == [128, 128, 129, 127]
    # 64.5 -> 65; 0.25 -> none; exactly one; 512 * 0.471... = 241.45 -> 241; the rest
    assert P.segment_counts([o for o, _ in C.RAMPS["6-narrow"]]) == [65, 0, 1, 241, 205]
    # a stop is prepended at 0: 512 * f32(0.1) = 51.2 -> 51; 512 * (f32(0.35) - f32(0.1)) -> 128; the hard stop: none
    assert P.segment_counts([o for o, _ in C.RAMPS["4-hard-stop"]]) == [51, 128, 0, 333]


def test_hard_stop_texels_by_hand(built):
    """The two texels at the hard stop of "4-hard-stop" (counts 51 + 128: texels 178 and 179) are the two colours given
    at 0.35, premultiplied: (0, 1, 0.3) * 0.4 and (0.1, 0, 1) * 1.  Channels at 0 and 1 are exact; the others pass
    through encode and decode and are held to one f16 ULP.  The single texel of the one-sample segment of "6-narrow" is
    its later stop."""
    for rows in (uploaded_ramp(C.RAMPS["4-hard-stop"]), P.ramp(C.RAMPS["4-hard-stop"])[1].view(np.uint16)):
        left, right = [int(v) for v in rows[178]], [int(v) for v in rows[179]]
        assert left[0] == 0 and left[1] == f16_bits(0.4) and abs(left[2] - f16_bits(0.3 * 0.4)) <= 1 and left[3] == f16_bits(0.4)
        assert abs(right[0] - f16_bits(0.1)) <= 1 and right[1:] == [0, 0x3c00, 0x3c00]
        # first offset > 0: texels 0..50 are the first stop's colour
        assert all(int(rows[i][3]) == f16_bits(0.9) for i in (0, 25, 50)) and int(rows[0][2]) == 0
    for rows in (uploaded_ramp(C.RAMPS["6-narrow"]), P.ramp(C.RAMPS["6-narrow"])[1].view(np.uint16)):
        assert [int(v) for v in rows[65]] == [0, 0, f16_bits(0.5), f16_bits(0.5)]
        assert [int(v) for v in rows[64]] == [0, 0x3c00, 0, 0x3c00]


def test_f16_tie_rounds_away_from_zero(built):
    """Texel 5 of "3-translucent" is 0.25305176997...: its f32 is 0.2530517578125 = 1036.5 * 2^-12, an exact tie between
    two f16.  The host's conversion (the reference's jmath.Float16bits) rounds it away from zero; RTNE would not."""
    r64, r16 = P.ramp(C.RAMPS["3-translucent"])
    assert float(np.float32(r64[5, 0])) == 1036.5 * 2.0 ** -12
    assert int(r16.view(np.uint16)[5, 0]) == 0x340d and int(np.float16(np.float32(r64[5, 0])).view(np.uint16)) == 0x340c
    assert int(uploaded_ramp(C.RAMPS["3-translucent"])[5, 0]) == 0x340d


def test_image_at_integer_placement_by_hand(built):
    """"image-integer": the 5 x 3 image at (3, 2).  Pixel (3 + i, 2 + j) is texel (i, j): alpha a8 / 255 rounded to f32
    and f16; an opaque texel shows its decoded colour (the un-premultiplying store divides by 1), a transparent one
    nothing; every pixel outside the image is untouched."""
    case = C.BY_NAME["image-integer"]
    img, _ = oracle_render(case)
    px = C.IMAGES["5x3"]
    seen = set()
    for j in range(3):
        for i in range(5):
            got = [int(v) for v in img[2 + j, 3 + i]]
            a8 = int(px[j, i, 3])
            seen.add(a8)
            assert got[3] == f16_bits(np.float32(a8) / np.float32(255.0)), (i, j)
            if a8 == 255:
                assert got[:3] == [f16_bits(P.srgb_decode(px[j, i, c] / 255.0)) for c in range(3)], (i, j)
            if a8 == 0:
                assert got == [0, 0, 0, 0], (i, j)
    assert seen == {0, 128, 255}
    outside = np.ones((case.height, case.width), bool)
    outside[2:5, 3:8] = False
    assert not img[outside].any()


def test_sweep_polynomial_distance():
    """The distance of the shader's polynomial from atan(s) / 2 pi: 2.652e-5 turns (0.0136 ramp steps of a full-turn
    sweep), a property of the rule's four constants, recorded in DESIGN 5.  The same on a four times denser grid."""
    d = P.sweep_polynomial_distance()
    assert 2.65e-5 < d < 2.655e-5, d
    assert abs(P.sweep_polynomial_distance(1 << 18) - d) < 1e-9


# ---- sensitivity: each near miss of the reference fails on a named case --------------------------------------------------
NEAR_MISSES = {
    "centre": "linear-axis",
    "index512": "linear-hard-stop",
    "floor_index": "radial-inside",
    "reflect_as_repeat": "linear-similarity",
    "no_swapped_flip": "radial-swapped",
    "no_t_sign": "radial-r0-gt-r1",
    "ramp_linear_light": "ramp-knee-5",
    "ramp_not_premultiplied": "ramp-translucent-rows",
    "counts_by_floor": "ramp-knee-5",
    "unpremul_before_f16": "linear-hard-stop",
    "image_texel_centres": "image-translated",
    "image_interp_before_premul": "image-rotated",
    "alpha_as_srgb": "image-integer",
}


def test_near_misses_are_all_named():
    assert set(NEAR_MISSES) == set(P.DEFECTS) and len(P.DEFECTS) == 13


@pytest.mark.parametrize("defect", list(NEAR_MISSES))
def test_near_miss_fails(built, defect):
    case = C.BY_NAME[NEAR_MISSES[defect]]
    img = oracle_render(case)[0].view(np.float16).astype(np.float64)
    assert not P.check_image(case, img)["bad"].any()
    bad = P.check_image(case, img, defect)["bad"]
    assert bad.any(), "%s passes with the reference's %s" % (case.name, defect)


# ---- the ramp cache: one Host over several recordings --------------------------------------------------------------------
RETAINED = 64
cache_stops, cache_scene, cache_pixel = C.cache_stops, C.cache_scene, C.cache_pixel


class CacheModel:
    """Which ramps of a frame find a slot: one that is cached, one that comes while fewer than 64 are cached, or one
    for which a cached ramp was last used more than two frames ago.  The others get a row past the retained 64."""
    def __init__(self):
        self.used, self.epoch = {}, 0

    def frame(self, keys):
        self.epoch += 1
        no_slot = 0
        for k in keys:
            if k in self.used:
                self.used[k] = self.epoch
            elif len(self.used) < RETAINED:
                self.used[k] = self.epoch
            else:
                stale = [q for q, e in self.used.items() if e + 2 < self.epoch]
                if stale:
                    del self.used[stale[0]]
                    self.used[k] = self.epoch
                else:
                    no_slot += 1
        return no_slot


def test_ramp_cache_over_recordings(built):
    """70 distinct gradients per frame for 5 frames, the colours changing per frame; a frame of 3 gradients (three that
    the cache holds); 70 again.  In every frame each gradient's pixel at t = 1/4 is texel round(511 / 4) = 128 of ITS
    ramp (opaque over a transparent base: the pixel is the texel), the ramp image never has more rows than 64 plus
    the frame's ramps without a slot, and the frame of 3 uploads at most 64 rows."""
    frames = [[cache_stops(i, f) for i in range(70)] for f in range(5)]
    frames.append(frames[3][:3])
    frames.append([cache_stops(i, 6) for i in range(70)])
    host, model = Host(), CacheModel()
    heights = []
    for f, stops_list in enumerate(frames):
        rec = host.record(*cache_scene(stops_list))
        rows = K.ramp_rows(rec)
        heights.append(rows.shape[0])
        no_slot = model.frame([repr(s) for s in stops_list])
        assert rows.shape[0] <= RETAINED + no_slot, "frame %d: %d ramp rows, %d ramps without a slot" % (f, rows.shape[0], no_slot)
        if len(stops_list) <= 3:
            assert rows.shape[0] <= RETAINED, "frame %d uses %d ramps and uploads %d rows" % (f, len(stops_list), rows.shape[0])
        o = OracleEngine()
        o.run(rec)
        img = o.target(rec)
        for k, stops in enumerate(stops_list):
            x, y, want = cache_pixel(k, stops)
            assert [int(v) for v in img[y, x]] == want, "frame %d, gradient %d" % (f, k)
    assert heights[0] == 70 and max(heights) <= RETAINED + 70
