"""CPU: the battery of hand-written command lists of tests/ptcl_streams.py before it goes to a GPU.  Every frame validates; the
oracle's fine stage -- on the buffers of a small carrier scene, overwritten with the frame -- gives the eager interpreter's f16
bits on every finite stream; the interpreter's blend is the scalar one of fine_by_hand on the source-over words; and eleven near
misses of the kernel's layer machinery, written as variants of the interpreter, each change the bits of streams named here: that
is how the battery shows it can see that class of kernel bug.  Last, the grid of every (mix, operator) pair through the whole
oracle pipeline against the W3C formulas in float64."""
import numpy as np
import pytest

import composite_ref
import fine_by_hand
import ptcl_streams as P

GROUPS = ["A", "B", "C", "D"]


@pytest.mark.parametrize("group", GROUPS)
def test_every_stream_validates(group):
    fs = P.frames(group)
    assert sum(len(f.streams) for f in fs) == len(P.battery()[group])
    for f in fs:
        assert P.validate(f)
        offs = f.blend_offsets
        assert len(set(offs)) == len(offs)


def test_validate_refuses_what_must_not_reach_a_gpu():
    ok = [P.SOLID, P.color(P.BACK), P.BEGIN, P.SOLID, P.end_clip(0, 1.0), P.END]

    def frame(cmds):
        return P.Frame([P.Stream("x", "X", cmds)])
    assert P.validate(frame(ok))
    with pytest.raises(AssertionError, match="END_CLIP at depth 0"):
        P.validate(frame([P.SOLID, P.end_clip(0, 1.0), P.END]))
    with pytest.raises(AssertionError, match="no END"):
        P.validate(frame([P.SOLID] * 70))                      # (the zero padding behind it would end it: not good enough)
    deep = frame([P.BEGIN] * 6 + [P.SOLID, P.color(P.BACK)] + [P.end_clip(0, 1.0)] * 6 + [P.END])
    assert P.validate(deep)
    with pytest.raises(AssertionError, match="spill index"):
        P.validate(deep, spill_capacity=300)
    back = frame(ok)
    back.ptcl[1], back.ptcl[2] = P.TAG["jump"], 1              # a loop
    with pytest.raises(AssertionError, match="jump from"):
        P.validate(back)
    out = frame(ok)
    out.ptcl[1], out.ptcl[2] = P.TAG["jump"], len(out.ptcl)    # outside
    with pytest.raises(AssertionError, match="jump from"):
        P.validate(out)
    with pytest.raises(AssertionError, match="does not fit"):
        P.validate(frame(ok), ptcl_words=100)


def test_the_backdrops_are_what_their_names_say():
    """The colour in front of the last END_CLIP, as the interpreter has it: the odd value in exactly one pixel or in all."""
    by_name = {s.name: s for s in P.battery()["B"]}

    def raw(b):
        return P.run_tile(by_name["B_%s_0000_1_solid" % b], raw_before_last_end=True).view(np.uint32)
    for b, pattern, count in (("sixteen_all", 0x41800000, 256), ("sixteen_one", 0x41800000, 1), ("sixteen_alpha_one", 0x41800000, 1),
                              ("sixteenup_all", 0x41800001, 256), ("sixteenup_one", 0x41800001, 1), ("negzero_all", 0x80000000, 512),
                              ("inf_one", 0xff800000, 1)):
        r = raw(b)
        assert int((r == pattern).sum()) == count, (b, int((r == pattern).sum()))
        if count == 1:  # every other pixel holds the plain backdrop
            assert int((r == r[0]).all(axis=1).sum()) == 255
    r = raw("nan_one").view(np.float32)
    assert int(np.isnan(r).any(axis=1).sum()) == 1 and int((r == r[0]).all(axis=1).sum()) == 255
    assert not np.isnan(raw("inf_one").view(np.float32)).any()
    r = raw("negative_one").view(np.float32)
    assert int((r < 0).any(axis=1).sum()) == 1
    r = raw("alpha0_all").view(np.float32)
    assert np.all(r[:, 3] == 0) and np.all(r[:, :3] > 0)
    for b, n in (("lum_one", 1), ("lum_grey_all", 256)):
        r = raw(b).view(np.float32)
        lum = composite_ref._lum([r[:, k] / np.maximum(r[:, 3], np.float32(1e-15)) for k in range(3)])
        assert int((lum > 1).sum()) == n, (b, int((lum > 1).sum()))
    # the memo streams: lum(cb) <= 1 before the Plus layer, > 1 behind it
    assert P.battery()["C"] and any(x.cmds[:len(P.memo_prefix(0x0c00))] == tuple(P.memo_prefix(0x0c00)) for x in P.battery()["C"])
    last = P.run_tile(P.Stream("prefix", "C", P.memo_prefix(0x0c00) + [P.END]), raw_before_last_end=True)
    assert np.all(last[:, :3] == 1.0) and np.all(last[:, 3] == 0.5)


def test_finite_streams_stay_finite():
    """`finite` is a statement about the stream; the interpreter's result has to bear it out."""
    for g in GROUPS:
        for s in P.battery()[g]:
            if s.finite:
                h = P.expected(s)
                assert not ((h & 0x7fff) >= 0x7c00).any(), s.name


@pytest.fixture(scope="module")
def oracle_area(built):
    return P.OracleFine(0)


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_fine_area_gives_the_interpreters_bits(oracle_area, group):
    problems = []
    n = 0
    for f in P.frames(group):
        got = oracle_area.run(f)
        for s, tile in zip(f.streams, got):
            if s.finite:
                n += 1
                m = P.mismatch(s, tile, P.expected(s), "oracle", "interpreter")
                if m:
                    problems.append(m)
    assert n > 0
    assert not problems, "%d of %d finite streams differ:\n%s" % (len(problems), n, "\n".join(problems[:10]))


@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("group", ["B", "C"])
def test_oracle_fine_msaa_gives_the_interpreters_bits_without_fills(built, group, aa):
    """The multisampled stages differ from Area in a FILL's coverage alone: streams without one hold there too."""
    o = P.OracleFine(aa)
    pick = [s for s in P.battery()[group] if s.finite and not s.has_fill]
    assert pick
    for i in range(0, len(pick), P.TILES):
        f = P.Frame(pick[i:i + P.TILES])
        for s, tile in zip(f.streams, o.run(f)):
            m = P.mismatch(s, tile, P.expected(s), "oracle", "interpreter")
            assert m is None, m


def test_interpreter_blend_is_the_scalar_blend_on_source_over_words():
    """composite_ref.blend_mix_compose (arrays) against fine_by_hand.blend_mix_compose (one pixel, one operation per line) on the
    backdrop and the sources group A blends: every mix mode, both alphas, the areas of the diagonal."""
    areas = np.unique(P._fill_areas(tuple(tuple(float(v) for v in s) for s in P.DIAGONAL), 0, False))[::7]
    bg = np.array([np.float32(v) for v in P.BACK], np.float32)
    for mix in range(16):
        for alpha in (1.0, 0.625):
            src = (np.array(P.SRC, np.float32)[None, :] * areas[:, None]) * np.float32(alpha)
            got = composite_ref.blend_mix_compose(np.broadcast_to(bg, src.shape), src, mix << 8)
            for i in range(src.shape[0]):
                want = fine_by_hand.blend_mix_compose(list(bg), list(src[i]), fine_by_hand.MIX_NAMES[mix])[0]
                assert [P.bits(v) for v in want] == [P.bits(v) for v in got[i]], (mix, alpha, float(areas[i]))


# Which streams tell each near miss from the rule.  (name of the variant, streams that MUST change, why.)
NEAR_MISSES = [
    ("no_range_test", ["B_far_all_0900_1_solid"],
     "shortcut without the range test: soft light on cb = 1e20 overflows, cs' * 0 is NaN, the shortcut keeps the backdrop"),
    ("no_lum_test", ["B_lum_grey_all_0c00_1_solid", "B_lum_grey_all_0e00_1_solid"],
     "shortcut without the luminance test: clip_color of (l, l, l) with l > 1 divides 0 by 0"),
    ("memo_across_plus", ["C_memo_plus_0c00", "C_memo_plus_0e00"],
     "the memo of the first hue layer kept across the Plus layer that lifts lum(cb) to 2"),
    ("luminosity_shortcut", ["B_grey_all_0f00_1_solid"],
     "luminosity closed by the shortcut: on a grey backdrop lum(c) - min(c) vanishes and the rule gives NaN"),
    ("compose_ignored", ["A_0003_a1", "A_0105_a0.625", "A_0f0c_a1"], "compose byte ignored"),
    ("fa_fb_swapped", ["A_0001_a1", "A_0004_a0.625", "A_0509_a1"], "Fa and Fb exchanged"),
    ("tier_off_by_one", ["D_every_level_6", "D_every_level_7", "D_depth7_level5_only_inner"], "a spilled level read from the slot below"),
    ("inner_saves_not_zero", ["D_innermost_only_2", "D_innermost_only_5", "C_begin_x4_drawn"],
     "pending inner levels saved with the colour instead of the zeros they start from"),
    ("end_clip_area_one", ["A_0000_a1", "A_0c00_a0.625", "D_every_level_1"], "END_CLIP's area taken as 1"),
    ("alpha3_is_solid", ["B_inrange_0000_pat3_fill", "B_inrange_0100_pat3_fill"],
     "an alpha of bit pattern 3 taken for a SOLID: the COLOR behind the layer is drawn with area 1"),
    ("neg_zero_alpha", ["B_negzero_all_0000_neg0_solid"],
     "an alpha of -0 taken as +0: the plain arm's bg + src turns the backdrop's -0 into +0"),
]


@pytest.mark.parametrize("variant,must,why", NEAR_MISSES, ids=[n[0] for n in NEAR_MISSES])
def test_the_battery_sees_the_near_miss(variant, must, why):
    assert sorted(n[0] for n in NEAR_MISSES) == sorted(P.VARIANTS)
    by_name = {s.name: s for g in GROUPS for s in P.battery()[g]}
    for name in must:
        s = by_name[name]
        rule, miss = P.expected(s), P.run_tile(s, variant)
        assert (P.canon(rule) != P.canon(miss)).any(), "%s does not tell `%s` (%s) from the rule" % (name, variant, why)


# ---- the grid of (mix, operator) cells through the whole pipeline ----------------------------------------------------------------
def test_blend_grid_on_the_oracle_follows_the_w3c_formulas(built):
    import jello_amd
    from oracle.oracle_engine import OracleEngine
    s, p, cells = P.blend_grid()
    assert len(cells) == 16 * 13
    rec = jello_amd.Host().record(s, p)
    o = OracleEngine()
    o.run(rec)
    bad = P.check_grid(o.target(rec), cells)
    assert not bad, bad
