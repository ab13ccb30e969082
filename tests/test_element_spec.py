"""CPU: the definitions of tests/element_streams.py -- tag monoid, draw monoid, binning, tile_alloc by their rules in numpy -- against
oracle_dispatch of the same stage, on the case lists test_gpu_element_stages.py runs on the GPU.  The oracle is a port of the shaders, the
definitions are not: where the two agree, a GPU mismatch is the kernel's; where they cannot, the exception is named here.

TILE_ALLOC_BROADCAST_SLOT: tile_alloc.wgsl:92-104 hands a workgroup's offset to its threads through paths[workgroup * 256 + 255].tiles,
written without the n_drawobj test of line 106 -- in the last workgroup that is a word of an entry behind the last draw object, which
no stage reads.  The oracle does the same; the definition (and the kernel, which has the offset in a register) leaves those entries
alone.  The word is exempt from the poison check on the oracle's buffers only.

TILE_ALLOC_CLEAR_ON_OVERFLOW: tile_alloc.wgsl:118-122 clears [offset, offset + count) per workgroup, with offset = 0 for a workgroup
that did not fit: after a failure the cleared set is the union of those ranges, clipped by the buffer.  The definition is the kernels'
rule, one clear of [0, min(total, tiles_size)); both hold the tiles every consumer may read after a frame WITHOUT failure, and with
FAILED_TILE_ALLOC set the frame is rendered again.  The oracle's tiles are not compared in the cases that set the bit.
"""
import numpy as np
import pytest

import element_streams as E

PATHTAG = E.pathtag_streams()
BINNING = E.binning_cases()
TILES = E.tile_alloc_cases()


def test_tag_byte_table_is_the_word_rule(built):
    """Every byte value in every byte position, alone and against a background of random bytes: the per-byte table summed over a word
    is what the oracle's pathtag_reduce gives for that word (a workgroup of one such word and 255 zero words)."""
    rng = np.random.default_rng(5)
    words = [np.uint32(b << (8 * k)) for b in range(256) for k in range(4)]
    words += list(rng.integers(0, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32))
    scene = np.zeros((len(words), E.WG), np.uint32)
    scene[:, 0] = words
    bufs = {"cfg": E.config(), "scene": scene.reshape(-1), "reduced": E.poisoned((len(words), 5))}
    got = E.run_oracle(bufs, [("pathtag_reduce", len(words), ["cfg", "scene", "reduced"])])
    assert np.array_equal(got["reduced"].reshape(-1, 5), E.tag_word_monoids(np.array(words, np.uint32)))


@pytest.mark.parametrize("name,wgs,kind", PATHTAG, ids=[s[0] for s in PATHTAG])
def test_pathtag_definition_is_the_oracles(built, name, wgs, kind):
    counts = E.host_counts(wgs)
    assert counts["large"] == (wgs > 256)
    scene = E.pathtag_scene(wgs, kind)
    bufs, dispatches = E.pathtag_job(scene, counts)
    E.check_pathtag(E.run_oracle(bufs, dispatches), E.pathtag_by_definition(scene, counts), counts, "oracle")


@pytest.mark.parametrize("n", E.DRAW_COUNTS)
def test_draw_definition_is_the_oracles(built, n):
    n_wgs = E.host_draw_counts(n)["draw_reduce"]
    assert n_wgs == min((n + 255) // 256, 256)
    bufs, dispatches, tags = E.draw_job(n, n_wgs)
    want = E.draw_by_definition(tags, bufs["path_bbox"], n_wgs, len(bufs["clip_inp"]), len(bufs["info"]))
    E.check_draw(E.run_oracle(bufs, dispatches), want, "oracle")


@pytest.mark.parametrize("case", BINNING, ids=[c.name for c in BINNING])
def test_binning_definition_is_the_oracles(built, case):
    bufs, dispatches = E.binning_job(case)
    E.check_binning(E.run_oracle(bufs, dispatches), E.binning_by_definition(case), case, "oracle")


@pytest.mark.parametrize("case", TILES, ids=[c.name for c in TILES])
def test_tile_alloc_definition_is_the_oracles(built, case):
    bufs, dispatches = E.tile_alloc_job(case)
    E.check_tile_alloc(E.run_oracle(bufs, dispatches), E.tile_alloc_by_definition(case), case, "oracle", oracle=True)


def test_case_lists_hold_what_they_are_for(built):
    """The properties the cases were chosen for, checked on the definitions: the draw counts' base / remainder split, an odd and an
    even tile total, which workgroups overflow."""
    split = {n: divmod((n + 255) // 256, 256) for n in E.DRAW_COUNTS}
    assert {b for b, _ in split.values()} == {0, 1, 2, 3} and {r for _, r in split.values()} >= {0, 1, 255}
    assert split[65536 + 255 * 256] == (1, 255) and split[65536 + 255 * 256 + 1] == (2, 0) and 1 < split[200000][1] < 255
    by = {c.name: E.tile_alloc_by_definition(c) for c in TILES}
    assert by["total_odd"]["total"] % 2 == 1 and by["total_even"]["total"] % 2 == 0
    assert by["one_tile_too_small"]["bump"][0] == E.FAILED_TILE_ALLOC and by["one_tile_too_small"]["n_zero"] == by["one_tile_too_small"]["total"] - 1
    b = {c.name: (c, E.binning_by_definition(c)) for c in BINNING}
    case, d = b["last_workgroups_overflow"]
    over = np.flatnonzero((d["headers"][:, 1] == 0) & (np.arange(len(d["headers"])) > 0) & (d["headers"][:, 0] > 0))
    assert d["bump"][0] == E.FAILED_BINNING and over.size == 1 and over[0] // E.WG == case.n_wgs - 1
    case, d = b["bins_512"]
    assert d["bump"][1] < 512 + 128 + 16 and d["headers"][:256, 0].min() >= 1  # element 0 covers 512 bins and is listed in 256
    assert E.host_draw_counts(65537)["binning"] == 257 and E.host_draw_counts(65537)["tile_alloc"] == 257


def test_scan_u32_definition():
    v = np.array([5, 0xffffffff, 7, 1, 2, 3], np.uint32)
    out, total = E.scan_u32(v, 1, 6)
    assert list(out) == [0, 5, 4, 11, 12, 14] and total == 17
    out, total = E.scan_u32(v, 2, 3)
    assert list(out) == [0, 5, 12] and total == 14
    assert E.scan_u32(v, 1, 0)[1] == 0 and len(E.scan_u32(v, 1, 0)[0]) == 0
