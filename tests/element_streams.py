"""Hand-built inputs for the element stages in front of path_count -- the path-tag scan (pathtag_reduce / reduce2 / scan1 / scan),
draw_reduce / draw_leaf, binning, tile_alloc -- and for the single-launch u32 scan, each with its DEFINITION in numpy: what every
output word has to be, stated from the stage's rule (shared/pathtag.wgsl, shared/drawtag.wgsl, binning.wgsl, tile_alloc.wgsl) and
not as a port of it.  Nothing here shares code with oracle/ or the kernels: the tag monoid is defined per tag byte and summed (not the
SWAR form of reduce_tag), every scan is an np.cumsum in uint32, binning and tile_alloc are loops over boxes.

test_element_spec.py holds the definitions against the oracle on the CPU, test_gpu_element_stages.py holds the kernels against both.
The buffer scheme is test_gpu_clip.py's: outputs are poisoned, the defined words compared, the words behind them must keep the poison.
"""
import functools

import numpy as np

import jello_amd
from jello_amd._lib import CConfig, PathEl
from clip_streams import EVERYTHING
from devmem import CANARY

WG = 256
N_TILE = 256                         # bins a workgroup of binning can address (config.wgsl:52)
LB_TILE = 16384                      # elements per workgroup of the look-back scan (kernels_scan.hip)
POISON = CANARY * 0x01010101
STAGE = {n: i for i, n in enumerate(jello_amd.STAGE_NAMES)}
FAILED_BINNING, FAILED_TILE_ALLOC, FAILED_FLATTEN = 1, 2, 4   # bump.failed bits (shared/bump.wgsl)
BUMP = {n: i for i, n in enumerate(jello_amd.engine.BUMP_NAMES)}


def poisoned(shape):
    return np.full(shape, POISON, np.uint32)


def config(**fields):
    """A JlConfig as 25 words: the fields by name (jello_amd._lib.CConfig), everything else zero."""
    c = CConfig()
    for k, v in fields.items():
        assert hasattr(c, k), k
        setattr(c, k, int(v))
    return np.frombuffer(bytes(c), np.uint32).copy()


def excl_cumsum(m):
    """Exclusive prefix sums of the rows of m, mod 2^32."""
    m = np.ascontiguousarray(m, np.uint32)
    out = np.zeros_like(m)
    if len(m) > 1:
        np.cumsum(m[:-1], axis=0, dtype=np.uint32, out=out[1:])
    return out


def wsum(m):
    return m.sum(axis=0, dtype=np.uint32)


# ---- what the host computes for a tag count --------------------------------------------------------------------------------------
class ArrayPath:
    """A polyline as jello_amd.Path's interface, built from an (n, 2) array without a Python loop per element."""

    def __init__(self, pts, close=True):
        n = len(pts) + (1 if close else 0)
        a = np.zeros(n, np.dtype([("kind", "<i4"), ("pad", "<i4"), ("pts", "<f8", 6)]))
        a["kind"][1:len(pts)] = 1
        a["pts"][:len(pts), :2] = pts
        if close:
            a["kind"][-1] = 4
        self._a, self.els = a, range(n)

    def _c(self):
        return (PathEl * len(self._a)).from_buffer(self._a)


def zigzag(n_points, width, rows_apart=1.0, step=0.25):
    """n_points of a sawtooth that fills `width` px rows one after the other: consecutive points always differ (a zero-length
    segment is not encoded), every segment is about a pixel long."""
    i = np.arange(n_points)
    per_row = int(width / step)
    x = (i % per_row) * step
    y = (i // per_row) * rows_apart + np.where(i % 2 == 0, 0.0, 0.7)
    return np.stack([x, y], axis=1)


def scene_of_tag_wgs(tag_wgs, n_paths=1, width=256):
    """(scene, params) of `n_paths` filled zigzags whose padded tag words make exactly `tag_wgs` workgroups of 256 words: one tag
    byte per segment, aimed at the middle of the last workgroup so that the few tags per path besides the segments cannot matter.
    The caller asserts the count on the recording."""
    from jello_amd import scene as S
    n_segments = (tag_wgs - 1) * 4 * WG + 2 * WG
    s = S.Scene()
    per = n_segments // n_paths
    rows = 0.0
    for k in range(n_paths):
        n = per if k < n_paths - 1 else n_segments - per * (n_paths - 1)
        pts = zigzag(n, width)
        pts[:, 1] += rows
        rows = float(np.ceil(pts[-1, 1])) + 1.0
        s.fill(S.Fill.NonZero, None, S.Brush.solid((0.2 + 0.05 * (k % 8), 0.5, 0.9, 0.7)), None, ArrayPath(pts))
    side = max(width, int(rows) + 2)
    return s, S.RenderParams(width, side)


@functools.lru_cache(maxsize=None)
def host_counts(tag_wgs):
    """The workgroup counts and buffer sizes (bytes) new_workgroup_counts / new_buffer_sizes give a scene of `tag_wgs` tag-word
    workgroups, read from a recording of such a scene."""
    s, p = scene_of_tag_wgs(tag_wgs, n_paths=max(1, tag_wgs // 256))
    rec = jello_amd.Host().record(s, p)
    wg = rec.workgroup_counts()
    assert wg["path_reduce"][0] == tag_wgs, (wg["path_reduce"], tag_wgs)
    sizes = {"reduced": rec.buffer("reducedBuf")[1], "tagmonoid": rec.buffer("tagmonoidBuf")[1]}
    if wg["use_large_path_scan"]:
        sizes["reduced2"], sizes["reduced_scan"] = rec.buffer("reduced2Buf")[1], rec.buffer("reducedScanBuf")[1]
    return {"large": wg["use_large_path_scan"], "reduce": wg["path_reduce"][0], "reduce2": wg["path_reduce2"][0], "scan1": wg["path_scan1"][0],
            "scan": wg["path_scan"][0], "sizes": sizes}


@functools.lru_cache(maxsize=None)
def host_draw_counts(n_drawobj):
    """The same for a scene of n_drawobj draw objects (one small rectangle each): workgroups of draw_reduce / draw_leaf, binning and
    tile_alloc."""
    from jello_amd import scene as S
    s = scene_of_objects(n_drawobj)
    rec = jello_amd.Host().record(s, S.RenderParams(64, 64))
    assert rec.config["n_drawobj"] == n_drawobj
    wg = rec.workgroup_counts()
    return {"draw_reduce": wg["draw_reduce"][0], "draw_leaf": wg["draw_leaf"][0], "binning": wg["binning"][0], "tile_alloc": wg["tile_alloc"][0]}


# ---- tag monoid --------------------------------------------------------------------------------------------------------------------
def _tag_byte_table():
    """TagMonoid of one tag byte (shared/pathtag.wgsl:13-21): bits 0-1 segment type (0 none, 1 line, 2 quad, 3 cubic = its point
    count), 4 subpath end (one more point), 8 f32 coordinates (two words per point, else one), 0x10 path, 0x20 transform, 0x40 style
    (two words)."""
    t = np.zeros((256, 5), np.uint8)
    for b in range(256):
        seg = b & 3
        points = seg + (1 if b & 4 else 0)
        t[b] = (1 if b & 0x20 else 0,               # trans_ix
                1 if seg else 0,                    # pathseg_ix
                points * (2 if b & 8 else 1),       # pathseg_offset
                2 if b & 0x40 else 0,               # style_ix
                1 if b & 0x10 else 0)               # path_ix
    return t


TAG_BYTE = _tag_byte_table()


def tag_word_monoids(words):
    """[n, 5] u32: a word's monoid is the sum of its four bytes' monoids."""
    by = np.ascontiguousarray(words, "<u4").view(np.uint8)
    return TAG_BYTE[by].reshape(-1, 4, 5).sum(axis=1, dtype=np.uint32)


PATHTAG_WGS_SMALL = (1, 2, 255, 256)
PATHTAG_WGS_LARGE = (257, 511, 512, 513, 3840, 3841, 4096, 4097)  # scan1 grids 2, 2, 2, 3, 15, 16, 16, 17
PATHTAG_BASE = 3  # config.pathtag_base: the tag words do not start the scene buffer


def pathtag_streams():
    """(name, tag-word workgroups, kind): random tag bytes at every workgroup count, all-ones and all-zero words at a few."""
    out = [("random_%d" % w, w, "random") for w in PATHTAG_WGS_SMALL + PATHTAG_WGS_LARGE]
    out += [("ones_%d" % w, w, "ones") for w in (2, 257, 3841)] + [("zeros_%d" % w, w, "zeros") for w in (2, 257)]
    return out


def pathtag_scene(tag_wgs, kind):
    """The scene buffer: PATHTAG_BASE words that are no tags, then tag_wgs * 256 tag words."""
    n = tag_wgs * WG
    if kind == "random":
        w = np.random.default_rng(0x70617468 + tag_wgs).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    else:
        w = np.full(n, 0xffffffff if kind == "ones" else 0, np.uint32)
    return np.concatenate([np.full(PATHTAG_BASE, 0xffffffff, np.uint32), w])


def pathtag_by_definition(scene, counts):
    """reduced [reduce, 5], tag monoids [reduce * 256, 5]; on the three-level route also reduced2 [256, 5] and the first `reduce`
    entries of reducedScan.  The tail of `reduced` behind the written workgroups is POISON (the tests upload it so), so every entry
    of reduced2 is defined: the sum of its 256 entries of `reduced`, an entry past the buffer reading as zero."""
    m = tag_word_monoids(scene[PATHTAG_BASE:])
    n_wg = counts["reduce"]
    assert len(m) == n_wg * WG
    out = {"reduced": m.reshape(n_wg, WG, 5).sum(axis=1, dtype=np.uint32), "tagmonoid": excl_cumsum(m)}
    if counts["large"]:
        n_red = counts["sizes"]["reduced"] // 20
        full = np.zeros((counts["reduce2"] * WG, 5), np.uint32)
        full[:n_red] = POISON
        full[:n_wg] = out["reduced"]
        out["reduced2"] = full.reshape(counts["reduce2"], WG, 5).sum(axis=1, dtype=np.uint32)
        out["reduced_scan"] = excl_cumsum(out["reduced"])
    return out


# ---- draw monoid -------------------------------------------------------------------------------------------------------------------
NOP, COLOR, BEGIN_CLIP, END_CLIP = 0, 0x50, 0x9, 0x21
DRAW_KINDS_WITH_INFO = (0x50, 0x114, 0x29c, 0x254, 0x248, 0x9)
# (blocks of 256 objects) = 256 * base + remainder: 65536 + 255 * 256 is (1, 255), the largest remainder; one object more is (2, 0)
DRAW_COUNTS = (1, 255, 256, 257, 65535, 65536, 65537, 65536 + 255 * 256, 65536 + 255 * 256 + 1, 131072, 131073, 200000)
DRAWTAG_BASE, DRAWDATA_BASE = 5, 2


def draw_tags(n):
    """Random 32-bit words (never one of the tags draw_leaf writes info for), with nop, solid colour, begin-clip and end-clip at
    known positions: every 7th, 5th, 11th and 13th object, first match."""
    t = np.random.default_rng(0x64726177 + n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    t[np.isin(t, DRAW_KINDS_WITH_INFO + (END_CLIP, NOP))] ^= 0x80000000
    i = np.arange(n)
    for period, tag in ((13, END_CLIP), (11, BEGIN_CLIP), (5, COLOR), (7, NOP)):
        t[i % period == period - 1] = tag
    return t


def draw_monoid_of(tags):
    """[n, 4] u32, shared/drawtag.wgsl:46-53: path_ix counts the objects that are no nop, clip_ix bit 0, scene_offset bits 2-4,
    info_offset bits 6-9."""
    t = np.asarray(tags, np.uint32)
    return np.stack([(t != 0).astype(np.uint32), t & 1, (t >> 2) & 7, (t >> 6) & 0xf], axis=1)


def draw_pack(n):
    """cfg, scene, path_bbox (draw_flags random, the rest unused) for n draw objects."""
    tags = draw_tags(n)
    tot = wsum(draw_monoid_of(tags))
    n_path, n_clip, n_info = max(int(tot[0]), 1), max(int(tot[1]), 1), max(int(tot[3]), 1)
    scene = np.concatenate([np.full(DRAWTAG_BASE, 0x50, np.uint32), tags])
    pb = np.zeros((n_path, 6), np.uint32)
    pb[:, 4] = np.random.default_rng(n).integers(0, 1 << 32, n_path, dtype=np.uint64).astype(np.uint32)
    cfg = config(n_drawobj=n, n_path=n_path, n_clip=n_clip, bin_data_start=n_info, drawtag_base=DRAWTAG_BASE, drawdata_base=DRAWDATA_BASE)
    return cfg, scene, pb, tags, (n_path, n_clip, n_info)


def draw_by_definition(tags, path_bbox, n_wgs, n_clip, n_info):
    """draw_reduced [n_wgs, 4]; draw_monoids [n, 4]; clip_inp [n_clip, 2] and info [n_info] with POISON where nothing is written.
    The blocks of 256 objects are dealt to the 256 workgroups in order and as evenly as possible, the earlier workgroups taking the
    extra one (draw_reduce.wgsl:30-36)."""
    n = len(tags)
    m = draw_monoid_of(tags)
    ex = excl_cumsum(m)
    blocks = np.array_split(np.arange((n + WG - 1) // WG), WG)
    reduced = np.zeros((n_wgs, 4), np.uint32)
    for w in range(n_wgs):
        if len(blocks[w]):
            reduced[w] = wsum(m[blocks[w][0] * WG:(blocks[w][-1] + 1) * WG])
    clip_inp = poisoned((n_clip, 2))
    for tag in (BEGIN_CLIP, END_CLIP):
        i = np.flatnonzero(tags == tag).astype(np.uint32)
        clip_inp[ex[i, 1], 0] = i
        clip_inp[ex[i, 1], 1] = ex[i, 0] if tag == BEGIN_CLIP else ~i
    info = poisoned(n_info)
    i = np.flatnonzero(tags == COLOR)
    flags = np.where(ex[i, 0] < len(path_bbox), path_bbox[np.minimum(ex[i, 0], len(path_bbox) - 1), 4], 0)
    info[ex[i, 3]] = flags
    return {"draw_reduced": reduced, "draw_monoid": ex, "clip_inp": clip_inp, "info": info}


# ---- binning -----------------------------------------------------------------------------------------------------------------------
CLEARED = (0x7fffffff, 0x7fffffff, -0x80000000, -0x80000000)  # a path box as bbox_clear leaves it


class BinCase:
    """One binning dispatch: n draw objects, object i draws path i.  boxes: [n, 4] integer path boxes; clip_ix: [n] (0: not
    clipped); clips: [k, 4] f32 clip boxes, of which the config announces n_clip."""

    def __init__(self, name, boxes, width_px, height_px, clip_ix=None, clips=None, n_clip=None, short_by=None, lines_over=False, bin_data_start=7):
        self.name = name
        self.boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
        self.n = len(self.boxes)
        self.wt, self.ht = (width_px + 15) // 16, (height_px + 15) // 16
        self.clip_ix = np.zeros(self.n, np.uint32) if clip_ix is None else np.asarray(clip_ix, np.uint32)
        self.clips = np.zeros((1, 4), np.float32) if clips is None else np.asarray(clips, np.float32).reshape(-1, 4)
        self.n_clip = len(self.clips) if n_clip is None else n_clip
        self.short_by, self.lines_over, self.bin_data_start = short_by, lines_over, bin_data_start
        self.n_wgs = (self.n + WG - 1) // WG
        self.lines_size = 1000
        self.lines_on_entry = self.lines_size + 1 if lines_over else self.lines_size
        total = sum(len(v) for v in _covered_bins(self)[1].values())
        # `short_by` words too small for the last chunk: exactly the workgroups from the last one with elements on overflow
        self.binning_size = total + 9 if short_by is None else max(total - short_by, 0)
        self.bin_data_words = bin_data_start + self.binning_size + 16  # (the buffer is longer than the config says: poison behind)

    def pack(self):
        dm = np.zeros((self.n, 4), np.uint32)
        dm[:, 0] = np.arange(self.n)
        dm[:, 1] = self.clip_ix
        pb = np.zeros((self.n, 6), np.int32)
        pb[:, :4] = self.boxes.astype(np.int32)
        bump = np.zeros(8, np.uint32)
        bump[BUMP["lines"]] = self.lines_on_entry
        cfg = config(width_in_tiles=self.wt, height_in_tiles=self.ht, n_drawobj=self.n, n_path=self.n, n_clip=self.n_clip,
                     bin_data_start=self.bin_data_start, lines_size=self.lines_size, binning_size=self.binning_size)
        return cfg, dm, pb, self.clips, bump


def _covered_bins(case):
    """(boxes f32 [n, 4], {(workgroup, bin): [elements, ascending]}) by the rules stated in binning_by_definition."""
    n = case.n
    clip = np.tile(np.array(EVERYTHING, np.float32), (n, 1))
    has = case.clip_ix > 0
    last = np.uint32((case.n_clip - 1) & 0xffffffff)   # (u32 as the shader computes it: n_clip = 0 clamps nothing)
    ix = np.minimum((case.clip_ix[has] - 1).astype(np.uint32), last)
    inside = ix < len(case.clips)                      # (a read past the buffer gives zeros)
    clip[has] = np.where(inside[:, None], case.clips[np.minimum(ix, len(case.clips) - 1)], np.float32(0))
    pb = case.boxes.astype(np.int32).astype(np.float32)
    box = np.concatenate([np.maximum(clip[:, :2], pb[:, :2]), np.minimum(clip[:, 2:], pb[:, 2:])], axis=1).astype(np.float32)
    wb, hb = (case.wt + 15) // 16, (case.ht + 15) // 16
    live = (box[:, 0] < box[:, 2]) & (box[:, 1] < box[:, 3])
    scaled = box * np.float32(1.0 / 256.0)
    lo = np.floor(scaled[:, :2]).astype(np.int64)
    hi = np.ceil(scaled[:, 2:]).astype(np.int64)
    x0, y0 = np.clip(np.where(live, lo[:, 0], 0), 0, wb), np.clip(np.where(live, lo[:, 1], 0), 0, hb)
    x1, y1 = np.clip(np.where(live, hi[:, 0], 0), 0, wb), np.clip(np.where(live, hi[:, 1], 0), 0, hb)
    lists = {}
    for e in np.flatnonzero((x0 < x1) & (y0 < y1)):
        for y in range(y0[e], y1[e]):
            for x in range(x0[e], x1[e]):
                b = y * wb + x
                if b < N_TILE:
                    lists.setdefault((int(e) // WG, b), []).append(int(e))
    return box, lists


def binning_by_definition(case):
    """What binning leaves: `boxes` f32 [n, 4] (path box met with the clip box, bit for bit), `headers` [n_wgs * 256, 2] (element
    count, chunk offset) in workgroup-major, then bin, order, `bin_data` with `defined` (the chunk lists, ascending element order) and
    `unspecified` (where the chunks that did not fit were dumped at offset 0), and `bump` (8 words).

    The rules (binning.wgsl): an element covers the bins [floor(x0 / 256), ceil(x1 / 256)) x [floor(y0 / 256), ceil(y1 / 256)) of its box
    if x0 < x1 and y0 < y1, none otherwise; the ranges are clamped to the target's bins, and an empty x range empties the y range.
    A bin is addressed by y * width_in_bins + x in a table of N_TILE = 256 entries: a covered bin with an index of 256 or more is
    dropped (the shader would write past its table: binning.wgsl:52,131).  A workgroup takes 256 elements; its bin `b` gets the
    header [workgroup * 256 + b].  Chunk offsets run on through the headers; a chunk that would end past binning_size gets offset 0
    and sets FAILED_BINNING.  bump.lines > lines_size on entry: FAILED_FLATTEN and nothing else."""
    binning_size, n_wgs = case.binning_size, case.n_wgs
    bump = np.zeros(8, np.uint32)
    bump[BUMP["lines"]] = case.lines_on_entry
    out = {"bump": bump, "boxes": None, "headers": None}
    if case.lines_on_entry > case.lines_size:
        bump[BUMP["failed"]] = FAILED_FLATTEN
        return out
    out["boxes"], lists = _covered_bins(case)
    headers = np.zeros((n_wgs * WG, 2), np.uint32)
    size = case.bin_data_words
    data, defined, unspecified = poisoned(size), np.zeros(size, bool), np.zeros(size, bool)
    offset = 0
    for key in sorted(lists):
        headers[key[0] * WG + key[1], 0] = len(lists[key])
    for h in range(len(headers)):
        count = int(headers[h, 0])
        if offset + count > binning_size:
            bump[BUMP["failed"]] |= FAILED_BINNING
            unspecified[case.bin_data_start:case.bin_data_start + count] = True
        else:
            headers[h, 1] = offset
            if count:
                at = case.bin_data_start + offset
                data[at:at + count] = lists[(h // WG, h % WG)]
                defined[at:at + count] = True
        offset += count
    bump[BUMP["binning"]] = offset
    defined &= ~unspecified
    out.update(headers=headers, bin_data=data, defined=defined, unspecified=unspecified)
    return out


@functools.lru_cache(maxsize=None)
def binning_cases():
    rng = np.random.default_rng(0x62696e73)
    W = H = 1024  # 4 x 4 bins

    def rand_boxes(n, w, h, p_empty=0.0):
        x0, y0 = rng.integers(-300, w + 100, n), rng.integers(-300, h + 100, n)
        b = np.stack([x0, y0, x0 + rng.integers(1, 700, n), y0 + rng.integers(1, 700, n)], axis=1)
        b[rng.random(n) < p_empty] = CLEARED
        return b
    on_lines = []
    for a, b in ((0, 256), (0, 255), (0, 257), (256, 512), (255, 512), (257, 512), (1, 2), (511, 513)):
        on_lines += [(a, 0, b, 10), (0, a, 10, b), (a, a, b, b)]
    odd = [CLEARED, (10, 10, 10, 10), (20, 10, 10, 20), (10, 20, 20, 10), (5, 5, 5, 300), (5, 5, 300, 5), (300, 0, 300, 700),
           (-500, 10, -1, 300), (-500, 10, 0, 300), (-500, 10, 1, 300), (1024, 10, 2000, 300), (1023, 10, 2000, 300), (10, -500, 300, 0),
           (10, -500, 300, -1), (10, 1024, 300, 3000), (10, 1025, 300, 3000), (-1000000000, -1000000000, 1000000000, 1000000000),
           (-1000000000, 0, -999999000, 1000000000), (999999000, 0, 1000000000, 100), (0x7fffffff, 0, 0x7fffffff, 10),
           (-0x80000000, -0x80000000, 0x7fffffff, 0x7fffffff)]
    clips = np.array([(0, 0, 300, 300), (256, 256, 512, 512), (100, 100, 100, 400), (600, 0, 500, 1024), (-1e9, -1e9, 1e9, 1e9),
                      (255.5, 255.5, 256.5, 256.5)], np.float32)
    whole = (0, 0, 1024, 1024)
    n_c = 3 * len(clips)
    out = [
        BinCase("bin_lines", on_lines, W, H),
        BinCase("empty_inverted_outside_huge", odd, W, H),
        BinCase("one_object", [(100, 100, 600, 300)], W, H),
        # clip_ix 0 (no clip), 1 .. n_clip, n_clip itself and past it (clamped to the last box); two more boxes behind n_clip in the buffer
        BinCase("clip_ix", [whole] * n_c, W, H, clip_ix=np.arange(n_c) % (len(clips) + 3), clips=clips, n_clip=len(clips) - 2),
        BinCase("no_clips_but_clip_ix", [whole] * 4, W, H, clip_ix=[0, 1, 2, 7], clips=clips[:1], n_clip=0),
        BinCase("odd_target_1000x520", rand_boxes(300, 1000, 520), 1000, 520),
        # 32 x 16 = 512 bins: bins 256 and above are dropped
        BinCase("bins_512", np.concatenate([[(0, 0, 8192, 4096), (0, 1792, 8192, 2304), (4000, 2048, 4100, 4096)], rand_boxes(40, 8192, 4096)]), 8192, 4096),
        BinCase("one_covers_all_255_none", [(0, 0, 4096, 4096)] + [CLEARED] * 255, 4096, 4096),
        BinCase("n_256", rand_boxes(256, W, H, 0.2), W, H),
        BinCase("n_257", rand_boxes(257, W, H, 0.2), W, H),
        BinCase("n_3000", rand_boxes(3000, W, H, 0.5), W, H),
        BinCase("n_65537", rand_boxes(65537, W, H, 0.97), W, H),  # 257 workgroups: the loop over the workgroup totals takes a second step
        BinCase("last_workgroups_overflow", rand_boxes(1500, W, H, 0.3), W, H, short_by=1),
        BinCase("everything_overflows", rand_boxes(700, W, H), W, H, short_by=10 ** 9),
        BinCase("lines_overflowed_before", rand_boxes(300, W, H), W, H, lines_over=True),
    ]
    return out


# ---- tile_alloc --------------------------------------------------------------------------------------------------------------------
class TileCase:
    """One tile_alloc dispatch: n draw objects with the draw boxes `boxes` (f32 [n, 4]) and tags `tags`."""

    def __init__(self, name, boxes, width_px, height_px, tags=None, short_by=None, failed_on_entry=0):
        self.name = name
        self.boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        self.n = len(self.boxes)
        self.tags = np.full(self.n, COLOR, np.uint32) if tags is None else np.asarray(tags, np.uint32)
        self.wt, self.ht = (width_px + 15) // 16, (height_px + 15) // 16
        self.short_by, self.failed_on_entry = short_by, failed_on_entry
        self.n_wgs = (self.n + WG - 1) // WG
        self.tiles_size = 1 << 31
        total = int(tile_alloc_by_definition(self)["total"])
        self.tiles_size = total + 37 if short_by is None else max(total - short_by, 0)

    def pack(self):
        scene = np.concatenate([np.full(DRAWTAG_BASE, 0x50, np.uint32), self.tags])
        bump = np.zeros(8, np.uint32)
        bump[BUMP["failed"]] = self.failed_on_entry
        cfg = config(width_in_tiles=self.wt, height_in_tiles=self.ht, n_drawobj=self.n, n_path=self.n, drawtag_base=DRAWTAG_BASE,
                     tiles_size=self.tiles_size)
        return cfg, scene, self.boxes, bump


def tile_alloc_by_definition(case):
    """`paths` [n, 5] (the tile box x0, y0, x1, y1 and the index of the path's first tile), `bump` (8 words), `n_zero`: the tiles
    [0, n_zero) are cleared, n_zero = min(all tiles, tiles_size).

    The rules (tile_alloc.wgsl): an object whose tag is neither nop nor end-clip and whose box has x0 < x1 and y0 < y1 owns the tiles
    [floor(x0 / 16), ceil(x1 / 16)) x [floor(y0 / 16), ceil(y1 / 16)), clamped to the target's tiles; every other object owns none and
    has the box (0, 0, 0, 0).  Tiles are dealt in object order.  A workgroup of 256 objects whose tiles would end past tiles_size
    starts at 0 instead and sets FAILED_TILE_ALLOC.  FAILED_BINNING or FAILED_FLATTEN on entry: nothing is written."""
    tiles_size = case.tiles_size
    bump = np.zeros(8, np.uint32)
    bump[BUMP["failed"]] = case.failed_on_entry
    box = case.boxes
    live = (case.tags != NOP) & (case.tags != END_CLIP) & (box[:, 0] < box[:, 2]) & (box[:, 1] < box[:, 3])
    scaled = box * np.float32(1.0 / 16.0)
    lo, hi = np.floor(scaled[:, :2]).astype(np.int64), np.ceil(scaled[:, 2:]).astype(np.int64)
    x0, y0 = np.clip(np.where(live, lo[:, 0], 0), 0, case.wt), np.clip(np.where(live, lo[:, 1], 0), 0, case.ht)
    x1, y1 = np.clip(np.where(live, hi[:, 0], 0), 0, case.wt), np.clip(np.where(live, hi[:, 1], 0), 0, case.ht)
    count = ((x1 - x0) * (y1 - y0)).astype(np.uint32)
    first = excl_cumsum(count[:, None])[:, 0].astype(np.int64)
    total = int(count.sum(dtype=np.uint64))
    assert total < 1 << 32
    if case.failed_on_entry & (FAILED_BINNING | FAILED_FLATTEN):
        return {"bump": bump, "paths": None, "n_zero": 0, "total": total}
    paths = np.stack([x0, y0, x1, y1, first], axis=1).astype(np.uint32)
    for w in range(case.n_wgs):
        sl = slice(w * WG, min((w + 1) * WG, case.n))
        wg_first, wg_count = int(first[sl][0]), int(count[sl].sum(dtype=np.uint64))
        if wg_first + wg_count > tiles_size:
            bump[BUMP["failed"]] |= FAILED_TILE_ALLOC
            paths[sl, 4] -= np.uint32(wg_first)
    bump[BUMP["tile"]] = total
    return {"bump": bump, "paths": paths, "n_zero": min(total, tiles_size), "total": total}


@functools.lru_cache(maxsize=None)
def tile_alloc_cases():
    rng = np.random.default_rng(0x74696c65)
    W, H = 1000, 520  # 63 x 33 tiles: not a multiple of 16 px

    def rand(n, p_empty=0.3):
        x0, y0 = rng.uniform(-100, W + 50, n), rng.uniform(-100, H + 50, n)
        b = np.stack([x0, y0, x0 + rng.uniform(0.01, 200, n), y0 + rng.uniform(0.01, 200, n)], axis=1).astype(np.float32)
        b[rng.random(n) < p_empty] = (1e9, 1e9, -1e9, -1e9)
        return b

    def tags_for(n):
        t = np.full(n, COLOR, np.uint32)
        t[2::7], t[3::11], t[5::13] = NOP, END_CLIP, BEGIN_CLIP
        return t
    on_lines = []
    for a, b in ((0, 16), (0, 15), (0, 17), (16, 32), (15.5, 32), (16.5, 32.5), (992, 1000), (992, 1008), (999, 1001), (31.999, 32.001)):
        on_lines += [(a, 0, b, 10), (0, a, 10, min(b, 600)), (a, a, b, b)]
    odd = [(10, 10, 10, 10), (20, 10, 10, 20), (5, 5, 5, 300), (5, 5, 300, 5), (-500, 10, -1, 300), (-500, 10, 0.001, 300), (1000, 10, 2000, 300),
           (1008, 10, 2000, 300), (10, 528, 300, 3000), (10, 519.5, 300, 3000), (-1e9, -1e9, 1e9, 1e9), (0, 0, 1000, 520), (0, 0, 1008, 528)]
    even = rand(513)
    out = [
        TileCase("tile_lines", on_lines, W, H),
        TileCase("empty_inverted_outside_huge", odd, W, H),
        TileCase("one_object", [(3, 3, 40, 40)], W, H),
        TileCase("nop_and_end_clip_count_zero", rand(600, 0.0), W, H, tags=tags_for(600)),
        TileCase("n_256", rand(256), W, H),
        TileCase("n_257", rand(257), W, H, tags=tags_for(257)),
        TileCase("n_65537", rand(65537, 0.9), W, H, tags=tags_for(65537)),
        TileCase("no_tiles_at_all", [(1e9, 1e9, -1e9, -1e9)] * 300, W, H),
        TileCase("one_tile_too_small", rand(1500), W, H, short_by=1),
        TileCase("far_too_small", rand(1500), W, H, short_by=10 ** 9),
        TileCase("binning_failed_before", rand(300), W, H, failed_on_entry=FAILED_BINNING),
        TileCase("flatten_failed_before", rand(300), W, H, failed_on_entry=FAILED_FLATTEN),
        TileCase("tile_alloc_failed_before", rand(300), W, H, failed_on_entry=FAILED_TILE_ALLOC),  # (its own bit does not stop it)
    ]
    # a total that is even and one that is odd: the clear stores two tiles at a time and patches the odd one
    parity = tile_alloc_by_definition(TileCase("", even, W, H))["total"] % 2
    names = ("total_even", "total_odd") if parity == 0 else ("total_odd", "total_even")
    out += [TileCase(names[0], even, W, H), TileCase(names[1], np.concatenate([even, [(0, 0, 16, 16)]]), W, H)]  # (one tile more)
    return out


# ---- the u32 scan ------------------------------------------------------------------------------------------------------------------
def scan_u32(values, stride, n):
    """(out [n], total): out[i] = the sum of values[0], values[stride], ... values[(i - 1) * stride] mod 2^32."""
    v = np.asarray(values, np.uint32)[:n * stride:stride][:n]
    inc = np.cumsum(v, dtype=np.uint32)
    out = np.zeros(n, np.uint32)
    out[1:] = inc[:-1]
    return out, int(inc[-1]) if n else 0


SCAN_N = (0, 1, 63, 64, 65, 16383, 16384, 16385, 32767, 32769, 64 * LB_TILE + 1, 65 * LB_TILE + 16385)


def scan_values(n, stride, kind):
    if kind == "ones":
        return np.ones(max(n * stride, 1), np.uint32)
    if kind == "zeros":
        return np.zeros(max(n * stride, 1), np.uint32)
    return np.random.default_rng(0x7363616e + n + stride).integers(0, 1 << 32, max(n * stride, 1), dtype=np.uint64).astype(np.uint32)


# ---- buffers, dispatch lists, the oracle, and the checks both test modules make -----------------------------------------------------
def scene_of_objects(n):
    """A scene of n draw objects (a small rectangle each), by doubling."""
    from jello_amd import scene as S
    chunk, out = S.Scene(), S.Scene()
    chunk.fill(S.Fill.NonZero, None, S.Brush.solid((1, 0, 0, 1)), None, S.Path.rect(1, 1, 3, 3))
    while n:
        if n & 1:
            out.append(chunk)
        n >>= 1
        if n:
            twice = S.Scene()
            twice.append(chunk)
            twice.append(chunk)
            chunk = twice
    return out


def pathtag_job(scene, counts):
    """(buffers, dispatches) of the path-tag scan as the host records it for these counts: name -> array, and (stage, workgroups,
    bound buffer names).  Outputs are poisoned; so is the tail of `reduced` that no workgroup writes."""
    sz = counts["sizes"]
    bufs = {"cfg": config(pathtag_base=PATHTAG_BASE), "scene": scene, "reduced": poisoned((sz["reduced"] // 20, 5)),
            "tagmonoid": poisoned((sz["tagmonoid"] // 20, 5))}
    if not counts["large"]:
        return bufs, [("pathtag_reduce", counts["reduce"], ["cfg", "scene", "reduced"]),
                      ("pathtag_scan_small", counts["scan"], ["cfg", "scene", "reduced", "tagmonoid"])]
    bufs["reduced2"], bufs["reduced_scan"] = poisoned((sz["reduced2"] // 20, 5)), poisoned((sz["reduced_scan"] // 20, 5))
    return bufs, [("pathtag_reduce", counts["reduce"], ["cfg", "scene", "reduced"]),
                  ("pathtag_reduce2", counts["reduce2"], ["reduced", "reduced2"]),
                  ("pathtag_scan1", counts["scan1"], ["reduced", "reduced2", "reduced_scan"]),
                  ("pathtag_scan_large", counts["scan"], ["cfg", "scene", "reduced_scan", "tagmonoid"])]


def check_pathtag(got, want, counts, who):
    n = counts["reduce"]
    assert np.array_equal(got["reduced"][:n], want["reduced"]), who + ": reduced"
    assert np.all(got["reduced"][n:] == POISON), who + ": reduced behind the written workgroups"
    if counts["large"]:
        bad = np.flatnonzero((got["reduced2"] != want["reduced2"]).any(axis=1))
        assert bad.size == 0, "%s: reduced2 differs at entries %s (scan1 grid %d)" % (who, bad[:8], counts["scan1"])
        assert np.array_equal(got["reduced_scan"][:n], want["reduced_scan"]), who + ": reducedScan"
    bad = np.flatnonzero((got["tagmonoid"] != want["tagmonoid"]).any(axis=1))
    assert bad.size == 0, "%s: %d tag monoids differ, first at word %d: %s want %s" % (
        who, bad.size, bad[0], got["tagmonoid"][bad[0]], want["tagmonoid"][bad[0]])


def draw_job(n, n_wgs):
    cfg, scene, pb, tags, (n_path, n_clip, n_info) = draw_pack(n)
    bufs = {"cfg": cfg, "scene": scene, "path_bbox": pb, "draw_reduced": poisoned((n_wgs, 4)), "draw_monoid": poisoned((n, 4)),
            "info": poisoned(n_info), "clip_inp": poisoned((n_clip, 2))}
    return bufs, [("draw_reduce", n_wgs, ["cfg", "scene", "draw_reduced"]),
                  ("draw_leaf", n_wgs, ["cfg", "scene", "draw_reduced", "path_bbox", "draw_monoid", "info", "clip_inp"])], tags


def check_draw(got, want, who):
    assert np.array_equal(got["draw_reduced"], want["draw_reduced"]), who + ": draw_reduced"
    bad = np.flatnonzero((got["draw_monoid"] != want["draw_monoid"]).any(axis=1))
    assert bad.size == 0, "%s: %d draw monoids differ, first at object %d: %s want %s" % (
        who, bad.size, bad[0], got["draw_monoid"][bad[0]], want["draw_monoid"][bad[0]])
    assert np.array_equal(got["clip_inp"], want["clip_inp"]), who + ": clip_inp (records and the poison between them)"
    assert np.array_equal(got["info"], want["info"]), who + ": info (the words of the 0x50 objects and the poison between them)"


def binning_job(case, extra=16):
    """`extra`: poisoned elements behind every output, which must come back untouched."""
    cfg, dm, pb, clips, bump = case.pack()
    bufs = {"cfg": cfg, "dm": dm, "path_bbox": pb, "clip_bbox": clips, "boxes": poisoned((case.n + extra, 4)), "bump": bump,
            "bin_data": poisoned(case.bin_data_words), "headers": poisoned((case.n_wgs * WG + extra, 2))}
    return bufs, [("binning", case.n_wgs, ["cfg", "dm", "path_bbox", "clip_bbox", "boxes", "bump", "bin_data", "headers"])]


def check_binning(got, want, case, who):
    assert np.array_equal(got["bump"], want["bump"]), "%s: bump %s want %s" % (who, got["bump"], want["bump"])
    n, nh = case.n, case.n_wgs * WG
    if want["boxes"] is None:  # the early-out: nothing but the failed bit
        assert all(np.all(got[k] == POISON) for k in ("boxes", "headers", "bin_data")), who + ": written to after the early-out"
        return
    bad = np.flatnonzero((got["boxes"][:n] != want["boxes"].view(np.uint32)).any(axis=1))
    assert bad.size == 0, "%s: intersected boxes differ at %s, first %s want %s" % (
        who, bad[:8], got["boxes"][bad[0]].view(np.float32), want["boxes"][bad[0]])
    bad = np.flatnonzero((got["headers"][:nh] != want["headers"]).any(axis=1))
    assert bad.size == 0, "%s: bin headers differ at %s, first %s want %s" % (who, bad[:8], got["headers"][bad[0]], want["headers"][bad[0]])
    assert np.all(got["boxes"][n:] == POISON) and np.all(got["headers"][nh:] == POISON), who + ": boxes / headers behind the last element"
    data, d, u = got["bin_data"], want["defined"], want["unspecified"]
    assert np.array_equal(data[d], want["bin_data"][d]), who + ": bin_data lists"
    assert np.all(data[~(d | u)] == POISON), who + ": bin_data outside the lists"


def tile_alloc_job(case, extra=64):
    cfg, scene, boxes, bump = case.pack()
    bufs = {"cfg": cfg, "scene": scene, "draw_bbox": boxes, "bump": bump, "paths": poisoned((case.n_wgs * WG + extra, 8)),
            "tiles": poisoned((case.tiles_size + extra, 2))}
    return bufs, [("tile_alloc", case.n_wgs, ["cfg", "scene", "draw_bbox", "bump", "paths", "tiles"])]


def check_tile_alloc(got, want, case, who, oracle=False):
    """oracle=True makes the two exceptions test_element_spec.py names: TILE_ALLOC_BROADCAST_SLOT and TILE_ALLOC_CLEAR_ON_OVERFLOW."""
    assert np.array_equal(got["bump"], want["bump"]), "%s: bump %s want %s" % (who, got["bump"], want["bump"])
    n = case.n
    if want["paths"] is None:
        assert np.all(got["paths"] == POISON) and np.all(got["tiles"] == POISON), who + ": written to after the early-out"
        return
    bad = np.flatnonzero((got["paths"][:n, :5] != want["paths"]).any(axis=1))
    assert bad.size == 0, "%s: paths differ at %s, first %s want %s" % (who, bad[:8], got["paths"][bad[0], :5], want["paths"][bad[0]])
    behind = got["paths"][n:].copy()
    if oracle:
        behind[np.arange(n, len(got["paths"])) % WG == WG - 1, 4] = POISON
    assert np.all(behind == POISON), who + ": paths behind the last draw object"
    if oracle and want["bump"][BUMP["failed"]] & FAILED_TILE_ALLOC:
        return
    z = want["n_zero"]
    assert np.all(got["tiles"][:z] == 0), who + ": tiles [0, %d) are not all zero" % z
    assert np.all(got["tiles"][z:] == POISON), who + ": tiles from %d on were written to" % z


def run_oracle(bufs, dispatches):
    """The dispatches on the oracle, on copies of `bufs`; returns the copies."""
    from oracle.oracle_engine import OBuf, lib
    L = lib()
    out = {k: np.ascontiguousarray(v).copy() for k, v in bufs.items()}
    for stage, gx, names in dispatches:
        b = (OBuf * len(names))(*[OBuf(out[k].ctypes.data, out[k].nbytes) for k in names])
        assert L.oracle_dispatch(STAGE[stage], gx, 1, 1, b, len(names)) == 0, stage
    return {k: (v.view(np.uint32) if v.dtype.itemsize == 4 else v) for k, v in out.items()}
