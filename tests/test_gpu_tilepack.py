"""-m gpu: jh_pack_tiles / jh_unpack_tiles (include/jello_hip.h "tile-packed frame transport") against
tests/tilepack_ref.py, the numpy restatement of the format text: byte for byte over the pack's whole size, poison beyond it,
pitches and alignments, frames of one class, rendered frames in both texel sizes, a captured graph, determinism, refused
calls, malformed packs behind a guard band, band mode and the profiler.  The answer is exact: no tolerance anywhere."""
import ctypes
import struct

import numpy as np
import pytest

import jello_amd
from jello_amd import Surface, scenes, tilepack
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS

import tilepack_ref as ref
from devmem import CANARY, DevBuf
from tilepack_cases import CASES, DTYPES, case_frames, make_frame

pytestmark = pytest.mark.gpu

def laid_out(frame, pitch, offset, tail=64):
    """The frame's rows `pitch` bytes apart, `offset` bytes into a CANARY-filled byte array with `tail` bytes behind."""
    h, w = frame.shape[:2]
    tb = 4 * frame.dtype.itemsize
    host = np.full(offset + pitch * h + tail, CANARY, np.uint8)
    rows = host[offset:offset + pitch * h].reshape(h, pitch)
    rows[:, :w * tb] = np.ascontiguousarray(frame).view(np.uint8).reshape(h, w * tb)
    return host


def poison_frame(h, w, tb):
    return np.full((h, w, tb), CANARY, np.uint8).view(DTYPES[tb]).reshape(h, w, 4)


def frame_of(host, h, w, tb, pitch, offset):
    rows = host[offset:offset + pitch * h].reshape(h, pitch)
    return np.ascontiguousarray(rows[:, :w * tb]).view(DTYPES[tb]).reshape(h, w, 4)


def check_pack_and_unpack(engine, f, r, src_pitch=None, src_offset=0, ref_pitch=None, ref_offset=0, dst_offset=0, what=""):
    """jh_pack_tiles of f (against r) = ref.pack over the pack's whole size, CANARY beyond it; jh_unpack_tiles of that pack into a
    poisoned frame with the same pitch = ref.unpack into poison, with the pitch padding and everything around it untouched."""
    h, w = f.shape[:2]
    tb = 4 * f.dtype.itemsize
    src_pitch = w * tb if src_pitch is None else src_pitch
    ref_pitch = w * tb if ref_pitch is None else ref_pitch
    want = ref.pack(f, r)
    bound = tilepack.bound(w, h, tb)
    assert len(want) <= bound
    bufs = []
    try:
        src = DevBuf(engine, data=laid_out(f, src_pitch, src_offset))
        bufs.append(src)
        rb = None
        if r is not None:
            rb = DevBuf(engine, data=laid_out(r, ref_pitch, ref_offset))
            bufs.append(rb)
        dst = DevBuf(engine, dst_offset + bound + 256)
        bufs.append(dst)
        engine.pack_tiles(src.ptr + src_offset, src_pitch, w, h, tb, ref_ptr=None if rb is None else rb.ptr + ref_offset,
                          ref_pitch=ref_pitch, out_device_ptr=dst.ptr + dst_offset, out_capacity=bound)
        engine.sync()
        got = dst.bytes()
        body = got[dst_offset:dst_offset + len(want)].tobytes()
        if body != want:
            i = next(i for i in range(len(want)) if body[i] != want[i])
            raise AssertionError("%s: pack differs from the reference at byte %d of %d (got %d, want %d); headers %r / %r" %
                                 (what, i, len(want), body[i], want[i], struct.unpack_from("<8I", body), struct.unpack_from("<8I", want)))
        assert np.all(got[:dst_offset] == CANARY) and np.all(got[dst_offset + len(want):] == CANARY), what + ": bytes beyond the pack written"
        assert engine.read_pack(dst.ptr + dst_offset, bound) == want
        # unpack, from the device copy of the pack, into poison
        out = DevBuf(engine, src_offset + src_pitch * h + 64)
        bufs.append(out)
        before = engine.unpack_rejects()
        engine.unpack_tiles((dst.ptr + dst_offset, len(want)), out.ptr + src_offset, src_pitch, w, h, tb)
        assert engine.unpack_rejects() == before
        expect = poison_frame(h, w, tb)
        assert ref.unpack(want, expect) == 0
        got = out.bytes()
        assert np.array_equal(got, laid_out(expect, src_pitch, src_offset)), what + ": unpack differs (or wrote outside the frame's texels)"
    finally:
        for b in bufs:
            b.free()
    return want


@pytest.mark.parametrize("w,h,tb,kind", CASES)
def test_battery_matches_reference(engine, w, h, tb, kind):
    f, r = case_frames(w, h, tb, kind)
    check_pack_and_unpack(engine, f, r, what="%dx%d tb%d %s" % (w, h, tb, kind))


@pytest.mark.parametrize("tb", [4, 8])
@pytest.mark.parametrize("layout", ["pitch+64", "pitch+tb", "offset_tb", "dst_offset_tb", "ref_other_pitch"])
def test_pitch_and_alignment(engine, tb, layout):
    """A pitch larger than the row (16-B aligned rows with padding), a pitch of texel_bytes * width + texel_bytes (rows at
    every texel alignment), frames and packs that start one texel off a 16-B boundary, a reference with a pitch of its own."""
    w, h = 203, 77
    f = make_frame(w, h, tb, 5)
    f2, r = case_frames(w, h, tb, "mixed")
    kw = {"pitch+64": dict(src_pitch=(w * tb + 15) // 16 * 16 + 64), "pitch+tb": dict(src_pitch=w * tb + tb, ref_pitch=w * tb + tb),
          "offset_tb": dict(src_offset=tb, ref_offset=16 - tb), "dst_offset_tb": dict(dst_offset=tb),
          "ref_other_pitch": dict(ref_pitch=w * tb + 48)}[layout]
    check_pack_and_unpack(engine, f, None, what=layout, **{k: v for k, v in kw.items() if not k.startswith("ref")})
    check_pack_and_unpack(engine, f2, r, what=layout + " with a reference", **kw)


@pytest.mark.parametrize("tb", [4, 8])
@pytest.mark.parametrize("w,h", [(250, 40), (1000, 700)])
def test_frames_of_one_class(engine, tb, w, h):
    """All-SKIP (the pack is the header alone), all-SOLID, all-RAW (the pack reaches jh_pack_bound); 1000 x 700 is 2 772 tiles,
    44 workgroups per pass."""
    rng = np.random.default_rng(w + tb)
    noise = rng.integers(0, 256, size=(h, w, 4)).astype(DTYPES[tb]) | 1
    flat = np.empty_like(noise)
    flat[...] = np.array([1, 2, 3, 0xF0], DTYPES[tb])
    p = check_pack_and_unpack(engine, noise, noise.copy(), what="all SKIP")
    assert len(p) == 32
    p = check_pack_and_unpack(engine, flat, None, what="all SOLID")
    n = ((w + 15) // 16) * ((h + 15) // 16)
    assert struct.unpack_from("<8I", p)[4:7] == (n, n, 0)
    p = check_pack_and_unpack(engine, noise, None, what="all RAW")
    assert struct.unpack_from("<8I", p)[4:7] == (n, 0, n) and len(p) == tilepack.bound(w, h, tb)
    p = check_pack_and_unpack(engine, noise, flat, what="all RAW against a reference")
    assert struct.unpack_from("<8I", p)[4:8] == (n, 0, n, 1)


def test_more_tiles_than_one_run_of_64_per_workgroup(engine):
    """4096 x 4112 texels = 65 792 tiles: the workgroups' runs grow beyond 64 tiles and the last one is short.  Mostly flat
    (a frame of noise this size would only make the reference slow), with noisy and changed tiles spread over it."""
    w, h = 4096, 4112
    rng = np.random.default_rng(17)
    a = np.zeros((h, w, 4), np.uint8)
    a[...] = (10, 20, 30, 255)
    for _ in range(600):
        y, x = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
        a[y:y + 40, x:x + 40] = rng.integers(0, 256, size=(40, 40, 4), dtype=np.uint8)
    b = a.copy()
    for i in range(300):
        y, x = int(rng.integers(0, h - 24)), int(rng.integers(0, w - 24))
        b[y:y + 24, x:x + 24] = (200, 0, 0, 255) if i % 2 else rng.integers(0, 256, size=(24, 24, 4), dtype=np.uint8)
    b[-1, -1] = (1, 1, 1, 1)  # the last tile
    cls = ref.classify(b, a)
    assert {ref.SKIP, ref.SOLID, ref.RAW} == set(cls) and cls[-1] == ref.RAW
    check_pack_and_unpack(engine, b, a, what="65 792 tiles with a reference")
    check_pack_and_unpack(engine, a, None, what="65 792 tiles")


def _two_scenes():
    return scenes.scene_large_shapes(1536, 60), scenes.scene_large_shapes(1536, 61)  # (the 61st shape is a stroked circle)


def test_rendered_surfaces_travel_as_a_pack(engine):
    """render_to_surface of two scenes that differ by one shape; the second packed against the first, downloaded and applied
    to the host copy of the first gives the full download of the second."""
    (s0, p0), (s1, p1) = _two_scenes()
    w, h = p0.width, p0.height
    a, b = DevBuf(engine, 4 * w * h), DevBuf(engine, 4 * w * h)
    try:
        for (s, p, buf) in ((s0, p0, a), (s1, p1, b)):
            _, _, bump, _ = engine.render_to_surface(s, p, Surface.RGBA8_UNORM, out_device_ptr=buf.ptr)
            assert bump["failed"] == 0
        pack = engine.pack_tiles(b.ptr, 4 * w, w, h, 4, ref_ptr=a.ptr)
        host_a, host_b = a.bytes().reshape(h, w, 4), b.bytes().reshape(h, w, 4)
        assert not np.array_equal(host_a, host_b)
        assert pack == ref.pack(host_b, host_a)
        hdr = tilepack.parse_header(pack)
        assert 0 < hdr["n_entries"] < (w // 16) * (h // 16) // 4 and len(pack) < host_b.nbytes // 4  # one shape is a small part
        out = host_a.copy()
        assert tilepack.apply(pack, out) == 0
        assert np.array_equal(out, host_b)
        # and on the device: unpack into the first surface makes it the second
        engine.unpack_tiles(pack, a.ptr, 4 * w, w, h, 4)
        engine.sync()
        assert np.array_equal(a.bytes().reshape(h, w, 4), host_b)
    finally:
        a.free()
        b.free()


def test_rendered_rgba16f_targets_travel_as_a_pack(engine):
    """The same with the RGBA16F target itself (texel_bytes = 8)."""
    (s0, p0), (s1, p1) = _two_scenes()
    w, h = p0.width, p0.height
    a, b = DevBuf(engine, 8 * w * h), DevBuf(engine, 8 * w * h)
    try:
        for (s, p, buf) in ((s0, p0, a), (s1, p1, b)):
            rec, bump, _ = engine.render(s, p, out_device_ptr=buf.ptr)
            assert bump["failed"] == 0
        engine.sync()
        pack = engine.pack_tiles(b.ptr, 8 * w, w, h, 8, ref_ptr=a.ptr, ref_pitch=8 * w)
        host_a = a.bytes().view(np.uint16).reshape(h, w, 4)
        host_b = b.bytes().view(np.uint16).reshape(h, w, 4)
        assert not np.array_equal(host_a, host_b)
        assert pack == ref.pack(host_b, host_a)
        out = host_a.copy()
        assert tilepack.apply(pack, out) == 0
        assert np.array_equal(out, host_b)
        # without a reference the whole frame travels and lands in a poisoned array
        whole = engine.pack_tiles(b.ptr, 8 * w, w, h, 8)
        assert whole == ref.pack(host_b)
        out = poison_frame(h, w, 8)
        assert tilepack.apply(whole, out) == 0 and np.array_equal(out, host_b)
    finally:
        a.free()
        b.free()


def test_captured_frame_blit_pack(engine):
    """capture(recording, surface=..., pack=...): frame -> blit -> pack as one graph.  The pack adds exactly its two kernel
    launches and no other node; two replays give the same bytes, the reference's pack of the blitted surface."""
    s, p = scenes.scene_c3(3000, 1024)
    p.bump = jello_amd.BumpSizes(ptcl=1 << 23, blend_spill=1 << 20)
    w, h = p.width, p.height
    rec = jello_amd.Host().record(s, p)
    engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
    engine.sync()
    assert engine.download(rec.buffer("bumpBuf")[0], dtype=np.uint32)[0] == 0
    cap = tilepack.bound(w, h, 4)
    surf, dst = DevBuf(engine, 4 * w * h), DevBuf(engine, cap)
    g0 = g1 = None
    try:
        engine.pack_tiles(surf.ptr, 4 * w, w, h, 4, out_device_ptr=dst.ptr)  # once eagerly: the scratch arrays exist
        engine.sync()
        g0 = engine.capture(rec, surface=(surf.ptr, 4 * w, Surface.RGBA8_SRGB))
        g1 = engine.capture(rec, surface=(surf.ptr, 4 * w, Surface.RGBA8_SRGB), pack=(surf.ptr, 4 * w, None, 0, dst.ptr, cap, 4))
        k0, o0 = engine.graph_node_counts(g0)
        k1, o1 = engine.graph_node_counts(g1)
        assert k1 == k0 + 2 and o1 == o0, ((k0, o0), (k1, o1))
        outs = []
        for _ in range(2):
            engine.clear(dst.id)
            engine.clear(surf.id)
            engine.replay(g1)
            engine.sync()
            outs.append(engine.read_pack(dst.ptr, cap))
        want = ref.pack(surf.bytes().reshape(h, w, 4))
        assert outs[0] == outs[1] == want
        assert tilepack.parse_header(want)["n_raw"] > 0 and tilepack.parse_header(want)["n_solid"] > 0
    finally:
        for g in (g0, g1):
            if g is not None:
                engine.graph_destroy(g)
        engine.release(rec)
        surf.free()
        dst.free()


def test_packing_twice_gives_identical_bytes(engine):
    """Determinism: the same frame packed into two poisoned destinations, and once more after other work on the context."""
    f, r = case_frames(250, 40, 4, "mixed")
    big = make_frame(1000, 700, 8, 77)
    outs = []
    for frame, rf in ((f, r), (big, None)):
        h, w = frame.shape[:2]
        tb = 4 * frame.dtype.itemsize
        cap = tilepack.bound(w, h, tb) + 128
        src = DevBuf(engine, data=frame.tobytes())
        rb = DevBuf(engine, data=rf.tobytes()) if rf is not None else None
        d = [DevBuf(engine, cap) for _ in range(3)]
        try:
            for i, dst in enumerate(d):
                if i == 2:
                    engine.debug_poison_scratch(0x5A)  # what the scratch arrays held before must not matter
                engine.pack_tiles(src.ptr, w * tb, w, h, tb, ref_ptr=None if rb is None else rb.ptr, out_device_ptr=dst.ptr, out_capacity=cap)
            engine.sync()
            got = [x.bytes().tobytes() for x in d]
            assert got[0] == got[1] == got[2]
            outs.append(got[0])
        finally:
            for x in d + [src] + ([rb] if rb else []):
                x.free()
    assert len(outs) == 2


def test_refused_calls_touch_nothing(engine):
    """Every JH_ERR_INVALID case leaves the destination as it was, and a valid call on the same context works after each."""
    hip, ctx = engine.hip, engine.ctx
    w, h, tb = 37, 21, 4
    f = make_frame(w, h, tb, 8)
    want = ref.pack(f)
    bound = tilepack.bound(w, h, tb)
    src = DevBuf(engine, data=laid_out(f, 4 * w, 0))
    src8 = DevBuf(engine, data=laid_out(make_frame(w, h, 8, 9), 8 * w, 0))
    canary = DevBuf(engine, bound + 256)
    good = DevBuf(engine, bound)
    packbuf = DevBuf(engine, data=want)
    frame = DevBuf(engine, 4 * w * h + 64)
    assert hip.jh_pack_bound(w, h, 3) == 0 and hip.jh_pack_bound(w, h, 4) == bound
    pack_cases = [
        ("null src", (None, 4 * w, None, 0, w, h, 4, canary.ptr, bound)),
        ("null dst", (src.ptr, 4 * w, None, 0, w, h, 4, None, bound)),
        ("texel size 3", (src.ptr, 4 * w, None, 0, w, h, 3, canary.ptr, bound)),
        ("texel size 16", (src.ptr, 16 * w, None, 0, w, h, 16, canary.ptr, bound * 4)),
        ("texel size 0", (src.ptr, 4 * w, None, 0, w, h, 0, canary.ptr, bound)),
        ("pitch below the row", (src.ptr, 4 * w - 4, None, 0, w, h, 4, canary.ptr, bound)),
        ("pitch not a multiple of 4", (src.ptr, 4 * w + 2, None, 0, w, h, 4, canary.ptr, bound)),
        ("src not a multiple of 4", (src.ptr + 2, 4 * w, None, 0, w, h, 4, canary.ptr, bound)),
        ("src not a multiple of 8", (src8.ptr + 4, 8 * w, None, 0, w, h, 8, canary.ptr, 2 * bound)),
        ("pitch not a multiple of 8", (src8.ptr, 8 * w + 4, None, 0, w, h, 8, canary.ptr, 2 * bound)),
        ("dst not a multiple of 4", (src.ptr, 4 * w, None, 0, w, h, 4, canary.ptr + 1, bound)),
        ("ref pitch below the row", (src.ptr, 4 * w, src.ptr, 4 * w - 4, w, h, 4, canary.ptr, bound)),
        ("ref not a multiple of 4", (src.ptr, 4 * w, src.ptr + 1, 4 * w, w, h, 4, canary.ptr, bound)),
        ("capacity below the bound", (src.ptr, 4 * w, None, 0, w, h, 4, canary.ptr, bound - 1)),
        ("width 0", (src.ptr, 4 * w, None, 0, 0, h, 4, canary.ptr, bound)),
        ("height 0", (src.ptr, 4 * w, None, 0, w, 0, 4, canary.ptr, bound)),
    ]
    unpack_cases = [
        ("null pack", (None, len(want), canary.ptr, 4 * w, w, h, 4)),
        ("null dst", (packbuf.ptr, len(want), None, 4 * w, w, h, 4)),
        ("pack_bytes below 32", (packbuf.ptr, 31, canary.ptr, 4 * w, w, h, 4)),
        ("texel size 2", (packbuf.ptr, len(want), canary.ptr, 4 * w, w, h, 2)),
        ("pitch below the row", (packbuf.ptr, len(want), canary.ptr, 4 * w - 4, w, h, 4)),
        ("pitch not a multiple of 4", (packbuf.ptr, len(want), canary.ptr, 4 * w + 1, w, h, 4)),
        ("dst not a multiple of 4", (packbuf.ptr, len(want), canary.ptr + 2, 4 * w, w, h, 4)),
        ("pack not a multiple of 4", (packbuf.ptr + 2, len(want) - 2, canary.ptr, 4 * w, w, h, 4)),
        ("width 0", (packbuf.ptr, len(want), canary.ptr, 4 * w, 0, h, 4)),
        ("height 0", (packbuf.ptr, len(want), canary.ptr, 4 * w, w, 0, 4)),
    ]
    try:
        for fn, cases in ((hip.jh_pack_tiles, pack_cases), (hip.jh_unpack_tiles, unpack_cases)):
            for what, args in cases:
                assert fn(ctx, *args) == JH_ERR_INVALID, what
                engine.sync()
                assert np.all(canary.bytes() == CANARY), what
                assert hip.jh_pack_tiles(ctx, src.ptr, 4 * w, None, 0, w, h, 4, good.ptr, bound) == 0, what
                assert hip.jh_unpack_tiles(ctx, good.ptr, bound, frame.ptr, 4 * w, w, h, 4) == 0, what
                engine.sync()
                assert good.bytes()[:len(want)].tobytes() == want, "valid pack after " + what
                assert np.array_equal(frame_of(frame.bytes(), h, w, 4, 4 * w, 0), f), "valid unpack after " + what
        assert engine.unpack_rejects() == 0
    finally:
        for b in (src, src8, canary, good, packbuf, frame):
            b.free()


def _set_entry(p, e, word0=None, word1=None):
    b = bytearray(p)
    w0, w1 = struct.unpack_from("<II", b, 32 + 8 * e)
    struct.pack_into("<II", b, 32 + 8 * e, w0 if word0 is None else word0, w1 if word1 is None else word1)
    return bytes(b)


def _set_header(p, i, v):
    b = bytearray(p)
    struct.pack_into("<I", b, 4 * i, v)
    return bytes(b)


@pytest.mark.parametrize("tb", [4, 8])
def test_malformed_packs_on_the_device(engine, tb):
    """Packs a wire could deliver: the reject counter rises by what the reference rejects, the frame is what the reference's
    unpack leaves, and the guard band around the frame (pitch padding included) keeps its poison.  pack_bytes is the exact
    length of the uploaded bytes; the buffer behind it is poison, so a read beyond pack_bytes would show as wrong texels."""
    w, h = 50, 40  # 4 x 3 tiles
    f = make_frame(w, h, tb, 99)
    p = ref.pack(f)
    n_entries, n_solid, n_raw = struct.unpack_from("<8I", p, 0)[4:7]
    first_raw = next(e for e in range(n_entries) if struct.unpack_from("<I", p, 32 + 8 * e)[0] >> 31)
    first_solid = next(e for e in range(n_entries) if not struct.unpack_from("<I", p, 32 + 8 * e)[0] >> 31)
    all_bad = p
    for e in range(n_entries):
        all_bad = _set_entry(all_bad, e, word0=(struct.unpack_from("<I", p, 32 + 8 * e)[0] & 0x80000000) | (12 + e))
    cases = {
        "a good pack": p,
        "tile index = tile count": _set_entry(p, first_solid, word0=12),
        "raw tile index far out of range": _set_entry(p, first_raw, word0=0xFFFFFFFF),
        "solid payload index = n_solid": _set_entry(p, first_solid, word1=n_solid),
        "raw payload index = n_raw": _set_entry(p, first_raw, word1=n_raw),
        "raw payload index huge": _set_entry(p, first_raw, word1=0xFFFFFFFF),
        "every tile index out of range": all_bad,
        "truncated inside the raw section": p[:-tb],
        "truncated to the header": p[:32],
        "magic": _set_header(p, 0, 0x3150544B),
        "width": _set_header(p, 1, w + 16),
        "height": _set_header(p, 2, h + 16),
        "texel size": _set_header(p, 3, 12 - tb),
        "n_entries != n_solid + n_raw": _set_header(p, 4, n_entries - 1),
        "n_raw beyond the bytes": _set_header(_set_header(p, 6, n_raw + 1), 5, n_solid - 1),
        "counts near 2^32": _set_header(_set_header(p, 5, 0xFFFFFFFF - n_raw), 4, 0xFFFFFFFF),
        "more entries than tiles": _set_header(_set_header(p, 5, n_solid + 1), 4, n_entries + 1),
    }
    pitch, offset = w * tb + 32, 256
    assert engine.unpack_rejects(reset=True) >= 0
    for what, bad in cases.items():
        expect = poison_frame(h, w, tb)
        want_rejects = ref.unpack(bad, expect)
        again = poison_frame(h, w, tb)
        assert tilepack.apply(bad, again) == want_rejects and np.array_equal(again, expect), what
        pk = DevBuf(engine, data=bad + bytes([CANARY]) * 4096)
        out = DevBuf(engine, offset + pitch * h + 256)
        try:
            engine.unpack_tiles((pk.ptr, len(bad)), out.ptr + offset, pitch, w, h, tb)
            assert engine.unpack_rejects(reset=True) == want_rejects, what
            assert np.array_equal(out.bytes(), laid_out(expect, pitch, offset, tail=256)), what
        finally:
            pk.free()
            out.free()
    assert engine.unpack_rejects() == 0


def test_band_mode_does_not_affect_pack_or_unpack(engine):
    f, r = case_frames(250, 40, 4, "mixed")
    engine.set_band(1, 2)  # (bin rows of 256 pixel rows: a blit would write nothing of this frame)
    try:
        check_pack_and_unpack(engine, f, r, what="in band mode")
    finally:
        engine.set_band()


def test_profile_has_pack_and_unpack_queries(engine):
    f = make_frame(250, 40, 4, 3)
    src, dst, out = DevBuf(engine, data=f.tobytes()), DevBuf(engine, tilepack.bound(250, 40, 4)), DevBuf(engine, f.nbytes)
    engine.profile(True)
    try:
        with engine.profile_group("transport"):
            engine.pack_tiles(src.ptr, 1000, 250, 40, 4, out_device_ptr=dst.ptr)
            engine.unpack_tiles((dst.ptr, dst.n), out.ptr, 1000, 250, 40, 4)
        tree = engine.profile_collect_tree()
        engine.pack_tiles(src.ptr, 1000, 250, 40, 4, out_device_ptr=dst.ptr)
        flat = engine.profile_collect()
    finally:
        engine.profile(False)
        for b in (src, dst, out):
            b.free()
    for label in ("pack", "unpack"):
        q = [n for n in tree if n["label"] == label]
        assert len(q) == 1 and q[0]["kind"] == "query" and q[0]["stage"] == -1, label
        assert tree[q[0]["parent"]]["label"] == "transport" and q[0]["gpu_end_ms"] >= q[0]["gpu_start_ms"]
    assert flat == []
