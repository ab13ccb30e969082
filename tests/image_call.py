"""What the -m gpu tests of the image calls (jh_blur ... jh_turbulence) share, beside devmem.py: the comparison of f16 bits and
its failure text, images that are freed whatever happens, the rendered scene, and the frames of the five tests every call has --
the battery, the captured frame, the refusals, the profile query -- with the call itself passed in.  DESIGN.md 5.16."""
import contextlib
import ctypes

import numpy as np
import pytest

import jello_amd
from jello_amd import Brush, Cap, Fill, ImageFormat, Join, Path, RenderParams, Scene, Stroke, Surface
from jello_amd.engine import JH_ERR_INVALID, RUN_DISPATCHES, RUN_UPLOADS

import blur_ref
import surface_ref
from devmem import CANARY, DevBuf, Image, _id, target_of

JH_ERR_OOM = -5
CANARY16 = CANARY | (CANARY << 8)


def differences(name, got, want, exact=False):
    """The failure text of a comparison of f16 bits; two NaNs count as equal unless `exact` ("equal": only NaN payloads differ)."""
    bad = got != want
    if not exact:
        bad &= ~(((got & 0x7FFF) > 0x7C00) & ((want & 0x7FFF) > 0x7C00))
    bad = np.argwhere(bad)
    if len(bad) == 0:
        return "%s: equal" % (name,)
    i = tuple(int(v) for v in bad[0])
    return "%s: %d of %d values differ, first at (y, x, ch) = %s: got %#06x, want %#06x" % (name, len(bad), got.size, i, got[i], want[i])


def assert_same_bits(got, want, name):
    """Equal f16 bit patterns, a NaN equal to any NaN (blur_ref.same_bits, which every *_ref.py shares)."""
    assert blur_ref.same_bits(got, want), differences(name, got, want)


def assert_equal_bits(got, want, name):
    """Equal bits, NaN payloads included: for the calls whose rule fixes them."""
    assert np.array_equal(got, want), differences(name, got, want, exact=True)


@contextlib.contextmanager
def images(engine, *specs):
    """One object of the context per spec, every one freed on exit, also when the body raises: (H, W, 4) uint16 bits -> an uploaded
    Image; (width, height) -> an Image that is only created (never written); (width, height, ImageFormat.RGBA8) -> an uploaded
    RGBA8 image of that many texels (of 4 bytes: the image a call must refuse for its format); a number of bytes -> a DevBuf of
    CANARY."""
    made = []
    try:
        for s in specs:
            if isinstance(s, np.ndarray):
                made.append(Image(engine, s))
            elif isinstance(s, tuple) and s[2:] == (ImageFormat.RGBA8,):
                made.append(Image(engine, np.full((s[1], s[0], 2), 0x1111, np.uint16), fmt=ImageFormat.RGBA8))
            elif isinstance(s, tuple):
                made.append(Image(engine, None, *s))
            else:
                made.append(DevBuf(engine, s))
        yield made
    finally:
        for m in made:
            m.free()


_SCENES = {  # size: the disc, the cubic -- two drawings, not one scaled: the rendered bits feed exact comparisons
    (128, 128): ((50, 44, 30), ((10, 100), (40, 4, 90, 120, 120, 16))),
    (64, 48): ((24, 20, 13), ((6, 40), (20, 2, 44, 46, 58, 8))),
}


def scene(size=(128, 128), stroke=5, color=(0.9, 0.4, 0.1, 1.0)):
    """(scene, params): a filled disc and, over it, a translucent stroked cubic of width `stroke` (None: the disc alone)."""
    disc, (start, curve) = _SCENES[size]
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid(color), None, Path.circle(*disc))
    if stroke is not None:
        s.stroke(Stroke(stroke, Join.Round, 4, Cap.Round, Cap.Round), None, Brush.solid((0.1, 0.3, 0.9, 0.8)), None,
                 Path().move_to(*start).cubic_to(*curve))
    return s, RenderParams(*size)


def run_case(engine, case, call, source_bits, prior, in_place=False, dst_size=None):
    """The body of a battery test: the source uploaded (`source_bits` None: the call has none; a case of kind "never": only
    created), dst holding `prior` (None: only created, of `dst_size`; `in_place`: dst is the source), call(src, dst), and what dst
    holds afterwards -- having asserted that a written source of its own still holds its bits."""
    never = case.get("kind") == "never"  # (a never-written image reads as zero; its memory holds anything)
    specs = [] if source_bits is None else [source_bits.shape[1::-1] if never else source_bits]
    if not in_place:
        specs.append(dst_size if prior is None else prior)
    with images(engine, *specs) as made:
        src, dst = (None if source_bits is None else made[0]), made[-1]
        call(src, dst)
        got = dst.bits()
        if src is not None and src is not dst and not never:
            assert np.array_equal(src.bits(), source_bits)  # the source is only read
    return got


def captured_call(engine, enqueue, clear_first=None):
    """enqueue() -- a call of the C ABI, returning its code -- inside a capture of the context (after the clear of a buffer, if one is
    given): (rc, message, graph).  The graph is the caller's to destroy."""
    hip, ctx = engine.hip, engine.ctx
    engine._check(hip.jh_graph_begin(ctx), "graph_begin")
    try:
        if clear_first is not None:
            engine.clear(clear_first)
        rc = enqueue()
        msg = hip.jh_last_error(ctx).decode()
    finally:
        g = ctypes.c_void_p()
        engine._check(hip.jh_graph_end(ctx, ctypes.byref(g)), "graph_end")
    return rc, msg, g


def captured_with_the_frame(engine, scene, eager, capture_keywords, want, extra_launches, out_size=None, baseline_surface=False,
                            same=assert_same_bits):
    """capture(<the call>=..., surface=...): record and run the scene, make the call eagerly -- eager(target id, out id) -- and blit
    what it wrote: the reference want(the plain target) and its RGBA8_SRGB conversion.  Then the capture with
    capture_keywords(out id) has `extra_launches` kernel nodes more than the baseline capture and no other node more, and replayed
    twice onto a cleared surface it gives the eager bytes.  `out_size`: the call writes a second image of that size, which the blit
    reads, and leaves the target as rendered; None: it works on the target in place, which then holds the reference after every
    replay.  `baseline_surface`: the baseline is the frame with the blit of its own target, not the frame alone."""
    s, p = scene
    w, h = p.width, p.height
    ow, oh = out_size or (w, h)
    fmt = Surface.RGBA8_SRGB
    rec = jello_amd.Host().record(s, p)
    g = None
    with images(engine, ow * oh * 4, *([out_size] if out_size else []), *([w * h * 4] if baseline_surface else [])) as made:
        surf, out, full = made[0], (made[1] if out_size else None), (made[-1] if baseline_surface else None)
        out_id = out.id if out else None
        surface = lambda: surf.bytes()[:ow * oh * 4].reshape(oh, ow, 4)  # noqa: E731
        try:
            engine.run(rec, RUN_UPLOADS | RUN_DISPATCHES)
            t = rec.target
            plain = target_of(engine, rec)
            eager(t["id"], out_id)
            engine.blit(out_id if out else t["id"], ow, oh, fmt, out_device_ptr=surf.ptr)
            eager_bytes = surface()
            wanted = want(plain)
            same(out.bits() if out else target_of(engine, rec), wanted, "the eager call")
            assert np.array_equal(eager_bytes, surface_ref.convert(wanted, int(fmt)))
            if not out:
                assert (wanted != plain).any()
            g0 = engine.capture(rec, surface=(full.ptr, w * 4, fmt)) if baseline_surface else engine.capture(rec)
            g = engine.capture(rec, surface=(surf.ptr, ow * 4, fmt), **capture_keywords(out_id))
            (k0, o0), (k1, o1) = engine.graph_node_counts(g0), engine.graph_node_counts(g)
            engine.graph_destroy(g0)
            assert (k1, o1) == (k0 + extra_launches, o0)
            for _ in range(2):
                engine.clear(surf.id)
                engine.replay(g)
                engine.sync()
                assert np.array_equal(surface(), eager_bytes)
                if not out:
                    same(target_of(engine, rec), wanted, "the replayed target")
            if out:
                assert np.array_equal(target_of(engine, rec), plain)
        finally:
            if g is not None:
                engine.graph_destroy(g)


def common_refusals(call, rgba8, rects=(("", "", "rect"),), source=True):
    """The rows of check_refusals' `refused` that every image call has, made with the file's adapter call(s=, d=, <rect keyword>=,
    null=) (a call without a source: no s=): the descriptor, the ids, the formats, and per rectangle of the call -- `rects`:
    (the description's prefix, the role in the message: "", "source " or "destination ", the adapter's keyword) -- the six ways
    not to lie inside the image (an end that wraps in 32 bits on either axis among them).  The words are those of the one place in jello_hip.cpp that refuses them."""
    rows = {"null descriptor": (lambda: call(null=True), b"null descriptor")}
    for role, key in (("source", "s"), ("destination", "d")) if source else (("destination", "d"),):
        rows["unknown " + role] = (lambda key=key: call(**{key: _id()}), b"unknown " + role.encode() + b" image id")
        rows[role + " not RGBA16F"] = (lambda key=key: call(**{key: rgba8.id}), b"the " + role.encode() + b" is not an RGBA16F image")
    for prefix, role, key in rects:
        is_ = b"the " + role.encode() + b"rectangle is "
        for what, rect, word in (("beyond the right edge", (8, 0, 9, 4), b"not inside the " + role.encode() + b"image"),
                                 ("beyond the bottom edge", (0, 9, 4, 4), b"not inside the " + role.encode() + b"image"),
                                 ("whose end wraps", (0xFFFFFFFF, 0, 2, 2), b"not inside the " + role.encode() + b"image"),
                                 ("whose bottom end wraps", (0, 0xFFFFFFFF, 2, 2), b"not inside the " + role.encode() + b"image"),
                                 ("empty in x only", (2, 2, 0, 4), b"empty in one dimension"),
                                 ("empty in y only", (2, 2, 4, 0), b"empty in one dimension")):
            rows["%srectangle %s" % (prefix, what)] = (lambda key=key, rect=rect: call(**{key: rect}), (is_, word))
    return rows


def check_refusals(engine, who, call, refused, untouched, raises=(), accepted=()):
    """The frame of a refusal test.  Every row of `refused` -- description: (callable, word or words) -- returns JH_ERR_INVALID with
    a message that starts "<who>: " and holds the words; so does the plain call() in band mode (b"band"); every callable of
    `raises` -- a call through Engine -- raises ValueError with that prefix.  After all that every (image, bits) of `untouched` holds
    its bits and a canary buffer allocated behind the caller's images its canary; then every callable of `accepted` returns 0, and
    the canary buffer still holds."""
    hip, ctx = engine.hip, engine.ctx
    prefix = who.encode() + b": "
    with images(engine, 256) as (guard,):
        for what, (f, words) in refused.items():
            assert f() == JH_ERR_INVALID, what
            msg = hip.jh_last_error(ctx)
            assert msg.startswith(prefix) and all(w in msg for w in ((words,) if isinstance(words, bytes) else words)), (what, msg)
        engine.set_band(0, 1)
        try:
            assert call() == JH_ERR_INVALID
            assert hip.jh_last_error(ctx).startswith(prefix) and b"band" in hip.jh_last_error(ctx)
        finally:
            engine.set_band()
        for f in raises:
            with pytest.raises(ValueError, match=who + ": "):
                f()
        for im, bits in untouched:
            assert np.array_equal(im.bits(), bits)  # no refusal touched a texel
        assert np.all(guard.bytes() == CANARY)
        for n, f in enumerate(accepted):
            assert f() == 0, (n, hip.jh_last_error(ctx))
        assert np.all(guard.bytes() == CANARY)


def canary_bits(w=16, h=12):
    """The bits of the w x h images a refusal test calls with: no refusal may change one of them."""
    return np.full((h, w, 4), CANARY16, np.uint16)


def one_query(engine, label, call):
    """With the profile on, call() inside the group "post" is one query of the tree, named `label`, under that group, with an
    interval; outside a group it leaves no flat record."""
    engine.profile(True)
    try:
        with engine.profile_group("post"):
            call()
        tree = engine.profile_collect_tree()
        call()
        flat = engine.profile_collect()
    finally:
        engine.profile(False)
    assert [(n["kind"], n["label"], n["parent"], n["stage"]) for n in tree] == [("group", "post", -1, -1), ("query", label, 0, -1)]
    assert tree[1]["gpu_end_ms"] >= tree[1]["gpu_start_ms"]
    assert flat == []
