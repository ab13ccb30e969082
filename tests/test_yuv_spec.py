"""CPU: the YUV blit's conversion rule (include/jello_hip.h "YUV blit") -- the committed coefficient header
against its generator, both against tests/yuv_ref.py (which derives the tables on its own from exact fractions) and against
the sixteen rows the rule prints; hand values, greys, ranges and the distance to the exact formula over all 2^24 code triples,
plane shapes and edge replication, the Python enums against the header, the Go shim's C calls against the declarations."""
import importlib.util
import os

import numpy as np
import pytest

import yuv_ref as ref
from abi_text import c_values, go_calls, header_arity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "jello_amd", "csrc", "yuv_matrix_lut.h")
GEN = os.path.join(ROOT, "tools", "gen_yuv_table.py")

# the rows of the rule: (matrix, range) -> Y row, Cb row, Cr row
ROWS = {
    (ref.BT601, ref.LIMITED): ([16829, 33039, 6416], [-9714, -19070, 28784], [28784, -24103, -4681]),
    (ref.BT601, ref.FULL): ([19595, 38470, 7471], [-11058, -21710, 32768], [32768, -27439, -5329]),
    (ref.BT709, ref.LIMITED): ([11966, 40254, 4064], [-6596, -22188, 28784], [28784, -26145, -2639]),
    (ref.BT709, ref.FULL): ([13933, 46871, 4732], [-7509, -25259, 32768], [32768, -29763, -3005]),
}
TABLES = list(ROWS)


def _gen():
    spec = importlib.util.spec_from_file_location("gen_yuv_table", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_committed_header_is_the_generators_output():
    g = _gen()
    with open(HEADER) as f:
        text = f.read()
    assert text == g.render(g.tables())
    rows, offs = g.parse(text)
    assert offs == [16, 0] and len(rows) == 4


def test_header_generator_and_reference_equal_the_printed_rows():
    g = _gen()
    with open(HEADER) as f:
        rows, offs = g.parse(f.read())
    gen = {(m, r): t for (m, r), t in zip([(m, r) for m in ref.MATRICES for r in ref.RANGES], g.tables())}
    for i, key in enumerate((m, r) for m in ref.MATRICES for r in ref.RANGES):  # the header's order: matrix major, range minor
        want = [c for row in ROWS[key] for c in row]
        assert rows[i] == want, key
        assert [c for row in gen[key][3] for c in row] == want, key
        assert gen[key][2] == offs[key[1]] == (16 if key[1] == ref.LIMITED else 0)
        m, off = ref.table(*key)
        assert [c for row in m for c in row] == want and off == offs[key[1]], key


@pytest.mark.parametrize("key", TABLES)
def test_row_sums(key):
    y, cb, cr = ROWS[key]
    assert sum(y) == (56284 if key[1] == ref.LIMITED else 65536)  # rne(219/255 * 2^16) = rne(56283.86)
    assert sum(cb) == 0 and sum(cr) == 0
    # every coefficient is within one unit of round-half-even(exact * 2^16): only the green one may have been adjusted
    exact, _ = ref.exact_matrix(*key)
    for k, row in enumerate((y, cb, cr)):
        adj = [c - ref._rne(e * 65536) for c, e in zip(row, exact[k])]
        assert adj[0] == 0 and adj[2] == 0 and abs(adj[1]) <= 1, (key, k, adj)


def _one(rgb, matrix, rng):
    y, cb, cr = ref.from_codes(np.array([[rgb]], np.uint8), matrix, rng)
    return int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])


WHITE, BLACK, RED, GREEN, BLUE, YELLOW = (255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)
HAND = [
    (ref.BT709, ref.LIMITED, WHITE, (235, 128, 128)), (ref.BT709, ref.LIMITED, BLACK, (16, 128, 128)),
    (ref.BT709, ref.LIMITED, RED, (63, 102, 240)), (ref.BT709, ref.LIMITED, GREEN, (173, 42, 26)),
    (ref.BT709, ref.LIMITED, BLUE, (32, 240, 118)), (ref.BT709, ref.LIMITED, (200, 100, 50), (117, 96, 174)),
    (ref.BT601, ref.LIMITED, RED, (81, 90, 240)), (ref.BT601, ref.LIMITED, GREEN, (145, 54, 34)),
    (ref.BT601, ref.LIMITED, BLUE, (41, 240, 110)),
    (ref.BT709, ref.FULL, RED, (54, 99, 255)), (ref.BT709, ref.FULL, BLUE, (18, 255, 116)), (ref.BT709, ref.FULL, YELLOW, (237, 1, 140)),
    (ref.BT601, ref.FULL, RED, (76, 85, 255)), (ref.BT601, ref.FULL, BLUE, (29, 255, 107)),
]


@pytest.mark.parametrize("matrix,rng,rgb,want", HAND)
def test_hand_values(matrix, rng, rgb, want):
    assert _one(rgb, matrix, rng) == want  # one pixel: the edge rule makes it its own 2 x 2 block
    for h, w in ((2, 2), (4, 6), (3, 5)):  # a uniform block
        y, cb, cr = ref.from_codes(np.tile(np.array(rgb, np.uint8), (h, w, 1)), matrix, rng)
        assert np.all(y == want[0]) and np.all(cb == want[1]) and np.all(cr == want[2])


def test_hand_value_red_over_blue():
    img = np.array([[RED, RED], [BLUE, BLUE]], np.uint8)
    assert ref.chroma_sums(img).tolist() == [[[510, 0, 510]]]
    y, cb, cr = ref.from_codes(img, ref.BT709, ref.LIMITED)
    assert y.tolist() == [[63, 63], [32, 32]] and cb.tolist() == [[171]] and cr.tolist() == [[179]]


def test_hand_value_through_the_transfer():
    """(c, a) = (1, 0.5) on all channels: code 128 (NONE) or 188 (SRGB), a grey either way."""
    px = np.array([[[1.0, 1.0, 1.0, 0.5]]], np.float16).view(np.uint16)
    for transfer, code in ((ref.NONE, 128), (ref.SRGB, 188)):
        assert ref.codes_of(px, transfer).tolist() == [[[code] * 3]]
        for matrix, rng in TABLES:
            y, cbcr = ref.convert(px, ref.NV12, matrix, rng, transfer)
            assert cbcr.tolist() == [[[128, 128]]]
            assert y[0, 0] == ref.luma(np.array([code] * 3), matrix, rng)
    y, cb, cr = ref.convert(px, ref.I420, ref.BT709, ref.LIMITED, ref.NONE)
    assert (y[0, 0], cb[0, 0], cr[0, 0]) == (16 + ((56284 * 128 + 32768) >> 16), 128, 128) == (126, 128, 128)


@pytest.mark.parametrize("key", TABLES)
def test_every_grey_has_neutral_chroma(key):
    g = np.arange(256, dtype=np.uint8)
    px = np.stack([g, g, g], axis=-1)  # 256 greys
    for h, w in ((1, 1), (2, 2), (3, 3), (1, 2), (2, 1), (5, 7)):
        for code in px:
            y, cb, cr = ref.from_codes(np.tile(code, (h, w, 1)), *key)
            assert np.all(cb == 128) and np.all(cr == 128)
            assert cb.shape == cr.shape == ((h + 1) // 2, (w + 1) // 2)
    # mixed greys, odd edges: still neutral (each chroma row sums to 0, so M . S = 0 whenever S_R = S_G = S_B)
    rng = np.random.default_rng(5)
    v = rng.integers(0, 256, size=(7, 9), dtype=np.uint8)
    _, cb, cr = ref.from_codes(np.stack([v, v, v], axis=-1), *key)
    assert np.all(cb == 128) and np.all(cr == 128)


@pytest.mark.parametrize("key", TABLES)
def test_all_code_triples_range_and_distance_to_the_exact_formula(key):
    """All 2^24 (R, G, B): limited-range outputs stay in [16, 235] / [16, 240] before the clamp; |fixed - exact| < 0.51 for
    luma and for the chroma of uniform blocks (S = 4 x the code).  The exact value is evaluated in binary64 from the exact
    fractions: its own error is below 1e-10, far inside the gap between the largest distance (about 0.5015) and 0.51."""
    exact, off = ref.exact_matrix(*key)
    e = [[float(c) for c in row] for row in exact]
    worst = [0.0, 0.0]
    for b0 in range(0, 256, 32):
        i = np.arange(b0 << 16, (b0 + 32) << 16, dtype=np.int64)
        c = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1)
        f = c.astype(np.float64)
        y = ref.luma(c, *key, clamp=False)
        cb, cr = ref.chroma_of_sums(4 * c, *key, clamp=False)
        if key[1] == ref.LIMITED:
            assert y.min() >= 16 and y.max() <= 235
            assert min(cb.min(), cr.min()) >= 16 and max(cb.max(), cr.max()) <= 240
        else:
            assert y.min() >= 0 and y.max() <= 255 and min(cb.min(), cr.min()) >= 0 and max(cb.max(), cr.max()) <= 256
        worst[0] = max(worst[0], np.abs(y - (off + f @ np.array(e[0]))).max())
        for v, row in ((cb, e[1]), (cr, e[2])):
            worst[1] = max(worst[1], np.abs(v - (128 + f @ np.array(row))).max())
    print("table %r: largest |fixed - exact| luma %.5f chroma %.5f" % (key, worst[0], worst[1]))
    assert worst[0] < 0.51 and worst[1] < 0.51


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 2), (3, 7), (1001, 517)])
def test_plane_shapes_and_edge_replication(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    codes = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    # the image padded explicitly to even sizes by repeating the last column / row
    padded = np.pad(codes, ((0, h & 1), (0, w & 1), (0, 0)), mode="edge")
    for key in TABLES:
        y, cb, cr = ref.from_codes(codes, *key)
        assert y.shape == (h, w) and cb.shape == cr.shape == ((h + 1) // 2, (w + 1) // 2)
        assert y.dtype == cb.dtype == cr.dtype == np.uint8
        yp, cbp, crp = ref.from_codes(padded, *key)
        assert np.array_equal(yp[:h, :w], y) and np.array_equal(cbp, cb) and np.array_equal(crp, cr)
        # and the padded image's chroma is the plain 2 x 2 box sum
        p = padded.astype(np.int64)
        box = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        assert np.array_equal(ref.chroma_sums(codes), box)
    img = np.zeros((h, w, 4), np.uint16)
    y, cbcr = ref.convert(img, ref.NV12, ref.BT709, ref.LIMITED, ref.NONE)
    assert y.shape == (h, w) and cbcr.shape == ((h + 1) // 2, (w + 1) // 2, 2)
    assert np.all(y == 16) and np.all(cbcr == 128)


def test_yuv_enums_match_header():
    from jello_amd import YuvLayout, YuvMatrix, YuvRange, YuvTransfer
    names = ["JH_YUV_NV12", "JH_YUV_I420", "JH_YUV_BT601", "JH_YUV_BT709", "JH_YUV_LIMITED", "JH_YUV_FULL", "JH_YUV_TRANSFER_NONE",
             "JH_YUV_TRANSFER_SRGB"]
    vals = c_values(names)
    assert vals == [YuvLayout.NV12, YuvLayout.I420, YuvMatrix.BT601, YuvMatrix.BT709, YuvRange.LIMITED, YuvRange.FULL,
                        YuvTransfer.NONE, YuvTransfer.SRGB] == [0, 1, 0, 1, 0, 1, 0, 1]
    assert [e.name for e in YuvLayout] == ["NV12", "I420"] and [e.name for e in YuvMatrix] == ["BT601", "BT709"]
    assert [e.name for e in YuvRange] == ["LIMITED", "FULL"] and [e.name for e in YuvTransfer] == ["NONE", "SRGB"]
    assert (ref.NV12, ref.I420, ref.BT601, ref.BT709, ref.LIMITED, ref.FULL, ref.NONE, ref.SRGB) == (0, 1, 0, 1, 0, 1, 0, 1)

def test_go_shim_calls_blit_yuv_as_declared():
    decl = header_arity()
    assert decl.get("jh_blit_yuv") == 5
    calls = go_calls()
    assert len(calls) > 20
    for name, n in calls:
        assert name in decl, "hip_engine.go calls %s, which include/jello_hip.h does not declare" % name
        assert decl[name] == n, "hip_engine.go calls %s with %d arguments, the header declares %d" % (name, n, decl[name])
    assert "jh_blit_yuv" in {n for n, _ in calls}


def _oracle_target(scene, params):
    import jello_amd
    from oracle.oracle_engine import OracleEngine
    rec = jello_amd.Host().record(scene, params)
    orc = OracleEngine()
    orc.run(rec)
    return np.asarray(orc.target(rec)).copy()


def test_oracle_frames_are_plausible(built):
    """yuv_ref on the oracle's frames (scene_c1, a small scene_c4): plane sizes, and mean luma = the luma of the mean code
    within 1 (luma is affine in the codes up to half a code of rounding per pixel)."""
    from jello_amd import scenes
    for s, p in (scenes.scene_c1(), scenes.scene_c4(300, 256)):
        img = _oracle_target(s, p)
        h, w = img.shape[:2]
        for transfer in ref.TRANSFERS:
            codes = ref.codes_of(img, transfer)
            mean = codes.reshape(-1, 3).astype(np.float64).mean(axis=0)
            for matrix, rng in TABLES:
                y, cbcr = ref.convert(img, ref.NV12, matrix, rng, transfer)
                y2, cb, cr = ref.convert(img, ref.I420, matrix, rng, transfer)
                assert y.shape == (h, w) and cbcr.shape == ((h + 1) // 2, (w + 1) // 2, 2)
                assert np.array_equal(y, y2) and np.array_equal(cbcr[..., 0], cb) and np.array_equal(cbcr[..., 1], cr)
                m, off = ref.table(matrix, rng)
                want = off + (m[0][0] * mean[0] + m[0][1] * mean[1] + m[0][2] * mean[2]) / 65536.0
                assert abs(y.astype(np.float64).mean() - want) < 1.0
                assert y.std() > 0  # (the scenes are not blank)
