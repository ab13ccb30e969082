"""CPU: the exact-coverage reference of tests/exact_coverage.py checked against itself and against closed forms before
it judges any image: shoelace and clipped areas, per-pixel values of half-planes and rectangles, the symmetries of the
winding integral, fine supersampling, the sample positions (confirmed on the oracle) and msaa_delta with the mask LUT
the host uploads."""
import numpy as np
import pytest

import jello_amd
from jello_amd import Aa, Brush, Fill, Host, Path, RenderParams, Scene
from oracle.oracle_engine import OracleEngine

import exact_coverage as X


def shoelace(p):
    p = np.asarray(p, np.float64)
    q = np.roll(p, -1, axis=0)
    return 0.5 * float(np.sum(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]))


def clip_to_rect(p, w, h):
    """Sutherland-Hodgman against [0, w] x [0, h] (exact area for a simple polygon and a convex window)."""
    pts = [tuple(v) for v in np.asarray(p, np.float64)]
    for axis, bound, keep_ge in ((0, 0.0, True), (0, float(w), False), (1, 0.0, True), (1, float(h), False)):
        out = []
        for i, cur in enumerate(pts):
            prv = pts[i - 1]
            cin = cur[axis] >= bound if keep_ge else cur[axis] <= bound
            pin = prv[axis] >= bound if keep_ge else prv[axis] <= bound
            if cin != pin:
                t = (bound - prv[axis]) / (cur[axis] - prv[axis])
                out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
            if cin:
                out.append(cur)
        pts = out
        if not pts:
            return np.zeros((0, 2))
    return np.array(pts)


def simple_polygon(rng, cx, cy, rmin, rmax, n):
    """Star-shaped around (cx, cy) with sorted angles: simple."""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = rng.uniform(rmin, rmax, n)
    return np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)


@pytest.mark.parametrize("seed", range(8))
def test_sum_is_the_shoelace_area(seed):
    rng = np.random.default_rng(seed)
    p = simple_polygon(rng, 40, 30, 5, 25, 12)
    acc = X.area_acc([p], 80, 64)
    want = shoelace(p)
    assert abs(acc.sum() - want) <= 1e-9 * abs(want)
    assert abs(X.area_acc([p[::-1]], 80, 64).sum() + want) <= 1e-9 * abs(want)


@pytest.mark.parametrize("seed", range(8))
def test_sum_is_the_clipped_area_past_every_side(seed):
    rng = np.random.default_rng(100 + seed)
    w, h = 48, 40
    p = simple_polygon(rng, rng.uniform(10, 38), rng.uniform(10, 30), 20, 70, 15)
    assert p[:, 0].min() < 0 and p[:, 1].min() < 0 and p[:, 0].max() > w and p[:, 1].max() > h
    want = shoelace(clip_to_rect(p, w, h))
    assert abs(X.area_acc([p], w, h).sum() - want) <= 1e-9 * abs(want)


def _box_cov(lo, hi, n):
    c = np.arange(n, dtype=np.float64)
    return np.clip(np.minimum(c + 1, hi) - np.maximum(c, lo), 0.0, 1.0)


@pytest.mark.parametrize("r", [(3.25, 2.5, 17.75, 11.125), (0.0, 0.0, 20.0, 14.0), (-5.5, 4.0, 7.0625, 30.0),
                               (16 - 2 ** -20, 1 + 2 ** -10, 19 + 2 ** -20, 9.999)])
def test_rectangles_give_the_closed_form(r):
    x0, y0, x1, y1 = r
    w, h = 20, 14
    acc = X.area_acc([[(x0, y0), (x1, y0), (x1, y1), (x0, y1)]], w, h)
    want = _box_cov(y0, y1, h)[:, None] * _box_cov(x0, x1, w)[None, :]
    assert np.abs(acc - want).max() <= 1e-12


@pytest.mark.parametrize("a", [0.0, 2.5, 7.3125, 11 - 2 ** -20])
def test_half_planes_give_the_closed_form(a):
    w, h = 12, 9
    big = 1000.0
    right = [(a, -big), (big, -big), (big, big), (a, big)]        # x >= a
    below = [(-big, a), (big, a), (big, big), (-big, big)]        # y >= a
    assert np.abs(X.area_acc([right], w, h) - _box_cov(a, big, w)[None, :]).max() <= 1e-12
    assert np.abs(X.area_acc([below], w, h) - _box_cov(a, big, h)[:, None]).max() <= 1e-12


def test_translation_reversal_and_copies():
    rng = np.random.default_rng(5)
    p = rng.uniform(2, 30, (9, 2))           # self-intersecting
    w, h = 40, 36
    acc = X.area_acc([p], w, h)
    shifted = X.area_acc([p + (3.0, 2.0)], w, h)
    assert np.abs(shifted[2:, 3:] - acc[:-2, :-3]).max() <= 1e-12
    assert np.abs(X.area_acc([p[::-1]], w, h) + acc).max() <= 1e-12
    assert np.abs(X.area_acc([p, p], w, h) - 2 * acc).max() <= 1e-12
    assert np.abs(X.area_acc([p, p[::-1]], w, h)).max() <= 1e-12
    for S in (8, 16):
        wind = X.sample_winding([p], w, h, S)
        assert np.array_equal(X.sample_winding([p[::-1]], w, h, S), -wind)
        assert np.array_equal(X.sample_winding([p, p], w, h, S), 2 * wind)
        assert not X.sample_winding([p, p[::-1]], w, h, S).any()


def _supersampled(p, w, h, n):
    """Mean winding number over n x n midpoints per pixel (ray towards -x, upward edges +1), one row at a time."""
    out = np.zeros((h, w))
    xs = (np.arange(w * n) + 0.5) / n
    e = X.edges_of([p])
    for r in range(h * n):
        y = (r + 0.5) / n
        wind = np.zeros(w * n)
        for x0, y0, x1, y1 in e:
            if min(y0, y1) <= y < max(y0, y1):
                xc = x0 + (y - y0) * (x1 - x0) / (y1 - y0)
                wind += np.where(xs > xc, 1.0 if y1 < y0 else -1.0, 0.0)
        out[r // n] += wind.reshape(w, n).sum(axis=1)
    return out / (n * n)


@pytest.mark.parametrize("seed", range(3))
def test_agrees_with_256x256_supersampling(seed):
    rng = np.random.default_rng(40 + seed)
    w, h = 10, 8
    p = rng.uniform(-1, [w + 1, h + 1], (6, 2))
    err = np.abs(X.area_acc([p], w, h) - _supersampled(p, w, h, 256))
    assert err.max() <= 1 / 256 + 1e-9


def _uploaded_luts():
    s = Scene()
    s.fill(Fill.NonZero, None, Brush.solid((1, 1, 1, 1)), None, Path.rect(1, 1, 5, 5))
    out = {}
    for aa, S in ((Aa.Msaa8, 8), (Aa.Msaa16, 16)):
        rec = Host().record(s, RenderParams(16, 16, aa=aa))
        for c in rec.commands():
            if c["kind"] == jello_amd.CMD.UPLOAD and c["buf_name"].lower().startswith("mask"):
                b = np.frombuffer(c["data"], np.uint8)
                w, hh = X.LUT_SHAPE[S]
                out[S] = b[:w * hh] if S == 8 else b[:2 * w * hh].view(np.uint16)
    return out


def test_lut_is_the_half_plane_definition(built):
    """The uploaded LUT equals the geometric reading of it used here: bit i set iff sample i is on the +x side."""
    luts = _uploaded_luts()
    for S in (8, 16):
        assert np.array_equal(X.lut_bits(luts[S], S), X.lut_from_definition(S)[0].T)


def test_msaa_delta_is_reproduced(built):
    luts = _uploaded_luts()
    assert round(X.msaa_delta(8, luts[8]), 4) == 0.0558
    assert round(X.msaa_delta(16, luts[16]), 4) == 0.0286


@pytest.mark.parametrize("S", [8, 16])
def test_lut_outside_the_delta_band_is_exact(built, S):
    """Random lines, looked up the way fine.wgsl:299-303 forms the index: every sample farther than delta - 1e-3
    from the line is classified as its true side."""
    lut = X.lut_bits(_uploaded_luts()[S], S)
    W, H = X.LUT_SHAPE[S]
    half = H // 2
    rng = np.random.default_rng(S)
    n = 200_000
    a, t, pos = rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.integers(0, 2, n).astype(bool)
    ix = pos * (W * half) + np.floor(np.minimum(a * half, half - 1.0)).astype(int) * W + np.floor(t * W).astype(int)
    bits, d = X._classify(X.sample_points(S), a, t, pos)
    far = np.abs(d) > X.msaa_delta(S) - X.TILE_CLAMP
    assert np.array_equal(lut[ix].T[far], bits[far])
    assert (~far).mean() < 0.2


@pytest.mark.parametrize("S,aa", [(8, Aa.Msaa8), (16, Aa.Msaa16)])
def test_sample_positions_on_the_oracle(built, S, aa):
    """Axis-aligned half-planes at the sub-pixel offsets j / S, half-way between two sample rows / columns and so
    farther than msaa_delta from every sample: the oracle counts exactly the samples of sample_points() on the covered
    side, so their x and y coordinates are each a permutation of (i + 0.5) / S."""
    sp = X.sample_points(S)
    assert 0.5 / S > X.msaa_delta(S)
    for j in range(S + 1):
        f = j / S
        for vertical in (True, False):
            s = Scene()
            r = (4 + f, -8, 40, 40) if vertical else (-8, 4 + f, 40, 40)
            s.fill(Fill.NonZero, None, Brush.solid((1, 1, 1, 1)), None, Path.rect(*r))
            rec = Host().record(s, RenderParams(16, 16, aa=aa))
            o = OracleEngine()
            o.run(rec)
            alpha = o.target(rec).view(np.float16).astype(np.float64)[..., 3]
            px = alpha[8, 4] if vertical else alpha[4, 8]
            want = np.mean(sp[:, 0 if vertical else 1] > f)
            assert px == want, (vertical, f, px, want)
