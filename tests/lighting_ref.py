"""The lighting rule (include/jello_hip.h "Lighting") in numpy, written from the rule alone: what jh_lighting has to
produce, bit for bit.  Every binary32 operation is one numpy float32 operation (correctly rounded), fmaf is image_ref.fmaf32 (exact),
min and max are composite_ref's minNum and maxNum; indices are int64; binary64 appears in plan() and table() only.

  check(**kw)      ValueError for a descriptor the rule refuses
  plan(**kw)       jh_lighting_plan: dict(s (2, 3), ldir, p, sdir, cone), float32
  table(e)         the 4097 float32 entries of exponent e;  which(**kw) the tables a descriptor needs
  lighting(...)    the image jh_lighting leaves in dst
  exact(...)       the specification evaluated in binary64 (no table, no rounding): what the rule approximates

The keywords are those of Engine.lighting.  lighting() takes switches that build near misses of the rule (tests/test_lighting_spec.py
asserts that the battery of tests/lighting_cases.py tells each of them from the rule): interior_factor=True (the interior's 1/4 at
edges and corners), half=False (texel centres without the + 0.5), normal_first=True (N divided by its length before the dot
product), reciprocal=True (l = v * (1 / len)), h_first=True (H = h / hlen, then the dot product over nlen), entries=1024 (a smaller
table), index_rounded=True (the table index rounded to nearest), alpha_one=True (SPECULAR stored opaque), clamp_first=True (min(k, 1)
before the multiply by the colour)."""
import math

import numpy as np

from image_ref import fmaf32, fmax, fmin, resolve, same_bits  # noqa: F401 (same_bits is part of this module's interface)

DIFFUSE, SPECULAR = 0, 1
DISTANT, POINT, SPOT = 0, 1, 2
KIND_NAMES = {DIFFUSE: "diffuse", SPECULAR: "specular"}
LIGHT_NAMES = {DISTANT: "distant", POINT: "point", SPOT: "spot"}
ENTRIES, STEPS = 4097, 4096
TABLE_SPEC, TABLE_SPOT = 1, 2
MAX_EXTENT = 1 << 23
F = np.float32

DEFAULTS = dict(kind=DIFFUSE, light=DISTANT, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0),
                direction=(0.0, 0.0, 1.0), position=(0.0, 0.0, 0.0), points_at=(0.0, 0.0, 0.0), spot_exponent=1.0, cone_cos=-1.0)


def _desc(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown keywords %s" % sorted(unknown))
    d = dict(DEFAULTS, **kw)
    d["kind"], d["light"] = int(d["kind"]), int(d["light"])
    for k in ("surface_scale", "constant", "specular_exponent", "spot_exponent"):
        d[k] = F(d[k])
    d["color"] = np.asarray(d["color"], F)
    for k in ("direction", "position", "points_at"):
        d[k] = tuple(float(v) for v in d[k])
    d["cone_cos"] = float(d["cone_cos"])
    return d


def _length(v):
    x, y, z = v
    s = x * x + y * y + z * z
    return math.sqrt(s) if math.isfinite(s) else math.inf


def _finite32(v):
    with np.errstate(all="ignore"):
        return math.isfinite(v) and bool(np.isfinite(F(v)))


def check(**kw):
    """The descriptor with its defaults and its values in the rule's formats; ValueError for what the rule refuses."""
    d = _desc(kw)
    if d["kind"] not in (DIFFUSE, SPECULAR) or d["light"] not in (DISTANT, POINT, SPOT):
        raise ValueError("unknown kind or light")
    if not np.isfinite(d["surface_scale"]):
        raise ValueError("surface_scale")
    if not (np.isfinite(d["constant"]) and d["constant"] >= 0):
        raise ValueError("constant")
    if d["kind"] == SPECULAR and not (1 <= d["specular_exponent"] <= 128):
        raise ValueError("specular_exponent")
    if not (np.all(np.isfinite(d["color"])) and np.all(d["color"] >= 0)):
        raise ValueError("color")
    if d["light"] == DISTANT:
        n = _length(d["direction"]) if all(math.isfinite(v) for v in d["direction"]) else math.inf
        if not (math.isfinite(n) and n > 0):
            raise ValueError("direction")
        return d
    if not all(_finite32(v) for v in d["position"]):
        raise ValueError("position")
    if d["light"] == SPOT:
        if not all(math.isfinite(v) for v in d["points_at"]):
            raise ValueError("points_at")
        n = _length(tuple(a - b for a, b in zip(d["points_at"], d["position"])))
        if not (math.isfinite(n) and n > 0):
            raise ValueError("points_at is the position")
        if not (1 <= d["spot_exponent"] <= 128):
            raise ValueError("spot_exponent")
        if not (-1.0 <= d["cone_cos"] <= 1.0):
            raise ValueError("cone_cos")
    return d


def _unit(v):
    n = _length(v)
    return np.array([F(c / n) for c in v], F)


def plan(**kw):
    d = check(**kw)
    ss = float(d["surface_scale"])
    p = dict(s=np.array([[F(-ss * 2.0 / float(span * wsum)) for wsum in (2, 3, 4)] for span in (1, 2)], F), ldir=np.zeros(3, F), p=np.zeros(3, F),
             sdir=np.zeros(3, F), cone=F(0.0))
    if d["light"] == DISTANT:
        p["ldir"] = _unit(d["direction"])
        return p
    p["p"] = np.array([F(v) for v in d["position"]], F)
    if d["light"] == SPOT:
        p["sdir"] = _unit(tuple(a - b for a, b in zip(d["points_at"], d["position"])))
        p["cone"] = F(d["cone_cos"])
    return p


_TABLES = {}


def table(e, steps=STEPS):
    """T[i] = (float)pow(i / steps, e) in binary64 (libm's pow through math.pow), i = 0 .. steps."""
    key = (F(e).tobytes(), steps)
    if key not in _TABLES:
        ee = float(F(e))
        _TABLES[key] = np.array([math.pow(i / float(steps), ee) for i in range(steps + 1)], np.float64).astype(F)
    return _TABLES[key]


def which(**kw):
    d = check(**kw)
    return (TABLE_SPEC if d["kind"] == SPECULAR and d["specular_exponent"] != 1 else 0) | (TABLE_SPOT if d["light"] == SPOT and d["spot_exponent"] != 1 else 0)


def power(t, e, entries=ENTRIES, index_rounded=False):
    """Pw(t, e), t float32 in [0, 1]."""
    if F(e) == 1:
        return t
    steps = entries - 1
    T = table(e, steps)
    u = (t * F(steps)).astype(F)
    i = np.rint(u).astype(np.int64) if index_rounded else u.astype(np.int64)  # (the cast truncates)
    i = np.minimum(i, steps - 1)
    f = (u - i.astype(F)).astype(F)
    return fmaf32(f, (T[i + 1] - T[i]).astype(F), T[i])


def alpha_of(src_bits):
    return np.ascontiguousarray(src_bits, np.uint16)[..., 3].view(np.float16).astype(F)


def normal(A, X, Y, s, interior_factor=False):
    """(Nx, Ny), float32 (len(Y), len(X)), at the texels X x Y (int64) of the alpha image A (H, W) float32; s the plan's (2, 3)."""
    H, W = A.shape
    xl, xh, yl, yh = np.maximum(X - 1, 0), np.minimum(X + 1, W - 1), np.maximum(Y - 1, 0), np.minimum(Y + 1, H - 1)
    left, right, up, down = (X > 0)[None, :], (X + 1 < W)[None, :], (Y > 0)[:, None], (Y + 1 < H)[:, None]
    span_x, span_y = (xh - xl)[None, :], (yh - yl)[:, None]
    wsum_y, wsum_x = 2 + up.astype(np.int64) + down, 2 + left.astype(np.int64) + right
    two = F(2.0)

    def at(rows, cols):
        return A[rows][:, cols]

    def weighted(before, after, a0, a1, a2):  # the weights (1, 2, 1) over what exists, ascending, left to right
        mid = (two * a1).astype(F)
        c = np.where(before, (a0 + mid).astype(F), mid)
        return np.where(after, (c + a2).astype(F), c).astype(F)

    def c(col):
        return weighted(up, down, at(yl, col), at(Y, col), at(yh, col))

    def r(row):
        return weighted(left, right, at(row, xl), at(row, X), at(row, xh))

    with np.errstate(all="ignore"):
        gx, gy = (c(xh) - c(xl)).astype(F), (r(yh) - r(yl)).astype(F)
        if interior_factor:  # (a wrong variant)
            sx, sy = np.broadcast_to(s[1, 2], gx.shape), np.broadcast_to(s[1, 2], gy.shape)
        else:
            sx, sy = s[np.maximum(span_x, 1) - 1, wsum_y - 2], s[np.maximum(span_y, 1) - 1, wsum_x - 2]
        nx = np.where(span_x == 0, F(0.0), (sx * gx).astype(F)).astype(F)
        ny = np.where(span_y == 0, F(0.0), (sy * gy).astype(F)).astype(F)
    return np.broadcast_to(nx, gx.shape), np.broadcast_to(ny, gy.shape)


def lighting(src_bits, rect=None, dst_bits=None, interior_factor=False, half=True, normal_first=False, reciprocal=False, h_first=False,
             entries=ENTRIES, index_rounded=False, alpha_one=False, clamp_first=False, **kw):
    """The image jh_lighting leaves in dst.  src_bits: (H, W, 4) uint16 f16 bit patterns (a never-written source: all zero); rect = (x,
    y, width, height), None: the whole image; dst_bits: what dst held (None: never written, transparent black).  (H, W, 4) uint16."""
    d, p = check(**kw), plan(**kw)
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    H, W, _ = src_bits.shape
    if W > MAX_EXTENT or H > MAX_EXTENT:
        raise ValueError("an extent above 2^23")
    out = np.zeros_like(src_bits) if dst_bits is None else np.array(dst_bits, np.uint16)
    x, y, rw, rh = resolve(src_bits.shape, rect)
    if rw == 0 or rh == 0:
        return out
    A = alpha_of(src_bits)
    X, Y = x + np.arange(rw, dtype=np.int64), y + np.arange(rh, dtype=np.int64)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        nx, ny = normal(A, X, Y, p["s"], interior_factor)
        nlen = np.sqrt(fmaf32(nx, nx, fmaf32(ny, ny, one))).astype(F)
        shape = nx.shape
        if d["light"] == DISTANT:
            lx, ly, lz = (np.broadcast_to(p["ldir"][k], shape) for k in range(3))
        else:
            off = F(0.5) if half else F(0.0)
            Z = (d["surface_scale"] * A[Y][:, X]).astype(F)
            vx = np.broadcast_to((p["p"][0] - (X.astype(F) + off).astype(F)).astype(F)[None, :], shape)
            vy = np.broadcast_to((p["p"][1] - (Y.astype(F) + off).astype(F)).astype(F)[:, None], shape)
            vz = (p["p"][2] - Z).astype(F)
            ln = np.sqrt(fmaf32(vz, vz, fmaf32(vy, vy, (vx * vx).astype(F)))).astype(F)
            if reciprocal:  # (a wrong variant)
                rl = (one / ln).astype(F)
                lx, ly, lz = (vx * rl).astype(F), (vy * rl).astype(F), (vz * rl).astype(F)
            else:
                lx, ly, lz = (vx / ln).astype(F), (vy / ln).astype(F), (vz / ln).astype(F)
        C = [np.broadcast_to(d["color"][k], shape) for k in range(3)]
        if d["light"] == SPOT:
            S = p["sdir"]
            m = (-fmaf32(lz, S[2], fmaf32(ly, S[1], (lx * S[0]).astype(F)))).astype(F)
            lit = (m > 0) & (m >= p["cone"])
            t = np.where(lit, fmin(m, one), zero).astype(F)
            pw = power(t, d["spot_exponent"], entries, index_rounded)
            C = [np.where(lit, (c * pw).astype(F), zero).astype(F) for c in C]
        if normal_first:  # (a wrong variant)
            nx, ny, nz, div = (nx / nlen).astype(F), (ny / nlen).astype(F), (one / nlen).astype(F), None
        else:
            nz, div = None, nlen
        if d["kind"] == DIFFUSE:
            dot = fmaf32(nx, lx, fmaf32(ny, ly, lz if nz is None else (nz * lz).astype(F)))
            t = fmax(dot if div is None else (dot / div).astype(F), zero)
        else:
            hz = (lz + one).astype(F)
            hlen = np.sqrt(fmaf32(hz, hz, fmaf32(ly, ly, (lx * lx).astype(F)))).astype(F)
            if h_first:  # (a wrong variant)
                hx, hy, hz = (lx / hlen).astype(F), (ly / hlen).astype(F), (hz / hlen).astype(F)
                q = (fmaf32(nx, hx, fmaf32(ny, hy, hz)) / nlen).astype(F)
            else:
                dot = fmaf32(nx, lx, fmaf32(ny, ly, hz if nz is None else (nz * hz).astype(F)))
                q = (dot / (hlen if div is None else (div * hlen).astype(F))).astype(F)
            t = power(fmin(fmax(q, zero), one), d["specular_exponent"], entries, index_rounded)
        k = (d["constant"] * t).astype(F)
        if clamp_first:  # (a wrong variant)
            V = [(fmin(k, one) * c).astype(F) for c in C]
        else:
            V = [fmin((k * c).astype(F), one) for c in C]
        if d["kind"] == DIFFUSE:
            v = np.stack(V + [np.broadcast_to(one, shape)], axis=-1)
        else:
            a = fmax(fmax(V[0], V[1]), V[2])
            a_inv = (one / fmax(a, F(1e-6))).astype(F)
            v = np.stack([((c * a_inv).astype(F) + zero).astype(F) for c in V] + [(a + zero).astype(F)], axis=-1)
            if alpha_one:  # (a wrong variant)
                v = np.stack(V + [np.broadcast_to(one, shape)], axis=-1)
        out[y:y + rh, x:x + rw] = v.astype(F).astype(np.float16).view(np.uint16)
    return out


def exact(src_bits, rect=None, **kw):
    """The specification in binary64 on the same inputs (the alpha as stored, the light as the descriptor's doubles, real pow):
    ((rh, rw, 3) the premultiplied colour min(k C, 1) before any store, (rh, rw) the SPECULAR alpha).  Where a length is 0 the
    result is whatever numpy gives; the tests look only at texels where every length is well away from 0."""
    d = check(**kw)
    src_bits = np.ascontiguousarray(src_bits, np.uint16)
    x, y, rw, rh = resolve(src_bits.shape, rect)
    A = alpha_of(src_bits).astype(np.float64)
    H, W = A.shape
    X, Y = x + np.arange(rw, dtype=np.int64), y + np.arange(rh, dtype=np.int64)
    ss = float(d["surface_scale"])
    s64 = np.array([[-ss * 2.0 / (span * wsum) for wsum in (2, 3, 4)] for span in (1, 2)])
    with np.errstate(all="ignore"):
        xl, xh, yl, yh = np.maximum(X - 1, 0), np.minimum(X + 1, W - 1), np.maximum(Y - 1, 0), np.minimum(Y + 1, H - 1)
        up, down, left, right = (Y > 0)[:, None], (Y + 1 < H)[:, None], (X > 0)[None, :], (X + 1 < W)[None, :]

        def c(col):
            return np.where(up, A[yl][:, col], 0.0) + 2.0 * A[Y][:, col] + np.where(down, A[yh][:, col], 0.0)

        def r(row):
            return np.where(left, A[row][:, xl], 0.0) + 2.0 * A[row][:, X] + np.where(right, A[row][:, xh], 0.0)

        span_x, span_y = (xh - xl)[None, :], (yh - yl)[:, None]
        wsum_y, wsum_x = 2 + up.astype(np.int64) + down, 2 + left.astype(np.int64) + right
        nx = np.where(span_x == 0, 0.0, s64[np.maximum(span_x, 1) - 1, wsum_y - 2] * (c(xh) - c(xl)))
        ny = np.where(span_y == 0, 0.0, s64[np.maximum(span_y, 1) - 1, wsum_x - 2] * (r(yh) - r(yl)))
        nlen = np.sqrt(nx * nx + ny * ny + 1.0)
        if d["light"] == DISTANT:
            n = _length(d["direction"])
            lx, ly, lz = (np.full(nx.shape, v / n) for v in d["direction"])
        else:
            px, py, pz = d["position"]
            vx, vy, vz = np.broadcast_to((px - (X + 0.5))[None, :], nx.shape), np.broadcast_to((py - (Y + 0.5))[:, None], nx.shape), pz - ss * A[Y][:, X]
            ln = np.sqrt(vx * vx + vy * vy + vz * vz)
            lx, ly, lz = vx / ln, vy / ln, vz / ln
        C = [np.full(nx.shape, float(v)) for v in d["color"]]
        if d["light"] == SPOT:
            sv = tuple(a - b for a, b in zip(d["points_at"], d["position"]))
            n = _length(sv)
            m = -(lx * sv[0] + ly * sv[1] + lz * sv[2]) / n
            lit = (m > 0) & (m >= d["cone_cos"])
            pw = np.power(np.clip(m, 0.0, 1.0), float(d["spot_exponent"]))
            C = [np.where(lit, v * pw, 0.0) for v in C]
        if d["kind"] == DIFFUSE:
            t = np.maximum((nx * lx + ny * ly + lz) / nlen, 0.0)
        else:
            hz = lz + 1.0
            hlen = np.sqrt(lx * lx + ly * ly + hz * hz)
            t = np.power(np.clip((nx * lx + ny * ly + hz) / (nlen * hlen), 0.0, 1.0), float(d["specular_exponent"]))
        k = float(d["constant"]) * t
        V = np.stack([np.minimum(k * v, 1.0) for v in C], axis=-1)
    return V, V.max(axis=-1)
