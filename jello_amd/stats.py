"""The record of jh_stats on the host: ``Stats`` reads its bytes, ``merge`` combines the records of disjoint
rectangles, and ``levels`` / ``equalize`` turn a histogram into the LINEAR and TABLE functions of ``Engine.color_filter`` --
``engine.color_filter(img, funcs=stats.levels(engine.stats(img), clip=(0.01, 0.01))[:3] + [None])``.  Plain numpy, no GPU; every
function states its arithmetic."""
import numpy as np

from .imagecalls import COLOR_MAX_VALUES, ColorFunc, StatsWhat

RECORD = np.dtype([("x", "<u4"), ("y", "<u4"), ("width", "<u4"), ("height", "<u4"), ("what", "<u4"), ("population", "<u4"), ("transfer", "<u4"),
                   ("reserved", "<u4"), ("content_count", "<u4"), ("bounds", "<u4", (4,)), ("population_count", "<u4"), ("nan_count", "<u4", (4,)),
                   ("min_bits", "<u2", (4,)), ("max_bits", "<u2", (4,)), ("histogram", "<u4", (4, 256))])  # jh_stats_record
MIN_NEUTRAL, MAX_NEUTRAL = 0x7C00, 0xFC00  # what a channel without a non-NaN value reports: +Inf and -Inf


def _key(bits):
    """The order key of non-NaN f16 patterns (include/jello_stats.h): negative: ~h, else h | 0x8000, compared unsigned -- totalOrder."""
    h = np.asarray(bits, np.uint32)
    return np.where(h & 0x8000, ~h & 0xFFFF, h | 0x8000).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & 0x8000, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint16)


class Stats:
    """A view of one jh_stats_record.  `record` is the numpy structured scalar; the attributes name its fields."""

    def __init__(self, data):
        raw = np.frombuffer(bytes(data), np.uint8)
        if raw.size != RECORD.itemsize:
            raise ValueError("jh_stats: a record has %d bytes, not %d" % (RECORD.itemsize, raw.size))
        self.record = raw.copy().view(RECORD)[0]

    parse = classmethod(lambda cls, data: cls(data))

    def tobytes(self):
        return self.record.tobytes()

    def __eq__(self, other):
        return isinstance(other, Stats) and self.tobytes() == other.tobytes()

    rect = property(lambda s: tuple(int(s.record[k]) for k in ("x", "y", "width", "height")))
    what = property(lambda s: StatsWhat(int(s.record["what"])))
    population = property(lambda s: int(s.record["population"]))
    transfer = property(lambda s: int(s.record["transfer"]))
    content_count = property(lambda s: int(s.record["content_count"]))
    population_count = property(lambda s: int(s.record["population_count"]))
    nan_count = property(lambda s: tuple(int(v) for v in s.record["nan_count"]))
    min_bits = property(lambda s: tuple(int(v) for v in s.record["min_bits"]))
    max_bits = property(lambda s: tuple(int(v) for v in s.record["max_bits"]))
    histogram = property(lambda s: s.record["histogram"])

    @property
    def bounds(self):
        """(x, y, width, height) of the content's box in image coordinates, or None without content (or without BOUNDS)."""
        x0, y0, x1, y1 = (int(v) for v in self.record["bounds"])
        return None if x1 == x0 or y1 == y0 else (x0, y0, x1 - x0, y1 - y0)

    @property
    def minimum(self):
        """The four minima as float (+Inf for a channel without a non-NaN value)."""
        return tuple(float(v) for v in np.array(self.min_bits, np.uint16).view(np.float16))

    @property
    def maximum(self):
        return tuple(float(v) for v in np.array(self.max_bits, np.uint16).view(np.float16))


def parse(data):
    """The Stats of sizeof(jh_stats_record) bytes."""
    return Stats(data)


def merge(a, b):
    """The record of the union of two DISJOINT rectangles of one image under one descriptor, from their records -- the integer
    combine of the call's second launch: the rectangle is the box of the two; content_count, population_count, nan_count and every
    bin are sums; bounds is the box of the two boxes (a record without content has none); min_bits / max_bits are the min / max
    under the order key where EXTREMES was asked for.  A record of an image without texels (width x height = 0) is neutral.
    ValueError when what, population or transfer differ."""
    ra, rb = a.record, b.record
    if any(int(ra[k]) != int(rb[k]) for k in ("what", "population", "transfer")):
        raise ValueError("jh_stats: merge takes records of one descriptor")
    if int(ra["width"]) * int(ra["height"]) == 0:
        return Stats(b.tobytes())
    if int(rb["width"]) * int(rb["height"]) == 0:
        return Stats(a.tobytes())
    out = np.zeros((), RECORD)
    x0, y0 = min(int(ra["x"]), int(rb["x"])), min(int(ra["y"]), int(rb["y"]))
    x1 = max(int(ra["x"]) + int(ra["width"]), int(rb["x"]) + int(rb["width"]))
    y1 = max(int(ra["y"]) + int(ra["height"]), int(rb["y"]) + int(rb["height"]))
    out["x"], out["y"], out["width"], out["height"] = x0, y0, x1 - x0, y1 - y0
    for k in ("what", "population", "transfer"):
        out[k] = ra[k]
    what = int(ra["what"])
    out["content_count"] = int(ra["content_count"]) + int(rb["content_count"])
    if what & StatsWhat.BOUNDS:
        boxes = [r["bounds"].astype(np.int64) for r in (ra, rb) if int(r["content_count"])]
        if boxes:
            out["bounds"] = [min(bx[0] for bx in boxes), min(bx[1] for bx in boxes), max(bx[2] for bx in boxes), max(bx[3] for bx in boxes)]
    if what & (StatsWhat.EXTREMES | StatsWhat.HISTOGRAM):
        out["population_count"] = int(ra["population_count"]) + int(rb["population_count"])
        out["nan_count"] = ra["nan_count"] + rb["nan_count"]
    if what & StatsWhat.EXTREMES:
        out["min_bits"] = _unkey(np.minimum(_key(ra["min_bits"]), _key(rb["min_bits"])))
        out["max_bits"] = _unkey(np.maximum(_key(ra["max_bits"]), _key(rb["max_bits"])))
    if what & StatsWhat.HISTOGRAM:
        out["histogram"] = ra["histogram"] + rb["histogram"]
    return Stats(out.tobytes())


def percentile_codes(hist, clip=(0.0, 0.0)):
    """(lo, hi) codes of one channel's 256 bins under `clip` = (fraction cut at the dark end, at the bright end): with N the bins' sum
    and the population sorted by code, lo is the code of the texel of rank floor(clip[0] N) and hi that of rank N - 1 -
    floor(clip[1] N) -- clip 0: the lowest and the highest occupied bin.  None for N = 0 or when the ranks cross."""
    h = np.asarray(hist, np.int64)
    n = int(h.sum())
    if not (0.0 <= clip[0] < 1.0 and 0.0 <= clip[1] < 1.0):
        raise ValueError("jh_stats: a clip fraction lies in [0, 1)")
    k_lo, k_hi = int(np.floor(clip[0] * n)), n - 1 - int(np.floor(clip[1] * n))
    if n == 0 or k_lo > k_hi:
        return None
    cum = np.cumsum(h)
    return int(np.searchsorted(cum, k_lo, side="right")), int(np.searchsorted(cum, k_hi, side="right"))


def levels(stats, clip=(0.0, 0.0)):
    """Four colorfilter.linear entries (ColorFunc.LINEAR, slope, intercept), one per channel, that stretch the clipped range of the
    histogram to [0, 1]: with (lo, hi) = percentile_codes of the channel, slope = 255 / (hi - lo) and intercept = -lo / (hi - lo), in
    binary64, so that the value lo / 255 goes to 0 and hi / 255 to 1.  A channel with hi == lo or without population gets (1, 0).
    The codes are those of the record's transfer: under SRGB the functions belong to ColorSpace.SRGB."""
    if not stats.what & StatsWhat.HISTOGRAM:
        raise ValueError("jh_stats: levels needs a record with the histogram")
    out = []
    for c in range(4):
        codes = percentile_codes(stats.histogram[c], clip)
        if codes is None or codes[1] == codes[0]:
            out.append((ColorFunc.LINEAR, 1.0, 0.0))
        else:
            lo, hi = codes
            out.append((ColorFunc.LINEAR, 255.0 / (hi - lo), -float(lo) / (hi - lo)))
    return out


def equalize(stats, n=COLOR_MAX_VALUES):
    """Four colorfilter.table entries (ColorFunc.TABLE, n values) that equalise each channel: with cum the running sum of the
    channel's bins, N their total and m the count of the lowest occupied bin, value k = (cum[255 k // (n - 1)] - m) / (N - m)
    clamped at 0, the classic histogram equalisation sampled at the n inputs k / (n - 1) of feComponentTransfer's table.  A channel
    without population or with one occupied bin gets the identity k / (n - 1).  2 <= n <= JH_COLOR_MAX_VALUES = 64."""
    if not 2 <= int(n) <= COLOR_MAX_VALUES:
        raise ValueError("jh_stats: equalize takes 2 <= n <= %d values" % COLOR_MAX_VALUES)
    if not stats.what & StatsWhat.HISTOGRAM:
        raise ValueError("jh_stats: equalize needs a record with the histogram")
    n = int(n)
    out = []
    for c in range(4):
        h = stats.histogram[c].astype(np.int64)
        total, cum = int(h.sum()), np.cumsum(h)
        m = int(h[np.flatnonzero(h)[0]]) if total else 0
        if total == m:
            out.append((ColorFunc.TABLE, tuple(k / (n - 1) for k in range(n))))
        else:
            out.append((ColorFunc.TABLE, tuple(max(int(cum[255 * k // (n - 1)]) - m, 0) / (total - m) for k in range(n))))
    return out
