"""3D colour lookup tables for ``Engine.lut3d`` (jh_lut3d, the rule: DESIGN.md 5.23): the identity, a table from a function, the
``.cube`` text format, and the image a table travels as.  Plain numpy, no GPU.

A table is an (N, N, N, 3) array indexed [b, g, r]: ``lut[k, j, i]`` is the output colour for the input (r, g, b) = (i, j, k) /
(N - 1) -- red varies fastest in memory, the order of a ``.cube`` file.  Its image is (N * N, N, 4) f16 bit patterns, entry
(i, j, k) at the texel (x = i, y = j + N k), alpha 1.0: ``engine.upload_image(lut_id, lut3d.as_image(lut3d.from_cube(text)))``,
then ``engine.lut3d(image, lut_id)``.
"""
import numpy as np

MIN_SIZE, MAX_SIZE = 2, 65  # JH_LUT3D_MIN_SIZE, JH_LUT3D_MAX_SIZE


def _size(n):
    n = int(n)
    if not MIN_SIZE <= n <= MAX_SIZE:
        raise ValueError("lut3d: size outside 2..65")
    return n


def identity(n):
    """The (n, n, n, 3) float64 table that maps every colour to itself: entry [k, j, i] = (i, j, k) / (n - 1)."""
    n = _size(n)
    v = np.arange(n, dtype=np.float64) / float(n - 1)
    b, g, r = np.meshgrid(v, v, v, indexing="ij")
    return np.stack([r, g, b], axis=-1)


def from_function(n, fn):
    """The table of `fn`, which takes an (..., 3) float64 array of (r, g, b) in [0, 1] and returns the colours of the same shape."""
    out = np.asarray(fn(identity(n)), np.float64)
    if out.shape != (n, n, n, 3):
        raise ValueError("lut3d: the function returns another shape than it was given")
    return out


def as_image(lut):
    """The (N * N, N, 4) uint16 image of f16 bit patterns of an (N, N, N, 3) table: each value rounded once to f16, alpha 1.0."""
    lut = np.asarray(lut, np.float64)
    if lut.ndim != 4 or lut.shape[3] != 3 or not (lut.shape[0] == lut.shape[1] == lut.shape[2]):
        raise ValueError("lut3d: a table is an (N, N, N, 3) array")
    n = _size(lut.shape[0])
    image = np.empty((n * n, n, 4), np.uint16)
    with np.errstate(over="ignore"):
        image[..., :3] = lut.reshape(n * n, n, 3).astype(np.float16).view(np.uint16)
    image[..., 3] = 0x3C00
    return image


def from_image(array):
    """The (N, N, N, 3) float64 table an (N * N, N, 4) image of f16 bit patterns holds; the alpha channel is dropped."""
    a = np.ascontiguousarray(array, np.uint16)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] != a.shape[1] * a.shape[1]:
        raise ValueError("lut3d: a table's image is (N * N, N, 4)")
    n = _size(a.shape[1])
    return a[..., :3].view(np.float16).astype(np.float64).reshape(n, n, n, 3)


def from_cube(text):
    """The table of a ``.cube`` text: ``LUT_3D_SIZE N`` and N^3 lines of three numbers, red varying fastest; ``#`` comments, blank
    lines and ``TITLE`` are skipped.  ``DOMAIN_MIN`` / ``DOMAIN_MAX`` must be 0 0 0 / 1 1 1 (a shaper is jh_color_filter's work);
    ValueError for another domain, a 1D LUT, an unknown keyword, a size outside 2..65 or a wrong number of entries."""
    n, rows = None, []
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].strip()
        if not line:
            continue
        word = line.split()[0]
        if word == "TITLE":
            continue
        if word == "LUT_1D_SIZE" or word == "LUT_1D_INPUT_RANGE":
            raise ValueError("lut3d: a 1D LUT is not a 3D table")
        if word == "LUT_3D_SIZE":
            fields = line.split()
            if n is not None or len(fields) != 2 or not fields[1].isdigit():
                raise ValueError("lut3d: LUT_3D_SIZE takes one integer, once")
            n = _size(fields[1])
            continue
        if word in ("DOMAIN_MIN", "DOMAIN_MAX"):
            try:
                values = [float(v) for v in line.split()[1:]]
            except ValueError:
                values = []
            if values != [0.0 if word == "DOMAIN_MIN" else 1.0] * 3:
                raise ValueError("lut3d: %s must be %s" % (word, "0 0 0" if word == "DOMAIN_MIN" else "1 1 1"))
            continue
        if word[0].isalpha() or word[0] == "_":
            raise ValueError("lut3d: unknown keyword %s" % word)
        try:
            row = [float(v) for v in line.split()]
        except ValueError:
            row = []
        if len(row) != 3:
            raise ValueError("lut3d: an entry is three numbers")
        rows.append(row)
    if n is None:
        raise ValueError("lut3d: no LUT_3D_SIZE")
    if len(rows) != n ** 3:
        raise ValueError("lut3d: %d entries for a table of %d" % (len(rows), n ** 3))
    return np.array(rows, np.float64).reshape(n, n, n, 3)


def to_cube(array, title=None):
    """The ``.cube`` text of an (N, N, N, 3) table: every value with the 17 significant digits that give a float64 back."""
    lut = np.asarray(array, np.float64)
    if lut.ndim != 4 or lut.shape[3] != 3 or not (lut.shape[0] == lut.shape[1] == lut.shape[2]):
        raise ValueError("lut3d: a table is an (N, N, N, 3) array")
    n = _size(lut.shape[0])
    lines = ["TITLE \"%s\"" % title] if title is not None else []
    lines += ["LUT_3D_SIZE %d" % n, "DOMAIN_MIN 0.0 0.0 0.0", "DOMAIN_MAX 1.0 1.0 1.0"]
    lines += ["%.17g %.17g %.17g" % tuple(row) for row in lut.reshape(-1, 3)]
    return "\n".join(lines) + "\n"
