"""Host-side consumer of tile packs (jh_pack_tiles; the format is in include/jello_hip.h and DESIGN.md 5.4).  numpy only, no GPU.

    bound(w, h, texel_bytes)    size of the largest pack of such a frame (jh_pack_bound)
    parse_header(pack)          the header as a dict, with the section offsets and the total size
    apply(pack, array)          writes the pack's SOLID and RAW tiles into an (H, W, 4) uint8 / uint16 array in place

A pack that came over a wire is untrusted: apply validates it by the rules jh_unpack_tiles uses, never raises on its
content and never writes outside the array; it returns the number of rejects (entries; a rejected header counts once).
"""
import numpy as np

MAGIC = 0x3150544A  # "JTP1"
TILE = 16
HEADER_BYTES = 32
FLAG_REFERENCE = 1


def _align16(n):
    return (n + 15) & ~15


def _tiles(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def bound(width, height, texel_bytes):
    """Size of the all-RAW pack of a width x height frame: no pack is larger.  0 for a texel size other than 4 or 8."""
    if texel_bytes not in (4, 8):
        return 0
    tx, ty = _tiles(width, height)
    n = tx * ty
    return HEADER_BYTES + _align16(8 * n) + n * 256 * texel_bytes


def parse_header(pack):
    """The header's fields plus entries_offset, solid_offset, raw_offset and total_bytes, or None when `pack` is shorter
    than a header, has another magic, a texel size other than 4 or 8 or counts that do not add up."""
    if len(pack) < HEADER_BYTES:
        return None
    magic, width, height, tb, n_entries, n_solid, n_raw, flags = (int(v) for v in np.frombuffer(pack, dtype="<u4", count=8))
    if magic != MAGIC or tb not in (4, 8) or n_solid + n_raw != n_entries:
        return None
    solid_offset = HEADER_BYTES + _align16(8 * n_entries)
    raw_offset = solid_offset + _align16(tb * n_solid)
    return {"width": width, "height": height, "texel_bytes": tb, "n_entries": n_entries, "n_solid": n_solid, "n_raw": n_raw,
            "flags": flags, "entries_offset": HEADER_BYTES, "solid_offset": solid_offset, "raw_offset": raw_offset,
            "total_bytes": raw_offset + 256 * tb * n_raw}


def apply(pack, array):
    """Writes the SOLID and RAW tiles of `pack` into `array` in place: (H, W, 4) uint8 for 4-byte texels, uint16 for 8-byte
    ones, C-contiguous texels.  SKIP tiles keep what the array holds.  Returns the number of rejects."""
    if array.ndim != 3 or array.shape[2] != 4 or array.dtype not in (np.uint8, np.uint16) or array.strides[2] != array.itemsize \
            or array.strides[1] != 4 * array.itemsize:
        raise ValueError("apply: the array must be (H, W, 4) uint8 or uint16 with contiguous texels")
    height, width = array.shape[:2]
    tb = 4 * array.itemsize
    h = parse_header(pack)
    tiles_x, tiles_y = _tiles(width, height)
    n_tiles = tiles_x * tiles_y
    if h is None or h["width"] != width or h["height"] != height or h["texel_bytes"] != tb or h["n_entries"] > n_tiles \
            or h["total_bytes"] > len(pack):
        return 1
    entries = np.frombuffer(pack, dtype="<u4", count=2 * h["n_entries"], offset=HEADER_BYTES).reshape(-1, 2)
    solid = np.frombuffer(pack, dtype=array.dtype, count=4 * h["n_solid"], offset=h["solid_offset"]).reshape(-1, 4)
    raw = np.frombuffer(pack, dtype=array.dtype, count=1024 * h["n_raw"], offset=h["raw_offset"]).reshape(-1, TILE, TILE, 4)
    rejects = 0
    for word0, k in entries.tolist():
        t, is_raw = word0 & 0x7FFFFFFF, word0 >> 31
        if t >= n_tiles or k >= (h["n_raw"] if is_raw else h["n_solid"]):
            rejects += 1
            continue
        y0, x0 = (t // tiles_x) * TILE, (t % tiles_x) * TILE
        view = array[y0:y0 + TILE, x0:x0 + TILE]  # (clipped to the frame by the slice)
        view[...] = raw[k, :view.shape[0], :view.shape[1]] if is_raw else solid[k]
    return rejects
