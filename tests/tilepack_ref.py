"""Reference implementation of the tile pack, written from the format text alone (include/jello_hip.h).
Deliberately plain -- one tile at a time, bytes compared as bytes -- and independent of jello_amd/tilepack.py.

Format.  A frame: `height` rows of `width` texels of 4 or 8 bytes.  Tiles of 16 x 16 texels, tiles_x = ceil(width / 16),
tiles_y = ceil(height / 16), t = ty * tiles_x + tx; only in-frame texels are compared.  Classes, by precedence: SKIP (a
reference is given and the tile equals the reference's), SOLID (all in-frame texels equal; one texel stored), RAW (256
texels, row-major, out-of-frame texels zero).  Pack = header of 8 little-endian u32 (magic 0x3150544A, width, height,
texel_bytes, n_entries, n_solid, n_raw, flags with bit 0 = reference used) | entries (word0 = t | RAW << 31, word1 = index in
its section), ascending t | solid texels | raw blocks; every section starts at the next multiple of 16, padding is zero.
Reading: the header is rejected (one reject, nothing written) unless magic / width / height / texel_bytes are the expected
ones, n_solid + n_raw = n_entries, n_entries <= tile count and the total size <= len(pack); an entry is rejected when its
tile index >= tile count or its payload index >= its section's count.

Frames here are numpy arrays of shape (H, W, 4): uint8 (4-byte texels) or uint16 (8-byte texels).
"""
import struct

import numpy as np

MAGIC = 0x3150544A
SKIP, SOLID, RAW = "skip", "solid", "raw"


def _pad16(b):
    return b + bytes(-len(b) % 16)


def classify(frame, ref=None):
    """Class of every tile, in tile-index order."""
    h, w = frame.shape[:2]
    out = []
    for y0 in range(0, h, 16):
        for x0 in range(0, w, 16):
            tile = frame[y0:y0 + 16, x0:x0 + 16]
            if ref is not None and tile.tobytes() == ref[y0:y0 + 16, x0:x0 + 16].tobytes():
                out.append(SKIP)
                continue
            texels = tile.reshape(-1, 4)  # (unsigned integers: equal values are equal bytes)
            out.append(SOLID if bool((texels == texels[0]).all()) else RAW)
    return out


def pack(frame, ref=None):
    h, w = frame.shape[:2]
    tb = 4 * frame.dtype.itemsize
    assert frame.shape[2] == 4 and tb in (4, 8) and (ref is None or (ref.shape == frame.shape and ref.dtype == frame.dtype))
    entries, solid, raw = b"", b"", b""
    n_solid = n_raw = 0
    t = 0
    classes = classify(frame, ref)
    for y0 in range(0, h, 16):
        for x0 in range(0, w, 16):
            c = classes[t]
            tile = frame[y0:y0 + 16, x0:x0 + 16]
            if c == SOLID:
                entries += struct.pack("<II", t, n_solid)
                solid += tile[0, 0].tobytes()
                n_solid += 1
            elif c == RAW:
                entries += struct.pack("<II", t | (1 << 31), n_raw)
                block = np.zeros((16, 16, 4), dtype=frame.dtype)
                block[:tile.shape[0], :tile.shape[1]] = tile
                raw += block.tobytes()
                n_raw += 1
            t += 1
    header = struct.pack("<8I", MAGIC, w, h, tb, n_solid + n_raw, n_solid, n_raw, 0 if ref is None else 1)
    return header + _pad16(entries) + _pad16(solid) + raw


def total_size(pack_bytes):
    """Total size of the pack, from its header alone."""
    _, _, _, tb, n_entries, n_solid, n_raw, _ = struct.unpack_from("<8I", pack_bytes, 0)
    return 32 + (8 * n_entries + 15) // 16 * 16 + (tb * n_solid + 15) // 16 * 16 + 256 * tb * n_raw


def unpack(pack_bytes, frame):
    """Applies the pack to `frame` in place; returns the number of rejects."""
    h, w = frame.shape[:2]
    tb = 4 * frame.dtype.itemsize
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    if len(pack_bytes) < 32:
        return 1
    magic, pw, ph, ptb, n_entries, n_solid, n_raw, _ = struct.unpack_from("<8I", pack_bytes, 0)
    if magic != MAGIC or (pw, ph, ptb) != (w, h, tb) or n_solid + n_raw != n_entries or n_entries > n_tiles:
        return 1
    off_solid = 32 + (8 * n_entries + 15) // 16 * 16
    off_raw = off_solid + (tb * n_solid + 15) // 16 * 16
    if off_raw + 256 * tb * n_raw > len(pack_bytes):
        return 1
    rejects = 0
    tiles_x = (w + 15) // 16
    for e in range(n_entries):
        word0, k = struct.unpack_from("<II", pack_bytes, 32 + 8 * e)
        t, is_raw = word0 & 0x7FFFFFFF, bool(word0 >> 31)
        if t >= n_tiles or k >= (n_raw if is_raw else n_solid):
            rejects += 1
            continue
        y0, x0 = 16 * (t // tiles_x), 16 * (t % tiles_x)
        th, tw = min(16, h - y0), min(16, w - x0)
        if is_raw:
            block = np.frombuffer(pack_bytes, dtype=frame.dtype, count=1024, offset=off_raw + 256 * tb * k).reshape(16, 16, 4)
            frame[y0:y0 + th, x0:x0 + tw] = block[:th, :tw]
        else:
            frame[y0:y0 + th, x0:x0 + tw] = np.frombuffer(pack_bytes, dtype=frame.dtype, count=4, offset=off_solid + tb * k)
    return rejects
