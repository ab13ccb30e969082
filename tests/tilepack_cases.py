"""The frames the tile-pack tests run on (tests/test_tilepack_spec.py on the CPU, tests/test_gpu_tilepack.py on the device):
every size with both texel sizes, without a reference and with one that is equal everywhere, different everywhere or mixed."""
import numpy as np

SIZES = [(1, 1), (16, 16), (17, 33), (250, 40), (1024, 16)]  # (width, height)
DTYPES = {4: np.uint8, 8: np.uint16}
REFS = ["none", "equal", "different", "mixed"]


def make_frame(width, height, texel_bytes, seed):
    """A frame with flat and noisy tiles side by side: tile (tx, ty) is one colour when (tx + ty) is even, noise otherwise
    (a one-tile frame is noise unless it is a single texel)."""
    dt = DTYPES[texel_bytes]
    rng = np.random.default_rng(seed)
    f = rng.integers(0, np.iinfo(dt).max + 1, size=(height, width, 4), dtype=dt)
    for ty in range((height + 15) // 16):
        for tx in range((width + 15) // 16):
            if (tx + ty) % 2 == 0 and (width > 16 or height > 16):
                f[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = rng.integers(0, np.iinfo(dt).max + 1, size=4, dtype=dt)
    return f


def make_ref(frame, kind, seed):
    """The reference frame of a case: None, equal everywhere, different in every texel, or equal except in every third tile
    (where one texel differs)."""
    if kind == "none":
        return None
    r = frame.copy()
    if kind == "different":
        r[..., 0] ^= 1
    elif kind == "mixed":
        h, w = frame.shape[:2]
        tiles_x = (w + 15) // 16
        rng = np.random.default_rng(seed + 1000)
        for t in range(tiles_x * ((h + 15) // 16)):
            if t % 3 == 0:
                y0, x0 = 16 * (t // tiles_x), 16 * (t % tiles_x)
                y = y0 + int(rng.integers(0, min(16, h - y0)))
                x = x0 + int(rng.integers(0, min(16, w - x0)))
                r[y, x, 3] ^= 0x80
    return r


CASES = [(w, h, tb, kind) for (w, h) in SIZES for tb in (4, 8) for kind in REFS]


def case_frames(w, h, tb, kind):
    seed = w * 131 + h * 7 + tb
    f = make_frame(w, h, tb, seed)
    return f, make_ref(f, kind, seed)
