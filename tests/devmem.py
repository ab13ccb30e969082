"""What the -m gpu tests of the post-render calls share: ids that never collide within a session, caller-owned device memory
behind a canary, context images, the frame's RGBA16F target, and the scene set the blits are tested on."""
import numpy as np

import jello_amd
from jello_amd import ImageFormat, scenes

CANARY = 0xA7
_next_id = [0x7E57_5000_0000]


def _id():
    _next_id[0] += 1
    return _next_id[0]


class DevBuf:
    """A context buffer used as caller-owned device memory: `data` (bytes-like) or `nbytes` of CANARY."""

    def __init__(self, engine, nbytes=None, data=None):
        host = np.full(max(int(nbytes), 16), CANARY, np.uint8) if data is None else np.frombuffer(bytes(data), np.uint8)
        self.e, self.id, self.n = engine, _id(), host.size
        engine._check(engine.hip.jh_upload(engine.ctx, self.id, host.ctypes.data, self.n), "upload")
        self.ptr = engine.hip.jh_buffer_device_ptr(engine.ctx, self.id)

    def bytes(self):
        return self.e.download(self.id, self.n).copy()

    def free(self):
        self.e.hip.jh_free(self.e.ctx, self.id)


class Image:
    """An image of the context: uploaded from (H, W, 4) uint16 bits, or only created (`bits` None: never written)."""

    def __init__(self, engine, bits=None, width=None, height=None, fmt=ImageFormat.RGBA16_FLOAT):
        self.e, self.id = engine, _id()
        if bits is None:
            self.w, self.h = width, height
            engine.create_image(self.id, width, height, fmt)
        else:
            bits = np.ascontiguousarray(bits, np.uint16)
            self.h, self.w, _ = bits.shape
            engine.upload_image(self.id, bits, fmt)

    def bits(self):
        return self.e.download_image(self.id, self.w, self.h).copy()

    def free(self):
        self.e.free_image(self.id)


def target_of(engine, rec):
    t = rec.target
    return engine.download_image(t["id"], t["width"], t["height"]).copy()


def _fuzz(seed, size=256):
    return scenes.scene_fuzz(seed, size=size)


def _odd(w, h, seed):
    s, p = scenes.scene_fuzz(seed, size=max(w, h), n=20)
    p.width, p.height = w, h
    return s, p


def _msaa(aa):
    s, p = scenes.scene_c1()
    p.aa = aa
    return s, p


SCENES = {
    "c1_area": scenes.scene_c1,
    "c1_msaa8": lambda: _msaa(jello_amd.Aa.Msaa8),
    "c1_msaa16": lambda: _msaa(jello_amd.Aa.Msaa16),
    "images": scenes.scene_images,
    "c4_small": lambda: scenes.scene_c4(1500, 512),
    "odd_1x1": lambda: _odd(1, 1, 11),
    "odd_3x7": lambda: _odd(3, 7, 12),
    "odd_1001x517": lambda: _odd(1001, 517, 13),
}
SCENES.update({"fuzz%d" % k: (lambda k=k: _fuzz(k)) for k in range(8)})
