"""The one Python statement of a 4:2:0 frame's layout (jello_amd/imagecalls.py: yuv_plane_shapes, packed_plane_offsets), without a
GPU: the planes' shapes of include/jello_frame.h, and how the engine packs them into a buffer of its own -- one after the other,
tight rows, each start a multiple of 16 -- on the way out (Engine._yuv_desc, Engine._download_yuv) and on the way in
(_yuv_array_source).  The values are written out, not computed."""
import numpy as np
import pytest

import jello_amd
from jello_amd import YuvLayout
from jello_amd.imagecalls import _yuv_array_source, packed_plane_offsets, yuv_plane_shapes

NV12, I420 = int(YuvLayout.NV12), int(YuvLayout.I420)

# (width, height, layout): shapes [(rows, bytes per row)], offsets, total
CASES = [
    ((5, 3, NV12), [(3, 5), (2, 6)], [0, 16], 32),
    ((5, 3, I420), [(3, 5), (2, 3), (2, 3)], [0, 16, 32], 48),
    ((17, 3, NV12), [(3, 17), (2, 18)], [0, 64], 112),
    ((17, 3, I420), [(3, 17), (2, 9), (2, 9)], [0, 64, 96], 128),
    ((1, 1, NV12), [(1, 1), (1, 2)], [0, 16], 32),
    ((1, 1, I420), [(1, 1), (1, 1), (1, 1)], [0, 16, 32], 48),
    ((0, 0, NV12), [(0, 0), (0, 0)], [0, 0], 0),
]


@pytest.mark.parametrize("frame,shapes,offsets,total", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_the_shapes_and_the_packed_offsets(frame, shapes, offsets, total):
    assert yuv_plane_shapes(*frame) == shapes
    assert packed_plane_offsets(yuv_plane_shapes(*frame)) == (offsets, total)
    assert jello_amd.Engine.yuv_plane_shapes(*frame) == shapes  # (what tests and tools call)
    assert jello_amd.Engine.yuv_plane_shapes(frame[0], frame[1], YuvLayout(frame[2])) == shapes


@pytest.mark.parametrize("frame,shapes,offsets,total", [c for c in CASES if c[0][0]], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_host_arrays_are_placed_at_those_offsets_with_tight_pitches(frame, shapes, offsets, total):
    w, h, layout = frame
    arrays = [np.full(s, 10 * (i + 1), np.uint8) for i, s in enumerate(shapes)]
    for planes in ([arrays] if layout == I420 else [arrays, [arrays[0], arrays[1].reshape(shapes[1][0], -1, 2)]]):
        host, placed, rect = _yuv_array_source(planes, layout, None)
        assert placed == [(o, rb) for o, (_, rb) in zip(offsets, shapes)] and rect == (0, 0, w, h)
        assert host.dtype == np.uint8 and host.size == total
        want = np.zeros(total, np.uint8)  # (the bytes between a plane's end and the next start are zero)
        for i, (o, (rows, rb)) in enumerate(zip(offsets, shapes)):
            want[o:o + rows * rb] = 10 * (i + 1)
        assert np.array_equal(host, want)


def test_a_frame_without_texels_uploads_nothing():
    assert _yuv_array_source((np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8)), NV12, None) is None
