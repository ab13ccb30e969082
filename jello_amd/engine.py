"""Recording and Engine wrappers.

``Host.record`` = renderer.RenderFull (render.go:572-588): produces the Recording (no GPU needed).
``Engine``      = engine/hip_engine: replays a Recording on the MI355X through the C ABI.
"""
import ctypes
import enum

import numpy as np

from . import _lib
from ._lib import CConfig, CProfileNode, CProfileRecord, CYuvDesc
# the image calls' enums, constants, descriptor builders and queries; imported whole, so that they stay reachable as engine.<name>
from .imagecalls import (  # noqa: F401
    BlurEdge, BLUR_MAX_SIGMA, blur_taps, _rect, _blur_desc, COMPOSITE_TINT, _composite_desc, ResampleFilter, RESAMPLE_STRAIGHT, RESAMPLE_MAX_TAPS,
    resample_taps, _resample_desc, MorphOp, MorphEdge, MORPH_STRAIGHT, MORPH_MAX_RADIUS, _morph_desc, WarpFilter, WarpEdge, WARP_STRAIGHT, WARP_MAX_SIDE,
    _matrix6, warp_plan, warp_bounds, _warp_desc, ConvolveEdge, ConvolveMode, CONVOLVE_MAX_ORDER, CONVOLVE_MAX_TAPS, _order2, convolve_weights,
    _convolve_desc, LightKind, LightSource, LIGHTING_TABLE_ENTRIES, LIGHTING_TABLE_SPEC, LIGHTING_TABLE_SPOT, _vec3, _lighting_desc, lighting_plan,
    lighting_tables, TurbulenceKind, TURBULENCE_MAX_OCTAVES, _pair, _turbulence_desc, turbulence_plan, turbulence_tables, DisplaceChannel,
    DISPLACE_STRAIGHT, AFFINE_IDENTITY, displace_offset, _displace_desc, ShadowFlags, SHADOW_MAX_EXTENT, _shadow_desc, shadow_plan, shadow_bounds,
    box_shadow_geometry, PERSPECTIVE_STRAIGHT, PROJECTIVE_IDENTITY, _matrix9, perspective_plan, perspective_bounds, _perspective_desc, ColorSpace, ColorFunc, COLOR_CLAMP, COLOR_MAX_VALUES, COLOR_POST_SHIFT,
    IDENTITY_MATRIX, _color_desc, color_tables, _lut3d_desc, LUT3D_MIN_SIZE, LUT3D_MAX_SIZE, composite_clip, DistanceWhich, DistanceEdge, DistanceFlags, DISTANCE_MAX_RADIUS, _distance_desc,
    distance_plan, LoadAlpha, ChromaFilter, LOAD_TRANSFER, _load_surface_desc, _load_yuv_desc, _surface_array_source, yuv_plane_shapes, packed_plane_offsets, _yuv_array_source, load_texels, load_yuv_codes,
    StatsWhat, StatsPopulation, StatsTransfer, STATS_MAX_TEXELS, STATS_MAX_PARTIALS, STATS_RECORD_BYTES, _stats_desc, stats_plan, stats_codes,
)
from .scene import Compose, Mix

STAGE_NAMES = ["pathtag_reduce", "pathtag_reduce2", "pathtag_scan1", "pathtag_scan_small", "pathtag_scan_large", "bbox_clear",
               "flatten", "draw_reduce", "draw_leaf", "clip_reduce", "clip_leaf", "binning", "tile_alloc", "backdrop_dyn",
               "path_count_setup", "path_count", "coarse", "path_tiling_setup", "path_tiling", "fine_area", "fine_msaa8", "fine_msaa16"]


JH_ERR_INVALID = -1  # jh_status: the call was refused, nothing was launched or written


class ImageFormat(enum.IntEnum):
    """JlImageFormat (include/jello_formats.h): the texel format of a context image."""
    RGBA8 = 0
    RGBA8_SRGB = 1
    BGRA8 = 2
    RGBA16_FLOAT = 3


class Surface(enum.IntEnum):
    """jh_surface_format (include/jello_hip.h): RendererOptions.SurfaceFormat of the reference (lib.go:19-22)."""
    RGBA8_UNORM = 0
    BGRA8_UNORM = 1
    RGBA8_SRGB = 2
    BGRA8_SRGB = 3


class YuvLayout(enum.IntEnum):
    """jh_yuv_layout: NV12 = Y plane + interleaved (Cb, Cr) plane; I420 = Y, Cb, Cr planes (YV12: swap the chroma pointers)."""
    NV12 = 0
    I420 = 1


class YuvMatrix(enum.IntEnum):
    """jh_yuv_matrix."""
    BT601 = 0
    BT709 = 1


class YuvRange(enum.IntEnum):
    """jh_yuv_range: LIMITED = Y in [16, 235], chroma in [16, 240]; FULL = [0, 255]."""
    LIMITED = 0
    FULL = 1


class YuvTransfer(enum.IntEnum):
    """jh_yuv_transfer: the R'G'B' codes are those of Surface.RGBA8_UNORM (NONE) or Surface.RGBA8_SRGB (SRGB)."""
    NONE = 0
    SRGB = 1


# a context buffer that blit / render_to_surface convert into when the caller passes no device pointer (it only grows)
_SURFACE_BUFFER_ID = 0x5355524641434500
# context buffers of pack_tiles (the pack, when the caller passes no device pointer) and unpack_tiles (an uploaded pack)
_PACK_BUFFER_ID = 0x5041434B4F555400
_UNPACK_BUFFER_ID = 0x5041434B494E0000
_DASH_ELS_BUFFER_ID = 0x44415348454C5300
_DASH_INDEX_BUFFER_ID = 0x44415348494E4400
DASH_EL = np.dtype([("kind", "<u4"), ("p", "<f4", 6)])  # jh_dash_out_el, 28 bytes
# a context buffer that blit_yuv / render_to_yuv convert into when the caller passes no planes (it only grows)
_YUV_BUFFER_ID = 0x5955565F4F555400
# context buffers that load_surface / load_yuv upload host arrays into before they convert them (they only grow)
_LOAD_SURFACE_BUFFER_ID = 0x4C4F41445F535200
_LOAD_YUV_BUFFER_ID = 0x4C4F41445F595500
# a context buffer that stats writes its record into when the caller passes no device pointer
_STATS_BUFFER_ID = 0x53544154535F5200


class CMD:
    UPLOAD, UPLOAD_UNIFORM, UPLOAD_IMAGE, WRITE_IMAGE, DISPATCH, DISPATCH_INDIRECT, DOWNLOAD, CLEAR, FREE_BUFFER, FREE_IMAGE = range(10)


BUMP_NAMES = ["failed", "binning", "ptcl", "tile", "seg_counts", "segments", "blend", "lines"]  # the words of a BumpAllocators
RUN_UPLOADS, RUN_DISPATCHES, RUN_FREES, RUN_ALL = 1, 2, 4, 7
RUN_SKIP_FINE, RUN_ONLY_FINE = 8, 16  # with RUN_DISPATCHES: everything but the fine stage / the fine stage alone


class Recording:
    """A renderer.Recording plus the RenderConfig it was built from."""

    def __init__(self, L, handle):
        self._L, self._h = L, handle

    def __del__(self):
        try:
            self._L.jl_recording_free(self._h)
        except Exception:
            pass

    def __len__(self):
        return self._L.jl_recording_len(self._h)

    def commands(self):
        n = len(self)
        arr = self._L.jl_recording_commands(self._h)
        out = []
        for i in range(n):
            c = arr[i]
            binds = []
            for j in range(c.n_bindings):
                b = c.bindings[j]
                d = {"kind": b.kind, "id": b.id, "size": b.size, "width": b.width, "height": b.height, "format": b.format}
                if b.kind == 3:
                    d["ids"] = [b.ids[k] for k in range(b.count)]
                    d["dims"] = [(b.dims[3 * k], b.dims[3 * k + 1], b.dims[3 * k + 2]) for k in range(b.count)]
                binds.append(d)
            data = ctypes.string_at(c.data, c.data_len) if c.data_len else b""
            out.append({"kind": c.kind, "shader": c.shader, "wg": tuple(c.wg), "buf_id": c.buf_id, "buf_size": c.buf_size,
                        "buf_name": (c.buf_name or b"").decode(), "img_id": c.img_id, "img_w": c.img_w, "img_h": c.img_h,
                        "img_format": c.img_format, "data": data, "offset": c.offset, "size": c.size, "bindings": binds,
                        "coords": tuple(c.coords)})
        return out

    @property
    def config(self):
        c = self._L.jl_recording_config(self._h).contents
        return {f: (list(getattr(c, f)) if f == "base_color" else getattr(c, f)) for f, _ in CConfig._fields_}

    def config_bytes(self):
        return ctypes.string_at(self._L.jl_recording_config(self._h), ctypes.sizeof(CConfig))

    @property
    def target(self):
        i, w, h = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        self._L.jl_recording_target(self._h, ctypes.byref(i), ctypes.byref(w), ctypes.byref(h))
        return {"id": i.value, "width": w.value, "height": h.value}

    def buffer(self, name):
        sz = ctypes.c_uint64()
        i = self._L.jl_recording_buffer(self._h, name.encode(), ctypes.byref(sz))
        if i == 0:
            raise KeyError(name)
        return i, sz.value

    def workgroup_counts(self):
        names = ["path_reduce", "path_reduce2", "path_scan1", "path_scan", "bbox_clear", "flatten", "draw_reduce", "draw_leaf",
                 "clip_reduce", "clip_leaf", "binning", "tile_alloc", "path_count_setup", "backdrop", "coarse", "path_tiling_setup", "fine"]
        out = (ctypes.c_uint32 * (3 * len(names) + 1))()
        self._L.jl_recording_wg_counts(self._h, out, len(out))
        d = {n: tuple(out[3 * i:3 * i + 3]) for i, n in enumerate(names)}
        d["use_large_path_scan"] = bool(out[3 * len(names)])
        return d


class Host:
    """renderer.Renderer + renderer.Resolver + FullShaders: the recording side (CPU only)."""

    def __init__(self):
        self._L = _lib.load_host()
        self._h = self._L.jl_host_new()

    def __del__(self):
        try:
            self._L.jl_host_free(self._h)
        except Exception:
            pass

    def record(self, scene, params, robust=False):
        p = params._c()
        h = self._L.jl_record(self._h, scene._h, ctypes.byref(p), 1 if robust else 0)
        if not h:
            raise RuntimeError(self._L.jl_last_error().decode())
        return Recording(self._L, h)


class Engine:
    """engine/hip_engine: one context = one GPU + one stream.  Raises if no MI355X/HIP is available."""

    def __init__(self, device=0):
        self._L = _lib.load_host()
        self._h = self._L.jl_engine_new(device)
        if not self._h:
            raise RuntimeError("hip_engine: " + self._L.jl_last_error().decode())
        self.ctx = self._L.jl_engine_ctx(self._h)
        self.hip = self._L.hip

    def close(self):
        if self._h:
            self._L.jl_engine_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what, invalid=RuntimeError, host=False):
        """Raises for a non-zero `rc` of the call `what`: `invalid` for JH_ERR_INVALID, RuntimeError for every other code.  The
        text is jh_last_error's -- the C ABI was called directly -- or, with host=True, jl_last_error's (a jl_engine_* call)."""
        if rc != 0:
            text = self._L.jl_last_error() if host else self.hip.jh_last_error(self.ctx)
            raise (invalid if rc == JH_ERR_INVALID else RuntimeError)("%s failed (%d): %s" % (what, rc, text.decode()))

    @staticmethod
    def _frame_out():
        """The (bump, attempts) out-parameters of the jl_engine_render* calls."""
        return (ctypes.c_uint32 * 8)(), ctypes.c_int()

    def _frame(self, h, bump, attempts, label):
        """(Recording, bump dict, attempts) of the handle such a call returned; raises in `label`'s name if it returned none."""
        if not h:
            raise RuntimeError(label + ": " + self._L.jl_last_error().decode())
        return Recording(self._L, h), dict(zip(BUMP_NAMES, bump)), attempts.value

    def _own_buffer(self, buffer_id, nbytes):
        """Device pointer of the context buffer `buffer_id`, created or grown to `nbytes` first (it only grows)."""
        self._check(self.hip.jh_buffer_create(self.ctx, buffer_id, nbytes), "buffer_create")
        return self.hip.jh_buffer_device_ptr(self.ctx, buffer_id)

    def run(self, recording, flags=RUN_ALL, out_device_ptr=None):
        self._check(self._L.jl_engine_run(self._h, recording._h, flags, 0, out_device_ptr), "run_recording", host=True)

    def release(self, recording):
        self._check(self._L.jl_engine_release(self._h, recording._h), "release", host=True)

    def render(self, scene, params, out_device_ptr=None, robust=True, retain=False):
        """RenderToTexture (+ regrow loop).  Returns (Recording, bump dict, attempts)."""
        p = params._c()
        bump, attempts = self._frame_out()
        h = self._L.jl_engine_render(self._h, scene._h, ctypes.byref(p), out_device_ptr, 1 if robust else 0, 1 if retain else 0, bump, ctypes.byref(attempts))
        return self._frame(h, bump, attempts, "render_to_texture")

    def _surface(self, width, height, fmt, out_device_ptr, pitch):
        """(device pointer, pitch) to convert into: the caller's, or the engine's own buffer (tightly packed rows)."""
        if out_device_ptr is not None:
            return out_device_ptr, (4 * width if pitch is None else pitch)
        return self._own_buffer(_SURFACE_BUFFER_ID, max(4 * width * height, 16)), 4 * width

    def _download_surface(self, width, height):
        out = np.empty((height, width, 4), dtype=np.uint8)
        if out.nbytes:
            self._check(self.hip.jh_download(self.ctx, _SURFACE_BUFFER_ID, out.ctypes.data, 0, out.nbytes), "download")
        return out

    def _blit(self, src_image_id, ptr, pitch, width, height, fmt):
        self._check(self.hip.jh_blit(self.ctx, src_image_id, ptr, pitch, width, height, int(fmt)), "blit")

    def blit(self, src_image_id, width, height, fmt, out_device_ptr=None, pitch=None):
        """The blit pass of RenderToSurface (jh_blit): the RGBA16F image `src_image_id` premultiplied and converted to the
        Surface format `fmt`.  Into `out_device_ptr` (rows `pitch` bytes apart, default 4 * width; returns None) or, without
        a pointer, returned as an (height, width, 4) uint8 array."""
        ptr, pitch = self._surface(width, height, fmt, out_device_ptr, pitch)
        self._blit(src_image_id, ptr, pitch, width, height, fmt)
        return None if out_device_ptr is not None else self._download_surface(width, height)

    def render_to_surface(self, scene, params, fmt, out_device_ptr=None, pitch=None, robust=True):
        """RenderToSurface (lib.go:266-333): RenderToTexture into the engine's own RGBA16F target, then the blit.
        Returns (surface, Recording, bump dict, attempts); surface is an (H, W, 4) uint8 array without `out_device_ptr`,
        None with it.  The Recording's target image is the engine's target until the next render_to_surface."""
        ptr, pitch = self._surface(params.width, params.height, fmt, out_device_ptr, pitch)
        p = params._c()
        bump, attempts = self._frame_out()
        h = self._L.jl_engine_render_to_surface(self._h, scene._h, ctypes.byref(p), ptr, pitch, int(fmt), 1 if robust else 0, bump,
                                                ctypes.byref(attempts))
        frame = self._frame(h, bump, attempts, "render_to_surface")
        return (None if out_device_ptr is not None else self._download_surface(params.width, params.height),) + frame

    yuv_plane_shapes = staticmethod(yuv_plane_shapes)  # [(rows, bytes per row)] of a frame's planes: imagecalls.yuv_plane_shapes

    def _yuv_desc(self, width, height, layout, matrix, rng, transfer, planes):
        """(CYuvDesc, own) for `planes` = [(device pointer, pitch or None)] per plane, or None: the engine's own buffer, the
        planes as packed_plane_offsets lays them out (own = their offsets)."""
        shapes = yuv_plane_shapes(width, height, layout)
        d = CYuvDesc(int(layout), int(matrix), int(rng), int(transfer))
        own = None
        if planes is None:
            own, total = packed_plane_offsets(shapes)
            base = self._own_buffer(_YUV_BUFFER_ID, max(total, 16))
            planes = [(base + o, None) for o in own]
        for i, pl in enumerate(planes):
            ptr, pitch = pl if isinstance(pl, (tuple, list)) else (pl, None)
            d.plane[i] = ptr
            d.pitch[i] = (shapes[i][1] if i < len(shapes) else 0) if pitch is None else pitch
        return d, own

    def _download_yuv(self, width, height, layout, own):
        out = []
        for (rows, rb), off in zip(yuv_plane_shapes(width, height, layout), own):
            a = np.empty((rows, rb), dtype=np.uint8)
            if a.nbytes:
                self._check(self.hip.jh_download(self.ctx, _YUV_BUFFER_ID, a.ctypes.data, off, a.nbytes), "download")
            out.append(a)
        if int(layout) == YuvLayout.NV12:
            out[1] = out[1].reshape(out[1].shape[0], -1, 2)
        return tuple(out)

    def _blit_yuv(self, src_image_id, width, height, desc):
        self._check(self.hip.jh_blit_yuv(self.ctx, src_image_id, width, height, ctypes.byref(desc)), "blit_yuv")

    def blit_yuv(self, src_image_id, width, height, layout=YuvLayout.NV12, matrix=YuvMatrix.BT709, range=YuvRange.LIMITED,
                 transfer=YuvTransfer.NONE, planes=None):
        """jh_blit_yuv: the RGBA16F image `src_image_id` as 8-bit Y'CbCr 4:2:0 (the rule: include/jello_hip.h "YUV blit").
        Into `planes` = [(device pointer, pitch)] -- Y and CbCr for NV12; Y, Cb and Cr for I420; a pitch of None means tightly
        packed rows; returns None -- or, without planes, returned as uint8 arrays: (Y (H, W), CbCr (ceil(H/2), ceil(W/2), 2))
        for NV12, (Y, Cb, Cr) for I420."""
        d, own = self._yuv_desc(width, height, layout, matrix, range, transfer, planes)
        self._blit_yuv(src_image_id, width, height, d)
        return None if own is None else self._download_yuv(width, height, layout, own)

    def render_to_yuv(self, scene, params, layout=YuvLayout.NV12, matrix=YuvMatrix.BT709, range=YuvRange.LIMITED,
                      transfer=YuvTransfer.NONE, planes=None, robust=True):
        """RenderToTexture into the engine's own RGBA16F target, then blit_yuv.  Returns (planes, Recording, bump dict,
        attempts); planes as blit_yuv returns them.  The Recording's target image is the engine's target until the next
        render_to_surface / render_to_yuv."""
        d, own = self._yuv_desc(params.width, params.height, layout, matrix, range, transfer, planes)
        p = params._c()
        bump, attempts = self._frame_out()
        h = self._L.jl_engine_render_to_yuv(self._h, scene._h, ctypes.byref(p), ctypes.byref(d), 1 if robust else 0, bump,
                                            ctypes.byref(attempts))
        frame = self._frame(h, bump, attempts, "render_to_yuv")
        return (None if own is None else self._download_yuv(params.width, params.height, layout, own),) + frame

    def _upload_own(self, buffer_id, host):
        """`host` (uint8, contiguous) into the engine's own buffer `buffer_id`; returns its device pointer."""
        self._check(self.hip.jh_upload(self.ctx, buffer_id, host.ctypes.data, host.size), "upload")
        return self.hip.jh_buffer_device_ptr(self.ctx, buffer_id)

    def load_surface(self, dst_id, pixels, fmt, alpha=LoadAlpha.STRAIGHT, rect=None, pitch=None):
        """jh_load_surface: an 8-bit frame in the Surface format `fmt` INTO the RGBA16F image `dst_id` (the rule: DESIGN.md 5.21) --
        a decoded picture or a screen capture as the source of composite(), warp(), place_layer() ...  `pixels` is an (H, W, 4)
        uint8 array, uploaded to a buffer of the engine's own first, or a device pointer to rows `pitch` bytes apart (None: 4 x
        the rectangle's width).  `alpha`: byte 3 is straight alpha, the alpha the colour is premultiplied by (what blit() writes),
        or ignored (LoadAlpha.OPAQUE).  `rect` = (x, y, width, height) is the rectangle of dst the frame fills and has the size of
        (None: for an array (0, 0, W, H) of the array's own size -- the call never reads more than was uploaded, and an array
        larger than the image is refused; for a device pointer the whole image, with a pitch given).  Texels outside it keep
        their bits.  One launch, no scratch: always capturable.  Stream-ordered, returns nothing; ValueError for a call the rule
        refuses."""
        if isinstance(pixels, np.ndarray):
            source = _surface_array_source(pixels, rect)
            if source is None:
                return
            host, pitch, rect = source
            src = self._upload_own(_LOAD_SURFACE_BUFFER_ID, host)
        else:
            src = pixels
            if pitch is None:
                if rect is None:
                    raise ValueError("jh_load_surface: a device pointer needs a pitch or a rectangle")
                pitch = 4 * int(rect[2])
        d = _load_surface_desc(fmt, alpha, src, pitch, rect)
        self._check(self.hip.jh_load_surface(self.ctx, dst_id, ctypes.byref(d)), "load_surface", invalid=ValueError)

    def load_yuv(self, dst_id, planes, layout=YuvLayout.NV12, matrix=YuvMatrix.BT709, range=YuvRange.LIMITED, transfer=YuvTransfer.NONE,
                 chroma=ChromaFilter.BILINEAR, rect=None):
        """jh_load_yuv: an 8-bit Y'CbCr 4:2:0 frame INTO the RGBA16F image `dst_id`, opaque (the rule: DESIGN.md 5.21) -- a decoded
        video frame as the source of composite(), warp(), project_layer() ...  `planes` is either the uint8 arrays as blit_yuv()
        returns them -- (Y (H, W), CbCr (ceil(H/2), ceil(W/2), 2)) for NV12, (Y, Cb, Cr) for I420 -- uploaded to a buffer of the
        engine's own first, or [(device pointer, pitch)] per plane.  `matrix` and `range` name the coefficients, `transfer` whether
        the R'G'B' codes are sRGB-encoded (YuvTransfer.SRGB: decoded to linear) or linear; `chroma` how the half-resolution planes
        are read.  `rect` = (x, y, width, height) is the rectangle of dst the frame fills and has the size of (None: for arrays
        (0, 0, W, H) of the luma plane's own size -- the call never reads more than was uploaded, and a frame larger than the image
        is refused; for device pointers the whole image).  One launch, no scratch: always capturable.  Stream-ordered, returns
        nothing; ValueError for a call the rule refuses."""
        planes = list(planes)
        if any(isinstance(p, np.ndarray) for p in planes):
            source = _yuv_array_source(planes, layout, rect)
            if source is None:
                return
            host, placed, rect = source
            base = self._upload_own(_LOAD_YUV_BUFFER_ID, host)
            planes = [(base + o, pitch) for o, pitch in placed]
        d = _load_yuv_desc(layout, matrix, range, transfer, chroma, planes, rect)
        self._check(self.hip.jh_load_yuv(self.ctx, dst_id, ctypes.byref(d)), "load_yuv", invalid=ValueError)

    def blur(self, image_id, width, height, sigma, dst_image_id=None, edge=BlurEdge.ZERO, rect=None):
        """jh_blur: the Gaussian blur (the rule: DESIGN.md 5.7) of the RGBA16F image `image_id` into `dst_image_id` -- None: in
        place.  `sigma` is a scalar or (sigma_x, sigma_y), each in [0, 64]; `rect` = (x, y, width, height) is the rectangle of the
        destination that is written (None: the whole image); texels outside it keep their bits, source texels outside it take
        part.  Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _blur_desc(sigma, edge, rect)
        dst = image_id if dst_image_id is None else dst_image_id
        self._check(self.hip.jh_blur(self.ctx, image_id, dst, width, height, ctypes.byref(d)), "blur", invalid=ValueError)

    def composite(self, src_id, dst_id, mix=Mix.Normal, compose=Compose.SrcOver, opacity=1.0, tint=None, src_rect=None, offset=(0, 0)):
        """jh_composite: the RGBA16F image `src_id` blended onto the RGBA16F image `dst_id` (another image; the sizes may differ)
        by the rule of DESIGN.md 5.8 -- any Mix but Clip, any Compose, `opacity` in [0, 1]; `tint` = (r, g, b, a) replaces the
        source's colour and scales its alpha (a shadow out of a blurred layer); `src_rect` = (sx, sy, sw, sh) is the part of the
        source that is placed (None: all of it), `offset` = (dx, dy) where its top-left lands in dst, negative or beyond dst
        included: it is clipped, and only the placed rectangle is written.  Stream-ordered, returns nothing; ValueError for a
        call the rule refuses."""
        d = _composite_desc(mix, compose, opacity, tint, src_rect, offset)
        self._check(self.hip.jh_composite(self.ctx, src_id, dst_id, ctypes.byref(d)), "composite", invalid=ValueError)

    def resample(self, src_id, dst_id, filter=ResampleFilter.CATMULL_ROM, src_rect=None, dst_rect=None, premultiplied=True):
        """jh_resample: the rectangle `src_rect` = (x, y, width, height) of the RGBA16F image `src_id` (None: the whole image)
        resized into the rectangle `dst_rect` of the RGBA16F image `dst_id` (another image; None: the whole image) by the rule of
        DESIGN.md 5.9, at most 16:1 down on either axis.  `premultiplied`: colour is weighted by alpha while it is filtered (the
        default); False filters the four channels as they are stored (JH_RESAMPLE_STRAIGHT: data images, constant alpha).  Only the
        destination rectangle is written.  The context holds the tap tables of one geometry (filter and the rectangles' extents): a
        call with another uploads its own and makes graphs captured before it stale.  Stream-ordered, returns nothing; ValueError
        for a call the rule refuses."""
        d = _resample_desc(filter, src_rect, dst_rect, premultiplied)
        self._check(self.hip.jh_resample(self.ctx, src_id, dst_id, ctypes.byref(d)), "resample", invalid=ValueError)

    def color_filter(self, src_id, dst_id=None, matrix=None, funcs=None, space=ColorSpace.LINEAR, clamp=True, rect=None):
        """jh_color_filter: a colour matrix and per-channel transfer functions (the rule: DESIGN.md 5.10) on the rectangle `rect` =
        (x, y, width, height) of the RGBA16F image `src_id` (None: the whole image), written to the same rectangle of `dst_id` --
        None: in place.  `matrix`: 20 values, row-major 4 x 5 on the un-premultiplied (r, g, b, a, 1) (None: the identity);
        `funcs`: None or four entries as colorfilter.linear / gamma / table / discrete make them (None: IDENTITY), applied after
        the matrix; `space`: ColorSpace.SRGB encodes the colour channels before the matrix and decodes them after the funcs;
        `clamp`: the matrix's result and each func's are clamped to [0, 1].  jello_amd.colorfilter has the Filter Effects
        constructors, each the keywords of this call.  The context holds the tables of one (funcs, space, clamp): a call with
        another uploads its own and makes graphs captured before it stale; LINEAR space without funcs needs none.
        Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _color_desc(matrix, funcs, space, clamp, rect)
        dst = src_id if dst_id is None else dst_id
        self._check(self.hip.jh_color_filter(self.ctx, src_id, dst, ctypes.byref(d)), "color_filter", invalid=ValueError)

    def lut3d(self, src_id, lut_id, dst_id=None, rect=None):
        """jh_lut3d: the 3D colour lookup table held by the RGBA16F image `lut_id` -- N texels wide and N * N high, 2 <= N <= 65,
        entry (r, g, b) at (x = r, y = g + N b), as jello_amd.lut3d.as_image lays a table out -- applied by tetrahedral
        interpolation (the rule: DESIGN.md 5.23) to the rectangle `rect` = (x, y, width, height) of the RGBA16F image `src_id` (None:
        the whole image), written to the same rectangle of `dst_id` -- None: in place.  The colour is clamped to [0, 1] before the
        lookup, alpha is copied.  N is read from the LUT image's width.  The table is an image like any other: upload_image writes
        it, every image call can (bake_lut), it may be the source, never the destination.  Stream-ordered, capturable at any time,
        returns nothing; ValueError for a call the rule refuses."""
        n = ctypes.c_uint32(0)  # (an unknown id leaves 0, and the call refuses the id before it looks at the size)
        self.hip.jh_image_size(self.ctx, lut_id, ctypes.byref(n), None)
        d = _lut3d_desc(n.value, rect)
        dst = src_id if dst_id is None else dst_id
        self._check(self.hip.jh_lut3d(self.ctx, src_id, dst, lut_id, ctypes.byref(d)), "lut3d", invalid=ValueError)

    def bake_lut(self, lut_id, n, steps):
        """A chain of colour calls as ONE table: uploads lut3d.identity(n) as the RGBA16F image `lut_id` (n x n * n), then runs each
        of `steps` -- a dict of color_filter's keywords but the ids, e.g. colorfilter.sepia(1) -- over it in place.  lut3d(image,
        lut_id) then applies the whole chain in one launch, up to the table's resolution: exactly for chains that are affine per
        cell, by tetrahedral interpolation between the entries otherwise."""
        from . import lut3d as _lut3d
        self.upload_image(lut_id, _lut3d.as_image(_lut3d.identity(n)))
        for step in steps:
            self.color_filter(lut_id, **step)

    def morphology(self, src_id, dst_id=None, op=MorphOp.DILATE, radius=1, edge=MorphEdge.ZERO, rect=None, premultiplied=True):
        """jh_morphology: the RGBA16F image `src_id` eroded or dilated by a box (the rule: DESIGN.md 5.11) into the image `dst_id`
        of the same size -- None: in place.  `radius` is a scalar or (rx, ry), integers in [0, 255]: the window of a texel is
        (2 rx + 1) x (2 ry + 1).  `edge`: what a position outside the image is (MorphEdge).  `rect` = (x, y, width, height) is the
        rectangle of the destination that is written (None: the whole image); texels outside it keep their bits, source texels
        outside it take part.  `premultiplied`: the operands are colour times alpha, what feMorphology is defined on (the default);
        False takes the four channels as they are stored (JH_MORPH_STRAIGHT: data images, masks).  Stream-ordered, returns nothing;
        ValueError for a call the rule refuses."""
        d = _morph_desc(op, radius, edge, rect, premultiplied)
        dst = src_id if dst_id is None else dst_id
        self._check(self.hip.jh_morphology(self.ctx, src_id, dst, ctypes.byref(d)), "morphology", invalid=ValueError)

    def distance(self, src_id, dst_id=None, channel=3, threshold=0.5, which=DistanceWhich.OUTER, edge=DistanceEdge.ZERO, max_distance=1, scale=1.0,
                 offset=0.0, color=(1.0, 1.0, 1.0, 1.0), rect=None, straight=False):
        """jh_distance: the Euclidean distance to the shape in the RGBA16F image `src_id`, capped at `max_distance` and put through a
        linear ramp (the rule: DESIGN.md 5.20), into the image `dst_id` of the same size -- None: in place.  A texel is a seed iff its
        `channel` (0..3; 3: alpha) is >= `threshold`.  `which`: the distance s to the nearest seed (OUTER), to the nearest non-seed
        (INNER), or signed, negative inside, zero on the texel edge between the classes (SIGNED).  `edge`: under ZERO every position
        outside the image is a non-seed, under CLAMP there is none.  `max_distance`: R, an integer in [1, 255]; s is R + 1 where
        nothing lies within R.  The texel is `color` (premultiplied) times v = clamp(s scale + offset, 0, 1), stored by the store
        rule, or as it is with `straight` (masks, SDF textures).  jello_amd.distance has the ramps -- outline, inset, glow, sdf --
        each the keywords of this call.  `rect` = (x, y, width, height) is the rectangle of the destination that is written (None:
        the whole image); texels outside it keep their bits, seeds outside it count.  Stream-ordered, returns nothing; ValueError
        for a call the rule refuses."""
        d = _distance_desc(channel, threshold, which, edge, max_distance, scale, offset, color, rect, straight)
        dst = src_id if dst_id is None else dst_id
        self._check(self.hip.jh_distance(self.ctx, src_id, dst, ctypes.byref(d)), "distance", invalid=ValueError)

    def stats(self, image_id, rect=None, what=StatsWhat.ALL, channel=3, threshold=2.0 ** -24, population=StatsPopulation.ALL,
              transfer=StatsTransfer.LINEAR, out_device_ptr=None):
        """jh_stats: the content box, the channel extremes and four 256-bin histograms (the parts `what` names; the rule: DESIGN.md
        5.22) of the rectangle `rect` = (x, y, width, height) of the RGBA16F image `image_id` (None: the whole image), which is only
        read.  A texel is content iff its `channel` (0..3; 3: alpha) is >= `threshold` (the default: the smallest positive f16 --
        what is not transparent).  `population`: the extremes and the histogram are taken over every texel of the rectangle (ALL) or
        over the content texels (CONTENT).  `transfer`: the histogram's code for R, G, B.  With `out_device_ptr` --
        STATS_RECORD_BYTES of device memory on an 8-byte boundary -- the call is stream-ordered and returns None; without one the
        record goes into a buffer of the engine's own, the call waits, and a jello_amd.stats.Stats is returned.  ValueError for a
        call the rule refuses."""
        from . import stats as _stats
        d = _stats_desc(what, channel, threshold, population, transfer, rect)
        ptr = out_device_ptr if out_device_ptr is not None else self._own_buffer(_STATS_BUFFER_ID, STATS_RECORD_BYTES)
        self._check(self.hip.jh_stats(self.ctx, image_id, ctypes.byref(d), ptr), "stats", invalid=ValueError)
        if out_device_ptr is not None:
            return None
        return _stats.Stats(self.download(_STATS_BUFFER_ID, STATS_RECORD_BYTES))

    def content_bounds(self, image_id, channel=3, threshold=2.0 ** -24, rect=None):
        """The box (x, y, width, height), in image coordinates, of the texels of `rect` (None: the whole image) whose `channel` is >=
        `threshold`, or None when there is none: stats(what=BOUNDS) -- the rectangle the other image calls take for a layer."""
        return self.stats(image_id, rect, StatsWhat.BOUNDS, channel, threshold).bounds

    def auto_levels(self, src_id, dst_id=None, clip=(0.0, 0.0), population=StatsPopulation.CONTENT, transfer=StatsTransfer.LINEAR, channel=3,
                    threshold=2.0 ** -24, rect=None):
        """Stretches the colour channels of `src_id` to the full range, two calls with the host in between: stats(HISTOGRAM) over the
        `population`, then color_filter(src -> dst; None: in place) with the LINEAR functions stats.levels(record, clip) computes for R,
        G and B -- alpha keeps its values -- in ColorSpace.SRGB when the codes are `transfer` SRGB's.  `clip` = (dark, bright)
        fractions of the population that may saturate.  Returns the record."""
        from . import stats as _stats
        record = self.stats(src_id, rect, StatsWhat.HISTOGRAM, channel, threshold, population, transfer)
        funcs = _stats.levels(record, clip)[:3] + [None]
        self.color_filter(src_id, dst_id, funcs=funcs, space=ColorSpace.SRGB if int(transfer) == StatsTransfer.SRGB else ColorSpace.LINEAR, clamp=True, rect=rect)
        return record

    def round_outline(self, layer_id, target_id, width, color, scratch_image_id):
        """outline() with a disc instead of a box, and a width that may be fractional, three calls: distance(layer -> scratch, OUTER,
        the ramp distance.outline(width), the colour in the descriptor): the coverage of the layer's alpha >= 0.5 grown by a disc of
        radius `width`, in the outline's colour; composite(scratch -> target); composite(layer -> target).  `layer_id` and
        `scratch_image_id` are RGBA16F images of one size (the scratch's content is overwritten), `color` = (r, g, b, a), not
        premultiplied, as outline()'s tint."""
        from . import distance as ramps
        r, g, b, a = (float(c) for c in color)
        self.distance(layer_id, scratch_image_id, color=(r * a, g * a, b * a, a), **ramps.outline(width))
        self.composite(scratch_image_id, target_id)
        self.composite(layer_id, target_id)

    def glow(self, layer_id, target_id, radius, color, scratch_image_id, inner=False):
        """A glow of `radius` texels around a layer (inner: inside it) onto a target, two calls: distance(layer -> scratch, the ramp
        distance.glow(radius, inner), the colour in the descriptor): `color` at the shape's edge, falling linearly to nothing
        `radius` away; composite(scratch -> target, Plus) -- or SrcAtop for an inner glow, onto a target that holds the layer.
        `color` = (r, g, b, a), not premultiplied."""
        from . import distance as ramps
        r, g, b, a = (float(c) for c in color)
        self.distance(layer_id, scratch_image_id, color=(r * a, g * a, b * a, a), **ramps.glow(radius, inner))
        self.composite(scratch_image_id, target_id, compose=Compose.SrcAtop if inner else Compose.Plus)

    def warp(self, src_id, dst_id, matrix, filter=WarpFilter.BILINEAR, edge=WarpEdge.ZERO, src_rect=None, dst_rect=None, premultiplied=True):
        """jh_warp: the rectangle `src_rect` = (x, y, width, height) of the RGBA16F image `src_id` (None: the whole image) under the
        affine map `matrix` = (a, b, c, d, e, f), x' = a x + c y + e, y' = b x + d y + f, into the RGBA16F image `dst_id` (another
        image) by the rule of DESIGN.md 5.12.  The matrix takes continuous coordinates of the source rectangle to continuous
        coordinates of the destination IMAGE; `dst_rect` (None: the whole image) is only what gets written.  `edge`: what a tap
        outside the source rectangle reads (WarpEdge).  `premultiplied`: colour is weighted by alpha while it is filtered (the
        default); False filters the four channels as they are stored (JH_WARP_STRAIGHT: data images).  There is no minification
        prefilter: below about 1:2 resample() comes first.  One launch, no scratch: always capturable.  Stream-ordered, returns
        nothing; ValueError for a call the rule refuses."""
        d = _warp_desc(matrix, filter, edge, src_rect, dst_rect, premultiplied)
        self._check(self.hip.jh_warp(self.ctx, src_id, dst_id, ctypes.byref(d)), "warp", invalid=ValueError)

    def convolve(self, src_id, dst_id, weights, order=None, target=None, edge=ConvolveEdge.CLAMP, mode=ConvolveMode.PREMULTIPLIED, bias=0.0, rect=None):
        """jh_convolve: the RGBA16F image `src_id` under a small convolution kernel (the rule: DESIGN.md 5.13) into the RGBA16F image
        `dst_id`, another image of the same size.  `weights` are float32 IN THE ORDER THEY ARE APPLIED (a correlation: weights[j][i]
        multiplies the texel at (X - target_x + i, Y - target_y + j)); `order` is a scalar or (order_x, order_y), each in 1..15 (None:
        the shape of a two-dimensional `weights`); `target` = (target_x, target_y) (None: the centre, order // 2, the
        specification's default).  `edge`: what a tap outside the IMAGE reads (ConvolveEdge); `mode`: the operand (ConvolveMode);
        `bias` is added after the sum (times the result's alpha under PREMULTIPLIED).  `rect` = (x, y, width, height) is the
        rectangle of the destination that is written (None: the whole image); source texels outside it take part.  Nothing is
        clamped: color_filter(clamp=True) comes after where [0, 1] is wanted.  jello_amd.convolution has feConvolveMatrix's
        attributes (from_svg, which flips and divides) and the usual kernels, each the keywords of this call.  One launch, no
        scratch: always capturable.  Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _convolve_desc(weights, order, target, edge, mode, bias, rect)
        self._check(self.hip.jh_convolve(self.ctx, src_id, dst_id, ctypes.byref(d)), "convolve", invalid=ValueError)

    def lighting(self, src_id, dst_id, **keywords):
        """jh_lighting: feDiffuseLighting or feSpecularLighting (the rule: DESIGN.md 5.14) of the ALPHA channel of the RGBA16F image
        `src_id`, the height map, into the RGBA16F image `dst_id`, another image of the same size.  Keywords: `kind` (LightKind),
        `light` (LightSource), `surface_scale`, `constant` (kd or ks, >= 0), `specular_exponent` in [1, 128], `color` = (r, g, b) LINEAR and
        >= 0, `direction` = (x, y, z) towards a DISTANT light, `position` of a POINT or SPOT light and `points_at`, `spot_exponent` in
        [1, 128] and `cone_cos` in [-1, 1] (-1: no cone) of a SPOT light -- coordinates in texels of the image, texel (X, Y) at (X +
        0.5, Y + 0.5) -- and `rect` = (x, y, width, height), the rectangle of the destination that is written (None: the whole image);
        the alpha outside it takes part in the normals.  jello_amd.lighting has the specification's attributes (distant, point, spot,
        diffuse, specular: azimuth and elevation, the cone angle, lighting-color in sRGB), each a part of these keywords.  DIFFUSE
        gives an opaque image, SPECULAR one whose alpha is the largest of its premultiplied channels.  The context holds the power
        tables of one pair of exponents: a call with another uploads its own and makes graphs captured before it stale; exponents
        of 1 need none.  Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _lighting_desc(**keywords)
        self._check(self.hip.jh_lighting(self.ctx, src_id, dst_id, ctypes.byref(d)), "lighting", invalid=ValueError)

    def bevel(self, layer_id, target_id, scratch_a, scratch_b, sigma, light, size, surface_scale=5.0, ks=0.75, exponent=20.0, color=(1.0, 1.0, 1.0)):
        """The specification's worked example (a lit bevel of a layer's alpha) as four calls on RGBA16F images of one `size` = (width,
        height): blur(layer -> scratch_a, sigma); lighting(scratch_a -> scratch_b, SPECULAR, **light) -- `light` the keywords of
        lighting.distant / point / spot, `color` linear; composite(layer onto scratch_b, DestIn): the highlight inside the layer;
        composite(layer onto target), composite(scratch_b onto target, Plus).  The four images are distinct; the layer is only read."""
        self.blur(layer_id, size[0], size[1], sigma, dst_image_id=scratch_a)
        self.lighting(scratch_a, scratch_b, kind=LightKind.SPECULAR, surface_scale=surface_scale, constant=ks, specular_exponent=exponent, color=color, **light)
        self.composite(layer_id, scratch_b, compose=Compose.DestIn)
        self.composite(layer_id, target_id)
        self.composite(scratch_b, target_id, compose=Compose.Plus)

    def turbulence(self, dst_id, base_frequency, octaves=1, seed=0, kind=TurbulenceKind.TURBULENCE, stitch_tile=None, origin=(0.0, 0.0), rect=None):
        """jh_turbulence: feTurbulence (the rule: DESIGN.md 5.15) GENERATED into the RGBA16F image `dst_id` -- Perlin turbulence or, with
        `kind` = TurbulenceKind.FRACTAL_NOISE, fractal noise, all four channels, straight colour.  `base_frequency`: cells per texel, one
        number or (x, y), >= 0; `octaves` 0 .. 16; `seed` an int32; `stitch_tile` = (x, y, width, height) turns stitchTiles on for
        that tile (None: off); `origin` = (x, y): the coordinate of the image's corner -- texel (X, Y) is the noise at (origin.x + X +
        0.5, origin.y + Y + 0.5), so images with adjoining origins continue one field; `rect` = (x, y, width, height), the rectangle
        that is written (None: the whole image).  The context holds the tables of one seed: a call with another uploads its own (8.4
        KB) and makes graphs captured before it stale.  Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _turbulence_desc(base_frequency, octaves, seed, kind, stitch_tile, origin, rect)
        self._check(self.hip.jh_turbulence(self.ctx, dst_id, ctypes.byref(d)), "turbulence", invalid=ValueError)

    def lit_noise(self, dst_id, scratch_id, light, base_frequency=0.05, octaves=4, seed=0, kind=TurbulenceKind.TURBULENCE, stitch_tile=None,
                  origin=(0.0, 0.0), surface_scale=5.0, kd=1.0, color=(1.0, 1.0, 1.0)):
        """The specification's textured surface (lit paper, stone, cloth) as two calls on RGBA16F images of one size: turbulence into
        `scratch_id`, then lighting(scratch -> dst, DIFFUSE, **light) of the scratch's alpha -- `light` the keywords of lighting.distant /
        point / spot, `color` linear.  The two images are distinct; `dst_id` ends opaque."""
        self.turbulence(scratch_id, base_frequency, octaves, seed, kind, stitch_tile, origin)
        self.lighting(scratch_id, dst_id, kind=LightKind.DIFFUSE, surface_scale=surface_scale, constant=kd, color=color, **light)

    def displace(self, src_id, map_id, dst_id, scale, x_channel=DisplaceChannel.R, y_channel=DisplaceChannel.G, matrix=AFFINE_IDENTITY,
                 filter=WarpFilter.BILINEAR, edge=WarpEdge.ZERO, src_rect=None, dst_rect=None, premultiplied=True):
        """jh_displace: feDisplacementMap (the rule: DESIGN.md 5.17) -- warp() of the RGBA16F image `src_id` into the RGBA16F image
        `dst_id` (another image) with every destination texel's source position moved by `scale` x (m - 0.5), m the `x_channel`
        (`y_channel`) of the texel at the same place of the RGBA16F image `map_id`, which has dst's size; the map's channels are
        read as stored (un-premultiplied).  `scale` is in texels of the source rectangle, one number or (x, y).  `matrix`, `filter`,
        `edge`, `src_rect`, `dst_rect` and `premultiplied` are warp()'s; the identity is what the specification's primitive needs,
        and under another matrix the displacement is added after the affine map, in source space.  `map_id` may be `dst_id`
        (noise generated into dst and displaced over in place: distort()) or `src_id`.  One launch, no scratch: always
        capturable.  Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _displace_desc(scale, x_channel, y_channel, matrix, filter, edge, src_rect, dst_rect, premultiplied)
        self._check(self.hip.jh_displace(self.ctx, src_id, map_id, dst_id, ctypes.byref(d)), "displace", invalid=ValueError)

    def distort(self, src_id, dst_id, scale, x_channel=DisplaceChannel.R, y_channel=DisplaceChannel.G, filter=WarpFilter.BILINEAR,
                edge=WarpEdge.ZERO, premultiplied=True, **turbulence_keywords):
        """The specification's usual pair (heat haze, ripples, a roughened edge) as two calls on RGBA16F images of one size:
        turbulence(dst, **turbulence_keywords) -- `base_frequency` among them -- then displace(src, map = dst, dst, scale, ...): the
        noise is the map and is overwritten texel by texel as it is used, so no third image is needed.  `src_id` is another image
        than `dst_id`."""
        self.turbulence(dst_id, **turbulence_keywords)
        self.displace(src_id, dst_id, dst_id, scale, x_channel, y_channel, filter=filter, edge=edge, premultiplied=premultiplied)

    def shadow(self, dst_id, box, radius, sigma, color, matrix=None, rect=None, over=False, invert=False):
        """jh_shadow: the Gaussian blur of the rounded rectangle `box` = (x0, y0, x1, y1) with corner radius `radius` (clamped to
        half the smaller side) by `sigma`, times `color` = (r, g, b, a), premultiplied and linear, GENERATED into the RGBA16F image
        `dst_id` (the rule: DESIGN.md 5.18) -- no source image, no scratch, one launch whose cost does not depend on sigma.  `matrix`
        = (a, b, c, d, e, f) takes the shape's space to dst's texel space (None: the identity); the blur lives in shape space, so
        a rotated box has a rotated shadow and a non-uniform scale an anisotropic blur.  `rect` = (x, y, width, height) is the
        rectangle of dst that is written (None: the whole image; shadow_bounds gives the one outside which there is no shadow).
        `over`: the shadow is laid over what dst holds, in place (Normal + SrcOver, exactly composite()'s); `invert`: the coverage
        is 1 - S (inset shadows).  Always capturable.  Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _shadow_desc(box, radius, sigma, color, matrix, rect, over, invert)
        self._check(self.hip.jh_shadow(self.ctx, dst_id, ctypes.byref(d)), "shadow", invalid=ValueError)

    def box_shadow(self, target, box, radius, sigma, offset, spread, color, matrix=None):
        """CSS box-shadow of the border box `box` = (x0, y0, x1, y1) with corner radius `radius` onto `target` = (image id, width,
        height) -- or the dict a Recording's .target is -- in ONE call: the box shifted by `offset` = (dx, dy) and grown by `spread`
        (box_shadow_geometry), blurred by `sigma` (CSS's blur radius is 2 sigma), laid over the target (shadow(over=True)) inside
        shadow_bounds' rectangle only.  Returns that rectangle; nothing is enqueued when it is empty.  It is drop_shadow() for the
        shape whose blur has a closed form; a layer of any other shape goes through drop_shadow()."""
        tid, width, height = (target["id"], target["width"], target["height"]) if isinstance(target, dict) else target
        shape, r = box_shadow_geometry(box, radius, offset, spread)
        rect = shadow_bounds(shape, r, sigma, (width, height), matrix)
        if rect[2] == 0 or rect[3] == 0:
            return rect
        self.shadow(tid, shape, r, sigma, color, matrix, rect, over=True)
        return rect

    def place_layer(self, layer_id, target_id, matrix, scratch_image_id, layer_size, target_size, filter=WarpFilter.BILINEAR, **composite_keywords):
        """A cached layer onto a target under an affine transform, two calls: warp(layer -> scratch, edge ZERO, dst_rect =
        warp_bounds(...)): the layer in target space, written only where it can be other than transparent black;
        composite(scratch -> target, src_rect = that rectangle, offset = its corner, **composite_keywords).  `layer_size` and
        `target_size` are (width, height) of the layer and of the target; the scratch is an RGBA16F image of the target's size (the
        rectangle of it is overwritten).  Returns the rectangle; nothing is enqueued when it is empty."""
        for k in ("src_rect", "offset"):
            if k in composite_keywords:
                raise ValueError("place_layer: %s is the placed rectangle's" % k)
        rect = warp_bounds(matrix, layer_size, filter, target_size)
        if rect[2] == 0 or rect[3] == 0:
            return rect
        self.warp(layer_id, scratch_image_id, matrix, filter=filter, edge=WarpEdge.ZERO, dst_rect=rect)
        self.composite(scratch_image_id, target_id, src_rect=rect, offset=(rect[0], rect[1]), **composite_keywords)
        return rect

    def perspective(self, src_id, dst_id, matrix, filter=WarpFilter.BILINEAR, edge=WarpEdge.ZERO, src_rect=None, dst_rect=None, premultiplied=True):
        """jh_perspective: warp() under a projective map (the rule: DESIGN.md 5.19).  `matrix` = (a, b, p, c, d, q, e, f, s), x' w =
        a x + c y + e, y' w = b x + d y + f, w = p x + q y + s, takes continuous coordinates of the source rectangle `src_rect` of the
        RGBA16F image `src_id` to continuous coordinates of the destination IMAGE `dst_id` (another RGBA16F image); `dst_rect` is
        only what gets written.  jello_amd.perspective has the constructors: affine, from_quad, from_matrix3d, rotate_x, rotate_y,
        compose.  A destination texel whose source lies behind the viewer (w <= 0) is transparent black whatever `edge` says.  The
        other arguments are warp()'s.  There is no minification prefilter: toward the horizon the result aliases.  One launch, no
        scratch: always capturable.  Stream-ordered, returns nothing; ValueError for a call the rule refuses."""
        d = _perspective_desc(matrix, filter, edge, src_rect, dst_rect, premultiplied)
        self._check(self.hip.jh_perspective(self.ctx, src_id, dst_id, ctypes.byref(d)), "perspective", invalid=ValueError)

    def project_layer(self, layer_id, target_id, matrix, scratch_image_id, layer_size, target_size, filter=WarpFilter.BILINEAR, **composite_keywords):
        """place_layer() under a projective transform, two calls: perspective(layer -> scratch, edge ZERO, dst_rect =
        perspective_bounds(...)): the layer in target space, written only where it can be other than transparent black (the whole
        target when the layer reaches w <= 0); composite(scratch -> target, src_rect = that rectangle, offset = its corner,
        **composite_keywords).  `matrix` has nine entries; the other arguments and the result are place_layer()'s."""
        for k in ("src_rect", "offset"):
            if k in composite_keywords:
                raise ValueError("project_layer: %s is the placed rectangle's" % k)
        rect = perspective_bounds(matrix, layer_size, filter, target_size)
        if rect[2] == 0 or rect[3] == 0:
            return rect
        self.perspective(layer_id, scratch_image_id, matrix, filter=filter, edge=WarpEdge.ZERO, dst_rect=rect)
        self.composite(scratch_image_id, target_id, src_rect=rect, offset=(rect[0], rect[1]), **composite_keywords)
        return rect

    def outline(self, layer_id, target_id, radius, color, scratch_image_id):
        """A layer with an outline (a halo) of `radius` texels onto a target, three calls: morphology(layer -> scratch, DILATE, edge
        ZERO); composite(scratch -> target, tint=color): the grown alpha in the outline's colour; composite(layer -> target).
        `layer_id` and `scratch_image_id` are RGBA16F images of one size (the scratch's content is overwritten), `color` =
        (r, g, b, a)."""
        self.morphology(layer_id, scratch_image_id, op=MorphOp.DILATE, radius=radius, edge=MorphEdge.ZERO)
        self.composite(scratch_image_id, target_id, tint=color)
        self.composite(layer_id, target_id)

    def luminance_mask(self, layer_id, mask_id, scratch_id):
        """`mask-type: luminance`, two calls: color_filter(mask -> scratch, luminance_to_alpha): the mask's luminance becomes the
        scratch's alpha; composite(scratch -> layer, DstIn): the layer is kept where that alpha is.  Three RGBA16F images; the
        scratch is at least as large as the mask and its content is overwritten."""
        from . import colorfilter
        self.color_filter(mask_id, scratch_id, **colorfilter.luminance_to_alpha())
        self.composite(scratch_id, layer_id, compose=Compose.DestIn)

    def drop_shadow(self, layer_id, target_id, width, height, sigma, offset, color, scratch_image_id, spread=0):
        """A layer with its drop shadow onto a target, three calls: blur(layer -> scratch, edge ZERO); composite(scratch -> target,
        tint=color, offset): the blurred alpha in the shadow's colour, shifted; composite(layer -> target).  `layer_id` and
        `scratch_image_id` are RGBA16F images of width x height (the scratch's content is overwritten), `color` = (r, g, b, a).
        `spread` > 0 (a scalar or (rx, ry), CSS box-shadow's spread radius) grows the layer first, four calls: morphology(layer ->
        scratch, DILATE, edge ZERO), then the scratch is blurred in place."""
        if any(int(r) != 0 for r in (spread if isinstance(spread, (tuple, list)) else (spread,))):
            self.morphology(layer_id, scratch_image_id, op=MorphOp.DILATE, radius=spread, edge=MorphEdge.ZERO)
            self.blur(scratch_image_id, width, height, sigma, edge=BlurEdge.ZERO)
        else:
            self.blur(layer_id, width, height, sigma, dst_image_id=scratch_image_id, edge=BlurEdge.ZERO)
        self.composite(scratch_image_id, target_id, tint=color, offset=offset)
        self.composite(layer_id, target_id)

    def _pack_tiles(self, src_ptr, pitch, ref_ptr, ref_pitch, width, height, texel_bytes, dst_ptr, capacity):
        self._check(self.hip.jh_pack_tiles(self.ctx, src_ptr, pitch, ref_ptr, ref_pitch, width, height, texel_bytes, dst_ptr, capacity),
                    "pack_tiles")

    def pack_tiles(self, src_ptr, pitch, width, height, texel_bytes, ref_ptr=None, ref_pitch=None, out_device_ptr=None,
                   out_capacity=None):
        """jh_pack_tiles: the frame at the device pointer `src_ptr` (rows `pitch` bytes apart, texels of 4 or 8 bytes) as a
        tile pack (the format: include/jello_hip.h), against the reference frame at `ref_ptr` if one is given.  Into
        `out_device_ptr` (`out_capacity` bytes, default and at least tilepack.bound(...); stream-ordered, returns None) or,
        without a pointer, downloaded (read_pack) and returned as bytes."""
        bound = int(self.hip.jh_pack_bound(width, height, texel_bytes))
        if out_device_ptr is not None:
            dst, cap = out_device_ptr, (bound if out_capacity is None else out_capacity)
        else:
            cap = max(bound, 32)
            dst = self._own_buffer(_PACK_BUFFER_ID, cap)
        rp = 0 if ref_ptr is None else (pitch if ref_pitch is None else ref_pitch)
        self._pack_tiles(src_ptr, pitch, ref_ptr, rp, width, height, texel_bytes, dst, cap)
        return None if out_device_ptr is not None else self.read_pack(dst, cap)

    def read_pack(self, ptr, capacity):
        """The pack at the device pointer `ptr` as bytes: downloads its 32-byte header, then exactly its total size."""
        out = np.empty(capacity, dtype=np.uint8)
        size = ctypes.c_uint64()
        self._check(self._L.jl_engine_read_pack(self._h, ptr, capacity, out.ctypes.data, capacity, ctypes.byref(size)), "read_pack", host=True)
        return out[:size.value].tobytes()

    def unpack_tiles(self, pack, dst_ptr, pitch, width, height, texel_bytes):
        """jh_unpack_tiles: writes the SOLID and RAW tiles of `pack` into the frame at the device pointer `dst_ptr` and nothing
        else.  `pack` is bytes (uploaded for the caller) or (device pointer, size).  Stream-ordered."""
        if isinstance(pack, (bytes, bytearray, memoryview)):
            data = bytes(pack)
            buf = ctypes.create_string_buffer(data, max(len(data), 1))
            ptr, size = self._own_buffer(_UNPACK_BUFFER_ID, len(data)), len(data)
            self._check(self.hip.jh_upload(self.ctx, _UNPACK_BUFFER_ID, buf, size), "upload")
        else:
            ptr, size = pack
        self._check(self.hip.jh_unpack_tiles(self.ctx, ptr, size, dst_ptr, pitch, width, height, texel_bytes), "unpack_tiles")

    def unpack_rejects(self, reset=False):
        """Entries (a bad header: one) unpack_tiles has ignored since the last reset.  Waits for the stream."""
        n = ctypes.c_uint32(0)
        self._check(self.hip.jh_debug_unpack_rejects(self.ctx, ctypes.byref(n), 1 if reset else 0), "unpack_rejects")
        return n.value

    @staticmethod
    def _dash_job(paths, patterns, offsets):
        """The host arrays of jh_dash for a batch: (elements, descriptors, concatenated patterns), ctypes arrays."""
        if not (len(paths) == len(patterns) == len(offsets)):
            raise ValueError("dash_paths: paths, patterns and offsets differ in length")
        n_els = sum(len(p.els) for p in paths)
        els = (_lib.PathEl * max(n_els, 1))()
        desc = (_lib.CDashPath * max(len(paths), 1))()
        flat = [float(d) for pat in patterns for d in pat]
        dashes = (ctypes.c_double * max(len(flat), 1))(*flat)
        k = d0 = 0
        for i, (path, pat, off) in enumerate(zip(paths, patterns, offsets)):
            desc[i].first_el, desc[i].n_els, desc[i].first_dash, desc[i].n_dash, desc[i].offset = k, len(path.els), d0, len(pat), float(off)
            for kind, pts in path.els:
                els[k].kind = kind
                for j in range(6):
                    els[k].pts[j] = pts[j]
                k += 1
            d0 += len(pat)
        return els, n_els, desc, dashes, len(flat)

    def dash_into(self, paths, patterns, offsets, els_ptr, capacity, index_ptr):
        """jh_dash: the dashes of the batch into caller-owned device memory -- `capacity` elements of 28 bytes at `els_ptr`,
        len(paths) + 1 words at `index_ptr`.  Stream-ordered, returns nothing; ValueError for an input the rule rejects."""
        els, n_els, desc, dashes, n_dashes = self._dash_job(paths, patterns, offsets)
        self._check(self.hip.jh_dash(self.ctx, els, n_els, desc, len(paths), dashes, n_dashes, els_ptr, capacity, index_ptr), "dash_paths",
                    invalid=ValueError)

    def dash_paths(self, paths, patterns, offsets, capacity=None, raw=False):
        """The dashes of every path of the batch (scene.Path objects; one pattern and one offset each), computed on the device
        by the rule of DESIGN.md 5.6: a list of Paths, or with raw=True (elements as a DASH_EL array, the len(paths) + 1
        exclusive offsets).  The element buffer is sized from a bound (or `capacity`) and regrown once from the need the first
        call reports."""
        n_els = sum(len(p.els) for p in paths)
        cap = int(capacity) if capacity is not None else 8 * n_els + 256
        index = np.zeros(len(paths) + 1, dtype=np.uint32)
        index_ptr = self._own_buffer(_DASH_INDEX_BUFFER_ID, index.nbytes)
        for attempt in range(2):
            self.dash_into(paths, patterns, offsets, self._own_buffer(_DASH_ELS_BUFFER_ID, max(cap, 1) * DASH_EL.itemsize), cap, index_ptr)
            self._check(self.hip.jh_download(self.ctx, _DASH_INDEX_BUFFER_ID, index.ctypes.data, 0, index.nbytes), "download")
            if int(index[-1]) <= cap:
                break
            cap = int(index[-1])
        total = int(index[-1])
        els = np.zeros(total, dtype=DASH_EL)
        if total:
            self._check(self.hip.jh_download(self.ctx, _DASH_ELS_BUFFER_ID, els.ctypes.data, 0, els.nbytes), "download")
        if raw:
            return els, index
        from .scene import Path
        out = []
        for i in range(len(paths)):
            p = Path()
            p.els = [(int(e["kind"]), tuple(float(v) for v in e["p"])) for e in els[index[i]:index[i + 1]]]
            out.append(p)
        return out

    def capture(self, recording, out_device_ptr=None, surface=None, pack=None, yuv=None, blur=None, composite=None, resample=None, color=None,
                morphology=None, warp=None, convolve=None, lighting=None, turbulence=None, displace=None, shadow=None, perspective=None, distance=None,
                load_surface=None, load_yuv=None, stats=None, lut3d=None):
        """Capture one dispatch-only replay of `recording` into a hipGraph; returns an opaque handle for replay().
        The recording must have been run once (buffers + scratch exist).  surface=(device pointer, pitch, Surface format)
        appends the blit of the frame's target into that surface (one more kernel launch).
        pack=(src, pitch, ref, ref_pitch, dst, capacity, texel_bytes) appends jh_pack_tiles of the frame-sized image at the
        device pointer `src` -- the surface, or the RGBA16F target -- against `ref` (or None) into `dst` (two more launches);
        a frame of this size must have been packed once eagerly.
        yuv=(planes, YuvLayout, YuvMatrix, YuvRange, YuvTransfer), planes as for blit_yuv, appends the conversion of the
        frame's target into those planes (one more kernel launch).
        blur=dict(sigma=..., edge=..., rect=...) (edge and rect optional, as for blur()) blurs the frame's target in place after
        the render and before the surface, YUV or pack conversion of the same capture (two more launches); a rectangle of this
        size must have been blurred once eagerly.
        composite=dict(src=image id, ...) (the other keywords of composite(), optional) blends that image onto the frame's target
        after the blur and before the surface, YUV or pack conversion of the same capture (one more launch).
        resample=dict(dst=image id, width=..., height=..., ...) (the other keywords of resample(), optional) resizes the frame's
        target into the RGBA16F image `dst` of width x height after the blur and the composite (two more launches); the surface,
        YUV or pack conversion of the same capture then reads that image at its size.  This geometry must have been resampled once
        eagerly, and no other since.
        color=dict(...) (the keywords of color_filter() but the ids, e.g. **colorfilter.grayscale(1)) filters the frame's target
        in place after the blur and the composite and before the resample (one more launch); a filter that needs tables must have
        run once eagerly, and no other such filter since.
        morphology=dict(...) (the keywords of morphology() but the ids) erodes or dilates the frame's target in place, after the
        render and BEFORE the blur (three more launches) -- the order of a shadow with spread; a call of this rectangle size and
        these radii must have run once eagerly.
        warp=dict(dst=image id, width=..., height=..., matrix=..., ...) (the other keywords of warp(), optional) transforms the
        frame's target into the RGBA16F image `dst` of width x height where resample= would resize it (one more launch, nothing to
        run eagerly first); the surface, YUV or pack conversion of the same capture then reads that image at its size.  It is
        exclusive with resample=: giving both is a ValueError before anything is captured.
        convolve=dict(dst=image id, ...) (the other keywords of convolve(), `weights` among them) convolves the frame's target into
        the RGBA16F image `dst` of the target's size after the color filter (one more launch, nothing to run eagerly first); the
        later steps of the same capture -- resample or warp, the surface, YUV or pack conversion -- then read `dst`.
        lighting=dict(dst=image id, ...) (the other keywords of lighting()) lights the alpha of the frame's target into the RGBA16F
        image `dst` of the target's size after the color filter and BEFORE the convolve (one more launch); lighting whose exponents
        need tables must have run once eagerly, and no other such since.  The later steps -- convolve, resample or warp, the
        conversion -- then read `dst`.  So the order of a capture is: render, morphology, blur, composite, color, lighting, convolve,
        resample or warp, then the surface, YUV or pack conversion.
        turbulence=dict(dst=image id, ...) (the other keywords of turbulence(), `base_frequency` among them) generates noise into the
        RGBA16F image `dst` right after the frame and before every other step (one more launch), so that composite=dict(src=dst, ...)
        of the same capture can lay it over the frame; the frame's target stays what the later steps read.  Turbulence with this seed
        must have run once eagerly, and none with another seed since.
        displace=dict(map=image id, dst=image id, width=..., height=..., scale=..., ...) (the other keywords of displace(),
        optional) displaces the frame's target into the RGBA16F image `dst` of width x height by the RGBA16F image `map` of that
        size where warp= would transform it (one more launch, nothing to run eagerly first); the conversion of the same capture
        then reads `dst`.  It is exclusive with resample= and with warp=.  It runs after turbulence=, so one capture can make the
        map (turbulence=dict(dst=m, ...)) and use it (displace=dict(map=m, ...)); `map` may be `dst`.
        shadow=dict(box=..., radius=..., sigma=..., color=..., ...) (the other keywords of shadow(), optional; dst=image id: another
        image than the frame's target) draws a blurred rounded rectangle right after turbulence= and before every other step (one
        more launch, nothing to run eagerly first) -- with over=True onto the frame's target, which the later steps then read.
        perspective=dict(dst=image id, width=..., height=..., matrix=..., ...) (the other keywords of perspective(), optional; the
        matrix has nine entries) transforms the frame's target into the RGBA16F image `dst` of width x height where warp= would (one
        more launch, nothing to run eagerly first); the conversion of the same capture then reads `dst`.  It is exclusive with
        resample=, warp= and displace=.
        distance=dict(...) (the keywords of distance() but the ids) turns the frame's target into its distance field in place, after
        the morphology and before the blur (two more launches); a call whose planes are no smaller (distance_plan's scratch_bytes)
        must have run once eagerly.
        load_surface=dict(dst=image id, pixels=device pointer, fmt=..., ...) and load_yuv=dict(dst=image id, planes=[(device pointer,
        pitch)], ...) (the other keywords of load_surface() and load_yuv(), optional; device memory only: a capture cannot upload)
        convert a frame into the RGBA16F image `dst` right after the frame and before turbulence= (one more launch each, nothing to
        run eagerly first), so that composite=dict(src=dst, ...) of the same capture lays the loaded frame over the rendered one.  The
        graph holds the pointers: a replay converts what they hold then.
        stats=dict(out=device pointer, ...) (the other keywords of stats() but the id, optional) writes the record of the frame's
        target -- as it is after the render and after the other image keywords of the same capture that work on it in place; the
        target itself, not the image a lighting=, convolve=, resample=, warp=, displace= or perspective= wrote -- into `out` on every
        replay, before the surface, YUV or pack conversion (two more launches); one stats() call must have run once eagerly.
        lut3d=dict(lut=image id, ...) (the other keywords of lut3d() but the ids, optional) puts the frame's target through that
        table in place, right after color= and before lighting= (one more launch, nothing to run eagerly first)."""
        for name, step, key in (("load_surface", load_surface, "pixels"), ("load_yuv", load_yuv, "planes")):
            if step is None:
                continue
            if "dst" not in step or key not in step:
                raise ValueError("capture: %s= needs dst= and %s=" % (name, key))
            if isinstance(step[key], np.ndarray) or (key == "planes" and any(isinstance(p, np.ndarray) for p in step[key])):
                raise ValueError("capture: %s= takes device memory, not arrays (a capture cannot upload)" % name)
        if sum(step is not None for step in (resample, warp, displace, perspective)) > 1:
            raise ValueError("capture: resample=, warp=, displace= and perspective= are exclusive (each would feed the conversion)")
        if stats is not None and stats.get("out") is None:
            raise ValueError("capture: stats= needs out=, a device pointer (a capture cannot wait for a record)")
        self._check(self.hip.jh_graph_begin(self.ctx), "graph_begin")
        try:
            self.run(recording, RUN_DISPATCHES, out_device_ptr)
            t = recording.target
            if load_surface is not None:
                self.load_surface(load_surface["dst"], **{k: v for k, v in load_surface.items() if k != "dst"})
            if load_yuv is not None:
                self.load_yuv(load_yuv["dst"], **{k: v for k, v in load_yuv.items() if k != "dst"})
            if turbulence is not None:
                self.turbulence(turbulence["dst"], **{k: v for k, v in turbulence.items() if k != "dst"})
            if shadow is not None:
                self.shadow(shadow.get("dst", t["id"]), **{k: v for k, v in shadow.items() if k != "dst"})
            if morphology is not None:
                self.morphology(t["id"], **morphology)
            if distance is not None:
                self.distance(t["id"], **distance)
            if blur is not None:
                self.blur(t["id"], t["width"], t["height"], blur["sigma"], edge=blur.get("edge", BlurEdge.ZERO), rect=blur.get("rect"))
            if composite is not None:
                self.composite(composite["src"], t["id"], **{k: v for k, v in composite.items() if k != "src"})
            if color is not None:
                self.color_filter(t["id"], **color)
            if lut3d is not None:
                self.lut3d(t["id"], lut3d["lut"], **{k: v for k, v in lut3d.items() if k != "lut"})
            if lighting is not None:
                self.lighting(t["id"], lighting["dst"], **{k: v for k, v in lighting.items() if k != "dst"})
                t = {"id": lighting["dst"], "width": t["width"], "height": t["height"]}
            if convolve is not None:
                self.convolve(t["id"], convolve["dst"], **{k: v for k, v in convolve.items() if k != "dst"})
                t = {"id": convolve["dst"], "width": t["width"], "height": t["height"]}
            if resample is not None:
                self.resample(t["id"], resample["dst"], **{k: v for k, v in resample.items() if k not in ("dst", "width", "height")})
                t = {"id": resample["dst"], "width": resample["width"], "height": resample["height"]}
            if warp is not None:
                self.warp(t["id"], warp["dst"], warp["matrix"], **{k: v for k, v in warp.items() if k not in ("dst", "width", "height", "matrix")})
                t = {"id": warp["dst"], "width": warp["width"], "height": warp["height"]}
            if displace is not None:
                self.displace(t["id"], displace["map"], displace["dst"], displace["scale"],
                              **{k: v for k, v in displace.items() if k not in ("map", "dst", "width", "height", "scale")})
                t = {"id": displace["dst"], "width": displace["width"], "height": displace["height"]}
            if perspective is not None:
                self.perspective(t["id"], perspective["dst"], perspective["matrix"],
                                 **{k: v for k, v in perspective.items() if k not in ("dst", "width", "height", "matrix")})
                t = {"id": perspective["dst"], "width": perspective["width"], "height": perspective["height"]}
            if stats is not None:
                self.stats(recording.target["id"], out_device_ptr=stats["out"], **{k: v for k, v in stats.items() if k != "out"})
            if surface is not None:
                ptr, pitch, fmt = surface
                self._blit(t["id"], ptr, pitch, t["width"], t["height"], fmt)
            if yuv is not None:
                planes, layout, matrix, rng, transfer = yuv
                d, _ = self._yuv_desc(t["width"], t["height"], layout, matrix, rng, transfer, planes)
                self._blit_yuv(t["id"], t["width"], t["height"], d)
            if pack is not None:
                src, spitch, ref, rpitch, dst, cap, tb = pack
                self._pack_tiles(src, spitch, ref, rpitch or 0, t["width"], t["height"], tb, dst, cap)
        finally:
            g = ctypes.c_void_p()
            rc = self.hip.jh_graph_end(self.ctx, ctypes.byref(g))
        self._check(rc, "graph_end")
        return g

    def replay(self, graph):
        self._check(self.hip.jh_graph_launch(self.ctx, graph), "graph_launch")

    def graph_node_counts(self, graph):
        """(kernel launches, other nodes) of one replay of a captured frame."""
        k, o = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self.hip.jh_graph_node_counts(self.ctx, graph, ctypes.byref(k), ctypes.byref(o)), "graph_node_counts")
        return k.value, o.value

    def graph_destroy(self, graph):
        self.hip.jh_graph_destroy(self.ctx, graph)

    def sync(self):
        self._check(self.hip.jh_sync(self.ctx), "sync")

    def scratch_bytes(self, slot=-1):
        """Capacity of the context's internal scratch arrays (all of them, or one slot)."""
        return int(self.hip.jh_debug_scratch_bytes(self.ctx, slot))

    def trim_scratch(self):
        """Frees the internal scratch arrays (they only grow): after a frame much larger than the ones to come."""
        if hasattr(self.hip, "jh_scratch_trim"):  # (an older library under JELLO_HIP_LIB, tools/lab.py kstats: nothing to give back)
            self._check(self.hip.jh_scratch_trim(self.ctx), "scratch_trim")

    def set_stream(self, stream_ptr):
        self._check(self.hip.jh_set_stream(self.ctx, stream_ptr), "set_stream")

    def clear(self, buf_id, offset=0, size=-1):
        self._check(self.hip.jh_clear(self.ctx, buf_id, offset, size), "clear")

    def set_band(self, bin_row0=0, bin_row1=0xffffffff):
        """Band mode (sharding.band_for_rank): write the PTCL and rasterise only the bin rows [bin_row0, bin_row1);
        no arguments = the whole target."""
        self._check(self.hip.jh_set_band(self.ctx, int(bin_row0), int(bin_row1)), "set_band")

    def download(self, buf_id, nbytes=None, offset=0, dtype=np.uint8):
        size = self.hip.jh_buffer_size(self.ctx, buf_id)
        if nbytes is None:
            nbytes = size - offset
        out = np.empty(nbytes, dtype=np.uint8)
        self._check(self.hip.jh_download(self.ctx, buf_id, out.ctypes.data, offset, nbytes), "download")
        return out.view(dtype)

    def upload_image(self, image_id, array, fmt=ImageFormat.RGBA16_FLOAT):
        """jh_image_upload: the (H, W, 4) `array` of texels in the ImageFormat `fmt` as the image `image_id`, created or replaced."""
        a = np.ascontiguousarray(array)
        self._check(self.hip.jh_image_upload(self.ctx, image_id, a.shape[1], a.shape[0], int(fmt), a.ctypes.data, a.nbytes), "image_upload")

    def create_image(self, image_id, width, height, fmt):
        """jh_image_create: the image `image_id` of width x height texels in the ImageFormat `fmt`, without content."""
        self._check(self.hip.jh_image_create(self.ctx, image_id, width, height, int(fmt)), "image_create")

    def free_image(self, image_id):
        """jh_image_free."""
        self._check(self.hip.jh_image_free(self.ctx, image_id), "image_free")

    def download_image(self, img_id, width, height):
        out = np.empty((height, width, 4), dtype=np.uint16)
        self._check(self.hip.jh_image_download(self.ctx, img_id, out.ctypes.data, out.nbytes), "image_download")
        return out

    def profile(self, on=True):
        self.hip.jh_profile_enable(self.ctx, 1 if on else 0)

    def profile_collect(self, max_records=4096):
        arr = (CProfileRecord * max_records)()
        n = self.hip.jh_profile_collect(self.ctx, arr, max_records)
        if n < 0:
            self._check(n, "profile_collect")
        return [(STAGE_NAMES[arr[i].stage], arr[i].ms) for i in range(n)]

    def profile_collect_tree(self, max_nodes=1 << 16):
        """Profiler.Collect (profiler.go:337-385): list of dicts {kind, parent, stage, label, cpu_start_ms, cpu_end_ms,
        gpu_start_ms, gpu_end_ms}; a node's parent precedes it."""
        arr = (CProfileNode * max_nodes)()
        n = self.hip.jh_profile_collect_tree(self.ctx, arr, max_nodes)
        if n < 0:
            self._check(n, "profile_collect_tree")
        return [{"kind": "group" if arr[i].kind == 0 else "query", "parent": arr[i].parent, "stage": arr[i].stage,
                 "label": arr[i].label.decode(), "cpu_start_ms": arr[i].cpu_start_ms, "cpu_end_ms": arr[i].cpu_end_ms,
                 "gpu_start_ms": arr[i].gpu_start_ms, "gpu_end_ms": arr[i].gpu_end_ms} for i in range(n)]

    def profile_group(self, label):
        """Context manager: ProfilerGroup.Nest(label) ... End()."""
        eng = self

        class _G:
            def __enter__(self_inner):
                eng._check(eng.hip.jh_profile_group_begin(eng.ctx, label.encode()), "profile_group_begin")

            def __exit__(self_inner, *a):
                eng._check(eng.hip.jh_profile_group_end(eng.ctx), "profile_group_end")
        return _G()

    def debug_poison_scratch(self, byte=0xA5):
        """jh_debug_poison_scratch: scratch memory as a fresh, non-zero allocation would be (tests only)."""
        rc = self.hip.jh_debug_poison_scratch(self.ctx, int(byte))
        if rc != 0:
            raise RuntimeError("jh_debug_poison_scratch failed: %d" % rc)

    def graph_self_cleans(self):
        """Replays that found one of the internal counters dirty (failed frame, poisoned scratch) and zeroed it first."""
        return int(self.hip.jh_debug_graph_self_cleans(self.ctx))

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cus, mem = ctypes.c_int(), ctypes.c_uint64()
        self.hip.jh_device_info(self.ctx, name, 256, ctypes.byref(cus), ctypes.byref(mem))
        return {"name": name.value.decode(), "compute_units": cus.value, "total_mem": mem.value}
