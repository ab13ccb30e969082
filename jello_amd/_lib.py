"""Locating, building and loading the native libraries (ctypes).

The product path fails loudly if the HIP extension is missing: there is no CPU fallback anywhere in
this package.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


class HostLibraryMissing(RuntimeError):
    pass


def lib_paths():
    # JELLO_HIP_LIB: an experiment library built with `make -C jello_amd/csrc VARIANT=...` (tools/ only; the tests and
    # bench.py's default run never set it)
    return {
        "hip": os.environ.get("JELLO_HIP_LIB") or os.path.join(_HERE, "libjello_hip.so"),
        # JELLO_HOST_LIB: the sanitizer build of tools/sanitize_cpu.sh (CPU suite under ASan / UBSan)
        "host": os.environ.get("JELLO_HOST_LIB") or os.path.join(_HERE, "libjello_host.so"),
    }


def build(verbose=False):
    """Compile every HIP extension for gfx950 (hipcc cross-compiles without a GPU) and the host lib."""
    for sub in ("csrc", "host"):
        cmd = ["make", "-C", os.path.join(_HERE, sub), "-j8"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if verbose or r.returncode != 0:
            print(r.stdout)
        if r.returncode != 0:
            raise RuntimeError("build failed in jello_amd/%s" % sub)
    return lib_paths()


_host = None


def load_host():
    """Load libjello_host.so (which pulls in libjello_hip.so through its rpath)."""
    global _host
    if _host is not None:
        return _host
    p = lib_paths()
    for k in ("hip", "host"):
        if not os.path.exists(p[k]):
            raise HostLibraryMissing(
                "%s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the render path)" % p[k])
    ctypes.CDLL(p["hip"], mode=ctypes.RTLD_GLOBAL)
    _host = ctypes.CDLL(p["host"])
    _declare(_host)
    return _host


# ---- ctypes mirrors of the structs in host/capi.cpp ----
class PathEl(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("pad", ctypes.c_int32), ("pts", ctypes.c_double * 6)]


class CColorStop(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_float), ("pad", ctypes.c_float), ("rgba", ctypes.c_double * 4)]


class CBrush(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32), ("extend", ctypes.c_int32), ("color", ctypes.c_double * 4),
        ("p0", ctypes.c_double * 2), ("p1", ctypes.c_double * 2),
        ("r0", ctypes.c_float), ("r1", ctypes.c_float), ("t0", ctypes.c_float), ("t1", ctypes.c_float),
        ("stops", ctypes.POINTER(CColorStop)), ("n_stops", ctypes.c_int32),
        ("image_width", ctypes.c_uint32), ("image_height", ctypes.c_uint32),
        ("image_pixels", ctypes.c_void_p), ("image_key", ctypes.c_uint64),
    ]


class CStroke(ctypes.Structure):
    _fields_ = [("width", ctypes.c_double), ("join", ctypes.c_int32), ("start_cap", ctypes.c_int32),
                ("end_cap", ctypes.c_int32), ("pad", ctypes.c_int32), ("miter_limit", ctypes.c_double),
                ("dash_pattern", ctypes.POINTER(ctypes.c_double)), ("n_dash", ctypes.c_int32), ("pad2", ctypes.c_int32),
                ("dash_offset", ctypes.c_double)]


class CBumpSizes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("bin_data", "tiles", "lines", "seg_counts", "segments", "blend_spill", "ptcl")]


class CRenderParams(ctypes.Structure):
    _fields_ = [("base_color", ctypes.c_double * 4), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("aa", ctypes.c_int32), ("pad", ctypes.c_uint32), ("bump", CBumpSizes)]


class CBinding(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("count", ctypes.c_uint32), ("id", ctypes.c_uint64), ("size", ctypes.c_uint64),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("format", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("ids", ctypes.POINTER(ctypes.c_uint64)), ("dims", ctypes.POINTER(ctypes.c_uint32))]


class CCommand(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("shader", ctypes.c_int32), ("wg", ctypes.c_uint32 * 3), ("pad", ctypes.c_uint32),
                ("buf_id", ctypes.c_uint64), ("buf_size", ctypes.c_uint64), ("buf_name", ctypes.c_char_p),
                ("img_id", ctypes.c_uint64), ("img_w", ctypes.c_uint32), ("img_h", ctypes.c_uint32),
                ("img_format", ctypes.c_int32), ("n_bindings", ctypes.c_int32),
                ("data", ctypes.POINTER(ctypes.c_uint8)), ("data_len", ctypes.c_uint64),
                ("offset", ctypes.c_uint64), ("size", ctypes.c_int64), ("bindings", ctypes.POINTER(CBinding)),
                ("coords", ctypes.c_uint32 * 4)]


class CConfig(ctypes.Structure):
    """include/jello_formats.h JlConfig (renderer/config.go ConfigUniform)."""
    _fields_ = [("width_in_tiles", ctypes.c_uint32), ("height_in_tiles", ctypes.c_uint32), ("target_width", ctypes.c_uint32),
                ("target_height", ctypes.c_uint32), ("base_color", ctypes.c_float * 4),
                ("n_drawobj", ctypes.c_uint32), ("n_path", ctypes.c_uint32), ("n_clip", ctypes.c_uint32),
                ("bin_data_start", ctypes.c_uint32), ("pathtag_base", ctypes.c_uint32), ("pathdata_base", ctypes.c_uint32),
                ("drawtag_base", ctypes.c_uint32), ("drawdata_base", ctypes.c_uint32), ("transform_base", ctypes.c_uint32),
                ("style_base", ctypes.c_uint32), ("lines_size", ctypes.c_uint32), ("binning_size", ctypes.c_uint32),
                ("tiles_size", ctypes.c_uint32), ("seg_counts_size", ctypes.c_uint32), ("segments_size", ctypes.c_uint32),
                ("blend_size", ctypes.c_uint32), ("ptcl_size", ctypes.c_uint32)]


class CDashPath(ctypes.Structure):
    """jh_dash_path (include/jello_hip.h)."""
    _fields_ = [("first_el", ctypes.c_uint32), ("n_els", ctypes.c_uint32), ("first_dash", ctypes.c_uint32), ("n_dash", ctypes.c_uint32),
                ("offset", ctypes.c_double)]


class CYuvDesc(ctypes.Structure):
    """jh_yuv_desc (include/jello_hip.h)."""
    _fields_ = [("layout", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32), ("transfer", ctypes.c_int32),
                ("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_uint64 * 3)]


class CBlurDesc(ctypes.Structure):
    """jh_blur_desc (include/jello_hip.h)."""
    _fields_ = [("sigma_x", ctypes.c_float), ("sigma_y", ctypes.c_float), ("edge", ctypes.c_int32), ("x", ctypes.c_uint32),
                ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32)]


class CCompositeDesc(ctypes.Structure):
    """jh_composite_desc (include/jello_hip.h)."""
    _fields_ = [("mix", ctypes.c_uint32), ("compose", ctypes.c_uint32), ("opacity", ctypes.c_float), ("flags", ctypes.c_uint32),
                ("tint", ctypes.c_float * 4), ("sx", ctypes.c_uint32), ("sy", ctypes.c_uint32), ("sw", ctypes.c_uint32),
                ("sh", ctypes.c_uint32), ("dx", ctypes.c_int32), ("dy", ctypes.c_int32)]


class CResampleDesc(ctypes.Structure):
    """jh_resample_desc (include/jello_hip.h)."""
    _fields_ = [("filter", ctypes.c_int32), ("flags", ctypes.c_uint32), ("src_x", ctypes.c_uint32), ("src_y", ctypes.c_uint32),
                ("src_width", ctypes.c_uint32), ("src_height", ctypes.c_uint32), ("dst_x", ctypes.c_uint32), ("dst_y", ctypes.c_uint32),
                ("dst_width", ctypes.c_uint32), ("dst_height", ctypes.c_uint32)]


class CColorFunc(ctypes.Structure):
    """jh_color_func (include/jello_hip.h)."""
    _fields_ = [("type", ctypes.c_int32), ("n", ctypes.c_uint32), ("slope", ctypes.c_float), ("intercept", ctypes.c_float),
                ("amplitude", ctypes.c_float), ("exponent", ctypes.c_float), ("offset", ctypes.c_float), ("values", ctypes.c_float * 64)]


class CColorDesc(ctypes.Structure):
    """jh_color_desc (include/jello_hip.h)."""
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("matrix", ctypes.c_float * 20), ("space", ctypes.c_int32), ("flags", ctypes.c_uint32), ("func", CColorFunc * 4)]


class CMorphDesc(ctypes.Structure):
    """jh_morph_desc (include/jello_hip.h)."""
    _fields_ = [("op", ctypes.c_int32), ("edge", ctypes.c_int32), ("flags", ctypes.c_uint32), ("radius_x", ctypes.c_uint32),
                ("radius_y", ctypes.c_uint32), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32)]


class CWarpDesc(ctypes.Structure):
    """jh_warp_desc (include/jello_hip.h)."""
    _fields_ = [("matrix", ctypes.c_double * 6), ("filter", ctypes.c_int32), ("edge", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("src_x", ctypes.c_uint32), ("src_y", ctypes.c_uint32), ("src_width", ctypes.c_uint32), ("src_height", ctypes.c_uint32),
                ("dst_x", ctypes.c_uint32), ("dst_y", ctypes.c_uint32), ("dst_width", ctypes.c_uint32), ("dst_height", ctypes.c_uint32)]


class CConvolveDesc(ctypes.Structure):
    """jh_convolve_desc (include/jello_hip.h)."""
    _fields_ = [("order_x", ctypes.c_uint32), ("order_y", ctypes.c_uint32), ("target_x", ctypes.c_uint32), ("target_y", ctypes.c_uint32),
                ("edge", ctypes.c_int32), ("mode", ctypes.c_int32), ("bias", ctypes.c_float), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("weights", ctypes.c_float * 225)]


class CLightingDesc(ctypes.Structure):
    """jh_lighting_desc (include/jello_hip.h)."""
    _fields_ = [("kind", ctypes.c_int32), ("light", ctypes.c_int32), ("surface_scale", ctypes.c_float), ("constant", ctypes.c_float),
                ("specular_exponent", ctypes.c_float), ("spot_exponent", ctypes.c_float), ("color", ctypes.c_float * 3), ("x", ctypes.c_uint32),
                ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("direction", ctypes.c_double * 3),
                ("position", ctypes.c_double * 3), ("points_at", ctypes.c_double * 3), ("cone_cos", ctypes.c_double)]


class CLightPlan(ctypes.Structure):
    """jh_light_plan (include/jello_hip.h)."""
    _fields_ = [("s", ctypes.c_float * 6), ("ldir", ctypes.c_float * 3), ("p", ctypes.c_float * 3), ("sdir", ctypes.c_float * 3),
                ("cone", ctypes.c_float)]


class CTurbulenceDesc(ctypes.Structure):
    """jh_turbulence_desc (include/jello_hip.h)."""
    _fields_ = [("kind", ctypes.c_int32), ("octaves", ctypes.c_uint32), ("seed", ctypes.c_int32), ("stitch", ctypes.c_int32), ("x", ctypes.c_uint32),
                ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("base_frequency", ctypes.c_double * 2),
                ("tile", ctypes.c_double * 4), ("origin", ctypes.c_double * 2)]


class CTurbPlan(ctypes.Structure):
    """jh_turb_plan (include/jello_hip.h)."""
    _fields_ = [("frequency", ctypes.c_double * 2), ("step", ctypes.c_int64 * 2), ("start", ctypes.c_int64 * 2), ("wrap", ctypes.c_int32 * 2),
                ("width", ctypes.c_int32 * 2), ("max_extent", ctypes.c_uint32 * 2), ("key", ctypes.c_uint32), ("stitched", ctypes.c_uint32)]


class CDisplaceDesc(ctypes.Structure):
    """jh_displace_desc (include/jello_hip.h)."""
    _fields_ = [("matrix", ctypes.c_double * 6), ("filter", ctypes.c_int32), ("edge", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("src_x", ctypes.c_uint32), ("src_y", ctypes.c_uint32), ("src_width", ctypes.c_uint32), ("src_height", ctypes.c_uint32),
                ("dst_x", ctypes.c_uint32), ("dst_y", ctypes.c_uint32), ("dst_width", ctypes.c_uint32), ("dst_height", ctypes.c_uint32),
                ("scale_x", ctypes.c_float), ("scale_y", ctypes.c_float), ("x_channel", ctypes.c_int32), ("y_channel", ctypes.c_int32)]


class CShadowDesc(ctypes.Structure):
    """jh_shadow_desc (include/jello_hip.h)."""
    _fields_ = [("matrix", ctypes.c_double * 6), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("radius", ctypes.c_float), ("sigma", ctypes.c_float), ("box", ctypes.c_float * 4), ("color", ctypes.c_float * 4)]


class CShadowPlan(ctypes.Structure):
    """jh_shad_plan (include/jello_hip.h)."""
    _fields_ = [("m", ctypes.c_int64 * 6), ("centre", ctypes.c_int64 * 2), ("a", ctypes.c_float), ("b", ctypes.c_float), ("radius", ctypes.c_float),
                ("core", ctypes.c_float), ("straight", ctypes.c_float), ("sigma", ctypes.c_float), ("inv_s", ctypes.c_float), ("window", ctypes.c_float),
                ("n", ctypes.c_uint32), ("k", ctypes.c_uint32)]


class CPerspectiveDesc(ctypes.Structure):
    """jh_perspective_desc (include/jello_hip.h)."""
    _fields_ = [("matrix", ctypes.c_double * 9), ("filter", ctypes.c_int32), ("edge", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("src_x", ctypes.c_uint32), ("src_y", ctypes.c_uint32), ("src_width", ctypes.c_uint32), ("src_height", ctypes.c_uint32),
                ("dst_x", ctypes.c_uint32), ("dst_y", ctypes.c_uint32), ("dst_width", ctypes.c_uint32), ("dst_height", ctypes.c_uint32)]


class CDistanceDesc(ctypes.Structure):
    """jh_distance_desc (include/jello_hip.h)."""
    _fields_ = [("channel", ctypes.c_int32), ("threshold", ctypes.c_float), ("which", ctypes.c_int32), ("edge", ctypes.c_int32),
                ("max_distance", ctypes.c_uint32), ("scale", ctypes.c_float), ("offset", ctypes.c_float), ("color", ctypes.c_float * 4),
                ("flags", ctypes.c_uint32), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32)]


class CDistPlan(ctypes.Structure):
    """jh_dist_plan (include/jello_hip.h)."""
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("radius", ctypes.c_uint32),
                ("cap", ctypes.c_uint32), ("planes", ctypes.c_uint32), ("plane_columns", ctypes.c_uint32), ("plane_rows", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("scratch_bytes", ctypes.c_uint64)]


class CStatsDesc(ctypes.Structure):
    """jh_stats_desc (include/jello_hip.h)."""
    _fields_ = [("what", ctypes.c_uint32), ("channel", ctypes.c_int32), ("threshold", ctypes.c_float), ("population", ctypes.c_int32),
                ("transfer", ctypes.c_int32), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32)]


class CStatsRecord(ctypes.Structure):
    """jh_stats_record (include/jello_hip.h)."""
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("what", ctypes.c_uint32),
                ("population", ctypes.c_uint32), ("transfer", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("content_count", ctypes.c_uint32),
                ("bounds", ctypes.c_uint32 * 4), ("population_count", ctypes.c_uint32), ("nan_count", ctypes.c_uint32 * 4),
                ("min_bits", ctypes.c_uint16 * 4), ("max_bits", ctypes.c_uint16 * 4), ("histogram", (ctypes.c_uint32 * 256) * 4)]


class CStatsPlan(ctypes.Structure):
    """jh_stats_plan_t (include/jello_hip.h)."""
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("launches", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("record_bytes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64)]


class CLoadSurfaceDesc(ctypes.Structure):
    """jh_load_surface_desc (include/jello_hip.h)."""
    _fields_ = [("format", ctypes.c_int32), ("alpha", ctypes.c_int32), ("src", ctypes.c_void_p), ("pitch", ctypes.c_uint64), ("x", ctypes.c_uint32),
                ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32)]


class CLoadYuvDesc(ctypes.Structure):
    """jh_load_yuv_desc (include/jello_hip.h)."""
    _fields_ = [("layout", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32), ("transfer", ctypes.c_int32),
                ("chroma", ctypes.c_int32), ("reserved", ctypes.c_int32), ("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_uint64 * 3),
                ("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32)]


class CLut3dDesc(ctypes.Structure):
    """jh_lut3d_desc (include/jello_hip.h)."""
    _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32)]


class CProfileRecord(ctypes.Structure):
    """jh_profile_record (include/jello_hip.h)."""
    _fields_ = [("stage", ctypes.c_int32), ("pad", ctypes.c_uint32), ("ms", ctypes.c_float)]


class CProfileNode(ctypes.Structure):
    """jh_profile_node (include/jello_hip.h)."""
    _fields_ = [("kind", ctypes.c_int32), ("parent", ctypes.c_int32), ("stage", ctypes.c_int32), ("pad", ctypes.c_uint32),
                ("label", ctypes.c_char * 48), ("cpu_start_ms", ctypes.c_double), ("cpu_end_ms", ctypes.c_double),
                ("gpu_start_ms", ctypes.c_float), ("gpu_end_ms", ctypes.c_float)]


def _declare(L):
    vp, ci, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    dp = ctypes.POINTER(ctypes.c_double)
    L.jl_last_error.restype = ctypes.c_char_p
    L.jl_scene_new.restype = vp
    L.jl_scene_free.argtypes = [vp]
    L.jl_scene_reset.argtypes = [vp]
    L.jl_scene_fill.argtypes = [vp, ci, dp, ctypes.POINTER(CBrush), dp, ctypes.POINTER(PathEl), ci]
    L.jl_scene_stroke.argtypes = [vp, ctypes.POINTER(CStroke), dp, ctypes.POINTER(CBrush), dp, ctypes.POINTER(PathEl), ci]
    L.jl_dash_path.restype = ctypes.c_int64
    L.jl_dash_path.argtypes = [ctypes.POINTER(PathEl), ci, dp, ci, ctypes.c_double, ctypes.POINTER(PathEl), ctypes.c_int64]
    L.jl_scene_push_layer.argtypes = [vp, ci, ci, ctypes.c_float, dp, ctypes.POINTER(PathEl), ci]
    L.jl_scene_pop_layer.argtypes = [vp]
    L.jl_scene_append.argtypes = [vp, vp, dp]
    L.jl_scene_apply_transform.argtypes = [vp, dp]
    L.jl_scene_stream.restype = ctypes.c_uint64
    L.jl_scene_stream.argtypes = [vp, ci, ctypes.POINTER(vp)]
    L.jl_scene_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    L.jl_scene_bump_sizes.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp]
    L.jl_scene_bump_sizes_clamped.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32]
    L.jl_scene_bump_sizes_clamped.restype = ctypes.c_uint32
    L.jl_scene_bump_estimate.argtypes = [vp, dp, ctypes.POINTER(ctypes.c_uint32)]
    L.jl_scene_fill_stroke_cubics.argtypes = [vp, ci, dp, dp, dp, dp, ci, ci, ci]
    L.jl_ptcl_stats.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    L.jl_host_new.restype = vp
    L.jl_host_free.argtypes = [vp]
    L.jl_record.restype = vp
    L.jl_record.argtypes = [vp, vp, ctypes.POINTER(CRenderParams), ci]
    L.jl_recording_free.argtypes = [vp]
    L.jl_recording_len.argtypes = [vp]
    L.jl_recording_commands.restype = ctypes.POINTER(CCommand)
    L.jl_recording_commands.argtypes = [vp]
    L.jl_recording_config.restype = ctypes.POINTER(CConfig)
    L.jl_recording_config.argtypes = [vp]
    L.jl_recording_target.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.jl_recording_buffer.restype = ctypes.c_uint64
    L.jl_recording_buffer.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    L.jl_recording_wg_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ci]
    L.jl_engine_new.restype = vp
    L.jl_engine_new.argtypes = [ci]
    L.jl_engine_free.argtypes = [vp]
    L.jl_engine_ctx.restype = vp
    L.jl_engine_ctx.argtypes = [vp]
    L.jl_engine_run.argtypes = [vp, vp, cu, ctypes.c_uint64, vp]
    L.jl_engine_release.argtypes = [vp, vp]
    L.jl_engine_render.restype = vp
    L.jl_engine_render.argtypes = [vp, vp, ctypes.POINTER(CRenderParams), vp, ci, ci, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ci)]
    L.jl_engine_render_to_surface.restype = vp
    L.jl_engine_render_to_surface.argtypes = [vp, vp, ctypes.POINTER(CRenderParams), vp, ctypes.c_uint64, ci, ci,
                                              ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ci)]
    L.jl_engine_render_to_yuv.restype = vp
    L.jl_engine_render_to_yuv.argtypes = [vp, vp, ctypes.POINTER(CRenderParams), ctypes.POINTER(CYuvDesc), ci, ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ci)]
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    L.jl_engine_read_pack.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
    # the context-free queries of the image calls (include/jello_queries.h): jl_<name>, and below jh_<name>, take the same arguments
    queries = {
        "blur_taps": [ctypes.c_float, vp, ctypes.POINTER(u32)],
        "resample_taps": [ci, u32, u32, u32, vp, ctypes.POINTER(u32), ctypes.POINTER(u32)],
        "color_tables": [ctypes.POINTER(CColorDesc), vp, vp, ctypes.POINTER(u32)],
        "warp_plan": [dp, ctypes.POINTER(ctypes.c_int64)],
        "warp_bounds": [dp, u32, u32, ci, u32, u32, ctypes.POINTER(u32)],
        "convolve_weights": [u32, u32, dp, ctypes.c_double, ctypes.POINTER(ctypes.c_float)],
        "lighting_plan": [ctypes.POINTER(CLightingDesc), ctypes.POINTER(CLightPlan)],
        "lighting_tables": [ctypes.POINTER(CLightingDesc), vp, vp, ctypes.POINTER(u32)],
        "turbulence_plan": [ctypes.POINTER(CTurbulenceDesc), ctypes.POINTER(CTurbPlan)],
        "turbulence_tables": [ctypes.POINTER(CTurbulenceDesc), vp, vp],
        "displace_offset": [ctypes.c_float, ctypes.c_uint16, ctypes.POINTER(ctypes.c_int64)],
        "shadow_plan": [ctypes.POINTER(CShadowDesc), ctypes.POINTER(CShadowPlan)],
        "shadow_bounds": [ctypes.POINTER(CShadowDesc), u32, u32, ctypes.POINTER(u32)],
        "perspective_plan": [dp, dp],
        "perspective_bounds": [dp, u32, u32, ci, u32, u32, ctypes.POINTER(u32)],
        "distance_plan": [ctypes.POINTER(CDistanceDesc), u32, u32, ctypes.POINTER(CDistPlan)],
        "stats_plan": [ctypes.POINTER(CStatsDesc), u32, u32, ctypes.POINTER(CStatsPlan)],
        "stats_codes": [ci, u64, vp, vp],
        "load_texel": [ci, ci, u64, vp, vp],
        "load_yuv_codes": [ci, ci, u64, vp, vp, vp, vp],
        "lut3d_identity": [u32, vp],
        "lut3d_texels": [u32, vp, vp, u64, vp],
    }
    for name, argtypes in queries.items():
        getattr(L, "jl_" + name).argtypes = argtypes
    L.jl_composite_clip.argtypes = [u32, u32, u32, u32, u32, u32, ctypes.c_int32, ctypes.c_int32, u32, u32, ctypes.POINTER(u32)]
    # C ABI of libjello_hip.so (include/jello_hip.h), reachable through the same process image
    hip = ctypes.CDLL(lib_paths()["hip"])
    L.hip = hip
    hip.jh_last_error.restype = ctypes.c_char_p
    hip.jh_last_error.argtypes = [vp]
    hip.jh_stage_name.restype = ctypes.c_char_p
    hip.jh_download.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint64]
    hip.jh_upload.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64]
    hip.jh_buffer_create.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64]
    hip.jh_buffer_size.restype = ctypes.c_uint64
    hip.jh_buffer_size.argtypes = [vp, ctypes.c_uint64]
    hip.jh_buffer_device_ptr.restype = vp
    hip.jh_buffer_device_ptr.argtypes = [vp, ctypes.c_uint64]
    hip.jh_image_download.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64]
    hip.jh_image_device_ptr.restype = vp
    hip.jh_image_device_ptr.argtypes = [vp, ctypes.c_uint64]
    hip.jh_image_size.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.jh_sync.argtypes = [vp]
    hip.jh_set_stream.argtypes = [vp, vp]
    hip.jh_set_band.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32]
    hip.jh_profile_enable.argtypes = [vp, ci]
    hip.jh_profile_collect.argtypes = [vp, vp, ci]
    hip.jh_profile_group_begin.argtypes = [vp, ctypes.c_char_p]
    hip.jh_profile_group_end.argtypes = [vp]
    hip.jh_profile_collect_tree.argtypes = [vp, vp, ci]
    hip.jh_image_create.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ci]
    hip.jh_image_upload.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ci, vp, ctypes.c_uint64]
    hip.jh_image_free.argtypes = [vp, ctypes.c_uint64]
    hip.jh_image_import.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint32, ctypes.c_uint32, ci]
    hip.jh_blit.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ci]
    hip.jh_blit_yuv.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(CYuvDesc)]
    hip.jh_pack_bound.restype = u64
    hip.jh_pack_bound.argtypes = [u32, u32, u32]
    hip.jh_pack_tiles.argtypes = [vp, vp, u64, vp, u64, u32, u32, u32, vp, u64]
    hip.jh_unpack_tiles.argtypes = [vp, vp, u64, vp, u64, u32, u32, u32]
    hip.jh_dash.argtypes = [vp, ctypes.POINTER(PathEl), u64, ctypes.POINTER(CDashPath), u32, dp, u64, vp, u64, vp]
    for name, argtypes in queries.items():
        getattr(hip, "jh_" + name).argtypes = argtypes
    hip.jh_blur.argtypes = [vp, u64, u64, u32, u32, ctypes.POINTER(CBlurDesc)]
    hip.jh_composite.argtypes = [vp, u64, u64, ctypes.POINTER(CCompositeDesc)]
    hip.jh_resample.argtypes = [vp, u64, u64, ctypes.POINTER(CResampleDesc)]
    hip.jh_color_filter.argtypes = [vp, u64, u64, ctypes.POINTER(CColorDesc)]
    hip.jh_morphology.argtypes = [vp, u64, u64, ctypes.POINTER(CMorphDesc)]
    hip.jh_warp.argtypes = [vp, u64, u64, ctypes.POINTER(CWarpDesc)]
    hip.jh_convolve.argtypes = [vp, u64, u64, ctypes.POINTER(CConvolveDesc)]
    hip.jh_lighting.argtypes = [vp, u64, u64, ctypes.POINTER(CLightingDesc)]
    hip.jh_turbulence.argtypes = [vp, u64, ctypes.POINTER(CTurbulenceDesc)]
    hip.jh_displace.argtypes = [vp, u64, u64, u64, ctypes.POINTER(CDisplaceDesc)]
    hip.jh_shadow.argtypes = [vp, u64, ctypes.POINTER(CShadowDesc)]
    hip.jh_perspective.argtypes = [vp, u64, u64, ctypes.POINTER(CPerspectiveDesc)]
    hip.jh_distance.argtypes = [vp, u64, u64, ctypes.POINTER(CDistanceDesc)]
    hip.jh_stats.argtypes = [vp, u64, ctypes.POINTER(CStatsDesc), vp]
    hip.jh_load_surface.argtypes = [vp, u64, ctypes.POINTER(CLoadSurfaceDesc)]
    hip.jh_load_yuv.argtypes = [vp, u64, ctypes.POINTER(CLoadYuvDesc)]
    hip.jh_lut3d.argtypes = [vp, u64, u64, u64, ctypes.POINTER(CLut3dDesc)]
    hip.jh_debug_lut3d_variant.argtypes = [vp, ci]
    hip.jh_debug_unpack_rejects.argtypes = [vp, ctypes.POINTER(u32), ci]
    hip.jh_debug_scan_u32.argtypes = [vp, u64, u64, u32, u32, u64, u32, u64, u32]
    hip.jh_image_write.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint64]
    hip.jh_buffer_import.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64]
    hip.jh_graph_begin.argtypes = [vp]
    hip.jh_graph_end.argtypes = [vp, ctypes.POINTER(vp)]
    hip.jh_graph_launch.argtypes = [vp, vp]
    hip.jh_graph_node_counts.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    hip.jh_graph_destroy.argtypes = [vp, vp]
    hip.jh_free.argtypes = [vp, ctypes.c_uint64]
    hip.jh_clear.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64]
    hip.jh_pool_bytes.restype = ctypes.c_uint64
    hip.jh_pool_bytes.argtypes = [vp]
    hip.jh_device_info.argtypes = [vp, ctypes.c_char_p, ci, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_uint64)]
    hip.jh_debug_poison_scratch.argtypes = [vp, ci]
    hip.jh_debug_scratch_bytes.restype = ctypes.c_uint64
    hip.jh_debug_scratch_bytes.argtypes = [vp, ci]
    if hasattr(hip, "jh_debug_flatten_regions"):
        hip.jh_debug_flatten_regions.restype = ci
        hip.jh_debug_flatten_regions.argtypes = [vp, ctypes.c_uint32]
    if hasattr(hip, "jh_scratch_trim"):
        hip.jh_scratch_trim.restype = ci
        hip.jh_scratch_trim.argtypes = [vp]
    hip.jh_set_clip_depth_hint.argtypes = [vp, ctypes.c_uint32]
    if hasattr(hip, "jh_debug_clip_hint_overflows"):  # (an experiment library built from older sources, JELLO_HIP_LIB, may lack it)
        hip.jh_debug_clip_hint_overflows.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    hip.jh_debug_graph_self_cleans.restype = ctypes.c_uint64
    hip.jh_debug_graph_self_cleans.argtypes = [vp]
