// jello_frame.h -- what a frame is, for the calls that write one (jh_blit, jh_blit_yuv: DESIGN.md 5.3, 5.5) and the calls that read one
// (jh_load_surface, jh_load_yuv: 5.21).  Compiled by the library, the four launchers (kernels_surface.hip, kernels_yuv.hip,
// kernels_load.hip), the load rule (jello_load.h) and the stand-alone check (tools/load_check.cpp).  Every *_error is nullptr for "legal".
//   surface   rows of 4 * width bytes, `pitch` apart, in one of the four jh_surface_format
//   4:2:0     plane 0 = Y, width bytes to a row; NV12: plane 1 = (Cb, Cr) pairs, 2 ceil(width / 2) bytes, plane 2 ignored; I420: planes
//             1, 2 = Cb, Cr, ceil(width / 2) bytes each; chroma planes have ceil(height / 2) rows.  Any pitch >= the row's bytes.
// Which fault a call names first is the call's: jh_blit_yuv walks plane by plane (null, then pitch); the loads refuse every null plane
// before their rectangle and the pitches after it, against its width -- jframe_yuv_planes_error takes the faults to look for.
#pragma once
#include <stdint.h>

#include "jello_hip.h"

#if defined(__HIPCC__)
#define JFRAME_HD __host__ __device__ __forceinline__
#else
#define JFRAME_HD static inline
#endif

JFRAME_HD uint32_t jframe_clamp8(int32_t v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
JFRAME_HD bool jframe_surface_format_ok(int format) { return format >= JH_SURFACE_RGBA8_UNORM && format <= JH_SURFACE_BGRA8_SRGB; }
JFRAME_HD bool jframe_surface_srgb(int format) { return format == JH_SURFACE_RGBA8_SRGB || format == JH_SURFACE_BGRA8_SRGB; }
JFRAME_HD bool jframe_surface_bgra(int format) { return format == JH_SURFACE_BGRA8_UNORM || format == JH_SURFACE_BGRA8_SRGB; }
static inline const char* jframe_surface_format_error(int format) { return jframe_surface_format_ok(format) ? nullptr : "unknown surface format"; }
static inline const char* jframe_surface_pitch_error(uint64_t pitch, uint32_t width) { return pitch < 4ull * width ? "pitch below 4 * width" : nullptr; }

// The first illegal value of the four.
static inline const char* jframe_yuv_enums_error(int layout, int matrix, int range, int transfer) {
    if (layout != JH_YUV_NV12 && layout != JH_YUV_I420) return "unknown layout";
    if (matrix != JH_YUV_BT601 && matrix != JH_YUV_BT709) return "unknown matrix";
    if (range != JH_YUV_LIMITED && range != JH_YUV_FULL) return "unknown range";
    if (transfer != JH_YUV_TRANSFER_NONE && transfer != JH_YUV_TRANSFER_SRGB) return "unknown transfer";
    return nullptr;
}
static inline uint64_t jframe_chroma_extent(uint32_t n) { return ((uint64_t)n + 1u) / 2u; }  // ceil(n / 2)
static inline int jframe_yuv_planes(int layout) { return layout == JH_YUV_NV12 ? 2 : 3; }
static inline uint64_t jframe_yuv_row_bytes(int layout, int i, uint32_t width) {  // of a row of plane i of a frame `width` texels wide
    return i == 0 ? width : (layout == JH_YUV_NV12 ? 2u : 1u) * jframe_chroma_extent(width);
}
static inline bool jframe_plane_null(const void* plane) { return plane == nullptr; }
static inline bool jframe_pitch_short(int layout, int i, uint64_t pitch, uint32_t width) { return pitch < jframe_yuv_row_bytes(layout, i, width); }
// The first fault among `faults` of the planes a (legal) layout uses, plane by plane and null before pitch.
enum { JFRAME_NULL_PLANE = 1, JFRAME_SHORT_PITCH = 2 };
static inline const char* jframe_yuv_planes_error(int layout, const void* const* planes, const uint64_t* pitches, uint32_t width, int faults) {
    for (int i = 0; i < jframe_yuv_planes(layout); i++) {
        if ((faults & JFRAME_NULL_PLANE) && jframe_plane_null(planes[i])) return "null plane";
        if ((faults & JFRAME_SHORT_PITCH) && jframe_pitch_short(layout, i, pitches[i], width)) return "pitch below the row's bytes";
    }
    return nullptr;
}
