// jello_displace.h -- the host half of the displacement rule (DESIGN.md 5.17 "Displacement rule"): which descriptor is legal and the
// offset one map value gives.  Compiled by the library (jello_amd/csrc/jello_hip.cpp: jh_displace), by the kernels
// (jello_amd/csrc/kernels_displace.hip: jdisp_offset is the one text the device, the library and the stand-alone check compile), by
// the query both libraries compile (include/jello_queries.h: jq_displace_offset) and by tools/displace_check.cpp; tests/displace_ref.py restates it.
// The matrix, the plan, the taps and the index rules are include/jello_warp.h's, unchanged.
//
//   map       m = the stored f16 of the chosen channel of the MAP's texel (X, Y), widened to binary32 (exact); un-premultiplied.
//   offset    t = m - 0.5f: exact for every finite f16 (m is a multiple of 2^-24 below 2^16, so is t, and it has at most 24
//             significant bits: below one half in magnitude m spans 2^-1 .. 2^-24, above it m's 11 bits and the one half span at
//             most 18).  d = scale t, one binary32 product.  A NaN d (a NaN m, 0 x Inf) counts as +0; otherwise d is clamped to
//             [-2^22, 2^22] (an infinite d too).  D = (int64) rint(d 2^32), ties to even: the scaling by a power of two is exact (no
//             overflow: 2^54; a subnormal d only grows), and a binary32 of 2^23 and above is an integer already, so is the conversion.
//   position  U = P (2 X + 1) + Q (2 Y + 1) + R + Dx, V = S (2 X + 1) + T (2 Y + 1) + W + Dy: |U| < 2^55 + 2^54 < 2^56.
#pragma once
#include <math.h>
#include <stdint.h>

#include "jello_color.h"  // jcolor_f16_value: the value of an f16 bit pattern
#include "jello_warp.h"

#if defined(__HIPCC__)
#define JDISP_HD __host__ __device__ __forceinline__
#else
#define JDISP_HD static inline
#endif

#define JDISP_R 0
#define JDISP_G 1
#define JDISP_B 2
#define JDISP_A 3
#define JDISP_CHANNELS 4
#define JDISP_STRAIGHT JWARP_STRAIGHT
#define JDISP_MAX_OFFSET 4194304.0f  /* |d|: 2^22 texels of the source rectangle */

static inline bool jdisp_channel_ok(int channel) { return channel >= 0 && channel < JDISP_CHANNELS; }

// The value of an f16 bit pattern as binary32, exactly (a NaN is some NaN): on the host the table headers' widening, on the device the
// hardware's conversion (jd::f16_to_f32 of dmath.h), which is exact too.
JDISP_HD float jdisp_f16(uint16_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    union { uint16_t u; _Float16 f; } c;
    c.u = bits;
    return (float)c.f;
#else
    return (float)jcolor_f16_value(bits);
#endif
}

// D of one axis: the displacement, in units of 2^-32 texel of the source rectangle, that the map value `f16_bits` gives under `scale`.
JDISP_HD int64_t jdisp_offset(float scale, uint16_t f16_bits) {
    const float t = jdisp_f16(f16_bits) - 0.5f;
    float d = scale * t;
    if (d != d) d = 0.0f;
    d = d < -JDISP_MAX_OFFSET ? -JDISP_MAX_OFFSET : (d > JDISP_MAX_OFFSET ? JDISP_MAX_OFFSET : d);
    return (int64_t)__builtin_rintf(d * 4294967296.0f);
}

// nullptr for a legal descriptor between a src_w x src_h source, a map_w x map_h map and a dst_w x dst_h destination (the matrix apart:
// jwarp_plan; the rectangles apart: jimage_rect_check), else what is wrong with it (jh_displace puts "jh_displace: " in front).
static inline const char* jdisp_desc_error(int filter, int edge, uint32_t flags, float scale_x, float scale_y, int x_channel, int y_channel, uint32_t src_w,
                                           uint32_t src_h, uint32_t map_w, uint32_t map_h, uint32_t dst_w, uint32_t dst_h) {
    if (const char* why = jwarp_desc_error(filter, edge, flags, src_w, src_h, dst_w, dst_h)) return why;
    if (!jdisp_channel_ok(x_channel) || !jdisp_channel_ok(y_channel)) return "a channel outside 0..3";
    if (!isfinite(scale_x) || !isfinite(scale_y)) return "a scale is not finite";
    if (map_w != dst_w || map_h != dst_h) return "the map's size is not the destination's";
    return nullptr;
}
