// jello_queries.h -- the context-free queries of the image calls: the taps, tables, plans, bounds, weights and offsets a caller can ask
// for without a GPU (documented call by call in jello_hip.h).  Each query has one body here, jq_<name>, over the rule header of its
// call: the null checks, the rule's legality check, the computation, then the optional outputs.  It takes the exported function's
// parameters and returns null for success or the reason of the refusal; on a refusal nothing is written.  Compiled by the library
// (jello_amd/csrc/jello_hip.cpp expands JQ_QUERY_LIST to the jh_<name>, which answer JH_ERR_INVALID without the reason), by the C++
// host twin (jello_amd/host/capi.cpp expands both lists to the jl_<name>, which answer -1 and keep "<name>: <reason>" for
// jl_last_error) and by tools/queries_check.cpp; tests/test_queries.py holds the two libraries against each other (the perspective
// queries: tests/test_perspective_spec.py).
#pragma once
#include <stdint.h>

#include "jello_blur.h"
#include "jello_color.h"
#include "jello_composite.h"
#include "jello_convolve.h"
#include "jello_displace.h"
#include "jello_distance.h"
#include "jello_lighting.h"
#include "jello_load.h"
#include "jello_lut3d.h"
#include "jello_perspective.h"
#include "jello_resample.h"
#include "jello_shadow.h"
#include "jello_stats.h"
#include "jello_turbulence.h"
#include "jello_warp.h"

// jh_blit's sRGB thresholds as a host constant, for jq_stats_codes (a file that includes this one does not include the kernels'
// blit_convert.h, which takes the table as a device constant).
#define JSRGB_ENCODE_TABLE static const
#include "../jello_amd/csrc/srgb_encode_lut.h"
#undef JSRGB_ENCODE_TABLE

static inline const char* jq_blur_taps(float sigma, float* weights, uint32_t* radius) {
    if (!jblur_sigma_ok(sigma)) return "sigma is negative, above 64 or NaN";
    const uint32_t R = jblur_taps(sigma, weights);
    if (radius) *radius = R;
    return nullptr;
}

static inline const char* jq_resample_taps(int filter, uint32_t n_in, uint32_t n_out, uint32_t i, float* weights, uint32_t* first, uint32_t* count) {
    if (!jresample_filter_ok(filter) || !jresample_sizes_ok(n_in, n_out) || i >= n_out)
        return "unknown filter, sizes outside 1 <= n_in <= 16 n_out, or an index outside the axis";
    uint32_t f = 0u;
    const uint32_t n = jresample_taps(filter, n_in, n_out, i, weights, &f, nullptr);
    if (n == 0u) return "a window without taps";
    if (first) *first = f;
    if (count) *count = n;
    return nullptr;
}

static inline const char* jq_color_tables(const jh_color_desc* desc, float* pre, uint16_t* post, uint32_t* which) {
    if (!desc) return "null descriptor";
    if (const char* why = jcolor_desc_error(desc)) return why;
    const uint32_t w = jcolor_tables(desc, pre, post);
    if (which) *which = w;
    return nullptr;
}

static inline const char* jq_warp_plan(const double* matrix, int64_t* plan) {
    if (!matrix || !plan) return "null argument";
    return jwarp_plan(matrix, plan);
}

static inline const char* jq_warp_bounds(const double* matrix, uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h, uint32_t* rect) {
    if (!matrix || !rect) return "null argument";
    return jwarp_bounds(matrix, src_w, src_h, filter, dst_w, dst_h, rect);
}

static inline const char* jq_convolve_weights(uint32_t order_x, uint32_t order_y, const double* kernel_matrix, double divisor, float* weights) {
    if (!kernel_matrix || !weights) return "null argument";
    return jconv_weights(order_x, order_y, kernel_matrix, divisor, weights);
}

static inline const char* jq_lighting_plan(const jh_lighting_desc* desc, jh_light_plan* plan) {
    if (!desc || !plan) return "null argument";
    return jlight_plan(desc, plan);
}

static inline const char* jq_lighting_tables(const jh_lighting_desc* desc, float* spec_table, float* spot_table, uint32_t* which) {
    if (!desc) return "null descriptor";
    if (const char* why = jlight_desc_error(desc)) return why;
    const uint32_t w = jlight_tables(desc, spec_table, spot_table);
    if (which) *which = w;
    return nullptr;
}

static inline const char* jq_turbulence_plan(const jh_turbulence_desc* desc, jh_turb_plan* plan) {
    if (!desc || !plan) return "null argument";
    return jturb_plan(desc, plan);
}

static inline const char* jq_turbulence_tables(const jh_turbulence_desc* desc, uint8_t* selector, float* gradients) {
    if (!desc) return "null descriptor";
    if (const char* why = jturb_desc_error(desc)) return why;
    jturb_tables(desc->seed, selector, gradients);
    return nullptr;
}

static inline const char* jq_displace_offset(float scale, uint16_t f16_bits, int64_t* out) {
    if (!out) return "null argument";
    *out = jdisp_offset(scale, f16_bits);
    return nullptr;
}

static inline const char* jq_shadow_plan(const jh_shadow_desc* desc, jh_shad_plan* plan) {
    if (!desc || !plan) return "null argument";
    return jshadow_plan(desc, plan);
}

static inline const char* jq_shadow_bounds(const jh_shadow_desc* desc, uint32_t dst_w, uint32_t dst_h, uint32_t* rect) {
    if (!desc || !rect) return "null argument";
    return jshadow_bounds(desc, dst_w, dst_h, rect);
}

static inline const char* jq_perspective_plan(const double* matrix, double* plan) {
    if (!matrix || !plan) return "null argument";
    return jpersp_plan(matrix, plan);
}

static inline const char* jq_perspective_bounds(const double* matrix, uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h, uint32_t* rect) {
    if (!matrix || !rect) return "null argument";
    return jpersp_bounds(matrix, src_w, src_h, filter, dst_w, dst_h, rect);
}

static inline const char* jq_distance_plan(const jh_distance_desc* desc, uint32_t image_w, uint32_t image_h, jh_dist_plan* plan) {
    if (!desc || !plan) return "null argument";
    return jdist_plan(desc, image_w, image_h, plan);
}

static inline const char* jq_stats_plan(const jh_stats_desc* desc, uint32_t image_w, uint32_t image_h, jh_stats_plan_t* plan) {
    if (!desc || !plan) return "null argument";
    return jstats_plan(desc, image_w, image_h, plan);
}

static inline const char* jq_stats_codes(int transfer, uint64_t n, const uint16_t* f16_bits, uint8_t* codes) {
    if (n != 0u && (!f16_bits || !codes)) return "null argument";
    return jstats_codes(transfer, n, f16_bits, codes, kSrgbEncodeThreshold);
}

static inline const char* jq_load_texel(int format_or_transfer, int alpha, uint64_t n, const uint8_t* rgba, uint16_t* out) {
    if (n != 0u && (!rgba || !out)) return "null argument";
    return jload_texels(format_or_transfer, alpha, n, rgba, out);
}

static inline const char* jq_load_yuv_codes(int matrix, int range, uint64_t n, const uint8_t* y, const uint16_t* s_cb, const uint16_t* s_cr, uint8_t* rgb) {
    if (n != 0u && (!y || !s_cb || !s_cr || !rgb)) return "null argument";
    return jload_yuv_codes(matrix, range, n, y, s_cb, s_cr, rgb);
}

static inline const char* jq_lut3d_identity(uint32_t n, uint16_t* out_texels) {
    if (!out_texels) return "null argument";
    return jlut_identity_query(n, out_texels);
}

static inline const char* jq_lut3d_texels(uint32_t n, const uint16_t* lut_texels, const uint16_t* in_texels, uint64_t count, uint16_t* out_texels) {
    if (!lut_texels || (count != 0u && (!in_texels || !out_texels))) return "null argument";
    return jlut_texels(n, lut_texels, in_texels, count, out_texels);
}

// (the geometry of jh_composite: out[6] = {sx', sy', dx', dy', w, h}, all zero when nothing is left)
static inline const char* jq_composite_clip(uint32_t src_w, uint32_t src_h, uint32_t sx, uint32_t sy, uint32_t sw, uint32_t sh, int32_t dx, int32_t dy,
                                            uint32_t dst_w, uint32_t dst_h, uint32_t* out) {
    jcomp_rect r;
    if (!out || jcomp_clip(src_w, src_h, sx, sy, sw, sh, dx, dy, dst_w, dst_h, &r))
        return "the source rectangle is not inside the source image or is empty in one dimension";
    out[0] = r.sx; out[1] = r.sy; out[2] = r.dx; out[3] = r.dy; out[4] = r.w; out[5] = r.h;
    return nullptr;
}

// The queries, each named here and nowhere else in the two libraries:
//   X(name, (the exported function's parameters), (the same as arguments))
// JQ_QUERY_LIST: exported by both libraries, as jh_<name> (declared in jello_hip.h) and as its host twin jl_<name>.
// JQ_HOST_QUERY_LIST: exported by the host library alone, as jl_<name>.
#define JQ_QUERY_LIST(X)                                                                                                                    \
    X(blur_taps, (float sigma, float* weights, uint32_t* radius), (sigma, weights, radius))                                                 \
    X(resample_taps, (int filter, uint32_t n_in, uint32_t n_out, uint32_t i, float* weights, uint32_t* first, uint32_t* count),            \
      (filter, n_in, n_out, i, weights, first, count))                                                                                      \
    X(color_tables, (const jh_color_desc* desc, float* pre, uint16_t* post, uint32_t* which), (desc, pre, post, which))                     \
    X(warp_plan, (const double* matrix, int64_t* plan), (matrix, plan))                                                                     \
    X(warp_bounds, (const double* matrix, uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h, uint32_t* rect),     \
      (matrix, src_w, src_h, filter, dst_w, dst_h, rect))                                                                                   \
    X(convolve_weights, (uint32_t order_x, uint32_t order_y, const double* kernel_matrix, double divisor, float* weights),                 \
      (order_x, order_y, kernel_matrix, divisor, weights))                                                                                  \
    X(lighting_plan, (const jh_lighting_desc* desc, jh_light_plan* plan), (desc, plan))                                                     \
    X(lighting_tables, (const jh_lighting_desc* desc, float* spec_table, float* spot_table, uint32_t* which),                              \
      (desc, spec_table, spot_table, which))                                                                                                \
    X(turbulence_plan, (const jh_turbulence_desc* desc, jh_turb_plan* plan), (desc, plan))                                                  \
    X(turbulence_tables, (const jh_turbulence_desc* desc, uint8_t* selector, float* gradients), (desc, selector, gradients))               \
    X(displace_offset, (float scale, uint16_t f16_bits, int64_t* out), (scale, f16_bits, out))                                              \
    X(shadow_plan, (const jh_shadow_desc* desc, jh_shad_plan* plan), (desc, plan))                                                        \
    X(shadow_bounds, (const jh_shadow_desc* desc, uint32_t dst_w, uint32_t dst_h, uint32_t* rect), (desc, dst_w, dst_h, rect))        \
    X(perspective_plan, (const double* matrix, double* plan), (matrix, plan))                                                               \
    X(perspective_bounds, (const double* matrix, uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h, uint32_t* rect), \
      (matrix, src_w, src_h, filter, dst_w, dst_h, rect))                                                                                   \
    X(distance_plan, (const jh_distance_desc* desc, uint32_t image_w, uint32_t image_h, jh_dist_plan* plan), (desc, image_w, image_h, plan)) \
    X(stats_plan, (const jh_stats_desc* desc, uint32_t image_w, uint32_t image_h, jh_stats_plan_t* plan), (desc, image_w, image_h, plan))   \
    X(stats_codes, (int transfer, uint64_t n, const uint16_t* f16_bits, uint8_t* codes), (transfer, n, f16_bits, codes))                    \
    X(load_texel, (int format_or_transfer, int alpha, uint64_t n, const uint8_t* rgba, uint16_t* out), (format_or_transfer, alpha, n, rgba, out)) \
    X(load_yuv_codes, (int matrix, int range, uint64_t n, const uint8_t* y, const uint16_t* s_cb, const uint16_t* s_cr, uint8_t* rgb),     \
      (matrix, range, n, y, s_cb, s_cr, rgb))                                                                                               \
    X(lut3d_identity, (uint32_t n, uint16_t* out_texels), (n, out_texels))                                                                  \
    X(lut3d_texels, (uint32_t n, const uint16_t* lut_texels, const uint16_t* in_texels, uint64_t count, uint16_t* out_texels),             \
      (n, lut_texels, in_texels, count, out_texels))
#define JQ_HOST_QUERY_LIST(X)                                                                                                               \
    X(composite_clip,                                                                                                                       \
      (uint32_t src_w, uint32_t src_h, uint32_t sx, uint32_t sy, uint32_t sw, uint32_t sh, int32_t dx, int32_t dy, uint32_t dst_w, uint32_t dst_h, \
       uint32_t* out),                                                                                                                      \
      (src_w, src_h, sx, sy, sw, sh, dx, dy, dst_w, dst_h, out))
