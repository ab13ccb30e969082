// queries_check.cpp -- include/jello_queries.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/queries_check.cpp -o /tmp/queries_check && /tmp/queries_check
//
// Calls every jq_<name> with a legal input into heap buffers of exactly the sizes jello_hip.h documents -- a write past one is an
// AddressSanitizer report --, with each pointer argument null in turn -- a null that is read or written is a report too; the
// answer must be the reason for a required argument and success for an optional one --, and with one illegal descriptor or value,
// after which every output must be as it was.  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <memory>

#include "jello_queries.h"

static int g_fail = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            g_fail = 1;                                              \
        }                                                            \
    } while (0)

// A heap buffer of exactly n entries, every byte 0xA5.
template <class T>
struct Buf {
    std::unique_ptr<T[]> p;
    size_t n;
    explicit Buf(size_t count) : p(new T[count]), n(count) { memset((void*)p.get(), 0xA5, n * sizeof(T)); }
    operator T*() { return p.get(); }
    bool untouched() const {
        const unsigned char* b = (const unsigned char*)p.get();
        for (size_t i = 0; i < n * sizeof(T); i++)
            if (b[i] != 0xA5) return false;
        return true;
    }
};
static bool is(const char* why, const char* want) { return why && strcmp(why, want) == 0; }

static void blur() {
    Buf<float> w(11);  // sigma 1.5: R = ceil(4.5) = 5, 2R + 1 taps
    Buf<uint32_t> r(1);
    CHECK(!jq_blur_taps(1.5f, w, r) && r[0] == 5u && !w.untouched());
    CHECK(!jq_blur_taps(1.5f, nullptr, r) && !jq_blur_taps(1.5f, w, nullptr));
    Buf<float> w_max(2u * JBLUR_MAX_RADIUS + 1u);
    CHECK(!jq_blur_taps(JBLUR_MAX_SIGMA, w_max, r) && r[0] == JBLUR_MAX_RADIUS);
    Buf<float> w2(11);
    Buf<uint32_t> r2(1);
    CHECK(is(jq_blur_taps(-1.0f, w2, r2), "sigma is negative, above 64 or NaN") && jq_blur_taps(NAN, w2, r2) && jq_blur_taps(64.5f, w2, r2));
    CHECK(w2.untouched() && r2.untouched());
}

static void resample() {
    Buf<float> w(JRESAMPLE_MAX_TAPS);
    Buf<uint32_t> first(1), count(1);
    for (int filter = 0; filter < JRESAMPLE_FILTERS; filter++) {  // the widest window: 16:1 down
        CHECK(!jq_resample_taps(filter, 1600u, 100u, 50u, w, first, count) && count[0] >= 1u && count[0] <= JRESAMPLE_MAX_TAPS);
        CHECK(!jq_resample_taps(filter, 7u, 100u, 99u, w, first, count) && first[0] + count[0] <= 7u);
    }
    CHECK(!jq_resample_taps(3, 100u, 37u, 5u, nullptr, first, count) && !jq_resample_taps(3, 100u, 37u, 5u, w, nullptr, count) &&
          !jq_resample_taps(3, 100u, 37u, 5u, w, first, nullptr));
    Buf<float> w2(JRESAMPLE_MAX_TAPS);
    Buf<uint32_t> f2(1), c2(1);
    CHECK(jq_resample_taps(4, 100u, 37u, 5u, w2, f2, c2) && jq_resample_taps(0, 0u, 37u, 5u, w2, f2, c2) && jq_resample_taps(0, 593u, 37u, 5u, w2, f2, c2) &&
          jq_resample_taps(0, 100u, 37u, 37u, w2, f2, c2));
    CHECK(w2.untouched() && f2.untouched() && c2.untouched());
}

static void color() {
    Buf<jh_color_desc> d(1);
    memset(d, 0, sizeof(jh_color_desc));
    d[0].space = JH_COLOR_SRGB;
    d[0].flags = JH_COLOR_CLAMP;
    d[0].func[0].type = JH_COLOR_FUNC_LINEAR;
    d[0].func[0].slope = 0.5f;
    d[0].func[3].type = JH_COLOR_FUNC_TABLE;
    d[0].func[3].n = JH_COLOR_MAX_VALUES;
    for (uint32_t k = 0; k < JH_COLOR_MAX_VALUES; k++) d[0].func[3].values[k] = (float)k / 63.0f;
    Buf<float> pre(3u * 65536u);
    Buf<uint16_t> post(4u * 65536u);
    Buf<uint32_t> which(1);
    CHECK(!jq_color_tables(d, pre, post, which) && which[0] != 0u && !pre.untouched() && !post.untouched());
    CHECK(!jq_color_tables(d, nullptr, post, which) && !jq_color_tables(d, pre, nullptr, which) && !jq_color_tables(d, pre, post, nullptr));
    Buf<float> pre2(3u * 65536u);
    Buf<uint16_t> post2(4u * 65536u);
    Buf<uint32_t> which2(1);
    CHECK(is(jq_color_tables(nullptr, pre2, post2, which2), "null descriptor"));
    d[0].func[3].n = JH_COLOR_MAX_VALUES + 1u;
    CHECK(is(jq_color_tables(d, pre2, post2, which2), "a func has no values or more than 64"));
    CHECK(pre2.untouched() && post2.untouched() && which2.untouched());
}

static void warp() {
    Buf<double> m(6);
    const double legal[6] = {2.0, 0.5, -0.25, 1.5, 3.0, -7.0};
    memcpy(m, legal, sizeof legal);
    Buf<int64_t> plan(6);
    Buf<uint32_t> rect(4);
    CHECK(!jq_warp_plan(m, plan) && !plan.untouched());
    CHECK(!jq_warp_bounds(m, 40u, 30u, JWARP_BICUBIC, 100u, 90u, rect) && rect[0] + rect[2] <= 100u && rect[1] + rect[3] <= 90u);
    Buf<int64_t> plan2(6);
    Buf<uint32_t> rect2(4);
    CHECK(is(jq_warp_plan(nullptr, plan2), "null argument") && is(jq_warp_plan(m, nullptr), "null argument"));
    CHECK(is(jq_warp_bounds(nullptr, 40u, 30u, 0, 100u, 90u, rect2), "null argument") && is(jq_warp_bounds(m, 40u, 30u, 0, 100u, 90u, nullptr), "null argument"));
    m[3] = -0.0625;  // a d - b c = 0
    CHECK(is(jq_warp_plan(m, plan2), "the determinant is 0") && is(jq_warp_bounds(m, 40u, 30u, 0, 100u, 90u, rect2), "the determinant is 0"));
    CHECK(plan2.untouched() && rect2.untouched());
}

static void convolve() {
    const uint32_t n = JCONV_MAX_TAPS;  // the largest kernel: 15 x 15
    Buf<double> km(n);
    for (uint32_t k = 0; k < n; k++) km[k] = (double)k - 100.0;
    Buf<float> w(n);
    CHECK(!jq_convolve_weights(JCONV_MAX_ORDER, JCONV_MAX_ORDER, km, 0.0, w) && !w.untouched());
    Buf<float> w2(n);
    CHECK(is(jq_convolve_weights(15u, 15u, nullptr, 0.0, w2), "null argument") && is(jq_convolve_weights(15u, 15u, km, 0.0, nullptr), "null argument"));
    CHECK(is(jq_convolve_weights(16u, 15u, km, 0.0, w2), "an order outside 1..15"));
    CHECK(w2.untouched());
}

static void lighting() {
    Buf<jh_lighting_desc> d(1);
    memset(d, 0, sizeof(jh_lighting_desc));
    d[0].kind = JH_LIGHTING_SPECULAR;
    d[0].light = JH_LIGHT_SPOT;
    d[0].surface_scale = 2.0f; d[0].constant = 0.75f; d[0].specular_exponent = 3.0f; d[0].spot_exponent = 2.0f;
    d[0].color[0] = d[0].color[1] = d[0].color[2] = 1.0f;
    d[0].position[0] = 10.0; d[0].position[1] = 20.0; d[0].position[2] = 30.0;
    d[0].cone_cos = 0.5;
    Buf<jh_light_plan> plan(1);
    Buf<float> spec(JLIGHT_ENTRIES), spot(JLIGHT_ENTRIES);
    Buf<uint32_t> which(1);
    CHECK(!jq_lighting_plan(d, plan) && !plan.untouched());
    CHECK(!jq_lighting_tables(d, spec, spot, which) && which[0] == (JLIGHT_TABLE_SPEC | JLIGHT_TABLE_SPOT) && spec[JLIGHT_ENTRIES - 1u] == 1.0f && spot[JLIGHT_ENTRIES - 1u] == 1.0f);
    CHECK(!jq_lighting_tables(d, nullptr, spot, which) && !jq_lighting_tables(d, spec, nullptr, which) && !jq_lighting_tables(d, spec, spot, nullptr));
    Buf<jh_light_plan> plan2(1);
    Buf<float> spec2(JLIGHT_ENTRIES), spot2(JLIGHT_ENTRIES);
    Buf<uint32_t> which2(1);
    CHECK(is(jq_lighting_plan(nullptr, plan2), "null argument") && is(jq_lighting_plan(d, nullptr), "null argument"));
    CHECK(is(jq_lighting_tables(nullptr, spec2, spot2, which2), "null descriptor"));
    d[0].spot_exponent = 129.0f;
    CHECK(is(jq_lighting_plan(d, plan2), "the spot_exponent is outside [1, 128]") && is(jq_lighting_tables(d, spec2, spot2, which2), "the spot_exponent is outside [1, 128]"));
    CHECK(plan2.untouched() && spec2.untouched() && spot2.untouched() && which2.untouched());
}

static void turbulence() {
    Buf<jh_turbulence_desc> d(1);
    memset(d, 0, sizeof(jh_turbulence_desc));
    d[0].kind = JH_TURBULENCE_TURBULENCE;
    d[0].octaves = 3u; d[0].seed = 7; d[0].stitch = 1;
    d[0].base_frequency[0] = 0.05; d[0].base_frequency[1] = 0.03;
    d[0].tile[2] = 64.0; d[0].tile[3] = 48.0;
    Buf<jh_turb_plan> plan(1);
    Buf<uint8_t> P(256);
    Buf<float> G(JTURB_GRADIENT_FLOATS);
    CHECK(!jq_turbulence_plan(d, plan) && !plan.untouched());
    CHECK(!jq_turbulence_tables(d, P, G) && !P.untouched() && !G.untouched());
    CHECK(!jq_turbulence_tables(d, nullptr, G) && !jq_turbulence_tables(d, P, nullptr));
    Buf<jh_turb_plan> plan2(1);
    Buf<uint8_t> P2(256);
    Buf<float> G2(JTURB_GRADIENT_FLOATS);
    CHECK(is(jq_turbulence_plan(nullptr, plan2), "null argument") && is(jq_turbulence_plan(d, nullptr), "null argument"));
    CHECK(is(jq_turbulence_tables(nullptr, P2, G2), "null descriptor"));
    d[0].octaves = JTURB_MAX_OCTAVES + 1u;
    CHECK(is(jq_turbulence_plan(d, plan2), "more than 16 octaves") && is(jq_turbulence_tables(d, P2, G2), "more than 16 octaves"));
    CHECK(plan2.untouched() && P2.untouched() && G2.untouched());
}

static void displace() {
    Buf<int64_t> out(1);
    CHECK(!jq_displace_offset(12.5f, 0x3A00u, out) && !out.untouched());  // (every scale and bit pattern is legal: tools/displace_check.cpp walks them)
    CHECK(!jq_displace_offset(INFINITY, 0x7E00u, out) && out[0] == 0);    // (a NaN product counts as 0)
    CHECK(is(jq_displace_offset(12.5f, 0x3A00u, nullptr), "null argument"));
}

static void shadow() {
    Buf<jh_shadow_desc> d(1);
    memset(d, 0, sizeof(jh_shadow_desc));
    d[0].matrix[0] = d[0].matrix[3] = 1.0;
    d[0].box[0] = 10.0f; d[0].box[1] = 8.0f; d[0].box[2] = 50.0f; d[0].box[3] = 30.0f;
    d[0].radius = 6.0f;
    d[0].sigma = 2.0f;
    Buf<jh_shad_plan> plan(1);
    Buf<uint32_t> rect(4);
    CHECK(!jq_shadow_plan(d, plan) && !plan.untouched() && plan[0].n == 16u && plan[0].k == JSHADOW_K);
    CHECK(!jq_shadow_bounds(d, 64u, 48u, rect) && rect[0] == 1u && rect[1] == 0u && rect[2] == 58u && rect[3] == 39u);  // grown by 7.25: 2.75 .. 57.25, 0.75 .. 37.25
    Buf<jh_shad_plan> plan2(1);
    Buf<uint32_t> rect2(4);
    CHECK(is(jq_shadow_plan(nullptr, plan2), "null argument") && is(jq_shadow_plan(d, nullptr), "null argument"));
    CHECK(is(jq_shadow_bounds(nullptr, 64u, 48u, rect2), "null argument") && is(jq_shadow_bounds(d, 64u, 48u, nullptr), "null argument"));
    CHECK(is(jq_shadow_bounds(d, JSHADOW_MAX_EXTENT + 1u, 48u, rect2), "an image extent above 2^23"));
    d[0].sigma = -1.0f;
    CHECK(is(jq_shadow_plan(d, plan2), "sigma is outside [0, 2^16] or not finite") && is(jq_shadow_bounds(d, 64u, 48u, rect2), "sigma is outside [0, 2^16] or not finite"));
    d[0].sigma = 2.0f;
    d[0].matrix[0] = NAN;
    CHECK(is(jq_shadow_plan(d, plan2), "a matrix entry is not finite") && is(jq_shadow_bounds(d, 64u, 48u, rect2), "a matrix entry is not finite"));
    CHECK(plan2.untouched() && rect2.untouched());
}

static void perspective() {
    Buf<double> m(9);
    const double keystone[9] = {1.0, 0.0, 0.25, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};  // w = 1 + x / 4
    memcpy(m, keystone, sizeof keystone);
    Buf<double> plan(9);
    Buf<uint32_t> rect(4);
    CHECK(!jq_perspective_plan(m, plan) && !plan.untouched() && plan[0] == 1.0 && plan[6] == -0.25 && plan[8] == 1.0);
    CHECK(!jq_perspective_bounds(m, 4u, 2u, JWARP_NEAREST, 16u, 8u, rect) && rect[0] == 0u && rect[1] == 0u && rect[2] == 4u && rect[3] == 4u);  // x: -4/7 .. 36/17, y: -4/7 .. 20/7
    Buf<double> plan2(9);
    Buf<uint32_t> rect2(4);
    CHECK(is(jq_perspective_plan(nullptr, plan2), "null argument") && is(jq_perspective_plan(m, nullptr), "null argument"));
    CHECK(is(jq_perspective_bounds(nullptr, 4u, 2u, 0, 16u, 8u, rect2), "null argument") && is(jq_perspective_bounds(m, 4u, 2u, 0, 16u, 8u, nullptr), "null argument"));
    CHECK(is(jq_perspective_bounds(m, 4u, 2u, 3, 16u, 8u, rect2), "unknown filter") && is(jq_perspective_bounds(m, 4u, 2u, 0, 32769u, 8u, rect2), "an image side above 32768"));
    m[8] = NAN;
    CHECK(is(jq_perspective_plan(m, plan2), "a matrix entry is not finite") && is(jq_perspective_bounds(m, 4u, 2u, 0, 16u, 8u, rect2), "a matrix entry is not finite"));
    m[8] = 0.0;
    m[2] = 0.0;
    CHECK(is(jq_perspective_plan(m, plan2), "the determinant is 0"));
    CHECK(plan2.untouched() && rect2.untouched());
}

static void distance() {
    Buf<jh_distance_desc> d(1);
    memset(d, 0, sizeof(jh_distance_desc));
    d[0].channel = 3; d[0].threshold = 0.5f; d[0].which = JDIST_SIGNED; d[0].max_distance = 7u; d[0].scale = 1.0f;
    d[0].x = 3u; d[0].y = 5u; d[0].width = 40u; d[0].height = 20u;
    Buf<jh_dist_plan> plan(1);
    CHECK(!jq_distance_plan(d, 100u, 50u, plan) && plan[0].x == 3u && plan[0].y == 5u && plan[0].width == 40u && plan[0].height == 20u && plan[0].radius == 7u &&
          plan[0].cap == 64u && plan[0].planes == 2u && plan[0].plane_columns == 54u && plan[0].plane_rows == 20u && plan[0].scratch_bytes == 4320u);
    Buf<jh_dist_plan> plan2(1);
    CHECK(is(jq_distance_plan(nullptr, 100u, 50u, plan2), "null argument") && is(jq_distance_plan(d, 100u, 50u, nullptr), "null argument"));
    CHECK(is(jq_distance_plan(d, 42u, 50u, plan2), "the rectangle is not inside the image"));
    d[0].max_distance = 256u;
    CHECK(is(jq_distance_plan(d, 100u, 50u, plan2), "max_distance outside [1, 255]"));
    d[0].max_distance = 7u;
    d[0].scale = INFINITY;
    CHECK(is(jq_distance_plan(d, 100u, 50u, plan2), "scale or offset is not finite"));
    CHECK(plan2.untouched());
}

static void stats() {
    Buf<jh_stats_desc> d(1);
    memset(d, 0, sizeof(jh_stats_desc));
    d[0].what = JSTATS_BOUNDS | JSTATS_HISTOGRAM; d[0].channel = 3; d[0].threshold = 0.5f; d[0].population = JSTATS_CONTENT; d[0].transfer = JSTATS_SRGB;
    d[0].x = 3u; d[0].y = 5u; d[0].width = 40u; d[0].height = 20u;
    Buf<jh_stats_plan_t> plan(1);
    CHECK(!jq_stats_plan(d, 100u, 50u, plan) && plan[0].x == 3u && plan[0].y == 5u && plan[0].width == 40u && plan[0].height == 20u && plan[0].launches == 2u &&
          plan[0].reserved == 0u && plan[0].record_bytes == sizeof(jh_stats_record) && plan[0].scratch_bytes == 1024u * 4168u);
    Buf<jh_stats_plan_t> plan2(1);
    CHECK(is(jq_stats_plan(nullptr, 100u, 50u, plan2), "null argument") && is(jq_stats_plan(d, 100u, 50u, nullptr), "null argument"));
    CHECK(is(jq_stats_plan(d, 42u, 50u, plan2), "the rectangle is not inside the image"));
    d[0].what = 8u;
    CHECK(is(jq_stats_plan(d, 100u, 50u, plan2), "unknown bits in what"));
    d[0].what = 1u;
    d[0].threshold = INFINITY;
    CHECK(is(jq_stats_plan(d, 100u, 50u, plan2), "threshold is not finite"));
    CHECK(plan2.untouched());
    Buf<uint16_t> bits(5);
    bits[0] = 0x0000; bits[1] = 0x3c00; bits[2] = 0x3800; bits[3] = 0x7e00; bits[4] = 0xfc00;
    Buf<uint8_t> codes(5);
    CHECK(!jq_stats_codes(JSTATS_LINEAR, 5u, bits, codes) && codes[0] == 0 && codes[1] == 255 && codes[2] == 128 && codes[3] == 0 && codes[4] == 0);
    CHECK(!jq_stats_codes(JSTATS_SRGB, 5u, bits, codes) && codes[0] == 0 && codes[1] == 255 && codes[2] == 188 && codes[3] == 0 && codes[4] == 0);
    CHECK(!jq_stats_codes(JSTATS_SRGB, 0u, nullptr, nullptr));
    Buf<uint8_t> codes2(5);
    CHECK(is(jq_stats_codes(0, 5u, nullptr, codes2), "null argument") && is(jq_stats_codes(0, 5u, bits, nullptr), "null argument"));
    CHECK(is(jq_stats_codes(2, 5u, bits, codes2), "unknown transfer") && is(jq_stats_codes(-1, 5u, bits, codes2), "unknown transfer"));
    CHECK(codes2.untouched());
}

static void composite() {
    static const char* const kWhy = "the source rectangle is not inside the source image or is empty in one dimension";
    Buf<uint32_t> out(6);
    CHECK(!jq_composite_clip(40u, 30u, 4u, 5u, 20u, 10u, -3, 7, 64u, 12u, out) && out[0] == 7u && out[1] == 5u && out[2] == 0u && out[3] == 7u && out[4] == 17u && out[5] == 5u);
    Buf<uint32_t> out2(6);
    CHECK(is(jq_composite_clip(40u, 30u, 4u, 5u, 20u, 10u, -3, 7, 64u, 12u, nullptr), kWhy));
    CHECK(is(jq_composite_clip(40u, 30u, 30u, 5u, 20u, 10u, 0, 0, 64u, 12u, out2), kWhy) && is(jq_composite_clip(40u, 30u, 4u, 5u, 0u, 10u, 0, 0, 64u, 12u, out2), kWhy));
    CHECK(out2.untouched());
}

static void load() {
    Buf<uint8_t> px(8);
    for (int i = 0; i < 8; i++) px[i] = (uint8_t)(31 * i + 7);
    Buf<uint16_t> out(8);
    CHECK(!jq_load_texel(JH_SURFACE_BGRA8_SRGB, JH_LOAD_ALPHA_PREMULTIPLIED, 2u, px, out) && !out.untouched());
    CHECK(!jq_load_texel(4 + JH_YUV_TRANSFER_SRGB, JH_LOAD_ALPHA_OPAQUE, 2u, px, out) && out[3] == 0x3c00u && out[7] == 0x3c00u);
    CHECK(!jq_load_texel(0, 0, 0u, nullptr, nullptr));
    Buf<uint16_t> out2(8);
    CHECK(is(jq_load_texel(0, 0, 2u, nullptr, out2), "null argument") && is(jq_load_texel(0, 0, 2u, px, nullptr), "null argument"));
    CHECK(is(jq_load_texel(6, 0, 2u, px, out2), "unknown surface format or transfer") && is(jq_load_texel(0, 3, 2u, px, out2), "unknown alpha mode"));
    CHECK(out2.untouched());
    Buf<uint8_t> y(3), rgb(9);
    Buf<uint16_t> s_cb(3), s_cr(3);
    y[0] = 235; y[1] = 63; y[2] = 16;
    s_cb[0] = 2048; s_cb[1] = 16 * 102; s_cb[2] = 4080;
    s_cr[0] = 2048; s_cr[1] = 16 * 240; s_cr[2] = 0;
    CHECK(!jq_load_yuv_codes(JH_YUV_BT709, JH_YUV_LIMITED, 3u, y, s_cb, s_cr, rgb) && rgb[0] == 255 && rgb[1] == 255 && rgb[2] == 255 && rgb[3] == 255 &&
          rgb[4] == 1 && rgb[5] == 0);
    Buf<uint8_t> rgb2(9);
    CHECK(is(jq_load_yuv_codes(2, 0, 3u, y, s_cb, s_cr, rgb2), "unknown matrix or range") && is(jq_load_yuv_codes(0, 0, 3u, y, s_cb, s_cr, nullptr), "null argument") &&
          is(jq_load_yuv_codes(0, 0, 3u, nullptr, s_cb, s_cr, rgb2), "null argument"));
    s_cr[2] = 4081;
    CHECK(is(jq_load_yuv_codes(0, 0, 3u, y, s_cb, s_cr, rgb2), "a chroma sum above 16 * 255"));
    CHECK(rgb2.untouched());
}

static void lut3d() {
    const uint32_t n = 3u;
    Buf<uint16_t> table(4u * n * n * n);
    CHECK(!jq_lut3d_identity(n, table) && !table.untouched() && table[0] == 0u && table[3] == 0x3c00u && table[4u * 26u] == 0x3c00u && table[4u] == 0x3800u);
    Buf<uint16_t> in(4u * 5u), out(4u * 5u);
    for (uint32_t i = 0; i < 20u; i++) in[i] = (uint16_t)(0x3000u + 97u * i);
    CHECK(!jq_lut3d_texels(n, table, in, 5u, out) && !out.untouched());
    CHECK(!jq_lut3d_texels(n, table, nullptr, 0u, nullptr));  // (no texels: only the table is needed)
    Buf<uint16_t> most(4u * JLUT_MAX_SIZE * JLUT_MAX_SIZE * JLUT_MAX_SIZE), least(4u * 8u);
    CHECK(!jq_lut3d_identity(JLUT_MAX_SIZE, most) && !jq_lut3d_identity(JLUT_MIN_SIZE, least) && !jq_lut3d_texels(JLUT_MAX_SIZE, most, in, 5u, out));
    Buf<uint16_t> t2(4u * 8u), o2(4u * 5u);
    CHECK(is(jq_lut3d_identity(n, nullptr), "null argument") && is(jq_lut3d_identity(1u, t2), "size outside 2..65") && jq_lut3d_identity(66u, t2) && jq_lut3d_identity(0u, t2));
    CHECK(is(jq_lut3d_texels(n, nullptr, in, 5u, o2), "null argument") && is(jq_lut3d_texels(n, table, nullptr, 5u, o2), "null argument") &&
          is(jq_lut3d_texels(n, table, in, 5u, nullptr), "null argument") && is(jq_lut3d_texels(1u, table, in, 5u, o2), "size outside 2..65") &&
          jq_lut3d_texels(66u, table, in, 5u, o2));
    CHECK(t2.untouched() && o2.untouched());
}

int main() {
    load();
    lut3d();
    blur();
    resample();
    color();
    warp();
    convolve();
    lighting();
    turbulence();
    displace();
    shadow();
    perspective();
    distance();
    stats();
    composite();
    if (g_fail) return 1;
    printf("ok\n");
    return 0;
}
