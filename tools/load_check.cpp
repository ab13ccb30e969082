// load_check.cpp -- include/jello_load.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/load_check.cpp -o /tmp/load_check && /tmp/load_check
//
// Four things.  (1) The tables against long double: every coefficient is the integer nearest to exact * 2^16, U(c) is the binary32
// nearest to c / 255, L(c) is the sRGB decode in binary64 rounded once, and the f16 tables are the rounding of U and L.  (2) jload_codes
// over all 2^24 (Y, Cb, Cr) triples (as replicated sums) of the BT.709 limited table against the same formula in __int128 with a floor
// division in place of the shift: no sum overflows, and the shift is arithmetic.  (3) jload_chroma_other and jload_chroma_sum on every
// texel of frames up to 5 x 5 against a written-out walk over the chroma samples with the tent weights of their positions, from exactly
// sized arrays (a read past an end is an AddressSanitizer report).  (4) The descriptors' legality from both sides of every boundary.
// (5) include/jello_frame.h, the frame rule the loads share with jh_blit and jh_blit_yuv: plane counts and row bytes of both layouts at
// widths 1..9 against a walk over the pixels, every predicate from both sides, the enum words, clamp8.  Prints "ok" and returns 0.
//
// With arguments -- W H LAYOUT CHROMA MATRIX RANGE TRANSFER HEX, HEX the bytes of the Y, Cb and Cr planes one after the other (W H,
// then twice ceil(W/2) ceil(H/2)), two hex digits each -- it prints the texels of the frame, H lines of W texels "rrrr gggg bbbb aaaa"
// separated by " | ".  tests/test_load_spec.py compares that with tests/load_ref.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jello_load.h"

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            failures++;                                           \
            printf("line %d: %s\n", __LINE__, #c);                \
        }                                                         \
    } while (0)

static void check_tables() {
    const long double kr[2] = {0.299L, 0.2126L}, kb[2] = {0.114L, 0.0722L};
    for (int m = 0; m < 2; m++)
        for (int r = 0; r < 2; r++) {
            const long double kg = 1.0L - kr[m] - kb[m], sy = r == 0 ? 255.0L / 219.0L : 1.0L, s = r == 0 ? 255.0L / 224.0L : 1.0L;
            const long double exact[5] = {sy, 2.0L * (1.0L - kr[m]) * s, -2.0L * kb[m] * (1.0L - kb[m]) / kg * s, -2.0L * kr[m] * (1.0L - kr[m]) / kg * s,
                                          2.0L * (1.0L - kb[m]) * s};
            for (int i = 0; i < 5; i++) {
                CHECK(kLoadYuv[m][r][i] == (int32_t)llrintl(exact[i] * 65536.0L));
                CHECK(fabsl((long double)kLoadYuv[m][r][i] - exact[i] * 65536.0L) < 0.5L);
            }
            CHECK(kLoadYuvOffset[r] == (r == 0 ? 16 : 0));
        }
    for (uint32_t c = 0; c < 256u; c++) {
        const float u = jload_unorm(c);
        const long double q = (long double)c / 255.0L, d = fabsl((long double)u - q);
        CHECK(d <= fabsl((long double)nextafterf(u, 2.0f) - q) && d <= fabsl((long double)nextafterf(u, -1.0f) - q));
        const double x = (double)c / 255.0;
        CHECK(jload_linear(c) == (float)(x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4)));
        CHECK(kLoadUnormF16[c] == jload_f16(u) && kLoadSrgbF16[c] == jload_f16(jload_linear(c)));
        for (int t = 0; t < 2; t++) {  // the f16 entry is within half an f16 ulp of the binary32 value
            const double v = t ? (double)jload_linear(c) : (double)u, h = jcolor_f16_value(t ? kLoadSrgbF16[c] : kLoadUnormF16[c]);
            const double ulp = ldexp(1.0, (v < 6.103515625e-05 ? -14 : ilogb(v)) - 10);
            CHECK(fabs(h - v) <= 0.5 * ulp);
        }
    }
    CHECK(kLoadUnormF16[255] == 0x3c00u && kLoadSrgbF16[255] == 0x3c00u && kLoadUnormF16[0] == 0u && kLoadSrgbF16[0] == 0u);
}

static __int128 floor_div(__int128 a, __int128 b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static uint32_t wide_code(__int128 sum) {
    const __int128 v = floor_div(sum + (1 << 19), 1 << 20);
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
static uint64_t check_codes() {
    const int32_t* k = kLoadYuv[JH_YUV_BT709][JH_YUV_LIMITED];
    const int32_t off = kLoadYuvOffset[JH_YUV_LIMITED];
    uint64_t n = 0, bad = 0;
    for (int32_t y = 0; y < 256; y++)
        for (int32_t cb = 0; cb < 256; cb++)
            for (int32_t cr = 0; cr < 256; cr++, n++) {
                const __int128 luma = (__int128)16 * k[0] * (y - off), u = 16 * cb - 2048, v = 16 * cr - 2048;
                const uint32_t want = wide_code(luma + k[1] * v) | (wide_code(luma + k[2] * u + k[3] * v) << 8) | (wide_code(luma + k[4] * u) << 16);
                bad += jload_codes(k, off, y, 16 * cb, 16 * cr) != want;
            }
    CHECK(bad == 0);
    // the extreme sums of every table stay inside int32 (the rule's "below 6.0e8")
    for (int m = 0; m < 2; m++)
        for (int r = 0; r < 2; r++) {
            const int32_t* t = kLoadYuv[m][r];
            const int64_t luma = (int64_t)16 * t[0] * 255, c1 = (int64_t)llabs(t[1]) * 2048, g = ((int64_t)llabs(t[2]) + llabs(t[3])) * 2048, c4 = (int64_t)llabs(t[4]) * 2048;
            CHECK(luma + c1 + (1 << 19) < 600000000 && luma + g + (1 << 19) < 600000000 && luma + c4 + (1 << 19) < 600000000);
        }
    return n;
}

// S of texel x (y) by the positions: chroma sample c of an axis sits at 2 c + 1/2, the texel at x; its tent weight, in quarters, is
// 4 - |2 x - 4 c - 1| where that is positive (3 for the texel's own sample, 1 for the neighbour on its side), and a sample outside
// the plane is the edge sample.
static int32_t walk_sum(const std::vector<uint8_t>& plane, uint32_t cw, uint32_t ch, uint32_t x, uint32_t y, bool bilinear) {
    if (!bilinear) return 16 * plane[(size_t)(y / 2u) * cw + x / 2u];
    int32_t sum = 0;
    for (int64_t cy = -1; cy <= (int64_t)ch; cy++)
        for (int64_t cx = -1; cx <= (int64_t)cw; cx++) {
            const int64_t wx = 4 - llabs(2 * (int64_t)x - 4 * cx - 1), wy = 4 - llabs(2 * (int64_t)y - 4 * cy - 1);
            if (wx <= 0 || wy <= 0) continue;
            const size_t ix = (size_t)(cx < 0 ? 0 : (cx >= (int64_t)cw ? cw - 1 : cx)), iy = (size_t)(cy < 0 ? 0 : (cy >= (int64_t)ch ? ch - 1 : cy));
            sum += (int32_t)(wx * wy) * plane[iy * cw + ix];
        }
    return sum;
}
static int32_t rule_sum(const std::vector<uint8_t>& plane, uint32_t cw, uint32_t ch, uint32_t x, uint32_t y, int chroma) {
    const uint32_t cx0 = x >> 1, cy0 = y >> 1, cx1 = jload_chroma_other(x, cw), cy1 = jload_chroma_other(y, ch);
    return jload_chroma_sum(chroma, plane[(size_t)cy0 * cw + cx0], plane[(size_t)cy0 * cw + cx1], plane[(size_t)cy1 * cw + cx0], plane[(size_t)cy1 * cw + cx1]);
}
static uint32_t check_chroma() {
    uint32_t frames = 0, seed = 12345u;
    for (uint32_t h = 1; h <= 5u; h++)
        for (uint32_t w = 1; w <= 5u; w++, frames++) {
            const uint32_t cw = (w + 1u) / 2u, ch = (h + 1u) / 2u;
            std::vector<uint8_t> plane((size_t)cw * ch);
            for (auto& b : plane) { seed = seed * 1664525u + 1013904223u; b = (uint8_t)(seed >> 24); }
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) {
                    CHECK(rule_sum(plane, cw, ch, x, y, JH_CHROMA_BILINEAR) == walk_sum(plane, cw, ch, x, y, true));
                    CHECK(rule_sum(plane, cw, ch, x, y, JH_CHROMA_REPLICATE) == walk_sum(plane, cw, ch, x, y, false));
                }
        }
    return frames;
}

static bool same(const char* got, const char* want) { return want ? got && !strcmp(got, want) : !got; }

// include/jello_frame.h: what the way out (jh_blit, jh_blit_yuv) and the way in share.  The plane count and the rows' bytes against a
// count made by walking the pixels, two per chroma sample; every predicate from both sides of its boundary; the words.
static uint32_t check_frame() {
    uint32_t widths = 0;
    for (int layout = JH_YUV_NV12; layout <= JH_YUV_I420; layout++)
        for (uint32_t w = 1; w <= 9u; w++, widths++) {
            uint64_t luma = 0, samples = 0;
            for (uint32_t x = 0; x < w; x++) { luma++; if (x % 2u == 0u) samples++; }  // (a sample per pair of pixels begun)
            CHECK(jframe_chroma_extent(w) == samples);
            std::vector<uint64_t> need = {luma, layout == JH_YUV_NV12 ? 2u * samples : samples};  // NV12: a (Cb, Cr) pair per sample
            if (layout == JH_YUV_I420) need.push_back(samples);
            CHECK(jframe_yuv_planes(layout) == (int)need.size());
            uint8_t byte = 0;
            const void* planes[3] = {&byte, &byte, &byte};
            uint64_t pitches[3] = {need[0], need[1], need.size() > 2u ? need[2] : 0u};
            const int both = JFRAME_NULL_PLANE | JFRAME_SHORT_PITCH;
            CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, both), nullptr));
            for (int i = 0; i < 3; i++) {
                const bool used = i < (int)need.size();
                if (used) {
                    CHECK(jframe_yuv_row_bytes(layout, i, w) == need[(size_t)i]);
                    CHECK(!jframe_pitch_short(layout, i, need[(size_t)i], w) && jframe_pitch_short(layout, i, need[(size_t)i] - 1u, w));
                }
                planes[i] = nullptr;  // a null plane: refused where the layout uses it, under NULL_PLANE only; index 2 of NV12 is ignored
                CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, both), used ? "null plane" : nullptr));
                CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, JFRAME_NULL_PLANE), used ? "null plane" : nullptr));
                CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, JFRAME_SHORT_PITCH), nullptr));
                planes[i] = &byte;
                pitches[i]--;  // a pitch one short (of NV12's index 2: 2^64 - 1, ignored)
                CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, both), used ? "pitch below the row's bytes" : nullptr));
                CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, JFRAME_SHORT_PITCH), used ? "pitch below the row's bytes" : nullptr));
                CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, JFRAME_NULL_PLANE), nullptr));
                if (used && i + 1 < (int)need.size()) {  // plane by plane, null before pitch: a later null plane comes second, an own one first
                    planes[i + 1] = nullptr;
                    CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, both), "pitch below the row's bytes"));
                    planes[i + 1] = &byte; planes[i] = nullptr;
                    CHECK(same(jframe_yuv_planes_error(layout, planes, pitches, w, both), "null plane"));
                    planes[i] = &byte;
                }
                pitches[i]++;
            }
            CHECK(same(jframe_surface_pitch_error(4u * (uint64_t)w, w), nullptr) && same(jframe_surface_pitch_error(4u * (uint64_t)w - 1u, w), "pitch below 4 * width"));
        }
    CHECK(jframe_plane_null(nullptr) && !jframe_plane_null(&widths));
    CHECK(jframe_chroma_extent(0u) == 0u && jframe_chroma_extent(0xffffffffu) == 0x80000000ull);
    CHECK(same(jframe_surface_pitch_error(0u, 0u), nullptr) && same(jframe_surface_pitch_error(0x3fffffffcull - 1u, 0xffffffffu), "pitch below 4 * width"));
    const char* words[4] = {"unknown layout", "unknown matrix", "unknown range", "unknown transfer"};
    for (int field = 0; field < 4; field++)
        for (int v = -1; v <= 2; v++) {
            int e[4] = {JH_YUV_I420, JH_YUV_BT709, JH_YUV_FULL, JH_YUV_TRANSFER_SRGB};
            e[field] = v;
            CHECK(same(jframe_yuv_enums_error(e[0], e[1], e[2], e[3]), v == 0 || v == 1 ? nullptr : words[field]));
            for (int later = field + 1; later < 4; later++) {  // the first illegal value is the one named
                e[later] = 2;
                CHECK(same(jframe_yuv_enums_error(e[0], e[1], e[2], e[3]), v == 0 || v == 1 ? words[field + 1] : words[field]));
            }
        }
    for (int f = -1; f <= 4; f++) {
        CHECK(jframe_surface_format_ok(f) == (f >= 0 && f <= 3) && same(jframe_surface_format_error(f), f >= 0 && f <= 3 ? nullptr : "unknown surface format"));
        CHECK(jframe_surface_srgb(f) == (f == 2 || f == 3) && jframe_surface_bgra(f) == (f == 1 || f == 3));
    }
    for (int32_t v = -300; v <= 600; v++) CHECK(jframe_clamp8(v) == (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)));
    CHECK(jframe_clamp8(INT32_MIN) == 0u && jframe_clamp8(INT32_MAX) == 255u);
    return widths;
}

static void check_legality() {
    uint8_t byte = 0;
    jh_load_surface_desc s = {JH_SURFACE_RGBA8_UNORM, JH_LOAD_ALPHA_STRAIGHT, &byte, 40, 0, 0, 10, 2};
    CHECK(!jload_surface_desc_error(&s));
    for (int f = -1; f <= 4; f++) { s.format = f; CHECK((jload_surface_desc_error(&s) == nullptr) == (f >= 0 && f <= 3)); }
    s.format = 0;
    for (int a = -1; a <= 3; a++) { s.alpha = a; CHECK((jload_surface_desc_error(&s) == nullptr) == (a >= 0 && a <= 2)); }
    s.alpha = 0; s.src = nullptr;
    CHECK(jload_surface_desc_error(&s) != nullptr);
    // (a descriptor's pitches are not the descriptor check's: short ones pass it, and jframe_yuv_planes_error finds them)
    jh_load_yuv_desc y = {JH_YUV_NV12, JH_YUV_BT709, JH_YUV_LIMITED, JH_YUV_TRANSFER_NONE, JH_CHROMA_BILINEAR, 0, {&byte, &byte, nullptr}, {0, 0, 0}, 0, 0, 9, 3};
    CHECK(!jload_yuv_desc_error(&y) && same(jframe_yuv_planes_error(y.layout, y.plane, y.pitch, 9, JFRAME_SHORT_PITCH), "pitch below the row's bytes"));
    y.layout = JH_YUV_I420;
    CHECK(same(jload_yuv_desc_error(&y), "null plane"));  // (the third plane)
    y.plane[2] = &byte;
    CHECK(!jload_yuv_desc_error(&y));
    int32_t* fields[5] = {&y.layout, &y.matrix, &y.range, &y.transfer, &y.chroma};
    for (int32_t* f : fields) {
        const int32_t keep = *f;
        for (int32_t v = -1; v <= 2; v++) { *f = v; CHECK((jload_yuv_desc_error(&y) == nullptr) == (v == 0 || v == 1)); }
        *f = keep;
    }
    uint8_t px[4] = {1, 2, 3, 4};
    uint16_t out[4];
    CHECK(!jload_texels(3, 2, 1, px, out) && !jload_texels(4, 0, 1, px, out) && !jload_texels(5, 1, 1, px, out));
    CHECK(jload_texels(6, 0, 1, px, out) && jload_texels(-1, 0, 1, px, out) && jload_texels(0, 3, 1, px, out));
    uint16_t s_ok = 4080, s_bad = 4081;
    uint8_t rgb[3];
    CHECK(!jload_yuv_codes(1, 1, 1, px, &s_ok, &s_ok, rgb) && jload_yuv_codes(1, 1, 1, px, &s_bad, &s_ok, rgb) && jload_yuv_codes(2, 0, 1, px, &s_ok, &s_ok, rgb));
}

static int print_frame(char** a) {
    const uint32_t w = (uint32_t)atoi(a[0]), h = (uint32_t)atoi(a[1]);
    const int layout = atoi(a[2]), chroma = atoi(a[3]), matrix = atoi(a[4]), range = atoi(a[5]), transfer = atoi(a[6]);
    const uint32_t cw = (w + 1u) / 2u, ch = (h + 1u) / 2u;
    const size_t n = (size_t)w * h + 2u * (size_t)cw * ch;
    if (w == 0u || h == 0u || w > 64u || h > 64u || strlen(a[7]) != 2u * n || jframe_yuv_enums_error(layout, matrix, range, transfer) || (unsigned)chroma > 1u)
        return 2;
    std::vector<uint8_t> bytes(n);
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(a[7] + 2u * i, "%2x", &v) != 1) return 2;
        bytes[i] = (uint8_t)v;
    }
    const std::vector<uint8_t> Y(bytes.begin(), bytes.begin() + (size_t)w * h), Cb(bytes.begin() + (size_t)w * h, bytes.begin() + (size_t)w * h + (size_t)cw * ch),
        Cr(bytes.begin() + (size_t)w * h + (size_t)cw * ch, bytes.end());
    for (uint32_t y = 0; y < h; y++) {
        for (uint32_t x = 0; x < w; x++) {
            const uint32_t c = jload_codes(kLoadYuv[matrix][range], kLoadYuvOffset[range], Y[(size_t)y * w + x], rule_sum(Cb, cw, ch, x, y, chroma), rule_sum(Cr, cw, ch, x, y, chroma));
            uint32_t tx, ty;
            jload_texel(transfer == JH_YUV_TRANSFER_SRGB, JH_LOAD_ALPHA_STRAIGHT, c & 0xffu, (c >> 8) & 0xffu, c >> 16, 255u, &tx, &ty);
            printf("%s%04x %04x %04x %04x", x ? " | " : "", tx & 0xffffu, tx >> 16, ty & 0xffffu, ty >> 16);
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 9) return print_frame(argv + 1);
    if (argc != 1) return 2;
    check_tables();
    const uint64_t triples = check_codes();
    const uint32_t frames = check_chroma();
    const uint32_t widths = check_frame();
    check_legality();
    if (failures) {
        printf("FAILED: %d checks\n", failures);
        return 1;
    }
    printf("ok: 4 tables, %llu triples, %u frames, %u layout widths\n", (unsigned long long)triples, frames, widths);
    return 0;
}
