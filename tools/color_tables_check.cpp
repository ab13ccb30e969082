// color_tables_check.cpp -- include/jello_color.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/color_tables_check.cpp -o /tmp/color_tables_check && /tmp/color_tables_check
//
// Builds the tables of every func type (TABLE and DISCRETE with n = 1, 2, 3, 64) in both spaces and under both clamp settings into
// arrays of exactly 3 x 65 536 floats and 4 x 65 536 f16 bit patterns (so that a write past either end is an AddressSanitizer
// report), and checks what the rule promises: `which` is what the descriptor needs and only those tables are written, no entry is a
// NaN other than the canonical ones, a clamped table stays inside [0, 1], the f16 conversions round-trip every bit pattern, the key
// ignores what a func's type does not use, and the refusals.  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jello_color.h"

static const uint16_t kUntouched = 0xdeadu;

static jh_color_func make_func(int type, uint32_t n) {
    jh_color_func f;
    memset(&f, 0, sizeof f);
    f.type = type;
    f.n = n;
    f.slope = 1.5f; f.intercept = -0.25f;
    f.amplitude = 1.1f; f.exponent = 2.2f; f.offset = -0.05f;
    for (uint32_t k = 0; k < n && k < JH_COLOR_MAX_VALUES; k++) f.values[k] = (float)((k * 37u) % 11u) / 10.0f;
    return f;
}

static int check(const jh_color_desc& d) {
    if (jcolor_desc_error(&d)) return 1;
    std::vector<float> pre(3u * JCOLOR_ENTRIES, -7.0f);
    std::vector<uint16_t> post(4u * JCOLOR_ENTRIES, kUntouched);
    const uint32_t which = jcolor_tables(&d, pre.data(), post.data());
    if (which != jcolor_which(&d)) return 2;
    const bool clamp = (d.flags & JH_COLOR_CLAMP) != 0u;
    for (uint32_t c = 0; c < 3u; c++) {
        const bool exists = (which & JCOLOR_PRE(c)) != 0u;
        if (exists != (d.space == JH_COLOR_SRGB)) return 3;
        for (uint32_t h = 0; h < JCOLOR_ENTRIES; h++) {
            const float v = pre[c * JCOLOR_ENTRIES + h];
            if (!exists) { if (v != -7.0f) return 4; continue; }
            const bool nan_in = (h & 0x7fffu) > 0x7c00u;
            if ((v != v) != nan_in) return 5;
            if (!nan_in && signbit(v) != ((h & 0x8000u) != 0u)) return 6;  // enc is odd, +-0 keep their sign
        }
    }
    for (uint32_t i = 0; i < 4u; i++) {
        const bool exists = (which & JCOLOR_POST(i)) != 0u;
        if (exists != (d.func[i].type != JH_COLOR_FUNC_IDENTITY || (d.space == JH_COLOR_SRGB && i < 3u))) return 7;
        for (uint32_t h = 0; h < JCOLOR_ENTRIES; h++) {
            const uint16_t g = post[i * JCOLOR_ENTRIES + h];
            if (!exists) { if (g != kUntouched) return 8; continue; }
            if ((g & 0x7fffu) > 0x7c00u && g != 0x7e00u) return 9;
            if ((h & 0x7fffu) > 0x7c00u && g != 0x7e00u) return 10;
            if (clamp && (h & 0x7fffu) <= 0x7c00u && !(g <= 0x3c00u)) return 11;  // +0 .. 1.0 as bit patterns
        }
    }
    return 0;
}

int main() {
    for (uint32_t h = 0; h < JCOLOR_ENTRIES; h++) {
        const double v = jcolor_f16_value(h);
        const uint16_t back = jcolor_f16_bits(v);
        if (back != ((h & 0x7fffu) > 0x7c00u ? 0x7e00u : h)) { printf("f16 %#06x does not round-trip (%#06x)\n", h, back); return 1; }
    }
    // ties go to the even side, the overflow threshold, the smallest subnormal's half
    if (jcolor_f16_bits(1.0 + ldexp(1.0, -11)) != 0x3c00u || jcolor_f16_bits(1.0 + 3.0 * ldexp(1.0, -11)) != 0x3c02u ||
        jcolor_f16_bits(65519.99) != 0x7bffu || jcolor_f16_bits(65520.0) != 0x7c00u || jcolor_f16_bits(ldexp(1.0, -25)) != 0x0000u ||
        jcolor_f16_bits(ldexp(1.5, -25)) != 0x0001u || jcolor_f16_bits(-0.0) != 0x8000u || jcolor_f16_bits(ldexp(1.0, -14) - ldexp(1.0, -26)) != 0x0400u) {
        printf("the f16 rounding is wrong\n");
        return 1;
    }
    int cases = 0;
    const int types[] = {JH_COLOR_FUNC_IDENTITY, JH_COLOR_FUNC_LINEAR, JH_COLOR_FUNC_GAMMA, JH_COLOR_FUNC_TABLE, JH_COLOR_FUNC_DISCRETE};
    const uint32_t counts[] = {1u, 2u, 3u, 64u};
    for (int space : {JH_COLOR_LINEAR, JH_COLOR_SRGB})
        for (uint32_t flags : {0u, JH_COLOR_CLAMP})
            for (int type : types)
                for (uint32_t n : counts) {
                    if (n != 1u && type != JH_COLOR_FUNC_TABLE && type != JH_COLOR_FUNC_DISCRETE) continue;
                    jh_color_desc d;
                    memset(&d, 0, sizeof d);
                    d.space = space;
                    d.flags = flags;
                    for (int i = 0; i < 4; i++) d.func[i] = make_func(i == 1 ? JH_COLOR_FUNC_IDENTITY : type, n);
                    if (int rc = check(d)) { printf("space %d, flags %u, type %d, n %u: check %d failed\n", space, flags, type, n, rc); return 1; }
                    cases++;
                }
    // the key: what a type does not use is no part of it, what it uses is
    jh_color_desc a, b;
    memset(&a, 0, sizeof a);
    a.func[0] = make_func(JH_COLOR_FUNC_LINEAR, 0u);
    a.func[2] = make_func(JH_COLOR_FUNC_TABLE, 3u);
    b = a;
    b.func[0].exponent = 9.0f; b.func[0].values[5] = 4.0f; b.func[2].values[3] = 1.0f; b.func[2].slope = 0.0f; b.matrix[7] = 2.0f; b.x = 3u;
    jcolor_key ka, kb;
    jcolor_key_of(&a, &ka);
    jcolor_key_of(&b, &kb);
    if (!jcolor_key_equal(&ka, &kb)) { printf("the key depends on unused parameters\n"); return 1; }
    b.func[2].values[2] = 0.125f;
    jcolor_key_of(&b, &kb);
    if (jcolor_key_equal(&ka, &kb)) { printf("the key misses a value\n"); return 1; }
    // refusals
    jh_color_desc bad = a;
    bad.space = 2;
    if (!jcolor_desc_error(&bad)) return 1;
    bad = a; bad.flags = 2u;
    if (!jcolor_desc_error(&bad)) return 1;
    bad = a; bad.func[3].type = 5;
    if (!jcolor_desc_error(&bad)) return 1;
    bad = a; bad.func[3].type = -1;
    if (!jcolor_desc_error(&bad)) return 1;
    bad = a; bad.func[2].n = 0u;
    if (!jcolor_desc_error(&bad)) return 1;
    bad = a; bad.func[2].n = 65u;
    if (!jcolor_desc_error(&bad)) return 1;
    bad = a; bad.func[0].slope = INFINITY;
    if (!jcolor_desc_error(&bad)) return 1;
    bad = a; bad.func[2].values[1] = NAN;
    if (!jcolor_desc_error(&bad)) return 1;
    printf("ok: %d descriptors\n", cases);
    return 0;
}
