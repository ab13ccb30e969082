// shadow_check.cpp -- include/jello_shadow.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/shadow_check.cpp -o /tmp/shadow_check && /tmp/shadow_check
//
// Without arguments, five things.  (1) The plan against long double and __int128: the centre within one unit of the exact one, the
// half sizes, the clamped radius and the scalars within one binary32 ulp of their long double values, N from both sides of its
// thresholds, the position of the far corner of the largest image in __int128 (no overflow) and its binary32 value within 2^-24 + half an
// ulp.  (2) G: against erfl on every 64th binary32 in [0, 4.5] (at most 2^-19: Phi within 2^-20), every binary32 of [0.5, 1] in turn for
// monotonicity, oddness, G(+-4) = +-1 and beyond.  (3) The legality boundaries of jshadow_desc_error, each from both sides, the reason
// named.  (4) The bounds: worked cases, and by brute force on small images that every texel outside the rectangle has S < 2^-12.  (5)
// The coverage's consequences: S = 1 deep inside, 0 far outside, the reflection in x exact.  Prints "ok: ..." and returns 0.
//
// With arguments -- x0 y0 x1 y1 radius sigma a b c d e f width height -- it prints the binary32 bits of S of every texel of a width x
// height image by jshadow_texel, row by row, eight hexadecimal digits each: tests/test_shadow_spec.py holds tests/shadow_ref.py to them.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jello_shadow.h"

typedef __int128 i128;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static bool is(const char* got, const char* want) { return got && want && strcmp(got, want) == 0; }
static float ulp(float v) { return nextafterf(fabsf(v), INFINITY) - fabsf(v); }
static bool near32(float got, long double want) { return fabsl((long double)got - want) <= (long double)ulp(got); }

static jh_shadow_desc desc(float x0, float y0, float x1, float y1, float radius, float sigma) {
    jh_shadow_desc d;
    memset(&d, 0, sizeof d);
    d.matrix[0] = d.matrix[3] = 1.0;
    d.box[0] = x0; d.box[1] = y0; d.box[2] = x1; d.box[3] = y1;
    d.radius = radius; d.sigma = sigma;
    d.color[3] = 1.0f;
    return d;
}

static void plans() {
    const float boxes[][4] = {{0, 0, 10, 6}, {-3.25f, 1.5f, 100.75f, 40.0f}, {0.1f, 0.2f, 0.3f, 0.7f}, {-4194304.0f, -4194304.0f, 4194304.0f, 4194304.0f}, {5, 5, 5, 9}, {1e-30f, 0, 7, 1e-20f}};
    const float radii[] = {0.0f, 0.5f, 3.0f, 1e9f, 1e-30f}, sigmas[] = {0.0f, 0.001f, 0.00390625f, 0.5f, 8.0f, 65536.0f};
    for (const auto& b : boxes)
        for (float r : radii)
            for (float s : sigmas) {
                jh_shadow_desc d = desc(b[0], b[1], b[2], b[3], r, s);
                jh_shad_plan p;
                CHECK(!jshadow_plan(&d, &p));
                const long double cx = ((long double)b[0] + b[2]) / 2, cy = ((long double)b[1] + b[3]) / 2, a = ((long double)b[2] - b[0]) / 2, bb = ((long double)b[3] - b[1]) / 2;
                const long double rr = fminl(r, fminl(a, bb)), sg = fmaxl(s, 0.00390625L);
                CHECK(fabsl((long double)p.centre[0] - cx * 4294967296.0L) <= 1.5L && fabsl((long double)p.centre[1] - cy * 4294967296.0L) <= 1.5L);
                CHECK(near32(p.a, a) && near32(p.b, bb) && near32(p.radius, rr) && near32(p.core, a - rr) && near32(p.straight, bb - rr));
                CHECK(p.radius <= p.a && p.radius <= p.b && p.core >= 0.0f && p.straight >= 0.0f);
                CHECK(near32(p.sigma, sg) && near32(p.inv_s, 1.0L / (sg * sqrtl(2.0L))) && near32(p.window, 4.0L * sg) && p.k == 4u);
                const long double rho = rr / sg;
                CHECK(p.n == (rho <= 0.5L ? 4u : rho <= 1.5L ? 8u : 16u) || fabsl(rho - 0.5L) < 1e-12L || fabsl(rho - 1.5L) < 1e-12L);
                CHECK(p.m[0] == ((int64_t)1 << 31) && p.m[1] == 0 && p.m[2] == 0 && p.m[3] == 0 && p.m[4] == ((int64_t)1 << 31) && p.m[5] == 0);
            }
    // N from both sides of its thresholds (sigma = 2: rho = r / 2)
    const struct { float r; uint32_t n; } steps[] = {{0.0f, 4u}, {1.0f, 4u}, {1.0000001f, 8u}, {3.0f, 8u}, {3.0000002f, 16u}, {50.0f, 16u}};
    for (const auto& s : steps) {
        jh_shadow_desc d = desc(-100, -100, 100, 100, s.r, 2.0f);
        jh_shad_plan p;
        CHECK(!jshadow_plan(&d, &p) && p.n == s.n);
    }
    // the far corner of the largest image under the largest inverse coefficients: exact in int64
    jh_shadow_desc d = desc(-4194304.0f, -4194304.0f, 4194304.0f - 1.0f, 4194304.0f, 1.0f, 1.0f);
    d.matrix[0] = 1.0 / 64.0; d.matrix[3] = -1.0 / 64.0; d.matrix[1] = 1.0 / 128.0; d.matrix[4] = 32768.0; d.matrix[5] = -32768.0;
    jh_shad_plan p;
    CHECK(!jshadow_plan(&d, &p));
    const uint32_t far = JSHADOW_MAX_EXTENT - 1u;
    for (int axis = 0; axis < 2; axis++) {
        const int64_t* m = p.m + 3 * axis;
        const i128 exact = (i128)m[0] * (2 * (i128)far + 1) + (i128)m[1] * (2 * (i128)far + 1) + m[2] - p.centre[axis];
        const int64_t got = jwarp_position(m[0], m[1], m[2], far, far) - p.centre[axis];
        CHECK((i128)got == exact);
        const float x = jshadow_to_f32(got);
        CHECK(fabsl((long double)x - (long double)got / 4294967296.0L) <= 5.9604644775390625e-08L + (long double)ulp(x) / 2);
    }
    const int64_t samples[] = {0, 1, -1, 255, 256, -256, ((int64_t)1 << 32) - 1, -((int64_t)1 << 32), ((int64_t)3 << 31) + 12345, -(((int64_t)7 << 40) + 99), ((int64_t)1 << 61) + 77};
    for (int64_t v : samples) {
        const float x = jshadow_to_f32(v);
        CHECK(fabsl((long double)x - (long double)v / 4294967296.0L) <= 5.9604644775390625e-08L + (long double)ulp(x) / 2);
    }
}

static void erf_checks() {
    long double worst = 0.0L;
    float prev = 0.0f;
    uint32_t bits;
    const float top = 4.5f;
    uint32_t top_bits;
    memcpy(&top_bits, &top, 4);
    for (bits = 0u; bits <= top_bits; bits += 64u) {
        float z;
        memcpy(&z, &bits, 4);
        const float g = jshadow_erf(z);
        const long double e = fabsl((long double)g - erfl((long double)z));
        worst = e > worst ? e : worst;
        CHECK(g >= prev && g <= 1.0f);
        CHECK(jshadow_erf(-z) == -g);
        prev = g;
    }
    CHECK(worst <= 1.9073486328125e-06L);  // 2^-19 on erf: 2^-20 on Phi
    const float half = 0.5f, one = 1.0f;
    uint32_t lo_bits, hi_bits;
    memcpy(&lo_bits, &half, 4);
    memcpy(&hi_bits, &one, 4);
    prev = jshadow_erf(half);
    uint32_t inversions = 0u;
    for (bits = lo_bits; bits <= hi_bits; bits++) {
        float z;
        memcpy(&z, &bits, 4);
        const float g = jshadow_erf(z);
        inversions += g < prev ? 1u : 0u;
        prev = g;
    }
    CHECK(inversions == 0u);
    CHECK(jshadow_erf(4.0f) == 1.0f && jshadow_erf(-4.0f) == -1.0f && jshadow_erf(1e30f) == 1.0f && jshadow_erf(-INFINITY) == -1.0f);
    CHECK(jshadow_erf(0.0f) == 0.0f && jshadow_erf(1e-40f) >= 0.0f);
    printf("G: worst |G - erf| %.3Le\n", worst);
}

static void legality() {
    const struct { jh_shadow_desc legal, illegal; const char* why; } rows[] = {
        {desc(0, 0, 3.4e38f, 1, 0, 1), desc(0, 0, INFINITY, 1, 0, 1), "the box is not finite"},
        {desc(0, 0, 1, 1, 0, 1), desc(0, NAN, 1, 1, 0, 1), "the box is not finite"},
        {desc(2, 0, 2, 1, 0, 1), desc(2, 0, 1.9999999f, 1, 0, 1), "the box has x1 < x0 or y1 < y0"},
        {desc(0, 5, 1, 5, 0, 1), desc(0, 5, 1, 4.9999995f, 0, 1), "the box has x1 < x0 or y1 < y0"},
        {desc(-4194304.0f, 0, 4194304.0f, 1, 0, 1), desc(-4194304.5f, 0, 1, 1, 0, 1), "a box coordinate above 2^22"},
        {desc(0, 0, 1, 4194304.0f, 0, 1), desc(0, 0, 1, 4194304.5f, 0, 1), "a box coordinate above 2^22"},
        {desc(0, 0, 1, 1, 0.0f, 1), desc(0, 0, 1, 1, -1e-45f, 1), "the radius is negative or not finite"},
        {desc(0, 0, 1, 1, 3.4e38f, 1), desc(0, 0, 1, 1, INFINITY, 1), "the radius is negative or not finite"},
        {desc(0, 0, 1, 1, 0, 0.0f), desc(0, 0, 1, 1, 0, -1e-45f), "sigma is outside [0, 2^16] or not finite"},
        {desc(0, 0, 1, 1, 0, 65536.0f), desc(0, 0, 1, 1, 0, 65536.008f), "sigma is outside [0, 2^16] or not finite"},
        {desc(0, 0, 1, 1, 0, 1), desc(0, 0, 1, 1, 0, NAN), "sigma is outside [0, 2^16] or not finite"},
    };
    for (const auto& r : rows) {
        jh_shad_plan p;
        memset(&p, 0xA5, sizeof p);
        jh_shad_plan before = p;
        // (the first row's legal side has a coordinate above 2^22: legal for the finiteness check alone)
        CHECK(!is(jshadow_desc_error(&r.legal), r.why));
        CHECK(is(jshadow_desc_error(&r.illegal), r.why));
        CHECK(is(jshadow_plan(&r.illegal, &p), r.why) && memcmp(&p, &before, sizeof p) == 0);
        uint32_t rect[4] = {7u, 7u, 7u, 7u};
        CHECK(is(jshadow_bounds(&r.illegal, 10u, 10u, rect), r.why) && rect[0] == 7u && rect[3] == 7u);
    }
    jh_shadow_desc d = desc(0, 0, 1, 1, 0, 1);
    d.flags = 3u;
    CHECK(!jshadow_desc_error(&d));
    d.flags = 4u;
    CHECK(is(jshadow_desc_error(&d), "unknown flag bits"));
    d.flags = 0u;
    d.matrix[0] = 0.0;
    jh_shad_plan p;
    CHECK(is(jshadow_plan(&d, &p), "the determinant is 0"));
    uint32_t rect[4];
    d.matrix[0] = 1.0;
    CHECK(!jshadow_bounds(&d, JSHADOW_MAX_EXTENT, JSHADOW_MAX_EXTENT, rect));
    CHECK(is(jshadow_bounds(&d, JSHADOW_MAX_EXTENT + 1u, 1u, rect), "an image extent above 2^23") && is(jshadow_bounds(&d, 1u, JSHADOW_MAX_EXTENT + 1u, rect), "an image extent above 2^23"));
}

static void bounds() {
    uint32_t r[4];
    jh_shadow_desc d = desc(100, 50, 400, 250, 10, 8);  // grown by 29: 71 .. 429, 21 .. 279; - 1 and + 1
    CHECK(!jshadow_bounds(&d, 4096u, 4096u, r) && r[0] == 70u && r[1] == 20u && r[2] == 360u && r[3] == 260u);
    CHECK(!jshadow_bounds(&d, 300u, 100u, r) && r[0] == 70u && r[1] == 20u && r[2] == 230u && r[3] == 80u);
    CHECK(!jshadow_bounds(&d, 60u, 4096u, r) && r[0] == 0u && r[1] == 0u && r[2] == 0u && r[3] == 0u);  // wholly outside
    d = desc(5, 5, 5, 9, 0, 1);
    CHECK(!jshadow_bounds(&d, 64u, 64u, r) && r[2] == 0u && r[3] == 0u);  // empty in a dimension: S = 0
    // brute force: every texel outside the rectangle is below 2^-12
    const double mats[][6] = {{1, 0, 0, 1, 0, 0}, {1, 0, 0, 1, 0.5, -0.25}, {0.8660254037844387, 0.5, -0.5, 0.8660254037844387, 12, -3}, {-1, 0, 0, 1, 40, 0}, {2, 0, 0, 0.5, -5, 3}};
    const float cfg[][6] = {{10, 8, 30, 20, 0, 0.5f}, {10, 8, 30, 20, 4, 2}, {12, 12, 24, 24, 6, 1}, {-5, -5, 8, 50, 3, 3}, {15, 10, 15.5f, 10.25f, 1, 0.001f}, {0, 0, 40, 30, 20, 6}};
    uint32_t outside = 0u;
    for (const auto& m : mats)
        for (const auto& c : cfg) {
            d = desc(c[0], c[1], c[2], c[3], c[4], c[5]);
            memcpy(d.matrix, m, sizeof d.matrix);
            jh_shad_plan p;
            CHECK(!jshadow_plan(&d, &p) && !jshadow_bounds(&d, 56u, 48u, r));
            for (uint32_t Y = 0; Y < 48u; Y++)
                for (uint32_t X = 0; X < 56u; X++) {
                    if (X >= r[0] && X < r[0] + r[2] && Y >= r[1] && Y < r[1] + r[3]) continue;
                    outside++;
                    CHECK(jshadow_texel(&p, X, Y) < 0.000244140625f);
                }
        }
    CHECK(outside > 1000u);
}

static void consequences() {
    jh_shadow_desc d = desc(-40, -25, 40, 25, 9, 2);
    d.matrix[4] = 50.0; d.matrix[5] = 30.0;  // the centre at texel corner (50, 30): texels X and 99 - X mirror each other
    jh_shad_plan p;
    CHECK(!jshadow_plan(&d, &p));
    CHECK(jshadow_texel(&p, 50u, 30u) == 1.0f && jshadow_texel(&p, 0u, 0u) == 0.0f);
    float worst_y = 0.0f;
    for (uint32_t Y = 0; Y < 60u; Y++)
        for (uint32_t X = 0; X < 50u; X++) {
            const float s = jshadow_texel(&p, X, Y);
            CHECK(s >= 0.0f && s <= 1.0f);
            CHECK(s == jshadow_texel(&p, 99u - X, Y));
            worst_y = fmaxf(worst_y, fabsf(s - jshadow_texel(&p, X, 59u - Y)));
        }
    CHECK(worst_y <= 4.0f * 5.9604644775390625e-08f * 16.0f);  // (the caps add in the other order: rounding only)
}

int main(int argc, char** argv) {
    if (argc == 15) {
        jh_shadow_desc d = desc(strtof(argv[1], nullptr), strtof(argv[2], nullptr), strtof(argv[3], nullptr), strtof(argv[4], nullptr), strtof(argv[5], nullptr), strtof(argv[6], nullptr));
        for (int i = 0; i < 6; i++) d.matrix[i] = strtod(argv[7 + i], nullptr);
        jh_shad_plan p;
        if (const char* why = jshadow_plan(&d, &p)) { printf("refused: %s\n", why); return 2; }
        const uint32_t w = (uint32_t)atoi(argv[13]), h = (uint32_t)atoi(argv[14]);
        for (uint32_t Y = 0; Y < h; Y++) {
            for (uint32_t X = 0; X < w; X++) {
                const float s = jshadow_texel(&p, X, Y);
                uint32_t bits;
                memcpy(&bits, &s, 4);
                printf("%08x ", bits);
            }
            printf("\n");
        }
        return 0;
    }
    plans();
    erf_checks();
    legality();
    bounds();
    consequences();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok: plan, G, legality, bounds, consequences\n");
    return 0;
}
