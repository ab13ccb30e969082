// displace_check.cpp -- include/jello_displace.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/displace_check.cpp -o /tmp/displace_check && /tmp/displace_check
//
// Four things.  (1) jdisp_offset over all 65 536 f16 bit patterns x a list of scales against the rule worked in long double and
// __int128: t = m - 0.5 exact (checked: the binary32 difference equals the long double one), d = the binary32 product -- the exact
// product of two binary32 rounded half to even on its own integer mantissa, not the compiler's multiplication --, a NaN 0, the clamp,
// d 2^32 rounded half to even in __int128.  (2) The clamp from both sides: 2^22 and its binary32 neighbours, -2^22 likewise, +-Inf,
// +-FLT_MAX.  (3) NaN -> 0: every NaN pattern, and 0 x Inf in both orders.  (4) The legality boundaries of jdisp_desc_error, each from
// both sides, the reason named.  Prints "ok" and returns 0.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "jello_displace.h"

typedef __int128 i128;

// The value of an f16 bit pattern, written out here (not the header's widening).
static long double half_value(uint16_t h, bool* nan) {
    const int e = (h >> 10) & 31, m = h & 1023;
    *nan = e == 31 && m != 0;
    long double v;
    if (e == 0) v = ldexpl((long double)m, -24);
    else if (e == 31) v = INFINITY;
    else v = ldexpl((long double)(1024 + m), e - 25);
    return (h & 0x8000) ? -v : v;
}

// a b rounded to binary32, half to even, from the exact product (48 bits: exact in long double's 64)
static float product32(float a, float b) {
    const long double p = (long double)a * (long double)b;  // exact
    if (p != p || isinf(p) || p == 0.0L) return (float)p;
    int e;
    const long double m = frexpl(fabsl(p), &e);  // |p| = m 2^e, 0.5 <= m < 1
    int keep = 24;
    if (e - 1 < -126) keep = 24 - (-126 - (e - 1));  // a subnormal result keeps fewer bits
    if (keep < 0) return p < 0 ? -0.0f : 0.0f;   // (below half the smallest subnormal)
    const long double scaled = ldexpl(m, keep);  // the kept bits before the point
    long double r = floorl(scaled);
    const long double rem = scaled - r;
    if (rem > 0.5L || (rem == 0.5L && fmodl(r, 2.0L) == 1.0L)) r += 1.0L;
    const long double v = ldexpl(r, e - keep);
    return (float)(p < 0 ? -v : v);  // exact: at most 24 bits (an overflow to Inf is the conversion's)
}

static i128 rint_scaled(long double d) {  // d 2^32 half to even; |d| <= 2^22, d a binary32
    const long double s = ldexpl(d, 32);  // exact
    long double r = floorl(s);
    const long double rem = s - r;
    if (rem > 0.5L || (rem == 0.5L && fmodl(fabsl(r), 2.0L) == 1.0L)) r += 1.0L;
    return (i128)r;
}

static i128 rule(float scale, uint16_t h) {
    bool nan;
    const long double m = half_value(h, &nan);
    if (nan) return 0;
    const long double t = m - 0.5L;  // exact
    float d = product32(scale, (float)t);
    if (d != d) return 0;
    if (d > 4194304.0f) d = 4194304.0f;
    if (d < -4194304.0f) d = -4194304.0f;
    return rint_scaled((long double)d);
}

static const float kScales[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 20.0f, -7.3f, 256.0f, 1e-3f, 3.14159274f, 1e30f, -1e30f, 8388608.0f, 8388609.0f, -8388608.0f,
                                128.06f, 1e-30f, 1e-44f, 2.3283064e-10f, 2.3841858e-07f, 7.1525574e-07f, FLT_MAX, -FLT_MAX, 4194304.0f, 65.0078125f, INFINITY,
                                -INFINITY};

static int check_offsets() {
    for (float scale : kScales)
        for (uint32_t h = 0; h < 65536u; h++) {
            bool nan;
            const long double m = half_value((uint16_t)h, &nan);
            if (!nan && !isinf(m) && (long double)(jdisp_f16((uint16_t)h) - 0.5f) != m - 0.5L) {
                fprintf(stderr, "t is not exact for %#06x\n", h);
                return 1;
            }
            const int64_t got = jdisp_offset(scale, (uint16_t)h);
            const i128 want = rule(scale, (uint16_t)h);
            if ((i128)got != want) {
                fprintf(stderr, "offset(%a, %#06x) = %lld, the rule gives %lld\n", (double)scale, h, (long long)got, (long long)want);
                return 1;
            }
            if (got > ((int64_t)1 << 54) || got < -((int64_t)1 << 54)) return 1;
        }
    return 0;
}

static int check_clamp_and_nan() {
    const int64_t top = (int64_t)1 << 54;
    // t = 0.5 (m = 1.0): d = scale / 2
    const float at = 8388608.0f, above = nextafterf(at, INFINITY), below = nextafterf(at, 0.0f);
    if (jdisp_offset(at, 0x3c00) != top || jdisp_offset(above, 0x3c00) != top || jdisp_offset(below, 0x3c00) != top - ((int64_t)1 << 30)) return 1;
    if (jdisp_offset(-at, 0x3c00) != -top || jdisp_offset(-above, 0x3c00) != -top || jdisp_offset(-below, 0x3c00) != -top + ((int64_t)1 << 30)) return 1;
    if (jdisp_offset(1.0f, 0x7c00) != top || jdisp_offset(1.0f, 0xfc00) != -top || jdisp_offset(-1e-30f, 0x7c00) != -top) return 1;
    if (jdisp_offset(FLT_MAX, 0x7bff) != top || jdisp_offset(FLT_MAX, 0xfbff) != -top || jdisp_offset(INFINITY, 0x3c00) != top) return 1;
    // NaN -> 0
    for (uint32_t h = 0x7c01; h < 0x8000u; h++)
        if (jdisp_offset(3.0f, (uint16_t)h) != 0 || jdisp_offset(3.0f, (uint16_t)(h | 0x8000u)) != 0) return 1;
    if (jdisp_offset(0.0f, 0x7c00) != 0 || jdisp_offset(-0.0f, 0xfc00) != 0 || jdisp_offset(INFINITY, 0x3800) != 0 || jdisp_offset(NAN, 0x3c00) != 0) return 1;
    // the rounding of D: t = 2^-11 times 2^-22 is one half of 2^-32 (to even: 0), times 3 x 2^-22 three halves (to even: 2)
    const float q = 2.3841858e-07f;  // 2^-22
    if (jdisp_offset(q, 0x3801) != 0 || jdisp_offset(3.0f * q, 0x3801) != 2 || jdisp_offset(-3.0f * q, 0x3801) != -2 || jdisp_offset(5.0f * q, 0x3801) != 2) return 1;
    return 0;
}

static int check_legality() {
    const struct { int filter, edge; uint32_t flags; float sx, sy; int cx, cy; uint32_t sw, sh, mw, mh, dw, dh; const char* word; } rows[] = {
        {0, 0, 0u, 0.0f, 0.0f, 0, 0, 1u, 1u, 1u, 1u, 1u, 1u, nullptr},
        {2, 3, 1u, -FLT_MAX, FLT_MAX, 3, 3, 32768u, 32768u, 32768u, 32768u, 32768u, 32768u, nullptr},
        {3, 0, 0u, 1.0f, 1.0f, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "filter"},
        {-1, 0, 0u, 1.0f, 1.0f, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "filter"},
        {0, 4, 0u, 1.0f, 1.0f, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "edge"},
        {0, -1, 0u, 1.0f, 1.0f, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "edge"},
        {0, 0, 2u, 1.0f, 1.0f, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "flag"},
        {0, 0, 0u, 1.0f, 1.0f, 4, 1, 8u, 8u, 8u, 8u, 8u, 8u, "channel"},
        {0, 0, 0u, 1.0f, 1.0f, 0, -1, 8u, 8u, 8u, 8u, 8u, 8u, "channel"},
        {0, 0, 0u, INFINITY, 1.0f, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "not finite"},
        {0, 0, 0u, 1.0f, -INFINITY, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "not finite"},
        {0, 0, 0u, 1.0f, NAN, 0, 1, 8u, 8u, 8u, 8u, 8u, 8u, "not finite"},
        {0, 0, 0u, 1.0f, 1.0f, 0, 1, 8u, 8u, 9u, 8u, 8u, 8u, "map"},
        {0, 0, 0u, 1.0f, 1.0f, 0, 1, 8u, 8u, 8u, 7u, 8u, 8u, "map"},
        {0, 0, 0u, 1.0f, 1.0f, 0, 1, 32769u, 8u, 8u, 8u, 8u, 8u, "32768"},
        {0, 0, 0u, 1.0f, 1.0f, 0, 1, 8u, 8u, 8u, 32769u, 8u, 32769u, "32768"},
    };
    for (const auto& r : rows) {
        const char* why = jdisp_desc_error(r.filter, r.edge, r.flags, r.sx, r.sy, r.cx, r.cy, r.sw, r.sh, r.mw, r.mh, r.dw, r.dh);
        if ((why == nullptr) != (r.word == nullptr) || (why && !strstr(why, r.word))) {
            fprintf(stderr, "legality: got \"%s\", expected \"%s\"\n", why ? why : "legal", r.word ? r.word : "legal");
            return 1;
        }
    }
    return 0;
}

int main() {
    if (check_offsets()) { fprintf(stderr, "offsets failed\n"); return 1; }
    if (check_clamp_and_nan()) { fprintf(stderr, "clamp / NaN failed\n"); return 1; }
    if (check_legality()) { fprintf(stderr, "legality failed\n"); return 1; }
    printf("ok: %zu scales x 65536 bit patterns, the clamp, NaN, legality\n", sizeof(kScales) / sizeof(kScales[0]));
    return 0;
}
