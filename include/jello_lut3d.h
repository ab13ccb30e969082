// jello_lut3d.h -- the 3D colour lookup rule (DESIGN.md 5.23 "LUT rule"): an N x N x N table of colours, held as an RGBA16F image,
// applied to the texels of an RGBA16F image by tetrahedral interpolation.  Which descriptor is legal, and -- the one text the kernel
// (jello_amd/csrc/kernels_lut3d.hip), the library's queries and their host twin (include/jello_queries.h) and the stand-alone check
// (tools/lut3d_check.cpp) all compile -- the position, the walk and the sum.  tests/lut3d_ref.py restates the rule from the text
// below and includes nothing of this file.
//
//   the LUT   an RGBA16F image N texels wide and N^2 high, 2 <= N <= 65.  Entry (i, j, k) -- indexed by (red, green, blue) -- is the
//             texel (x = i, y = j + N k): red varies fastest, the .cube order.  Its r, g, b are the output colour for the input
//             (i, j, k) / (N - 1); its alpha is ignored.  A never-written LUT reads as zeros.
//   per texel binary32, nothing contracted but the stated fmaf; h_c is the stored (un-premultiplied) f16 of channel c, widened
//     clamp     c = h > 0 ? h : 0; c = c < 1 ? c : 1 -- compare and select: NaN and -0 become +0
//     position  p = c (N - 1), k = min((int)p, N - 2), f = p - (float)k.  Every operation is exact for every f16 h and every legal
//               N, and so are 1 - f and the differences of two fractions: the weights below sum to exactly 1.
//     walk      from V0 = (k_r, k_g, k_b) one step of +1 along one axis at a time, in descending order of the fractions, to V1, V2
//               and V3 = (k_r + 1, k_g + 1, k_b + 1); ties go r before g before b: the stable sort decided by f_r >= f_g,
//               f_r >= f_b, f_g >= f_b.  With f1 >= f2 >= f3 in that order  w0 = 1 - f1, w1 = f1 - f2, w2 = f2 - f3, w3 = f3.
//     sum       per colour channel  m = w0 V0.c; m = fmaf(w1, V1.c, m); m = fmaf(w2, V2.c, m); m = fmaf(w3, V3.c, m).  A zero weight
//               is multiplied, not skipped: 0 x Inf is NaN.
//     store     f16(m), round to nearest even; a NaN result is any NaN.  Alpha is the source's bit pattern, copied.
#pragma once
#include <stdint.h>

#include "jello_color.h"  // jcolor_f16_value, jcolor_f16_bits: f16 on the host
#include "jello_image.h"

#if defined(__HIPCC__)
#define JLUT_HD __host__ __device__ __forceinline__
#else
#define JLUT_HD static inline
#endif

#define JLUT_MIN_SIZE 2u
#define JLUT_MAX_SIZE 65u
#define JLUT_STAGED_MAX_SIZE 17u  // the largest table the kernel copies into LDS: 17^3 x 8 B = 39 304 B

// ---- the pieces ----

JLUT_HD float jlut_widen(uint32_t h) {  // the value of an f16 bit pattern, exactly
#if defined(__HIP_DEVICE_COMPILE__)
    union { uint16_t u; _Float16 h; } c;
    c.u = (uint16_t)h;
    return (float)c.h;
#else
    return (float)jcolor_f16_value(h & 0xffffu);
#endif
}
// binary32 to f16 bits, round to nearest even: the hardware's conversion on the device, jello_color.h's on the host (the widening
// to binary64 is exact, so it is one rounding too).  The device's value passes through an empty asm first: the compiler otherwise
// folds the last fmaf, whose table operand is a widened f16, and this conversion into one v_fma_mixlo_f16, and gfx950 rounds that
// instruction ONCE, from the exact sum to f16 -- not the binary32 fmaf rounded again, which is the rule (they differ where the
// binary32 sum is a tie of two f16: one texel in 2^18 on the battery).
JLUT_HD uint32_t jlut_f16(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(v));  // (not volatile: it may move, so the two texels of a lane keep their loads together)
    union { uint16_t u; _Float16 h; } c;
    c.h = (_Float16)v;
    return c.u;
#else
    return jcolor_f16_bits((double)v);
#endif
}

// Steps 1 and 2 for one channel: the cell index k in [0, N - 2] and the fraction f in [0, 1] of the f16 bit pattern h under
// nm1 = N - 1.
JLUT_HD void jlut_position(uint32_t h, uint32_t nm1, uint32_t* k, float* f) {
    float c = jlut_widen(h);
    c = c > 0.0f ? c : 0.0f;
    c = c < 1.0f ? c : 1.0f;
    const float p = c * (float)nm1;
    int32_t i = (int32_t)p;
    i = i < (int32_t)nm1 - 1 ? i : (int32_t)nm1 - 1;
    *k = (uint32_t)i;
    *f = p - (float)i;
}

// Step 3: from the fractions f[0..2] of (r, g, b) and the step each axis makes in the table (s[0..2], any unit), the steps in the
// order they are taken, o[0..2], and the weights w[0..3] of V0, V1 = V0 + o[0], V2 = V1 + o[1], V3 = V2 + o[2].  Compare and select
// only: the place of each axis in the order is a sum of the three comparisons.
JLUT_HD void jlut_walk(const float* f, const uint32_t* s, uint32_t* o, float* w) {
    const uint32_t rg = f[0] >= f[1] ? 1u : 0u, rb = f[0] >= f[2] ? 1u : 0u, gb = f[1] >= f[2] ? 1u : 0u;
    const uint32_t place_r = 2u - rg - rb, place_g = rg + 1u - gb;  // (place_b = rb + gb: the one that is left)
    const float f1 = place_r == 0u ? f[0] : (place_g == 0u ? f[1] : f[2]);
    const float f2 = place_r == 1u ? f[0] : (place_g == 1u ? f[1] : f[2]);
    const float f3 = place_r == 2u ? f[0] : (place_g == 2u ? f[1] : f[2]);
    o[0] = place_r == 0u ? s[0] : (place_g == 0u ? s[1] : s[2]);
    o[1] = place_r == 1u ? s[0] : (place_g == 1u ? s[1] : s[2]);
    o[2] = place_r == 2u ? s[0] : (place_g == 2u ? s[1] : s[2]);
    w[0] = 1.0f - f1;
    w[1] = f1 - f2;
    w[2] = f2 - f3;
    w[3] = f3;
}

// Steps 1 to 3 for a texel (x = g << 16 | r, y = a << 16 | b) and a table of n: the four entry indices (x + n (y' + n z')) and the weights.
JLUT_HD void jlut_vertices(uint32_t x, uint32_t y, uint32_t n, uint32_t* index, float* w) {
    uint32_t k[3], o[3];
    float f[3];
    jlut_position(x & 0xffffu, n - 1u, &k[0], &f[0]);
    jlut_position(x >> 16, n - 1u, &k[1], &f[1]);
    jlut_position(y & 0xffffu, n - 1u, &k[2], &f[2]);
    const uint32_t s[3] = {1u, n, n * n};
    jlut_walk(f, s, o, w);
    index[0] = k[0] + n * (k[1] + n * k[2]);
    index[1] = index[0] + o[0];
    index[2] = index[1] + o[1];
    index[3] = index[2] + o[2];
}

// Steps 4 and 5: the texel from the weights, the four entries (vx[i] = g << 16 | r, vy[i] = a << 16 | b of Vi) and the source's y word.
JLUT_HD void jlut_sum(const float* w, const uint32_t* vx, const uint32_t* vy, uint32_t src_y, uint32_t* ox, uint32_t* oy) {
    float m[3];
    m[0] = w[0] * jlut_widen(vx[0] & 0xffffu);
    m[1] = w[0] * jlut_widen(vx[0] >> 16);
    m[2] = w[0] * jlut_widen(vy[0] & 0xffffu);
    for (int i = 1; i < 4; i++) {
        m[0] = __builtin_fmaf(w[i], jlut_widen(vx[i] & 0xffffu), m[0]);
        m[1] = __builtin_fmaf(w[i], jlut_widen(vx[i] >> 16), m[1]);
        m[2] = __builtin_fmaf(w[i], jlut_widen(vy[i] & 0xffffu), m[2]);
    }
    *ox = jlut_f16(m[0]) | (jlut_f16(m[1]) << 16);
    *oy = jlut_f16(m[2]) | (src_y & 0xffff0000u);
}

// ---- the host half ----

// nullptr for a legal size and flags, else what is wrong (the rectangle: jimage_rect_check; the LUT image's size: jlut_image_error).
static inline const char* jlut_check(uint32_t size, uint32_t flags) {
    if (size < JLUT_MIN_SIZE || size > JLUT_MAX_SIZE) return "size outside 2..65";
    if (flags != 0u) return "unknown flag bits";
    return nullptr;
}
// The image of a table of `size` is size texels wide and size^2 high.
static inline const char* jlut_image_error(uint32_t size, uint32_t image_w, uint32_t image_h) {
    return image_w == size && image_h == size * size ? nullptr : "the LUT image is not size x size^2";
}

// The rule on one texel over a host table: lut holds n^3 entries of four f16 bit patterns (r, g, b, a), in[4] and out[4] likewise.
static inline void jlut_texel(uint32_t n, const uint16_t* lut, const uint16_t* in, uint16_t* out) {
    uint32_t index[4], vx[4], vy[4], ox, oy;
    float w[4];
    jlut_vertices((uint32_t)in[0] | ((uint32_t)in[1] << 16), (uint32_t)in[2] | ((uint32_t)in[3] << 16), n, index, w);
    for (int i = 0; i < 4; i++) {
        const uint16_t* e = lut + 4u * (size_t)index[i];
        vx[i] = (uint32_t)e[0] | ((uint32_t)e[1] << 16);
        vy[i] = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
    }
    jlut_sum(w, vx, vy, (uint32_t)in[3] << 16, &ox, &oy);
    out[0] = (uint16_t)(ox & 0xffffu); out[1] = (uint16_t)(ox >> 16); out[2] = (uint16_t)(oy & 0xffffu); out[3] = (uint16_t)(oy >> 16);
}

// The identity table of n: entry (i, j, k) = (f16(i / (n - 1)), f16(j / (n - 1)), f16(k / (n - 1)), 1.0), each rounded once from
// binary64; out holds n^3 entries of four f16 bit patterns.
static inline void jlut_identity(uint32_t n, uint16_t* out) {
    uint16_t v[JLUT_MAX_SIZE];
    for (uint32_t i = 0; i < n; i++) v[i] = jcolor_f16_bits((double)i / (double)(n - 1u));
    for (uint32_t k = 0; k < n; k++)
        for (uint32_t j = 0; j < n; j++)
            for (uint32_t i = 0; i < n; i++) {
                uint16_t* e = out + 4u * ((size_t)i + n * ((size_t)j + n * (size_t)k));
                e[0] = v[i]; e[1] = v[j]; e[2] = v[k]; e[3] = 0x3c00u;
            }
}

// The batch queries' bodies.
static inline const char* jlut_identity_query(uint32_t n, uint16_t* out) {
    if (const char* why = jlut_check(n, 0u)) return why;
    jlut_identity(n, out);
    return nullptr;
}
static inline const char* jlut_texels(uint32_t n, const uint16_t* lut, const uint16_t* in, uint64_t count, uint16_t* out) {
    if (const char* why = jlut_check(n, 0u)) return why;
    for (uint64_t i = 0; i < count; i++) jlut_texel(n, lut, in + 4u * i, out + 4u * i);
    return nullptr;
}
