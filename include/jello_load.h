// jello_load.h -- the load rule (DESIGN.md 5.21 "Load rule"): 8-bit surfaces and 8-bit Y'CbCr 4:2:0 frames into RGBA16F images, the
// inverse of jh_blit and jh_blit_yuv.  Which descriptor is legal (rectangle: jello_image.h; frame: jello_frame.h), the coefficient rows, and -- the
// one text the kernels (jello_amd/csrc/kernels_load.hip), the library's queries and their host twin (include/jello_queries.h) and the
// stand-alone check (tools/load_check.cpp) all compile -- the chroma sum, the codes and the texel.  tests/load_ref.py restates the
// rule from the text below and includes nothing of this file.
//
//   texel     from four 8-bit codes (r, g, b, a) and a transfer:  U(c) = the binary32 nearest to c / 255 (= (float)c / 255.0f);
//             L(c) = kSrgbToLinear[c], the decode table of the fine kernel.  Colour = L(c) under an sRGB format or transfer, U(c)
//             otherwise; alpha is always U(a).
//               STRAIGHT        texel_pack(colour, U(a)): RGBA16F images hold straight colour
//               PREMULTIPLIED   texel_unpremultiply(colour, U(a)), the store rule of DESIGN.md 5.8 (what jh_blit writes is
//                               premultiplied); a = 0 under a non-zero colour gives large values or Inf, by that rule
//               OPAQUE          byte 3 is ignored, alpha is 1.0
//             BGRA formats swap bytes 0 and 2.  Under STRAIGHT and OPAQUE a channel is one of 256 f16 patterns per table
//             (jello_amd/csrc/load_decode_lut.h, tools/gen_load_tables.py).
//   chroma    planes are ceil(w / 2) x ceil(h / 2), sample (cx, cy) at luma position (2 cx + 1/2, 2 cy + 1/2) -- jh_blit_yuv's siting.
//             For the texel (x, y): cx0 = x >> 1, cx1 = clamp(cx0 + (x odd ? 1 : -1), 0, ceil(w / 2) - 1), cy0, cy1 the same in y.
//             The sum S is 16 x a code:  REPLICATE  S = 16 C[cy0][cx0]
//                                        BILINEAR   S = 9 C[cy0][cx0] + 3 C[cy0][cx1] + 3 C[cy1][cx0] + C[cy1][cx1]
//   codes     in integers, Y' = Y - o, u = S_cb - 2048, v = S_cr - 2048, >> arithmetic:
//               R = clamp8((16 Ky Y' + Krv v         + 2^19) >> 20)
//               G = clamp8((16 Ky Y' + Kgu u + Kgv v + 2^19) >> 20)
//               B = clamp8((16 Ky Y' + Kbu u         + 2^19) >> 20)
//             every sum stays below 6.0e8 in magnitude; the coefficients need 19 bits with their sign, the operands 13.
//   yuv texel the texel rule on (R, G, B, 255), transfer SRGB or NONE, straight: what jh_load_surface makes of those codes.
#pragma once
#include <stdint.h>
#include <string.h>

#include "jello_color.h"  // jcolor_f16_bits: binary64 to f16 on the host
#include "jello_frame.h"  // what a surface and a 4:2:0 frame are: formats, enums, planes, pitches, clamp8
#include "jello_image.h"

#if defined(__HIPCC__)
#define JLOAD_HD __host__ __device__ __forceinline__
#else
#define JLOAD_HD static inline
#endif
#define JLOAD_TABLE static constexpr
#include "../jello_amd/csrc/load_decode_lut.h"

// ---- the pieces ----

JLOAD_HD float jload_bits_f32(uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(bits);
#else
    float f;
    memcpy(&f, &bits, 4);
    return f;
#endif
}
// binary32 to f16 bits, round to nearest even: the hardware's conversion on the device, jello_color.h's on the host (the widening
// to binary64 is exact, so it is one rounding too).
JLOAD_HD uint16_t jload_f16(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    union { uint16_t u; _Float16 h; } c;
    c.h = (_Float16)v;
    return c.u;
#else
    return jcolor_f16_bits((double)v);
#endif
}
JLOAD_HD float jload_unorm(uint32_t c) { return (float)c / 255.0f; }                 // U(c)
JLOAD_HD float jload_linear(uint32_t c) { return jload_bits_f32(kLoadSrgbF32[c]); }  // L(c)

// A texel is the two words of an RGBA16F texel: x = g << 16 | r, y = a << 16 | b.  The codes (r, g, b, a) are in RGBA order: the
// caller has swapped a BGRA pixel's bytes 0 and 2.
// STRAIGHT and OPAQUE: every channel is an entry of a table of 256 f16 patterns -- `colour` is kLoadSrgbF16 or kLoadUnormF16 and
// `unorm` kLoadUnormF16, or a workgroup's copies of them.
JLOAD_HD void jload_texel_tables(const uint16_t* colour, const uint16_t* unorm, bool opaque, uint32_t r, uint32_t g, uint32_t b, uint32_t a, uint32_t* x,
                                 uint32_t* y) {
    *x = (uint32_t)colour[r] | ((uint32_t)colour[g] << 16);
    *y = (uint32_t)colour[b] | ((opaque ? 0x3c00u : (uint32_t)unorm[a]) << 16);
}
// PREMULTIPLIED, from the binary32 colour values (L or U of the codes) and av = U(a) -- the store rule: a_inv = 1 / max(a, 1e-6),
// f16(c * a_inv + 0.0f), f16(a + 0.0f), every operation rounded once.  Its home is texel_unpremultiply of jello_amd/csrc/texel_io.h,
// which is device code and which k_load_surface calls; this is the copy the host compiles (the queries, their twin, the stand-alone
// check).  tests/test_gpu_load.py compares the two on the device's output over every (code, alpha) pair of both transfers.
JLOAD_HD void jload_texel_premultiplied(float rv, float gv, float bv, float av, uint32_t* x, uint32_t* y) {
    const float a_inv = 1.0f / __builtin_fmaxf(av, 1e-6f);
    *x = (uint32_t)jload_f16(rv * a_inv + 0.0f) | ((uint32_t)jload_f16(gv * a_inv + 0.0f) << 16);
    *y = (uint32_t)jload_f16(bv * a_inv + 0.0f) | ((uint32_t)jload_f16(av + 0.0f) << 16);
}
// The texel rule whole, from the committed tables.
JLOAD_HD void jload_texel(bool srgb, int alpha, uint32_t r, uint32_t g, uint32_t b, uint32_t a, uint32_t* x, uint32_t* y) {
    if (alpha != JH_LOAD_ALPHA_PREMULTIPLIED)
        jload_texel_tables(srgb ? kLoadSrgbF16 : kLoadUnormF16, kLoadUnormF16, alpha == JH_LOAD_ALPHA_OPAQUE, r, g, b, a, x, y);
    else if (srgb)
        jload_texel_premultiplied(jload_linear(r), jload_linear(g), jload_linear(b), jload_unorm(a), x, y);
    else
        jload_texel_premultiplied(jload_unorm(r), jload_unorm(g), jload_unorm(b), jload_unorm(a), x, y);
}

// The second chroma column (row) a texel at x (y) of an axis with n chroma samples blends with: the neighbour on the texel's side
// of its own sample, the edge sample repeated.
JLOAD_HD uint32_t jload_chroma_other(uint32_t x, uint32_t n) {
    const uint32_t c0 = x >> 1;
    if (x & 1u) return c0 + 1u < n ? c0 + 1u : n - 1u;
    return c0 > 0u ? c0 - 1u : 0u;
}
// S of the four samples c00 = C[cy0][cx0], c01 = C[cy0][cx1], c10 = C[cy1][cx0], c11 = C[cy1][cx1].
JLOAD_HD int32_t jload_chroma_sum(int chroma, int32_t c00, int32_t c01, int32_t c10, int32_t c11) {
    return chroma == JH_CHROMA_BILINEAR ? 9 * c00 + 3 * c01 + 3 * c10 + c11 : 16 * c00;
}
JLOAD_HD int32_t jload_mul(int32_t a, int32_t b) {  // both operands within 24 bits with their sign, the product within 32
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}
// The codes of (Y, S_cb, S_cr) under the row k = {Ky, Krv, Kgu, Kgv, Kbu} and the luma offset `off`, as r | g << 8 | b << 16.
JLOAD_HD uint32_t jload_codes(const int32_t* k, int32_t off, int32_t y, int32_t s_cb, int32_t s_cr) {
    const int32_t u = s_cb - 2048, v = s_cr - 2048;
    const int32_t luma = jload_mul(k[0], 16 * (y - off)) + (1 << 19);
    const uint32_t r = jframe_clamp8((luma + jload_mul(k[1], v)) >> 20);
    const uint32_t g = jframe_clamp8((luma + jload_mul(k[2], u) + jload_mul(k[3], v)) >> 20);
    const uint32_t b = jframe_clamp8((luma + jload_mul(k[4], u)) >> 20);
    return r | (g << 8) | (b << 16);
}

// ---- the host half ----

static inline bool jload_alpha_ok(int alpha) { return alpha == JH_LOAD_ALPHA_STRAIGHT || alpha == JH_LOAD_ALPHA_PREMULTIPLIED || alpha == JH_LOAD_ALPHA_OPAQUE; }
// nullptr for a legal descriptor, else what is wrong with it -- its rectangle apart (jimage_rect_check) and its pitches, which are judged against that rectangle's width (jello_frame.h).
static inline const char* jload_surface_desc_error(const jh_load_surface_desc* d) {
    if (const char* why = jframe_surface_format_error(d->format)) return why;
    if (!jload_alpha_ok(d->alpha)) return "unknown alpha mode";
    if (!d->src) return "null src";
    return nullptr;
}
static inline const char* jload_yuv_desc_error(const jh_load_yuv_desc* d) {
    if (const char* why = jframe_yuv_enums_error(d->layout, d->matrix, d->range, d->transfer)) return why;
    if (d->chroma != JH_CHROMA_REPLICATE && d->chroma != JH_CHROMA_BILINEAR) return "unknown chroma filter";
    return jframe_yuv_planes_error(d->layout, d->plane, d->pitch, 0u, JFRAME_NULL_PLANE);
}

// The batch queries' bodies.  texels: `format_or_transfer` is a jh_surface_format, or 4 + a jh_yuv_transfer for RGBA codes under
// that transfer (what jh_load_yuv does with its codes); rgba: n pixels of 4 bytes in the format's order; out: 4 n f16 bit patterns.
static inline const char* jload_texels(int format_or_transfer, int alpha, uint64_t n, const uint8_t* rgba, uint16_t* out) {
    const bool transfer = format_or_transfer == 4 + JH_YUV_TRANSFER_NONE || format_or_transfer == 4 + JH_YUV_TRANSFER_SRGB;
    if (!transfer && !jframe_surface_format_ok(format_or_transfer)) return "unknown surface format or transfer";
    if (!jload_alpha_ok(alpha)) return "unknown alpha mode";
    const bool srgb = transfer ? format_or_transfer == 4 + JH_YUV_TRANSFER_SRGB : jframe_surface_srgb(format_or_transfer);
    const bool bgra = !transfer && jframe_surface_bgra(format_or_transfer);
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* p = rgba + 4u * i;
        uint32_t x, y;
        jload_texel(srgb, alpha, p[bgra ? 2 : 0], p[1], p[bgra ? 0 : 2], p[3], &x, &y);
        out[4u * i] = (uint16_t)(x & 0xffffu); out[4u * i + 1u] = (uint16_t)(x >> 16);
        out[4u * i + 2u] = (uint16_t)(y & 0xffffu); out[4u * i + 3u] = (uint16_t)(y >> 16);
    }
    return nullptr;
}
// y: n codes; s_cb, s_cr: n sums in [0, 4080]; rgb: 3 n codes out.
static inline const char* jload_yuv_codes(int matrix, int range, uint64_t n, const uint8_t* y, const uint16_t* s_cb, const uint16_t* s_cr, uint8_t* rgb) {
    if (jframe_yuv_enums_error(JH_YUV_NV12, matrix, range, JH_YUV_TRANSFER_NONE)) return "unknown matrix or range";
    for (uint64_t i = 0; i < n; i++)
        if (s_cb[i] > 4080u || s_cr[i] > 4080u) return "a chroma sum above 16 * 255";
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t c = jload_codes(kLoadYuv[matrix][range], kLoadYuvOffset[range], y[i], s_cb[i], s_cr[i]);
        rgb[3u * i] = (uint8_t)(c & 0xffu); rgb[3u * i + 1u] = (uint8_t)((c >> 8) & 0xffu); rgb[3u * i + 2u] = (uint8_t)(c >> 16);
    }
    return nullptr;
}
