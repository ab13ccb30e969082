// blit_convert.h -- the per-pixel conversion rule shared by jh_blit (kernels_surface.hip) and jh_blit_yuv (kernels_yuv.hip):
// premultiply in f32, clamp with NaN -> 0, then rint_f32(v * 255) or the sRGB threshold table (include/jello_hip.h, DESIGN.md
// "Surface blit").  Every function is internal to the file that includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dmath.h"
#include "srgb_encode_lut.h"

namespace {

// clamp to [0, 1] by comparisons: NaN (inf * 0 included) fails both and becomes 0, +inf becomes 1, -0 becomes +0
__device__ __forceinline__ float blit_clamp01(float p) {
    const float v = p > 0.0f ? p : 0.0f;
    return v < 1.0f ? v : 1.0f;
}

__device__ __forceinline__ uint32_t blit_unorm(float v) { return (uint32_t)__builtin_rintf(v * 255.0f); }

// sRGB code of v in [0, 1]: a hardware log2 / exp2 estimate of 255 enc(v) (the constants folded: 255 * 12.92, 255 * 1.055,
// 255 * 0.055; an fma is fine in an estimate), rounded -- within one code of the rule -- then corrected against the thresholds.  lut[u] = (threshold of
// code u, threshold of code u + 1) with code 0's threshold 0 and code 256's +inf: the code is the u with
// lut[u].x <= v < lut[u].y, one 8-B LDS read per channel.
__device__ __forceinline__ uint32_t blit_srgb(float v, const float2* lut) {
    const float e = v <= 0.0031308f ? v * 3294.6f
                                    : __builtin_fmaf(269.025f, __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(v) * (1.0f / 2.4f)), -14.025f);
    int u = (int)__builtin_rintf(e);
    u = u < 0 ? 0 : (u > 255 ? 255 : u);
    const float2 t = lut[u];
    return (uint32_t)(u - (v < t.x ? 1 : 0) + (v >= t.y ? 1 : 0));
}

// one RGBA16F texel (x = r | g << 16, y = b | a << 16, f16 bits) -> the surface's 4 bytes, byte 0 lowest
template <bool SRGB, bool BGRA>
__device__ __forceinline__ uint32_t blit_pixel(uint2 t, const float2* lut) {
    // (not jd::rgba16f_to_f32: alpha first -- with the four conversions in the helper's order the compiler reorders k_blit_yuv)
    const float a = jd::f16_to_f32((uint16_t)(t.y >> 16));
    const float r = blit_clamp01(jd::f16_to_f32((uint16_t)(t.x & 0xffffu)) * a);
    const float g = blit_clamp01(jd::f16_to_f32((uint16_t)(t.x >> 16)) * a);
    const float b = blit_clamp01(jd::f16_to_f32((uint16_t)(t.y & 0xffffu)) * a);
    const uint32_t ua = blit_unorm(blit_clamp01(a));
    uint32_t c0, c1, c2;
    if (SRGB) {
        c0 = blit_srgb(r, lut); c1 = blit_srgb(g, lut); c2 = blit_srgb(b, lut);
    } else {
        c0 = blit_unorm(r); c1 = blit_unorm(g); c2 = blit_unorm(b);
    }
    if (BGRA) { const uint32_t s = c0; c0 = c2; c2 = s; }
    return c0 | (c1 << 8) | (c2 << 16) | (ua << 24);
}

// The table blit_srgb reads, filled by the 256 threads of a block (i = threadIdx.x; the caller synchronises): entry i =
// (threshold of code i, threshold of code i + 1).
__device__ __forceinline__ void blit_srgb_lut_fill(float2* lut, uint32_t i) {
    lut[i] = make_float2(i == 0u ? 0.0f : kSrgbEncodeThreshold[i - 1u], i == 255u ? __builtin_huge_valf() : kSrgbEncodeThreshold[i]);
}

}  // namespace
