// warp_taps.h -- the device half of the warp rule from the source position on, which jh_warp and
// jh_displace share word for word: the taps and weights of each axis, each tap index resolved against the source rectangle by the
// edge mode (axis_taps), the direct 8-byte tap loads, the sums (rows, then columns, single fmaf's) and the store (tap_sum).
// kernels_warp.hip gives axis_taps the plan's position, kernels_displace.hip the plan's plus the map's offset.  k_warp keeps tap_sum's
// loop written out: called as a helper it changes that kernel's instructions, and a change of one is a change of both.
// The host half is include/jello_warp.h.  Every function is internal to the file that includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_warp.h"
#include "texel_io.h"

namespace {

template <int FILTER>
struct Taps { static constexpr int N = FILTER == JWARP_NEAREST ? 1 : (FILTER == JWARP_BILINEAR ? 2 : 4); };

// The taps of one axis at position U against the extent n: weights, the indices to load (always inside [0, n)) and whether the
// operand is the loaded texel (false: ZERO's +0).
template <int FILTER, int EDGE>
JD void axis_taps(int64_t U, int32_t n, float (&w)[Taps<FILTER>::N], int32_t (&idx)[Taps<FILTER>::N], bool (&live)[Taps<FILTER>::N]) {
    constexpr int N = Taps<FILTER>::N;
    int32_t i0;
    if (FILTER == JWARP_NEAREST) {
        i0 = jwarp_nearest(U);
        w[0] = 1.0f;
    } else {
        float f;
        i0 = jwarp_split(U, &f);
        if (FILTER == JWARP_BILINEAR) {
            w[0] = 1.0f - f;
            w[N - 1] = f;
        } else {
            float c[4];
            jwarp_cubic_weights(f, c);
#pragma unroll
            for (int k = 0; k < N; k++) w[k] = c[k];
            i0 -= 1;
        }
    }
    if (EDGE == JWARP_EDGE_ZERO || EDGE == JWARP_EDGE_CLAMP) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int32_t i = i0 + k;
            live[k] = EDGE == JWARP_EDGE_CLAMP || (i >= 0 && i < n);
            idx[k] = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
        }
    } else {
        const int32_t period = EDGE == JWARP_EDGE_REPEAT ? n : 2 * n;
        int32_t m = jwarp_mod(i0, period);
#pragma unroll
        for (int k = 0; k < N; k++) {
            live[k] = true;
            idx[k] = (EDGE == JWARP_EDGE_REPEAT || m < n) ? m : 2 * n - 1 - m;
            m = m + 1 == period ? 0 : m + 1;
        }
    }
}

// The texel the rule stores for the taps of the two axes (axis_taps of U against the source rectangle's width, of V against its
// height): src is the rectangle's first texel (null: never written, transparent black), src_w the texels to a row of its image.  The
// loads of a lane are unconditional (a tap ZERO takes out reads the rectangle's nearest texel and is replaced by +0 afterwards), so
// all of them can be in flight together.
template <int FILTER, int EDGE, bool STRAIGHT>
JD uint2 tap_sum(const uint2* src, uint32_t src_w, const float (&wx)[Taps<FILTER>::N], const int32_t (&ix)[Taps<FILTER>::N], const bool (&lx)[Taps<FILTER>::N],
                 const float (&wy)[Taps<FILTER>::N], const int32_t (&iy)[Taps<FILTER>::N], const bool (&ly)[Taps<FILTER>::N]) {
    constexpr int N = Taps<FILTER>::N;
    uint2 t[N][N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint2* srow = src + (uint64_t)(uint32_t)iy[j] * src_w;
#pragma unroll
        for (int i = 0; i < N; i++) {
            t[j][i] = make_uint2(0u, 0u);
            if (src) t[j][i] = srow[ix[i]];
            if (EDGE == JWARP_EDGE_ZERO && !(lx[i] && ly[j])) t[j][i] = make_uint2(0u, 0u);
        }
    }
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < N; j++) {
        float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int i = 0; i < N; i++) fma4(h, wx[i], texel_widen<STRAIGHT>(t[j][i]));
        fma4(v, wy[j], h);
    }
    return texel_store<STRAIGHT>(v);
}

}  // namespace
