// jello_blur.h -- the host half of the blur rule (DESIGN.md 5.7 "Blur rule"): which sigma is legal, the radius, and the taps of
// one axis, and the bytes of the intermediate.  Compiled by the library and the launcher (jello_amd/csrc/jello_hip.cpp:
// jh_blur; kernels_blur.hip: the intermediate), by the query both libraries compile (include/jello_queries.h: jq_blur_taps) and by tools/image_rect_check.cpp;
// tests/blur_ref.py restates it.  The device half -- the two fused-multiply-add sums over these taps -- is jello_amd/csrc/kernels_blur.hip.
//
//   sigma   given as binary32, used as binary64; legal: 0 <= sigma <= JBLUR_MAX_SIGMA (a NaN is not)
//   R       ceil(3 sigma) in binary64, so R <= JBLUR_MAX_RADIUS; sigma = 0: R = 0 and the single tap 1.0f
//   g_k     exp(-(double)(k k) / (2.0 sigma sigma)), k = 0..R: one libm exp per tap, the rule's only inexact library call
//   S       g_0 + 2 (g_1 + g_2 + ... + g_R), the bracket summed in that order in binary64
//   w_k     (float)(g_k / S), w_-k = w_k; stored as weights[k + R], 2R + 1 entries
#pragma once
#include <math.h>
#include <stdint.h>
#include "jello_image.h"

#define JBLUR_MAX_SIGMA 64.0f
#define JBLUR_MAX_RADIUS 192u

static inline bool jblur_sigma_ok(float sigma) { return sigma >= 0.0f && sigma <= JBLUR_MAX_SIGMA; }  // (false for a NaN)

// R of a legal sigma.
static inline uint32_t jblur_radius(float sigma) { return (uint32_t)ceil(3.0 * (double)sigma); }

// The 2R + 1 taps of a legal sigma into weights (which may be null: the radius alone).  Returns R.
static inline uint32_t jblur_taps(float sigma, float* weights) {
    const uint32_t R = jblur_radius(sigma);
    if (!weights) return R;
    if (R == 0u) {
        weights[0] = 1.0f;
        return 0u;
    }
    const double s = (double)sigma, den = 2.0 * s * s;
    double g[JBLUR_MAX_RADIUS + 1u];
    for (uint32_t k = 0; k <= R; k++) g[k] = exp(-(double)(k * k) / den);
    double side = g[1];
    for (uint32_t k = 2; k <= R; k++) side = side + g[k];
    const double S = g[0] + 2.0 * side;
    for (uint32_t k = 0; k <= R; k++) {
        const float w = (float)(g[k] / S);
        weights[R + k] = w;
        weights[R - k] = w;
    }
    return R;
}

// The intermediate between the two passes: a binary32 texel (16 bytes) per column of the rectangle r (resolved, inside an image of
// `height` rows) and per row of the image within radius_y of r's.  jh_blur sizes it and jh_blur_launch fills it by these two alone.
static inline jimage_rows jblur_scratch_rows(jimage_rect r, uint32_t radius_y, uint32_t height) { return jimage_row_window(r.y, r.h, radius_y, height); }
static inline uint64_t jblur_scratch_bytes(jimage_rect r, uint32_t radius_y, uint32_t height) { return (uint64_t)jblur_scratch_rows(r, radius_y, height).n_rows * r.w * 16u; }
