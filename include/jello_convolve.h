// jello_convolve.h -- the host half of the convolve rule (DESIGN.md 5.13 "Convolve rule"): which descriptor is legal (its rectangle
// apart: jello_image.h), and the weights of an feConvolveMatrix: the 180-degree flip and the divisor, which the device never sees.
// Compiled by the library (jello_amd/csrc/jello_hip.cpp: jh_convolve), by the kernels
// (jello_amd/csrc/kernels_convolve.hip: the limits; the index rules are jwarp_index of jello_warp.h, included here and not copied),
// by the query both libraries compile (include/jello_queries.h: jq_convolve_weights) and by tools/convolve_check.cpp; tests/convolve_ref.py
// restates it.
//
//   weights   binary32, row-major with stride order_x, IN THE ORDER THEY ARE APPLIED: w[j][i] multiplies the operand at the image
//             position (X - target_x + i, Y - target_y + j) -- a correlation.
//   legal     1 <= order_x, order_y <= 15; target_x < order_x, target_y < order_y; a known edge and mode; every weight that is read
//             (the first order_x order_y) and the bias finite.
//   edge      a tap index i against the IMAGE's extent n: jwarp_index(edge, i, n), the four rules of the warp.
//   from SVG  weights[j ox + i] = (float)(kernelMatrix[(oy - 1 - j) ox + (ox - 1 - i)] / d): the quotient in binary64, rounded once to
//             binary32; d = divisor if it is not 0, otherwise the sum of kernelMatrix in ascending index order in binary64, or 1.0 if
//             that sum is 0 (the specification's default).
#pragma once
#include <math.h>
#include <stdint.h>

#include "jello_warp.h"

#define JCONV_MAX_ORDER 15u
#define JCONV_MAX_TAPS 225u
#define JCONV_EDGE_ZERO JWARP_EDGE_ZERO
#define JCONV_EDGE_CLAMP JWARP_EDGE_CLAMP
#define JCONV_EDGE_REPEAT JWARP_EDGE_REPEAT
#define JCONV_EDGE_MIRROR JWARP_EDGE_MIRROR
#define JCONV_PREMULTIPLIED 0
#define JCONV_STRAIGHT 1
#define JCONV_PRESERVE_ALPHA 2
#define JCONV_MODES 3

static inline bool jconv_order_ok(uint32_t order_x, uint32_t order_y) {
    return order_x >= 1u && order_x <= JCONV_MAX_ORDER && order_y >= 1u && order_y <= JCONV_MAX_ORDER;
}
static inline bool jconv_mode_ok(int mode) { return mode >= 0 && mode < JCONV_MODES; }

// nullptr for a legal descriptor (the rectangle and the images apart), else what is wrong with it (jh_convolve puts "jh_convolve: "
// in front).  `weights` holds at least order_x * order_y values once the orders are legal; nothing of it is read before that.
static inline const char* jconv_desc_error(uint32_t order_x, uint32_t order_y, uint32_t target_x, uint32_t target_y, int edge, int mode,
                                           const float* weights, float bias) {
    if (!jconv_order_ok(order_x, order_y)) return "an order outside 1..15";
    if (target_x >= order_x || target_y >= order_y) return "the target is outside the kernel";
    if (!jwarp_edge_ok(edge)) return "unknown edge mode";
    if (!jconv_mode_ok(mode)) return "unknown mode";
    for (uint32_t k = 0; k < order_x * order_y; k++)
        if (!isfinite(weights[k])) return "a weight is not finite";
    return isfinite(bias) ? nullptr : "the bias is not finite";
}

// The weights of feConvolveMatrix's kernelMatrix and divisor (see "from SVG" above) into weights[order_x * order_y]; nullptr, or what
// is wrong (weights may then be partly written).
static inline const char* jconv_weights(uint32_t order_x, uint32_t order_y, const double* kernel_matrix, double divisor, float* weights) {
    if (!jconv_order_ok(order_x, order_y)) return "an order outside 1..15";
    const uint32_t n = order_x * order_y;
    if (!isfinite(divisor)) return "the divisor is not finite";
    double sum = 0.0;
    for (uint32_t k = 0; k < n; k++) {
        if (!isfinite(kernel_matrix[k])) return "a kernelMatrix entry is not finite";
        sum = sum + kernel_matrix[k];
    }
    double d = divisor;
    if (d == 0.0) {
        if (!isfinite(sum)) return "the sum of kernelMatrix is not finite";
        d = sum == 0.0 ? 1.0 : sum;
    }
    for (uint32_t k = 0; k < n; k++) {
        const float w = (float)(kernel_matrix[n - 1u - k] / d);  // (row oy - 1 - j, column ox - 1 - i: the reversed index)
        if (!isfinite(w)) return "a weight does not come out finite";
        weights[k] = w;
    }
    return nullptr;
}
