// jello_resample.h -- the host half of the resample rule (DESIGN.md 5.9 "Resample rule"): which sizes are legal, and the window and
// the taps of one output index of one axis, and the bytes of the intermediate.  Compiled by the library and the launcher
// (jello_amd/csrc/jello_hip.cpp: jh_resample; kernels_resample.hip: the intermediate), by the query both libraries compile
// (include/jello_queries.h: jq_resample_taps) and by tools/image_rect_check.cpp; tests/resample_ref.py restates it.  The device half
// -- the two fused-multiply-add sums over these taps -- is jello_amd/csrc/kernels_resample.hip.
//
// One axis, n_in source texels (the source RECTANGLE's extent) onto n_out; binary64 throughout, nothing contracted:
//   scale    (double)n_in / (double)n_out;  fs = max(scale, 1.0);  support = base fs, base = 0.5 BOX, 1.0 TRIANGLE, 2.0 CATMULL_ROM,
//            3.0 LANCZOS3.  Legal: n_in >= 1, n_out >= 1, n_in <= 16 n_out.
//   window   c = ((double)i + 0.5) scale;  lo = max(0, (int64)(c - support + 0.5));  hi = min(n_in, (int64)(c + support + 0.5))
//            (the casts truncate);  g_k = f(((double)k - c + 0.5) / fs), k = lo .. hi - 1;  leading and trailing g_k that are
//            exactly 0.0 are dropped, interior zeros stay.
//   filters  BOX 1.0 if -0.5 < x <= 0.5;  TRIANGLE x = |x|, 1.0 - x if x < 1.0;  CATMULL_ROM a = -0.5, x = |x|,
//            ((a + 2.0) x - (a + 3.0)) x x + 1.0 if x < 1.0, (((x - 5.0) x + 8.0) x - 4.0) a if x < 2.0;  LANCZOS3
//            sinc(x) sinc(x / 3.0) if -3.0 <= x < 3.0, sinc(0) = 1, else t = x M_PI, sin(t) / t;  0.0 elsewhere.  sin is the libm
//            call, the rule's only inexact library call.
//   taps     S = the sum of the window's g_k, ascending k;  w_k = (float)(g_k / S).
#pragma once
#include <math.h>
#include <stdint.h>
#include "jello_image.h"

#define JRESAMPLE_BOX 0
#define JRESAMPLE_TRIANGLE 1
#define JRESAMPLE_CATMULL_ROM 2
#define JRESAMPLE_LANCZOS3 3
#define JRESAMPLE_FILTERS 4
#define JRESAMPLE_MAX_RATIO 16u
// The most taps a window has, 2 x 3.0 x 16 = twice the widest support.  With s = support, hi - lo = trunc(c + s + 0.5) -
// trunc(c - s + 0.5) (before the clipping, which only shortens it, and for c - s + 0.5 < 0, where the cast rounds up, lo is 0
// anyway).  floor(y + 2 s) - floor(y) is 2 s when 2 s is an integer and at most floor(2 s) + 1 when it is not.  2 s <= 96; at 96
// (LANCZOS3 at 16:1) it is an integer, below 96 floor(2 s) + 1 <= 96.  tests/test_resample_spec.py asserts it over its sweep.
#define JRESAMPLE_MAX_TAPS 96u

static inline bool jresample_filter_ok(int filter) { return filter >= 0 && filter < JRESAMPLE_FILTERS; }
static inline bool jresample_sizes_ok(uint32_t n_in, uint32_t n_out) {
    return n_in >= 1u && n_out >= 1u && (uint64_t)n_in <= (uint64_t)JRESAMPLE_MAX_RATIO * n_out;
}

static inline double jresample_sinc(double x) {
    if (x == 0.0) return 1.0;
    const double t = x * M_PI;
    return sin(t) / t;
}

// f(x) of a legal filter.
static inline double jresample_filter(int filter, double x) {
    switch (filter) {
        case JRESAMPLE_BOX: return (-0.5 < x && x <= 0.5) ? 1.0 : 0.0;
        case JRESAMPLE_TRIANGLE:
            x = fabs(x);
            return x < 1.0 ? 1.0 - x : 0.0;
        case JRESAMPLE_CATMULL_ROM: {
            const double a = -0.5;
            x = fabs(x);
            if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
            if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
            return 0.0;
        }
        default: return (-3.0 <= x && x < 3.0) ? jresample_sinc(x) * jresample_sinc(x / 3.0) : 0.0;
    }
}

// The taps of output i (< n_out) of a legal filter and legal sizes: the window's first source index into *first, its weights into
// weights (JRESAMPLE_MAX_TAPS entries are enough; may be null: the window alone), and, when sum is not null, S into *sum.  Returns
// the count of taps, or 0 for a window the bound above does not hold for (there is none).
static inline uint32_t jresample_taps(int filter, uint32_t n_in, uint32_t n_out, uint32_t i, float* weights, uint32_t* first, double* sum) {
    static const double kBase[JRESAMPLE_FILTERS] = {0.5, 1.0, 2.0, 3.0};
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale > 1.0 ? scale : 1.0;
    const double support = kBase[filter] * fs;
    const double c = ((double)i + 0.5) * scale;
    int64_t lo = (int64_t)(c - support + 0.5), hi = (int64_t)(c + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > (int64_t)n_in) hi = (int64_t)n_in;
    if (hi - lo > (int64_t)JRESAMPLE_MAX_TAPS) return 0u;
    double g[JRESAMPLE_MAX_TAPS];
    for (int64_t k = lo; k < hi; k++) g[k - lo] = jresample_filter(filter, ((double)k - c + 0.5) / fs);
    int64_t a = 0, b = hi - lo;
    while (a < b && g[a] == 0.0) a++;
    while (b > a && g[b - 1] == 0.0) b--;
    double S = 0.0;
    for (int64_t k = a; k < b; k++) S = S + g[k];
    if (weights)
        for (int64_t k = a; k < b; k++) weights[k - a] = (float)(g[k] / S);
    if (first) *first = (uint32_t)(lo + a);
    if (sum) *sum = S;
    return (uint32_t)(b - a);
}

// The intermediate between the two passes: a binary32 texel (16 bytes) per row of the source rectangle and per column of the
// destination rectangle (both resolved).  jh_resample sizes it and jh_resample_launch fills it by these two alone.
static inline uint32_t jresample_scratch_rows(jimage_rect src) { return src.h; }
static inline uint64_t jresample_scratch_bytes(jimage_rect src, jimage_rect dst) { return (uint64_t)jresample_scratch_rows(src) * dst.w * 16u; }
