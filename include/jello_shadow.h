// jello_shadow.h -- the shadow rule (DESIGN.md 5.18 "Shadow rule"; include/jello_hip.h "Shadow" states all of it): which descriptor is
// legal, the plan, the bounds rectangle -- binary64 appears in these only -- and the device half as functions the kernel compiles too:
// the position as binary32, the erf approximant, the band term, the cap sum and the coverage.  Compiled by the library
// (jello_amd/csrc/jello_hip.cpp: jh_shadow), by the kernel (jello_amd/csrc/kernels_shadow.hip), by the queries both libraries compile
// (include/jello_queries.h: jq_shadow_plan, jq_shadow_bounds) and by tools/shadow_check.cpp; tests/shadow_ref.py restates it.
// The matrix's legality and inverse are include/jello_warp.h's jwarp_plan, unchanged.
//
//   legal     box finite, x1 >= x0, y1 >= y0, every coordinate within [-2^22, 2^22]; radius finite, >= 0; sigma finite, in [0, 2^16];
//             no flag bit but OVER and INVERT; the matrix legal for jwarp_plan.
//   plan      binary64, every operation rounded once: centre = (x0 + x1) / 2, a = (x1 - x0) / 2, likewise y and b; r = min(radius, a, b);
//             sigma' = max(sigma, 2^-8); C = rint(centre 2^32); then rounded once to binary32: a, b, r, core = a - r, straight = b - r,
//             sigma', inv_s = 1 / (sigma' sqrt 2), window = K sigma', K = 4; N = 4 for r / sigma' <= 0.5, 8 for <= 1.5, else 16.
//   position  U = P (2 X + 1) + Q (2 Y + 1) + R - Cx, V likewise, int64, units of 2^-32; x = (float)(int32)(U >> 32) +
//             (float)((uint32)U >> 8) 2^-24, the sum rounded once (the low 8 bits dropped).
//   G         the erf approximant: t = minNum(|z|, 4); u = t (a1 + t (a2 + t (a3 + t (a4 + t (a5 + t a6))))), five fmaf and a product;
//             four times s = s (2 + s) from s = u; e = 1 - 1 / (1 + s); G = copysign(e, z).  Abramowitz & Stegun 7.1.28 with p - 1
//             carried in place of p.  Every step is monotone in t (the coefficients are positive), so G is, in binary32.
//   band      B(p, w) = G((p + w) inv_s) - G((p - w) inv_s) >= 0 for w >= 0.
//   coverage  acc = B(y, straight) B(x, a); with r > 0 the cap above (q = y - straight) and the cap below (q = -y - straight), in
//             that order, each adding by jshadow_cap; S = minNum(0.25 acc, 1).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "jello_hip.h"
#include "jello_warp.h"

#if defined(__HIPCC__)
#define JSHADOW_HD __host__ __device__ __forceinline__
#else
#define JSHADOW_HD static inline
#endif

#define JSHADOW_OVER 1u
#define JSHADOW_INVERT 2u
#define JSHADOW_K 4u
#define JSHADOW_SIGMA_FLOOR 0.00390625 /* 2^-8 */
#define JSHADOW_SIGMA_MAX 65536.0
#define JSHADOW_BOX_MAX 4194304.0      /* 2^22 */
#define JSHADOW_MAX_EXTENT 8388608u    /* 2^23 */
#define JSHADOW_BOUNDS_GROW 3.625      /* sigma: Phi(-3.625) = 1.45e-4, below 2^-12 = 2.44e-4 with room for G's error */

// ---- the legal descriptor ----

// nullptr for a legal descriptor (the rectangle, the image and the matrix apart), else what is wrong with it (jh_shadow puts
// "jh_shadow: " in front).
static inline const char* jshadow_desc_error(const jh_shadow_desc* d) {
    for (int i = 0; i < 4; i++)
        if (!isfinite(d->box[i])) return "the box is not finite";
    if (!(d->box[2] >= d->box[0] && d->box[3] >= d->box[1])) return "the box has x1 < x0 or y1 < y0";
    for (int i = 0; i < 4; i++)
        if (fabs((double)d->box[i]) > JSHADOW_BOX_MAX) return "a box coordinate above 2^22";
    if (!(isfinite(d->radius) && d->radius >= 0.0f)) return "the radius is negative or not finite";
    if (!(isfinite(d->sigma) && d->sigma >= 0.0f && (double)d->sigma <= JSHADOW_SIGMA_MAX)) return "sigma is outside [0, 2^16] or not finite";
    if ((d->flags & ~(JSHADOW_OVER | JSHADOW_INVERT)) != 0u) return "unknown flag bits";
    return nullptr;
}
static inline const char* jshadow_extent_error(uint32_t width, uint32_t height) {
    return width > JSHADOW_MAX_EXTENT || height > JSHADOW_MAX_EXTENT ? "an image extent above 2^23" : nullptr;
}

// ---- the plan ----

static inline double jshadow_sigma(const jh_shadow_desc* d) { return (double)d->sigma < JSHADOW_SIGMA_FLOOR ? JSHADOW_SIGMA_FLOOR : (double)d->sigma; }
static inline uint32_t jshadow_steps(double rho) { return rho <= 0.5 ? 4u : (rho <= 1.5 ? 8u : 16u); }

// The plan of a descriptor; nullptr, or what is wrong with it (the plan is then untouched).
static inline const char* jshadow_plan(const jh_shadow_desc* d, jh_shad_plan* out) {
    if (const char* why = jshadow_desc_error(d)) return why;
    jh_shad_plan p;
    memset(&p, 0, sizeof p);
    if (const char* why = jwarp_plan(d->matrix, p.m)) return why;
    const double x0 = d->box[0], y0 = d->box[1], x1 = d->box[2], y1 = d->box[3];
    const double cx = (x0 + x1) * 0.5, cy = (y0 + y1) * 0.5, a = (x1 - x0) * 0.5, b = (y1 - y0) * 0.5;
    const double side = a < b ? a : b, r = (double)d->radius < side ? (double)d->radius : side;
    const double sigma = jshadow_sigma(d);
    p.centre[0] = (int64_t)rint(cx * 4294967296.0);  // (|centre| <= 2^22: 2^54; the scaling is exact)
    p.centre[1] = (int64_t)rint(cy * 4294967296.0);
    p.a = (float)a;
    p.b = (float)b;
    p.radius = (float)r;
    p.core = (float)(a - r);
    p.straight = (float)(b - r);
    p.sigma = (float)sigma;
    p.inv_s = (float)(1.0 / (sigma * 1.4142135623730951));
    p.window = (float)((double)JSHADOW_K * sigma);
    p.n = jshadow_steps(r / sigma);
    p.k = JSHADOW_K;
    *out = p;
    return nullptr;
}

// The bounds rectangle {x, y, width, height} of a dst_w x dst_h destination: outside it the rule's S is below 2^-12.  The box grown by
// JSHADOW_BOUNDS_GROW sigma' on every side, its four corners through the matrix (binary64, uncontracted: (a x + c y) + e, (b x + d y)
// + f), floor(min) - 1 and ceil(max) + 1, clipped to the image; empty, or a box empty in one dimension (S = 0): 0, 0, 0, 0.  nullptr,
// or what is wrong with the arguments (rect is then untouched).  The flags are checked and not used: the bounds are those of S, also
// under INVERT.
static inline const char* jshadow_bounds(const jh_shadow_desc* d, uint32_t dst_w, uint32_t dst_h, uint32_t rect[4]) {
    if (const char* why = jshadow_desc_error(d)) return why;
    int64_t plan[6];
    if (const char* why = jwarp_plan(d->matrix, plan)) return why;
    if (const char* why = jshadow_extent_error(dst_w, dst_h)) return why;
    const double* m = d->matrix;
    const double g = JSHADOW_BOUNDS_GROW * jshadow_sigma(d);
    const double xs[2] = {(double)d->box[0] - g, (double)d->box[2] + g}, ys[2] = {(double)d->box[1] - g, (double)d->box[3] + g};
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) {
            const double ax = m[0] * xs[i], cy = m[2] * ys[j], bx = m[1] * xs[i], dy = m[3] * ys[j];
            const double v[2] = {(ax + cy) + m[4], (bx + dy) + m[5]};
            for (int k = 0; k < 2; k++) {
                if (v[k] != v[k]) { lo[k] = -INFINITY; hi[k] = INFINITY; }  // (Inf - Inf of overflowed products: the whole axis)
                lo[k] = v[k] < lo[k] ? v[k] : lo[k];
                hi[k] = v[k] > hi[k] ? v[k] : hi[k];
            }
        }
    const double lim[2] = {(double)dst_w, (double)dst_h};
    uint32_t first[2] = {0u, 0u}, count[2] = {0u, 0u};
    bool empty = !(d->box[2] > d->box[0] && d->box[3] > d->box[1]);
    for (int k = 0; k < 2 && !empty; k++) {
        double a = floor(lo[k]) - 1.0, b = ceil(hi[k]) + 1.0;
        a = a > 0.0 ? a : 0.0;
        b = b < lim[k] ? b : lim[k];
        if (!(b > a)) { empty = true; break; }
        first[k] = (uint32_t)a;
        count[k] = (uint32_t)(b - a);
    }
    rect[0] = empty ? 0u : first[0]; rect[1] = empty ? 0u : first[1]; rect[2] = empty ? 0u : count[0]; rect[3] = empty ? 0u : count[1];
    return nullptr;
}

// ---- what the kernel compiles too ----

// The scalars of a plan the coverage reads (the kernel keeps them in scalar registers).
struct jshadow_scalars { float a, radius, core, straight, inv_s, window, inv_n; uint32_t n; };
static inline jshadow_scalars jshadow_scalars_of(const jh_shad_plan* p) {
    return {p->a, p->radius, p->core, p->straight, p->inv_s, p->window, 1.0f / (float)p->n, p->n};  // (n is a power of two: exact)
}

// An int64 position (2^-32) as binary32: the whole part converted, the top 24 bits of the fraction exact, one rounded sum.
JSHADOW_HD float jshadow_to_f32(int64_t d) { return (float)(int32_t)(d >> 32) + (float)((uint32_t)d >> 8) * 5.9604644775390625e-08f; }
// A texel centre's position relative to the box centre, one axis: the row (P, Q, R) or (S, T, W) of the plan and that axis's centre.
JSHADOW_HD float jshadow_position(int64_t p, int64_t q, int64_t r, int64_t centre, uint32_t X, uint32_t Y) {
    return jshadow_to_f32(jwarp_position(p, q, r, X, Y) - centre);
}

JSHADOW_HD float jshadow_erf(float z) {
    const float t = __builtin_fminf(__builtin_fabsf(z), 4.0f);
    float q = 0.0000430638f;
    q = __builtin_fmaf(t, q, 0.0002765672f);
    q = __builtin_fmaf(t, q, 0.0001520143f);
    q = __builtin_fmaf(t, q, 0.0092705272f);
    q = __builtin_fmaf(t, q, 0.0422820123f);
    q = __builtin_fmaf(t, q, 0.0705230784f);
    float s = t * q;
    s = s * (2.0f + s);
    s = s * (2.0f + s);
    s = s * (2.0f + s);
    s = s * (2.0f + s);
    const float e = 1.0f - 1.0f / (1.0f + s);
    return __builtin_copysignf(e, z);
}
JSHADOW_HD float jshadow_band(float p, float w, float inv_s) { return jshadow_erf((p + w) * inv_s) - jshadow_erf((p - w) * inv_s); }

// One cap's sum added to acc, for a texel at x whose row lies q beyond the cap's first row (towards its tip; any sign).  The window
// [lo, hi] = [maxNum(q - window, 0), minNum(q + window, r)]; nothing where !(hi > lo).  t0 = 1 - sqrt(1 - lo / r), t1 likewise of hi, dt
// = (t1 - t0) / N.  Boundaries m_0 = lo, m_i = minNum(maxNum((r t_i) (2 - t_i), m_(i-1)), hi) with t_i = fmaf(i, dt, t0), m_N = hi.  Per
// sub-interval: dG = G((m_i - q) inv_s) - G((m_(i-1) - q) inv_s); mm = 0.5 (m_(i-1) + m_i); w = core + sqrt((r - mm) (r + mm)); acc =
// fmaf(dG, B(x, w), acc).
JSHADOW_HD float jshadow_cap(const jshadow_scalars& k, float x, float q, float acc) {
    const float r = k.radius;
    const float lo = __builtin_fmaxf(q - k.window, 0.0f), hi = __builtin_fminf(q + k.window, r);
    if (!(hi > lo)) return acc;
    const float t0 = 1.0f - sqrtf(1.0f - lo / r), t1 = 1.0f - sqrtf(1.0f - hi / r);
    const float dt = (t1 - t0) * k.inv_n;
    float m_prev = lo, g_prev = jshadow_erf((lo - q) * k.inv_s);
    for (uint32_t i = 1u; i <= k.n; i++) {
        float m = hi;
        if (i < k.n) {
            const float t = __builtin_fmaf((float)i, dt, t0);
            m = __builtin_fminf(__builtin_fmaxf((r * t) * (2.0f - t), m_prev), hi);
        }
        const float g = jshadow_erf((m - q) * k.inv_s);
        const float mm = 0.5f * (m_prev + m);
        const float w = k.core + sqrtf((r - mm) * (r + mm));
        acc = __builtin_fmaf(g - g_prev, jshadow_band(x, w, k.inv_s), acc);
        m_prev = m;
        g_prev = g;
    }
    return acc;
}
// S from the product of the two straight bands (`mid`) at the position (x, y): the caps added where the radius is not 0.
template <bool ROUND>
JSHADOW_HD float jshadow_finish(const jshadow_scalars& k, float mid, float x, float y) {
    float acc = mid;
    if (ROUND) {
        acc = jshadow_cap(k, x, y - k.straight, acc);
        acc = jshadow_cap(k, x, -y - k.straight, acc);
    }
    return __builtin_fminf(0.25f * acc, 1.0f);
}
JSHADOW_HD float jshadow_coverage(const jshadow_scalars& k, float x, float y) {
    const float mid = jshadow_band(y, k.straight, k.inv_s) * jshadow_band(x, k.a, k.inv_s);
    return k.radius > 0.0f ? jshadow_finish<true>(k, mid, x, y) : jshadow_finish<false>(k, mid, x, y);
}
// The premultiplied texel before the store: colour x S', S' = S or 1 - S under INVERT, one product per channel.
JSHADOW_HD void jshadow_premultiplied(const float color[4], float s, bool invert, float out[4]) {
    const float sp = invert ? 1.0f - s : s;
    for (int c = 0; c < 4; c++) out[c] = color[c] * sp;
}

// Texel (X, Y) of the image by the rule, on the host: S.
static inline float jshadow_texel(const jh_shad_plan* p, uint32_t X, uint32_t Y) {
    const jshadow_scalars k = jshadow_scalars_of(p);
    return jshadow_coverage(k, jshadow_position(p->m[0], p->m[1], p->m[2], p->centre[0], X, Y), jshadow_position(p->m[3], p->m[4], p->m[5], p->centre[1], X, Y));
}
