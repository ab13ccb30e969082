// jello_warp.h -- the host half of the warp rule (DESIGN.md 5.12 "Warp rule"): which matrix is legal, the six integers of the plan,
// the per-axis taps and the four index rules, and the bounds rectangle.  Compiled by the library (jello_amd/csrc/jello_hip.cpp:
// jh_warp), by the kernels (jello_amd/csrc/warp_taps.h and kernels_warp.hip: the index rules, the fraction and the
// cubic weights are the one text the device and the stand-alone check both compile), by the queries both libraries compile
// (include/jello_queries.h: jq_warp_plan, jq_warp_bounds) and by tools/warp_plan_check.cpp; tests/warp_ref.py restates it.
//
//   matrix    (a, b, c, d, e, f), binary64: x' = a x + c y + e, y' = b x + d y + f, from continuous coordinates of the source
//             RECTANGLE (origin its top-left corner, texel (i, j) centred at (i + 0.5, j + 0.5)) to those of the destination IMAGE.
//   inverse   binary64, nothing contracted (the build's -ffp-contract=off, as for jello_resample.h), every product and quotient
//             rounded once: det = a d - b c;  p = d / det, q = -c / det, r = (c f - d e) / det;  s = -b / det, t = a / det,
//             w = (b e - a f) / det.  u = p x' + q y' + r, v = s x' + t y' + w.
//   legal     the six entries finite; det finite and not 0; |p|, |q|, |s|, |t| <= 64; |r|, |w| <= 2^22.
//   plan      P = rint(p 2^31), likewise Q, S, T;  R = rint(r 2^32), likewise W;  rint rounds half to even.  Destination texel
//             (X, Y) of the image reads the source position U = P (2 X + 1) + Q (2 Y + 1) + R, V = S (2 X + 1) + T (2 Y + 1) + W, in
//             units of 2^-32 texel, exact in int64: |P| <= 2^37, 2 X + 1 < 2^16, |R| <= 2^54, so |U| < 2^55.
//   taps      NEAREST: i = U >> 32 (arithmetic: a floor), weight 1.0f.  BILINEAR: U' = U - 2^31, i0 = U' >> 32, k = (U' >> 16) &
//             0xffff (the low 16 bits dropped), f = (float)k 2^-16; taps i0, i0 + 1, weights 1.0f - f, f.  BICUBIC: the same i0 and
//             f, taps i0 - 1 .. i0 + 2, weights jwarp_cubic_weights (Catmull-Rom, binary32, the stated fmaf's and single products).
//   edge      a tap index i against the source rectangle's extent n: jwarp_index.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JWARP_HD __host__ __device__ __forceinline__
#else
#define JWARP_HD static inline
#endif

#define JWARP_NEAREST 0
#define JWARP_BILINEAR 1
#define JWARP_BICUBIC 2
#define JWARP_FILTERS 3
#define JWARP_EDGE_ZERO 0
#define JWARP_EDGE_CLAMP 1
#define JWARP_EDGE_REPEAT 2
#define JWARP_EDGE_MIRROR 3
#define JWARP_EDGES 4
#define JWARP_STRAIGHT 1u
#define JWARP_MAX_SIDE 32768u
#define JWARP_MAX_SCALE 64.0        /* |p|, |q|, |s|, |t| */
#define JWARP_MAX_OFFSET 4194304.0  /* |r|, |w|: 2^22 */

static inline bool jwarp_filter_ok(int filter) { return filter >= 0 && filter < JWARP_FILTERS; }
static inline bool jwarp_edge_ok(int edge) { return edge >= 0 && edge < JWARP_EDGES; }

// The inverse (p, q, r, s, t, w) of a matrix into inv; nullptr for a legal matrix, else which condition failed.
static inline const char* jwarp_inverse(const double m[6], double inv[6]) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5];
    for (int i = 0; i < 6; i++)
        if (!isfinite(m[i])) return "a matrix entry is not finite";
    const double ad = a * d, bc = b * c;
    const double det = ad - bc;
    if (!isfinite(det)) return "the determinant is not finite";
    if (det == 0.0) return "the determinant is 0";
    const double cf = c * f, de = d * e, be = b * e, af = a * f;
    inv[0] = d / det;
    inv[1] = -c / det;
    inv[2] = (cf - de) / det;
    inv[3] = -b / det;
    inv[4] = a / det;
    inv[5] = (be - af) / det;
    if (!(fabs(inv[0]) <= JWARP_MAX_SCALE && fabs(inv[1]) <= JWARP_MAX_SCALE && fabs(inv[3]) <= JWARP_MAX_SCALE && fabs(inv[4]) <= JWARP_MAX_SCALE))
        return "an inverse coefficient above 64 (a minification beyond 64:1)";
    if (!(fabs(inv[2]) <= JWARP_MAX_OFFSET && fabs(inv[5]) <= JWARP_MAX_OFFSET)) return "an inverse offset above 2^22";
    return nullptr;
}

// The plan (P, Q, R, S, T, W) of a matrix; nullptr for a legal matrix, else which condition failed (plan is then untouched).
static inline const char* jwarp_plan(const double m[6], int64_t plan[6]) {
    double inv[6];
    if (const char* why = jwarp_inverse(m, inv)) return why;
    for (int i = 0; i < 6; i++) plan[i] = (int64_t)rint(inv[i] * ((i % 3) == 2 ? 4294967296.0 : 2147483648.0));  // (the scalings are exact)
    return nullptr;
}
// Whether the six integers lie where a legal matrix's do: |P|, |Q|, |S|, |T| <= 64 x 2^31, |R|, |W| <= 2^22 x 2^32 (the limits above,
// scaled as jwarp_plan scales; both products are exact).  What a launcher asks of a plan it did not make: the positions then fit
// int64 and the taps' indices 32 bits.
static inline bool jwarp_plan_in_range(const int64_t plan[6]) {
    for (int i = 0; i < 6; i++) {
        const int64_t lim = (int64_t)((i % 3) == 2 ? JWARP_MAX_OFFSET * 4294967296.0 : JWARP_MAX_SCALE * 2147483648.0);
        if (plan[i] > lim || plan[i] < -lim) return false;
    }
    return true;
}

// The source position of destination texel (X, Y), one axis: the row (P, Q, R) or (S, T, W) of the plan.
JWARP_HD int64_t jwarp_position(int64_t p, int64_t q, int64_t r, uint32_t X, uint32_t Y) {
    return p * (int64_t)(2u * X + 1u) + q * (int64_t)(2u * Y + 1u) + r;
}
JWARP_HD int32_t jwarp_nearest(int64_t U) { return (int32_t)(U >> 32); }
// BILINEAR and BICUBIC: i0, and the fraction into *f (a multiple of 2^-16 in [0, 1): exact).
JWARP_HD int32_t jwarp_split(int64_t U, float* f) {
    const int64_t u = U - ((int64_t)1 << 31);
    *f = (float)(uint32_t)((u >> 16) & 0xffff) * 0.0000152587890625f;
    return (int32_t)(u >> 32);
}
// The Catmull-Rom weights of the taps i0 - 1 .. i0 + 2 at fraction f: binary32, these fmaf's and single multiplications.
JWARP_HD void jwarp_cubic_weights(float f, float w[4]) {
    w[0] = __builtin_fmaf(__builtin_fmaf(-0.5f, f, 1.0f), f, -0.5f) * f;
    w[1] = __builtin_fmaf(__builtin_fmaf(1.5f, f, -2.5f) * f, f, 1.0f);
    w[2] = __builtin_fmaf(__builtin_fmaf(-1.5f, f, 2.0f), f, 0.5f) * f;
    w[3] = (__builtin_fmaf(0.5f, f, -0.5f) * f) * f;
}

// i mod n with a non-negative result (n >= 1).
JWARP_HD int32_t jwarp_mod(int32_t i, int32_t n) {
    const int32_t m = i % n;
    return m < 0 ? m + n : m;
}
// Tap index i against the extent n >= 1 of the source rectangle: the index in [0, n) the tap reads, or -1 where it reads +0.0f in all
// four channels (ZERO outside the rectangle).  ZERO: i inside [0, n); CLAMP: min(max(i, 0), n - 1); REPEAT: i mod n; MIRROR:
// m = i mod 2 n, m below n, 2 n - 1 - m otherwise.
JWARP_HD int32_t jwarp_index(int edge, int32_t i, int32_t n) {
    switch (edge) {
        case JWARP_EDGE_ZERO: return (i >= 0 && i < n) ? i : -1;
        case JWARP_EDGE_CLAMP: return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
        case JWARP_EDGE_REPEAT: return jwarp_mod(i, n);
        default: {
            const int32_t m = jwarp_mod(i, 2 * n);
            return m < n ? m : 2 * n - 1 - m;
        }
    }
}

// The bounds rectangle {x, y, width, height}: under ZERO every destination texel outside it is transparent black.  The forward
// images (binary64, uncontracted: (a x + c y) + e, (b x + d y) + f) of the four corners of the src_w x src_h source rectangle grown
// by m = 0.5 NEAREST, 1 BILINEAR, 2 BICUBIC; floor(min) - 1 and ceil(max) + 1, clipped to the dst_w x dst_h image; empty: 0, 0, 0, 0.
// nullptr, or what is wrong with the arguments.
static inline const char* jwarp_bounds(const double m[6], uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h, uint32_t rect[4]) {
    static const double kGrow[JWARP_FILTERS] = {0.5, 1.0, 2.0};
    double inv[6];
    if (!jwarp_filter_ok(filter)) return "unknown filter";
    if (const char* why = jwarp_inverse(m, inv)) return why;
    if (src_w > JWARP_MAX_SIDE || src_h > JWARP_MAX_SIDE || dst_w > JWARP_MAX_SIDE || dst_h > JWARP_MAX_SIDE) return "an image side above 32768";
    const double g = kGrow[filter], xs[2] = {-g, (double)src_w + g}, ys[2] = {-g, (double)src_h + g};
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
    uint32_t first[2], count[2];
    for (int k = 0; k < 2; k++) {
        double a = floor(lo[k]) - 1.0, b = ceil(hi[k]) + 1.0;  // (an overflowed image is +-Inf and clips like any other)
        a = a > 0.0 ? a : 0.0;
        b = b < lim[k] ? b : lim[k];
        if (!(b > a)) { rect[0] = rect[1] = rect[2] = rect[3] = 0u; return nullptr; }
        first[k] = (uint32_t)a;
        count[k] = (uint32_t)(b - a);
    }
    rect[0] = first[0]; rect[1] = first[1]; rect[2] = count[0]; rect[3] = count[1];
    return nullptr;
}

// nullptr for a legal descriptor between a src_w x src_h and a dst_w x dst_h image (the matrix apart: jwarp_plan; the rectangles
// apart: jimage_rect_check), else what is wrong with it (jh_warp puts "jh_warp: " in front).
static inline const char* jwarp_desc_error(int filter, int edge, uint32_t flags, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h) {
    if (!jwarp_filter_ok(filter)) return "unknown filter";
    if (!jwarp_edge_ok(edge)) return "unknown edge mode";
    if ((flags & ~JWARP_STRAIGHT) != 0u) return "unknown flag bits";
    return src_w > JWARP_MAX_SIDE || src_h > JWARP_MAX_SIDE || dst_w > JWARP_MAX_SIDE || dst_h > JWARP_MAX_SIDE ? "an image side above 32768" : nullptr;
}
