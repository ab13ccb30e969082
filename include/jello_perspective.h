// jello_perspective.h -- the perspective rule up to the source position (DESIGN.md 5.19 "Perspective rule"): which matrix is legal,
// the nine doubles of the plan, the source position of a destination texel, and the bounds rectangle.  Compiled by the library
// (jello_amd/csrc/jello_hip.cpp: jh_perspective), by the kernels (jello_amd/csrc/kernels_perspective.hip: jpersp_position is the one
// text the device, the host and the stand-alone check compile), by the queries both libraries compile (include/jello_queries.h:
// jq_perspective_plan, jq_perspective_bounds) and by tools/perspective_check.cpp; tests/perspective_ref.py restates it.  From the
// position on -- taps, edge, sum, store, values -- the rule is include/jello_warp.h's and jello_amd/csrc/warp_taps.h's, unchanged.
//
//   matrix    (a, b, p, c, d, q, e, f, s), binary64, column-major so that it extends the Scene order: x' w = a x + c y + e,
//             y' w = b x + d y + f, w = p x + q y + s, from continuous coordinates of the source RECTANGLE (origin its top-left
//             corner, texel (i, j) centred at (i + 0.5, j + 0.5)) to those of the destination IMAGE.  p = q = 0, s = 1: jh_warp's.
//   plan      host only, binary64, nothing contracted, each product, difference and quotient rounded once.  The adjugate, nine
//             two-product differences:  ( d s - f q,  e q - c s,  c f - e d )
//                                       ( f p - b s,  a s - e p,  e b - a f )
//                                       ( b q - d p,  c p - a q,  a d - c b )
//             det = ((a adj00) + (c adj10)) + (e adj20).  G = adj scaled by 2^-k, 2^(k-1) < max |adj_ij| <= 2^k: an ldexp, which rounds
//             nothing (unless an entry 2^1022 below the largest goes subnormal, where ldexp rounds it once, half to even), so a
//             matrix whose inverse is dyadic stays exact.  G is negated when det < 0: every |G_ij| <= 1, one of them above 1/2, and
//             den > 0 <=> the forward w of the source position is > 0 (in front of the viewer).
//   legal     nine finite entries, nine finite adjugate entries, det finite and not 0; both images at most 32768 on a side.
//   position  device, binary64, per destination texel (X, Y) of the image: x' = X + 0.5, y' = Y + 0.5 (exact);
//             n_u = ((G0 x') + (G1 y')) + G2, n_v = ((G3 x') + (G4 y')) + G5, den = ((G6 x') + (G7 y')) + G8, five roundings each;
//             q = 1.0 / den (IEEE division); u = n_u q, v = n_v q.  The texel is VOID when !(den > 0) or when u or v is a NaN
//             (0 x Inf: a den so small that q overflows): it stores four +0.0 whatever the edge mode, and loads nothing.  Otherwise
//             u is clamped to [-2^22, 2^22] (an infinite u too) and U = (int64) rint(u 2^32), half to even; V likewise.  |U| <= 2^54.
//   fusing    the three-term sums are spelled as separate statements, one product or sum each, under `#pragma clang fp contract(off)`
//             where the compiler is clang (hipcc, both halves) and under __attribute__((optimize("fp-contract=off"))) where it is
//             GCC: whatever flags a caller builds with, no product is fused into a sum here.  (The builds pass -ffp-contract=off too.)
//   not done  no minification prefilter: toward the horizon the result aliases, and jh_resample first is the answer today.  No call
//             in place.  Under REPEAT / MIRROR a clamped position reads whatever the index rule gives there.
#pragma once
#include <math.h>
#include <stdint.h>

#include "jello_warp.h"

#if defined(__HIPCC__)
#define JPERSP_HD __host__ __device__ __forceinline__
#else
#define JPERSP_HD static inline
#endif
#if defined(__clang__)
#define JPERSP_UNFUSED
#define JPERSP_UNFUSED_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define JPERSP_UNFUSED __attribute__((optimize("fp-contract=off")))
#define JPERSP_UNFUSED_BODY
#else
#define JPERSP_UNFUSED
#define JPERSP_UNFUSED_BODY
#endif

#define JPERSP_STRAIGHT JWARP_STRAIGHT
#define JPERSP_MAX_SIDE JWARP_MAX_SIDE
#define JPERSP_MAX_POSITION 4194304.0 /* |u|, |v|: 2^22 */

// a b - c d: each product and the difference rounded once.
JPERSP_UNFUSED static inline double jpersp_diff(double a, double b, double c, double d) {
    JPERSP_UNFUSED_BODY
    const double ab = a * b;
    const double cd = c * d;
    return ab - cd;
}

// The adjugate (row-major, the order of the rule) and det of a matrix; nullptr for a legal matrix, else which condition failed.
JPERSP_UNFUSED static inline const char* jpersp_adjugate(const double m[9], double adj[9], double* det_out) {
    JPERSP_UNFUSED_BODY
    const double a = m[0], b = m[1], p = m[2], c = m[3], d = m[4], q = m[5], e = m[6], f = m[7], s = m[8];
    for (int i = 0; i < 9; i++)
        if (!isfinite(m[i])) return "a matrix entry is not finite";
    adj[0] = jpersp_diff(d, s, f, q); adj[1] = jpersp_diff(e, q, c, s); adj[2] = jpersp_diff(c, f, e, d);
    adj[3] = jpersp_diff(f, p, b, s); adj[4] = jpersp_diff(a, s, e, p); adj[5] = jpersp_diff(e, b, a, f);
    adj[6] = jpersp_diff(b, q, d, p); adj[7] = jpersp_diff(c, p, a, q); adj[8] = jpersp_diff(a, d, c, b);
    for (int i = 0; i < 9; i++)
        if (!isfinite(adj[i])) return "an adjugate entry is not finite";
    const double t0 = a * adj[0];
    const double t1 = c * adj[3];
    const double t2 = e * adj[6];
    const double t01 = t0 + t1;
    const double det = t01 + t2;
    if (!isfinite(det)) return "the determinant is not finite";
    if (det == 0.0) return "the determinant is 0";
    *det_out = det;
    return nullptr;
}

// The plan G[9] of a matrix; nullptr for a legal matrix, else which condition failed (G is then untouched).
static inline const char* jpersp_plan(const double m[9], double G[9]) {
    double adj[9], det;
    if (const char* why = jpersp_adjugate(m, adj, &det)) return why;
    double top = 0.0;
    for (int i = 0; i < 9; i++) top = fabs(adj[i]) > top ? fabs(adj[i]) : top;
    if (top == 0.0) return "the determinant is 0";  // (not reached: det would be 0)
    int k;
    const double mant = frexp(top, &k);  // top = mant 2^k, 1/2 <= mant < 1
    if (mant == 0.5) k -= 1;             // (a power of two is its own bound)
    for (int i = 0; i < 9; i++) {
        const double g = ldexp(adj[i], -k);
        G[i] = det < 0.0 ? -g : g;
    }
    return nullptr;
}

// The source position of destination texel (X, Y) under the plan G: false for a void texel (U and V are then untouched), else
// U and V in units of 2^-32 texel.
JPERSP_UNFUSED JPERSP_HD bool jpersp_position(const double* G, uint32_t X, uint32_t Y, int64_t* U, int64_t* V) {
    JPERSP_UNFUSED_BODY
    const double xp = (double)X + 0.5, yp = (double)Y + 0.5;
    const double ux = G[0] * xp;
    const double uy = G[1] * yp;
    const double uxy = ux + uy;
    const double nu = uxy + G[2];
    const double vx = G[3] * xp;
    const double vy = G[4] * yp;
    const double vxy = vx + vy;
    const double nv = vxy + G[5];
    const double dx = G[6] * xp;
    const double dy = G[7] * yp;
    const double dxy = dx + dy;
    const double den = dxy + G[8];
    if (!(den > 0.0)) return false;
    const double q = 1.0 / den;
    double u = nu * q;
    double v = nv * q;
    if (u != u || v != v) return false;
    u = u < -JPERSP_MAX_POSITION ? -JPERSP_MAX_POSITION : (u > JPERSP_MAX_POSITION ? JPERSP_MAX_POSITION : u);
    v = v < -JPERSP_MAX_POSITION ? -JPERSP_MAX_POSITION : (v > JPERSP_MAX_POSITION ? JPERSP_MAX_POSITION : v);
    *U = (int64_t)__builtin_rint(u * 4294967296.0);  // (the scaling is exact; at most 2^54)
    *V = (int64_t)__builtin_rint(v * 4294967296.0);
    return true;
}

// The bounds rectangle {x, y, width, height}: under ZERO every destination texel outside it is +0 in all four channels.  The forward
// images of the four corners of the src_w x src_h source rectangle grown by 0.5 NEAREST, 1 BILINEAR, 2 BICUBIC -- binary64,
// uncontracted, in this order: xw = ((a x) + (c y)) + e, yw = ((b x) + (d y)) + f, w = ((p x) + (q y)) + s, then x' = xw / w and
// y' = yw / w.  A corner with !(w > 0): the image of the rectangle is unbounded, the whole destination.  Otherwise floor(min) - 1
// and ceil(max) + 1, clipped to the dst_w x dst_h image (a NaN coordinate: the whole axis); empty: 0, 0, 0, 0.  nullptr, or what is
// wrong with the arguments (rect is then untouched).
JPERSP_UNFUSED static inline const char* jpersp_bounds(const double m[9], uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h,
                                                        uint32_t rect[4]) {
    JPERSP_UNFUSED_BODY
    static const double kGrow[JWARP_FILTERS] = {0.5, 1.0, 2.0};
    double adj[9], det;
    if (!jwarp_filter_ok(filter)) return "unknown filter";
    if (const char* why = jpersp_adjugate(m, adj, &det)) return why;
    if (src_w > JPERSP_MAX_SIDE || src_h > JPERSP_MAX_SIDE || dst_w > JPERSP_MAX_SIDE || dst_h > JPERSP_MAX_SIDE) return "an image side above 32768";
    const double g = kGrow[filter], xs[2] = {-g, (double)src_w + g}, ys[2] = {-g, (double)src_h + g};
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    bool whole = false;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) {
            const double ax = m[0] * xs[i], cy = m[3] * ys[j], bx = m[1] * xs[i], dy = m[4] * ys[j], px = m[2] * xs[i], qy = m[5] * ys[j];
            const double axcy = ax + cy, bxdy = bx + dy, pxqy = px + qy;
            const double xw = axcy + m[6], yw = bxdy + m[7], w = pxqy + m[8];
            if (!(w > 0.0)) { whole = true; continue; }
            const double v[2] = {xw / w, yw / w};
            for (int k = 0; k < 2; k++) {
                if (v[k] != v[k]) { lo[k] = -INFINITY; hi[k] = INFINITY; }  // (Inf - Inf of overflowed products, Inf / Inf: the whole axis)
                lo[k] = v[k] < lo[k] ? v[k] : lo[k];
                hi[k] = v[k] > hi[k] ? v[k] : hi[k];
            }
        }
    if (whole) lo[0] = lo[1] = -INFINITY, hi[0] = hi[1] = INFINITY;
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

// nullptr for a legal descriptor between a src_w x src_h and a dst_w x dst_h image (the matrix apart: jpersp_plan; the rectangles
// apart: jimage_rect_check), else what is wrong with it (jh_perspective puts "jh_perspective: " in front).
static inline const char* jpersp_desc_error(int filter, int edge, uint32_t flags, uint32_t src_w, uint32_t src_h, uint32_t dst_w, uint32_t dst_h) {
    return jwarp_desc_error(filter, edge, flags, src_w, src_h, dst_w, dst_h);
}
