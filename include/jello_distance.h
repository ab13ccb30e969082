// jello_distance.h -- the host half of the distance rule (DESIGN.md 5.20 "Distance rule") and the per-axis pieces of its device half:
// which descriptor is legal (its rectangle apart: jello_image.h), the geometry and bytes of the intermediate planes, the plan
// jh_distance_plan answers, and -- the one text the kernels (jello_amd/csrc/kernels_distance.hip) and the stand-alone check
// (tools/distance_check.cpp) both compile -- the clamped run-length step of the column pass, the combine and the stop of the row
// pass, the seed test and the value.  Compiled by the library (jello_amd/csrc/jello_hip.cpp: jh_distance), through
// include/jello_queries.h by both libraries, and by tools/distance_check.cpp; tests/distance_ref.py restates the rule from the set
// definition and includes nothing of this file.
//
//   seed      a texel whose chosen channel, widened to binary32, is >= threshold (IEEE: a NaN is no seed, -0 >= +0 holds)
//   feature   what a distance is measured to: OUTER: the seeds; INNER: the non-seeds, and under EDGE_ZERO every position outside the image
//   CAP       (R + 1)^2.  D = min(CAP, min over the features of dx^2 + dy^2), in integers
//   G         the column pass's answer per position: min(R + 1, rows to the nearest feature of that column).  A feature farther than R
//             rows away contributes at least CAP whatever dx is, so the clamp loses nothing, and G fits 9 bits (a uint16_t plane)
//   D         min(CAP, min over |dx| <= R of dx^2 + G(X + dx)^2); the walk outwards from dx = 0 may stop as soon as dx^2 >= the best
//             so far -- every later term is at least dx^2 -- so the stop is exact
#pragma once
#include <math.h>
#include <stdint.h>

#include "jello_hip.h"
#include "jello_image.h"

#if defined(__HIPCC__)
#define JDIST_HD __host__ __device__ __forceinline__
#else
#define JDIST_HD static inline
#endif

#define JDIST_MAX_RADIUS 255u
#define JDIST_OUTER 0
#define JDIST_INNER 1
#define JDIST_SIGNED 2
#define JDIST_EDGE_ZERO 0
#define JDIST_EDGE_CLAMP 1
#define JDIST_STRAIGHT 1u

// ---- the pieces of the two passes ----

// Whether a channel value is a seed.
JDIST_HD bool jdist_is_seed(float value, float threshold) { return value >= threshold; }
// The column pass's counter, "rows since the last feature", after one more row: 0 on a feature, else one more, clamped to R + 1.
JDIST_HD uint32_t jdist_run(uint32_t run, bool feature, uint32_t R) { return feature ? 0u : (run < R ? run + 1u : R + 1u); }
// What the counter starts from in front of the first row it walks.  That row is either the image's first (or last) row -- then under
// EDGE_ZERO the inner plane has a feature right outside the image, counter 0 -- or it lies R rows from the first row whose G is
// kept, and nothing before it can matter: R + 1.
JDIST_HD uint32_t jdist_run_start(bool at_image_border, bool inner, bool clamp, uint32_t R) { return at_image_border && inner && !clamp ? 0u : R + 1u; }
// The row pass: the best squared distance so far, after the column dx away whose G is g (g <= 256, dx <= 255: below 2^17).
JDIST_HD uint32_t jdist_combine(uint32_t best, uint32_t dx, uint32_t g) {
    const uint32_t d = dx * dx + g * g;
    return d < best ? d : best;
}
// Whether the walk may stop in front of the columns dx away.
JDIST_HD bool jdist_stop(uint32_t best, uint32_t dx) { return dx * dx >= best; }
JDIST_HD uint32_t jdist_cap(uint32_t R) { return (R + 1u) * (R + 1u); }

// The value v in [0, 1] of a texel: the distance s of `which`, through the ramp.  D_out is looked at for OUTER and for a non-seed
// under SIGNED, D_in for INNER and for a seed under SIGNED.  No NaN arises from finite scale and offset: s is finite, the fused
// product-sum of three finite values is a finite real rounded once (to +-Inf at most), and minNum / maxNum with 0 and 1 clamp that.
JDIST_HD float jdist_value(uint32_t D_out, uint32_t D_in, bool is_seed, int which, float scale, float offset) {
    float s;
    if (which == JDIST_OUTER) s = sqrtf((float)D_out);
    else if (which == JDIST_INNER) s = sqrtf((float)D_in);
    else s = is_seed ? 0.5f - sqrtf((float)D_in) : sqrtf((float)D_out) - 0.5f;
    return __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(s, scale, offset), 0.0f), 1.0f);
}

// ---- the host half ----

static inline bool jdist_finite(float v) { return v - v == 0.0f; }

// nullptr for a legal descriptor (the rectangle apart: jimage_rect_check), else what is wrong with it (jh_distance puts "jh_distance: " in front).
static inline const char* jdist_desc_error(const jh_distance_desc* d) {
    if (d->channel < 0 || d->channel > 3) return "unknown channel";
    if (d->which != JDIST_OUTER && d->which != JDIST_INNER && d->which != JDIST_SIGNED) return "unknown which";
    if (d->edge != JDIST_EDGE_ZERO && d->edge != JDIST_EDGE_CLAMP) return "unknown edge mode";
    if ((d->flags & ~JDIST_STRAIGHT) != 0u) return "unknown flag bits";
    if (d->max_distance < 1u || d->max_distance > JDIST_MAX_RADIUS) return "max_distance outside [1, 255]";
    if (!jdist_finite(d->threshold)) return "threshold is not finite";
    if (!jdist_finite(d->scale) || !jdist_finite(d->offset)) return "scale or offset is not finite";
    return nullptr;
}

// The intermediate: `planes` planes of uint16_t G values, each rect_h rows of rect_w + 2 R columns.  Row v of a plane is image row
// rect_y + v; column c is image column rect_x - R + c whether that column exists or not (a column the image does not have holds the
// padding the rule implies), so every window of the row pass has 2 R + 1 columns.  SIGNED has two planes, the outer one first.
static inline uint32_t jdist_planes(int which) { return which == JDIST_SIGNED ? 2u : 1u; }
static inline uint64_t jdist_plane_cols(uint32_t rect_w, uint32_t R) { return (uint64_t)rect_w + 2u * (uint64_t)R; }
static inline uint64_t jdist_plane_rows(uint32_t rect_h) { return rect_h; }
static inline uint64_t jdist_scratch_bytes(uint32_t rect_w, uint32_t rect_h, uint32_t R, int which) {
    return jdist_planes(which) * jdist_plane_rows(rect_h) * jdist_plane_cols(rect_w, R) * 2u;
}

// The plan of desc in an image_w x image_h image, or why there is none.
static inline const char* jdist_plan(const jh_distance_desc* d, uint32_t image_w, uint32_t image_h, jh_dist_plan* plan) {
    if (const char* why = jdist_desc_error(d)) return why;
    const jimage_rect named = {d->x, d->y, d->width, d->height};
    const int check = jimage_rect_check(named, image_w, image_h);
    if (check == JIMAGE_RECT_HALF_EMPTY) return "the rectangle is empty in one dimension";
    if (check != JIMAGE_RECT_OK) return "the rectangle is not inside the image";
    const jimage_rect r = jimage_resolve(named, image_w, image_h);
    plan->x = r.x; plan->y = r.y; plan->width = r.w; plan->height = r.h;
    plan->radius = d->max_distance;
    plan->cap = jdist_cap(d->max_distance);
    plan->planes = jdist_planes(d->which);
    plan->plane_columns = (uint32_t)jdist_plane_cols(r.w, d->max_distance);
    plan->plane_rows = (uint32_t)jdist_plane_rows(r.h);
    plan->reserved = 0u;
    plan->scratch_bytes = jimage_rect_empty(r) ? 0u : jdist_scratch_bytes(r.w, r.h, d->max_distance, d->which);
    return nullptr;
}
