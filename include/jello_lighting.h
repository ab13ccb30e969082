// jello_lighting.h -- the host half of the lighting rule (DESIGN.md 5.14 "Lighting rule"; include/jello_hip.h "Lighting" states all of
// it): which descriptor is legal (its rectangle apart: jello_image.h), the plan -- the only place binary64 appears --, the power
// tables, which of them a descriptor needs and the key they are resident under; and the part of the device half that has cases: the
// surface normal's (span, wsum) selection, its side sums and the table's index rule, as functions the kernel compiles too.  Compiled by
// the library (jello_amd/csrc/jello_hip.cpp: jh_lighting), by the kernel
// (jello_amd/csrc/kernels_lighting.hip), by the queries both libraries compile (include/jello_queries.h: jq_lighting_plan, jq_lighting_tables) and by
// tools/lighting_check.cpp; tests/lighting_ref.py restates it.
//
//   s         s[span - 1][wsum - 2] = (float)(-(double)surface_scale * 2.0 / (double)(span * wsum)), span in {1, 2}, wsum in {2, 3, 4}:
//             the specification's -surfaceScale times 1/4 (2, 4), 1/3 (2, 3), 1/2 (1, 4; 2, 2), 2/3 (1, 3) and 1 (1, 2)
//   unit      (x, y, z) / sqrt(x x + y y + z z): the sum and the root in binary64, left to right; each quotient in binary64, rounded once
//   table     T[i] = (float)pow((double)i / 4096.0, (double)e), i = 0 .. 4096: libm in binary64, rounded once; it never runs on the device
//   key       the bit patterns of specular_exponent and spot_exponent where their table is needed, 0 where it is not
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "jello_hip.h"

#if defined(__HIPCC__)
#define JLIGHT_HD __host__ __device__ __forceinline__
#else
#define JLIGHT_HD static inline
#endif

#define JLIGHT_DIFFUSE 0
#define JLIGHT_SPECULAR 1
#define JLIGHT_KINDS 2
#define JLIGHT_DISTANT 0
#define JLIGHT_POINT 1
#define JLIGHT_SPOT 2
#define JLIGHT_LIGHTS 3
#define JLIGHT_STEPS 4096
#define JLIGHT_ENTRIES 4097u  // T[0 .. 4096]
#define JLIGHT_TABLE_SPEC 1u  // bits of `which`
#define JLIGHT_TABLE_SPOT 2u
#define JLIGHT_MAX_EXTENT (1u << 23)  // (float)X + 0.5f is exact below it

// ---- the legal descriptor ----

static inline bool jlight_exponent_ok(float e) { return e >= 1.0f && e <= 128.0f; }  // (a NaN is not)
static inline bool jlight_fits_float(double v) { return isfinite(v) && isfinite((float)v); }
// |(x, y, z)| by the rule.
static inline double jlight_length(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }
static inline bool jlight_length_ok(double len) { return isfinite(len) && len > 0.0; }

// nullptr for a legal descriptor (the rectangle and the images apart), else what is wrong with it (jh_lighting puts "jh_lighting: " in
// front).  Fields the kind and the light do not use are not looked at.
static inline const char* jlight_desc_error(const jh_lighting_desc* d) {
    if (d->kind < 0 || d->kind >= JLIGHT_KINDS) return "unknown kind";
    if (d->light < 0 || d->light >= JLIGHT_LIGHTS) return "unknown light";
    if (!isfinite(d->surface_scale)) return "the surface_scale is not finite";
    if (!(isfinite(d->constant) && d->constant >= 0.0f)) return "the constant is negative or not finite";
    if (d->kind == JLIGHT_SPECULAR && !jlight_exponent_ok(d->specular_exponent)) return "the specular_exponent is outside [1, 128]";
    for (int c = 0; c < 3; c++)
        if (!(isfinite(d->color[c]) && d->color[c] >= 0.0f)) return "a color component is negative or not finite";
    if (d->light == JLIGHT_DISTANT) {
        for (int c = 0; c < 3; c++)
            if (!isfinite(d->direction[c])) return "the direction is not finite";
        if (!jlight_length_ok(jlight_length(d->direction[0], d->direction[1], d->direction[2]))) return "the direction has no finite non-zero length";
        return nullptr;
    }
    for (int c = 0; c < 3; c++)
        if (!jlight_fits_float(d->position[c])) return "the position is not finite in binary32";
    if (d->light == JLIGHT_SPOT) {
        double v[3];
        for (int c = 0; c < 3; c++) {
            if (!isfinite(d->points_at[c])) return "points_at is not finite";
            v[c] = d->points_at[c] - d->position[c];
        }
        if (!jlight_length_ok(jlight_length(v[0], v[1], v[2]))) return "points_at is the position, or too far from it";
        if (!jlight_exponent_ok(d->spot_exponent)) return "the spot_exponent is outside [1, 128]";
        if (!(d->cone_cos >= -1.0 && d->cone_cos <= 1.0)) return "the cone_cos is outside [-1, 1]";
    }
    return nullptr;
}

// ---- the plan ----

static inline void jlight_unit(double x, double y, double z, float out[3]) {
    const double len = jlight_length(x, y, z);
    out[0] = (float)(x / len);
    out[1] = (float)(y / len);
    out[2] = (float)(z / len);
}
// The plan of a descriptor; nullptr, or jlight_desc_error's answer (the plan is then untouched).
static inline const char* jlight_plan(const jh_lighting_desc* d, jh_light_plan* p) {
    if (const char* why = jlight_desc_error(d)) return why;
    memset(p, 0, sizeof *p);
    for (uint32_t span = 1; span <= 2u; span++)
        for (uint32_t wsum = 2; wsum <= 4u; wsum++) p->s[span - 1u][wsum - 2u] = (float)(-(double)d->surface_scale * 2.0 / (double)(span * wsum));
    if (d->light == JLIGHT_DISTANT) {
        jlight_unit(d->direction[0], d->direction[1], d->direction[2], p->ldir);
        return nullptr;
    }
    for (int c = 0; c < 3; c++) p->p[c] = (float)d->position[c];
    if (d->light == JLIGHT_SPOT) {
        jlight_unit(d->points_at[0] - d->position[0], d->points_at[1] - d->position[1], d->points_at[2] - d->position[2], p->sdir);
        p->cone = (float)d->cone_cos;
    }
    return nullptr;
}

// ---- the tables ----

static inline void jlight_table(float e, float* T) {
    for (uint32_t i = 0; i < JLIGHT_ENTRIES; i++) T[i] = (float)pow((double)i / 4096.0, (double)e);
}
// The tables a legal descriptor needs: JLIGHT_TABLE_SPEC | JLIGHT_TABLE_SPOT bits.
static inline uint32_t jlight_which(const jh_lighting_desc* d) {
    return (d->kind == JLIGHT_SPECULAR && d->specular_exponent != 1.0f ? JLIGHT_TABLE_SPEC : 0u) |
           (d->light == JLIGHT_SPOT && d->spot_exponent != 1.0f ? JLIGHT_TABLE_SPOT : 0u);
}
// The tables of a legal descriptor, each that is needed where its pointer is not null.  Returns jlight_which(d).
static inline uint32_t jlight_tables(const jh_lighting_desc* d, float* spec_table, float* spot_table) {
    const uint32_t which = jlight_which(d);
    if (spec_table && (which & JLIGHT_TABLE_SPEC)) jlight_table(d->specular_exponent, spec_table);
    if (spot_table && (which & JLIGHT_TABLE_SPOT)) jlight_table(d->spot_exponent, spot_table);
    return which;
}
struct jlight_key { uint32_t spec_bits, spot_bits; };
static inline void jlight_key_of(const jh_lighting_desc* d, jlight_key* k) {
    const uint32_t which = jlight_which(d);
    k->spec_bits = k->spot_bits = 0u;
    if (which & JLIGHT_TABLE_SPEC) memcpy(&k->spec_bits, &d->specular_exponent, 4);
    if (which & JLIGHT_TABLE_SPOT) memcpy(&k->spot_bits, &d->spot_exponent, 4);
}
static inline bool jlight_key_equal(const jlight_key* a, const jlight_key* b) { return a->spec_bits == b->spec_bits && a->spot_bits == b->spot_bits; }

// ---- what the kernel compiles too ----

// The table's index rule for t in [0, 1]: the segment i and the position f in it; Pw = fmaf(f, T[i + 1] - T[i], T[i]).
JLIGHT_HD int jlight_segment(float t, float* f) {
    const float u = t * 4096.0f;
    int i = (int)u;
    i = i < JLIGHT_STEPS - 1 ? i : JLIGHT_STEPS - 1;
    *f = u - (float)i;
    return i;
}
JLIGHT_HD float jlight_pw(const float* T, float t) {
    float f;
    const int i = jlight_segment(t, &f);
    return fmaf(f, T[i + 1] - T[i], T[i]);
}

// s(span, wsum) of the plan's six values s = &plan.s[0][0], span in {1, 2} (a span of 0 never asks), wsum in {2, 3, 4}: selects, so
// that the kernel indexes nothing.
JLIGHT_HD float jlight_s(const float* s, uint32_t span, uint32_t wsum) {
    const float one = wsum == 2u ? s[0] : (wsum == 3u ? s[1] : s[2]);
    const float two = wsum == 2u ? s[3] : (wsum == 3u ? s[4] : s[5]);
    return span == 2u ? two : one;
}
// A side sum: the weights (1, 2, 1) over (a0, a1, a2), of which a0 exists if `before` and a2 if `after`, ascending, left to right.
JLIGHT_HD float jlight_side(bool before, bool after, float a0, float a1, float a2) {
    const float mid = 2.0f * a1;
    const float c = before ? a0 + mid : mid;
    return after ? c + a2 : c;
}
// (Nx, Ny) at texel (X, Y) of a W x H image from a[j][i] = A(clamp(X - 1 + i, 0, W - 1), clamp(Y - 1 + j, 0, H - 1)): the clamped
// 3 x 3 neighbourhood, whose entries beyond the image are never part of a sum (they stand for x_lo = X or x_hi = X, likewise in y).
JLIGHT_HD void jlight_normal(const float* s, uint32_t X, uint32_t Y, uint32_t W, uint32_t H, const float (&a)[3][3], float* nx, float* ny) {
    const bool left = X > 0u, right = X + 1u < W, up = Y > 0u, down = Y + 1u < H;
    const uint32_t span_x = (uint32_t)left + (uint32_t)right, span_y = (uint32_t)up + (uint32_t)down;
    const uint32_t wsum_x = 2u + span_x, wsum_y = 2u + span_y;
    const float gx = jlight_side(up, down, a[0][2], a[1][2], a[2][2]) - jlight_side(up, down, a[0][0], a[1][0], a[2][0]);
    const float gy = jlight_side(left, right, a[2][0], a[2][1], a[2][2]) - jlight_side(left, right, a[0][0], a[0][1], a[0][2]);
    *nx = span_x == 0u ? 0.0f : jlight_s(s, span_x, wsum_y) * gx;
    *ny = span_y == 0u ? 0.0f : jlight_s(s, span_y, wsum_x) * gy;
}
