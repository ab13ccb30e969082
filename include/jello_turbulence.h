// jello_turbulence.h -- the host half of the turbulence rule (DESIGN.md 5.15 "Turbulence rule"; include/jello_hip.h "Turbulence" states
// all of it): which descriptor is legal (its rectangle apart: jello_image.h), the generator, the tables and the key they are resident
// under, the plan -- binary64 appears in the plan and the tables only --; and the part of the device half that has cases: the
// cell / fraction split, the stitch step, the lattice walk, the s-curve, the dot and the lerp, as functions the kernel compiles too.
// Compiled by the library (jello_amd/csrc/jello_hip.cpp: jh_turbulence), by the kernel
// (jello_amd/csrc/kernels_turbulence.hip), by the queries both libraries compile (include/jello_queries.h: jq_turbulence_plan, jq_turbulence_tables)
// and by tools/turbulence_check.cpp; tests/turbulence_ref.py restates it.
//
//   seed      the specification's setup_seed: s <= 0 becomes -(s mod (m - 1)) + 1 (the remainder C's, towards zero), s > m - 1 becomes
//             m - 1; m = 2^31 - 1.  The result is the KEY of the tables.
//   random    Park-Miller: a = 16807, q = 127773, r = 2836 (Schrage): s' = a (s mod q) - r (s div q), + m where that is <= 0.
//   tables    the specification's init, its order of draws: for k = 0 .. 3, i = 0 .. 255: x, y = ((random mod 512) - 256) / 256 (exact);
//             s = sqrt(x x + y y) in binary64 left to right; G[k][i] = ((float)(x / s), (float)(y / s)), each quotient binary64 rounded
//             once -- and (+0, +0) where x = y = 0 (the specification divides 0 by 0 there).  Then P[i] = i and for i = 255 .. 1:
//             swap P[i] and P[random mod 256].  The specification's duplicated upper halves (P[256 + i] = P[i], likewise G) are not
//             stored: every index is masked with 255 instead, which reads the same entry (jturb_lattice; tools/turbulence_check.cpp).
//   plan      per axis: f = base_frequency; under stitch and f != 0: t = tile_w f, lo = floor(t) / tile_w, hi = ceil(t) / tile_w, f =
//             lo if lo != 0 and f / lo < hi / f, else hi (every operation binary64, rounded once).  step = nearbyint(f 2^32); start =
//             nearbyint(((origin + 0.5) f) 2^32), ties to even; under stitch width = (int)(tile_w f + 0.5), wrap = floor(tile_x f) +
//             width (the specification's + 4096 dropped from both sides of its comparison), otherwise both 0.
//   legal     L = (2^62 - 1) >> max(octaves - 1, 0).  |f 2^32| and |(origin + 0.5) f 2^32| below 2^62 as binary64; |start| <= L;
//             max_extent = the largest image extent W with start + (W - 1) step <= L (at most 2^32 - 1); under stitch tile_w f + 0.5
//             and |floor(tile_x f)| below 2^31, and |wrap| and width at most (2^31 - 1) >> max(octaves - 1, 0).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "jello_hip.h"

#if defined(__HIPCC__)
#define JTURB_HD __host__ __device__ __forceinline__
#else
#define JTURB_HD static inline
#endif

#define JTURB_FRACTAL_NOISE 0
#define JTURB_TURBULENCE 1
#define JTURB_KINDS 2
#define JTURB_MAX_OCTAVES 16u
#define JTURB_RAND_M 2147483647
#define JTURB_RAND_A 16807
#define JTURB_RAND_Q 127773
#define JTURB_RAND_R 2836
#define JTURB_GRADIENT_FLOATS 2048u                          // G[4][256][2]
#define JTURB_DEVICE_BYTES (JTURB_GRADIENT_FLOATS * 4u + 256u)  // what the kernel reads: G as [b][channel][2], then P

// ---- the legal descriptor ----

// nullptr for a legal descriptor (the rectangle, the image and the position range apart: jturb_plan), else what is wrong with it
// (jh_turbulence puts "jh_turbulence: " in front).  The tile is not looked at without stitch.
static inline const char* jturb_desc_error(const jh_turbulence_desc* d) {
    if (d->kind < 0 || d->kind >= JTURB_KINDS) return "unknown kind";
    if (d->octaves > JTURB_MAX_OCTAVES) return "more than 16 octaves";
    if (d->stitch != 0 && d->stitch != 1) return "stitch is neither 0 nor 1";
    for (int a = 0; a < 2; a++) {
        if (!(isfinite(d->base_frequency[a]) && d->base_frequency[a] >= 0.0)) return "a base_frequency is negative or not finite";
        if (!isfinite(d->origin[a])) return "the origin is not finite";
    }
    if (d->stitch) {
        for (int a = 0; a < 4; a++)
            if (!isfinite(d->tile[a])) return "the stitch tile is not finite";
        if (!(d->tile[2] > 0.0 && d->tile[3] > 0.0)) return "the stitch tile is empty";
    }
    return nullptr;
}

// ---- the generator and the tables ----

static inline int32_t jturb_setup_seed(int32_t seed) {
    int64_t s = seed;
    if (s <= 0) s = -(s % (JTURB_RAND_M - 1)) + 1;
    if (s > JTURB_RAND_M - 1) s = JTURB_RAND_M - 1;
    return (int32_t)s;
}
static inline int32_t jturb_random(int32_t s) {
    int32_t r = JTURB_RAND_A * (s % JTURB_RAND_Q) - JTURB_RAND_R * (s / JTURB_RAND_Q);  // (both products and the difference fit)
    if (r <= 0) r += JTURB_RAND_M;
    return r;
}
// The tables of a seed: P[256] and G[4][256][2] (either may be null).  Returns the key.
static inline uint32_t jturb_tables(int32_t seed, uint8_t* P, float* G) {
    int32_t s = jturb_setup_seed(seed);
    const uint32_t key = (uint32_t)s;
    for (uint32_t k = 0; k < 4u; k++)
        for (uint32_t i = 0; i < 256u; i++) {
            s = jturb_random(s);
            const double x = (double)((s % 512) - 256) / 256.0;
            s = jturb_random(s);
            const double y = (double)((s % 512) - 256) / 256.0;
            const double len = sqrt(x * x + y * y);
            if (G) {
                G[(k * 256u + i) * 2u] = len == 0.0 ? 0.0f : (float)(x / len);
                G[(k * 256u + i) * 2u + 1u] = len == 0.0 ? 0.0f : (float)(y / len);
            }
        }
    uint8_t perm[256];
    for (uint32_t i = 0; i < 256u; i++) perm[i] = (uint8_t)i;
    for (uint32_t i = 255u; i > 0u; i--) {
        s = jturb_random(s);
        const uint32_t j = (uint32_t)(s % 256);
        const uint8_t t = perm[i];
        perm[i] = perm[j];
        perm[j] = t;
    }
    if (P) memcpy(P, perm, 256);
    return key;
}
// What the kernel reads, JTURB_DEVICE_BYTES: the gradients as [b][channel][2] binary32 -- one corner's four channels are 32
// contiguous bytes -- then P.
static inline void jturb_device_tables(const uint8_t* P, const float* G, char* blob) {
    float* g = (float*)blob;
    for (uint32_t b = 0; b < 256u; b++)
        for (uint32_t c = 0; c < 4u; c++) {
            g[(b * 4u + c) * 2u] = G[(c * 256u + b) * 2u];
            g[(b * 4u + c) * 2u + 1u] = G[(c * 256u + b) * 2u + 1u];
        }
    memcpy(blob + JTURB_GRADIENT_FLOATS * 4u, P, 256);
}

// ---- the plan ----

static inline uint32_t jturb_shift(uint32_t octaves) { return octaves ? octaves - 1u : 0u; }
// The plan of a descriptor; nullptr, or what is wrong with it (the plan is then untouched).
static inline const char* jturb_plan(const jh_turbulence_desc* d, jh_turb_plan* out) {
    if (const char* why = jturb_desc_error(d)) return why;
    const double two32 = 4294967296.0, two62 = 4611686018427387904.0, two31 = 2147483648.0;
    const uint32_t shift = jturb_shift(d->octaves);
    const __int128 L = ((((__int128)1) << 62) - 1) >> shift;
    jh_turb_plan p;
    memset(&p, 0, sizeof p);
    for (int a = 0; a < 2; a++) {
        double f = d->base_frequency[a];
        const double tile_o = d->tile[a], tile_e = d->tile[2 + a];
        if (d->stitch && f != 0.0) {
            const double t = tile_e * f;
            const double lo = floor(t) / tile_e, hi = ceil(t) / tile_e;
            f = (lo != 0.0 && f / lo < hi / f) ? lo : hi;
            if (!isfinite(f)) return "the stitched frequency is not finite";
        }
        const double fs = f * two32;
        if (!(fs < two62)) return "a base_frequency of 2^30 cells per texel or more";
        const double c = d->origin[a] + 0.5;
        const double cf = c * f;
        const double os = cf * two32;
        if (!(fabs(os) < two62)) return "the origin is beyond the position range";
        p.frequency[a] = f;
        p.step[a] = (int64_t)nearbyint(fs);
        p.start[a] = (int64_t)nearbyint(os);
        const __int128 start = p.start[a];
        if (start > L || -start > L) return "the origin is beyond the position range of this many octaves";
        __int128 extent = 0xffffffffu;
        if (p.step[a] != 0) {
            const __int128 e = (L - start) / (__int128)p.step[a] + 1;
            extent = e < extent ? e : extent;
        }
        p.max_extent[a] = (uint32_t)extent;
        if (d->stitch) {
            const double tf = tile_e * f;
            const double wd = tf + 0.5;
            const double fl = floor(tile_o * f);
            if (!(wd < two31 && fabs(fl) < two31)) return "the stitch tile is beyond the lattice range";
            const int64_t width = (int64_t)wd, wrap = (int64_t)fl + width, lim = (int64_t)0x7fffffff >> shift;
            if (width > lim || wrap > lim || -wrap > lim) return "the stitch tile is beyond the lattice range of this many octaves";
            p.width[a] = (int32_t)width;
            p.wrap[a] = (int32_t)wrap;
        }
    }
    p.key = (uint32_t)jturb_setup_seed(d->seed);
    p.stitched = (uint32_t)d->stitch;
    *out = p;
    return nullptr;
}

// ---- what the kernel compiles too ----

// A position p (2^-32 cell): its cell (an arithmetic shift: a floor) and the fraction r0 in [0, 1), 24 bits, exact.
JTURB_HD void jturb_split(int64_t p, int32_t* cell, float* r0) {
    *cell = (int32_t)(p >> 32);
    *r0 = (float)((uint32_t)p >> 8) * 5.9604644775390625e-08f;
}
// A lattice index i (a cell, or a cell + 1) under stitch, BEFORE the mask with 255: the comparison on the whole index, the
// subtraction modulo 2^32 (only its low 8 bits are used).
JTURB_HD uint32_t jturb_stitch(int32_t i, int32_t wrap, int32_t width) { return (uint32_t)i - (i >= wrap ? (uint32_t)width : 0u); }
// The lattice walk, on masked indices: first the x half -- P[bx0], P[bx1] -- then b[] = {b00, b10, b01, b11}.
JTURB_HD void jturb_lattice_x(const uint8_t* P, uint32_t bx0, uint32_t bx1, uint32_t* i, uint32_t* j) {
    *i = P[bx0 & 255u];
    *j = P[bx1 & 255u];
}
JTURB_HD void jturb_lattice_y(const uint8_t* P, uint32_t i, uint32_t j, uint32_t by0, uint32_t by1, uint32_t b[4]) {
    b[0] = P[(i + by0) & 255u];
    b[1] = P[(j + by0) & 255u];
    b[2] = P[(i + by1) & 255u];
    b[3] = P[(j + by1) & 255u];
}
JTURB_HD float jturb_s(float t) { return (t * t) * __builtin_fmaf(-2.0f, t, 3.0f); }
JTURB_HD float jturb_dot(float rx, float ry, float gx, float gy) { return __builtin_fmaf(ry, gy, rx * gx); }
JTURB_HD float jturb_lerp(float t, float a, float b) { return __builtin_fmaf(t, b - a, a); }
// One channel's noise of one octave from the four corners' gradients g[corner] = (x, y), corners as jturb_lattice_y's.
JTURB_HD float jturb_noise(float rx0, float ry0, float sx, float sy, const float g[4][2]) {
    const float rx1 = rx0 - 1.0f, ry1 = ry0 - 1.0f;
    const float u00 = jturb_dot(rx0, ry0, g[0][0], g[0][1]), u10 = jturb_dot(rx1, ry0, g[1][0], g[1][1]);
    const float u01 = jturb_dot(rx0, ry1, g[2][0], g[2][1]), u11 = jturb_dot(rx1, ry1, g[3][0], g[3][1]);
    return jturb_lerp(sy, jturb_lerp(sx, u00, u10), jturb_lerp(sx, u01, u11));
}
// The result of a sum: a channel's value before the rounding to f16.
JTURB_HD float jturb_result(int kind, float sum) {
    const float v = kind == JTURB_FRACTAL_NOISE ? __builtin_fmaf(sum, 0.5f, 0.5f) : sum;
    return fminf(fmaxf(v, 0.0f), 1.0f);
}

// Texel (X, Y) of the image by the rule, on the host: the four channels before the rounding to f16, from P[256] and G[4][256][2].
static inline void jturb_texel(const jh_turb_plan* p, int kind, uint32_t octaves, const uint8_t* P, const float* G, uint32_t X, uint32_t Y, float out[4]) {
    int64_t px = p->start[0] + (int64_t)X * p->step[0], py = p->start[1] + (int64_t)Y * p->step[1];
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ratio = 1.0f;
    for (uint32_t k = 0; k < octaves; k++) {
        int32_t ix, iy;
        float rx0, ry0;
        jturb_split(px * ((int64_t)1 << k), &ix, &rx0);
        jturb_split(py * ((int64_t)1 << k), &iy, &ry0);
        uint32_t bx0 = (uint32_t)ix, bx1 = (uint32_t)ix + 1u, by0 = (uint32_t)iy, by1 = (uint32_t)iy + 1u;
        if (p->stitched) {
            const int32_t wx = p->wrap[0] * (1 << k), nx = p->width[0] * (1 << k), wy = p->wrap[1] * (1 << k), ny = p->width[1] * (1 << k);
            bx0 = jturb_stitch(ix, wx, nx); bx1 = jturb_stitch(ix + 1, wx, nx);
            by0 = jturb_stitch(iy, wy, ny); by1 = jturb_stitch(iy + 1, wy, ny);
        }
        uint32_t i, j, b[4];
        jturb_lattice_x(P, bx0, bx1, &i, &j);
        jturb_lattice_y(P, i, j, by0 & 255u, by1 & 255u, b);
        const float sx = jturb_s(rx0), sy = jturb_s(ry0);
        for (uint32_t c = 0; c < 4u; c++) {
            float g[4][2];
            for (uint32_t q = 0; q < 4u; q++) { g[q][0] = G[(c * 256u + b[q]) * 2u]; g[q][1] = G[(c * 256u + b[q]) * 2u + 1u]; }
            const float n = jturb_noise(rx0, ry0, sx, sy, g);
            sum[c] = __builtin_fmaf(kind == JTURB_TURBULENCE ? fabsf(n) : n, ratio, sum[c]);
        }
        ratio *= 0.5f;
    }
    for (uint32_t c = 0; c < 4u; c++) out[c] = jturb_result(kind, sum[c]);
}
