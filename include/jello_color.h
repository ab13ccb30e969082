// jello_color.h -- the host half of the colour-filter rule (DESIGN.md 5.10 "Colour-filter rule"): which descriptors are legal, which
// tables a descriptor needs, and the tables themselves, one entry per f16 bit pattern.  Compiled by the library
// (jello_amd/csrc/jello_hip.cpp: jh_color_filter), by the query both libraries compile (include/jello_queries.h: jq_color_tables, which
// is jh_color_tables and its host twin jl_color_tables) and by nothing else (tools/color_tables_check.cpp is its stand-alone check); tests/color_ref.py restates it.  The device half -- the table reads, the four fused steps of
// the matrix, the clamp and the one rounding to f16 -- is jello_amd/csrc/kernels_color.hip.
//
// binary64 throughout, nothing contracted; x is the value of the f16 bit pattern that indexes the entry:
//   enc      a = |x|;  12.92 a if a <= 0.0031308, else 1.055 pow(a, 1.0 / 2.4) - 0.055;  the result takes x's sign (the curve of
//            DESIGN.md 5.3, extended odd: enc(-x) = -enc(x), +-0 keep their sign, +-Inf give +-Inf)
//   dec      a = |x|;  a / 12.92 if a <= 0.04045, else pow((a + 0.055) / 1.055, 2.4);  the result takes x's sign
//   PRE_c    (c = r, g, b; only in SRGB space)  (float)enc(x);  a NaN x gives the quiet binary32 NaN 0x7fc00000
//   func_i   IDENTITY x;  LINEAR slope x + intercept;  GAMMA amplitude pow(x, exponent) + offset;
//            TABLE (n values v_0 .. v_n-1; N = n - 1): v_0 if N = 0, else c = x > 0 ? x : 0, c = c < 1 ? c : 1, k = min((int)(c N),
//            N - 1), v_k + ((x - k / N) N) (v_k+1 - v_k) -- the input is clamped for the index only, outside [0, 1] the first and the
//            last segment go on;  DISCRETE: the same c, k = min((int)(c n), n - 1), v_k.  The parameters are binary32 values widened.
//   POST_i   y = func_i(x);  with JH_COLOR_CLAMP y = y > 0 ? y : 0, then y = y < 1 ? y : 1;  in SRGB space and for i = r, g, b y = dec(y);
//            the entry is f16(y), rounded once from binary64 to nearest even;  a NaN y, and every NaN x, gives 0x7e00
//   exists   PRE_c in SRGB space; POST_i where func_i is not IDENTITY or dec applies.  A channel whose composition is the identity
//            (IDENTITY without dec: the clamp has already been applied to the value that indexes) has no table.
// pow is the libm call, the rule's only inexact library call; it never runs on the device.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "jello_hip.h"

#define JCOLOR_ENTRIES JH_COLOR_TABLE_ENTRIES  // one per f16 bit pattern
#define JCOLOR_PRE(c) (1u << (c))          // bit of `which`: the PRE table of colour channel c = 0, 1, 2
#define JCOLOR_POST(i) (1u << (4u + (i)))  // the POST table of output channel i = 0 .. 3

// The value of an f16 bit pattern, exactly.
static inline double jcolor_f16_value(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    double v;
    if (e == 0u) v = ldexp((double)m, -24);
    else if (e == 31u) v = m ? (double)NAN : (double)INFINITY;
    else v = ldexp((double)(1024u + m), (int)e - 25);
    return (h & 0x8000u) ? -v : v;
}

// binary64 to f16, one rounding to nearest even (the default rounding mode is assumed, as everywhere in the project); NaN: 0x7e00.
static inline uint16_t jcolor_f16_bits(double v) {
    if (v != v) return 0x7e00u;
    const uint16_t sign = signbit(v) ? 0x8000u : 0u;
    const double a = fabs(v);
    if (a >= 65520.0) return sign | 0x7c00u;  // (the midpoint of 65504 and 2^16 goes to the even side, which is Inf)
    if (a < 6.103515625e-05) return sign | (uint16_t)rint(ldexp(a, 24));  // below 2^-14: a multiple of 2^-24; 1024 is the smallest normal
    int e = ilogb(a);
    uint32_t m = (uint32_t)rint(ldexp(a, 10 - e));  // 1024 .. 2048
    if (m == 2048u) { m = 1024u; e++; }
    return sign | (uint16_t)(((uint32_t)(e + 15) << 10) + (m - 1024u));
}

static inline double jcolor_enc(double x) {
    const double a = fabs(x);
    const double r = a <= 0.0031308 ? 12.92 * a : 1.055 * pow(a, 1.0 / 2.4) - 0.055;
    return copysign(r, x);
}
static inline double jcolor_dec(double x) {
    const double a = fabs(x);
    const double r = a <= 0.04045 ? a / 12.92 : pow((a + 0.055) / 1.055, 2.4);
    return copysign(r, x);
}

// Why a func is refused, or null for a legal one.  Only the parameters its type uses are looked at.
static inline const char* jcolor_func_error(const jh_color_func* f) {
    switch (f->type) {
        case JH_COLOR_FUNC_IDENTITY: return nullptr;
        case JH_COLOR_FUNC_LINEAR: return isfinite(f->slope) && isfinite(f->intercept) ? nullptr : "a func parameter is not finite";
        case JH_COLOR_FUNC_GAMMA:
            return isfinite(f->amplitude) && isfinite(f->exponent) && isfinite(f->offset) ? nullptr : "a func parameter is not finite";
        case JH_COLOR_FUNC_TABLE:
        case JH_COLOR_FUNC_DISCRETE:
            if (f->n == 0u || f->n > JH_COLOR_MAX_VALUES) return "a func has no values or more than 64";
            for (uint32_t k = 0; k < f->n; k++)
                if (!isfinite(f->values[k])) return "a func parameter is not finite";
            return nullptr;
        default: return "unknown func type";
    }
}
// Why the part of a descriptor the tables depend on (space, flags, funcs) is refused, or null.
static inline const char* jcolor_desc_error(const jh_color_desc* d) {
    if (d->space != JH_COLOR_LINEAR && d->space != JH_COLOR_SRGB) return "unknown colour space";
    if ((d->flags & ~(uint32_t)JH_COLOR_CLAMP) != 0u) return "unknown flag bits";
    for (int i = 0; i < 4; i++)
        if (const char* why = jcolor_func_error(&d->func[i])) return why;
    return nullptr;
}

static inline bool jcolor_dec_applies(const jh_color_desc* d, int i) { return d->space == JH_COLOR_SRGB && i < 3; }
// The tables a legal descriptor needs: JCOLOR_PRE(c) | JCOLOR_POST(i) bits.
static inline uint32_t jcolor_which(const jh_color_desc* d) {
    uint32_t w = d->space == JH_COLOR_SRGB ? JCOLOR_PRE(0) | JCOLOR_PRE(1) | JCOLOR_PRE(2) : 0u;
    for (int i = 0; i < 4; i++)
        if (d->func[i].type != JH_COLOR_FUNC_IDENTITY || jcolor_dec_applies(d, i)) w |= JCOLOR_POST(i);
    return w;
}

// What the tables are a function of, in one comparable form: the space, the clamp bit and, per func, the type and the parameters
// the type uses (everything else zero).  The matrix is no part of it.
struct jcolor_key {
    int space;
    uint32_t clamp;
    jh_color_func func[4];
};
static inline void jcolor_key_of(const jh_color_desc* d, jcolor_key* k) {
    memset(k, 0, sizeof *k);
    k->space = d->space;
    k->clamp = d->flags & JH_COLOR_CLAMP;
    for (int i = 0; i < 4; i++) {
        const jh_color_func& f = d->func[i];
        jh_color_func& o = k->func[i];
        o.type = f.type;
        if (f.type == JH_COLOR_FUNC_LINEAR) { o.slope = f.slope; o.intercept = f.intercept; }
        if (f.type == JH_COLOR_FUNC_GAMMA) { o.amplitude = f.amplitude; o.exponent = f.exponent; o.offset = f.offset; }
        if (f.type == JH_COLOR_FUNC_TABLE || f.type == JH_COLOR_FUNC_DISCRETE) {
            o.n = f.n;
            memcpy(o.values, f.values, sizeof(float) * f.n);
        }
    }
}
static inline bool jcolor_key_equal(const jcolor_key* a, const jcolor_key* b) { return memcmp(a, b, sizeof *a) == 0; }

// func_i(x) of a legal func.
static inline double jcolor_func(const jh_color_func* f, double x) {
    switch (f->type) {
        case JH_COLOR_FUNC_LINEAR: return (double)f->slope * x + (double)f->intercept;
        case JH_COLOR_FUNC_GAMMA: return (double)f->amplitude * pow(x, (double)f->exponent) + (double)f->offset;
        case JH_COLOR_FUNC_TABLE:
        case JH_COLOR_FUNC_DISCRETE: {
            const bool table = f->type == JH_COLOR_FUNC_TABLE;
            const uint32_t N = table ? f->n - 1u : f->n;
            if (N == 0u) return (double)f->values[0];
            double c = x > 0.0 ? x : 0.0;
            c = c < 1.0 ? c : 1.0;
            uint32_t k = (uint32_t)(c * (double)N);
            if (k > N - 1u) k = N - 1u;
            if (!table) return (double)f->values[k];
            const double vk = (double)f->values[k], vk1 = (double)f->values[k + 1u];
            return vk + ((x - (double)k / (double)N) * (double)N) * (vk1 - vk);
        }
        default: return x;
    }
}

// The tables of a legal descriptor: PRE_c into pre[c * JCOLOR_ENTRIES ..] and POST_i into post[i * JCOLOR_ENTRIES ..] for the
// tables that exist (the others' entries are left alone); either pointer may be null.  Returns jcolor_which(d).
static inline uint32_t jcolor_tables(const jh_color_desc* d, float* pre, uint16_t* post) {
    const uint32_t which = jcolor_which(d);
    const bool clamp = (d->flags & JH_COLOR_CLAMP) != 0u;
    if (pre && (which & JCOLOR_PRE(0))) {
        for (uint32_t h = 0; h < JCOLOR_ENTRIES; h++) {
            const double x = jcolor_f16_value(h);
            float e = (float)jcolor_enc(x);
            if (x != x) { const uint32_t q = 0x7fc00000u; memcpy(&e, &q, 4); }
            pre[h] = e;
        }
        memcpy(pre + JCOLOR_ENTRIES, pre, sizeof(float) * JCOLOR_ENTRIES);
        memcpy(pre + 2u * JCOLOR_ENTRIES, pre, sizeof(float) * JCOLOR_ENTRIES);
    }
    for (int i = 0; post && i < 4; i++) {
        if (!(which & JCOLOR_POST(i))) continue;
        uint16_t* t = post + (size_t)i * JCOLOR_ENTRIES;
        for (uint32_t h = 0; h < JCOLOR_ENTRIES; h++) {
            const double x = jcolor_f16_value(h);
            if (x != x) { t[h] = 0x7e00u; continue; }
            double y = jcolor_func(&d->func[i], x);
            if (clamp) {
                y = y > 0.0 ? y : 0.0;
                y = y < 1.0 ? y : 1.0;
            }
            if (jcolor_dec_applies(d, i)) y = jcolor_dec(y);
            t[h] = jcolor_f16_bits(y);
        }
    }
    return which;
}
