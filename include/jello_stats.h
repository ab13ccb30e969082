// jello_stats.h -- the stats rule (DESIGN.md 5.22 "Stats rule"): the content box, the channel extremes and four 256-bin histograms of a
// rectangle of an RGBA16F image.  Which descriptor is legal (its rectangle: jello_image.h), the plan jh_stats_plan answers, and -- the
// one text the kernels (jello_amd/csrc/kernels_stats.hip), the library's queries and their host twin (include/jello_queries.h) and the
// stand-alone check (tools/stats_check.cpp) all compile -- the content test, the 16-bit order key, the codes, the words of a partial
// record with their combine, and the words of the record.  tests/stats_ref.py restates the rule from the set definition and includes
// nothing of this file.
//
//   content   a texel whose chosen channel, widened to binary32, is >= threshold: jdist_is_seed of jello_distance.h, shared, not restated
//   key       of a non-NaN f16 pattern h, 16 bits, compared UNSIGNED: negative: ~h, else h | 0x8000.  -Inf 0x03FF < ... < -0 0x7FFF <
//             +0 0x8000 < ... < +Inf 0xFC00: the order of jmorph_key (jello_morph.h) on the widened value -- tools/stats_check.cpp walks
//             all patterns in key order and sees jmorph_key rise.  No value lies above key(+Inf) or below key(-Inf): the neutral
//             elements of min and max, and what a channel without a non-NaN value reports (min_bits 0x7C00, max_bits 0xFC00)
//   code      q = clamp01(v), jh_blit's clamp by comparisons (jello_amd/csrc/blit_convert.h: NaN -> 0, -0 -> +0, +Inf -> 1).  LINEAR:
//             rintf(q * 255.0f); the product of an f16 (11 bits) and 255 (8 bits) is exact in binary32.  SRGB: #{k : t[k] <= q} over
//             the 255 thresholds of jello_amd/csrc/srgb_encode_lut.h -- on the device blit_srgb's estimate corrected against the same
//             table (blit_convert.h), the same code by construction.  Alpha is always LINEAR
//   partial   what one workgroup of the first launch has seen, JSTATS_PARTIAL_WORDS uint32_t: the content count, the box (min x, min y,
//             max x + 1, max y + 1 in image coordinates), the population count, four NaN counts, four min keys, four max keys, then
//             the bins [channel][code].  Word i of the combination of two partials is jstats_word_combine(i, a, b): a sum, a min or a
//             max of integers -- commutative and associative, so the bytes do not depend on how the texels were dealt out
//   record    jstats_record_word(j, ...) of the combined partial: word j of jh_stats_record, parts not asked for as zeros
#pragma once
#include <stdint.h>

#include "jello_displace.h"  // jdisp_f16: the value of an f16 bit pattern as binary32, host and device
#include "jello_distance.h"  // jdist_is_seed, jdist_finite
#include "jello_hip.h"
#include "jello_image.h"

#if defined(__HIPCC__)
#define JSTATS_HD __host__ __device__ __forceinline__
#else
#define JSTATS_HD static inline
#endif

#define JSTATS_ALL 0
#define JSTATS_CONTENT 1
#define JSTATS_LINEAR 0
#define JSTATS_SRGB 1
#define JSTATS_BOUNDS 1u
#define JSTATS_EXTREMES 2u
#define JSTATS_HISTOGRAM 4u
#define JSTATS_MAX_TEXELS 2147483648ull
#define JSTATS_MAX_PARTIALS 1024u

// ---- the pieces ----

JSTATS_HD float jstats_f16(uint16_t bits) { return jdisp_f16(bits); }
JSTATS_HD bool jstats_is_nan(uint32_t h) { return (h & 0x7fffu) > 0x7c00u; }
JSTATS_HD bool jstats_is_content(uint16_t channel_bits, float threshold) { return jdist_is_seed(jstats_f16(channel_bits), threshold); }
// The key of a non-NaN f16 pattern, and the pattern of a key.
JSTATS_HD uint32_t jstats_key(uint32_t h) { return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u); }
JSTATS_HD uint32_t jstats_unkey(uint32_t k) { return (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu); }
#define JSTATS_KEY_MIN_NEUTRAL 0xfc00u  // key(+Inf): min_bits 0x7C00
#define JSTATS_KEY_MAX_NEUTRAL 0x03ffu  // key(-Inf): max_bits 0xFC00
// jh_blit's clamp (blit_clamp01 of jello_amd/csrc/blit_convert.h, which is device code; this is the text host and device compile).
JSTATS_HD float jstats_clamp01(float p) {
    const float v = p > 0.0f ? p : 0.0f;
    return v < 1.0f ? v : 1.0f;
}
JSTATS_HD uint32_t jstats_linear_code(float q) { return (uint32_t)__builtin_rintf(q * 255.0f); }
// #{k : t[k] <= q} over the 255 ascending thresholds t, q in [0, 1].
JSTATS_HD uint32_t jstats_srgb_code(float q, const float* t) {
    uint32_t lo = 0u, hi = 255u;  // the count lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (t[mid] <= q) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
// The code of channel c (0..3) of a texel under `transfer`; t: the thresholds (read under SRGB only).
JSTATS_HD uint32_t jstats_code(int transfer, uint32_t c, uint16_t bits, const float* t) {
    const float q = jstats_clamp01(jstats_f16(bits));
    return transfer == JSTATS_SRGB && c != 3u ? jstats_srgb_code(q, t) : jstats_linear_code(q);
}

// ---- the partial record ----

enum {
    JSTATS_W_CONTENT = 0,  // content texels
    JSTATS_W_X0 = 1, JSTATS_W_Y0 = 2, JSTATS_W_X1 = 3, JSTATS_W_Y1 = 4,  // the box: min x, min y, max x + 1, max y + 1
    JSTATS_W_POP = 5,      // texels of the population
    JSTATS_W_NAN = 6,      // [4]
    JSTATS_W_MIN = 10,     // [4] keys
    JSTATS_W_MAX = 14,     // [4] keys
    JSTATS_W_HIST = 18,    // [4][256]
    JSTATS_PARTIAL_WORDS = 18 + 1024
};
#define JSTATS_PARTIAL_BYTES (4u * (uint32_t)JSTATS_PARTIAL_WORDS)  // 4168: a multiple of 8
#define JSTATS_RECORD_HEAD_WORDS 22u                                 // the words of jh_stats_record in front of its histogram

enum { JSTATS_OP_SUM = 0, JSTATS_OP_MIN = 1, JSTATS_OP_MAX = 2 };
JSTATS_HD int jstats_word_op(uint32_t i) {
    if (i == JSTATS_W_X0 || i == JSTATS_W_Y0 || (i >= JSTATS_W_MIN && i < JSTATS_W_MAX)) return JSTATS_OP_MIN;
    if (i == JSTATS_W_X1 || i == JSTATS_W_Y1 || (i >= JSTATS_W_MAX && i < JSTATS_W_HIST)) return JSTATS_OP_MAX;
    return JSTATS_OP_SUM;
}
// Word i of the partial of no texel at all.
JSTATS_HD uint32_t jstats_word_neutral(uint32_t i) {
    if (i == JSTATS_W_X0 || i == JSTATS_W_Y0) return 0xffffffffu;
    if (i >= JSTATS_W_MIN && i < JSTATS_W_MAX) return JSTATS_KEY_MIN_NEUTRAL;
    if (i >= JSTATS_W_MAX && i < JSTATS_W_HIST) return JSTATS_KEY_MAX_NEUTRAL;
    return 0u;
}
JSTATS_HD uint32_t jstats_word_combine(uint32_t i, uint32_t a, uint32_t b) {
    const int op = jstats_word_op(i);
    return op == JSTATS_OP_SUM ? a + b : (op == JSTATS_OP_MIN ? (b < a ? b : a) : (a < b ? b : a));
}

// ---- the record ----

struct jstats_head { uint32_t x, y, w, h, what, population, transfer; };  // the resolved rectangle and the descriptor's three words
// Whether the population count, the NaN counts (either part) are written.
JSTATS_HD bool jstats_counts(uint32_t what) { return (what & (JSTATS_EXTREMES | JSTATS_HISTOGRAM)) != 0u; }
// Word j < JSTATS_RECORD_HEAD_WORDS of the record, from the combined words p[0 .. JSTATS_W_HIST) of all partials.
JSTATS_HD uint32_t jstats_record_word(uint32_t j, const jstats_head& hd, const uint32_t* p) {
    switch (j) {
        case 0: return hd.x;
        case 1: return hd.y;
        case 2: return hd.w;
        case 3: return hd.h;
        case 4: return hd.what;
        case 5: return hd.population;
        case 6: return hd.transfer;
        case 7: return 0u;
        default: break;
    }
    if (hd.w == 0u || hd.h == 0u) return 0u;  // an image without texels: zeros
    if (j == 8u) return p[JSTATS_W_CONTENT];
    if (j < 13u) return (hd.what & JSTATS_BOUNDS) && p[JSTATS_W_CONTENT] != 0u ? p[JSTATS_W_X0 + (j - 9u)] : 0u;
    if (j == 13u) return jstats_counts(hd.what) ? p[JSTATS_W_POP] : 0u;
    if (j < 18u) return jstats_counts(hd.what) ? p[JSTATS_W_NAN + (j - 14u)] : 0u;
    if (!(hd.what & JSTATS_EXTREMES)) return 0u;
    const uint32_t k = (j < 20u ? JSTATS_W_MIN : JSTATS_W_MAX) + 2u * ((j - 18u) & 1u);  // two 16-bit patterns to a word, the lower channel low
    return jstats_unkey(p[k]) | (jstats_unkey(p[k + 1u]) << 16);
}
// Word JSTATS_RECORD_HEAD_WORDS + i of the record: bin i of the histogram, from the combined bin.
JSTATS_HD uint32_t jstats_record_bin(const jstats_head& hd, uint32_t combined) {
    return (hd.what & JSTATS_HISTOGRAM) && hd.w != 0u && hd.h != 0u ? combined : 0u;
}

// ---- the host half ----

// nullptr for a legal descriptor (the rectangle apart: jimage_rect_check), else what is wrong with it (jh_stats puts "jh_stats: " in front).
static inline const char* jstats_desc_error(const jh_stats_desc* d) {
    if (d->what == 0u) return "what names no part";
    if ((d->what & ~(JSTATS_BOUNDS | JSTATS_EXTREMES | JSTATS_HISTOGRAM)) != 0u) return "unknown bits in what";
    if (d->channel < 0 || d->channel > 3) return "unknown channel";
    if (d->population != JSTATS_ALL && d->population != JSTATS_CONTENT) return "unknown population";
    if (d->transfer != JSTATS_LINEAR && d->transfer != JSTATS_SRGB) return "unknown transfer";
    if (!jdist_finite(d->threshold)) return "threshold is not finite";
    return nullptr;
}
// What is wrong with the rectangle desc names in an image_w x image_h image, or nullptr and the rectangle resolved.
static inline const char* jstats_rect_error(const jh_stats_desc* d, uint32_t image_w, uint32_t image_h, jimage_rect* r) {
    const jimage_rect named = {d->x, d->y, d->width, d->height};
    const int check = jimage_rect_check(named, image_w, image_h);
    if (check == JIMAGE_RECT_HALF_EMPTY) return "the rectangle is empty in one dimension";
    if (check != JIMAGE_RECT_OK) return "the rectangle is not inside the image";
    *r = jimage_resolve(named, image_w, image_h);
    if ((uint64_t)r->w * r->h > JSTATS_MAX_TEXELS) return "the rectangle has more than 2^31 texels";
    return nullptr;
}
static inline uint64_t jstats_scratch_bytes(jimage_rect r) { return jimage_rect_empty(r) ? 0u : (uint64_t)JSTATS_MAX_PARTIALS * JSTATS_PARTIAL_BYTES; }

// The plan of desc in an image_w x image_h image, or why there is none.
static inline const char* jstats_plan(const jh_stats_desc* d, uint32_t image_w, uint32_t image_h, jh_stats_plan_t* plan) {
    if (const char* why = jstats_desc_error(d)) return why;
    jimage_rect r;
    if (const char* why = jstats_rect_error(d, image_w, image_h, &r)) return why;
    plan->x = r.x; plan->y = r.y; plan->width = r.w; plan->height = r.h;
    plan->launches = jimage_rect_empty(r) ? 1u : 2u;
    plan->reserved = 0u;
    plan->record_bytes = sizeof(jh_stats_record);
    plan->scratch_bytes = jstats_scratch_bytes(r);
    return nullptr;
}

// The batch query's body: codes[i] = the code of f16_bits[i] under `transfer` (a colour channel's); t: the 255 thresholds.
static inline const char* jstats_codes(int transfer, uint64_t n, const uint16_t* f16_bits, uint8_t* codes, const float* t) {
    if (transfer != JSTATS_LINEAR && transfer != JSTATS_SRGB) return "unknown transfer";
    for (uint64_t i = 0; i < n; i++) codes[i] = (uint8_t)jstats_code(transfer, 0u, f16_bits[i], t);
    return nullptr;
}
