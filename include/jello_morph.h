// jello_morph.h -- the host half of the morphology rule (DESIGN.md 5.11 "Morphology rule"): which descriptor is legal (its
// rectangle apart: jello_image.h), the rows and bytes of the intermediate, and the order key with its inverse.  Compiled by the library
// (jello_amd/csrc/jello_hip.cpp: jh_morphology), by the kernels (jello_amd/csrc/kernels_morph.hip: the key and its inverse are the
// one text the device and the stand-alone check both compile) and by tools/morph_check.cpp; tests/morph_ref.py restates it.
//
//   operand   a binary32 value per channel (a widened f16, or the exact product of two)
//   order     IEEE 754 totalOrder on the non-NaN values: -Inf < ... < -0 < +0 < ... < +Inf; a NaN of either sign is sticky
//   key       k = bits ^ (((int32)bits >> 31) & 0x7fffffff), compared as a signed integer; a NaN maps to the extreme the operator
//             selects (DILATE: INT32_MAX, ERODE: INT32_MIN).  The other extreme is the operator's neutral element: no operand maps to
//             it, so "does not take part" (JH_MORPH_EDGE_CLAMP outside the image) is that key.
//   inverse   the same xor.  INT32_MAX gives 0x7fffffff and INT32_MIN gives 0xffffffff: NaNs, as the rule asks.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JMORPH_HD __host__ __device__ __forceinline__
#else
#define JMORPH_HD static inline
#endif

#define JMORPH_MAX_RADIUS 255u
#define JMORPH_ERODE 0
#define JMORPH_DILATE 1
#define JMORPH_EDGE_ZERO 0
#define JMORPH_EDGE_CLAMP 1
#define JMORPH_STRAIGHT 1u

// The key of a binary32 bit pattern under the operator (dilate != 0: DILATE).
JMORPH_HD int32_t jmorph_key(uint32_t bits, int dilate) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return dilate ? (int32_t)0x7fffffff : (int32_t)0x80000000u;
    return (int32_t)(bits ^ ((uint32_t)((int32_t)bits >> 31) & 0x7fffffffu));
}
// The bit pattern of a key (of a value: that value; of an extreme: a NaN).
JMORPH_HD uint32_t jmorph_unkey(int32_t key) { return (uint32_t)key ^ ((uint32_t)(key >> 31) & 0x7fffffffu); }
// The key that never wins: what a position that does not take part is staged as.
JMORPH_HD int32_t jmorph_neutral(int dilate) { return dilate ? (int32_t)0x80000000u : (int32_t)0x7fffffff; }
// What a position outside the image is staged as: ZERO: +0.0f, whose key is 0; CLAMP: the neutral key.
JMORPH_HD int32_t jmorph_pad(int dilate, int clamp) { return clamp ? jmorph_neutral(dilate) : 0; }

// nullptr for a legal descriptor (the rectangle apart: jimage_rect_check), else what is wrong with it (jh_morphology puts "jh_morphology: " in front).
static inline const char* jmorph_desc_error(int op, int edge, uint32_t flags, uint32_t radius_x, uint32_t radius_y) {
    if (op != JMORPH_ERODE && op != JMORPH_DILATE) return "unknown op";
    if (edge != JMORPH_EDGE_ZERO && edge != JMORPH_EDGE_CLAMP) return "unknown edge mode";
    if ((flags & ~JMORPH_STRAIGHT) != 0u) return "unknown flag bits";
    return radius_x > JMORPH_MAX_RADIUS || radius_y > JMORPH_MAX_RADIUS ? "a radius above 255" : nullptr;
}

// The intermediate: two planes of keys (16 bytes per texel), each rect_w texels wide and jmorph_plane_rows high.  Row v of a plane
// is image row rect_y - radius_y + v, whether that row exists or not: the rows a window can reach above and below the image are
// rows of the prefix plane like any other (they hold the padding), so every window of the column pass has 2 radius_y + 1 rows and
// the blocks of the prefix / suffix walk are aligned to the rectangle wherever it lies.
static inline uint64_t jmorph_plane_rows(uint32_t rect_h, uint32_t radius_y) { return (uint64_t)rect_h + 2u * (uint64_t)radius_y; }
static inline uint64_t jmorph_plane_bytes(uint32_t rect_w, uint32_t rect_h, uint32_t radius_y) { return jmorph_plane_rows(rect_h, radius_y) * rect_w * 16u; }
static inline uint64_t jmorph_scratch_bytes(uint32_t rect_w, uint32_t rect_h, uint32_t radius_y) { return 2u * jmorph_plane_bytes(rect_w, rect_h, radius_y); }
