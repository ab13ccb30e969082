// jello_image.h -- the geometry every image call shares (DESIGN.md 5.8 "What is shared"): the rectangle a descriptor names and what can
// be wrong with it, the image views the launchers take, and the rows of an image a pass with a vertical radius reads.  Host code only,
// compiled by the library and the launchers (jello_amd/csrc: jello_hip.cpp, kernels_*.hip through kcommon.h), by the rule headers that
// name a rectangle (jello_blur.h, jello_composite.h, jello_resample.h) and by tools/image_rect_check.cpp and tools/morph_check.cpp.
//   rectangle   (x, y, w, h) of a width x height image; w == h == 0: the whole image (x, y ignored), which may have no texels
//   refused     empty in exactly one dimension; not inside the image (the sums in 64 bits: x + w at the limits does not wrap)
#pragma once
#include <stdint.h>

struct jimage_rect { uint32_t x, y, w, h; };

// The rectangle a descriptor names in a width x height image: its own, or the whole image for 0 x 0.
static inline jimage_rect jimage_resolve(jimage_rect r, uint32_t width, uint32_t height) {
    if (r.w == 0u && r.h == 0u) { r.x = 0u; r.y = 0u; r.w = width; r.h = height; }
    return r;
}
static inline bool jimage_rect_empty(jimage_rect r) { return r.w == 0u || r.h == 0u; }
// Whether the texels of a resolved rectangle are texels of the image.
static inline bool jimage_rect_inside(jimage_rect r, uint32_t width, uint32_t height) { return (uint64_t)r.x + r.w <= width && (uint64_t)r.y + r.h <= height; }

// What is wrong with the rectangle a descriptor names (not yet resolved) against a width x height image.
enum { JIMAGE_RECT_OK = 0, JIMAGE_RECT_HALF_EMPTY = 1, JIMAGE_RECT_OUTSIDE = 2 };
static inline int jimage_rect_check(jimage_rect named, uint32_t width, uint32_t height) {
    if ((named.w == 0u) != (named.h == 0u)) return JIMAGE_RECT_HALF_EMPTY;
    return jimage_rect_inside(jimage_resolve(named, width, height), width, height) ? JIMAGE_RECT_OK : JIMAGE_RECT_OUTSIDE;
}

// An image as a launcher takes it: row-major RGBA16F texels, `width` to a row.  Two types, so that a call site cannot swap them.
struct jimage_src { const void* texels; uint32_t width, height; };  // texels == nullptr: never written, reads as transparent black
struct jimage_dst { void* texels; uint32_t width, height; };

// The rows of an image of `height` rows within radius_y of the rows [y, y + rect_h): what a row pass prepares for its column pass.
struct jimage_rows { uint32_t row0, n_rows; };
static inline jimage_rows jimage_row_window(uint32_t y, uint32_t rect_h, uint32_t radius_y, uint32_t height) {
    const uint32_t row0 = y > radius_y ? y - radius_y : 0u;
    const uint64_t row1 = (uint64_t)y + rect_h + radius_y < height ? (uint64_t)y + rect_h + radius_y : height;
    return {row0, (uint32_t)(row1 - row0)};
}
