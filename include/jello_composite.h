// jello_composite.h -- the host half of the composite rule (DESIGN.md 5.8 "Composite rule"): which source rectangle is legal and
// where a placed rectangle lands in dst.  Compiled by the library (jello_amd/csrc/jello_hip.cpp: jh_composite), by the host
// library's query (include/jello_queries.h: jq_composite_clip, which is jl_composite_clip), by tools/composite_clip_check.cpp, and by nothing else;
// tests/composite_ref.py restates it.  The device half -- the blend of the texels -- is jello_amd/csrc/kernels_composite.hip.
//
//   source rectangle   (sx, sy, sw, sh) inside the src_w x src_h image; sw == sh == 0: the whole image (sx, sy ignored);
//                      empty in exactly one dimension, or not inside the image: refused
//   placement          its top-left lands at the signed (dx, dy) of the dst_w x dst_h destination and is clipped to it
//   result             the part that is written: (sx', sy') in src, (dx', dy') in dst, w x h texels; w == h == 0 when nothing is left
// Every sum is formed in 64 bits, so int32 offsets and uint32 sizes at their limits neither wrap nor overflow.
#pragma once
#include <stdint.h>
#include "jello_image.h"

typedef struct jcomp_rect {
    uint32_t sx, sy;  // first texel read in src
    uint32_t dx, dy;  // first texel written in dst
    uint32_t w, h;    // texels per row, rows (both 0: nothing to write)
} jcomp_rect;

// One axis: n source texels from s on, the first placed at d of a destination of `size`.  Returns the count left; *s_out, *d_out
// are the first texel read and written (0 when nothing is left).
static inline uint32_t jcomp_clip_axis(uint32_t s, uint32_t n, int32_t d, uint32_t size, uint32_t* s_out, uint32_t* d_out) {
    const int64_t lo = d < 0 ? 0 : (int64_t)d;
    const int64_t end = (int64_t)d + (int64_t)n;  // |d| <= 2^31, n < 2^32
    const int64_t hi = end < (int64_t)size ? end : (int64_t)size;
    if (hi <= lo) {
        *s_out = 0u;
        *d_out = 0u;
        return 0u;
    }
    *s_out = (uint32_t)((int64_t)s + (lo - (int64_t)d));  // < s + n <= the source's size
    *d_out = (uint32_t)lo;
    return (uint32_t)(hi - lo);
}

// 0: *out is the clipped placement (possibly empty); -1: the source rectangle is refused (*out untouched).
static inline int jcomp_clip(uint32_t src_w, uint32_t src_h, uint32_t sx, uint32_t sy, uint32_t sw, uint32_t sh, int32_t dx, int32_t dy,
                             uint32_t dst_w, uint32_t dst_h, jcomp_rect* out) {
    if (jimage_rect_check({sx, sy, sw, sh}, src_w, src_h) != JIMAGE_RECT_OK) return -1;
    const jimage_rect s = jimage_resolve({sx, sy, sw, sh}, src_w, src_h);  // (the whole image may have no texels)
    jcomp_rect r;
    r.w = jcomp_clip_axis(s.x, s.w, dx, dst_w, &r.sx, &r.dx);
    r.h = jcomp_clip_axis(s.y, s.h, dy, dst_h, &r.sy, &r.dy);
    if (r.w == 0u || r.h == 0u) r.sx = r.sy = r.dx = r.dy = r.w = r.h = 0u;
    *out = r;
    return 0;
}
