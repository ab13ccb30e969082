// kernels_color.hip -- jh_color_filter: a colour matrix and per-channel transfer functions on an RGBA16F image, the device half of the
// rule in include/jello_hip.h ("Colour filter") and DESIGN.md 5.10; the tables come from the host (include/jello_color.h).  Per texel
// of the rectangle, binary32:
//   input    t_c = PRE_c[h_c] for the colour channels where a PRE table is given, else the f16 widened; alpha always widened
//   matrix   m = M[i][4], then m = fmaf(M[i][k], t_k, m) for k = 0, 1, 2, 3 -- the order include/jello_hip.h states, four fmaf and
//            nothing else
//   clamp    m = m > 0 ? m : 0; m = m < 1 ? m : 1 (with the flag; compare and select: NaN and -0 become +0)
//   round    g = f16(m), a NaN as 0x7e00
//   output   POST_i[g] where a POST table is given, else g
// Streaming: 8 B in and 8 B out per texel, nothing reused, no LDS: the pair walk of texel_io.h without a backdrop, a lane two
// neighbouring texels of a dst row, 16-byte accesses where a pair allows.  A work item is a row segment of 512 texels = one workgroup
// of 256 lanes; the grid is bounded by 8 x the CU count and strides.  src may be dst.
// The matrix, the clamp flag and the table pointers are kernel arguments: they sit in scalar registers, and an absent table is a
// branch on the scalar pipe.  Two instantiations: TABLES = false has no gather (LINEAR space, IDENTITY funcs: feColorMatrix,
// luminanceToAlpha, a tint); TABLES = true gathers up to 3 x 4 B and 4 x 2 B per texel from tables of 1.25 MB in all.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kColorThreads = 256;
constexpr uint32_t kColorEntries = 65536u;  // of a table: one per f16 bit pattern

struct ColorParams {  // by value in the kernel arguments
    float m[20];      // row-major 4 x 5
    uint32_t clamp;
    const float* pre;         // PRE_c at pre + c * kColorEntries, or null
    const uint16_t* post[4];  // POST_i, or null
};

template <bool TABLES>
JD uint2 color_texel(uint2 s, const ColorParams& p) {
    const uint32_t h[4] = {s.x & 0xffffu, s.x >> 16, s.y & 0xffffu, s.y >> 16};
    float t[4];
    t[3] = jd::f16_to_f32((uint16_t)h[3]);
    if (TABLES && p.pre) {
        for (int c = 0; c < 3; c++) t[c] = p.pre[(uint32_t)c * kColorEntries + h[c]];
    } else {
        for (int c = 0; c < 3; c++) t[c] = jd::f16_to_f32((uint16_t)h[c]);
    }
    uint32_t g[4];
    for (int i = 0; i < 4; i++) {
        float m = p.m[5 * i + 4];
        for (int k = 0; k < 4; k++) m = __builtin_fmaf(p.m[5 * i + k], t[k], m);
        if (p.clamp) {
            m = m > 0.0f ? m : 0.0f;
            m = m < 1.0f ? m : 1.0f;
        }
        g[i] = m != m ? 0x7e00u : (uint32_t)jd::f32_to_f16(m);
        if (TABLES && p.post[i]) g[i] = p.post[i][g[i]];
    }
    return make_uint2(g[0] | (g[1] << 16), g[2] | (g[3] << 16));
}

// The w x h texels at (x, y) of src (src_w texels per row; null: transparent black) into the same rectangle of dst (dst_w per row).
// item = row * segs + seg.
template <bool TABLES>
__global__ __launch_bounds__(kColorThreads) void k_color(const uint2* src, uint32_t src_w, uint2* dst, uint32_t dst_w, uint32_t x, uint32_t y,
                                                         uint32_t w, uint32_t segs, uint32_t total_items, ColorParams p) {
    pair_walk<kColorThreads, false>(src, src_w, x, y, dst, dst_w, x, y, w, 0u, segs, total_items, [&](uint2 s, uint2) { return color_texel<TABLES>(s, p); });
}

}  // namespace

// The rule on the rectangle r of the RGBA16F image src (null texels: transparent black; may be dst), written to the same rectangle
// of the image dst.  matrix: 20 floats, row-major 4 x 5; clamp: JH_COLOR_CLAMP's bit;
// pre: the three PRE tables of 65 536 floats one after the other, or null; post[i]: POST_i, 65 536 entries, or null.  One launch on
// `stream`, none for an empty rectangle.  Returns 0, -1 on arguments it refuses, -2 on a launch error.
extern "C" int jh_color_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect r, const float* matrix, int clamp, const float* pre,
                               const uint16_t* const* post, int num_cus) {
    if (!dst.texels || !matrix || !post) return -1;
    if (!jimage_rect_inside(r, src.width, src.height) || !jimage_rect_inside(r, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(r)) return 0;
    const uint64_t segs = walk_segs(r.w, kColorThreads), total = segs * r.h;
    if (total > 0x7fffffffull) return -1;
    ColorParams p;
    for (int i = 0; i < 20; i++) p.m[i] = matrix[i];
    p.clamp = clamp ? 1u : 0u;
    p.pre = pre;
    bool tables = pre != nullptr;
    for (int i = 0; i < 4; i++) {
        p.post[i] = post[i];
        tables = tables || post[i] != nullptr;
    }
    const dim3 grid(grid_blocks(total, 1u, 8u, num_cus)), block(kColorThreads);
    with_flag(tables, [&](auto tab) {
        hipLaunchKernelGGL(k_color<decltype(tab)::value>, grid, block, 0, stream, (const uint2*)src.texels, src.width, (uint2*)dst.texels, dst.width, r.x, r.y, r.w, (uint32_t)segs,
                           (uint32_t)total, p);
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
