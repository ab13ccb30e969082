// kernels_composite.hip -- jh_composite: one RGBA16F image blended onto another, the device half of the rule in include/jello_hip.h
// ("Composite") and DESIGN.md 5.8; the geometry comes from the host (include/jello_composite.h).  Per texel of the placed rectangle,
// every operation binary32 and rounded once:
//   source     (c_s, a_s) = the f16 texel; with the tint flag c_s = tint.rgb and a_s = a_s * tint.a; a_s = a_s * opacity; p_s = c_s * a_s
//   backdrop   (c_b, a_b) = the dst texel (never written: transparent black); p_b = c_b * a_b
//   blend      R = blend_rule((p_b, a_b), (p_s, a_s), mix << 8 | compose)      -- blend_rule.h, the text the fine kernel compiles
//   store      R by the store rule (texel_io.h): un-premultiplied as fine stores; a binary32 -0 leaves as +0
// Streaming: 8 B of source and 8 B of backdrop in, 8 B out per texel, nothing reused, no LDS: the pair walk of texel_io.h, a lane two
// neighbouring texels of a dst row, 16-byte accesses where a pair allows.  A work item is a row segment of 512 texels = one workgroup
// of 256 lanes; the grid is bounded by 8 x the CU count and strides.
// Mode, flags, opacity and tint are kernel arguments: they sit in scalar registers, and the switches of blend_rule are branches on the
// scalar pipe.  Two instantiations: FAST is Normal + SrcOver (the first arm of blend_rule alone: the shadow / overlay case), the other
// carries all sixteen mix modes and fourteen operators.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_composite.h"
#include "blend_rule.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kCompThreads = 256;

struct CompositeParams {  // by value in the kernel arguments
    uint32_t mode;        // mix << 8 | compose
    uint32_t tint_on;
    float opacity;
    float tint[4];
};

JD V4 comp_f32(uint2 t) {
    const float4 c = jd::rgba16f_to_f32(t);
    return v4(c.x, c.y, c.z, c.w);
}

template <bool FAST>
JD uint2 composite_texel(uint2 s, uint2 b, const CompositeParams& p) {
    V4 cs = comp_f32(s);
    const V4 cb = comp_f32(b);
    if (p.tint_on) cs = v4(p.tint[0], p.tint[1], p.tint[2], cs.w * p.tint[3]);
    const float as = cs.w * p.opacity;
    const V4 r = blend_rule(v4(cb.x * cb.w, cb.y * cb.w, cb.z * cb.w, cb.w), v4(cs.x * as, cs.y * as, cs.z * as, as), FAST ? 0u : p.mode);
    return texel_unpremultiply(make_float4(r.x, r.y, r.z, r.w));
}

// rect.w x rect.h texels: src (src_w texels per row; null: transparent black) from (rect.sx, rect.sy) onto dst (dst_w per row) at
// (rect.dx, rect.dy); has_backdrop = 0: dst's content is not read (transparent black).  item = row * segs + seg.
template <bool FAST>
__global__ __launch_bounds__(kCompThreads) void k_composite(const uint2* __restrict__ src, uint32_t src_w, uint2* dst, uint32_t dst_w,
                                                            uint32_t has_backdrop, jcomp_rect rect, uint32_t segs, uint32_t total_items,
                                                            CompositeParams p) {
    pair_walk<kCompThreads, true>(src, src_w, rect.sx, rect.sy, dst, dst_w, rect.dx, rect.dy, rect.w, has_backdrop, segs, total_items,
                                  [&](uint2 s, uint2 b) { return composite_texel<FAST>(s, b, p); });
}

}  // namespace

// The rectangle `rect` (jcomp_clip's result for these two images) of the RGBA16F image src (null texels: transparent black) blended
// onto the image dst; dst_has_content = 0: dst's memory is not read, the backdrop is transparent
// black.  mode = mix << 8 | compose (mix 0..15, compose 0..13); flags bit 0: the tint (four floats) is applied.  One launch on
// `stream`, none for an empty rectangle.  Returns 0, -1 on arguments it refuses, -2 on a launch error.
extern "C" int jh_composite_launch(hipStream_t stream, jimage_src src, jimage_dst dst, int dst_has_content, const jcomp_rect* rect, uint32_t mode,
                                   uint32_t flags, float opacity, const float* tint, int num_cus) {
    if (!dst.texels || !rect || !tint || (mode >> 8) > 15u || (mode & 0xffu) > 13u || (flags & ~1u) != 0u) return -1;
    const jcomp_rect r = *rect;
    if (!jimage_rect_inside({r.sx, r.sy, r.w, r.h}, src.width, src.height) || !jimage_rect_inside({r.dx, r.dy, r.w, r.h}, dst.width, dst.height)) return -1;
    if (r.w == 0u || r.h == 0u) return 0;
    const uint64_t segs = walk_segs(r.w, kCompThreads), total = segs * r.h;
    if (total > 0x7fffffffull) return -1;
    CompositeParams p;
    p.mode = mode;
    p.tint_on = flags & 1u;
    p.opacity = opacity;
    for (int i = 0; i < 4; i++) p.tint[i] = tint[i];
    const dim3 grid(grid_blocks(total, 1u, 8u, num_cus)), block(kCompThreads);
    with_flag(mode == 0u, [&](auto fast) {
        hipLaunchKernelGGL(k_composite<decltype(fast)::value>, grid, block, 0, stream, (const uint2*)src.texels, src.width, (uint2*)dst.texels, dst.width, dst_has_content ? 1u : 0u, r,
                           (uint32_t)segs, (uint32_t)total, p);
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
