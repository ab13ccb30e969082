// kernels_composite.hip -- jh_composite: one RGBA16F image blended onto another, the device half of the rule in include/jello_hip.h
// ("Composite") and DESIGN.md 5.8; the geometry comes from the host (include/jello_composite.h).  Per texel of the placed rectangle,
// every operation binary32 and rounded once:
//   source     (c_s, a_s) = the f16 texel; with the tint flag c_s = tint.rgb and a_s = a_s * tint.a; a_s = a_s * opacity; p_s = c_s * a_s
//   backdrop   (c_b, a_b) = the dst texel (never written: transparent black); p_b = c_b * a_b
//   blend      R = blend_rule((p_b, a_b), (p_s, a_s), mix << 8 | compose)      -- blend_rule.h, the text the fine kernel compiles
//   store      a_inv = 1 / max(R.a, 1e-6); dst = f16(R.rgb * a_inv + 0.0f), f16(R.a + 0.0f)   -- as fine stores; a binary32 -0 leaves as +0
// Streaming: 8 B of source and 8 B of backdrop in, 8 B out per texel, nothing reused, no LDS.  A lane owns two neighbouring texels
// of a dst row.  The pairs are laid on the row's 16-byte grid (`phase`: whether the rectangle's first texel of this row sits in the
// upper half of a 16-byte unit -- with an odd dst width that alternates from row to row), so a pair that lies inside the rectangle is
// one 16-byte load and one 16-byte store of dst, and a row's first or last texel alone an 8-byte one.  The source pair is one 16-byte
// load when its own address is aligned too (the parity of sx - dx and of the source width decide, per row), two 8-byte loads otherwise.
// A work item is a row segment of 512 texels = one workgroup of 256 lanes; the grid is bounded by 8 x the CU count and strides.
// Mode, flags, opacity and tint are kernel arguments: they sit in scalar registers, and the switches of blend_rule are branches on the
// scalar pipe.  Two instantiations: FAST is Normal + SrcOver (the first arm of blend_rule alone: the shadow / overlay case), the other
// carries all sixteen mix modes and fourteen operators.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_composite.h"
#include "blend_rule.h"
#include "blit_convert.h"
#include "kcommon.h"

namespace {

constexpr uint32_t kCompThreads = 256, kCompSeg = 2u * kCompThreads;  // texels of a work item

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
    const float a_inv = 1.0f / jd::fmax_(r.w, 1e-6f);
    const uint32_t ro = jd::f32_to_f16(r.x * a_inv + 0.0f), go = jd::f32_to_f16(r.y * a_inv + 0.0f), bo = jd::f32_to_f16(r.z * a_inv + 0.0f),
                   ao = jd::f32_to_f16(r.w + 0.0f);
    return make_uint2(ro | (go << 16), bo | (ao << 16));
}

// rect.w x rect.h texels: src (src_w texels per row; null: transparent black) from (rect.sx, rect.sy) onto dst (dst_w per row) at
// (rect.dx, rect.dy); has_backdrop = 0: dst's content is not read (transparent black).  item = row * segs + seg.
template <bool FAST>
__global__ __launch_bounds__(kCompThreads) void k_composite(const uint2* __restrict__ src, uint32_t src_w, uint2* dst, uint32_t dst_w,
                                                            uint32_t has_backdrop, jcomp_rect rect, uint32_t segs, uint32_t total_items,
                                                            CompositeParams p) {
    for (uint32_t it = blockIdx.x; it < total_items; it += gridDim.x) {
        const uint32_t row = it / segs, seg = it - row * segs;
        uint2* drow = dst + ((uint64_t)(rect.dy + row) * dst_w + rect.dx);
        const uint2* srow = src ? src + ((uint64_t)(rect.sy + row) * src_w + rect.sx) : nullptr;
        const uint32_t phase = (uint32_t)(((uintptr_t)drow >> 3) & 1u);
        const int64_t c = (int64_t)seg * kCompSeg + 2u * threadIdx.x - phase;  // the lane's texels c, c + 1 of the rectangle's row
        const bool va = c >= 0 && c < (int64_t)rect.w, vb = c + 1 < (int64_t)rect.w;
        if (!va && !vb) continue;
        uint2 sa = make_uint2(0u, 0u), sb = sa, ba = sa, bb = sa;
        if (va && vb) {
            if (has_backdrop) {
                const uint4 q = *(const uint4*)(drow + c);
                ba = make_uint2(q.x, q.y);
                bb = make_uint2(q.z, q.w);
            }
            if (srow) {
                const uint2* s = srow + c;
                if (((uintptr_t)s & 15u) == 0u) {  // (the same for every pair of the row)
                    const uint4 q = *(const uint4*)s;
                    sa = make_uint2(q.x, q.y);
                    sb = make_uint2(q.z, q.w);
                } else {
                    sa = s[0];
                    sb = s[1];
                }
            }
            const uint2 oa = composite_texel<FAST>(sa, ba, p), ob = composite_texel<FAST>(sb, bb, p);
            *(uint4*)(drow + c) = make_uint4(oa.x, oa.y, ob.x, ob.y);
        } else {  // the row's first or last texel alone
            const int64_t x = va ? c : c + 1;
            if (has_backdrop) ba = drow[x];
            if (srow) sa = srow[x];
            drow[x] = composite_texel<FAST>(sa, ba, p);
        }
    }
}

}  // namespace

// The rectangle `rect` (jcomp_clip's result for these two images) of the src_w x src_h RGBA16F image at src (null: transparent
// black) blended onto the dst_w x dst_h image at dst; dst_has_content = 0: dst's memory is not read, the backdrop is transparent
// black.  mode = mix << 8 | compose (mix 0..15, compose 0..13); flags bit 0: the tint (four floats) is applied.  One launch on
// `stream`, none for an empty rectangle.  Returns 0, -1 on arguments it refuses, -2 on a launch error.
extern "C" int jh_composite_launch(hipStream_t stream, const void* src, uint32_t src_w, uint32_t src_h, void* dst, uint32_t dst_w, uint32_t dst_h,
                                   int dst_has_content, const jcomp_rect* rect, uint32_t mode, uint32_t flags, float opacity, const float* tint,
                                   int num_cus) {
    if (!dst || !rect || !tint || (mode >> 8) > 15u || (mode & 0xffu) > 13u || (flags & ~1u) != 0u) return -1;
    const jcomp_rect r = *rect;
    if ((uint64_t)r.sx + r.w > src_w || (uint64_t)r.sy + r.h > src_h || (uint64_t)r.dx + r.w > dst_w || (uint64_t)r.dy + r.h > dst_h) return -1;
    if (r.w == 0u || r.h == 0u) return 0;
    const uint64_t segs = ((uint64_t)r.w + 1u + kCompSeg - 1u) / kCompSeg;  // (+ 1: the pair grid may start one texel before the row)
    const uint64_t total = segs * r.h;
    if (total > 0x7fffffffull) return -1;
    CompositeParams p;
    p.mode = mode;
    p.tint_on = flags & 1u;
    p.opacity = opacity;
    for (int i = 0; i < 4; i++) p.tint[i] = tint[i];
    const dim3 grid(blit_grid_blocks(total, num_cus)), block(kCompThreads);
    const uint2* s = (const uint2*)src;
    if (mode == 0u)
        hipLaunchKernelGGL(k_composite<true>, grid, block, 0, stream, s, src_w, (uint2*)dst, dst_w, dst_has_content ? 1u : 0u, r, (uint32_t)segs, (uint32_t)total, p);
    else
        hipLaunchKernelGGL(k_composite<false>, grid, block, 0, stream, s, src_w, (uint2*)dst, dst_w, dst_has_content ? 1u : 0u, r, (uint32_t)segs, (uint32_t)total, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
