// texel_io.h -- what the image kernels share besides their rules: how an RGBA16F texel is widened and stored, the streaming pair
// walk (kernels_composite.hip, kernels_color.hip) and the grid rule.  Tap loops, edge rules, LDS layouts and
// launch bounds stay in the kernel files.  Every function is internal to the file that includes it.
// The helpers' signatures are part of the generated code, and three loops stay written out for that reason ("What is
// shared"): the kernels' own __restrict__ parameters carry through the inlining, so the walk's pointer parameters have none (on src it
// costs k_composite two VGPRs); the 16-byte-or-two-8-byte load of a source pair as a helper of its own moves the register counts of
// k_composite and k_color; the pair store of the column passes (kernels_blur.hip, kernels_resample.hip) and the row staging loop
// (kernels_blur.hip, kernels_morph.hip) as helpers changed the instructions of k_blur_cols and k_morph_rows and measured slower on
// one configuration each.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "dmath.h"

namespace {

// ---- texel values ----

// Four binary32 as an RGBA16F texel, exactly: round to nearest even, subnormals kept (the default float mode).
JD uint2 texel_pack(const float4& v) {
    return make_uint2((uint32_t)jd::f32_to_f16(v.x) | ((uint32_t)jd::f32_to_f16(v.y) << 16), (uint32_t)jd::f32_to_f16(v.z) | ((uint32_t)jd::f32_to_f16(v.w) << 16));
}
// THE STORE RULE ("Store", is its home; include/jello_hip.h states it per call): a premultiplied binary32 result
// (p.rgb, a) leaves as a_inv = 1 / max(a, 1e-6), then f16(p.rgb * a_inv + 0.0f), f16(a + 0.0f), every operation rounded once, the
// max IEEE maxNum.  It is the fine kernel's un-premultiplying store, and the + 0.0f makes a binary32 -0 leave as +0.
JD uint2 texel_unpremultiply(const float4& v) {
    const float a_inv = 1.0f / jd::fmax_(v.w, 1e-6f);
    const uint32_t ro = jd::f32_to_f16(v.x * a_inv + 0.0f), go = jd::f32_to_f16(v.y * a_inv + 0.0f), bo = jd::f32_to_f16(v.z * a_inv + 0.0f),
                   ao = jd::f32_to_f16(v.w + 0.0f);
    return make_uint2(ro | (go << 16), bo | (ao << 16));
}
// What a call stores: its sums as they are under STRAIGHT, by the store rule otherwise.
template <bool STRAIGHT>
JD uint2 texel_store(const float4& v) { return STRAIGHT ? texel_pack(v) : texel_unpremultiply(v); }

// A source texel as the sums take it: widened, and its colour times its alpha unless STRAIGHT (exact: 11 + 11 bits; Inf x 0 is a NaN).
template <bool STRAIGHT>
JD float4 texel_widen(uint2 t) {
    const float4 c = jd::rgba16f_to_f32(t);
    return STRAIGHT ? c : make_float4(c.x * c.w, c.y * c.w, c.z * c.w, c.w);
}

JD void fma4(float4& a, float w, const float4& t) {
    a.x = __builtin_fmaf(w, t.x, a.x); a.y = __builtin_fmaf(w, t.y, a.y); a.z = __builtin_fmaf(w, t.z, a.z); a.w = __builtin_fmaf(w, t.w, a.w);
}

// ---- the streaming pair walk ----

// Row `row` (w texels) of a rectangle: of src (src_w texels per row; null: transparent black) from (sx, sy), into dst (dst_w per row)
// at (dx, dy), dst = texel(source texel, backdrop texel).  The backdrop is dst's texel under BACKDROP where has_backdrop is set,
// transparent black otherwise.  A work item is a row segment of 2 * THREADS texels, one workgroup of THREADS lanes, item = row * segs
// + seg, segs = ceil((w + 1) / (2 * THREADS)) (walk_segs), and the workgroups stride over the items.  A lane owns two neighbouring
// texels.  The pairs are laid on the dst row's 16-byte grid (`phase`: whether the row's first texel sits in the upper half of a
// 16-byte unit -- with an odd dst width that alternates from row to row), so a pair inside the rectangle is one 16-byte load and store
// of dst, and one 16-byte load of the source when its own address is aligned too, two 8-byte loads otherwise (the parity of sx - dx
// and of the widths decide, per row); a row's first or last texel alone is an 8-byte access.  src may be dst where the rectangles
// coincide: a lane reads its texels before it writes them and no other lane touches them.
template <uint32_t THREADS, bool BACKDROP, class F>
JD void pair_walk(const uint2* src, uint32_t src_w, uint32_t sx, uint32_t sy, uint2* dst, uint32_t dst_w, uint32_t dx, uint32_t dy, uint32_t w,
                  uint32_t has_backdrop, uint32_t segs, uint32_t total_items, F texel) {
    for (uint32_t it = blockIdx.x; it < total_items; it += gridDim.x) {
        const uint32_t row = it / segs, seg = it - row * segs;
        uint2* drow = dst + ((uint64_t)(dy + row) * dst_w + dx);
        const uint2* srow = src ? src + ((uint64_t)(sy + row) * src_w + sx) : nullptr;
        const uint32_t phase = (uint32_t)(((uintptr_t)drow >> 3) & 1u);
        const int64_t c = (int64_t)seg * (2u * THREADS) + 2u * threadIdx.x - phase;  // the lane's texels c, c + 1 of the rectangle's row
        const bool va = c >= 0 && c < (int64_t)w, vb = c + 1 < (int64_t)w;
        if (!va && !vb) continue;
        uint2 sa = make_uint2(0u, 0u), sb = sa, ba = sa, bb = sa;
        if (va && vb) {
            if (BACKDROP && has_backdrop) {
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
            const uint2 oa = texel(sa, ba), ob = texel(sb, bb);
            *(uint4*)(drow + c) = make_uint4(oa.x, oa.y, ob.x, ob.y);
        } else {  // the row's first or last texel alone
            const int64_t x = va ? c : c + 1;
            if (BACKDROP && has_backdrop) ba = drow[x];
            if (srow) sa = srow[x];
            drow[x] = texel(sa, ba);
        }
    }
}
inline uint64_t walk_segs(uint32_t w, uint32_t threads) { return ((uint64_t)w + 1u + 2u * threads - 1u) / (2u * threads); }  // (+ 1: the pair grid may start one texel before the row)

// ---- host side: the grid rule (the rectangles, the views and the row window the launchers take: include/jello_image.h, through kcommon.h) ----

// Workgroups to launch for `items` wave items, `waves` of them to a workgroup: at most per_cu workgroups per CU (256 CUs when the
// count is unknown), the rest by grid stride.
inline uint32_t grid_blocks(uint64_t items, uint32_t waves, uint32_t per_cu, int num_cus) {
    const uint64_t blocks = (items + waves - 1u) / waves, cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * per_cu;
    return (uint32_t)(blocks < cap ? blocks : cap);
}

// f(std::true_type) or f(std::false_type): a generic lambda launches the instantiation of a run-time flag, written once.
template <class F>
inline void with_flag(bool flag, F&& f) {
    if (flag) f(std::true_type{}); else f(std::false_type{});
}

}  // namespace
