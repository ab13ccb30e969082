// kernels_shadow.hip -- jh_shadow: the Gaussian blur of a rounded rectangle GENERATED into an RGBA16F image or laid over it, the device
// half of the rule in include/jello_hip.h ("Shadow") and DESIGN.md 5.18; the host half -- the legal descriptor, the plan, the bounds --
// and every function with cases (the position as binary32, the erf approximant G, the band term, the cap sum) are
// include/jello_shadow.h, the one text the library, the stand-alone check and this file compile.  There is no source image and no
// table: per destination texel two int64 positions, four G for the straight bands and, where a cap's window reaches the texel's row,
// 3 N + 1 more per cap (N = 4, 8 or 16); G is 5 fmaf, 13 other operations and one IEEE division.  The only memory traffic is the 8-byte
// store, and under OVER the 8-byte load before it.
// One launch.  A workgroup of 256 lanes owns a TILE of the destination, 64 texels x 16 rows, laid on the destination image's 128-byte
// lines as kernels_turbulence.hip lays its tiles, and walks its tiles by grid stride.  A wave owns 4 rows of the tile and a lane a
// vertical strip of them, 4 outputs of one column.  Under an axis-aligned matrix (plan m1 == m3 == 0, a scalar) x and B(x, a) are the
// strip's, computed once for its four texels.  Whether a cap is live is a branch per texel: a wave whose 64 x 4 texels see no cap
// window (every lane's hi <= lo) skips the loop and runs the exact band only.  Under OVER the strip's four backdrop texels are loaded
// before the arithmetic.
// k_shadow<ROUND, OVER>: r > 0 or r = 0 (the product of two bands, no cap code), STORE or OVER; INVERT, N and the axis flag are
// scalars.  4 instantiations; VGPRs, scratch and spills: DESIGN.md 5.18.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_shadow.h"
#include "blend_rule.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTileW = 64, kTileH = 16, kStrip = kTileH / kWaves;  // a lane's strip: 4 rows of one column
constexpr uint32_t kLine = 16;                                                                      // texels of a 128-byte line
constexpr uint32_t kPerCu = 8;                                                                      // workgroups to a CU

struct ShadowArgs {
    uint2* dst;               // the destination image
    uint32_t width;           // its texels per row
    uint32_t dx, dy, dw, dh;  // the rectangle that is written
    uint32_t tiles_x, total;
    uint32_t invert, has_backdrop, axis;  // INVERT; dst holds content (OVER reads it); m1 == m3 == 0
    int64_t m[6], centre[2];              // the plan's positions
    jshadow_scalars k;
    float color[4];
};

// The texel OVER leaves: `s`, what STORE would have written, as the source of jh_composite's rule (Normal + SrcOver, opacity 1, no
// tint: kernels_composite.hip's composite_texel<true>) onto the backdrop texel b.
JD uint2 shadow_over(uint2 s, uint2 b) {
    const float4 cs = jd::rgba16f_to_f32(s), cb = jd::rgba16f_to_f32(b);
    const V4 r = blend_rule(v4(cb.x * cb.w, cb.y * cb.w, cb.z * cb.w, cb.w), v4(cs.x * cs.w, cs.y * cs.w, cs.z * cs.w, cs.w), 0u);
    return texel_unpremultiply(make_float4(r.x, r.y, r.z, r.w));
}

template <bool ROUND, bool OVER>
__global__ __launch_bounds__(kThreads) void k_shadow(const ShadowArgs a) {
    const uint32_t lane = threadIdx.x & (kTileW - 1u), wave = threadIdx.x >> 6;
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t trow = it / a.tiles_x, tcol = it - trow * a.tiles_x;
        const uint32_t row0 = trow * kTileH;  // the tile's first row of the rectangle
        const uint32_t phase = (uint32_t)((((uintptr_t)a.dst >> 3) + (uint64_t)(a.dy + row0) * a.width + a.dx) & (kLine - 1u));
        const int32_t col0 = (int32_t)(tcol * kTileW) - (int32_t)phase;  // the tile's first column of the rectangle (may lie before it)
        const uint32_t r0 = row0 + wave * kStrip;                        // the strip's first row of the rectangle
        const int32_t c = col0 + (int32_t)lane;                          // the lane's column of the rectangle
        if (r0 >= a.dh || c < 0 || c >= (int32_t)a.dw) continue;
        const uint32_t X = a.dx + (uint32_t)c;
        uint2* out = a.dst + ((uint64_t)(a.dy + r0) * a.width + X);
        uint2 back[kStrip];
#pragma unroll
        for (uint32_t j = 0; j < kStrip; j++) {
            back[j] = make_uint2(0u, 0u);
            if (OVER && a.has_backdrop && r0 + j < a.dh) back[j] = out[(uint64_t)j * a.width];
        }
        float xs = 0.0f, bxs = 0.0f;  // under an axis-aligned matrix: the strip's x and B(x, a)
        if (a.axis) {
            xs = jshadow_position(a.m[0], a.m[1], a.m[2], a.centre[0], X, 0u);
            bxs = jshadow_band(xs, a.k.a, a.k.inv_s);
        }
#pragma unroll
        for (uint32_t j = 0; j < kStrip; j++) {
            if (r0 + j >= a.dh) break;
            const uint32_t Y = a.dy + r0 + j;
            float x = xs, bx = bxs;
            if (!a.axis) {
                x = jshadow_position(a.m[0], a.m[1], a.m[2], a.centre[0], X, Y);
                bx = jshadow_band(x, a.k.a, a.k.inv_s);
            }
            const float y = jshadow_position(a.m[3], a.m[4], a.m[5], a.centre[1], X, Y);
            const float s = jshadow_finish<ROUND>(a.k, jshadow_band(y, a.k.straight, a.k.inv_s) * bx, x, y);
            float p[4];
            jshadow_premultiplied(a.color, s, a.invert != 0u, p);
            uint2 t = texel_unpremultiply(make_float4(p[0], p[1], p[2], p[3]));
            if (OVER) t = shadow_over(t, back[j]);
            out[(uint64_t)j * a.width] = t;
        }
    }
}

}  // namespace

// The rectangle r of the RGBA16F image dst = the shadow of the rule: the plan of the descriptor, its colour and its flags (JSHADOW_OVER,
// JSHADOW_INVERT); dst_has_content = 0: under OVER dst's memory is not read, the backdrop is transparent black.  One launch on
// `stream`, no LDS.  Returns 0, -1 on arguments it refuses, -2 on a launch error.
extern "C" int jh_shadow_launch(hipStream_t stream, jimage_dst dst, int dst_has_content, jimage_rect r, const jh_shad_plan* plan, const float* color,
                                uint32_t flags, int num_cus) {
    if (!dst.texels || !plan || !color || (flags & ~(JSHADOW_OVER | JSHADOW_INVERT)) != 0u) return -1;
    if (plan->n != 4u && plan->n != 8u && plan->n != 16u) return -1;
    if (dst.width > JSHADOW_MAX_EXTENT || dst.height > JSHADOW_MAX_EXTENT) return -1;
    if (!jimage_rect_inside(r, dst.width, dst.height) || jimage_rect_empty(r)) return -1;
    const uint64_t tiles_x = ((uint64_t)r.w + (kLine - 1u) + (kTileW - 1u)) / kTileW;  // (+ 15: the grid of lines may start up to 15 texels before the row)
    const uint64_t total = tiles_x * (((uint64_t)r.h + kTileH - 1u) / kTileH);
    if (total > 0x7fffffffu) return -1;
    ShadowArgs a;
    a.dst = (uint2*)dst.texels;
    a.width = dst.width;
    a.dx = r.x; a.dy = r.y; a.dw = r.w; a.dh = r.h;
    a.tiles_x = (uint32_t)tiles_x;
    a.total = (uint32_t)total;
    a.invert = (flags & JSHADOW_INVERT) ? 1u : 0u;
    a.has_backdrop = dst_has_content ? 1u : 0u;
    a.axis = (plan->m[1] == 0 && plan->m[3] == 0) ? 1u : 0u;
    for (uint32_t i = 0; i < 6u; i++) a.m[i] = plan->m[i];
    a.centre[0] = plan->centre[0]; a.centre[1] = plan->centre[1];
    a.k = jshadow_scalars_of(plan);
    for (uint32_t i = 0; i < 4u; i++) a.color[i] = color[i];
    const dim3 grid(grid_blocks(total * kWaves, kWaves, kPerCu, num_cus));
    with_flag(plan->radius > 0.0f, [&](auto round) {
        with_flag((flags & JSHADOW_OVER) != 0u, [&](auto over) {
            hipLaunchKernelGGL((k_shadow<decltype(round)::value, decltype(over)::value>), grid, dim3(kThreads), 0, stream, a);
        });
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
