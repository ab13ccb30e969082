// kernels_perspective.hip -- jh_perspective: a rectangle of one RGBA16F image into a rectangle of another under a projective
// transform; the device half of the rule in include/jello_hip.h ("Perspective") and DESIGN.md 5.19.  The plan (nine doubles, host
// only) and the source position are include/jello_perspective.h's, compiled here too; everything after the position is jh_warp's text
// (warp_taps.h).  Per destination texel (X, Y) of the image
//   (U, V) = jpersp_position(G, X, Y), or the texel is void: den <= 0 (behind the viewer, or on the horizon) or a NaN position
//   axis_taps of U and of V, and the texel tap_sum stores for them; a void texel stores four +0.0 and loads nothing
// One launch, no LDS, no tables, no scratch: k_warp's shape.  A wave's item is a tile of the destination, 16 texels x 4 rows, laid on
// the 128-byte lines of the destination image (`phase`), four waves to a workgroup's 16 x 16, the workgroups striding over the tiles;
// a lane owns one texel.  The nine doubles travel in the kernel arguments (scalar registers); the position is 14 binary64 products and
// sums and one IEEE division per texel, on the vector unit at the binary64 rate.  24 instantiations, filter x edge x straight.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_perspective.h"
#include "kcommon.h"
#include "texel_io.h"
#include "warp_taps.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTile = 16;  // a workgroup's tile: 16 x 16, a wave's: 16 x 4

struct PerspectiveArgs {
    const uint2* src;  // the source rectangle's first texel (null: never written, transparent black)
    uint2* dst;        // the destination image
    double G[9];       // the plan
    uint32_t src_w, sw, sh;          // texels per row of the source image; the source rectangle's extents
    uint32_t dst_w, dx, dy, dw, dh;  // texels per row of the destination image; the destination rectangle
    uint32_t tiles_x, total;
};

template <int FILTER, int EDGE, bool STRAIGHT>
__global__ __launch_bounds__(kThreads) void k_perspective(const PerspectiveArgs a) {
    constexpr int N = Taps<FILTER>::N;
    const uint32_t tx = threadIdx.x & (kTile - 1u), ty = threadIdx.x >> 4;
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t trow = it / a.tiles_x, tcol = it - trow * a.tiles_x;
        const uint32_t row = trow * kTile + ty;
        if (row >= a.dh) continue;
        uint2* drow = a.dst + ((uint64_t)(a.dy + row) * a.dst_w + a.dx);  // the row's first texel
        const uint32_t phase = (uint32_t)(((uintptr_t)drow >> 3) & (kTile - 1u));  // texels from the 128-byte line to the row's first texel
        const int64_t c = (int64_t)tcol * kTile + tx - phase;  // the lane's texel of the rectangle's row
        if (c < 0 || c >= (int64_t)a.dw) continue;
        int64_t U, V;
        uint2 out = make_uint2(0u, 0u);  // (a void texel: four +0.0)
        if (jpersp_position(a.G, a.dx + (uint32_t)c, a.dy + row, &U, &V)) {
            float wx[N], wy[N];
            int32_t ix[N], iy[N];
            bool lx[N], ly[N];
            axis_taps<FILTER, EDGE>(U, (int32_t)a.sw, wx, ix, lx);
            axis_taps<FILTER, EDGE>(V, (int32_t)a.sh, wy, iy, ly);
            out = tap_sum<FILTER, EDGE, STRAIGHT>(a.src, a.src_w, wx, ix, lx, wy, iy, ly);
        }
        drow[c] = out;
    }
}

template <int FILTER, int EDGE>
void launch_edge(hipStream_t stream, dim3 grid, bool straight, const PerspectiveArgs& a) {
    with_flag(straight, [&](auto flag) {
        constexpr bool STRAIGHT = decltype(flag)::value;
        hipLaunchKernelGGL((k_perspective<FILTER, EDGE, STRAIGHT>), grid, dim3(kThreads), 0, stream, a);
    });
}
template <int FILTER>
void launch_filter(hipStream_t stream, dim3 grid, int edge, bool straight, const PerspectiveArgs& a) {
    switch (edge) {
        case JWARP_EDGE_ZERO: launch_edge<FILTER, JWARP_EDGE_ZERO>(stream, grid, straight, a); break;
        case JWARP_EDGE_CLAMP: launch_edge<FILTER, JWARP_EDGE_CLAMP>(stream, grid, straight, a); break;
        case JWARP_EDGE_REPEAT: launch_edge<FILTER, JWARP_EDGE_REPEAT>(stream, grid, straight, a); break;
        default: launch_edge<FILTER, JWARP_EDGE_MIRROR>(stream, grid, straight, a); break;
    }
}

}  // namespace

// The rectangle d of the RGBA16F image dst = the rectangle s of the image src (null texels: transparent black; another image than
// dst) under the plan (G[9] of include/jello_perspective.h, host memory, read during the call).  One launch on `stream`: one of the
// 24 instantiations of k_perspective, filter x edge x straight.  Returns 0, -1 on arguments it refuses (a plan outside a legal one's
// range among them: an entry that is not finite or above 1 in magnitude), -2 on a launch error.
extern "C" int jh_perspective_launch(hipStream_t stream, jimage_src src, jimage_rect s, jimage_dst dst, jimage_rect d, const double* plan, int filter, int edge,
                                     int straight, int num_cus) {
    if (!dst.texels || !plan || src.texels == dst.texels) return -1;
    if (jpersp_desc_error(filter, edge, 0u, src.width, src.height, dst.width, dst.height)) return -1;
    if (!jimage_rect_inside(s, src.width, src.height) || !jimage_rect_inside(d, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(s) || jimage_rect_empty(d)) return -1;
    for (int i = 0; i < 9; i++)
        if (!(plan[i] >= -1.0 && plan[i] <= 1.0)) return -1;
    PerspectiveArgs a;
    a.src = src.texels ? (const uint2*)src.texels + ((uint64_t)s.y * src.width + s.x) : nullptr;
    a.dst = (uint2*)dst.texels;
    for (int i = 0; i < 9; i++) a.G[i] = plan[i];
    a.src_w = src.width; a.sw = s.w; a.sh = s.h;
    a.dst_w = dst.width; a.dx = d.x; a.dy = d.y; a.dw = d.w; a.dh = d.h;
    a.tiles_x = (d.w + 2u * (kTile - 1u)) / kTile;  // (+ 15: the grid of lines may start up to 15 texels before the row)
    a.total = a.tiles_x * ((d.h + kTile - 1u) / kTile);
    const dim3 grid(grid_blocks((uint64_t)a.total * kWaves, kWaves, 8u, num_cus));
    switch (filter) {
        case JWARP_NEAREST: launch_filter<JWARP_NEAREST>(stream, grid, edge, straight != 0, a); break;
        case JWARP_BILINEAR: launch_filter<JWARP_BILINEAR>(stream, grid, edge, straight != 0, a); break;
        default: launch_filter<JWARP_BICUBIC>(stream, grid, edge, straight != 0, a); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
