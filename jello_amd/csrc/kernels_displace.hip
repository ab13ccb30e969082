// kernels_displace.hip -- jh_displace: feDisplacementMap, a rectangle of one RGBA16F image into a rectangle of another at positions
// that a third image, the map, moves texel by texel; the device half of the rule in include/jello_hip.h ("Displace") and DESIGN.md
// 5.17.  The host half -- what is legal and the offset one map value gives -- is include/jello_displace.h, compiled here too; the plan
// is jh_warp's (include/jello_warp.h), and everything after the position is jh_warp's text (warp_taps.h).  Per destination texel
// (X, Y) of the image
//   m = the map's texel (X, Y): the stored f16 of the x channel and of the y channel
//   U = P (2 X + 1) + Q (2 Y + 1) + R + jdisp_offset(scale_x, m_x),  V = S (2 X + 1) + T (2 Y + 1) + W + jdisp_offset(scale_y, m_y)
//   axis_taps of U and of V, and the texel tap_sum stores for them
// One launch, no LDS, no tables, no scratch: k_warp's shape.  A wave's item is a tile of the destination, 16 texels x 4 rows, laid on
// the 128-byte lines of the destination image (`phase`), four waves to a workgroup's 16 x 16, the workgroups striding over the tiles;
// a lane owns one texel.  The map has the destination's size, so a lane's map texel sits where its destination texel does: one
// coalesced 8-byte load per lane, a 128-byte line per tile row, issued before the plan's part of the position, which does not depend
// on it.  The channels are run-time scalars -- the 64-bit texel shifted by 16 x channel -- so there are k_warp's 24 instantiations,
// filter x edge x straight.  The map may be the destination: a lane reads its one map texel before it writes that texel, and no
// other lane touches it (the map pointer is not __restrict__, so the store stays behind the load).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_displace.h"
#include "kcommon.h"
#include "texel_io.h"
#include "warp_taps.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTile = 16;  // a workgroup's tile: 16 x 16, a wave's: 16 x 4
constexpr int64_t kMaxScale = (int64_t)1 << 37, kMaxOffset = (int64_t)1 << 54;  // 64 x 2^31, 2^22 x 2^32: what a legal plan stays inside

struct DisplaceArgs {
    const uint2* src;  // the source rectangle's first texel (null: never written, transparent black)
    const uint2* map;  // the map image, of the destination's size (null: never written, 0 in every channel); may be dst
    uint2* dst;        // the destination image
    int64_t P, Q, R, S, T, W;
    float scale_x, scale_y;
    uint32_t shift_x, shift_y;         // 16 x the channel: where its f16 sits in the 64-bit texel
    uint32_t src_w, sw, sh;            // texels per row of the source image; the source rectangle's extents
    uint32_t dst_w, dx, dy, dw, dh;    // texels per row of the destination image (and of the map); the destination rectangle
    uint32_t tiles_x, total;
};

template <int FILTER, int EDGE, bool STRAIGHT>
__global__ __launch_bounds__(kThreads) void k_displace(const DisplaceArgs a) {
    constexpr int N = Taps<FILTER>::N;
    const uint32_t tx = threadIdx.x & (kTile - 1u), ty = threadIdx.x >> 4;
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t trow = it / a.tiles_x, tcol = it - trow * a.tiles_x;
        const uint32_t row = trow * kTile + ty;
        if (row >= a.dh) continue;
        const uint64_t first = (uint64_t)(a.dy + row) * a.dst_w + a.dx;  // the row's first texel, in dst and in the map alike
        uint2* drow = a.dst + first;
        const uint32_t phase = (uint32_t)(((uintptr_t)drow >> 3) & (kTile - 1u));  // texels from the 128-byte line to the row's first texel
        const int64_t c = (int64_t)tcol * kTile + tx - phase;  // the lane's texel of the rectangle's row
        if (c < 0 || c >= (int64_t)a.dw) continue;
        // (unconditional, so that it is in flight under the plan's part of the position: without a map the lane's own destination
        // texel is loaded and replaced by 0)
        uint2 m = (a.map ? a.map : (const uint2*)a.dst)[first + (uint64_t)c];
        if (!a.map) m = make_uint2(0u, 0u);
        const uint32_t X = a.dx + (uint32_t)c, Y = a.dy + row;
        const int64_t U0 = jwarp_position(a.P, a.Q, a.R, X, Y), V0 = jwarp_position(a.S, a.T, a.W, X, Y);
        const uint64_t texel = (uint64_t)m.x | ((uint64_t)m.y << 32);
        const int64_t U = U0 + jdisp_offset(a.scale_x, (uint16_t)(texel >> a.shift_x));
        const int64_t V = V0 + jdisp_offset(a.scale_y, (uint16_t)(texel >> a.shift_y));
        float wx[N], wy[N];
        int32_t ix[N], iy[N];
        bool lx[N], ly[N];
        axis_taps<FILTER, EDGE>(U, (int32_t)a.sw, wx, ix, lx);
        axis_taps<FILTER, EDGE>(V, (int32_t)a.sh, wy, iy, ly);
        drow[c] = tap_sum<FILTER, EDGE, STRAIGHT>(a.src, a.src_w, wx, ix, lx, wy, iy, ly);
    }
}

template <int FILTER, int EDGE>
void launch_edge(hipStream_t stream, dim3 grid, bool straight, const DisplaceArgs& a) {
    with_flag(straight, [&](auto flag) {
        constexpr bool STRAIGHT = decltype(flag)::value;
        hipLaunchKernelGGL((k_displace<FILTER, EDGE, STRAIGHT>), grid, dim3(kThreads), 0, stream, a);
    });
}
template <int FILTER>
void launch_filter(hipStream_t stream, dim3 grid, int edge, bool straight, const DisplaceArgs& a) {
    switch (edge) {
        case JWARP_EDGE_ZERO: launch_edge<FILTER, JWARP_EDGE_ZERO>(stream, grid, straight, a); break;
        case JWARP_EDGE_CLAMP: launch_edge<FILTER, JWARP_EDGE_CLAMP>(stream, grid, straight, a); break;
        case JWARP_EDGE_REPEAT: launch_edge<FILTER, JWARP_EDGE_REPEAT>(stream, grid, straight, a); break;
        default: launch_edge<FILTER, JWARP_EDGE_MIRROR>(stream, grid, straight, a); break;
    }
}

}  // namespace

// The rectangle d of the RGBA16F image dst = the rectangle s of the image src (null texels: transparent black; another image than
// dst) under the plan (P, Q, R, S, T, W of include/jello_warp.h, host memory, read during the call), every position moved by the
// x_channel and y_channel of the image map (null texels: 0; of dst's size; may be dst or src) times scale_x and scale_y
// (include/jello_displace.h).  One launch on `stream`: one of the 24 instantiations of k_displace, filter x edge x straight.
// Returns 0, -1 on arguments it refuses (a plan outside a legal one's range among them: the kernel's indices are 32-bit), -2 on a
// launch error.
extern "C" int jh_displace_launch(hipStream_t stream, jimage_src src, jimage_rect s, jimage_src map, jimage_dst dst, jimage_rect d, const int64_t* plan,
                                  float scale_x, float scale_y, int x_channel, int y_channel, int filter, int edge, int straight, int num_cus) {
    if (!dst.texels || !plan || src.texels == dst.texels) return -1;
    if (jdisp_desc_error(filter, edge, 0u, scale_x, scale_y, x_channel, y_channel, src.width, src.height, map.width, map.height, dst.width, dst.height)) return -1;
    if (!jimage_rect_inside(s, src.width, src.height) || !jimage_rect_inside(d, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(s) || jimage_rect_empty(d)) return -1;
    for (int i = 0; i < 6; i++) {
        const int64_t lim = (i % 3) == 2 ? kMaxOffset : kMaxScale;
        if (plan[i] > lim || plan[i] < -lim) return -1;
    }
    DisplaceArgs a;
    a.src = src.texels ? (const uint2*)src.texels + ((uint64_t)s.y * src.width + s.x) : nullptr;
    a.map = (const uint2*)map.texels;
    a.dst = (uint2*)dst.texels;
    a.P = plan[0]; a.Q = plan[1]; a.R = plan[2]; a.S = plan[3]; a.T = plan[4]; a.W = plan[5];
    a.scale_x = scale_x; a.scale_y = scale_y;
    a.shift_x = 16u * (uint32_t)x_channel; a.shift_y = 16u * (uint32_t)y_channel;
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
