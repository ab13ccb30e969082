// kernels_warp.hip -- jh_warp: a rectangle of one RGBA16F image under an affine map into a rectangle of another, the device half of
// the rule in include/jello_hip.h ("Warp") and DESIGN.md 5.12; the host half -- the plan's six integers, the fraction, the cubic
// weights and the four index rules -- is include/jello_warp.h, compiled here too.  Per destination texel (X, Y) of the image
//   U = P (2 X + 1) + Q (2 Y + 1) + R,  V = S (2 X + 1) + T (2 Y + 1) + W          int64, exact: the source position in 2^-32 texel
//   taps and weights of each axis from U and V; each tap index resolved against the source rectangle by the edge mode
//   p = the f16 source texel widened, colour times alpha unless STRAIGHT; +0 in all four channels where ZERO says so
//   for each tap row j ascending: H_j = 0; H_j = fmaf(wx_i, p[i][j], H_j) for i ascending;  then V = 0; V = fmaf(wy_j, H_j, V)
//   store: STRAIGHT f16(V), otherwise V by the store rule (texel_io.h)
// One launch, no LDS, no tables, no scratch.  A wave's item is a TILE of the destination, 16 texels x 4 rows, not a row segment: under
// a rotation the preimage of a row crosses a source line per texel, the preimage of a tile is a compact parallelogram whose lines
// stay in the CU's vector cache for the tile's other rows.  Four waves make the 16 x 16 tile of a workgroup; the workgroups stride
// over the tiles in row-major order.  Each row of a tile is one 128-byte line of the destination IMAGE: the tile grid is laid on those
// lines, not on the rectangle's origin (`phase`, per row -- with a width that is no multiple of 16 it moves from row to row, as
// pair_walk's 16-byte phase does), and the lanes outside the rectangle are masked.  A lane owns one texel: its 1, 4 or 16 taps are
// direct 8-byte global loads, which assume no more alignment than a texel has.  The loads of a lane are unconditional (a tap ZERO
// takes out reads the rectangle's nearest texel and is replaced by +0 afterwards), so all of them can be in flight together.
// REPEAT and MIRROR divide once per axis and texel (the first tap's index) and step from there.
// The taps of an axis (Taps, axis_taps) are warp_taps.h's, shared with kernels_displace.hip; that header's tap_sum is this kernel's load
// and sum loop word for word, and the loop stays written out here because the helper's call changes this file's instructions (the
// reason three loops of texel_io.h stay written out: DESIGN.md 5.8 and 5.17).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_warp.h"
#include "kcommon.h"
#include "texel_io.h"
#include "warp_taps.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTile = 16;  // a workgroup's tile: 16 x 16, a wave's: 16 x 4
constexpr int64_t kMaxScale = (int64_t)1 << 37, kMaxOffset = (int64_t)1 << 54;  // 64 x 2^31, 2^22 x 2^32: what a legal plan stays inside

struct WarpArgs {
    const uint2* src;  // the source rectangle's first texel (null: never written, transparent black)
    uint2* dst;        // the destination image
    int64_t P, Q, R, S, T, W;
    uint32_t src_w, sw, sh;            // texels per row of the source image; the source rectangle's extents
    uint32_t dst_w, dx, dy, dw, dh;    // texels per row of the destination image; the destination rectangle
    uint32_t tiles_x, total;
};

template <int FILTER, int EDGE, bool STRAIGHT>
__global__ __launch_bounds__(kThreads) void k_warp(const WarpArgs a) {
    constexpr int N = Taps<FILTER>::N;
    const uint32_t tx = threadIdx.x & (kTile - 1u), ty = threadIdx.x >> 4;
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t trow = it / a.tiles_x, tcol = it - trow * a.tiles_x;
        const uint32_t row = trow * kTile + ty;
        if (row >= a.dh) continue;
        uint2* drow = a.dst + ((uint64_t)(a.dy + row) * a.dst_w + a.dx);
        const uint32_t phase = (uint32_t)(((uintptr_t)drow >> 3) & (kTile - 1u));  // texels from the 128-byte line to the row's first texel
        const int64_t c = (int64_t)tcol * kTile + tx - phase;  // the lane's texel of the rectangle's row
        if (c < 0 || c >= (int64_t)a.dw) continue;
        const uint32_t X = a.dx + (uint32_t)c, Y = a.dy + row;
        float wx[N], wy[N];
        int32_t ix[N], iy[N];
        bool lx[N], ly[N];
        axis_taps<FILTER, EDGE>(jwarp_position(a.P, a.Q, a.R, X, Y), (int32_t)a.sw, wx, ix, lx);
        axis_taps<FILTER, EDGE>(jwarp_position(a.S, a.T, a.W, X, Y), (int32_t)a.sh, wy, iy, ly);
        uint2 t[N][N];
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint2* srow = a.src + (uint64_t)(uint32_t)iy[j] * a.src_w;
#pragma unroll
            for (int i = 0; i < N; i++) {
                t[j][i] = make_uint2(0u, 0u);
                if (a.src) t[j][i] = srow[ix[i]];
                if (EDGE == JWARP_EDGE_ZERO && !(lx[i] && ly[j])) t[j][i] = make_uint2(0u, 0u);
            }
        }
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int j = 0; j < N; j++) {
            float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int i = 0; i < N; i++) fma4(h, wx[i], texel_widen<STRAIGHT>(t[j][i]));
            fma4(v, wy[j], h);
        }
        drow[c] = texel_store<STRAIGHT>(v);
    }
}

template <int FILTER, int EDGE>
void launch_edge(hipStream_t stream, dim3 grid, bool straight, const WarpArgs& a) {
    with_flag(straight, [&](auto flag) {
        constexpr bool STRAIGHT = decltype(flag)::value;
        hipLaunchKernelGGL((k_warp<FILTER, EDGE, STRAIGHT>), grid, dim3(kThreads), 0, stream, a);
    });
}
template <int FILTER>
void launch_filter(hipStream_t stream, dim3 grid, int edge, bool straight, const WarpArgs& a) {
    switch (edge) {
        case JWARP_EDGE_ZERO: launch_edge<FILTER, JWARP_EDGE_ZERO>(stream, grid, straight, a); break;
        case JWARP_EDGE_CLAMP: launch_edge<FILTER, JWARP_EDGE_CLAMP>(stream, grid, straight, a); break;
        case JWARP_EDGE_REPEAT: launch_edge<FILTER, JWARP_EDGE_REPEAT>(stream, grid, straight, a); break;
        default: launch_edge<FILTER, JWARP_EDGE_MIRROR>(stream, grid, straight, a); break;
    }
}

}  // namespace

// The rectangle d of the RGBA16F image dst = the rectangle s of the image src (null texels: transparent black; another image than
// dst) under the plan (P, Q, R, S, T, W of include/jello_warp.h, host
// memory, read during the call).  One launch on `stream`: one of the 24 instantiations of k_warp, filter x edge x straight.
// Returns 0, -1 on arguments it refuses (a plan outside a legal one's range among them: the kernel's indices are 32-bit), -2 on a
// launch error.
extern "C" int jh_warp_launch(hipStream_t stream, jimage_src src, jimage_rect s, jimage_dst dst, jimage_rect d, const int64_t* plan, int filter,
                              int edge, int straight, int num_cus) {
    if (!dst.texels || !plan || src.texels == dst.texels || !jwarp_filter_ok(filter) || !jwarp_edge_ok(edge)) return -1;
    if (src.width > JWARP_MAX_SIDE || src.height > JWARP_MAX_SIDE || dst.width > JWARP_MAX_SIDE || dst.height > JWARP_MAX_SIDE) return -1;
    if (!jimage_rect_inside(s, src.width, src.height) || !jimage_rect_inside(d, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(s) || jimage_rect_empty(d)) return -1;
    for (int i = 0; i < 6; i++) {
        const int64_t lim = (i % 3) == 2 ? kMaxOffset : kMaxScale;
        if (plan[i] > lim || plan[i] < -lim) return -1;
    }
    WarpArgs a;
    a.src = src.texels ? (const uint2*)src.texels + ((uint64_t)s.y * src.width + s.x) : nullptr;
    a.dst = (uint2*)dst.texels;
    a.P = plan[0]; a.Q = plan[1]; a.R = plan[2]; a.S = plan[3]; a.T = plan[4]; a.W = plan[5];
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
