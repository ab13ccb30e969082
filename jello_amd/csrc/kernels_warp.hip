// kernels_warp.hip -- jh_warp: a rectangle of one RGBA16F image under an affine map into a rectangle of another, the device half of
// the rule in include/jello_hip.h ("Warp") and DESIGN.md 5.12; the host half -- the plan's six integers, the fraction, the cubic
// weights and the four index rules -- is include/jello_warp.h, compiled here too.  The argument block, its fill, the taps of an axis
// and the launch ladder are the warp family's (warp_taps.h); this file's own are the position of destination texel (X, Y) of the image
//   U = P (2 X + 1) + Q (2 Y + 1) + R,  V = S (2 X + 1) + T (2 Y + 1) + W          int64, exact: the source position in 2^-32 texel
// and a kernel body of its own, k_warp_affine: the family's k_warp<AffinePosition> is the same rule, and measured slower than the
// parent's kernel beyond the margin of DESIGN.md 5.8 (NEAREST, 2048^2 -> 4096^2: DESIGN.md 5.12 has the runs).  So the walk and
// warp_taps.h's tap_sum loop stay written out here, word for word; a change of either there is a change here, and the batteries of
// both calls hold them to one reference (tests/warp_ref.py).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_warp.h"
#include "kcommon.h"
#include "warp_taps.h"

namespace {

struct AffinePosition {
    int64_t plan[6];  // P, Q, R, S, T, W
    JD bool operator()(uint32_t X, uint32_t Y, uint64_t, int64_t* U, int64_t* V) const {
        *U = jwarp_position(plan[0], plan[1], plan[2], X, Y);
        *V = jwarp_position(plan[3], plan[4], plan[5], X, Y);
        return true;
    }
};

template <int FILTER, int EDGE, bool STRAIGHT>
__global__ __launch_bounds__(kThreads) void k_warp_affine(const TileArgs a, const AffinePosition pos) {
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
        int64_t U, V;
        pos(a.dx + (uint32_t)c, a.dy + row, 0u, &U, &V);
        float wx[N], wy[N];
        int32_t ix[N], iy[N];
        bool lx[N], ly[N];
        axis_taps<FILTER, EDGE>(U, (int32_t)a.sw, wx, ix, lx);
        axis_taps<FILTER, EDGE>(V, (int32_t)a.sh, wy, iy, ly);
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

}  // namespace

// The rectangle d of the RGBA16F image dst = the rectangle s of the image src (null texels: transparent black; another image than
// dst) under the plan (P, Q, R, S, T, W of include/jello_warp.h, host memory, read during the call).  One launch on `stream`: one of
// the 24 instantiations of k_warp_affine, filter x edge x straight.  Returns 0, -1 on arguments it refuses (a plan outside a
// legal one's range among them: the kernel's indices are 32-bit), -2 on a launch error.
extern "C" int jh_warp_launch(hipStream_t stream, jimage_src src, jimage_rect s, jimage_dst dst, jimage_rect d, const int64_t* plan, int filter,
                              int edge, int straight, int num_cus) {
    TileArgs a;
    if (!plan || jwarp_desc_error(filter, edge, 0u, src.width, src.height, dst.width, dst.height) || !tile_args(src, s, dst, d, &a)) return -1;
    if (!jwarp_plan_in_range(plan)) return -1;
    AffinePosition pos;
    for (int i = 0; i < 6; i++) pos.plan[i] = plan[i];
    return tile_launch(stream, a, pos, filter, edge, straight, num_cus,
                       [](auto f, auto e, auto s) { return &k_warp_affine<decltype(f)::value, decltype(e)::value, decltype(s)::value>; });
}
