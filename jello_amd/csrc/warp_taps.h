// warp_taps.h -- the device text of the warp family, jh_warp, jh_displace and jh_perspective: one kernel,
// its argument block and the host function that fills it, and the ladder that launches one of its 24 instantiations, filter x edge x
// straight.  A call contributes its position rule and nothing else: a trivially copyable struct that travels in the kernel arguments
// and has
//   __device__ bool operator()(uint32_t X, uint32_t Y, uint64_t at, int64_t* U, int64_t* V) const
// from the lane's texel (X, Y) of the destination image, `at` its index in that image, to the source position (U, V) in 2^-32 texel, or
// false: the texel is void, stores four +0.0 and loads nothing (a rule that never says so returns a constant, and the branch leaves
// no instruction).  The position type is the kernel's first template argument, so a trace names the call.  jh_warp launches a body of
// its own through the same ladder (kernels_warp.hip says why).  Per destination texel
//   (U, V) by the position rule
//   taps and weights of each axis from U and V; each tap index resolved against the source rectangle by the edge mode (axis_taps)
//   p = the f16 source texel widened, colour times alpha unless STRAIGHT; +0 in all four channels where ZERO says so
//   for each tap row j ascending: H_j = 0; H_j = fmaf(wx_i, p[i][j], H_j) for i ascending;  then V = 0; V = fmaf(wy_j, H_j, V)
//   store: STRAIGHT f16(V), otherwise V by the store rule (texel_io.h)
// One launch, no LDS, no tables, no scratch.  A wave's item is a TILE of the destination, 16 texels x 4 rows, not a row segment: under
// a rotation the preimage of a row crosses a source line per texel, the preimage of a tile is a compact parallelogram whose lines
// stay in the CU's vector cache for the tile's other rows.  Four waves make the 16 x 16 tile of a workgroup; the workgroups stride
// over the tiles in row-major order.  Each row of a tile is one 128-byte line of the destination IMAGE: the tile grid is laid on those
// lines, not on the rectangle's origin (`phase`, per row -- with a width that is no multiple of 16 it moves from row to row, as
// pair_walk's 16-byte phase does), and the lanes outside the rectangle are masked.  A lane owns one texel: its 1, 4 or 16 taps are
// direct 8-byte global loads, which assume no more alignment than a texel has (tap_sum).  REPEAT and MIRROR divide once per axis and
// texel (the first tap's index) and step from there.
// The host half is include/jello_warp.h.  Every function is internal to the file that includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_image.h"
#include "../../include/jello_warp.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTile = 16;  // a workgroup's tile: 16 x 16, a wave's: 16 x 4

struct TileArgs {
    const uint2* src;  // the source rectangle's first texel (null: never written, transparent black)
    uint2* dst;        // the destination image
    uint32_t src_w, sw, sh;            // texels per row of the source image; the source rectangle's extents
    uint32_t dst_w, dx, dy, dw, dh;    // texels per row of the destination image; the destination rectangle
    uint32_t tiles_x, total;
};

// The argument block of the rectangle d of dst from the rectangle s of src (null texels: transparent black; another image than dst);
// false for what the kernel cannot run: no destination, the source's own image, a rectangle outside its image or without texels.
inline bool tile_args(jimage_src src, jimage_rect s, jimage_dst dst, jimage_rect d, TileArgs* a) {
    if (!dst.texels || src.texels == dst.texels) return false;
    if (!jimage_rect_inside(s, src.width, src.height) || !jimage_rect_inside(d, dst.width, dst.height)) return false;
    if (jimage_rect_empty(s) || jimage_rect_empty(d)) return false;
    a->src = src.texels ? (const uint2*)src.texels + ((uint64_t)s.y * src.width + s.x) : nullptr;
    a->dst = (uint2*)dst.texels;
    a->src_w = src.width; a->sw = s.w; a->sh = s.h;
    a->dst_w = dst.width; a->dx = d.x; a->dy = d.y; a->dw = d.w; a->dh = d.h;
    a->tiles_x = (d.w + 2u * (kTile - 1u)) / kTile;  // (+ 15: the grid of lines may start up to 15 texels before the row)
    a->total = a->tiles_x * ((d.h + kTile - 1u) / kTile);
    return true;
}

template <int FILTER>
struct Taps { static constexpr int N = FILTER == JWARP_NEAREST ? 1 : (FILTER == JWARP_BILINEAR ? 2 : 4); };

// The taps of one axis at position U against the extent n: weights, the indices to load (always inside [0, n)) and whether the
// operand is the loaded texel (false: ZERO's +0).
template <int FILTER, int EDGE>
JD void axis_taps(int64_t U, int32_t n, float (&w)[Taps<FILTER>::N], int32_t (&idx)[Taps<FILTER>::N], bool (&live)[Taps<FILTER>::N]) {
    constexpr int N = Taps<FILTER>::N;
    int32_t i0;
    if (FILTER == JWARP_NEAREST) {
        i0 = jwarp_nearest(U);
        w[0] = 1.0f;
    } else {
        float f;
        i0 = jwarp_split(U, &f);
        if (FILTER == JWARP_BILINEAR) {
            w[0] = 1.0f - f;
            w[N - 1] = f;
        } else {
            float c[4];
            jwarp_cubic_weights(f, c);
#pragma unroll
            for (int k = 0; k < N; k++) w[k] = c[k];
            i0 -= 1;
        }
    }
    if (EDGE == JWARP_EDGE_ZERO || EDGE == JWARP_EDGE_CLAMP) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int32_t i = i0 + k;
            live[k] = EDGE == JWARP_EDGE_CLAMP || (i >= 0 && i < n);
            idx[k] = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
        }
    } else {
        const int32_t period = EDGE == JWARP_EDGE_REPEAT ? n : 2 * n;
        int32_t m = jwarp_mod(i0, period);
#pragma unroll
        for (int k = 0; k < N; k++) {
            live[k] = true;
            idx[k] = (EDGE == JWARP_EDGE_REPEAT || m < n) ? m : 2 * n - 1 - m;
            m = m + 1 == period ? 0 : m + 1;
        }
    }
}

// The texel the rule stores for the taps of the two axes (axis_taps of U against the source rectangle's width, of V against its
// height): src is the rectangle's first texel (null: never written, transparent black), src_w the texels to a row of its image.  The
// loads of a lane are unconditional (a tap ZERO takes out reads the rectangle's nearest texel and is replaced by +0 afterwards), so
// all of them can be in flight together.  kernels_warp.hip's k_warp_affine keeps this loop, and k_warp's walk, written out a second
// time (as k_warp<AffinePosition> it measured slower than the parent's kernel: DESIGN.md 5.12): a change of one is a change of both.
template <int FILTER, int EDGE, bool STRAIGHT>
JD uint2 tap_sum(const uint2* src, uint32_t src_w, const float (&wx)[Taps<FILTER>::N], const int32_t (&ix)[Taps<FILTER>::N], const bool (&lx)[Taps<FILTER>::N],
                 const float (&wy)[Taps<FILTER>::N], const int32_t (&iy)[Taps<FILTER>::N], const bool (&ly)[Taps<FILTER>::N]) {
    constexpr int N = Taps<FILTER>::N;
    uint2 t[N][N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint2* srow = src + (uint64_t)(uint32_t)iy[j] * src_w;
#pragma unroll
        for (int i = 0; i < N; i++) {
            t[j][i] = make_uint2(0u, 0u);
            if (src) t[j][i] = srow[ix[i]];
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
    return texel_store<STRAIGHT>(v);
}

template <class POS, int FILTER, int EDGE, bool STRAIGHT>
__global__ __launch_bounds__(kThreads) void k_warp(const TileArgs a, const POS pos) {
    constexpr int N = Taps<FILTER>::N;
    const uint32_t tx = threadIdx.x & (kTile - 1u), ty = threadIdx.x >> 4;
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t trow = it / a.tiles_x, tcol = it - trow * a.tiles_x;
        const uint32_t row = trow * kTile + ty;
        if (row >= a.dh) continue;
        const uint64_t first = (uint64_t)(a.dy + row) * a.dst_w + a.dx;  // the row's first texel, as an index in the destination image
        uint2* drow = a.dst + first;
        const uint32_t phase = (uint32_t)(((uintptr_t)drow >> 3) & (kTile - 1u));  // texels from the 128-byte line to the row's first texel
        const int64_t c = (int64_t)tcol * kTile + tx - phase;  // the lane's texel of the rectangle's row
        if (c < 0 || c >= (int64_t)a.dw) continue;
        int64_t U, V;
        uint2 out = make_uint2(0u, 0u);  // (a void texel: four +0.0)
        if (pos(a.dx + (uint32_t)c, a.dy + row, first + (uint64_t)c, &U, &V)) {
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

// f(filter, edge, straight), the three run-time values as integral constants: the filter x edge x straight ladder, written once.  The
// caller has checked filter and edge (jwarp_filter_ok, jwarp_edge_ok).
template <int V>
using TapInt = std::integral_constant<int, V>;
template <int FILTER, class F>
void ladder_edge(int edge, bool straight, F& f) {
    with_flag(straight, [&](auto flag) {
        switch (edge) {
            case JWARP_EDGE_ZERO: f(TapInt<FILTER>{}, TapInt<JWARP_EDGE_ZERO>{}, flag); break;
            case JWARP_EDGE_CLAMP: f(TapInt<FILTER>{}, TapInt<JWARP_EDGE_CLAMP>{}, flag); break;
            case JWARP_EDGE_REPEAT: f(TapInt<FILTER>{}, TapInt<JWARP_EDGE_REPEAT>{}, flag); break;
            default: f(TapInt<FILTER>{}, TapInt<JWARP_EDGE_MIRROR>{}, flag); break;
        }
    });
}
template <class F>
void ladder(int filter, int edge, bool straight, F&& f) {
    switch (filter) {
        case JWARP_NEAREST: ladder_edge<JWARP_NEAREST>(edge, straight, f); break;
        case JWARP_BILINEAR: ladder_edge<JWARP_BILINEAR>(edge, straight, f); break;
        default: ladder_edge<JWARP_BICUBIC>(edge, straight, f); break;
    }
}
// One launch on `stream` of the instantiation (filter, edge, straight) of the kernel kernel_of(filter, edge, straight) names, on the
// family's grid, with the arguments (a, pos): 0, -2 on a launch error.
template <class POS, class K>
int tile_launch(hipStream_t stream, const TileArgs& a, const POS& pos, int filter, int edge, int straight, int num_cus, K&& kernel_of) {
    const dim3 grid(grid_blocks((uint64_t)a.total * kWaves, kWaves, 8u, num_cus));
    ladder(filter, edge, straight != 0, [&](auto f, auto e, auto s) { hipLaunchKernelGGL(kernel_of(f, e, s), grid, dim3(kThreads), 0, stream, a, pos); });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
// The same for the family's kernel under the position rule pos.
template <class POS>
int tile_launch(hipStream_t stream, const TileArgs& a, const POS& pos, int filter, int edge, int straight, int num_cus) {
    return tile_launch(stream, a, pos, filter, edge, straight, num_cus,
                       [](auto f, auto e, auto s) { return &k_warp<POS, decltype(f)::value, decltype(e)::value, decltype(s)::value>; });
}

}  // namespace
