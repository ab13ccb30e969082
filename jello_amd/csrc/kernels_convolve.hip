// kernels_convolve.hip -- jh_convolve: feConvolveMatrix on an RGBA16F image, the device half of the rule in include/jello_hip.h
// ("Convolve") and DESIGN.md 5.13; the host half -- the limits, the legal descriptor, the flip and the divisor -- is
// include/jello_convolve.h, and the index rules are jwarp_index of include/jello_warp.h.  Per destination texel (X, Y) of the rectangle
//   p(i, j) = the operand at the image position (X - target_x + i, Y - target_y + j), each axis resolved by the edge mode against the
//             IMAGE: the f16 texel widened, colour times alpha under PREMULTIPLIED; +0 in all channels where ZERO says so
//   acc = 0;  for j ascending, for i ascending: acc = fmaf(w[j][i], p(i, j), acc)                       one chain per channel
//   the bias (if it is not +-0), then the store of the mode
// One launch, no tables, no scratch: the weights travel in the kernel arguments and are read with scalar loads.  A workgroup of 256
// lanes owns a TILE of the destination, 64 texels x 16 rows, and stages the tile's source footprint, (64 + ox - 1) x (16 + oy - 1)
// operands of four binary32, into LDS once, the edge mode resolved while staging: the tap loop has no edge logic and a tap is one
// ds_read_b128.  The tiles are laid on the destination IMAGE's 128-byte lines (`phase`, taken at the tile's first row: with a width
// that is a multiple of 16 texels every row of every tile starts a line) and the lanes outside the rectangle are masked at the store.
// A wave owns 4 rows of the tile and a lane a VERTICAL strip of them, 4 outputs of one column: neighbouring lanes read neighbouring
// 16-byte slots of LDS, which has no bank conflict, and an operand that is loaded once feeds up to 4 outputs from registers --
// ox (oy + 3) LDS reads for 4 ox oy fma4.  Footprint rows ascending and i ascending is every output's chain in the rule's order.
// Orders 3 x 3 and 5 x 5 are compile-time instantiations (the loops unroll, the weights stay in scalar registers); every other order
// runs the general one, which walks run-time orders.  All of them give the rule's bits.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_convolve.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTileW = 64, kTileH = 16, kStrip = kTileH / kWaves;  // a lane's strip: 4 rows of one column
constexpr uint32_t kLine = 16;                // texels of a 128-byte line
constexpr uint32_t kMaxSide = 1u << 29;       // 2 n of MIRROR and a position 14 texels beyond it stay an int32

struct ConvArgs {
    const uint2* src;  // the source image (null: never written, transparent black)
    uint2* dst;        // the destination image, of the same size
    uint32_t width, height;  // texels per row and rows of both images
    uint32_t dx, dy, dw, dh;  // the rectangle that is written
    uint32_t ox, oy, tx, ty;  // orders and target
    int edge;
    float bias;
    uint32_t tiles_x, total;
    float w[JCONV_MAX_TAPS + 3u];  // (+ 3: taps_step reads four at a time)
};

// The operand of a source texel: MODE JCONV_PREMULTIPLIED colour times alpha, otherwise as stored (PRESERVE_ALPHA never reads .w).
template <int MODE>
JD float4 operand(uint2 t) { return MODE == JCONV_PREMULTIPLIED ? texel_widen<false>(t) : texel_widen<true>(t); }

// The general instantiation's step: footprint row fr of a strip (`row`: its first operand) into the outputs KLO .. KHI of the strip, whose
// kernel rows are fr - k, four taps at a time: the four weights of each kernel row are ONE scalar load of 16 bytes (a 4-byte
// alignment is all it needs), the loads of a step are issued together and waited for once, and the step has no branch.  The last
// step of a row loads up to three weights it does not use: ConvArgs::w is padded for the two that can lie behind the 225.
struct __attribute__((packed, aligned(4))) Weights4 { float v[4]; };
template <int KLO, int KHI, int N>
JD void taps_step(float4 (&acc)[kStrip], const float4* row, const float* w, uint32_t ox, uint32_t fr) {
    Weights4 wq[KHI - KLO + 1];
    float4 p[N];
#pragma unroll
    for (int k = KLO; k <= KHI; k++) wq[k - KLO] = *(const Weights4*)(w + (fr - (uint32_t)k) * ox);
#pragma unroll
    for (int i = 0; i < N; i++) p[i] = row[i];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int k = KLO; k <= KHI; k++) fma4(acc[k], wq[k - KLO].v[i], p[i]);
}
template <int KLO, int KHI>
JD void taps_row(float4 (&acc)[kStrip], const float4* row, const float* w, uint32_t ox, uint32_t fr) {
    uint32_t i = 0;
    for (; i + 4u <= ox; i += 4u) taps_step<KLO, KHI, 4>(acc, row + i, w + i, ox, fr);
    switch (ox - i) {
        case 1: taps_step<KLO, KHI, 1>(acc, row + i, w + i, ox, fr); break;
        case 2: taps_step<KLO, KHI, 2>(acc, row + i, w + i, ox, fr); break;
        case 3: taps_step<KLO, KHI, 3>(acc, row + i, w + i, ox, fr); break;
        default: break;
    }
}

// OX, OY: the orders at compile time, or 0 x 0: a.ox, a.oy.
template <int OX, int OY, int MODE>
__global__ __launch_bounds__(kThreads) void k_convolve(const ConvArgs a) {
    extern __shared__ float4 foot[];  // the footprint, row-major, fw operands to a row
    const uint32_t ox = OX ? (uint32_t)OX : a.ox, oy = OY ? (uint32_t)OY : a.oy;
    const uint32_t fw = kTileW + ox - 1u, fh = kTileH + oy - 1u;
    const uint32_t lane = threadIdx.x & (kTileW - 1u), wave = threadIdx.x >> 6;
    const uint32_t sx = threadIdx.x & 127u, sy = threadIdx.x >> 7;  // staging: two footprint rows at a time, a lane per column
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t trow = it / a.tiles_x, tcol = it - trow * a.tiles_x;
        const uint32_t row0 = trow * kTileH;  // the tile's first row of the rectangle
        const uint32_t phase = (uint32_t)((((uintptr_t)a.dst >> 3) + (uint64_t)(a.dy + row0) * a.width + a.dx) & (kLine - 1u));
        const int32_t col0 = (int32_t)(tcol * kTileW) - (int32_t)phase;  // the tile's first column of the rectangle (may lie before it)
        // stage: footprint (fx, fy) is the image position (X0 + fx, Y0 + fy)
        const int32_t X0 = (int32_t)a.dx + col0 - (int32_t)a.tx, Y0 = (int32_t)(a.dy + row0) - (int32_t)a.ty;
        if (sx < fw) {
            const int32_t ix = jwarp_index(a.edge, X0 + (int32_t)sx, (int32_t)a.width);
            for (uint32_t fy = sy; fy < fh; fy += 2u) {
                const int32_t iy = jwarp_index(a.edge, Y0 + (int32_t)fy, (int32_t)a.height);
                float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (a.src && ix >= 0 && iy >= 0) p = operand<MODE>(a.src[(uint64_t)(uint32_t)iy * a.width + (uint32_t)ix]);
                foot[fy * fw + sx] = p;
            }
        }
        __syncthreads();
        const uint32_t r0 = row0 + wave * kStrip;  // the strip's first row of the rectangle
        if (r0 < a.dh) {                           // (uniform in the wave)
            float4 acc[kStrip];
#pragma unroll
            for (uint32_t k = 0; k < kStrip; k++) acc[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float4* strip = foot + (wave * kStrip) * fw + lane;
            if (OX) {
#pragma unroll
                for (int fr = 0; fr < OY + (int)kStrip - 1; fr++) {
#pragma unroll
                    for (int i = 0; i < OX; i++) {
                        const float4 p = strip[fr * (int)fw + i];
#pragma unroll
                        for (int k = 0; k < (int)kStrip; k++)
                            if (fr - k >= 0 && fr - k < OY) fma4(acc[k], a.w[(fr - k) * OX + i], p);
                    }
                }
            } else {
                for (uint32_t fr = 0; fr < oy + kStrip - 1u; fr++) {
                    // the outputs footprint row fr feeds: k with 0 <= fr - k < oy, a range [klo, khi]; [0, 3] in all but the first and last three rows
                    const uint32_t klo = fr + 1u > oy ? fr + 1u - oy : 0u, khi = fr < kStrip - 1u ? fr : kStrip - 1u;
                    const float4* row = strip + fr * fw;
                    switch (klo * kStrip + khi) {
                        case 0: taps_row<0, 0>(acc, row, a.w, ox, fr); break;
                        case 1: taps_row<0, 1>(acc, row, a.w, ox, fr); break;
                        case 2: taps_row<0, 2>(acc, row, a.w, ox, fr); break;
                        case 3: taps_row<0, 3>(acc, row, a.w, ox, fr); break;
                        case 5: taps_row<1, 1>(acc, row, a.w, ox, fr); break;
                        case 6: taps_row<1, 2>(acc, row, a.w, ox, fr); break;
                        case 7: taps_row<1, 3>(acc, row, a.w, ox, fr); break;
                        case 10: taps_row<2, 2>(acc, row, a.w, ox, fr); break;
                        case 11: taps_row<2, 3>(acc, row, a.w, ox, fr); break;
                        default: taps_row<3, 3>(acc, row, a.w, ox, fr); break;
                    }
                }
            }
            const int32_t c = col0 + (int32_t)lane;  // the lane's column of the rectangle
            if (c >= 0 && c < (int32_t)a.dw) {
                const bool biased = a.bias != 0.0f;
#pragma unroll
                for (uint32_t k = 0; k < kStrip; k++) {
                    if (r0 + k >= a.dh) break;
                    const uint64_t at = (uint64_t)(a.dy + r0 + k) * a.width + (a.dx + (uint32_t)c);
                    float4 v = acc[k];
                    if (biased) {
                        if (MODE == JCONV_PREMULTIPLIED) {
                            v.w = v.w + a.bias;
                            v.x = __builtin_fmaf(a.bias, v.w, v.x); v.y = __builtin_fmaf(a.bias, v.w, v.y); v.z = __builtin_fmaf(a.bias, v.w, v.z);
                        } else {
                            v.x = v.x + a.bias; v.y = v.y + a.bias; v.z = v.z + a.bias;
                            if (MODE == JCONV_STRAIGHT) v.w = v.w + a.bias;
                        }
                    }
                    uint2 out;
                    if (MODE == JCONV_PRESERVE_ALPHA) {
                        const uint32_t alpha = a.src ? (a.src[at].y & 0xffff0000u) : 0u;  // the source texel's 16 bits, copied
                        v.w = 0.0f;
                        out = texel_pack(v);
                        out.y = (out.y & 0x0000ffffu) | alpha;
                    } else {
                        out = texel_store<MODE == JCONV_STRAIGHT>(v);
                    }
                    a.dst[at] = out;
                }
            }
        }
        __syncthreads();  // the next tile's staging overwrites the footprint
    }
}

template <int OX, int OY>
void launch_order(hipStream_t stream, dim3 grid, uint32_t lds, int mode, const ConvArgs& a) {
    switch (mode) {
        case JCONV_PREMULTIPLIED: hipLaunchKernelGGL((k_convolve<OX, OY, JCONV_PREMULTIPLIED>), grid, dim3(kThreads), lds, stream, a); break;
        case JCONV_STRAIGHT: hipLaunchKernelGGL((k_convolve<OX, OY, JCONV_STRAIGHT>), grid, dim3(kThreads), lds, stream, a); break;
        default: hipLaunchKernelGGL((k_convolve<OX, OY, JCONV_PRESERVE_ALPHA>), grid, dim3(kThreads), lds, stream, a); break;
    }
}

}  // namespace

// The rectangle r of the RGBA16F image dst = the convolution of the image src (null texels: transparent black; another image of the
// same size) with the order_x x order_y weights (host memory, read during the call) by the rule.  One launch on `stream`: one of the 9
// instantiations of k_convolve, order class (3 x 3, 5 x 5, general) x mode, with (64 + order_x - 1) x (16 + order_y - 1) x 16 bytes
// of LDS -- 19 KB at 3 x 3, 37 KB at 15 x 15.  Returns 0, -1 on arguments it refuses (sizes the kernel's 32-bit indices do not
// hold among them), -2 on a launch error.
extern "C" int jh_convolve_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect r, uint32_t order_x, uint32_t order_y,
                                  uint32_t target_x, uint32_t target_y, const float* weights, int edge, int mode, float bias, int num_cus) {
    if (!dst.texels || !weights || src.texels == dst.texels || src.width != dst.width || src.height != dst.height) return -1;
    if (!jconv_order_ok(order_x, order_y) || target_x >= order_x || target_y >= order_y || !jwarp_edge_ok(edge) || !jconv_mode_ok(mode)) return -1;
    if (dst.width > kMaxSide || dst.height > kMaxSide) return -1;
    if (!jimage_rect_inside(r, dst.width, dst.height) || jimage_rect_empty(r)) return -1;
    const uint64_t tiles_x = ((uint64_t)r.w + (kLine - 1u) + (kTileW - 1u)) / kTileW;  // (+ 15: the grid of lines may start up to 15 texels before the row)
    const uint64_t total = tiles_x * (((uint64_t)r.h + kTileH - 1u) / kTileH);
    if (total > 0x7fffffffu) return -1;
    ConvArgs a;
    a.src = (const uint2*)src.texels;
    a.dst = (uint2*)dst.texels;
    a.width = dst.width; a.height = dst.height;
    a.dx = r.x; a.dy = r.y; a.dw = r.w; a.dh = r.h;
    a.ox = order_x; a.oy = order_y; a.tx = target_x; a.ty = target_y;
    a.edge = edge;
    a.bias = bias;
    a.tiles_x = (uint32_t)tiles_x;
    a.total = (uint32_t)total;
    for (uint32_t k = 0; k < JCONV_MAX_TAPS + 3u; k++) a.w[k] = k < order_x * order_y ? weights[k] : 0.0f;
    const uint32_t lds = (kTileW + order_x - 1u) * (kTileH + order_y - 1u) * (uint32_t)sizeof(float4);
    const dim3 grid(grid_blocks(total * kWaves, kWaves, 8u, num_cus));
    if (order_x == 3u && order_y == 3u) launch_order<3, 3>(stream, grid, lds, mode, a);
    else if (order_x == 5u && order_y == 5u) launch_order<5, 5>(stream, grid, lds, mode, a);
    else launch_order<0, 0>(stream, grid, lds, mode, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
