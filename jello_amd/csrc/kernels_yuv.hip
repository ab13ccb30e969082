// kernels_yuv.hip -- jh_blit_yuv: the RGBA16F target -> planar 8-bit Y'CbCr 4:2:0 (NV12 or I420) for a video encoder on the
// host.  The rule is in include/jello_hip.h and DESIGN.md 5.5 ("YUV blit"); tests/yuv_ref.py restates it in numpy:
//   R'G'B' codes = bytes 0..2 of jh_blit's RGBA8_UNORM / RGBA8_SRGB pixel (blit_pixel, blit_convert.h)
//   Y  = clamp8(off + ((My . (R, G, B) + 2^15) >> 16))                        per pixel
//   Cb = clamp8(128 + ((Mb . (S_R, S_G, S_B) + 2^17) >> 18)), Cr with Mr      S = sum of the codes of the 2 x 2 luma positions,
//                                                                             the last column / row counted twice at an odd edge
// Streaming: 8 B read and 1.5 B written per pixel, nothing reused.  A lane converts chroma samples -- 2 x 2 pixels: two 16-B
// loads, adjacent lanes reading adjacent texels -- and leaves 2 + 2 luma bytes and the (Cb, Cr) pair in LDS; a block's tile is
// 512 samples of one pair of luma rows (1024 x 2 pixels).  After one barrier 192 lanes each move 16 B of the tile's three
// byte strings (luma row, luma row, chroma) from LDS to the planes: 16-B stores when every plane pointer and pitch is a
// multiple of 16 (`wide`); single-byte stores of the same bytes otherwise and for the last, partial 16 B of a row.
// Bytes between a row's end and its pitch, and rows below a plane, are never touched.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_frame.h"
#include "blit_convert.h"
#include "kcommon.h"
#include "texel_io.h"
#include "yuv_matrix_lut.h"

namespace {

constexpr uint32_t kYuvThreads = 256;

struct YuvCoef {
    int32_t y[3], cb[3], cr[3], off;
};
struct YuvPlanes {
    uint8_t* p[3];  // Y, CbCr interleaved (NV12) or Cb, - or Cr
    uint64_t pitch[3];
};

// row . (r, g, b) + bias with 24-bit multiplies (full rate; a 32-bit v_mul_lo is a quarter of it): the coefficients need 17 bits
// with their sign, the codes 8 and their sums over four pixels 10, and every result fits int32
__device__ __forceinline__ int32_t yuv_dot(const int32_t m[3], int32_t r, int32_t g, int32_t b, int32_t bias) {
    return __mul24(m[0], r) + __mul24(m[1], g) + __mul24(m[2], b) + bias;
}

// The two texels of a row that a chroma sample covers: x (even) and min(x + 1, width - 1).  One 16-B load where both lie inside
// the row and the address allows.  row == null: a never-written source reads as transparent black.
__device__ __forceinline__ void yuv_load2(const uint2* row, uint32_t x, uint32_t width, uint2& t0, uint2& t1) {
    t0 = t1 = make_uint2(0u, 0u);
    if (!row) return;
    const uint2* s = row + x;
    if (x + 1u < width) {
        if (((uintptr_t)s & 15u) == 0u) {  // (the same for every sample of the row)
            const uint4 a = *(const uint4*)s;
            t0 = make_uint2(a.x, a.y); t1 = make_uint2(a.z, a.w);
        } else {
            t0 = s[0]; t1 = s[1];
        }
    } else {
        t0 = t1 = s[0];
    }
}

constexpr uint32_t kYuvPerLane = 2;                          // chroma samples a lane converts per tile
constexpr uint32_t kYuvTile = kYuvThreads * kYuvPerLane;     // chroma samples of a tile
constexpr uint32_t kYuvChunks = kYuvTile / 8u;               // 16-B chunks of one of a tile's three byte strings (2 B per sample)
static_assert(3u * kYuvChunks <= kYuvThreads, "one lane per 16-B chunk");

// Work items are tiles of kYuvTile chroma samples of one pair of luma rows: tiles_per_pair per pair, pairs [pair0, pair0 +
// total_tiles / tiles_per_pair), numbered row-major; a block takes a tile at a time, the grid strides over them.
// LDS per tile (two of them, so that one barrier per tile is enough): [0, 2T) luma of row 2 * pair, [2T, 4T) luma of the row
// below, [4T, 6T) chroma -- (Cb, Cr) pairs for NV12; T bytes of Cb, then T bytes of Cr for I420.
template <bool SRGB, bool NV12>
__global__ __launch_bounds__(kYuvThreads) void k_blit_yuv(const uint2* __restrict__ src, YuvPlanes pl, YuvCoef k, uint32_t width,
                                                          uint32_t height, uint32_t pair0, uint32_t tiles_per_pair,
                                                          uint32_t total_tiles, uint32_t wide) {
    constexpr uint32_t T = kYuvTile;
    __shared__ float2 lut[SRGB ? 256 : 1];
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][6u * T];
    if (SRGB) {
        blit_srgb_lut_fill(lut, threadIdx.x);  // (kYuvThreads = 256 entries)
        __syncthreads();
    }
    const uint32_t cw = (width + 1u) >> 1;
    uint32_t buf = 0u;
    for (uint32_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x, buf ^= 1u) {
        const uint32_t pr = tile / tiles_per_pair;
        const uint32_t s0 = (tile - pr * tiles_per_pair) * T;  // first chroma sample of the tile
        const uint32_t pair = pair0 + pr;
        const uint32_t y0 = 2u * pair;
        const bool two_rows = y0 + 1u < height;  // else the last row counts twice
        const uint2* srow0 = src ? src + (uint64_t)y0 * width : nullptr;
        const uint2* srow1 = src ? srow0 + (two_rows ? width : 0u) : nullptr;
        uint8_t* st = stage[buf];
#pragma unroll
        for (uint32_t u = 0; u < kYuvPerLane; u++) {
            const uint32_t i = u * kYuvThreads + threadIdx.x;  // sample of the tile
            const uint32_t cx = s0 + i;
            if (cx >= cw) continue;
            uint2 t[4];
            yuv_load2(srow0, 2u * cx, width, t[0], t[1]);
            yuv_load2(srow1, 2u * cx, width, t[2], t[3]);
            int32_t sr = 0, sg = 0, sb = 0;
            uint32_t yy[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t px = blit_pixel<SRGB, false>(t[j], lut);
                const int32_t r = (int32_t)(px & 0xffu), g = (int32_t)((px >> 8) & 0xffu), b = (int32_t)((px >> 16) & 0xffu);
                yy[j] = jframe_clamp8(k.off + (yuv_dot(k.y, r, g, b, 1 << 15) >> 16));
                sr += r; sg += g; sb += b;
            }
            const uint32_t cb = jframe_clamp8(128 + (yuv_dot(k.cb, sr, sg, sb, 1 << 17) >> 18));
            const uint32_t cr = jframe_clamp8(128 + (yuv_dot(k.cr, sr, sg, sb, 1 << 17) >> 18));
            *(uint16_t*)(st + 2u * i) = (uint16_t)(yy[0] | (yy[1] << 8));
            *(uint16_t*)(st + 2u * T + 2u * i) = (uint16_t)(yy[2] | (yy[3] << 8));
            if (NV12) {
                *(uint16_t*)(st + 4u * T + 2u * i) = (uint16_t)(cb | (cr << 8));
            } else {
                st[4u * T + i] = (uint8_t)cb;
                st[5u * T + i] = (uint8_t)cr;
            }
        }
        __syncthreads();
        // 16-B chunk `q` of byte string `seg` (0, 1: luma rows; 2: chroma) -> its plane
        const uint32_t seg = threadIdx.x / kYuvChunks, q = threadIdx.x - seg * kYuvChunks;
        if (seg < 3u && (seg != 1u || two_rows)) {
            uint8_t* d;        // where byte 0 of the chunk goes
            uint32_t valid;    // bytes of the string (or of its half, I420 chroma) that lie inside the plane's row, from the chunk on
            if (seg < 2u) {
                d = pl.p[0] + (uint64_t)(y0 + seg) * pl.pitch[0] + 2u * s0 + 16u * q;
                valid = width - 2u * s0;
            } else if (NV12) {
                d = pl.p[1] + (uint64_t)pair * pl.pitch[1] + 2u * s0 + 16u * q;
                valid = 2u * (cw - s0);
            } else {
                const uint32_t half = q / (kYuvChunks / 2u), qq = q - half * (kYuvChunks / 2u);  // Cb, then Cr
                d = pl.p[1u + half] + (uint64_t)pair * pl.pitch[1u + half] + s0 + 16u * qq;
                valid = cw - s0;
                valid = valid > 16u * qq ? valid - 16u * qq : 0u;
            }
            if (seg < 2u || NV12) valid = valid > 16u * q ? valid - 16u * q : 0u;
            const uint8_t* from = st + 2u * T * seg + 16u * q;
            if (wide && valid >= 16u) {
                *(uint4*)d = *(const uint4*)from;
            } else {
                const uint32_t n = valid < 16u ? valid : 16u;
                for (uint32_t j = 0; j < n; j++) d[j] = from[j];
            }
        }
    }
}

}  // namespace

// Luma rows [row0, row1) (row0 even; row1 even or = height) of a width x height image at src (width * 8 bytes per row; null =
// all zero) and the chroma rows under them into planes[3] / pitches[3] (the third is unused for NV12).  layout, matrix, range,
// transfer: jh_yuv_layout, jh_yuv_matrix, jh_yuv_range, jh_yuv_transfer.  Returns 0, -1 on bad arguments, -2 on a launch error.
extern "C" int jh_blit_yuv_launch(hipStream_t stream, const void* src, void* const* planes, const uint64_t* pitches, uint32_t width,
                                  uint32_t height, uint32_t row0, uint32_t row1, int layout, int matrix, int range, int transfer,
                                  int num_cus) {
    if (jframe_yuv_enums_error(layout, matrix, range, transfer)) return -1;
    if ((row0 & 1u) || row1 > height || row1 < row0 || ((row1 & 1u) && row1 != height)) return -1;
    if (jframe_yuv_planes_error(layout, planes, pitches, width, JFRAME_NULL_PLANE | JFRAME_SHORT_PITCH)) return -1;
    const uint64_t cw = jframe_chroma_extent(width);
    YuvPlanes pl = {};
    uint32_t wide = 1u;
    for (int i = 0; i < jframe_yuv_planes(layout); i++) {
        pl.p[i] = (uint8_t*)planes[i];
        pl.pitch[i] = pitches[i];
        if (((uintptr_t)planes[i] | pitches[i]) & 15u) wide = 0u;
    }
    if (width == 0u || row1 == row0) return 0;
    const uint32_t pair0 = row0 / 2u, pair1 = (uint32_t)jframe_chroma_extent(row1);
    const uint64_t tiles_per_pair = (cw + kYuvTile - 1u) / kYuvTile;
    const uint64_t total = tiles_per_pair * (pair1 - pair0);
    if (total > 0x7fffffffull) return -1;
    YuvCoef k;
    const int* m = kYuvMatrix[matrix][range];
    for (int i = 0; i < 3; i++) { k.y[i] = m[i]; k.cb[i] = m[3 + i]; k.cr[i] = m[6 + i]; }
    k.off = kYuvOffset[range];
    const dim3 grid(grid_blocks(total, 1u, 8u, num_cus)), block(kYuvThreads);
    const uint2* s = (const uint2*)src;
    const uint32_t tpp = (uint32_t)tiles_per_pair, tt = (uint32_t)total;
    switch ((transfer == JH_YUV_TRANSFER_SRGB ? 2 : 0) + (layout == JH_YUV_I420 ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((k_blit_yuv<false, true>), grid, block, 0, stream, s, pl, k, width, height, pair0, tpp, tt, wide); break;
        case 1: hipLaunchKernelGGL((k_blit_yuv<false, false>), grid, block, 0, stream, s, pl, k, width, height, pair0, tpp, tt, wide); break;
        case 2: hipLaunchKernelGGL((k_blit_yuv<true, true>), grid, block, 0, stream, s, pl, k, width, height, pair0, tpp, tt, wide); break;
        default: hipLaunchKernelGGL((k_blit_yuv<true, false>), grid, block, 0, stream, s, pl, k, width, height, pair0, tpp, tt, wide); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
