// kernels_surface.hip -- jh_blit: the RGBA16F target (un-premultiplied, fine.wgsl:1092-1102) -> an 8-bit surface, the
// compute twin of the reference's blit pass (engine/wgpu_engine/lib.go:109-198: vec4(rgb * a, a) into the surface format).
// The conversion rule is in include/jello_hip.h and DESIGN.md ("Surface blit"); the hardware's float -> unorm / sRGB
// conversions are implementation-defined, so the project defines the answer itself:
//   p = c * a (f32, exact)   v = clamp(p, 0, 1) with NaN -> 0   unorm: rint_f32(v * 255)   sRGB: table of 255 thresholds.
// The per-pixel functions (blit_pixel and what it calls) live in blit_convert.h, which jh_blit_yuv (kernels_yuv.hip) shares.
// Streaming: 8 B read and 4 B written per pixel, nothing reused.  A lane converts four adjacent pixels (two 16-B loads -- or
// four 8-B loads when the source row is only 8-B aligned -- and one 16-B store); the first pixels of a row up to the
// destination's next 16-B boundary and the last width % 4 go through a one-pixel path, as does every pixel of a row whose
// destination is not 4-B aligned.  The destination bytes between 4 * width and the pitch are never touched.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_frame.h"
#include "blit_convert.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kBlitThreads = 256;

// Pixels of the row that go through the one-pixel path before the first four-pixel group (dst row not 16-B aligned yet);
// the whole row when its destination is not 4-B aligned.
__host__ __device__ __forceinline__ uint32_t blit_head(uintptr_t drow, uint32_t width) {
    if (drow & 3u) return width;
    const uint32_t h = (uint32_t)((16u - (drow & 15u)) & 15u) >> 2;
    return h < width ? h : width;
}

// A row is split into work items: [0, nvec) four-pixel groups, then the head pixels, then the tail pixels.  Blocks of
// kBlitThreads items, blocks_per_row per row, rows [row0, row0 + n_rows); the grid strides over them.
template <bool SRGB, bool BGRA>
__global__ __launch_bounds__(kBlitThreads) void k_blit(const uint2* __restrict__ src, uint8_t* __restrict__ dst, uint64_t pitch,
                                                       uint32_t width, uint32_t row0, uint32_t blocks_per_row, uint32_t total_blocks) {
    __shared__ float2 lut[SRGB ? 256 : 1];
    if (SRGB) {
        const uint32_t i = threadIdx.x;  // (kBlitThreads = 256 entries)
        blit_srgb_lut_fill(lut, i);
        __syncthreads();
    }
    for (uint32_t wb = blockIdx.x; wb < total_blocks; wb += gridDim.x) {
        const uint32_t r = wb / blocks_per_row;
        const uint32_t item = (wb - r * blocks_per_row) * kBlitThreads + threadIdx.x;
        const uint64_t y = (uint64_t)row0 + r;
        const uint2* srow = src ? src + y * width : nullptr;  // null: a never-written source reads as transparent black
        uint8_t* drow = dst + y * pitch;
        const uint32_t head = blit_head((uintptr_t)drow, width);
        const uint32_t nvec = (width - head) >> 2;
        const uint32_t n_one = width - 4u * nvec;  // head + tail
        if (item < nvec) {
            const uint32_t x = head + 4u * item;
            uint2 t0 = make_uint2(0u, 0u), t1 = t0, t2 = t0, t3 = t0;
            if (srow) {
                const uint2* s = srow + x;
                if (((uintptr_t)s & 15u) == 0u) {  // (the same for every group of the row)
                    const uint4 a = *(const uint4*)s, b = *(const uint4*)(s + 2);
                    t0 = make_uint2(a.x, a.y); t1 = make_uint2(a.z, a.w); t2 = make_uint2(b.x, b.y); t3 = make_uint2(b.z, b.w);
                } else {
                    t0 = s[0]; t1 = s[1]; t2 = s[2]; t3 = s[3];
                }
            }
            *(uint4*)(drow + 4u * (uint64_t)x) = make_uint4(blit_pixel<SRGB, BGRA>(t0, lut), blit_pixel<SRGB, BGRA>(t1, lut),
                                                            blit_pixel<SRGB, BGRA>(t2, lut), blit_pixel<SRGB, BGRA>(t3, lut));
        } else if (item < nvec + n_one) {
            const uint32_t j = item - nvec;
            const uint32_t x = j < head ? j : head + 4u * nvec + (j - head);
            const uint32_t o = blit_pixel<SRGB, BGRA>(srow ? srow[x] : make_uint2(0u, 0u), lut);
            uint8_t* d = drow + 4u * (uint64_t)x;
            if (((uintptr_t)d & 3u) == 0u) {
                *(uint32_t*)d = o;
            } else {
                d[0] = (uint8_t)o; d[1] = (uint8_t)(o >> 8); d[2] = (uint8_t)(o >> 16); d[3] = (uint8_t)(o >> 24);
            }
        }
    }
}

}  // namespace

// rows [row0, row1) of a width-wide image at src (width * 8 bytes per row; null = all zero) into dst (pitch bytes per row).
// format: jh_surface_format.  Returns 0, -1 on bad arguments, -2 on a launch error.
extern "C" int jh_blit_launch(hipStream_t stream, const void* src, void* dst, uint64_t pitch, uint32_t width, uint32_t row0,
                              uint32_t row1, int format, int num_cus) {
    if (!dst || !jframe_surface_format_ok(format) || jframe_surface_pitch_error(pitch, width) || row1 < row0) return -1;
    if (width == 0u || row1 == row0) return 0;
    // widest work list of any row: the head length depends on (dst + y * pitch) % 16, which repeats after at most 4 rows
    uint32_t items = 0u;
    for (uint32_t k = 0; k < 4u && row0 + k < row1; k++) {
        const uint32_t head = blit_head((uintptr_t)dst + (uint64_t)(row0 + k) * pitch, width);
        const uint32_t nvec = (width - head) >> 2;
        const uint32_t n = nvec + (width - 4u * nvec);
        items = n > items ? n : items;
    }
    const uint64_t blocks_per_row = (items + kBlitThreads - 1u) / kBlitThreads;
    const uint64_t total = blocks_per_row * (row1 - row0);
    if (total > 0x7fffffffull) return -1;
    const dim3 grid(grid_blocks(total, 1u, 8u, num_cus)), block(kBlitThreads);
    const uint2* s = (const uint2*)src;
    uint8_t* d = (uint8_t*)dst;
    const uint32_t bpr = (uint32_t)blocks_per_row, tb = (uint32_t)total;
    switch (format) {
        case JH_SURFACE_RGBA8_UNORM: hipLaunchKernelGGL((k_blit<false, false>), grid, block, 0, stream, s, d, pitch, width, row0, bpr, tb); break;
        case JH_SURFACE_BGRA8_UNORM: hipLaunchKernelGGL((k_blit<false, true>), grid, block, 0, stream, s, d, pitch, width, row0, bpr, tb); break;
        case JH_SURFACE_RGBA8_SRGB: hipLaunchKernelGGL((k_blit<true, false>), grid, block, 0, stream, s, d, pitch, width, row0, bpr, tb); break;
        default: hipLaunchKernelGGL((k_blit<true, true>), grid, block, 0, stream, s, d, pitch, width, row0, bpr, tb); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
