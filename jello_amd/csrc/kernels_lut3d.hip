// kernels_lut3d.hip -- jh_lut3d: a 3D colour lookup table, itself an RGBA16F image, applied to an RGBA16F image by tetrahedral
// interpolation; the device half of the rule in include/jello_hip.h ("3D LUT") and DESIGN.md 5.23.  The position, the walk and the
// sum are include/jello_lut3d.h's, the text the host compiles too.
// Streaming with four gathers per texel: 8 B in and 8 B out, the pair walk of texel_io.h without a backdrop as in kernels_color.hip
// -- a lane two neighbouring texels of a dst row, 16-byte accesses where a pair allows, a work item a row segment of 512 texels = one
// workgroup of 256 lanes, the grid bounded per CU and strided.  Per texel a lane computes three positions and the order of the walk
// with compare and select (no branch on the fractions), reads the four entries of its tetrahedron, 8 bytes each, and sums.  The two
// texels of a lane are independent, so its eight entry loads are in flight together.
// The table's base and its size are kernel arguments: they sit in scalar registers; a null table (never written) reads as zeros.
// Two instantiations: STAGED = false gathers from global memory (33^3 entries are 287 KB, 65^3 2.2 MB: the L2's); STAGED = true, for
// N <= 17, copies the table densely into LDS once per workgroup (at most 39 304 B = 31 blocks of 1 280: four workgroups to a CU) with
// 16-byte loads, and the gathers are 8-byte LDS reads.  Dense: entry e at byte 8 e, so the 64 banks of an 8-byte read see e mod 32;
// the entries of a tetrahedron differ by 1, N and N^2, and neighbouring texels' by what the content gives -- no padding helps a gather.
// src may be dst, and the table may be src; it is never dst.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "jello_lut3d.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kLutThreads = 256;
constexpr uint32_t kLutStagedEntries = JLUT_STAGED_MAX_SIZE * JLUT_STAGED_MAX_SIZE * JLUT_STAGED_MAX_SIZE;
constexpr uint32_t kLutFillTrips = (kLutStagedEntries / 2u + kLutThreads - 1u) / kLutThreads;  // 16-byte units of the largest staged table per lane: 10

JD uint2 lut_texel(uint2 s, const uint2* table, uint32_t n) {
    uint32_t index[4], vx[4], vy[4];
    float w[4];
    jlut_vertices(s.x, s.y, n, index, w);
    for (int i = 0; i < 4; i++) {
        const uint2 e = table[index[i]];
        vx[i] = e.x;
        vy[i] = e.y;
    }
    uint2 o;
    jlut_sum(w, vx, vy, s.y, &o.x, &o.y);
    return o;
}

// The w x h texels at (x, y) of src (src_w texels per row; null: transparent black) through the table lut of n^3 entries (null:
// zeros) into the same rectangle of dst (dst_w per row).  item = row * segs + seg.  STAGED: n^3 * 8 bytes of dynamic LDS.
template <bool STAGED>
__global__ __launch_bounds__(kLutThreads) void k_lut3d(const uint2* src, uint32_t src_w, uint2* dst, uint32_t dst_w, uint32_t x, uint32_t y, uint32_t w,
                                                       uint32_t segs, uint32_t total_items, const uint2* lut, uint32_t n) {
    if (!lut) {  // every entry is zero: the colour is +0 (the weights are finite and not negative), alpha the source's
        pair_walk<kLutThreads, false>(src, src_w, x, y, dst, dst_w, x, y, w, 0u, segs, total_items, [&](uint2 s, uint2) { return make_uint2(0u, s.y & 0xffff0000u); });
        return;
    }
    if (STAGED) {
        extern __shared__ uint4 staged[];  // n^3 entries of 8 bytes, dense
        const uint32_t entries = n * n * n, quads = entries >> 1;
        // All of a lane's loads first, then its writes: one round trip to memory, not one per trip.  No branch in either loop (the
        // compiler sinks a load into a branch that alone uses it): a trip past the end copies unit 0 onto unit 0 once more.
        uint4 q[kLutFillTrips];
#pragma unroll
        for (uint32_t j = 0; j < kLutFillTrips; j++) {
            const uint32_t i = threadIdx.x + j * kLutThreads;
            q[j] = ((const uint4*)lut)[i < quads ? i : 0u];  // (an image's texels start on 16 bytes)
        }
#pragma unroll
        for (uint32_t j = 0; j < kLutFillTrips; j++) {
            const uint32_t i = threadIdx.x + j * kLutThreads;
            staged[i < quads ? i : 0u] = q[j];
        }
        if ((entries & 1u) && threadIdx.x == 0u) ((uint2*)staged)[entries - 1u] = lut[entries - 1u];
        __syncthreads();
        const uint2* table = (const uint2*)staged;
        pair_walk<kLutThreads, false>(src, src_w, x, y, dst, dst_w, x, y, w, 0u, segs, total_items, [&](uint2 s, uint2) { return lut_texel(s, table, n); });
    } else {
        pair_walk<kLutThreads, false>(src, src_w, x, y, dst, dst_w, x, y, w, 0u, segs, total_items, [&](uint2 s, uint2) { return lut_texel(s, lut, n); });
    }
}

}  // namespace

// The rule on the rectangle r of the RGBA16F image src (null texels: transparent black; may be dst), written to the same rectangle
// of the image dst, through the table lut: n^3 entries of 8 bytes, entry (i, j, k) at i + n (j + n k), on a 16-byte boundary (null:
// zeros; may be src's texels, never dst's).  variant: 0 the launcher's choice (STAGED for n <= JLUT_STAGED_MAX_SIZE), 1 never
// STAGED, 2 STAGED (refused above the limit).  One launch on `stream`, none for an empty rectangle.  Returns 0, -1 on arguments it
// refuses, -2 on a launch error.
extern "C" int jh_lut3d_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect r, const void* lut, uint32_t n, int variant, int num_cus) {
    if (!dst.texels || n < JLUT_MIN_SIZE || n > JLUT_MAX_SIZE || ((uintptr_t)lut & 15u) || variant < 0 || variant > 2) return -1;
    if (variant == 2 && n > JLUT_STAGED_MAX_SIZE) return -1;
    if (!jimage_rect_inside(r, src.width, src.height) || !jimage_rect_inside(r, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(r)) return 0;
    const uint64_t segs = walk_segs(r.w, kLutThreads), total = segs * r.h;
    if (total > 0x7fffffffull) return -1;
    const bool staged = lut && variant != 1 && n <= JLUT_STAGED_MAX_SIZE;
    // (STAGED: a CU holds four workgroups, and each pays the copy once, so no more are launched than are resident)
    const dim3 grid(grid_blocks(total, 1u, staged ? 4u : 8u, num_cus)), block(kLutThreads);
    const uint32_t lds = staged ? n * n * n * 8u : 0u;
    with_flag(staged, [&](auto st) {
        hipLaunchKernelGGL(k_lut3d<decltype(st)::value>, grid, block, lds, stream, (const uint2*)src.texels, src.width, (uint2*)dst.texels, dst.width, r.x, r.y, r.w,
                           (uint32_t)segs, (uint32_t)total, (const uint2*)lut, n);
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
