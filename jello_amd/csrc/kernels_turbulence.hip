// kernels_turbulence.hip -- jh_turbulence: feTurbulence noise GENERATED into an RGBA16F image, the device half of the rule in
// include/jello_hip.h ("Turbulence") and DESIGN.md 5.15; the host half -- the legal descriptor, the generator, the tables, the plan --
// and the pieces with cases (the cell / fraction split, the stitch step, the lattice walk, the s-curve, the dot, the lerp) are
// include/jello_turbulence.h.  There is no source image: per destination texel and octave two int64 positions, six selector reads,
// four corners' gradients and about 75 vector operations; the only memory traffic is the 8-byte store.
// One launch.  A workgroup of 256 lanes owns a TILE of the destination, 64 texels x 16 rows, laid on the destination image's 128-byte
// lines as kernels_lighting.hip lays its tiles, and walks its tiles by grid stride.  The tables (resident in a scratch slot of the
// context, 8.25 KB, the gradients [lattice value][channel][2]: one corner's four channels are 32 contiguous bytes) are copied into LDS
// once per workgroup; there the two 16-byte halves of an entry sit in two arrays, GA[256] and GB[256], so that a corner is still two
// ds_read_b128 but the lattice values of a 16-lane group spread over all 16 slots of a bank row, not over the 8 even or the 8 odd ones
// (measured: 8 octaves 8-12 % faster than with the entries contiguous, 1 octave the same); then the selector, 256
// bytes, read with ds_read_u8.
// A wave owns 4 rows of the tile and a lane a vertical strip of them, 4 outputs of one column: what depends on x only -- the position,
// the cell, the fraction, the stitch step, sx and the two first-level selector reads -- is computed once per octave for four texels;
// what depends on y only is the same in every lane of the wave.  The octave count is a scalar loop bound (the position, the stitch
// pair and the ratio double or halve from octave to octave, which is p << k, wrap << k and 2^-k exactly: nothing overflows inside
// the legal range).  k_turb<KIND, STITCH> has 4 instantiations, 62 VGPRs without stitch and 63 with, none with scratch or spills: 8
// waves to a SIMD, so 8 workgroups to a CU (66 KB of its LDS) are launched and the rest of the tiles is walked by grid stride.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_turbulence.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTileW = 64, kTileH = 16, kStrip = kTileH / kWaves;  // a lane's strip: 4 rows of one column
constexpr uint32_t kLine = 16;                                                                      // texels of a 128-byte line
constexpr uint32_t kBlobVec = JTURB_DEVICE_BYTES / 16u;                                             // the tables, 16-byte units
constexpr uint32_t kEntries = 256;                                                                  // lattice values
constexpr uint32_t kPerCu = 8;                                                                      // workgroups to a CU: 62-63 VGPRs, 8 waves to a SIMD

struct TurbArgs {
    uint2* dst;               // the destination image
    uint32_t width, height;   // its texels per row and rows
    uint32_t dx, dy, dw, dh;  // the rectangle that is written
    uint32_t tiles_x, total;
    uint32_t octaves;
    int32_t wrap[2], extent[2];  // the stitch pair of octave 0, per axis
    int64_t start[2], step[2];   // the plan's positions
    const uint4* tables;         // device, JTURB_DEVICE_BYTES
};

template <int KIND, bool STITCH>
__global__ __launch_bounds__(kThreads) void k_turb(const TurbArgs a) {
    __shared__ uint4 lds[kBlobVec];
    // (unit i < 512 of the tables is half i & 1 of lattice value i >> 1: the first halves go to GA, the second to GB, the selector stays)
    for (uint32_t i = threadIdx.x; i < kBlobVec; i += kThreads) lds[i < 2u * kEntries ? ((i & 1u) * kEntries + (i >> 1)) : i] = a.tables[i];
    __syncthreads();
    const float4* GA = (const float4*)lds;  // GA[b]: (r.x, r.y, g.x, g.y), GB[b]: (b.x, b.y, a.x, a.y) of lattice value b
    const float4* GB = GA + kEntries;
    const uint8_t* P = (const uint8_t*)(lds + JTURB_GRADIENT_FLOATS / 4u);
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
        int64_t px = a.start[0] + (int64_t)X * a.step[0];
        int64_t py[kStrip];
#pragma unroll
        for (uint32_t j = 0; j < kStrip; j++) {
            const uint32_t row = r0 + j < a.dh ? r0 + j : a.dh - 1u;  // (a row past the rectangle repeats its last one and is not stored)
            py[j] = a.start[1] + (int64_t)(a.dy + row) * a.step[1];
        }
        float sum[kStrip][4];
#pragma unroll
        for (uint32_t j = 0; j < kStrip; j++)
#pragma unroll
            for (uint32_t ch = 0; ch < 4u; ch++) sum[j][ch] = 0.0f;
        float ratio = 1.0f;
        int32_t wrap_x = a.wrap[0], wrap_y = a.wrap[1], ext_x = a.extent[0], ext_y = a.extent[1];
        for (uint32_t k = 0; k < a.octaves; k++) {
            int32_t ix;
            float rx0;
            jturb_split(px, &ix, &rx0);
            const uint32_t bx0 = STITCH ? jturb_stitch(ix, wrap_x, ext_x) : (uint32_t)ix;
            const uint32_t bx1 = STITCH ? jturb_stitch(ix + 1, wrap_x, ext_x) : (uint32_t)ix + 1u;
            uint32_t pi, pj;
            jturb_lattice_x(P, bx0, bx1, &pi, &pj);
            const float sx = jturb_s(rx0), rx1 = rx0 - 1.0f;
#pragma unroll
            for (uint32_t j = 0; j < kStrip; j++) {
                int32_t iy;
                float ry0;
                jturb_split(py[j], &iy, &ry0);
                const uint32_t by0 = STITCH ? jturb_stitch(iy, wrap_y, ext_y) : (uint32_t)iy;
                const uint32_t by1 = STITCH ? jturb_stitch(iy + 1, wrap_y, ext_y) : (uint32_t)iy + 1u;
                uint32_t b[4];
                jturb_lattice_y(P, pi, pj, by0 & 255u, by1 & 255u, b);
                const float sy = jturb_s(ry0), ry1 = ry0 - 1.0f;
                const float4 g00a = GA[b[0]], g00b = GB[b[0]], g10a = GA[b[1]], g10b = GB[b[1]];
                const float4 g01a = GA[b[2]], g01b = GB[b[2]], g11a = GA[b[3]], g11b = GB[b[3]];
                const float gx[4][4] = {{g00a.x, g10a.x, g01a.x, g11a.x}, {g00a.z, g10a.z, g01a.z, g11a.z}, {g00b.x, g10b.x, g01b.x, g11b.x}, {g00b.z, g10b.z, g01b.z, g11b.z}};
                const float gy[4][4] = {{g00a.y, g10a.y, g01a.y, g11a.y}, {g00a.w, g10a.w, g01a.w, g11a.w}, {g00b.y, g10b.y, g01b.y, g11b.y}, {g00b.w, g10b.w, g01b.w, g11b.w}};
#pragma unroll
                for (uint32_t ch = 0; ch < 4u; ch++) {
                    const float u00 = jturb_dot(rx0, ry0, gx[ch][0], gy[ch][0]), u10 = jturb_dot(rx1, ry0, gx[ch][1], gy[ch][1]);
                    const float u01 = jturb_dot(rx0, ry1, gx[ch][2], gy[ch][2]), u11 = jturb_dot(rx1, ry1, gx[ch][3], gy[ch][3]);
                    const float n = jturb_lerp(sy, jturb_lerp(sx, u00, u10), jturb_lerp(sx, u01, u11));
                    sum[j][ch] = __builtin_fmaf(KIND == JTURB_TURBULENCE ? __builtin_fabsf(n) : n, ratio, sum[j][ch]);
                }
                py[j] += py[j];  // (the spare bit of the legal range: the doubling after the last octave still fits)
            }
            px += px;
            ratio *= 0.5f;
            if (STITCH) {  // (modulo 2^32: the doubling after the last octave may leave the legal range, and is not used)
                wrap_x = (int32_t)((uint32_t)wrap_x << 1); wrap_y = (int32_t)((uint32_t)wrap_y << 1);
                ext_x = (int32_t)((uint32_t)ext_x << 1); ext_y = (int32_t)((uint32_t)ext_y << 1);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kStrip; j++) {
            if (r0 + j >= a.dh) break;
            const uint32_t Y = a.dy + r0 + j;
            a.dst[(uint64_t)Y * a.width + X] =
                texel_pack(make_float4(jturb_result(KIND, sum[j][0]), jturb_result(KIND, sum[j][1]), jturb_result(KIND, sum[j][2]), jturb_result(KIND, sum[j][3])));
        }
    }
}

}  // namespace

// The rectangle r of the RGBA16F image dst = the turbulence of the rule: `kind`, `octaves`, the plan of the descriptor (its positions
// and, where plan->stitched, its stitch pair); tables: device memory, JTURB_DEVICE_BYTES as jturb_device_tables lays them out, 16-byte
// aligned.  One launch on `stream`, 8.25 KB of LDS.  Returns 0, -1 on arguments it refuses (an image beyond the plan's max_extent
// among them), -2 on a launch error.
extern "C" int jh_turbulence_launch(hipStream_t stream, jimage_dst dst, jimage_rect r, int kind, uint32_t octaves, const jh_turb_plan* plan, const void* tables,
                                    int num_cus) {
    if (!dst.texels || !plan || !tables || ((uintptr_t)tables & 15u) != 0u) return -1;
    if (kind < 0 || kind >= JTURB_KINDS || octaves > JTURB_MAX_OCTAVES) return -1;
    if (dst.width > plan->max_extent[0] || dst.height > plan->max_extent[1]) return -1;
    if (!jimage_rect_inside(r, dst.width, dst.height) || jimage_rect_empty(r)) return -1;
    const uint64_t tiles_x = ((uint64_t)r.w + (kLine - 1u) + (kTileW - 1u)) / kTileW;  // (+ 15: the grid of lines may start up to 15 texels before the row)
    const uint64_t total = tiles_x * (((uint64_t)r.h + kTileH - 1u) / kTileH);
    if (total > 0x7fffffffu) return -1;
    TurbArgs a;
    a.dst = (uint2*)dst.texels;
    a.width = dst.width; a.height = dst.height;
    a.dx = r.x; a.dy = r.y; a.dw = r.w; a.dh = r.h;
    a.tiles_x = (uint32_t)tiles_x;
    a.total = (uint32_t)total;
    a.octaves = octaves;
    for (uint32_t k = 0; k < 2u; k++) {
        a.wrap[k] = plan->wrap[k]; a.extent[k] = plan->width[k];
        a.start[k] = plan->start[k]; a.step[k] = plan->step[k];
    }
    a.tables = (const uint4*)tables;
    const dim3 grid(grid_blocks(total * kWaves, kWaves, kPerCu, num_cus));
    const bool stitch = plan->stitched != 0u;
    if (kind == JTURB_FRACTAL_NOISE) with_flag(stitch, [&](auto s) { hipLaunchKernelGGL((k_turb<JTURB_FRACTAL_NOISE, decltype(s)::value>), grid, dim3(kThreads), 0, stream, a); });
    else with_flag(stitch, [&](auto s) { hipLaunchKernelGGL((k_turb<JTURB_TURBULENCE, decltype(s)::value>), grid, dim3(kThreads), 0, stream, a); });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
