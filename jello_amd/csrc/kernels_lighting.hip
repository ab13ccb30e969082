// kernels_lighting.hip -- jh_lighting: feDiffuseLighting and feSpecularLighting on an RGBA16F image, the device half of the rule in
// include/jello_hip.h ("Lighting") and DESIGN.md 5.14; the host half -- the legal descriptor, the plan, the tables -- and the normal's
// cases are include/jello_lighting.h.  Per destination texel (X, Y) of the rectangle: the surface normal from the 3 x 3 neighbourhood of
// src's alpha (jlight_normal: the specification's nine cases), the light vector, the light's colour, then the diffuse or the specular
// term -- 8 bytes read and 8 written per texel, and between them 2-3 square roots, 4-5 IEEE divisions and up to two table powers.
// One launch.  A workgroup of 256 lanes owns a TILE of the destination, 64 texels x 16 rows, laid on the destination image's 128-byte
// lines as kernels_convolve.hip lays its tiles, and stages the alpha of the tile with a halo of 1 -- 66 x 18 binary32, 4.7 KB -- into
// LDS once, the indices clamped to the IMAGE while staging (which side sums exist is decided per texel, from X and Y alone).  A wave
// owns 4 rows of the tile and a lane a vertical strip of them, 4 outputs of one column: 18 ds_read_b32 for 4 outputs, neighbouring
// lanes on neighbouring banks.  The power tables (4097 binary32 each, resident in a scratch slot of the context) are copied into LDS
// once per workgroup, which then walks its tiles by grid stride: only as many workgroups to a CU are launched as its 160 KB of LDS hold
// at once -- 7 with one table, 4 with both, 8 without (measured: 4 with one table took 15-19 us longer at 4096^2, for want of waves) --
// so the copy (16 loads per lane and table) is spread over every tile the workgroup walks; a lookup is two neighbouring ds_read_b32 at
// a data-dependent address.  k_light<KIND, LIGHT, TABLES> has 12 instantiations, TABLES the bits of the tables in use; none has scratch.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_lighting.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = 4, kTileW = 64, kTileH = 16, kStrip = kTileH / kWaves;  // a lane's strip: 4 rows of one column
constexpr uint32_t kLine = 16;                                                                      // texels of a 128-byte line
constexpr uint32_t kFootW = kTileW + 2u, kFootH = kTileH + 2u, kFoot = (kFootW * kFootH + 3u) & ~3u;  // the staged alpha, floats (a multiple of 4)
constexpr uint32_t kTable = (JLIGHT_ENTRIES + 3u) & ~3u;                                            // a table's floats in LDS

struct LightArgs {
    const uint2* src;  // the source image (null: never written, alpha +0)
    uint2* dst;        // the destination image, of the same size
    uint32_t width, height;   // texels per row and rows of both images
    uint32_t dx, dy, dw, dh;  // the rectangle that is written
    uint32_t tiles_x, total;
    float s[6];  // the plan: s[span - 1][wsum - 2]
    float ldir[3], p[3], sdir[3], cone;
    float surface_scale, constant;
    float color[3];
    const float* spec_table;  // device, JLIGHT_ENTRIES each (null where TABLES has no bit for it)
    const float* spot_table;
};

// Pw(t, e != 1) of a table in LDS, t in [0, 1].
JD float table_power(const float* T, float t) {
    float f;
    const int i = jlight_segment(t, &f);
    const float lo = T[i], hi = T[i + 1];
    return __builtin_fmaf(f, hi - lo, lo);
}

template <int KIND, int LIGHT, int TABLES>
__global__ __launch_bounds__(kThreads) void k_light(const LightArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* foot = lds;  // row-major, kFootW to a row: (fx, fy) is the alpha at the image position clamp(X0 + fx), clamp(Y0 + fy)
    const float* tspec = lds + kFoot;
    const float* tspot = lds + kFoot + ((TABLES & (int)JLIGHT_TABLE_SPEC) ? kTable : 0u);
    if (TABLES & (int)JLIGHT_TABLE_SPEC)
        for (uint32_t i = threadIdx.x; i < JLIGHT_ENTRIES; i += kThreads) lds[kFoot + i] = a.spec_table[i];
    if (TABLES & (int)JLIGHT_TABLE_SPOT)
        for (uint32_t i = threadIdx.x; i < JLIGHT_ENTRIES; i += kThreads) lds[kFoot + ((TABLES & (int)JLIGHT_TABLE_SPEC) ? kTable : 0u) + i] = a.spot_table[i];
    const uint32_t lane = threadIdx.x & (kTileW - 1u), wave = threadIdx.x >> 6;
    const uint16_t* alpha = (const uint16_t*)a.src;  // a texel's alpha: its fourth f16
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t trow = it / a.tiles_x, tcol = it - trow * a.tiles_x;
        const uint32_t row0 = trow * kTileH;  // the tile's first row of the rectangle
        const uint32_t phase = (uint32_t)((((uintptr_t)a.dst >> 3) + (uint64_t)(a.dy + row0) * a.width + a.dx) & (kLine - 1u));
        const int32_t col0 = (int32_t)(tcol * kTileW) - (int32_t)phase;  // the tile's first column of the rectangle (may lie before it)
        const int32_t X0 = (int32_t)a.dx + col0 - 1, Y0 = (int32_t)(a.dy + row0) - 1;
        for (uint32_t k = threadIdx.x; k < kFootW * kFootH; k += kThreads) {
            const uint32_t fy = k / kFootW, fx = k - fy * kFootW;
            const uint32_t ix = (uint32_t)jd::iclamp_(X0 + (int32_t)fx, 0, (int32_t)a.width - 1), iy = (uint32_t)jd::iclamp_(Y0 + (int32_t)fy, 0, (int32_t)a.height - 1);
            foot[k] = alpha ? jd::f16_to_f32(alpha[((uint64_t)iy * a.width + ix) * 4u + 3u]) : 0.0f;
        }
        __syncthreads();  // (the first one also covers the tables)
        const uint32_t r0 = row0 + wave * kStrip;  // the strip's first row of the rectangle
        const int32_t c = col0 + (int32_t)lane;    // the lane's column of the rectangle
        if (r0 < a.dh && c >= 0 && c < (int32_t)a.dw) {
            const uint32_t X = a.dx + (uint32_t)c;
            const float* strip = foot + (wave * kStrip) * kFootW + lane;  // the neighbourhood's first row and column of the strip's first output
            float col[kStrip + 2u][3];
#pragma unroll
            for (uint32_t j = 0; j < kStrip + 2u; j++)
#pragma unroll
                for (uint32_t i = 0; i < 3u; i++) col[j][i] = strip[j * kFootW + i];
            const float xc = (float)X + 0.5f;
#pragma unroll
            for (uint32_t k = 0; k < kStrip; k++) {
                if (r0 + k >= a.dh) break;
                const uint32_t Y = a.dy + r0 + k;
                const float nb[3][3] = {{col[k][0], col[k][1], col[k][2]}, {col[k + 1u][0], col[k + 1u][1], col[k + 1u][2]}, {col[k + 2u][0], col[k + 2u][1], col[k + 2u][2]}};
                float nx, ny;
                jlight_normal(a.s, X, Y, a.width, a.height, nb, &nx, &ny);
                const float nlen = jd::sqrt_(__builtin_fmaf(nx, nx, __builtin_fmaf(ny, ny, 1.0f)));
                float lx = a.ldir[0], ly = a.ldir[1], lz = a.ldir[2];
                if (LIGHT != JLIGHT_DISTANT) {
                    const float Z = a.surface_scale * nb[1][1];
                    const float vx = a.p[0] - xc, vy = a.p[1] - ((float)Y + 0.5f), vz = a.p[2] - Z;
                    const float len = jd::sqrt_(__builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx)));
                    lx = vx / len; ly = vy / len; lz = vz / len;
                }
                float cr = a.color[0], cg = a.color[1], cb = a.color[2];
                if (LIGHT == JLIGHT_SPOT) {
                    const float m = -__builtin_fmaf(lz, a.sdir[2], __builtin_fmaf(ly, a.sdir[1], lx * a.sdir[0]));
                    const bool lit = m > 0.0f && m >= a.cone;
                    const float t = lit ? jd::fmin_(m, 1.0f) : 0.0f;  // (in [0, 1] whatever m is: the table is indexed with it)
                    const float pw = (TABLES & (int)JLIGHT_TABLE_SPOT) ? table_power(tspot, t) : t;
                    cr = lit ? cr * pw : 0.0f; cg = lit ? cg * pw : 0.0f; cb = lit ? cb * pw : 0.0f;
                }
                uint2 out;
                if (KIND == JLIGHT_DIFFUSE) {
                    const float t = jd::fmax_(__builtin_fmaf(nx, lx, __builtin_fmaf(ny, ly, lz)) / nlen, 0.0f);
                    const float kt = a.constant * t;
                    out = texel_pack(make_float4(jd::fmin_(kt * cr, 1.0f), jd::fmin_(kt * cg, 1.0f), jd::fmin_(kt * cb, 1.0f), 1.0f));
                } else {
                    const float hz = lz + 1.0f;
                    const float hlen = jd::sqrt_(__builtin_fmaf(hz, hz, __builtin_fmaf(ly, ly, lx * lx)));
                    const float q = __builtin_fmaf(nx, lx, __builtin_fmaf(ny, ly, hz)) / (nlen * hlen);
                    const float t0 = jd::fmin_(jd::fmax_(q, 0.0f), 1.0f);
                    const float t = (TABLES & (int)JLIGHT_TABLE_SPEC) ? table_power(tspec, t0) : t0;
                    const float kt = a.constant * t;
                    const float vr = jd::fmin_(kt * cr, 1.0f), vg = jd::fmin_(kt * cg, 1.0f), vb = jd::fmin_(kt * cb, 1.0f);
                    out = texel_unpremultiply(make_float4(vr, vg, vb, jd::fmax_(jd::fmax_(vr, vg), vb)));
                }
                a.dst[(uint64_t)Y * a.width + X] = out;
            }
        }
        __syncthreads();  // the next tile's staging overwrites the alpha
    }
}

template <int KIND, int LIGHT>
void launch_tables(hipStream_t stream, dim3 grid, uint32_t lds, uint32_t tables, const LightArgs& a) {
    // (the tables a kind and a light can have: SPEC under SPECULAR, SPOT under SPOT)
    constexpr int kSpec = KIND == JLIGHT_SPECULAR ? (int)JLIGHT_TABLE_SPEC : 0, kSpot = LIGHT == JLIGHT_SPOT ? (int)JLIGHT_TABLE_SPOT : 0;
    if (tables == (uint32_t)(kSpec | kSpot)) hipLaunchKernelGGL((k_light<KIND, LIGHT, kSpec | kSpot>), grid, dim3(kThreads), lds, stream, a);
    else if (tables == (uint32_t)kSpec) hipLaunchKernelGGL((k_light<KIND, LIGHT, kSpec>), grid, dim3(kThreads), lds, stream, a);
    else if (tables == (uint32_t)kSpot) hipLaunchKernelGGL((k_light<KIND, LIGHT, kSpot>), grid, dim3(kThreads), lds, stream, a);
    else hipLaunchKernelGGL((k_light<KIND, LIGHT, 0>), grid, dim3(kThreads), lds, stream, a);
}
template <int KIND>
void launch_light(hipStream_t stream, dim3 grid, uint32_t lds, int light, uint32_t tables, const LightArgs& a) {
    switch (light) {
        case JLIGHT_DISTANT: launch_tables<KIND, JLIGHT_DISTANT>(stream, grid, lds, tables, a); break;
        case JLIGHT_POINT: launch_tables<KIND, JLIGHT_POINT>(stream, grid, lds, tables, a); break;
        default: launch_tables<KIND, JLIGHT_SPOT>(stream, grid, lds, tables, a); break;
    }
}

}  // namespace

// The rectangle r of the RGBA16F image dst = the lighting of the alpha of the image src (null texels: alpha +0; another image of the same
// size) by the rule: `kind`, `light`, the plan of the descriptor, surface_scale, constant and color (3 binary32) as the descriptor has
// them; spec_table / spot_table: device memory, JLIGHT_ENTRIES binary32 each, null where the exponent is 1 or is not in use -- which
// selects the instantiation.  One launch on `stream`, 4.7 KB of LDS plus 16.4 KB per table.  Returns 0, -1 on arguments it refuses
// (an extent above 2^23 among them), -2 on a launch error.
extern "C" int jh_lighting_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect r, int kind, int light, const jh_light_plan* plan,
                                  float surface_scale, float constant, const float* color, const float* spec_table, const float* spot_table, int num_cus) {
    if (!dst.texels || !plan || !color || src.texels == dst.texels || src.width != dst.width || src.height != dst.height) return -1;
    if (kind < 0 || kind >= JLIGHT_KINDS || light < 0 || light >= JLIGHT_LIGHTS) return -1;
    if ((spec_table && kind != JLIGHT_SPECULAR) || (spot_table && light != JLIGHT_SPOT)) return -1;
    if (dst.width > JLIGHT_MAX_EXTENT || dst.height > JLIGHT_MAX_EXTENT) return -1;
    if (!jimage_rect_inside(r, dst.width, dst.height) || jimage_rect_empty(r)) return -1;
    const uint64_t tiles_x = ((uint64_t)r.w + (kLine - 1u) + (kTileW - 1u)) / kTileW;  // (+ 15: the grid of lines may start up to 15 texels before the row)
    const uint64_t total = tiles_x * (((uint64_t)r.h + kTileH - 1u) / kTileH);
    if (total > 0x7fffffffu) return -1;
    LightArgs a;
    a.src = (const uint2*)src.texels;
    a.dst = (uint2*)dst.texels;
    a.width = dst.width; a.height = dst.height;
    a.dx = r.x; a.dy = r.y; a.dw = r.w; a.dh = r.h;
    a.tiles_x = (uint32_t)tiles_x;
    a.total = (uint32_t)total;
    for (uint32_t k = 0; k < 6u; k++) a.s[k] = (&plan->s[0][0])[k];
    for (uint32_t k = 0; k < 3u; k++) { a.ldir[k] = plan->ldir[k]; a.p[k] = plan->p[k]; a.sdir[k] = plan->sdir[k]; a.color[k] = color[k]; }
    a.cone = plan->cone;
    a.surface_scale = surface_scale;
    a.constant = constant;
    a.spec_table = spec_table;
    a.spot_table = spot_table;
    const uint32_t tables = (spec_table ? JLIGHT_TABLE_SPEC : 0u) | (spot_table ? JLIGHT_TABLE_SPOT : 0u);
    const uint32_t lds = (kFoot + ((spec_table ? kTable : 0u) + (spot_table ? kTable : 0u))) * (uint32_t)sizeof(float);
    const uint32_t per_cu = tables == (JLIGHT_TABLE_SPEC | JLIGHT_TABLE_SPOT) ? 4u : (tables ? 7u : 8u);  // what 160 KB of LDS hold at once
    const dim3 grid(grid_blocks(total * kWaves, kWaves, per_cu, num_cus));
    if (kind == JLIGHT_DIFFUSE) launch_light<JLIGHT_DIFFUSE>(stream, grid, lds, light, tables, a);
    else launch_light<JLIGHT_SPECULAR>(stream, grid, lds, light, tables, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
