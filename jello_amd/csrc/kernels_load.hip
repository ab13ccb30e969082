// kernels_load.hip -- jh_load_surface and jh_load_yuv: 8-bit surfaces and planar 8-bit Y'CbCr 4:2:0 frames INTO a rectangle of an
// RGBA16F image, the inverses of kernels_surface.hip and kernels_yuv.hip.  The rule is include/jello_load.h (DESIGN.md 5.21 "Load
// rule"); tests/load_ref.py restates it in numpy.
// Streaming: 4 B (surface) or 1.5 B (YUV) read and 8 B written per texel, nothing reused.  Both kernels walk the destination as
// pair_walk (texel_io.h) does: a work item is a row segment of 2 * kLoadThreads texels, a lane owns two neighbouring texels laid on
// the destination row's 16-byte grid, so a pair inside the row is ONE 16-byte store and adjacent lanes write adjacent 16 bytes; a
// row's first or last texel alone is an 8-byte store.  The 256-entry decode tables a kernel needs are copied into LDS by the
// workgroup (512 B per f16 table, 1 KB per binary32 table), so a channel is one ds_read.  The source bytes are read straight from
// memory: a pair of surface pixels as one 8-byte load where the row allows, the luma and chroma bytes of a pair one by one (every
// byte a lane reads lies in a cache line its neighbours read too).  Texels outside the rectangle and source bytes between a row's
// end and its pitch are never touched.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_load.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kLoadThreads = 256;

// The lane's texels c, c + 1 of the rectangle's row for work item `it` (row-major segments), or false when neither lies in the row.
struct LoadPair {
    uint32_t row;
    int64_t c;
    bool va, vb;
    uint2* drow;
};
__device__ __forceinline__ bool load_pair(uint32_t it, uint32_t segs, uint2* dst, uint32_t dst_w, uint32_t dx, uint32_t dy, uint32_t w, LoadPair* p) {
    p->row = it / segs;
    const uint32_t seg = it - p->row * segs;
    p->drow = dst + ((uint64_t)(dy + p->row) * dst_w + dx);
    const uint32_t phase = (uint32_t)(((uintptr_t)p->drow >> 3) & 1u);
    p->c = (int64_t)seg * (2u * kLoadThreads) + 2u * threadIdx.x - phase;
    p->va = p->c >= 0 && p->c < (int64_t)w;
    p->vb = p->c + 1 < (int64_t)w;
    return p->va || p->vb;
}
__device__ __forceinline__ void store_pair(const LoadPair& p, uint2 ta, uint2 tb) {
    if (p.va && p.vb) *(uint4*)(p.drow + p.c) = make_uint4(ta.x, ta.y, tb.x, tb.y);
    else if (p.va) p.drow[p.c] = ta;
    else p.drow[p.c + 1] = tb;
}

// ---- surface ----

// One pixel's four bytes, as a word, from any address.
__device__ __forceinline__ uint32_t load_px_bytes(const uint8_t* s) {
    return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
}

// ALPHA: JH_LOAD_ALPHA_*.  STRAIGHT and OPAQUE look every channel up in f16 tables; PREMULTIPLIED takes the binary32 values from
// tables of its own through the store rule.
template <bool SRGB, int ALPHA>
__global__ __launch_bounds__(kLoadThreads) void k_load_surface(const uint8_t* __restrict__ src, uint64_t pitch, uint2* __restrict__ dst, uint32_t dst_w,
                                                               uint32_t dx, uint32_t dy, uint32_t w, uint32_t bgra, uint32_t segs, uint32_t total_items) {
    constexpr bool PREMUL = ALPHA == JH_LOAD_ALPHA_PREMULTIPLIED;
    __shared__ uint16_t colour16[PREMUL ? 1 : 256];
    __shared__ uint16_t unorm16[(PREMUL || ALPHA == JH_LOAD_ALPHA_OPAQUE || !SRGB) ? 1 : 256];  // (STRAIGHT's alpha, where colour16 is not it)
    __shared__ float colour32[PREMUL ? 256 : 1];
    __shared__ float unorm32[(PREMUL && SRGB) ? 256 : 1];
    {  // (kLoadThreads = 256 entries)
        const uint32_t t = threadIdx.x;
        if (!PREMUL) colour16[t] = SRGB ? kLoadSrgbF16[t] : kLoadUnormF16[t];
        if (!PREMUL && ALPHA == JH_LOAD_ALPHA_STRAIGHT && SRGB) unorm16[t] = kLoadUnormF16[t];
        if (PREMUL) colour32[t] = SRGB ? jload_linear(t) : jload_unorm(t);
        if (PREMUL && SRGB) unorm32[t] = jload_unorm(t);
        __syncthreads();
    }
    const uint16_t* a16 = (ALPHA == JH_LOAD_ALPHA_STRAIGHT && SRGB) ? unorm16 : colour16;
    const float* a32 = SRGB ? unorm32 : colour32;
    for (uint32_t it = blockIdx.x; it < total_items; it += gridDim.x) {
        LoadPair p;
        if (!load_pair(it, segs, dst, dst_w, dx, dy, w, &p)) continue;
        const uint8_t* srow = src + (uint64_t)p.row * pitch;
        uint32_t px[2] = {0u, 0u};
        if (p.va && p.vb) {
            const uint8_t* s = srow + 4 * p.c;
            if (((uintptr_t)s & 7u) == 0u) {  // (the same for every pair of the row)
                const uint2 q = *(const uint2*)s;
                px[0] = q.x; px[1] = q.y;
            } else if (((uintptr_t)s & 3u) == 0u) {
                px[0] = ((const uint32_t*)s)[0]; px[1] = ((const uint32_t*)s)[1];
            } else {
                px[0] = load_px_bytes(s); px[1] = load_px_bytes(s + 4);
            }
        } else if (p.va) {
            px[0] = load_px_bytes(srow + 4 * p.c);
        } else {
            px[1] = load_px_bytes(srow + 4 * (p.c + 1));
        }
        uint2 t[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t b0 = px[j] & 0xffu, g = (px[j] >> 8) & 0xffu, b2 = (px[j] >> 16) & 0xffu, a = px[j] >> 24;
            const uint32_t r = bgra ? b2 : b0, b = bgra ? b0 : b2;
            // (the store rule itself; jello_load.h's jload_texel_premultiplied is its host copy for the queries, and
            // tests/test_gpu_load.py holds this kernel to that query over every code x alpha pair)
            if (PREMUL) t[j] = texel_unpremultiply(make_float4(colour32[r], colour32[g], colour32[b], a32[a]));
            else jload_texel_tables(colour16, a16, ALPHA == JH_LOAD_ALPHA_OPAQUE, r, g, b, a, &t[j].x, &t[j].y);
        }
        store_pair(p, t[0], t[1]);
    }
}

// ---- YUV ----

struct LoadYuvPlanes {
    const uint8_t* p[3];  // Y, CbCr interleaved (NV12) or Cb, - or Cr
    uint64_t pitch[3];
};
struct LoadYuvCoef {
    int32_t k[5], off;
};

// (Cb, Cr) of chroma sample (cx, cy), both inside the planes.
template <bool NV12>
__device__ __forceinline__ void load_chroma(const LoadYuvPlanes& pl, uint32_t cx, uint32_t cy, int32_t* cb, int32_t* cr) {
    if (NV12) {
        const uint8_t* s = pl.p[1] + (uint64_t)cy * pl.pitch[1] + 2u * cx;
        *cb = s[0]; *cr = s[1];
    } else {
        *cb = pl.p[1][(uint64_t)cy * pl.pitch[1] + cx];
        *cr = pl.p[2][(uint64_t)cy * pl.pitch[2] + cx];
    }
}

// The texel of frame position (x, y), x < w, y < h.
template <bool NV12, bool BILINEAR>
__device__ __forceinline__ uint2 load_yuv_texel(const LoadYuvPlanes& pl, const LoadYuvCoef& k, const uint16_t* table, uint32_t x, uint32_t y, uint32_t cw,
                                                uint32_t ch) {
    const int32_t luma = pl.p[0][(uint64_t)y * pl.pitch[0] + x];
    const uint32_t cx0 = x >> 1, cy0 = y >> 1;
    int32_t cb00, cr00, s_cb, s_cr;
    load_chroma<NV12>(pl, cx0, cy0, &cb00, &cr00);
    if (BILINEAR) {
        const uint32_t cx1 = jload_chroma_other(x, cw), cy1 = jload_chroma_other(y, ch);
        int32_t cb01, cr01, cb10, cr10, cb11, cr11;
        load_chroma<NV12>(pl, cx1, cy0, &cb01, &cr01);
        load_chroma<NV12>(pl, cx0, cy1, &cb10, &cr10);
        load_chroma<NV12>(pl, cx1, cy1, &cb11, &cr11);
        s_cb = jload_chroma_sum(JH_CHROMA_BILINEAR, cb00, cb01, cb10, cb11);
        s_cr = jload_chroma_sum(JH_CHROMA_BILINEAR, cr00, cr01, cr10, cr11);
    } else {
        s_cb = jload_chroma_sum(JH_CHROMA_REPLICATE, cb00, 0, 0, 0);
        s_cr = jload_chroma_sum(JH_CHROMA_REPLICATE, cr00, 0, 0, 0);
    }
    const uint32_t c = jload_codes(k.k, k.off, luma, s_cb, s_cr);
    uint2 t;
    jload_texel_tables(table, table, true, c & 0xffu, (c >> 8) & 0xffu, c >> 16, 255u, &t.x, &t.y);
    return t;
}

// The transfer is only which table the workgroup copies into LDS.
template <bool NV12, bool BILINEAR>
__global__ __launch_bounds__(kLoadThreads) void k_load_yuv(LoadYuvPlanes pl, LoadYuvCoef k, uint2* __restrict__ dst, uint32_t dst_w, uint32_t dx, uint32_t dy,
                                                           uint32_t w, uint32_t h, uint32_t srgb, uint32_t segs, uint32_t total_items) {
    __shared__ uint16_t table[256];
    table[threadIdx.x] = srgb ? kLoadSrgbF16[threadIdx.x] : kLoadUnormF16[threadIdx.x];  // (kLoadThreads = 256 entries)
    __syncthreads();
    const uint32_t cw = (w + 1u) >> 1, ch = (h + 1u) >> 1;
    for (uint32_t it = blockIdx.x; it < total_items; it += gridDim.x) {
        LoadPair p;
        if (!load_pair(it, segs, dst, dst_w, dx, dy, w, &p)) continue;
        uint2 ta = make_uint2(0u, 0u), tb = ta;
        if (p.va) ta = load_yuv_texel<NV12, BILINEAR>(pl, k, table, (uint32_t)p.c, p.row, cw, ch);
        if (p.vb) tb = load_yuv_texel<NV12, BILINEAR>(pl, k, table, (uint32_t)(p.c + 1), p.row, cw, ch);
        store_pair(p, ta, tb);
    }
}

// Row segments of a rect.w x rect.h rectangle, or false when they do not fit one launch.
bool load_items(jimage_rect rect, uint32_t* segs, uint32_t* total) {
    const uint64_t s = walk_segs(rect.w, kLoadThreads), t = s * rect.h;
    if (t > 0x7fffffffull) return false;
    *segs = (uint32_t)s; *total = (uint32_t)t;
    return true;
}

}  // namespace

// The frame at src (rect.h rows of 4 * rect.w bytes, `pitch` apart, a jh_surface_format) into the rectangle rect of dst (inside it,
// not empty).  alpha: jh_load_alpha.  Returns 0, -1 on bad arguments, -2 on a launch error.
extern "C" int jh_load_surface_launch(hipStream_t stream, const void* src, uint64_t pitch, jimage_dst dst, jimage_rect rect, int format, int alpha,
                                      int num_cus) {
    if (!src || !dst.texels || !jframe_surface_format_ok(format) || !jload_alpha_ok(alpha) || jframe_surface_pitch_error(pitch, rect.w)) return -1;
    if (jimage_rect_empty(rect) || !jimage_rect_inside(rect, dst.width, dst.height)) return -1;
    uint32_t segs, total;
    if (!load_items(rect, &segs, &total)) return -1;
    const dim3 grid(grid_blocks(total, 1u, 8u, num_cus)), block(kLoadThreads);
    const uint32_t bgra = jframe_surface_bgra(format) ? 1u : 0u;
    const uint8_t* s = (const uint8_t*)src;
    uint2* d = (uint2*)dst.texels;
#define JH_LOAD_SURFACE(SRGB, ALPHA) \
    hipLaunchKernelGGL((k_load_surface<SRGB, ALPHA>), grid, block, 0, stream, s, pitch, d, dst.width, rect.x, rect.y, rect.w, bgra, segs, total)
    switch ((jframe_surface_srgb(format) ? 3 : 0) + alpha) {
        case 0: JH_LOAD_SURFACE(false, JH_LOAD_ALPHA_STRAIGHT); break;
        case 1: JH_LOAD_SURFACE(false, JH_LOAD_ALPHA_PREMULTIPLIED); break;
        case 2: JH_LOAD_SURFACE(false, JH_LOAD_ALPHA_OPAQUE); break;
        case 3: JH_LOAD_SURFACE(true, JH_LOAD_ALPHA_STRAIGHT); break;
        case 4: JH_LOAD_SURFACE(true, JH_LOAD_ALPHA_PREMULTIPLIED); break;
        default: JH_LOAD_SURFACE(true, JH_LOAD_ALPHA_OPAQUE); break;
    }
#undef JH_LOAD_SURFACE
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// The rect.w x rect.h 4:2:0 frame in planes[3] / pitches[3] (the third is unused for NV12) into the rectangle rect of dst (inside
// it, not empty).  layout, matrix, range, transfer, chroma: jh_yuv_layout, jh_yuv_matrix, jh_yuv_range, jh_yuv_transfer,
// jh_chroma_filter.  Returns 0, -1 on bad arguments, -2 on a launch error.
extern "C" int jh_load_yuv_launch(hipStream_t stream, const void* const* planes, const uint64_t* pitches, jimage_dst dst, jimage_rect rect, int layout,
                                  int matrix, int range, int transfer, int chroma, int num_cus) {
    if (jframe_yuv_enums_error(layout, matrix, range, transfer) || (chroma != JH_CHROMA_REPLICATE && chroma != JH_CHROMA_BILINEAR)) return -1;
    if (!dst.texels || jimage_rect_empty(rect) || !jimage_rect_inside(rect, dst.width, dst.height)) return -1;
    if (jframe_yuv_planes_error(layout, planes, pitches, rect.w, JFRAME_NULL_PLANE | JFRAME_SHORT_PITCH)) return -1;
    LoadYuvPlanes pl = {};
    for (int i = 0; i < jframe_yuv_planes(layout); i++) {
        pl.p[i] = (const uint8_t*)planes[i];
        pl.pitch[i] = pitches[i];
    }
    uint32_t segs, total;
    if (!load_items(rect, &segs, &total)) return -1;
    LoadYuvCoef k;
    for (int i = 0; i < 5; i++) k.k[i] = kLoadYuv[matrix][range][i];
    k.off = kLoadYuvOffset[range];
    const dim3 grid(grid_blocks(total, 1u, 8u, num_cus)), block(kLoadThreads);
    uint2* d = (uint2*)dst.texels;
    const uint32_t srgb = transfer == JH_YUV_TRANSFER_SRGB ? 1u : 0u;
#define JH_LOAD_YUV(NV12, BILINEAR) \
    hipLaunchKernelGGL((k_load_yuv<NV12, BILINEAR>), grid, block, 0, stream, pl, k, d, dst.width, rect.x, rect.y, rect.w, rect.h, srgb, segs, total)
    switch ((chroma == JH_CHROMA_BILINEAR ? 2 : 0) + (layout == JH_YUV_I420 ? 1 : 0)) {
        case 0: JH_LOAD_YUV(true, false); break;
        case 1: JH_LOAD_YUV(false, false); break;
        case 2: JH_LOAD_YUV(true, true); break;
        default: JH_LOAD_YUV(false, true); break;
    }
#undef JH_LOAD_YUV
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
