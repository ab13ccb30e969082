// kernels_resample.hip -- jh_resample: one RGBA16F image resized into a rectangle of another, the device half of the rule in
// include/jello_hip.h ("Resample") and DESIGN.md 5.9; the windows and taps come from the host (include/jello_resample.h), uploaded
// once per geometry as the tables of kcommon.h (JhResampleTables), so a captured launch reads them on every replay.  Per texel
//   p = the f16 source texel widened, colour times alpha unless STRAIGHT                       once per source texel, when it is staged
//   H = 0; for k ascending over the x window: H = fmaf(w_k, p[k], H)      k_resample_rows: f16 image -> binary32 rows (tmp)
//   V = 0; for k ascending over the y window: V = fmaf(w_k, H[k], V)      k_resample_cols: tmp -> f16 image
//   store: STRAIGHT f16(V), otherwise V by the store rule (texel_io.h)
// and every implementation has to produce these bits, so the order of a sum is fixed and the parallelism is across outputs: a lane of
// k_resample_rows carries one output texel x 4 channels, a lane of k_resample_cols 4 rows x 2 columns x 4 channels = 32 accumulators,
// all independent fmaf chains.
// Rows: an item is one source row x 64 neighbouring outputs, one wave each.  The wave stages the source span those outputs read
// (at 16:1 up to 63 x 16 + 96 texels) through a private LDS region, two texels per lane and step with 16-byte loads where the pair
// is aligned -- the global loads stay coalesced whatever the ratio -- then every lane walks its own window.  Its weight comes from
// the transposed table (tap j of output o at w_x[j * dst_w + o]): one coalesced global_load_dword per tap, into a VGPR.
// Columns: an item is 4 output rows x 128 columns (64 lanes x 2).  The wave copies the four rows' weights into LDS, then walks down
// the source rows the four windows cover, four rows' loads in flight at a time, each row loaded once (two float4 per lane) and added
// to every output row whose window holds it -- per output row that is its taps in ascending order.  The weight of an output row is
// the same in every lane; read from LDS it arrives in a VGPR (as a kernel argument or a scalar load it would sit in an SGPR and move
// every v_fmac_f32 of the loop into the 4-cycle class, DESIGN.md 4, the price table).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_resample.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kRowThreads = 128, kRowWaves = 2;  // k_resample_rows: two waves, two LDS regions of up to 1 190 float4 each
constexpr uint32_t kColThreads = 256, kColWaves = 4;
constexpr uint32_t kColStrip = 128, kColRows = 4;  // k_resample_cols: a wave's item is 128 columns (64 lanes x 2) x 4 output rows
// an upper bound of the span of a row item (64 windows that start at most 16 apart: 63 x 16 + 96, and room for the truncations),
// and what its skewed region takes
constexpr uint32_t kMaxSpan = JH_RESAMPLE_ROW_SEG * JRESAMPLE_MAX_RATIO + JRESAMPLE_MAX_TAPS;
constexpr uint32_t kMaxRegion = kMaxSpan - 1u + ((kMaxSpan - 1u) >> 4) + 1u;

// Rows [sy, sy + n_rows) of the source image (W texels per row; null: never written, transparent black), the columns of the source
// rectangle from sx on: H of every output column into tmp (n_rows x dw float4).  item = row * segs + seg; the waves stride over the
// items.  Dynamic LDS: a private region of `region` float4 per wave (the staged span, skewed).
template <bool STRAIGHT>
__global__ __launch_bounds__(kRowThreads) void k_resample_rows(const uint2* __restrict__ src, float4* __restrict__ tmp, uint32_t W, uint32_t sx,
                                                               uint32_t sy, uint32_t dw, uint32_t segs, uint32_t region, uint32_t total_items,
                                                               const uint2* __restrict__ win, const uint4* __restrict__ seg_tab,
                                                               const float* __restrict__ wx) {
    extern __shared__ float4 resample_lds[];
    const uint32_t wave = jk::uni(threadIdx.x >> 6), lane = jk::lane_id();
    float4* reg = resample_lds + wave * region;
    for (uint32_t it = blockIdx.x * kRowWaves + wave; it < total_items; it += gridDim.x * kRowWaves) {
        const uint32_t row = it / segs, sg = it - row * segs;
        const uint4 sd = seg_tab[sg];
        const uint32_t start = sd.x, len = sd.y, max_taps = sd.z;
        const uint32_t o = sg * JH_RESAMPLE_ROW_SEG + lane, oc = o < dw ? o : dw - 1u;  // (loads of a lane beyond the row stay inside the tables)
        const uint2 wn = win[oc];
        const uint32_t n_taps = o < dw ? wn.y : 0u, base = wn.x - start;
        const uint2* srow = src ? src + ((uint64_t)(sy + row) * W + sx + start) : nullptr;
        jk::wave_sync();  // (the reads of the item before come first)
        // two texels per lane and step: one 16-B load where the pair is 16-B aligned and inside the span, 8-B loads otherwise
        const bool pair_aligned = (((uintptr_t)srow) & 15u) == 0u;
        for (uint32_t e = 2u * lane; e < len; e += 128u) {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
            if (srow) {
                if (pair_aligned && e + 1u < len) {
                    const uint4 q = *(const uint4*)(srow + e);
                    a = texel_widen<STRAIGHT>(make_uint2(q.x, q.y));
                    b = texel_widen<STRAIGHT>(make_uint2(q.z, q.w));
                } else {
                    a = texel_widen<STRAIGHT>(srow[e]);
                    if (e + 1u < len) b = texel_widen<STRAIGHT>(srow[e + 1u]);
                }
            }
            reg[jh_resample_skew(e)] = a;
            if (e + 1u < len) reg[jh_resample_skew(e + 1u)] = b;
        }
        jk::wave_sync();
        // Every lane its own window, ascending.  The loads of a step are unconditional (the weight table is zero where an output has
        // fewer taps, the LDS index is held inside the span), so that four steps' loads can be in flight together; a tap beyond the
        // lane's window is not added: its fmaf must not execute (0 x Inf would be a NaN).
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float* wp = wx + oc;
#pragma unroll 4
        for (uint32_t j = 0; j < max_taps; j++) {
            const float w = wp[(uint64_t)j * dw];
            const uint32_t t = base + j < len ? base + j : len - 1u;
            const float4 p = reg[jh_resample_skew(t)];
            if (j < n_taps) fma4(acc, w, p);
        }
        if (o < dw) tmp[(uint64_t)row * dw + o] = acc;
    }
}

// The rectangle (dx, dy, dw, dh) of dst (DW texels per row) out of tmp (rows of the source rectangle x dw float4).  An item =
// kColRows output rows x kColStrip columns, one wave each; item = group * strips + strip.
template <bool STRAIGHT>
__global__ __launch_bounds__(kColThreads) void k_resample_cols(const float4* __restrict__ tmp, uint2* __restrict__ dst, uint32_t DW, uint32_t dx,
                                                               uint32_t dy, uint32_t dw, uint32_t dh, uint32_t strips, uint32_t total_items,
                                                               const uint2* __restrict__ win, const float* __restrict__ wy, uint32_t stride) {
    __shared__ float wl_all[kColWaves][kColRows * JRESAMPLE_MAX_TAPS];
    const uint32_t wave = jk::uni(threadIdx.x >> 6), lane = jk::lane_id();
    float* wl = wl_all[wave];
    for (uint32_t it = blockIdx.x * kColWaves + wave; it < total_items; it += gridDim.x * kColWaves) {
        const uint32_t grp = it / strips, strip = it - grp * strips;
        const uint32_t ry = grp * kColRows, n_o = dh - ry < kColRows ? dh - ry : kColRows;
        jk::wave_sync();  // (the reads of the item before come first)
        for (uint32_t i = lane; i < n_o * stride; i += 64u) wl[i] = wy[(uint64_t)ry * stride + i];
        jk::wave_sync();
        uint32_t first[kColRows], n_taps[kColRows], s_lo = 0xffffffffu, s_hi = 0u;
#pragma unroll
        for (uint32_t o = 0; o < kColRows; o++) {
            const uint2 wn = win[o < n_o ? ry + o : ry];
            first[o] = wn.x;
            n_taps[o] = o < n_o ? wn.y : 0u;
            if (o < n_o) {
                s_lo = wn.x < s_lo ? wn.x : s_lo;
                s_hi = wn.x + wn.y > s_hi ? wn.x + wn.y : s_hi;
            }
        }
        const uint32_t c = strip * kColStrip + 2u * lane;  // the lane's columns c, c + 1 of the rectangle; loads stay inside it
        const uint32_t ca = c < dw ? c : dw - 1u, cb = c + 1u < dw ? c + 1u : dw - 1u;
        float4 acc[kColRows][2];
#pragma unroll
        for (uint32_t o = 0; o < kColRows; o++) acc[o][0] = acc[o][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // source row s is tap s - first[o] of output row o (wave-uniform tests; s - first[o] wraps for s < first[o])
        auto add_row = [&](uint32_t s, const float4& a, const float4& b) {
#pragma unroll
            for (uint32_t o = 0; o < kColRows; o++) {
                const uint32_t j = s - first[o];
                if (j < n_taps[o]) {
                    const float w = wl[o * stride + j];
                    fma4(acc[o][0], w, a);
                    fma4(acc[o][1], w, b);
                }
            }
        };
        uint32_t s = s_lo;
        for (; s + 4u <= s_hi; s += 4u) {  // four rows' loads in flight before the first multiply-add: a 16:1 item walks up to 144 rows
            const float4* p = tmp + (uint64_t)s * dw;
            const float4 a0 = p[ca], b0 = p[cb], a1 = p[dw + ca], b1 = p[dw + cb];
            const float4 a2 = p[2ull * dw + ca], b2 = p[2ull * dw + cb], a3 = p[3ull * dw + ca], b3 = p[3ull * dw + cb];
            add_row(s, a0, b0);
            add_row(s + 1u, a1, b1);
            add_row(s + 2u, a2, b2);
            add_row(s + 3u, a3, b3);
        }
        for (; s < s_hi; s++) {
            const float4* p = tmp + (uint64_t)s * dw;
            add_row(s, p[ca], p[cb]);
        }
#pragma unroll
        for (uint32_t o = 0; o < kColRows; o++) {
            if (o >= n_o) break;
            uint2* d = dst + ((uint64_t)(dy + ry + o) * DW + dx + c);
            const uint2 ta = texel_store<STRAIGHT>(acc[o][0]), tb = texel_store<STRAIGHT>(acc[o][1]);
            if (c + 1u < dw && ((uintptr_t)d & 15u) == 0u) {
                *(uint4*)d = make_uint4(ta.x, ta.y, tb.x, tb.y);
            } else {
                if (c < dw) d[0] = ta;
                if (c + 1u < dw) d[1] = tb;
            }
        }
    }
}

}  // namespace

// The rectangle d of the RGBA16F image dst = the rectangle s of the image src (null texels: transparent black; another image than
// dst) resized by the tables of this geometry, which are device memory (the struct itself is read during the call).  tmp: device
// memory of jresample_scratch_bytes(s, d), the rows jresample_scratch_rows names.  Two launches on `stream`.
extern "C" int jh_resample_launch(hipStream_t stream, jimage_src src, jimage_rect s, jimage_dst dst, jimage_rect d, int straight,
                                  const JhResampleTables* tables, void* tmp, int num_cus) {
    if (!dst.texels || !tmp || !tables || src.texels == dst.texels) return -1;
    const JhResampleTables t = *tables;
    if (!t.win_x || !t.seg_x || !t.w_x || !t.win_y || !t.w_y) return -1;
    if (!jimage_rect_inside(s, src.width, src.height) || !jimage_rect_inside(d, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(s) || jimage_rect_empty(d)) return -1;
    const uint32_t dw = d.w, dh = d.h;
    if (t.taps_x == 0u || t.taps_x > JRESAMPLE_MAX_TAPS || t.stride_y == 0u || t.stride_y > JRESAMPLE_MAX_TAPS || t.region_x == 0u || t.region_x > kMaxRegion)
        return -1;
    const uint32_t segs = (dw + JH_RESAMPLE_ROW_SEG - 1u) / JH_RESAMPLE_ROW_SEG, strips = (dw + kColStrip - 1u) / kColStrip;
    const uint64_t items_h = (uint64_t)jresample_scratch_rows(s) * segs, items_v = (uint64_t)((dh + kColRows - 1u) / kColRows) * strips;
    if (items_h > 0x7fffffffull || items_v > 0x7fffffffull) return -1;
    const size_t lds = (size_t)kRowWaves * t.region_x * sizeof(float4);
    const dim3 grid_h(grid_blocks(items_h, kRowWaves, 8u, num_cus)), grid_v(grid_blocks(items_v, kColWaves, 8u, num_cus));
    with_flag(straight != 0, [&](auto flag) {
        constexpr bool STRAIGHT = decltype(flag)::value;
        hipLaunchKernelGGL(k_resample_rows<STRAIGHT>, grid_h, dim3(kRowThreads), lds, stream, (const uint2*)src.texels, (float4*)tmp, src.width, s.x, s.y, dw, segs, t.region_x,
                           (uint32_t)items_h, t.win_x, t.seg_x, t.w_x);
        hipLaunchKernelGGL(k_resample_cols<STRAIGHT>, grid_v, dim3(kColThreads), 0, stream, (const float4*)tmp, (uint2*)dst.texels, dst.width, d.x, d.y, dw, dh, strips,
                           (uint32_t)items_v, t.win_y, t.w_y, t.stride_y);
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
