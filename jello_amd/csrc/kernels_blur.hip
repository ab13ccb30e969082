// kernels_blur.hip -- jh_blur: separable Gaussian blur of an RGBA16F image, the device half of the rule in include/jello_hip.h
// ("Gaussian blur") and DESIGN.md 5.7; the taps come from the host (include/jello_blur.h) and travel in the kernel arguments, so a
// captured launch carries them.  Per texel and channel
//   H = 0; for k = -Rx..Rx ascending: H = fmaf(w_k, (float)src[x + k], H)          k_blur_rows: f16 image -> binary32 rows (tmp)
//   V = 0; for k = -Ry..Ry ascending: V = fmaf(w_k, H[y + k], V); dst = f16(V)     k_blur_cols: tmp -> f16 image
// and every implementation has to produce these bits, so the order of a sum is fixed and the parallelism is across outputs: a lane of
// k_blur_rows carries 4 neighbouring texels x 4 channels = 16 accumulators, a lane of k_blur_cols 8 rows x 2 columns x 4 channels =
// 64, all independent fmaf chains.  Both passes always run: with sigma = 0 a pass is the single tap 1.0f, which is exact, and an
// in-place blur never reads the image it is writing (rows read src and write tmp, columns read tmp and write dst).
// A tap outside the image: CLAMP stages / loads the nearest texel; ZERO must not execute the tap's fmaf.  The row pass stages -0.0f
// for it instead, which is the same thing: w >= +0, so the product is -0, and x + (-0) = x for every x, -0 and NaN included (+0
// would turn an accumulator of -0, which a product that underflows can leave, into +0).  The column pass skips the row.
// The weights are read from LDS into VGPRs: as kernel arguments they would sit in SGPRs and move every v_fmac_f32 of the tap loop
// into the 4-cycle class (the price table).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "../../include/jello_blur.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kBlurThreads = 256, kBlurWaves = 4;
constexpr uint32_t kMaxRadius = 192;               // JBLUR_MAX_RADIUS
constexpr uint32_t kTapSlots = 388;                // 2 * 192 + 1 taps, rounded up to whole float4s
struct BlurTaps { float w[kTapSlots]; };           // by value in the kernel arguments (1 552 bytes)
constexpr uint32_t kRowSeg = 256;                  // k_blur_rows: output texels of a wave's row segment (64 lanes x 4)
constexpr uint32_t kColStrip = 128, kColRows = 8;  // k_blur_cols: a wave's item is 128 columns (64 lanes x 2) x 8 output rows

// A staged row in LDS: texel t of the segment sits at float4 index t + t / 4.  A lane reads texels 4 * lane + c (c the same in
// every lane), i.e. 80 bytes apart instead of 64: the 16 lanes a ds_read_b128 serves together then hit 16 different bank quads
// (64 bytes apart they would share four).
__host__ __device__ __forceinline__ uint32_t skew(uint32_t t) { return t + (t >> 2); }

// The texel of column x of the row at srow (null: a never-written source, transparent black) as the row pass stages it.
template <bool CLAMP>
JD float4 staged_texel(const uint2* srow, int64_t x, uint32_t W) {
    if (x < 0 || x >= (int64_t)W) {
        if (!CLAMP) return make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
        x = x < 0 ? 0 : (int64_t)W - 1;
    }
    return srow ? jd::rgba16f_to_f32(srow[x]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// Rows [row0, row0 + n_rows) of the image, columns [x0, x0 + rw): H into tmp (n_rows x rw float4).  An item = one row segment of up
// to kRowSeg outputs, one wave each; item = row * segs + seg; the waves stride over the items.  Dynamic LDS: the taps, then a
// private region of `region` float4 per wave (the segment plus R texels on either side, skewed).
template <bool CLAMP>
__global__ __launch_bounds__(kBlurThreads) void k_blur_rows(const uint2* __restrict__ src, float4* __restrict__ tmp, uint32_t W, uint32_t x0,
                                                            uint32_t rw, uint32_t row0, uint32_t R, uint32_t segs, uint32_t region,
                                                            uint32_t total_items, BlurTaps taps) {
    extern __shared__ float4 blur_lds[];
    float* wl = (float*)blur_lds;
    const uint32_t n_taps = 2u * R + 1u;
    for (uint32_t i = threadIdx.x; i < n_taps; i += kBlurThreads) wl[i] = taps.w[i];
    __syncthreads();
    const uint32_t wave = jk::uni(threadIdx.x >> 6), lane = jk::lane_id();
    float4* reg = blur_lds + kTapSlots / 4u + wave * region;
    const float4* win = reg + 5u * lane;  // skew(4 * lane)
    for (uint32_t it = blockIdx.x * kBlurWaves + wave; it < total_items; it += gridDim.x * kBlurWaves) {
        const uint32_t row = it / segs, seg = it - row * segs;
        const uint32_t o0 = seg * kRowSeg, n_out = rw - o0 < kRowSeg ? rw - o0 : kRowSeg;
        const int64_t xs0 = (int64_t)x0 + o0 - R;  // the image column of staged texel 0
        const uint32_t n_stage = n_out + 2u * R;
        const uint2* srow = src ? src + (uint64_t)(row0 + row) * W : nullptr;
        jk::wave_sync();  // (the reads of the item before come first)
        // two texels per lane and step: one 16-B load where the pair is 16-B aligned and inside the row, 8-B loads otherwise
        const bool pair_aligned = srow && (((((uintptr_t)srow) >> 3) + (uint64_t)xs0) & 1u) == 0u;
        for (uint32_t e = 2u * lane; e < n_stage; e += 128u) {
            const int64_t xa = xs0 + e;
            float4 a, b;
            if (pair_aligned && xa >= 0 && xa + 1 < (int64_t)W) {
                const uint4 q = *(const uint4*)(srow + xa);
                a = jd::rgba16f_to_f32(make_uint2(q.x, q.y));
                b = jd::rgba16f_to_f32(make_uint2(q.z, q.w));
            } else {
                a = staged_texel<CLAMP>(srow, xa, W);
                b = staged_texel<CLAMP>(srow, xa + 1, W);
            }
            reg[skew(e)] = a;
            if (e + 1u < n_stage) reg[skew(e + 1u)] = b;
        }
        jk::wave_sync();
        // The lane's outputs are texels 4 * lane + o, o = 0..3; tap j of output o reads texel 4 * lane + o + j.  Four taps a step: the
        // window t0..t6 = texels 4 * lane + 4 g + 0..6 slides by four (three kept, four read), every output takes its taps in order.
        float4 acc0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), acc1 = acc0, acc2 = acc0, acc3 = acc0;
        float4 t0 = win[0], t1 = win[1], t2 = win[2];
        const uint32_t groups = n_taps >> 2;
        for (uint32_t g = 0; g < groups; g++) {
            const float4* p = win + 5u * g;  // skew(4 * lane + 4 * g + i) = 5 * lane + 5 * g + i + i / 4
            const float4 t3 = p[3], t4 = p[5], t5 = p[6], t6 = p[7];
            const float4 w = ((const float4*)wl)[g];
            fma4(acc0, w.x, t0); fma4(acc1, w.x, t1); fma4(acc2, w.x, t2); fma4(acc3, w.x, t3);
            fma4(acc0, w.y, t1); fma4(acc1, w.y, t2); fma4(acc2, w.y, t3); fma4(acc3, w.y, t4);
            fma4(acc0, w.z, t2); fma4(acc1, w.z, t3); fma4(acc2, w.z, t4); fma4(acc3, w.z, t5);
            fma4(acc0, w.w, t3); fma4(acc1, w.w, t4); fma4(acc2, w.w, t5); fma4(acc3, w.w, t6);
            t0 = t4; t1 = t5; t2 = t6;
        }
        for (uint32_t j = groups * 4u; j < n_taps; j++) {  // the last one or three taps (2 R + 1 is odd)
            const float w = wl[j];
            fma4(acc0, w, win[skew(j)]); fma4(acc1, w, win[skew(j + 1u)]); fma4(acc2, w, win[skew(j + 2u)]); fma4(acc3, w, win[skew(j + 3u)]);
        }
        const uint32_t o = 4u * lane;
        float4* out = tmp + (uint64_t)row * rw + o0 + o;
        if (o < n_out) out[0] = acc0;
        if (o + 1u < n_out) out[1] = acc1;
        if (o + 2u < n_out) out[2] = acc2;
        if (o + 3u < n_out) out[3] = acc3;
    }
}

// One input row of a k_blur_cols item: row s of the item is image row yc - R + s and tap s - o of output row o.  ALL: the row is in
// every one of the eight windows, nothing is tested.
template <bool CLAMP, bool ALL>
JD void cols_row(float4 (&acc)[kColRows][2], const float4* __restrict__ tmp, const float* wl, int64_t yc, uint32_t s, uint32_t R, uint32_t H,
                 uint32_t row0, uint32_t rw, uint32_t ca, uint32_t cb, uint32_t n_o, uint32_t n_taps) {
    int64_t i = yc - (int64_t)R + s;
    if (i < 0 || i >= (int64_t)H) {
        if (!CLAMP) return;  // ZERO: the tap contributes nothing
        i = i < 0 ? 0 : (int64_t)H - 1;
    }
    const float4* p = tmp + (uint64_t)(i - (int64_t)row0) * rw;
    const float4 a = p[ca], b = p[cb];
#pragma unroll
    for (uint32_t o = 0; o < kColRows; o++) {
        const uint32_t j = s - o;  // (wraps for s < o)
        if (ALL || (o < n_o && j < n_taps)) {
            const float w = wl[j];
            fma4(acc[o][0], w, a);
            fma4(acc[o][1], w, b);
        }
    }
}

// The rectangle (x0, y0, rw, rh) of dst out of tmp, whose row 0 is image row row0 (tmp holds every row of the image within R of the
// rectangle's).  An item = kColRows output rows x kColStrip columns, one wave each; item = group * strips + strip.  The wave walks
// down the input rows the item's windows cover, each row loaded once (two float4 per lane) and added to every output row whose
// window holds it -- per output row that is its taps in ascending order.
template <bool CLAMP>
__global__ __launch_bounds__(kBlurThreads) void k_blur_cols(const float4* __restrict__ tmp, uint2* __restrict__ dst, uint32_t W, uint32_t H,
                                                            uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh, uint32_t row0, uint32_t R,
                                                            uint32_t strips, uint32_t total_items, BlurTaps taps) {
    __shared__ float wl[kTapSlots];
    const uint32_t n_taps = 2u * R + 1u;
    for (uint32_t i = threadIdx.x; i < n_taps; i += kBlurThreads) wl[i] = taps.w[i];
    __syncthreads();
    const uint32_t wave = jk::uni(threadIdx.x >> 6), lane = jk::lane_id();
    for (uint32_t it = blockIdx.x * kBlurWaves + wave; it < total_items; it += gridDim.x * kBlurWaves) {
        const uint32_t grp = it / strips, strip = it - grp * strips;
        const uint32_t ry = grp * kColRows, n_o = rh - ry < kColRows ? rh - ry : kColRows;
        const uint32_t c = strip * kColStrip + 2u * lane;  // the lane's columns c, c + 1 of the rectangle; loads stay inside it
        const uint32_t ca = c < rw ? c : rw - 1u, cb = c + 1u < rw ? c + 1u : rw - 1u;
        float4 acc[kColRows][2];
#pragma unroll
        for (uint32_t o = 0; o < kColRows; o++) acc[o][0] = acc[o][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const int64_t yc = (int64_t)y0 + ry;  // the image row of output row 0
        const uint32_t n_in = n_o + 2u * R;   // input row s is image row yc - R + s, and tap s - o of output row o
        // rows [lo, hi) are in all eight windows (none when the item has fewer than eight rows or R < 4)
        const uint32_t lo = n_o == kColRows && n_taps >= kColRows ? kColRows - 1u : n_in, hi = lo < n_in ? n_taps : n_in;
        for (uint32_t s = 0; s < lo; s++) cols_row<CLAMP, false>(acc, tmp, wl, yc, s, R, H, row0, rw, ca, cb, n_o, n_taps);
        for (uint32_t s = lo; s < hi; s++) cols_row<CLAMP, true>(acc, tmp, wl, yc, s, R, H, row0, rw, ca, cb, n_o, n_taps);
        for (uint32_t s = hi; s < n_in; s++) cols_row<CLAMP, false>(acc, tmp, wl, yc, s, R, H, row0, rw, ca, cb, n_o, n_taps);
#pragma unroll
        for (uint32_t o = 0; o < kColRows; o++) {
            if (o >= n_o) break;
            uint2* d = dst + (uint64_t)(yc + o) * W + x0 + c;
            const uint2 ta = texel_pack(acc[o][0]), tb = texel_pack(acc[o][1]);
            if (c + 1u < rw && ((uintptr_t)d & 15u) == 0u) {
                *(uint4*)d = make_uint4(ta.x, ta.y, tb.x, tb.y);
            } else {
                if (c < rw) d[0] = ta;
                if (c + 1u < rw) d[1] = tb;
            }
        }
    }
}

}  // namespace

// The rectangle r of the RGBA16F image dst = the blur of the image src of the same size (null texels: transparent black; may be
// dst).  taps_x / taps_y: 2 R + 1 weights each (jblur_taps), read during the call.  tmp: device memory of jblur_scratch_bytes(r,
// radius_y, height), the rows jblur_scratch_rows names.  clamp: JH_BLUR_EDGE_CLAMP.  Two launches on `stream`.
extern "C" int jh_blur_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect r, int clamp, const float* taps_x, uint32_t radius_x,
                              const float* taps_y, uint32_t radius_y, void* tmp, int num_cus) {
    if (!dst.texels || !tmp || !taps_x || !taps_y || radius_x > kMaxRadius || radius_y > kMaxRadius) return -1;
    if (src.width != dst.width || src.height != dst.height || !jimage_rect_inside(r, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(r)) return 0;
    const jimage_rows rows = jblur_scratch_rows(r, radius_y, dst.height);
    const uint32_t segs = (r.w + kRowSeg - 1u) / kRowSeg, strips = (r.w + kColStrip - 1u) / kColStrip;
    const uint64_t items_h = (uint64_t)rows.n_rows * segs, items_v = (uint64_t)((r.h + kColRows - 1u) / kColRows) * strips;
    if (items_h > 0x7fffffffull || items_v > 0x7fffffffull) return -1;
    BlurTaps tx, ty;
    memset(&tx, 0, sizeof tx);
    memset(&ty, 0, sizeof ty);
    memcpy(tx.w, taps_x, (2u * radius_x + 1u) * sizeof(float));
    memcpy(ty.w, taps_y, (2u * radius_y + 1u) * sizeof(float));
    const uint32_t region = skew(kRowSeg - 1u + 2u * radius_x) + 1u;
    const size_t lds = (size_t)(kTapSlots / 4u + kBlurWaves * region) * sizeof(float4);
    const dim3 block(kBlurThreads), grid_h(grid_blocks(items_h, kBlurWaves, 8u, num_cus)), grid_v(grid_blocks(items_v, kBlurWaves, 8u, num_cus));
    with_flag(clamp != 0, [&](auto edge) {
        constexpr bool CLAMP = decltype(edge)::value;
        hipLaunchKernelGGL(k_blur_rows<CLAMP>, grid_h, block, lds, stream, (const uint2*)src.texels, (float4*)tmp, dst.width, r.x, r.w, rows.row0, radius_x, segs, region,
                           (uint32_t)items_h, tx);
        hipLaunchKernelGGL(k_blur_cols<CLAMP>, grid_v, block, 0, stream, (const float4*)tmp, (uint2*)dst.texels, dst.width, dst.height, r.x, r.y, r.w, r.h, rows.row0, radius_y,
                           strips, (uint32_t)items_v, ty);
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
