// kernels_distance.hip -- jh_distance: the Euclidean distance to a shape, capped at a radius R, through a linear ramp, the device half
// of the rule in include/jello_hip.h ("Distance") and DESIGN.md 5.20; the seed test, the run-length step, the combine, the stop and
// the value come from include/jello_distance.h, the one text this file and tools/distance_check.cpp both compile.  The squared
// distance D = min((R + 1)^2, min over the features of dx^2 + dy^2) is an integer defined on the SET of features, so any
// decomposition gives the same bits.  Two launches, ordered by the stream; no atomics, no hand-offs:
//   k_dist_cols   f16 image -> planes of G (uint16_t).  G(c, v) = min(R + 1, rows from row v to the nearest feature of column c).  A
//                 plane has rect_h rows of rect_w + 2 R columns: column c is image column rect_x - R + c whether it exists or not (one
//                 that does not holds the padding the rule implies: no seed; under EDGE_ZERO a non-seed at every row).  A lane owns a
//                 column, lanes along x: the 64 lanes of a wave read the chosen channel of 64 neighbouring texels (512 B) and write
//                 128 B of a plane row.  An item is one strip of 64 columns x one segment of rows (32 to max(64, 2 R) of them, as many as leave the
//                 launch about 1024 items); the lane walks the segment down
//                 with the counter "rows since the last feature" (clamped to R + 1), warmed up over the R rows above it, stores the
//                 counter, then walks up, warmed up over the R rows below, and stores the smaller of the two.  On the way up a feature
//                 is a stored 0, so the segment's texels are loaded once.  SIGNED walks both planes' counters at once.
//   k_dist_rows   planes -> f16 image.  An item is a row segment of kRowSeg outputs, one one-wave workgroup each: the segment's G and
//                 R more on each side are staged in LDS with 16-byte loads (the run is widened to the 16-byte grid of the plane's
//                 memory; a unit that is not wholly inside the planes is loaded halfword by halfword), then a lane per output walks
//                 D = min(CAP, min over |dx| <= R of dx^2 + G(X + dx)^2) outwards from dx = 0 and stops as soon as dx^2 >= the best
//                 so far -- exact, every later term is at least dx^2 -- so the cost follows the distance found, not R.  Neighbouring
//                 lanes read neighbouring halfwords: two lanes to a bank word, a broadcast, no conflict.  A wave
//                 whose staged segment holds no G <= R skips the walk: every D is CAP; one ballot decides.  Under SIGNED the lane's
//                 class is G_out(X) == 0 and selects the plane.  Then the square root, the ramp, colour x v and the store (texel_io.h).
// k_dist_rows<STRAIGHT, SIGNED>: four instantiations; channel, edge, R and OUTER / INNER are scalars.  VGPRs, LDS, scratch: DESIGN.md 5.20.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_distance.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kThreads = 64;        // both kernels: one wave per workgroup, a wave item each
constexpr uint32_t kStrip = 64;          // k_dist_cols: columns of an item, one per lane
constexpr uint32_t kMinSegRows = 32;     // k_dist_cols: rows of a segment, at least; at most max(64, 2 R), where the warm-up no more than doubles the loads;
constexpr uint32_t kColItems = 1024;     // in between as many as leave the launch about this many items (four waves a CU)
constexpr uint32_t kRowSeg = 256;        // k_dist_rows: outputs of an item, four per lane
constexpr uint32_t kStageUnits = (kRowSeg + 2u * JDIST_MAX_RADIUS + 7u) / 8u + 1u;  // 16-byte units of a staged run, widened to the grid: 97
constexpr uint32_t kPerCu = 32;          // workgroups to a CU, the rest by grid stride

struct ColArgs {
    const uint16_t* src;  // the source's f16 words (four to a texel), or null: never written
    uint16_t* planes;
    uint32_t W, H;             // the image
    uint32_t x0, y0, rw, rh;   // the rectangle
    uint32_t R, channel, clamp;
    uint32_t outer, inner;     // which planes are written; both: the outer one first
    float threshold;
    uint32_t pc;               // columns of a plane: rw + 2 R
    uint32_t seg_rows, strips, total;
};

// Whether image position (xi, Y) -- xi inside the image -- is a seed.
JD bool seed_at(const ColArgs& a, const uint16_t* __restrict__ src, uint32_t xi, uint32_t Y) {
    const float v = src ? jd::f16_to_f32(src[((uint64_t)Y * a.W + xi) * 4u + a.channel]) : 0.0f;
    return jdist_is_seed(v, a.threshold);
}

__global__ __launch_bounds__(kThreads) void k_dist_cols(const ColArgs a) {
    const uint32_t lane = jk::lane_id();
    const uint64_t plane_words = (uint64_t)a.rh * a.pc;
    // (the image and the two planes never overlap: the loads of the rows ahead need not wait for the plane's stores)
    const uint16_t* __restrict__ const src = a.src;
    uint16_t* __restrict__ const po = a.planes;
    uint16_t* __restrict__ const pi = a.planes + (a.outer ? plane_words : 0u);
    const bool zero_pad = a.clamp == 0u;
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t seg = it / a.strips, strip = it - seg * a.strips;
        const uint32_t c = strip * kStrip + lane;
        if (c >= a.pc) continue;
        const int64_t xs = (int64_t)a.x0 - a.R + c;  // the image column of plane column c
        const bool in_image = xs >= 0 && xs < (int64_t)a.W;
        const uint32_t xi = in_image ? (uint32_t)xs : 0u;
        const uint32_t v0 = seg * a.seg_rows, v1 = a.rh - v0 < a.seg_rows ? a.rh : v0 + a.seg_rows;  // the segment's rows of the rectangle
        const uint32_t Y0 = a.y0 + v0, Y1 = a.y0 + v1;                                              // ... and of the image
        // a column outside the image: no seed anywhere; a non-seed at every row under EDGE_ZERO, no position at all under CLAMP
        const bool pad_in = !in_image && zero_pad;
        // down: the counters in front of row ys, the warm-up rows [ys, Y0), then the segment
        const uint32_t ys = Y0 > a.R ? Y0 - a.R : 0u;
        uint32_t run_o = jdist_run_start(ys == 0u, false, !zero_pad, a.R), run_i = jdist_run_start(ys == 0u, true, !zero_pad, a.R);
        if (in_image) {
#pragma unroll 4
            for (uint32_t Y = ys; Y < Y0; Y++) {
                const bool s = seed_at(a, src, xi, Y);
                run_o = jdist_run(run_o, s, a.R);
                run_i = jdist_run(run_i, !s, a.R);
            }
        }
#pragma unroll 4
        for (uint32_t v = v0; v < v1; v++) {
            const bool s = in_image && seed_at(a, src, xi, a.y0 + v);
            run_o = jdist_run(run_o, s, a.R);
            run_i = jdist_run(run_i, in_image ? !s : pad_in, a.R);
            const uint64_t at = (uint64_t)v * a.pc + c;
            if (a.outer) po[at] = (uint16_t)run_o;
            if (a.inner) pi[at] = (uint16_t)run_i;
        }
        // up: the counters behind row ye - 1, the warm-up rows [Y1, ye) from the image, then the segment from what the way down stored
        const uint32_t ye = (uint64_t)Y1 + a.R < a.H ? Y1 + a.R : a.H;
        run_o = jdist_run_start(ye == a.H, false, !zero_pad, a.R);
        run_i = jdist_run_start(ye == a.H, true, !zero_pad, a.R);
        if (in_image) {
#pragma unroll 4
            for (uint32_t Y = ye; Y > Y1; Y--) {
                const bool s = seed_at(a, src, xi, Y - 1u);
                run_o = jdist_run(run_o, s, a.R);
                run_i = jdist_run(run_i, !s, a.R);
            }
        }
        for (uint32_t v = v1; v > v0; v--) {
            const uint64_t at = (uint64_t)(v - 1u) * a.pc + c;
            if (a.outer) {
                const uint32_t down = po[at];
                run_o = jdist_run(run_o, down == 0u, a.R);
                po[at] = (uint16_t)jd::umin_(down, run_o);
            }
            if (a.inner) {
                const uint32_t down = pi[at];
                run_i = jdist_run(run_i, down == 0u, a.R);
                pi[at] = (uint16_t)jd::umin_(down, run_i);
            }
        }
    }
}

struct RowArgs {
    const uint16_t* planes;
    uint32_t limit, plane_words;  // halfwords of all planes together, and of one
    uint2* dst;
    uint32_t W;                // texels of a row of dst
    uint32_t x0, y0, rw, rh;   // the rectangle
    uint32_t R, cap, which;
    uint32_t pc, segs, total;
    float scale, offset;
    float color[4];
};

// The halfwords [first, first + n) of the planes into the LDS region reg, widened to the 16-byte grid of the planes' memory; returns
// the halfword index in reg of `first`.  Units wholly inside [0, limit) are one 16-byte load, the others halfword loads (0 outside).
// (32-bit indices: the launcher refuses planes of 2^32 halfwords or more.)
JD uint32_t stage(const RowArgs& a, uint4* reg, uint32_t first, uint32_t n, uint32_t lane) {
    const uint32_t shift = first & 7u;  // (the planes start on a 16-byte boundary -- the launcher refuses other memory)
    const uint32_t base = first - shift;
    const uint32_t units = (shift + n + 7u) / 8u;  // (<= kStageUnits)
    for (uint32_t u = lane; u < units; u += kThreads) {
        const uint32_t h = base + 8u * u;  // (< limit, so h + 8 does not wrap)
        uint4 q;
        if (h + 8u <= a.limit) {
            q = *(const uint4*)(a.planes + h);
        } else {
            uint32_t w[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t lo = h + 2u * k < a.limit ? a.planes[h + 2u * k] : 0u, hi = h + 2u * k + 1u < a.limit ? a.planes[h + 2u * k + 1u] : 0u;
                w[k] = lo | (hi << 16);
            }
            q = make_uint4(w[0], w[1], w[2], w[3]);
        }
        reg[u] = q;
    }
    return shift;
}

// Whether any of the n halfwords of g is at most R, for the whole wave.
JD bool any_near(const uint16_t* g, uint32_t n, uint32_t R, uint32_t lane) {
    bool near = false;
    for (uint32_t e = lane; e < n; e += kThreads) near |= g[e] <= R;
    return __builtin_amdgcn_ballot_w64(near) != 0ull;
}

template <bool STRAIGHT, bool SIGNED>
__global__ __launch_bounds__(kThreads) void k_dist_rows(const RowArgs a) {
    __shared__ uint4 lds[(SIGNED ? 2u : 1u) * kStageUnits];
    const uint32_t lane = jk::lane_id();
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {
        const uint32_t v = it / a.segs, seg = it - v * a.segs;
        const uint32_t o0 = seg * kRowSeg, n_out = a.rw - o0 < kRowSeg ? a.rw - o0 : kRowSeg;
        const uint32_t n_stage = n_out + 2u * a.R;  // staged element e is plane column o0 + e; output o sits at element o + R
        const uint32_t first = v * a.pc + o0;
        jk::wave_sync();  // (the reads of the item before come first)
        const uint16_t* g0 = (const uint16_t*)lds + stage(a, lds, first, n_stage, lane);
        const uint16_t* g1 = g0;
        if (SIGNED) g1 = (const uint16_t*)(lds + kStageUnits) + stage(a, lds + kStageUnits, a.plane_words + first, n_stage, lane);
        jk::wave_sync();
        const bool walk = any_near(g0, n_stage, a.R, lane);  // (SIGNED: the outer plane -- without a seed near, every texel is a far non-seed)
        uint2* out = a.dst + ((uint64_t)(a.y0 + v) * a.W + a.x0 + o0);
        for (uint32_t o = lane; o < n_out; o += kThreads) {
            const uint32_t i = o + a.R;
            const bool seed = SIGNED && g0[i] == 0u;
            uint32_t best = a.cap;
            if (walk) {
                const uint16_t* g = seed ? g1 : g0;
                best = jdist_combine(best, 0u, g[i]);
                for (uint32_t dx = 1u; dx <= a.R && !jdist_stop(best, dx); dx++) {
                    best = jdist_combine(best, dx, g[i - dx]);
                    best = jdist_combine(best, dx, g[i + dx]);
                }
            }
            const float val = jdist_value(best, best, seed, (int)a.which, a.scale, a.offset);
            out[o] = texel_store<STRAIGHT>(make_float4(a.color[0] * val, a.color[1] * val, a.color[2] * val, a.color[3] * val));
        }
    }
}

}  // namespace

// The rectangle r of the RGBA16F image dst = the distance rule of desc (legal: jdist_desc_error) on the image src of the same size
// (null texels: transparent black; may be dst).  tmp: device memory of jdist_scratch_bytes(r.w, r.h, R, which) on a 16-byte boundary,
// the planes.  Two launches on `stream`.  Returns 0, -1 on arguments it refuses, -2 on a launch error.
extern "C" int jh_distance_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect r, const jh_distance_desc* desc, void* tmp, int num_cus) {
    if (!dst.texels || !tmp || ((uintptr_t)tmp & 15u) != 0u || !desc || jdist_desc_error(desc)) return -1;
    if (src.width != dst.width || src.height != dst.height || !jimage_rect_inside(r, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(r)) return 0;
    const uint32_t R = desc->max_distance;
    const uint64_t pc = jdist_plane_cols(r.w, R);
    if (pc > 0x7fffffffull) return -1;
    ColArgs c;
    c.src = (const uint16_t*)src.texels;
    c.planes = (uint16_t*)tmp;
    c.W = dst.width; c.H = dst.height;
    c.x0 = r.x; c.y0 = r.y; c.rw = r.w; c.rh = r.h;
    c.R = R;
    c.channel = (uint32_t)desc->channel;
    c.clamp = desc->edge == JDIST_EDGE_CLAMP ? 1u : 0u;
    c.outer = desc->which != JDIST_INNER ? 1u : 0u;
    c.inner = desc->which != JDIST_OUTER ? 1u : 0u;
    c.threshold = desc->threshold;
    c.pc = (uint32_t)pc;
    c.strips = (uint32_t)((pc + kStrip - 1u) / kStrip);
    const uint64_t seg_most = 2u * R > 64u ? 2u * R : 64u, seg_items = (uint64_t)r.h * c.strips / kColItems;
    c.seg_rows = (uint32_t)(seg_items < kMinSegRows ? kMinSegRows : (seg_items > seg_most ? seg_most : seg_items));
    const uint64_t items_cols = (uint64_t)((r.h + c.seg_rows - 1u) / c.seg_rows) * c.strips;
    RowArgs w;
    w.planes = (const uint16_t*)tmp;
    const uint64_t limit = jdist_scratch_bytes(r.w, r.h, R, desc->which) / 2u;
    if (limit > 0xffffff00ull) return -1;  // (the row pass indexes the planes in 32 bits, a 16-byte unit beyond the last halfword included)
    w.limit = (uint32_t)limit;
    w.plane_words = (uint32_t)((uint64_t)r.h * pc);
    w.dst = (uint2*)dst.texels;
    w.W = dst.width;
    w.x0 = r.x; w.y0 = r.y; w.rw = r.w; w.rh = r.h;
    w.R = R;
    w.cap = jdist_cap(R);
    w.which = (uint32_t)desc->which;
    w.pc = (uint32_t)pc;
    w.segs = (r.w + kRowSeg - 1u) / kRowSeg;
    const uint64_t items_rows = (uint64_t)r.h * w.segs;
    if (items_cols > 0x7fffffffull || items_rows > 0x7fffffffull) return -1;
    c.total = (uint32_t)items_cols;
    w.total = (uint32_t)items_rows;
    w.scale = desc->scale; w.offset = desc->offset;
    for (uint32_t i = 0; i < 4u; i++) w.color[i] = desc->color[i];
    hipLaunchKernelGGL(k_dist_cols, dim3(grid_blocks(items_cols, 1u, kPerCu, num_cus)), dim3(kThreads), 0, stream, c);
    const dim3 grid_rows(grid_blocks(items_rows, 1u, kPerCu, num_cus));
    with_flag((desc->flags & JDIST_STRAIGHT) != 0u, [&](auto straight) {
        with_flag(desc->which == JDIST_SIGNED, [&](auto two) {
            hipLaunchKernelGGL((k_dist_rows<decltype(straight)::value, decltype(two)::value>), grid_rows, dim3(kThreads), 0, stream, w);
        });
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
