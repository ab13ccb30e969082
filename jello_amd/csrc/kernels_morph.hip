// kernels_morph.hip -- jh_morphology: erode / dilate of an RGBA16F image by a box, the device half of the rule in
// include/jello_hip.h ("Morphology") and DESIGN.md 5.11; the order key and its inverse come from include/jello_morph.h, the one
// text this file and tools/morph_check.cpp both compile.  Per texel and channel the result is the least (ERODE) or greatest (DILATE)
// operand of the window [X - rx, X + rx] x [Y - ry, Y + ry] in IEEE totalOrder, a NaN sticky -- one of the operands, so nothing is
// rounded and ANY decomposition of the window gives the same bits.  The kernels use that freedom: everything between the load of
// a texel and the store of a result is a signed-integer min or max on keys (v_min_i32 / v_max_i32: no NaN or signed-zero modes),
// and no kernel walks the 2r + 1 positions of a window.  Three launches, ordered by the stream; no atomics, no hand-offs:
//   k_morph_rows    f16 image -> plane H (keys, 16 B per texel).  A wave stages a row segment plus rx texels on either side into its
//                   private LDS region, already as keys of p (colour times alpha unless STRAIGHT) and with the edge rule applied: a
//                   position outside the image is the key of +0.0f (ZERO) or the operator's neutral key (CLAMP: it does not take
//                   part).  Then it doubles in place, M_k[i] = op(M_k-1[i], M_k-1[i + 2^(k-1)]), floor(log2(2 rx + 1)) steps, and an
//                   output is op(M[o], M[o + 2 rx + 1 - 2^k]): two overlapping reads.  At most 8 steps for rx = 255.
//                   (A lane touches element base + lane, so the 64 lanes of a ds_read_b128 / ds_write_b128 cover 1 KB of
//                   consecutive LDS and no two of the 16 served together share a bank: the region needs no skew, unlike k_blur_rows,
//                   whose lanes sit four texels apart.)
//   k_morph_prefix  plane H -> plane P.  The planes have rect_h + 2 ry rows: row v is image row rect_y - ry + v whether it exists or
//                   not (a row outside the image is the padding key throughout and is never loaded), so every window of the column
//                   pass is exactly 2 ry + 1 rows and the blocks of 2 ry + 1 rows are aligned to the rectangle.  A lane owns a
//                   column and walks down a block: P[v] = op of H over the block's rows up to v.
//   k_morph_final   H, P -> f16 image.  The same walk bottom-up forms the suffix S[v] = op of H over the block's rows from v on; the
//                   window of output row v is rows v .. v + 2 ry, the end of v's block and the beginning of the next: op(S[v], P[v +
//                   2 ry]).  Un-keyed, stored as the rule says (STRAIGHT: exact; otherwise the store rule, texel_io.h).
// A column item is one texel per lane x 64 lanes (8-byte stores, 512 B per wave and row) instead of the blur's column pair: with
// blocks of up to 511 rows the strips are what gives the launch its items (DESIGN.md 5.11 has the count), and eight rows' loads are
// in flight per lane before the first is used.  Blocks shorter than kItemRows are grouped so that an item is never a row or two.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_morph.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kMorphThreads = 256, kMorphWaves = 4;  // k_morph_rows: four waves, four LDS regions
constexpr uint32_t kColThreads = 64;  // column kernels: one wave per workgroup -- no LDS to share, and with blocks of up to 511 rows
                                      // the items are few: one item per workgroup spreads them over the CUs
constexpr uint32_t kRowSeg = 256;      // k_morph_rows: output texels of a wave's row segment
constexpr uint32_t kColStrip = 64;     // column kernels: a wave's strip, one texel per lane
constexpr uint32_t kRowsInFlight = 8;  // column kernels: rows loaded before the first is used
constexpr uint32_t kItemRows = 32;     // column kernels: blocks are grouped until an item has at least this many rows

template <bool DILATE> JD int32_t pick(int32_t a, int32_t b) { return DILATE ? jd::imax_(a, b) : jd::imin_(a, b); }
template <bool DILATE> JD int4 pick4(const int4& a, const int4& b) {
    return make_int4(pick<DILATE>(a.x, b.x), pick<DILATE>(a.y, b.y), pick<DILATE>(a.z, b.z), pick<DILATE>(a.w, b.w));
}
JD int4 splat(int32_t k) { return make_int4(k, k, k, k); }

// The keys of a source texel: widened, colour times alpha unless STRAIGHT (exact: 11 + 11 bits; Inf x 0 is a NaN and gets its key).
template <bool DILATE, bool STRAIGHT>
JD int4 texel_keys(uint2 t) {
    const float4 p = texel_widen<STRAIGHT>(t);
    return make_int4(jmorph_key(__float_as_uint(p.x), DILATE), jmorph_key(__float_as_uint(p.y), DILATE), jmorph_key(__float_as_uint(p.z), DILATE),
                     jmorph_key(__float_as_uint(p.w), DILATE));
}
// Column x of the row at srow (null: a never-written source, transparent black, key 0) as the row pass stages it.
template <bool DILATE, bool STRAIGHT>
JD int4 staged_keys(const uint2* srow, int64_t x, uint32_t W, int32_t pad) {
    if (x < 0 || x >= (int64_t)W) return splat(pad);
    return srow ? texel_keys<DILATE, STRAIGHT>(srow[x]) : splat(0);
}

template <bool STRAIGHT>
JD uint2 stored_texel(const int4& k) {
    return texel_store<STRAIGHT>(make_float4(__uint_as_float(jmorph_unkey(k.x)), __uint_as_float(jmorph_unkey(k.y)), __uint_as_float(jmorph_unkey(k.z)),
                                             __uint_as_float(jmorph_unkey(k.w))));
}

// Rows [row0, row0 + n_rows) of the image, columns [x0, x0 + rw): the row extremum into plane rows vrow0 + row of H (rw int4 each).
// An item = one row segment of up to kRowSeg outputs, one wave each; item = row * segs + seg; the waves stride over the items.
// Dynamic LDS: a private region of kRowSeg + 2 R int4 per wave.
template <bool DILATE, bool STRAIGHT>
__global__ __launch_bounds__(kMorphThreads) void k_morph_rows(const uint2* __restrict__ src, int4* __restrict__ hp, uint32_t W, uint32_t x0, uint32_t rw,
                                                              uint32_t row0, uint32_t vrow0, uint32_t R, uint32_t segs, uint32_t region,
                                                              uint32_t total_items, int32_t pad) {
    extern __shared__ int4 morph_lds[];
    const uint32_t wave = jk::uni(threadIdx.x >> 6), lane = jk::lane_id();
    int4* reg = morph_lds + wave * region;
    const uint32_t L = 2u * R + 1u;
    for (uint32_t it = blockIdx.x * kMorphWaves + wave; it < total_items; it += gridDim.x * kMorphWaves) {
        const uint32_t row = it / segs, seg = it - row * segs;
        const uint32_t o0 = seg * kRowSeg, n_out = rw - o0 < kRowSeg ? rw - o0 : kRowSeg;
        const int64_t xs0 = (int64_t)x0 + o0 - R;  // the image column of staged element 0
        const uint32_t n_stage = n_out + 2u * R;   // (<= region)
        const uint2* srow = src ? src + (uint64_t)(row0 + row) * W : nullptr;
        jk::wave_sync();  // (the reads of the item before come first)
        // two texels per lane and step: one 16-B load where the pair is 16-B aligned and inside the row, 8-B loads otherwise
        const bool pair_aligned = srow && (((((uintptr_t)srow) >> 3) + (uint64_t)xs0) & 1u) == 0u;
        for (uint32_t e = 2u * lane; e < n_stage; e += 128u) {
            const int64_t xa = xs0 + e;
            int4 a, b;
            if (pair_aligned && xa >= 0 && xa + 1 < (int64_t)W) {
                const uint4 q = *(const uint4*)(srow + xa);
                a = texel_keys<DILATE, STRAIGHT>(make_uint2(q.x, q.y));
                b = texel_keys<DILATE, STRAIGHT>(make_uint2(q.z, q.w));
            } else {
                a = staged_keys<DILATE, STRAIGHT>(srow, xa, W, pad);
                b = staged_keys<DILATE, STRAIGHT>(srow, xa + 1, W, pad);
            }
            reg[e] = a;
            if (e + 1u < n_stage) reg[e + 1u] = b;
        }
        jk::wave_sync();
        // Doubling in place, ascending: element i of a step reads i and i + w, both at or above i, and the chunk that writes i has
        // read before it writes (the wave_sync between), so no step reads what it has written.  After the steps reg[i] covers the
        // staged elements [i, i + w), for i < n_stage - (w - 1).
        uint32_t w = 1u, n = n_stage;
        while (2u * w <= L) {
            n -= w;
            for (uint32_t base = 0; base < n; base += 64u) {
                const uint32_t i = base + lane;
                int4 v = splat(0);
                if (i < n) v = pick4<DILATE>(reg[i], reg[i + w]);
                jk::wave_sync();
                if (i < n) reg[i] = v;
                jk::wave_sync();
            }
            w *= 2u;
        }
        // output o covers the staged elements [o, o + L): two spans of w, the second starting at o + L - w (<= o + w)
        const uint32_t off = L - w;
        int4* out = hp + (uint64_t)(vrow0 + row) * rw + o0;
        for (uint32_t o = lane; o < n_out; o += 64u) out[o] = pick4<DILATE>(reg[o], reg[o + off]);
    }
}

// What the column kernels know of the planes: rw texels per row, nv rows, of which [vlo, vhi) are rows of the image (the others
// are the padding key and are not loaded: the index is held inside [vlo, vhi), which is never empty, and the value replaced).
struct MorphPlanes {
    uint32_t rw, nv, vlo, vhi;
    uint32_t L;       // 2 ry + 1, the rows of a block
    uint32_t group;   // blocks of an item
    uint32_t strips;  // strips of kColStrip columns
    int32_t pad;
};
JD int4 plane_h(const int4* __restrict__ hp, const MorphPlanes& m, uint32_t v, uint32_t cc) {
    const uint32_t vc = v < m.vlo ? m.vlo : (v >= m.vhi ? m.vhi - 1u : v);
    const int4 h = hp[(uint64_t)vc * m.rw + cc];
    return v == vc ? h : splat(m.pad);
}

// P[v] = op of H over the rows of v's block up to v, for every row of the planes.  An item = `group` blocks x one strip, one wave
// each; item = grp * strips + strip.
template <bool DILATE>
__global__ __launch_bounds__(kColThreads) void k_morph_prefix(const int4* __restrict__ hp, int4* __restrict__ pp, MorphPlanes m, uint32_t total_items) {
    const uint32_t lane = jk::lane_id();
    for (uint32_t it = blockIdx.x; it < total_items; it += gridDim.x) {
        const uint32_t grp = it / m.strips, strip = it - grp * m.strips;
        const uint32_t c = strip * kColStrip + lane;
        const bool active = c < m.rw;
        const uint32_t cc = active ? c : m.rw - 1u;  // (loads of a lane beyond the rectangle stay inside the plane)
        // the item's rows [v0, v1): `group` whole blocks (the last one of the planes may be short), walked as one run of rows so
        // that eight loads are in flight whatever the block length; pos = the row's place in its block
        const uint64_t r0 = (uint64_t)grp * m.group * m.L;  // (< nv: the launcher counts the items)
        const uint32_t v0 = (uint32_t)r0, v1 = (uint32_t)(r0 + (uint64_t)m.group * m.L < m.nv ? r0 + (uint64_t)m.group * m.L : m.nv);
        int4 run = splat(jmorph_neutral(DILATE));
        uint32_t pos = 0u, v = v0;
        for (; v + kRowsInFlight <= v1; v += kRowsInFlight) {
            int4 h[kRowsInFlight];
#pragma unroll
            for (uint32_t k = 0; k < kRowsInFlight; k++) h[k] = plane_h(hp, m, v + k, cc);
#pragma unroll
            for (uint32_t k = 0; k < kRowsInFlight; k++) {
                run = pos == 0u ? h[k] : pick4<DILATE>(run, h[k]);
                if (active) pp[(uint64_t)(v + k) * m.rw + c] = run;
                pos = pos + 1u == m.L ? 0u : pos + 1u;
            }
        }
        for (; v < v1; v++) {
            const int4 h = plane_h(hp, m, v, cc);
            run = pos == 0u ? h : pick4<DILATE>(run, h);
            if (active) pp[(uint64_t)v * m.rw + c] = run;
            pos = pos + 1u == m.L ? 0u : pos + 1u;
        }
    }
}

// The rectangle (x0, y0, rw, rh) of dst (W texels per row): output row v of the rectangle = op(S[v], P[v + L - 1]), S the suffix of
// H over v's block, formed on the way up.  Only the out_blocks blocks that hold an output row are walked; an item = `group` of
// them x one strip.
template <bool DILATE, bool STRAIGHT>
__global__ __launch_bounds__(kColThreads) void k_morph_final(const int4* __restrict__ hp, const int4* __restrict__ pp, uint2* __restrict__ dst, uint32_t W,
                                                               uint32_t x0, uint32_t y0, uint32_t rh, uint32_t out_blocks, MorphPlanes m, uint32_t total_items) {
    const uint32_t lane = jk::lane_id();
    for (uint32_t it = blockIdx.x; it < total_items; it += gridDim.x) {
        const uint32_t grp = it / m.strips, strip = it - grp * m.strips;
        const uint32_t c = strip * kColStrip + lane;
        const bool active = c < m.rw;
        const uint32_t cc = active ? c : m.rw - 1u;
        // the item's blocks [b0, b1) and rows [v0, v1), walked bottom-up as one run of rows; pos = the row's place in its block, and
        // the suffix starts anew below a block's first row.  Row v is an output row when v < rh; then v + L - 1 < nv is a row of P.
        const uint32_t b0 = grp * m.group, b1 = out_blocks - b0 < m.group ? out_blocks : b0 + m.group;  // (b0 < out_blocks)
        const uint32_t v0 = b0 * m.L, v1 = (uint64_t)b1 * m.L < m.nv ? b1 * m.L : m.nv;
        int4 suf = splat(jmorph_neutral(DILATE));
        uint32_t pos = (v1 - 1u - v0) % m.L, v = v1;  // rows [v, v1) are done
        for (; v >= v0 + kRowsInFlight; v -= kRowsInFlight) {
            int4 h[kRowsInFlight], p[kRowsInFlight];
#pragma unroll
            for (uint32_t k = 0; k < kRowsInFlight; k++) {
                const uint32_t vk = v - 1u - k;
                h[k] = plane_h(hp, m, vk, cc);
                p[k] = pp[(uint64_t)jd::umin_(vk + m.L - 1u, m.nv - 1u) * m.rw + cc];  // (a row of P also where vk is no output row)
            }
#pragma unroll
            for (uint32_t k = 0; k < kRowsInFlight; k++) {
                const uint32_t vk = v - 1u - k;
                suf = pick4<DILATE>(suf, h[k]);
                if (vk < rh && active) dst[(uint64_t)(y0 + vk) * W + x0 + c] = stored_texel<STRAIGHT>(pick4<DILATE>(suf, p[k]));
                if (pos == 0u) suf = splat(jmorph_neutral(DILATE));
                pos = pos == 0u ? m.L - 1u : pos - 1u;
            }
        }
        for (; v > v0; v--) {
            const uint32_t vk = v - 1u;
            const int4 h = plane_h(hp, m, vk, cc);
            const int4 p = pp[(uint64_t)jd::umin_(vk + m.L - 1u, m.nv - 1u) * m.rw + cc];
            suf = pick4<DILATE>(suf, h);
            if (vk < rh && active) dst[(uint64_t)(y0 + vk) * W + x0 + c] = stored_texel<STRAIGHT>(pick4<DILATE>(suf, p));
            if (pos == 0u) suf = splat(jmorph_neutral(DILATE));
            pos = pos == 0u ? m.L - 1u : pos - 1u;
        }
    }
}

}  // namespace

// The rectangle r of the RGBA16F image dst = the erosion (dilate = 0) or dilation of the image src of the same size (null texels:
// transparent black; may be dst) by the box of radius_x, radius_y (each <= JMORPH_MAX_RADIUS).  clamp: JH_MORPH_EDGE_CLAMP; straight:
// JH_MORPH_STRAIGHT.  tmp: device memory of jmorph_scratch_bytes(r.w, r.h, radius_y), the planes H and P.  Three launches on
// `stream`.  Returns 0, -1 on arguments it refuses, -2 on a launch error.
extern "C" int jh_morph_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect r, int dilate, int clamp, int straight,
                               uint32_t radius_x, uint32_t radius_y, void* tmp, int num_cus) {
    if (!dst.texels || !tmp || radius_x > JMORPH_MAX_RADIUS || radius_y > JMORPH_MAX_RADIUS) return -1;
    if (src.width != dst.width || src.height != dst.height || !jimage_rect_inside(r, dst.width, dst.height)) return -1;
    if (jimage_rect_empty(r)) return 0;
    const jimage_rows rows = jimage_row_window(r.y, r.h, radius_y, dst.height);
    const uint64_t nv = jmorph_plane_rows(r.h, radius_y);
    if (nv > 0x7fffffffull) return -1;
    MorphPlanes m;
    m.rw = r.w;
    m.nv = (uint32_t)nv;
    m.vlo = rows.row0 + radius_y - r.y;  // the plane row of image row rows.row0
    m.vhi = m.vlo + rows.n_rows;
    m.L = 2u * radius_y + 1u;
    m.group = m.L >= kItemRows ? 1u : (kItemRows + m.L - 1u) / m.L;
    m.strips = (r.w + kColStrip - 1u) / kColStrip;
    m.pad = jmorph_pad(dilate, clamp);
    const uint64_t blocks_all = (nv + m.L - 1u) / m.L, blocks_out = ((uint64_t)r.h + m.L - 1u) / m.L;
    const uint64_t items_rows = (uint64_t)rows.n_rows * ((r.w + kRowSeg - 1u) / kRowSeg);
    const uint64_t items_prefix = ((blocks_all + m.group - 1u) / m.group) * m.strips, items_final = ((blocks_out + m.group - 1u) / m.group) * m.strips;
    if (items_rows > 0x7fffffffull || items_prefix > 0x7fffffffull || items_final > 0x7fffffffull) return -1;
    int4* hp = (int4*)tmp;
    int4* pp = (int4*)((char*)tmp + jmorph_plane_bytes(r.w, r.h, radius_y));
    const uint32_t segs = (r.w + kRowSeg - 1u) / kRowSeg, region = kRowSeg + 2u * radius_x;
    const size_t lds = (size_t)kMorphWaves * region * sizeof(int4);
    const dim3 grid_rows(grid_blocks(items_rows, kMorphWaves, 8u, num_cus)), grid_prefix(grid_blocks(items_prefix, 1u, 32u, num_cus)),
        grid_final(grid_blocks(items_final, 1u, 32u, num_cus));
    with_flag(dilate != 0, [&](auto op) {
        with_flag(straight != 0, [&](auto flag) {
            constexpr bool DILATE = decltype(op)::value, STRAIGHT = decltype(flag)::value;
            hipLaunchKernelGGL((k_morph_rows<DILATE, STRAIGHT>), grid_rows, dim3(kMorphThreads), lds, stream, (const uint2*)src.texels, hp, dst.width, r.x, r.w, rows.row0, m.vlo,
                               radius_x, segs, region, (uint32_t)items_rows, m.pad);
            hipLaunchKernelGGL((k_morph_prefix<DILATE>), grid_prefix, dim3(kColThreads), 0, stream, (const int4*)hp, pp, m, (uint32_t)items_prefix);
            hipLaunchKernelGGL((k_morph_final<DILATE, STRAIGHT>), grid_final, dim3(kColThreads), 0, stream, (const int4*)hp, (const int4*)pp, (uint2*)dst.texels, dst.width, r.x, r.y,
                               r.h, (uint32_t)blocks_out, m, (uint32_t)items_final);
        });
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
