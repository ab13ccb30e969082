// kernels_stats.hip -- jh_stats: the content box, the channel extremes and four 256-bin histograms of a rectangle of an RGBA16F image,
// the device half of the rule in include/jello_hip.h ("Stats") and DESIGN.md 5.22; the content test, the order key, the clamp, the
// LINEAR code, the words of a partial record, their combine and the words of the record come from include/jello_stats.h, the one text
// this file and tools/stats_check.cpp both compile.  Every word of the record is an integer sum, min or max over the SET of texels, so
// any decomposition gives the same bytes.  Two launches, ordered by the stream; no global atomics, no fences, no fill:
//   k_stats         f16 image -> one partial record per workgroup.  The item shape of texel_io.h's pair walk, read only: an item is a
//                   row segment of 2 x 256 texels, a lane owns two neighbouring texels laid on the row's 16-byte grid -- one 16-byte load
//                   for a pair inside the rectangle, an 8-byte load for a row's first or last texel alone -- and the workgroups stride
//                   over the items; the next item's texels are loaded before the current ones are looked at.  A lane keeps the counts,
//                   the box and the keys' min / max in registers; at the end they cross the wave by DPP (kwave.h), the four waves
//                   through LDS.  The bins are uint32_t[4][256] in LDS, zeroed there per workgroup, added to with LDS atomics and copied
//                   to the partial once.  THE CONSTANT IMAGE -- a transparent background puts every lane of every wave on one bin per
//                   channel -- is met with a wave-uniform test: the code of the first active lane, one ballot of "the same", and that
//                   lane adds the popcount; a second round of the same takes the second value of a wave that lies across the edge of a
//                   mask; the lanes left after two rounds add 1 each (DESIGN.md 5.22 has the costs).
//   k_stats_finish  partials -> the record.  A workgroup owns 32 words of the partial layout: 16 groups of 32 lanes walk the partials
//                   16 apart, each lane combining its word (128-byte loads per group), the groups meet in LDS in a fixed order, and
//                   the words leave as the record's (jstats_record_word, jstats_record_bin) in 4-byte vector stores.  Bins are read
//                   only where HISTOGRAM is asked for: a partial's bins are not written otherwise.  Every byte of the record is
//                   written, so the caller's memory needs no fill; nothing of a partial is read that this call did not write.
// k_stats<BOX, HIST, SRGB>: BOX: bounds or extremes are asked for; five instantiations.  channel, threshold and population are scalars.
// VGPRs, LDS, scratch: DESIGN.md 5.22.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_stats.h"
#include "blit_convert.h"
#include "kcommon.h"
#include "texel_io.h"

namespace {

constexpr uint32_t kThreads = 256;     // k_stats: four waves to a workgroup, an item of 512 texels each trip
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kPerCu = 4;         // workgroups to a CU, the rest by grid stride: 1024 partials on 256 CUs (JSTATS_MAX_PARTIALS)
constexpr uint32_t kFinThreads = 512;  // k_stats_finish: kFinGroups groups of kFinWords lanes
constexpr uint32_t kFinWords = 32;
constexpr uint32_t kFinGroups = kFinThreads / kFinWords;
static_assert(JSTATS_W_HIST <= kFinWords && JSTATS_RECORD_HEAD_WORDS <= kFinWords, "the record's head comes from the first workgroup's words");
static_assert(JSTATS_PARTIAL_BYTES % 8u == 0u && (JSTATS_W_HIST * 4u) % 8u == 0u, "the bins of a partial are copied in 8-byte words");

struct StatsArgs {
    const uint2* src;    // the source's texels, or null: never written
    uint32_t* partials;  // gridDim.x partial records
    uint32_t W;          // texels of a row of src
    uint32_t x0, y0, w, h;  // the rectangle
    uint32_t segs, total;   // items of a row, and of the rectangle
    uint32_t channel, population;
    float threshold;
};

// The two texels of the lane in item `it` (zero where it has none): texels c and c + 1 of row `row` of the rectangle.
JD void fetch(const StatsArgs& a, uint32_t it, uint2& ta, uint2& tb) {
    ta = make_uint2(0u, 0u);
    tb = ta;
    if (it >= a.total || !a.src) return;
    const uint32_t row = it / a.segs, seg = it - row * a.segs;
    const uint2* srow = a.src + ((uint64_t)(a.y0 + row) * a.W + a.x0);
    const uint32_t phase = (uint32_t)(((uintptr_t)srow >> 3) & 1u);
    const int64_t c = (int64_t)seg * (2u * kThreads) + 2u * threadIdx.x - phase;
    const bool va = c >= 0 && c < (int64_t)a.w, vb = c + 1 < (int64_t)a.w;
    if (va && vb) {
        const uint4 q = *(const uint4*)(srow + c);  // (on the 16-byte grid: that is what the phase is for)
        ta = make_uint2(q.x, q.y);
        tb = make_uint2(q.z, q.w);
    } else if (va) {
        ta = srow[c];
    } else if (vb) {
        tb = srow[c + 1];
    }
}

// One more in bin `code` for every active lane.  Every lane of the wave calls this (the ballots are the wave's).
JD void bin_add(uint32_t* bins, uint32_t code, bool active) {
    uint64_t rest = __builtin_amdgcn_ballot_w64(active);
    // two rounds of "the code of the first lane left, and everyone who has it": a constant wave is done after one add of one lane, a
    // wave across an edge of a mask after two; what is left then adds lane by lane.  (All the conditions on `rest` are uniform.)
#pragma unroll
    for (uint32_t round = 0; round < 2u; round++) {
        if (rest == 0ull) return;
        const uint32_t lead = (uint32_t)__builtin_ctzll(rest);
        const uint32_t value = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)lead);
        const uint64_t same = __builtin_amdgcn_ballot_w64(active && code == value);
        if (jk::lane_id() == lead) __hip_atomic_fetch_add(bins + value, (uint32_t)__builtin_popcountll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        rest &= ~same;
    }
    if ((rest >> jk::lane_id()) & 1ull) __hip_atomic_fetch_add(bins + code, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct Acc {
    uint32_t content, pop, nan[4];
    uint32_t bx0, by0, bx1, by1;
    uint32_t kmin[4], kmax[4];
};

template <bool BOX, bool HIST, bool SRGB>
JD void texel(const StatsArgs& a, Acc& s, uint32_t* bins, const float2* lut, uint2 t, uint32_t x, uint32_t y, bool valid) {
    const uint32_t h[4] = {t.x & 0xffffu, t.x >> 16, t.y & 0xffffu, t.y >> 16};
    const uint32_t word = (a.channel & 2u) ? t.y : t.x;
    const bool content = valid && jstats_is_content((uint16_t)((a.channel & 1u) ? word >> 16 : word & 0xffffu), a.threshold);
    const bool in_pop = valid && (a.population == (uint32_t)JSTATS_ALL || content);
    s.content += content ? 1u : 0u;
    s.pop += in_pop ? 1u : 0u;
    if (BOX && content) {
        s.bx0 = jd::umin_(s.bx0, x); s.by0 = jd::umin_(s.by0, y);
        s.bx1 = jd::umax_(s.bx1, x + 1u); s.by1 = jd::umax_(s.by1, y + 1u);
    }
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        const bool nan = jstats_is_nan(h[c]);
        s.nan[c] += in_pop && nan ? 1u : 0u;
        if (BOX && in_pop && !nan) {
            const uint32_t k = jstats_key(h[c]);
            s.kmin[c] = jd::umin_(s.kmin[c], k);
            s.kmax[c] = jd::umax_(s.kmax[c], k);
        }
        if (HIST) {
            const float q = jstats_clamp01(jstats_f16((uint16_t)h[c]));
            const uint32_t code = SRGB && c != 3u ? blit_srgb(q, lut) : jstats_linear_code(q);
            bin_add(bins + 256u * c, code, in_pop);
        }
    }
}

// v combined over the wave by word i's operation, in every lane... of interest in lane 63 only; returned as a scalar.
JD uint32_t wave_combine(uint32_t i, uint32_t v) {
    const int op = jstats_word_op(i);
    if (op == JSTATS_OP_SUM) return jk::wave_reduce_u32(v);
    const uint32_t r = op == JSTATS_OP_MIN ? jk::wave_incl_scan_self(v, [](uint32_t p, uint32_t q) { return jd::umin_(p, q); })
                                           : jk::wave_incl_scan_self(v, [](uint32_t p, uint32_t q) { return jd::umax_(p, q); });
    return jk::read_lane(r, 63u);
}

template <bool BOX, bool HIST, bool SRGB>
__global__ __launch_bounds__(kThreads) void k_stats(const StatsArgs a) {
    __shared__ uint32_t bins[HIST ? 1024 : 1];
    __shared__ float2 lut[SRGB ? 256 : 1];
    __shared__ uint32_t red[kWaves][JSTATS_W_HIST];
    if (HIST) {
#pragma unroll
        for (uint32_t i = 0; i < 1024u / kThreads; i++) bins[threadIdx.x + i * kThreads] = 0u;
    }
    if (SRGB) blit_srgb_lut_fill(lut, threadIdx.x);
    if (HIST || SRGB) __syncthreads();
    Acc s;
    s.content = 0u; s.pop = 0u;
    s.bx0 = jstats_word_neutral(JSTATS_W_X0); s.by0 = jstats_word_neutral(JSTATS_W_Y0);
    s.bx1 = jstats_word_neutral(JSTATS_W_X1); s.by1 = jstats_word_neutral(JSTATS_W_Y1);
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        s.nan[c] = 0u;
        s.kmin[c] = jstats_word_neutral(JSTATS_W_MIN + c);
        s.kmax[c] = jstats_word_neutral(JSTATS_W_MAX + c);
    }
    uint2 ta, tb;
    fetch(a, blockIdx.x, ta, tb);
    for (uint32_t it = blockIdx.x; it < a.total; it += gridDim.x) {  // (uniform over the workgroup: every lane reaches every ballot)
        uint2 na, nb;
        fetch(a, it + gridDim.x, na, nb);  // (total + gridDim.x < 2^32: the launcher sees to it)
        const uint32_t row = it / a.segs, seg = it - row * a.segs;
        const uint32_t phase = a.src ? (uint32_t)(((uintptr_t)(a.src + ((uint64_t)(a.y0 + row) * a.W + a.x0)) >> 3) & 1u) : 0u;
        const int64_t c = (int64_t)seg * (2u * kThreads) + 2u * threadIdx.x - phase;
        const bool va = c >= 0 && c < (int64_t)a.w, vb = c + 1 < (int64_t)a.w;
        const uint32_t y = a.y0 + row, x = a.x0 + (uint32_t)c;  // (x of an invalid texel is not looked at)
        texel<BOX, HIST, SRGB>(a, s, bins, lut, ta, x, y, va);
        texel<BOX, HIST, SRGB>(a, s, bins, lut, tb, x + 1u, y, vb);
        ta = na;
        tb = nb;
    }
    // the registers: across the wave, then across the waves
    const uint32_t v[JSTATS_W_HIST] = {s.content, s.bx0, s.by0, s.bx1, s.by1, s.pop, s.nan[0], s.nan[1], s.nan[2], s.nan[3],
                                      s.kmin[0], s.kmin[1], s.kmin[2], s.kmin[3], s.kmax[0], s.kmax[1], s.kmax[2], s.kmax[3]};
    const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)JSTATS_W_HIST; i++) {
        const uint32_t r = wave_combine(i, v[i]);
        if (jk::lane_id() == 0u) red[wave][i] = r;
    }
    __syncthreads();  // (the bins' adds are done as well)
    uint32_t* partial = a.partials + (uint64_t)blockIdx.x * JSTATS_PARTIAL_WORDS;
    if (threadIdx.x < (uint32_t)JSTATS_W_HIST) {
        uint32_t r = red[0][threadIdx.x];
#pragma unroll
        for (uint32_t k = 1; k < kWaves; k++) r = jstats_word_combine(threadIdx.x, r, red[k][threadIdx.x]);
        partial[threadIdx.x] = r;
    }
    if (HIST) {
        uint2* out = (uint2*)(partial + JSTATS_W_HIST);
        const uint2* in = (const uint2*)bins;
#pragma unroll
        for (uint32_t i = 0; i < 512u / kThreads; i++) out[threadIdx.x + i * kThreads] = in[threadIdx.x + i * kThreads];
    }
}

struct FinishArgs {
    const uint32_t* partials;
    uint32_t n;     // partial records
    uint32_t* out;  // the caller's record
    jstats_head hd;
};

__global__ __launch_bounds__(kFinThreads) void k_stats_finish(const FinishArgs a) {
    __shared__ uint32_t sh[kFinGroups][kFinWords];
    __shared__ uint32_t head[kFinWords];
    const uint32_t w = threadIdx.x % kFinWords, g = threadIdx.x / kFinWords;
    const uint32_t i = blockIdx.x * kFinWords + w;  // the word of the partial layout
    const bool live = i < (uint32_t)JSTATS_PARTIAL_WORDS && (i < (uint32_t)JSTATS_W_HIST || (a.hd.what & JSTATS_HISTOGRAM) != 0u);
    uint32_t acc = jstats_word_neutral(i);
    if (live) {
#pragma unroll 8
        for (uint32_t p = g; p < a.n; p += kFinGroups) acc = jstats_word_combine(i, acc, a.partials[(uint64_t)p * JSTATS_PARTIAL_WORDS + i]);
    }
    sh[g][w] = acc;
    __syncthreads();
    if (g == 0u) {
        for (uint32_t k = 1; k < kFinGroups; k++) acc = jstats_word_combine(i, acc, sh[k][w]);  // (a fixed order; the operations commute anyway)
        if (blockIdx.x == 0u) head[w] = acc;
        if (i >= (uint32_t)JSTATS_W_HIST && i < (uint32_t)JSTATS_PARTIAL_WORDS) a.out[JSTATS_RECORD_HEAD_WORDS + (i - JSTATS_W_HIST)] = jstats_record_bin(a.hd, acc);
    }
    if (blockIdx.x != 0u) return;  // (uniform)
    __syncthreads();
    if (threadIdx.x < JSTATS_RECORD_HEAD_WORDS) a.out[threadIdx.x] = jstats_record_word(threadIdx.x, a.hd, head);
}

template <bool BOX, bool HIST, bool SRGB>
void launch_stats(dim3 grid, hipStream_t stream, const StatsArgs& s) {
    hipLaunchKernelGGL((k_stats<BOX, HIST, SRGB>), grid, dim3(kThreads), 0, stream, s);
}

}  // namespace

// The record of the rectangle r of the RGBA16F image src (null texels: transparent black) under desc (legal: jstats_desc_error; r of
// at most 2^31 texels) into `out`: sizeof(jh_stats_record) bytes of device memory on an 8-byte boundary.  tmp: device memory of
// jstats_scratch_bytes(r) on an 8-byte boundary, the partials (not looked at for an image without texels, which is one launch).  Two
// launches on `stream`.  Returns 0, -1 on arguments it refuses, -2 on a launch error.
extern "C" int jh_stats_launch(hipStream_t stream, jimage_src src, jimage_rect r, const jh_stats_desc* desc, void* out, void* tmp, int num_cus) {
    static_assert(sizeof(jh_stats_record) == 4u * (JSTATS_RECORD_HEAD_WORDS + 1024u), "the record's words are the rule's");
    if (!out || ((uintptr_t)out & 7u) != 0u || !desc || jstats_desc_error(desc)) return -1;
    if (!jimage_rect_inside(r, src.width, src.height) || (uint64_t)r.w * r.h > JSTATS_MAX_TEXELS) return -1;
    FinishArgs f;
    f.partials = (const uint32_t*)tmp;
    f.n = 0u;
    f.out = (uint32_t*)out;
    f.hd = {r.x, r.y, r.w, r.h, desc->what, (uint32_t)desc->population, (uint32_t)desc->transfer};
    if (!jimage_rect_empty(r)) {
        if (!tmp || ((uintptr_t)tmp & 7u) != 0u) return -1;
        StatsArgs s;
        s.src = (const uint2*)src.texels;
        s.partials = (uint32_t*)tmp;
        s.W = src.width;
        s.x0 = r.x; s.y0 = r.y; s.w = r.w; s.h = r.h;
        const uint64_t segs = walk_segs(r.w, kThreads), items = segs * r.h;
        if (items > 0xf0000000ull) return -1;  // (at most 2^31 / 512 + 2^31 for a legal rectangle)
        s.segs = (uint32_t)segs;
        s.total = (uint32_t)items;
        s.channel = (uint32_t)desc->channel;
        s.population = (uint32_t)desc->population;
        s.threshold = desc->threshold;
        uint32_t blocks = grid_blocks(items, 1u, kPerCu, num_cus);
        if (blocks > JSTATS_MAX_PARTIALS) blocks = JSTATS_MAX_PARTIALS;
        f.n = blocks;
        const dim3 grid(blocks);
        const bool box = (desc->what & (JSTATS_BOUNDS | JSTATS_EXTREMES)) != 0u, hist = (desc->what & JSTATS_HISTOGRAM) != 0u;
        if (!hist) {
            launch_stats<true, false, false>(grid, stream, s);
        } else {
            with_flag(box, [&](auto b) {
                with_flag(desc->transfer == JSTATS_SRGB, [&](auto t) { launch_stats<decltype(b)::value, true, decltype(t)::value>(grid, stream, s); });
            });
        }
    }
    hipLaunchKernelGGL(k_stats_finish, dim3((JSTATS_PARTIAL_WORDS + kFinWords - 1u) / kFinWords), dim3(kFinThreads), 0, stream, f);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
