// kernels_dash.hip -- the device stage of the dash rule (include/jello_hip.h "dashing").
//
// Every length, inverse and split is a function of include/jello_dash.h, which the host route compiles too; the kernels only
// decide who evaluates what:
//   k_dash_lengths     one wave per segment, a lane per panel (stride 64): panel lengths on 2^-32 units, summed with integer
//                      LDS atomics into the segment's 32 coarse sums -- the order of the additions cannot matter
//   k_dash_positions   one thread per subpath: the integer positions of its segments, whole / merged
//   k_dash_plan        one thread per segment: how many elements it emits, and whether its lead piece is relocated
//   jh_scan_u32 x 2    exclusive scans of both: because dashes are disjoint and ordered, the scan of the per-segment counts is
//                      already the canonical position (only the merged dash of a closed subpath moves, jdash_place)
//   k_dash_index       the n_paths + 1 exclusive offsets
//   k_dash_emit        one lane per output element (grid-stride over the total, which only the device knows): binary search for
//                      its segment, jdash_emit, a bounds-checked 28-byte store.  A segment that carries thousands of dashes is
//                      thousands of lanes.
// Scratch (slot map in kcommon.h): A the uploaded job, B JDashSegLen per segment, C counts and relocation flags (interleaved,
// n_segs + 1 pairs), D their scans, E JDashSubInfo per subpath.  Everything is written before it is read in every call.
#include "kcommon.h"

#include "../../include/jello_dash.h"

__global__ __launch_bounds__(JL_WG) void k_dash_lengths(JhDashJob job, JDashSegLen* __restrict__ lens) {
    __shared__ unsigned long long coarse[JL_WG / 64][JDASH_COARSE];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * (JL_WG / 64) + w;
    if (lane < JDASH_COARSE) coarse[w][lane] = 0ull;
    __syncthreads();
    const bool live = i < job.n_segs;
    uint32_t panels = 0u;
    if (live) {
        const JDashSeg g = job.segs[i];
        panels = jdash_panels(g);
        const uint32_t bp = jdash_block_panels(panels);
        for (uint32_t k = lane; k < panels; k += 64u) atomicAdd(&coarse[w][k / bp], (unsigned long long)jdash_panel_q32(g, panels, k));
        if (panels == 0u && lane == 0u) coarse[w][0] = (unsigned long long)jdash_line_q32(g);
    }
    __syncthreads();
    if (live) {
        if (lane < JDASH_COARSE) lens[i].coarse[lane] = (panels == 0u) ? 0 : (int64_t)coarse[w][lane];
        if (lane == 0u) {
            int64_t s32 = 0;
            for (int c = 0; c < JDASH_COARSE; c++) s32 += (int64_t)coarse[w][c];
            lens[i].q = jdash_q20_of_q32(s32);
            lens[i].start = 0;
            lens[i].panels = panels;
            lens[i].pad = 0u;
        }
    }
}

__global__ __launch_bounds__(JL_WG) void k_dash_positions(JhDashJob job, JDashSegLen* __restrict__ lens, JDashSubInfo* __restrict__ infos) {
    const uint32_t s = blockIdx.x * JL_WG + threadIdx.x;
    if (s >= job.n_subs) return;
    const JDashSub sub = job.subs[s];
    int64_t pos = 0;
    for (uint32_t i = sub.first_seg; i < sub.first_seg + sub.n_segs; i++) {
        lens[i].start = pos;
        pos += lens[i].q;
    }
    infos[s] = jdash_sub_info(job.pats[sub.pat], job.runs, sub.closed, pos);
}

__global__ __launch_bounds__(JL_WG) void k_dash_plan(JhDashJob job, const JDashSegLen* __restrict__ lens, const JDashSubInfo* __restrict__ infos,
                                                     uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * JL_WG + threadIdx.x;
    if (i > job.n_segs) return;
    uint32_t n = 0u, rel = 0u;
    if (i < job.n_segs) {
        const uint32_t s = job.segs[i].sub;
        const JDashSegPlan pl = jdash_plan(job.pats[job.subs[s].pat], job.runs, infos[s], lens[i]);
        n = jdash_plan_count(pl);
        rel = pl.relocated;
    }
    counts[2u * i] = n;  // (entry n_segs: the scans' totals land behind the last segment)
    counts[2u * i + 1u] = rel;
}

__global__ __launch_bounds__(JL_WG) void k_dash_index(JhDashJob job, const uint32_t* __restrict__ base, uint32_t* __restrict__ index) {
    const uint32_t p = blockIdx.x * JL_WG + threadIdx.x;
    if (p <= job.n_paths) index[p] = base[job.path_first_seg[p]];
}

__global__ __launch_bounds__(JL_WG) void k_dash_emit(JhDashJob job, const JDashSegLen* __restrict__ lens, const JDashSubInfo* __restrict__ infos,
                                                     const uint32_t* __restrict__ base, const uint32_t* __restrict__ rbase,
                                                     JDashEl* __restrict__ out, uint64_t capacity) {
    const uint32_t total = base[job.n_segs];
    for (uint64_t j64 = (uint64_t)blockIdx.x * JL_WG + threadIdx.x; j64 < total; j64 += (uint64_t)gridDim.x * JL_WG) {
        const uint32_t j = (uint32_t)j64;
        // the segment that holds element j: the last i with base[i] <= j (segments that emit nothing share their successor's base)
        uint32_t lo = 0u, hi = job.n_segs;  // base[lo] <= j < base[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (base[mid] <= j) lo = mid; else hi = mid;
        }
        const uint32_t i = lo;
        const JDashSeg g = job.segs[i];
        const JDashSub sub = job.subs[g.sub];
        const JDashPat pat = job.pats[sub.pat];
        const JDashSegLen len = lens[i];
        const JDashSegPlan pl = jdash_plan(pat, job.runs, infos[g.sub], len);
        const uint32_t r = j - base[i];
        const uint32_t first = sub.first_seg, end = sub.first_seg + sub.n_segs;
        const uint32_t at = base[first] + jdash_place(pl, r, base[i] - base[first], rbase[i] - rbase[first], rbase[end] - rbase[first],
                                                       base[end] - base[first]);
        if ((uint64_t)at < capacity) out[at] = jdash_emit(g, len, pat, job.runs, pl, r);
    }
}

// Enqueues the whole stage on L.stream; `job` points into the uploaded job (jh_dash, jello_hip.cpp).
JhResult jh_dash_launch(const JhLaunch& L, const JhDashJob& job, void* out, uint64_t capacity, uint32_t* index) {
    const uint64_t n1 = (uint64_t)job.n_segs + 1u;
    JDashSegLen* lens = (JDashSegLen*)jh_scratch_get(L.scratch, JH_SCR_B, n1 * sizeof(JDashSegLen));
    uint32_t* counts = (uint32_t*)jh_scratch_get(L.scratch, JH_SCR_C, n1 * 8u);
    uint32_t* scans = (uint32_t*)jh_scratch_get(L.scratch, JH_SCR_D, n1 * 8u);
    JDashSubInfo* infos = (JDashSubInfo*)jh_scratch_get(L.scratch, JH_SCR_E, ((uint64_t)job.n_subs + 1u) * sizeof(JDashSubInfo));
    if (!lens || !counts || !scans || !infos) return JH_L_SCRATCH;
    uint32_t* base = scans;
    uint32_t* rbase = scans + n1;
    const uint32_t wg = JL_WG;
    hipLaunchKernelGGL(k_dash_lengths, dim3((job.n_segs + 3u) / 4u), dim3(wg), 0, L.stream, job, lens);
    hipLaunchKernelGGL(k_dash_positions, dim3((job.n_subs + wg - 1u) / wg), dim3(wg), 0, L.stream, job, lens, infos);
    hipLaunchKernelGGL(k_dash_plan, dim3((uint32_t)((n1 + wg - 1u) / wg)), dim3(wg), 0, L.stream, job, lens, infos, counts);
    JhResult r = jh_scan_u32(L, counts, 2u, base, (uint32_t)n1, nullptr, nullptr);
    if (r != JH_L_OK) return r;
    r = jh_scan_u32(L, counts + 1, 2u, rbase, (uint32_t)n1, nullptr, nullptr);
    if (r != JH_L_OK) return r;
    hipLaunchKernelGGL(k_dash_index, dim3((job.n_paths + 1u + wg - 1u) / wg), dim3(wg), 0, L.stream, job, base, index);
    hipLaunchKernelGGL(k_dash_emit, dim3(L.cus() * 8u), dim3(wg), 0, L.stream, job, lens, infos, base, rbase, (JDashEl*)out, capacity);
    return JH_L_OK;
}
