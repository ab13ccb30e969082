// kwave.h -- the wave64 cross-lane primitives of every jello_amd kernel (device only; kcommon.h includes it): the DPP control
// words, one typed DPP move, the step table of a wave scan stated once, scans and neighbour reads on top of it, typed lane reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "dmath.h"

namespace jk {

JD uint32_t lane_id() { return threadIdx.x & 63u; }
JD uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }  // a value that is the same in every lane, as a scalar
JD uint64_t uni(uint64_t v) { return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32); }
// Orders this wave's LDS accesses (a wave's DS instructions execute in issue order; the fence only has to stop the
// compiler from moving them) -- the synchronisation primitive of kernels whose waves own private LDS regions.
JD void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// Values of any trivially copyable type of whole 32-bit words cross lanes word by word: v with f(i, word i of v) for each word
template <typename T, typename F> JD T map_words(T v, F f) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "lanes exchange whole 32-bit words");
    int w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; i++) w[i] = f(i, w[i]);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// ---- DPP: a VALU operand taken from another lane, no LDS crossbar round trip ----
#define JK_DPP_ROW_SHR(n) (0x110 + (n))  // lane - n of the own 16-lane row
#define JK_DPP_ROW_BCAST15 0x142         // lane 15 of the row below, to every lane of the row
#define JK_DPP_ROW_BCAST31 0x143         // lane 31, to every lane of the upper half
#define JK_DPP_WAVE_SHL1 0x130           // lane + 1 of the wave
#define JK_DPP_WAVE_SHR1 0x138           // lane - 1 of the wave
// v of the lane CTRL names, in the rows of the mask ROWS; `old` where the lane has no source or its row is masked out
template <int CTRL, int ROWS, typename T> JD T dpp_move(T old, T v) {
    int o[sizeof(T) / 4];
    __builtin_memcpy(o, &old, sizeof(T));
    return map_words(v, [&](unsigned i, int w) { return __builtin_amdgcn_update_dpp(o[i], w, CTRL, ROWS, 0xf, false); });
}

// The steps of an inclusive scan over the wave: row_shr 1, 2, 4, 8 inside each 16-lane row, then row_bcast:15 into rows 1 and 3
// and row_bcast:31 into rows 2 and 3.  One VALU instruction per step and word (__shfl_up compiles to ds_bpermute_b32, ~100
// cycles each and six of them dependent).  row_scan_steps: the scan of each row on its own.
template <typename Step> JD void row_scan_steps(Step&& step) {
    step.template operator()<JK_DPP_ROW_SHR(1), 0xf>();
    step.template operator()<JK_DPP_ROW_SHR(2), 0xf>();
    step.template operator()<JK_DPP_ROW_SHR(4), 0xf>();
    step.template operator()<JK_DPP_ROW_SHR(8), 0xf>();
}
template <typename Step> JD void wave_scan_steps(Step&& step) {
    row_scan_steps(step);
    step.template operator()<JK_DPP_ROW_BCAST15, 0xa>();
    step.template operator()<JK_DPP_ROW_BCAST31, 0xc>();
}
// v = op(v, the value from below); a lane without a source takes `fill` for it, or with SELF its own value
template <bool SELF, typename T, typename Op> struct ScanStep {
    T& v;
    const T fill;
    const Op op;
    template <int CTRL, int ROWS> JD void operator()() { v = op(v, dpp_move<CTRL, ROWS>(SELF ? v : fill, v)); }
};
// Inclusive scans over lanes 0..own (row_: within each 16-lane row).  op(own value, value from below) need not be commutative;
// fill: its neutral element.  _self: for an idempotent op (min, max, meet), which needs none.
template <typename T, typename Op> JD T wave_incl_scan(T v, T fill, Op op) { wave_scan_steps(ScanStep<false, T, Op>{v, fill, op}); return v; }
template <typename T, typename Op> JD T wave_incl_scan_self(T v, Op op) { wave_scan_steps(ScanStep<true, T, Op>{v, v, op}); return v; }
template <typename T, typename Op> JD T row_incl_scan(T v, T fill, Op op) { row_scan_steps(ScanStep<false, T, Op>{v, fill, op}); return v; }
JD uint32_t wave_incl_scan_u32(uint32_t v) { return wave_incl_scan(v, 0u, [](uint32_t a, uint32_t b) { return a + b; }); }
JD uint32_t wave_incl_max_u32(uint32_t v) { return wave_incl_scan(v, 0u, [](uint32_t a, uint32_t b) { return jd::umax_(a, b); }); }

// Neighbour reads: v of the lane below / above in the wave, of lane - N in the row; `fill` where there is none
template <typename T> JD T lane_prev(T v, T fill) { return dpp_move<JK_DPP_WAVE_SHR1, 0xf>(fill, v); }
template <typename T> JD T lane_next(T v, T fill) { return dpp_move<JK_DPP_WAVE_SHL1, 0xf>(fill, v); }
template <int N, typename T> JD T row_prev(T v, T fill) { return dpp_move<JK_DPP_ROW_SHR(N), 0xf>(fill, v); }

// Lane reads: v of lane `lane`, for a lane index that is uniform (v_readlane_b32, the result a scalar) or differs per lane
// (_var: ds_bpermute_b32, through the LDS crossbar)
template <typename T> JD T read_lane(T v, uint32_t lane) { return map_words(v, [=](unsigned, int w) { return __builtin_amdgcn_readlane(w, (int)lane); }); }
template <typename T> JD T read_lane_var(T v, uint32_t lane) { return map_words(v, [=](unsigned, int w) { return __builtin_amdgcn_ds_bpermute((int)(lane << 2), w); }); }

}  // namespace jk
