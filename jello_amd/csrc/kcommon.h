// kcommon.h -- shared device helpers: bounds-checked buffer views (the WGSL robust-access rule:
// out-of-range reads give zero, writes are dropped -- also what keeps a malformed scene from
// faulting the GPU), wave64/LDS block scans (on kwave.h), and the launcher declarations used by jello_hip.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jello_formats.h"
#include "../../include/jello_image.h"
#include "dmath.h"
#include "kwave.h"

#define JL_WG 256

namespace jk {

template <typename T>
struct Buf {
    T* p;
    uint32_t n;  // element count
    JD T rd(uint32_t i) const {
        if (i < n) return p[i];
        T z;
        __builtin_memset(&z, 0, sizeof(T));
        return z;
    }
    JD void wr(uint32_t i, const T& v) const {
        if (i < n) p[i] = v;
    }
    JD bool ok(uint32_t i) const { return i < n; }
};

template <typename T>
static inline Buf<T> mkbuf(void* p, uint64_t bytes) {
    Buf<T> b;
    b.p = (T*)p;
    uint64_t n = bytes / sizeof(T);
    b.n = n > 0xffffffffull ? 0xffffffffu : (uint32_t)n;
    return b;
}

// [p, p + n) of a bump counter for every ACTIVE lane of the wave, with ONE atomic: the lanes are served value by value (the
// lanes of a call site mostly ask for the same n: one round), a lane's offset = what the rounds before it and the lanes below
// it in its own round take.  By hand, because LLVM's atomic optimizer in its DPP strategy -- which does the same with a wave
// prefix sum -- returned wrong offsets for flatten's call sites (divergent branches inside loops; test_c2_blobs_all_joins_caps_evenodd
// failed with it and passes with the strategies None and Iterative), and None means 64 atomics per call.  The build no longer
// passes that strategy (round 6, csrc/Makefile); jh_selftest_atomics holds whatever the compiler does with this function and
// with the plain per-lane form to a serial sum.
JD uint32_t wave_bump(uint32_t* ctr, uint32_t n) {
    const uint64_t below = (1ull << lane_id()) - 1ull;
    uint64_t todo = __builtin_amdgcn_ballot_w64(true);
    const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
    uint32_t off = 0u, total = 0u;
    while (todo != 0ull) {  // uniform among the active lanes
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)n, __builtin_ctzll(todo));
        const uint64_t m = __builtin_amdgcn_ballot_w64(n == v);
        if (n == v) off = total + v * (uint32_t)__builtin_popcountll(m & below);
        total += v * (uint32_t)__builtin_popcountll(m);
        todo &= ~m;
    }
    uint32_t p = 0u;
    if (lane_id() == leader) p = atomicAdd(ctr, total);
    return (uint32_t)__builtin_amdgcn_readlane((int)p, (int)leader) + off;
}
JD uint32_t wave_reduce_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(v), 63);
}

// Exclusive scan of one u32 per thread across a 256-thread block.  `sh` needs 5 words.
// Returns the exclusive prefix; *total receives the block sum.
JD uint32_t block_excl_scan_u32(uint32_t v, uint32_t* sh, uint32_t* total) {
    uint32_t incl = wave_incl_scan_u32(v);
    uint32_t w = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 63u) sh[w] = incl;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        uint32_t s = sh[i];
        if (i < w) base += s;
    }
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    return base + incl - v;
}

// K-word monoid (component-wise u32 add): exclusive block scan.  sh needs 4*K words.
template <int K>
struct MonoidK {
    uint32_t v[K];
};
template <int K>
JD MonoidK<K> monoid_add(const MonoidK<K>& a, const MonoidK<K>& b) {
    MonoidK<K> c;
#pragma unroll
    for (int i = 0; i < K; i++) c.v[i] = a.v[i] + b.v[i];
    return c;
}
template <int K>
JD MonoidK<K> block_excl_scan_monoid(const MonoidK<K>& in, uint32_t* sh, MonoidK<K>* total) {
    MonoidK<K> incl;
#pragma unroll
    for (int i = 0; i < K; i++) incl.v[i] = wave_incl_scan_u32(in.v[i]);
    uint32_t w = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 63u) {
#pragma unroll
        for (int i = 0; i < K; i++) sh[w * K + i] = incl.v[i];
    }
    __syncthreads();
    MonoidK<K> out, tot;
#pragma unroll
    for (int i = 0; i < K; i++) {
        uint32_t base = 0, t = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            uint32_t s = sh[j * K + i];
            if (j < w) base += s;
            t += s;
        }
        out.v[i] = base + incl.v[i] - in.v[i];
        tot.v[i] = t;
    }
    *total = tot;
    return out;
}
template <int K>
JD MonoidK<K> block_reduce_monoid(const MonoidK<K>& in, uint32_t* sh) {
    MonoidK<K> r = in;
#pragma unroll
    for (int i = 0; i < K; i++) r.v[i] = wave_reduce_u32(r.v[i]);
    uint32_t w = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 0u) {
#pragma unroll
        for (int i = 0; i < K; i++) sh[w * K + i] = r.v[i];
    }
    __syncthreads();
    MonoidK<K> t;
#pragma unroll
    for (int i = 0; i < K; i++) t.v[i] = sh[i] + sh[K + i] + sh[2 * K + i] + sh[3 * K + i];
    return t;
}

// shared/pathtag.wgsl:58-71
JD MonoidK<5> reduce_tag(uint32_t tag_word) {
    MonoidK<5> c;
    uint32_t point_count = tag_word & 0x3030303u;
    c.v[1] = __popc((point_count * 7u) & 0x4040404u);          // pathseg_ix
    c.v[0] = __popc(tag_word & (0x20u * 0x1010101u));           // trans_ix
    uint32_t n_points = point_count + ((tag_word >> 2) & 0x1010101u);
    uint32_t a = n_points + (n_points & (((tag_word >> 3) & 0x1010101u) * 15u));
    a += a >> 8;
    a += a >> 16;
    c.v[2] = a & 0xffu;                                          // pathseg_offset
    c.v[4] = __popc(tag_word & (0x10u * 0x1010101u));            // path_ix
    c.v[3] = __popc(tag_word & (0x40u * 0x1010101u)) * 2u;       // style_ix
    return c;
}
JD void store_tm(JlTagMonoid* dst, const MonoidK<5>& m) {
    dst->trans_ix = m.v[0]; dst->pathseg_ix = m.v[1]; dst->pathseg_offset = m.v[2]; dst->style_ix = m.v[3]; dst->path_ix = m.v[4];
}
JD MonoidK<5> load_tm(const Buf<JlTagMonoid>& b, uint32_t i) {
    JlTagMonoid t = b.rd(i);
    MonoidK<5> m;
    m.v[0] = t.trans_ix; m.v[1] = t.pathseg_ix; m.v[2] = t.pathseg_offset; m.v[3] = t.style_ix; m.v[4] = t.path_ix;
    return m;
}
// pathtag_scan.wgsl (small variant): the prefix of workgroup wg = the sum of the wg entries of `parent` in front of it (sh: 20 words)
JD MonoidK<5> parent_prefix(const Buf<JlTagMonoid>& parent, uint32_t wg, uint32_t* sh) {
    MonoidK<5> agg;
#pragma unroll
    for (int i = 0; i < 5; i++) agg.v[i] = 0;
    if (threadIdx.x < wg) agg = load_tm(parent, threadIdx.x);
    return block_reduce_monoid<5>(agg, sh);
}
// shared/drawtag.wgsl:46-53
JD MonoidK<4> map_draw_tag(uint32_t t) {
    MonoidK<4> c;
    c.v[0] = (t != 0u) ? 1u : 0u;
    c.v[1] = t & 1u;
    c.v[2] = (t >> 2) & 7u;
    c.v[3] = (t >> 6) & 0xfu;
    return c;
}

}  // namespace jk

// ------------------------------------------------------------------------------------------------
// Host-side launcher interface (implemented in the kernels_*.hip files, called by jello_hip.cpp)
// ------------------------------------------------------------------------------------------------
struct JhBound {
    void* ptr;
    uint64_t size;  // bytes
    uint32_t width, height;
    int format;
};

// fine's image array: up to JH_FINE_INLINE_IMAGES descriptors travel in the kernel arguments, larger arrays as a device table
#define JH_FINE_INLINE_IMAGES 8
struct JhImageDesc {
    const void* ptr;  // RGBA8 texels, row-major; nullptr = never written (samples as transparent black)
    uint32_t width, height;
    uint32_t srgb;    // 1: JL_RGBA8_SRGB (decode to linear when sampled)
    uint32_t pad;
};

// ---- scratch arrays ----
// Per-context device arrays the launchers keep between kernels of a stage.  The slot NUMBERS are fixed: every slot's array
// starts slot * JH_SCR_SKEW bytes into its allocation, a measured tuning of k_flatten_lines (jh_scratch_get).  A..J are
// shared between stages on purpose -- a stage is done with its arrays when the next one starts, and the big ones of
// flatten sit where path_count's do, so a frame allocates them once:
//
//   slot      flatten           binning     tile_alloc  backdrop_dyn  path_count                 coarse               fine         jh_pack_tiles
//             (jh_dash, a call outside the frame's stages, uses A: the uploaded job, B: lengths / segment, C: counts and relocation
//              flags / segment, D: their scans, E: whole / merged / subpath, and SCAN_TMP through jh_scan_u32)
//   SCAN_TMP  (jh_scan_u32's control words and tile descriptors, whichever stage scans: flatten, path_count)   self-cleaned
//   A         counts / slot     wg totals   counts      wide list     sums / wave of 64 lines    counts + wg totals
//                                                                     + the number of such waves
//   B         bases / slot                  wg totals                 bases / wave of 64 lines   scratch PTCL (clips)
//             (path_count kept a count and a base per LINE here until its scan went over the wave sums: 2 x 4 B x the line buffer's
//              capacity; A and B are now as large as flatten's tag slots or coarse make them)
//   C         FlTemp.sinfo                                            tile_of / crossing         relocation side arrays
//   D         FlTemp.recs                                             list / crossing                                 clip levels
//   E                                                                 list_base / tile
//   F         item list                                               keys / crossing
//   G                                                                 dense tiles
//   H                                                                                                                               class / tile
//   I                                                                 path ranges + gate
//   J                                                                                                                               (solid, raw) / workgroup
//   FL_CTR    list counters / chunk fills                                                                            self-cleaned
//   BD_CTR                                              wide counter  (zeroed by k_pc_count)                         self-cleaned
//   PC_TOT                                                            crossings per path                             self-cleaned
//   BLUR      (jh_blur, a call outside the frame's stages: the binary32 rows between its two passes -- a slot of its own, so that a
//              frame between two blurs of one size never makes it grow and a captured blur stays valid)
//   RESAMPLE  (jh_resample, likewise: the binary32 rows between its two passes, source-rectangle rows x destination width x 16 B)
//   RESAMPLE_TAPS  (jh_resample: the uploaded window and tap tables of both axes for ONE geometry -- content that a captured call
//              reads on every replay, so nothing else may write the slot; the context keeps the key of what it holds)
//   COLOR_TABLES   (jh_color_filter, the same contract: the uploaded PRE and POST tables of ONE key, 3 x 65 536 floats then
//              4 x 65 536 f16 bit patterns, 1.25 MB; a call that needs no tables does not touch the slot)
//   LIGHT_TABLES   (jh_lighting, the contract of COLOR_TABLES: the uploaded power tables of ONE key, 4097 floats for the specular
//              exponent then 4097 for the spot exponent, 32.8 KB; a call that needs no table does not touch the slot)
//   TURB_TABLES    (jh_turbulence, the same contract: the uploaded tables of ONE seed as the kernel reads them, 2048 floats of
//              gradients laid out [lattice value][channel][2] then the 256 bytes of the selector, 8.25 KB)
//   MORPH     (jh_morphology, as BLUR: the two planes of order keys between its three passes, each (rect height + 2 radius_y) x
//              rect width x 16 B; it only grows and nothing else writes it, so a captured call stays valid)
//   DISTANCE  (jh_distance, as MORPH: the one or two planes of uint16_t run lengths between its two passes, each rect height x
//              (rect width + 2 max_distance) x 2 B; it only grows and nothing else writes it, so a captured call stays valid)
//   STATS     (jh_stats: the partial records between its two launches, JSTATS_MAX_PARTIALS x JSTATS_PARTIAL_BYTES = 4.07 MiB whatever
//              the image -- the grid cap of the largest device -- so one eager call makes every later call capturable; every word that
//              is read was written by the same call's first launch)
enum {
    JH_SCR_SCAN_TMP = 0,
    JH_SCR_A = 1,
    JH_SCR_B = 2,
    JH_SCR_C = 3,
    JH_SCR_D = 4,
    JH_SCR_E = 5,
    JH_SCR_F = 6,
    JH_SCR_G = 7,
    JH_SCR_H = 8,  // jh_pack_tiles (after the frame: shared with no stage)
    JH_SCR_I = 9,
    JH_SCR_J = 10,  // jh_pack_tiles
    JH_SCR_FL_CTR = 11,  // flatten's list counters / chunk fills: NOT shared with other stages (they survive between frames)
    JH_SCR_BD_CTR = 12,  // backdrop's wide-row counter: likewise
    JH_SCR_PC_TOT = 13,  // path_count's crossings per path (atomic sums): likewise, zeroed by the stage's last kernel
    JH_SCR_BLUR = 14,    // jh_blur's intermediate
    JH_SCR_RESAMPLE = 15,       // jh_resample's intermediate
    JH_SCR_RESAMPLE_TAPS = 16,  // jh_resample's tables
    JH_SCR_COLOR_TABLES = 17,   // jh_color_filter's tables
    JH_SCR_MORPH = 18,          // jh_morphology's intermediate planes
    JH_SCR_LIGHT_TABLES = 19,   // jh_lighting's tables
    JH_SCR_TURB_TABLES = 20,    // jh_turbulence's tables
    JH_SCR_DISTANCE = 21,       // jh_distance's intermediate planes
    JH_SCR_STATS = 22,          // jh_stats's partial records
    JH_SCR_COUNT = 23
};
struct JhScratch;  // per-context scratch allocator, defined in jello_hip.cpp
void* jh_scratch_get(JhScratch* s, int slot, uint64_t bytes);  // grows on demand, returns device pointer (nullptr on OOM)
uint64_t jh_scratch_cap(JhScratch* s, int slot);               // bytes the slot holds (>= what was last asked for)
// Self-cleaned counters (SCAN_TMP, FL_CTR, BD_CTR, PC_TOT): counters a stage needs zeroed when it starts are zeroed by the
// LAST kernel that runs before without using them (the stage's own last kernel of the frame before, or a kernel of the
// stage in front) instead of by a fill launch of ~4.4 us; a host-side flag per counter says whether that has happened since
// the counter was last used.  A stage that finds its flag down (first frame, an aborted frame, a stage run on its own, a
// scratch reallocation) fills as before.
// The slot <-> flag table (JH_CLEAN_*) is the allocator's, in jello_hip.cpp; launchers see the two calls below.
//   jh_scratch_acquire: jh_scratch_get + zero the first min(fill_bytes, capacity) bytes on `stream` if the flag is down;
//                       lowers the flag (the counters are in use).  nullptr, and nothing else done, on OOM.
//   jh_scratch_left_clean: a kernel that zeroes the counters again has been enqueued -- raises the flag.
#define JH_FILL_CAPACITY (~0ull)
void* jh_scratch_acquire(JhScratch* s, int slot, uint64_t bytes, uint64_t fill_bytes, hipStream_t stream);
void jh_scratch_left_clean(JhScratch* s, int slot);

// What the dispatcher held back in front of this command and the launcher does in passing (jello_hip.cpp, "held-back
// commands").  All false / zero when nothing was.
struct JhAbsorbed {
    bool bbox_clear;    // flatten: bbox_clear
    bool bump_clear;    // flatten: the recording's Clear(bump)
    bool pathtag_scan;  // flatten: the last pathtag scan -- the classification kernel produces the tag monoids in passing
    JhBound scan_reduced;    //   ... its `reduced` binding,
    uint32_t scan_wgs;       //   its workgroup count,
    bool scan_small;         //   pathtag_scan_small (else _large)
    bool reduce2;              // pathtag_scan1: pathtag_reduce2
    uint32_t reduce2_entries;  //   ... its workgroup count = the entries of reduced2 it would have written
    bool write_indirect;   // path_count / path_tiling: their setup command -- the kernel writes the indirect count itself
    JhBound tiling_ptcl;   // path_tiling: path_tiling_setup's ptcl binding (ptcl[0] = ~0 on failure)
};
// The same for flatten as the flag word k_flatten_classify takes as a kernel argument (device-visible: the values stay)
enum { JH_ABSORB_BBOX_CLEAR = 1u, JH_ABSORB_BUMP_CLEAR = 2u, JH_ABSORB_PATHTAG_SCAN = 8u };

struct JhLaunch {
    hipStream_t stream;
    JhScratch* scratch;
    uint32_t gx, gy, gz;
    const JhBound* b;  // at least the stage's minimum binding count (checked by the dispatcher against the stage table)
    int nb;
    const JhBound* images;  // JH_BIND_IMAGE_ARRAY contents for fine
    int n_images;
    const uint32_t* indirect;  // device pointer to IndirectCount (indirect dispatch) or nullptr
    int num_cus;
    const JlConfig* cfg_host;  // host shadow of the uploaded ConfigUniform bound at index 0, or nullptr
    uint32_t band_row0, band_row1;  // jh_set_band: bin rows [row0, row1) this context writes PTCL for and rasterises (0, ~0u = all)
    const JhImageDesc* image_table;  // device table of all n_images descriptors when n_images > JH_FINE_INLINE_IMAGES, else nullptr
    uint32_t clip_depth_hint;  // jh_set_clip_depth_hint: upper bound of the clip layers' nesting depth, 0 = unknown
    uint32_t* hint_overflow;   // device counter of the blend-stack saves dropped because that hint was too small (or nullptr)
    uint32_t debug_flatten;    // jh_debug_flatten_regions (tests): bit 0 = every wave of k_flatten_items starts in region 0 of the temporary, bit 1 = always 8 regions, bit 2 = batches allocate job by job, bit 3 = k_flatten_items runs as one workgroup
    JhAbsorbed absorbed;

    template <typename T> jk::Buf<T> buf(int slot) const { return jk::mkbuf<T>(b[slot].ptr, b[slot].size); }
    template <typename T> T* ptr(int slot) const { return (T*)b[slot].ptr; }
    uint32_t cus() const { return (uint32_t)(num_cus > 0 ? num_cus : 256); }
};

enum JhResult { JH_L_OK = 0, JH_L_BAD_BINDINGS, JH_L_SCRATCH };  // mapped to JH_ERR_* and a message by the dispatcher

// Generic device-side exclusive scan of u32 (stride in words between consecutive inputs).
// n is read from *n_dev when n_dev != nullptr (clamped to n_max), else n_max.  Writes out[0..n) and
// *total_dev (if non-null).  One launch (decoupled look-back).
JhResult jh_scan_u32(const JhLaunch& L, const uint32_t* in, uint32_t in_stride, uint32_t* out, uint32_t n_max, const uint32_t* n_dev,
                     uint32_t* total_dev);

// jh_dash (kernels_dash.hip): the uploaded job as device pointers (the structs: include/jello_dash.h), and the launcher that
// enqueues the stage's kernels on L.stream.  JH_L_SCRATCH when a scratch array could not be had; nothing is enqueued then.
struct JDashSeg;
struct JDashSub;
struct JDashPat;
struct JDashRun;
struct JhDashJob {
    const JDashSeg* segs;
    const JDashSub* subs;
    const JDashPat* pats;
    const JDashRun* runs;
    const uint32_t* path_first_seg;  // n_paths + 1
    uint32_t n_segs, n_subs, n_paths;
};
JhResult jh_dash_launch(const JhLaunch& L, const JhDashJob& job, void* out, uint64_t capacity, uint32_t* index);

// jh_resample (kernels_resample.hip): the tables of one geometry as the host lays them out (jello_hip.cpp builds and uploads them)
// and the kernels read them.  Windows are relative to the source rectangle.
#define JH_RESAMPLE_ROW_SEG 64u  // outputs of a row-pass item: one per lane of a wave
// A staged source span in LDS: texel t sits at float4 index t + t / 16, so that lanes whose windows start 16 texels apart (the 16:1
// limit) are 272 bytes apart instead of 256 and a ds_read_b128 of 16 lanes covers all 64 banks.
__host__ __device__ __forceinline__ uint32_t jh_resample_skew(uint32_t t) { return t + (t >> 4); }
struct JhResampleTables {
    const uint2* win_x;  // per output column: {first source column, taps}
    const uint4* seg_x;  // per segment of JH_RESAMPLE_ROW_SEG output columns: {first source column any of them reads, columns they span, most taps of one, 0}
    const float* w_x;    // tap j of output column o at w_x[j * dst_w + o] (the lanes of a wave read neighbouring words); zero where o has fewer taps
    const uint2* win_y;  // per output row: {first source row, taps}
    const float* w_y;    // tap j of output row o at w_y[o * stride_y + j]
    uint32_t taps_x, stride_y;  // the largest tap count of an output column / row
    uint32_t region_x;          // float4 slots of LDS a wave of the row pass needs: jh_resample_skew(longest span - 1) + 1
};

// The launchers outside the stage table, each documented at its definition (kernels_surface, _yuv, _pack, _blur, _composite, _resample, _color, _morph, _warp, _convolve, _lighting, _turbulence, _displace, _shadow, _perspective, _distance, _stats, _selftest .hip).  Declared
// here and nowhere else: the file that defines one and the file that calls it both include this, so a signature that changes on one
// side only does not compile.  int results: 0, -1 for arguments the launcher refuses (an image launcher, which takes the views and resolved
// rectangles of include/jello_image.h: a rectangle that is not inside its image), another negative value (-2) for a failed launch.
// jh_warp_launch, jh_displace_launch and jh_perspective_launch share warp_taps.h: one argument block, one ladder, each its own position rule.
extern "C" {
int jh_blit_launch(hipStream_t stream, const void* src, void* dst, uint64_t pitch, uint32_t width, uint32_t row0, uint32_t row1, int format,
                   int num_cus);
int jh_blit_yuv_launch(hipStream_t stream, const void* src, void* const* planes, const uint64_t* pitches, uint32_t width, uint32_t height,
                       uint32_t row0, uint32_t row1, int layout, int matrix, int range, int transfer, int num_cus);
uint32_t jh_pack_groups(uint32_t n_tiles, uint32_t* run_out);
int jh_pack_launch(hipStream_t stream, const void* src, uint64_t src_pitch, const void* ref, uint64_t ref_pitch, uint32_t width, uint32_t height,
                   uint32_t texel_bytes, void* dst, void* cls, void* totals);
int jh_unpack_launch(hipStream_t stream, const void* pack, uint64_t pack_bytes, void* dst, uint64_t dst_pitch, uint32_t width, uint32_t height,
                     uint32_t texel_bytes, uint32_t* rejects);
int jh_blur_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect rect, int clamp, const float* taps_x, uint32_t radius_x,
                   const float* taps_y, uint32_t radius_y, void* tmp, int num_cus);
struct jcomp_rect;  // include/jello_composite.h
int jh_composite_launch(hipStream_t stream, jimage_src src, jimage_dst dst, int dst_has_content, const jcomp_rect* rect, uint32_t mode,
                        uint32_t flags, float opacity, const float* tint, int num_cus);
int jh_resample_launch(hipStream_t stream, jimage_src src, jimage_rect src_rect, jimage_dst dst, jimage_rect dst_rect, int straight,
                       const JhResampleTables* tables, void* tmp, int num_cus);
int jh_color_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect rect, const float* matrix, int clamp, const float* pre,
                    const uint16_t* const* post, int num_cus);
int jh_morph_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect rect, int dilate, int clamp, int straight, uint32_t radius_x,
                    uint32_t radius_y, void* tmp, int num_cus);
int jh_warp_launch(hipStream_t stream, jimage_src src, jimage_rect src_rect, jimage_dst dst, jimage_rect dst_rect, const int64_t* plan, int filter,
                   int edge, int straight, int num_cus);
int jh_convolve_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect rect, uint32_t order_x, uint32_t order_y, uint32_t target_x,
                       uint32_t target_y, const float* weights, int edge, int mode, float bias, int num_cus);
struct jh_light_plan;  // include/jello_hip.h
int jh_lighting_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect rect, int kind, int light, const jh_light_plan* plan,
                       float surface_scale, float constant, const float* color, const float* spec_table, const float* spot_table, int num_cus);
struct jh_turb_plan;  // include/jello_hip.h
int jh_turbulence_launch(hipStream_t stream, jimage_dst dst, jimage_rect rect, int kind, uint32_t octaves, const jh_turb_plan* plan, const void* tables,
                         int num_cus);
int jh_displace_launch(hipStream_t stream, jimage_src src, jimage_rect src_rect, jimage_src map, jimage_dst dst, jimage_rect dst_rect, const int64_t* plan,
                       float scale_x, float scale_y, int x_channel, int y_channel, int filter, int edge, int straight, int num_cus);
struct jh_shad_plan;  // include/jello_hip.h
int jh_shadow_launch(hipStream_t stream, jimage_dst dst, int dst_has_content, jimage_rect rect, const jh_shad_plan* plan, const float* color,
                     uint32_t flags, int num_cus);
int jh_perspective_launch(hipStream_t stream, jimage_src src, jimage_rect src_rect, jimage_dst dst, jimage_rect dst_rect, const double* plan, int filter,
                          int edge, int straight, int num_cus);
struct jh_distance_desc;  // include/jello_hip.h
int jh_distance_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect rect, const jh_distance_desc* desc, void* tmp, int num_cus);
struct jh_stats_desc;  // include/jello_hip.h
int jh_stats_launch(hipStream_t stream, jimage_src src, jimage_rect rect, const jh_stats_desc* desc, void* out, void* tmp, int num_cus);
int jh_load_surface_launch(hipStream_t stream, const void* src, uint64_t pitch, jimage_dst dst, jimage_rect rect, int format, int alpha, int num_cus);
int jh_load_yuv_launch(hipStream_t stream, const void* const* planes, const uint64_t* pitches, jimage_dst dst, jimage_rect rect, int layout, int matrix,
                       int range, int transfer, int chroma, int num_cus);
int jh_lut3d_launch(hipStream_t stream, jimage_src src, jimage_dst dst, jimage_rect rect, const void* lut, uint32_t n, int variant, int num_cus);
int jh_selftest_math_launch(hipStream_t stream, int op, const float* a, const float* b, float* out, uint32_t n);
int jh_selftest_atomics_launch(hipStream_t stream, int form, uint32_t seed, uint32_t n_waves);
}

// Binding slots (the WGSL @binding order) of the stages whose bindings the held-back rules compare; the other stages name
// theirs next to their launcher.
enum { PR2_REDUCED, PR2_REDUCED2 };                            // pathtag_reduce2
enum { PS1_REDUCED, PS1_REDUCED2, PS1_OUT };                   // pathtag_scan1
#define PT_ABSORB_MAX 16u  // the largest grid of pathtag_scan1 that redoes a held-back pathtag_reduce2 in passing (kernels_scan.hip)
enum { PSC_CFG, PSC_SCENE, PSC_REDUCED, PSC_TM };              // pathtag_scan_small / _large
enum { BC_CFG, BC_BBOX };                                      // bbox_clear
enum { FL_CFG, FL_SCENE, FL_TM, FL_BBOX, FL_BUMP, FL_LINES };  // flatten
enum { PCS_BUMP, PCS_INDIRECT };                               // path_count_setup
enum { PC_CFG, PC_BUMP, PC_LINES, PC_PATHS, PC_TILES, PC_SEGC };  // path_count
enum { PTS_BUMP, PTS_INDIRECT, PTS_PTCL };                     // path_tiling_setup
enum { PT_BUMP, PT_SEGC, PT_LINES, PT_PATHS, PT_TILES, PT_SEGMENTS };  // path_tiling

// The stages in jh_stage order (SURVEY Appendix C = renderer/render.go dispatch order), each named here and nowhere else:
//   X(name, minimum binding count, slot read as JlConfig, slot read as JlBump, slot written as IndirectCount (-1: none), indirect only)
// The contract is what the launchers rely on instead of checking themselves (jello_hip.cpp, check_contract); "indirect only": the
// stage's grid comes from an IndirectCount, jh_dispatch is refused.  jello_hip.cpp builds its stage table -- name, contract,
// launcher -- from this list, its only caller of the launchers jh_launch_<name>.
#define JH_STAGE_LIST(X)                          \
    X(pathtag_reduce, 3, 0, -1, -1, false)        \
    X(pathtag_reduce2, 2, -1, -1, -1, false)      \
    X(pathtag_scan1, 3, -1, -1, -1, false)        \
    X(pathtag_scan_small, 4, 0, -1, -1, false)    \
    X(pathtag_scan_large, 4, 0, -1, -1, false)    \
    X(bbox_clear, 2, 0, -1, -1, false)            \
    X(flatten, 6, 0, 4, -1, false)                \
    X(draw_reduce, 3, 0, -1, -1, false)           \
    X(draw_leaf, 7, 0, -1, -1, false)             \
    X(clip_reduce, 4, -1, -1, -1, false)          \
    X(clip_leaf, 7, 0, -1, -1, false)             \
    X(binning, 8, 0, 5, -1, false)                \
    X(tile_alloc, 6, 0, 3, -1, false)             \
    X(backdrop_dyn, 4, 0, 1, -1, false)           \
    X(path_count_setup, 2, -1, 0, 1, false)       \
    X(path_count, 6, 0, 1, -1, true)              \
    X(coarse, 9, 0, 7, -1, false)                 \
    X(path_tiling_setup, 3, -1, 0, 1, false)      \
    X(path_tiling, 6, -1, 0, -1, true)            \
    X(fine_area, 7, 0, -1, -1, false)             \
    X(fine_msaa8, 9, 0, -1, -1, false)            \
    X(fine_msaa16, 9, 0, -1, -1, false)
#define JH_DECLARE_LAUNCHER(name, ...) JhResult jh_launch_##name(const JhLaunch& L);
JH_STAGE_LIST(JH_DECLARE_LAUNCHER)
#undef JH_DECLARE_LAUNCHER
