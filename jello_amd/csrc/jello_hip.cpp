// jello_hip.cpp -- implementation of the C ABI in include/jello_hip.h: context, pooled device
// buffers keyed by the recording's ResourceIDs, images in linear device memory, per-stage dispatch
// onto the HIP kernels, hipEvent profiling.  Replaces engine/wgpu_engine (wgpu.go:322-643) below
// the renderer.Recording boundary.  There is no CPU fallback here: if HIP is unavailable every
// call fails with JH_ERR_NO_DEVICE / JH_ERR_DEVICE.
#include "../../include/jello_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "kcommon.h"
#include "../../include/jello_blur.h"
#include "../../include/jello_composite.h"
#include "../../include/jello_resample.h"
#include "../../include/jello_color.h"
#include "../../include/jello_distance.h"
#include "../../include/jello_stats.h"
#include "../../include/jello_morph.h"
#include "../../include/jello_warp.h"
#include "../../include/jello_convolve.h"
#include "../../include/jello_lighting.h"
#include "../../include/jello_turbulence.h"
#include "../../include/jello_displace.h"
#include "../../include/jello_shadow.h"
#include "../../include/jello_perspective.h"
#include "../../include/jello_queries.h"
#include "../../include/jello_dash_host.h"

#ifndef JH_SCR_SKEW
#define JH_SCR_SKEW 1280u
#endif
// Self-cleaned slots and their "left clean by its kernels" flags (kcommon.h): the one place that pairs them.
enum { JH_CLEAN_FL_CTR = 1u, JH_CLEAN_BD_CTR = 2u, JH_CLEAN_SCAN = 8u, JH_CLEAN_PC_TOT = 16u };
static const struct { int slot; uint32_t flag; } kSelfCleaned[] = {
    {JH_SCR_FL_CTR, JH_CLEAN_FL_CTR}, {JH_SCR_BD_CTR, JH_CLEAN_BD_CTR}, {JH_SCR_SCAN_TMP, JH_CLEAN_SCAN}, {JH_SCR_PC_TOT, JH_CLEAN_PC_TOT}};
static uint32_t clean_flag_of(int slot) {
    for (const auto& k : kSelfCleaned)
        if (k.slot == slot) return k.flag;
    return 0u;  // (the other arrays are written before they are read in every frame)
}

struct JhScratch {
    void* ptr[JH_SCR_COUNT] = {};
    void* base[JH_SCR_COUNT] = {};  // what hipMalloc returned (ptr may be offset into it)
    uint64_t cap[JH_SCR_COUNT] = {};
    std::vector<void*> retired;  // old allocations kept until the next sync (kernels may still use them)
    uint32_t clean_flags = 0u;   // JH_CLEAN_*
    jh_ctx* ctx = nullptr;
};

struct Alloc {
    void* ptr = nullptr;
    uint64_t size = 0;      // logical size (bytes)
    uint64_t capacity = 0;  // allocation size class
    bool owned = true;
    uint32_t width = 0, height = 0;
    int format = 0;
    bool pending_clear = false;
    bool written = false;   // images: has content (uploaded / imported); a created-only image reads as zero like a new wgpu texture
    bool stored = false;    // images: bound as a dispatch's storage image (fine's target) -- has content for jh_blit, not for sampling
};

// One node of the profile tree (engine/wgpu_engine/profiler.go:96-158): a group (Start/Nest ... End: CPU interval and
// children) or a GPU query (ProfilerGroup.Compute: one hipEvent pair around a dispatch).
struct ProfEntry {
    int kind;    // JH_PROF_GROUP / JH_PROF_QUERY
    int parent;  // index of the enclosing group, -1 at top level
    int stage;   // query: jh_stage
    std::string label;
    double cpu_start_ms = 0.0, cpu_end_ms = 0.0;
    hipEvent_t start = nullptr, stop = nullptr;  // query only
};

// A recorded command that has not been launched yet: see "held-back commands" below.
enum HeldKind { HELD_NONE = -1, HELD_BUMP_CLEAR, HELD_BBOX_CLEAR, HELD_LAST_SCAN, HELD_REDUCE2, HELD_COUNT_SETUP, HELD_TILING_SETUP };
struct Held {
    HeldKind kind;
    int stage;  // jh_stage; -1 for HELD_BUMP_CLEAR, the recording's Clear command
    uint32_t gx, gy, gz;
    std::vector<JhBound> b;  // the command's bindings; HELD_BUMP_CLEAR: b[0] = the range to clear
};

struct JhGraph {  // a captured frame plus the resource generation it was captured against
    hipGraphExec_t exec;
    uint64_t generation;
    uint32_t kernel_nodes, other_nodes;  // what the capture recorded (jh_graph_node_counts)
    // JH_CLEAN_* flags that were up when the capture began: the graph holds NO fill for those counters and relies on the
    // frame before it having left them zeroed.  jh_graph_launch zeroes whichever of them is not clean at that moment (a frame
    // that failed half-way, jh_debug_poison_scratch) before the replay.
    uint32_t assumes_clean;
};

struct Staging {  // pinned host arena for uploads: the caller's slice is copied once, the DMA runs asynchronously
    char* base = nullptr;
    uint64_t cap = 0, used = 0;
};

struct jh_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    std::string name;
    uint64_t total_mem = 0;
    std::unordered_map<uint64_t, Alloc> buffers;
    std::unordered_map<uint64_t, Alloc> images;
    std::unordered_map<uint64_t, JlConfig> config_shadow;  // host copies of uploaded ConfigUniforms (by buffer id)
    std::multimap<uint64_t, void*> pool;  // capacity -> free allocation
    uint64_t pool_bytes = 0;
    JhScratch scratch;
    bool profiling = false;
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> free_events;
    std::vector<int> prof_stack;  // open groups (indices into prof)
    std::string last_error;
    uint32_t band_row0 = 0u, band_row1 = 0xffffffffu;  // jh_set_band
    uint32_t clip_depth_hint = 0u;                     // jh_set_clip_depth_hint
    uint32_t debug_flatten = 0u;                       // jh_debug_flatten_regions
    // Bumped whenever a device pointer a captured graph may have baked in goes away or moves: buffer / image free,
    // regrow or import, scratch regrow.  jh_graph_launch refuses a graph captured against an older generation.
    uint64_t generation = 0;
    bool capturing = false;
    uint32_t clean_at_capture_begin = 0u;
    uint64_t graph_self_cleans = 0;  // replays that had to zero a counter first (jh_debug_graph_self_cleans)
    Staging staging;
    // fine: descriptor table of the bound image array when it has more entries than fit in the kernel arguments
    void* image_table = nullptr;
    uint64_t image_table_cap = 0;
    uint32_t* hint_overflow = nullptr;  // device word: blend-stack saves fine had to drop because the clip-depth hint was too small
    std::vector<JhImageDesc> image_table_host;
    std::vector<Held> held;  // held-back commands, in recording order
    // jh_resample: the geometry whose tables the JH_SCR_RESAMPLE_TAPS slot holds, and where they lie in it
    struct {
        bool valid = false;
        int filter = 0;
        uint32_t sw = 0, sh = 0, dw = 0, dh = 0;
        JhResampleTables tables = {};
    } resample;
    // jh_color_filter: the key whose tables the JH_SCR_COLOR_TABLES slot holds, and where
    struct {
        bool valid = false;
        jcolor_key key = {};
        const char* dev = nullptr;
    } color;
    // jh_lighting: the key whose tables the JH_SCR_LIGHT_TABLES slot holds, and where
    struct {
        bool valid = false;
        jlight_key key = {};
        const char* dev = nullptr;
    } light;
    // jh_turbulence: the key (the seed after setup_seed) whose tables the JH_SCR_TURB_TABLES slot holds, and where
    struct {
        bool valid = false;
        uint32_t key = 0;
        const char* dev = nullptr;
    } turb;
    int debug_lut3d = 0;  // jh_debug_lut3d_variant (last: the members above stay where they were)
};

static int flush_held(jh_ctx* ctx);
#define JH_FLUSH(ctx)                              \
    do {                                           \
        int frc__ = flush_held(ctx);               \
        if (frc__ != JH_OK) return frc__;          \
    } while (0)

static int fail(jh_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->last_error = msg;
    return code;
}
static int hip_fail(jh_ctx* ctx, hipError_t e, const char* what) {
    return fail(ctx, JH_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(ctx, expr)                                \
    do {                                                  \
        hipError_t e__ = (expr);                          \
        if (e__ != hipSuccess) return hip_fail(ctx, e__, #expr); \
    } while (0)

// engine/wgpu_engine/wgpu.go:800-808 poolSizeClass with sizeClassBits = 1
static uint64_t pool_size_class(uint64_t x) {
    const uint32_t num_bits = 1;
    if (x > (1ull << num_bits)) {
        int a = __builtin_clzll(x - 1);
        uint64_t b = (x - 1) | (((~0ull / 2) >> num_bits) >> a);
        return b + 1;
    }
    return 1ull << num_bits;
}

static int pool_get(jh_ctx* ctx, uint64_t size, void** out, uint64_t* cap_out) {
    uint64_t cap = pool_size_class(size < 16 ? 16 : size);
    auto it = ctx->pool.find(cap);
    if (it != ctx->pool.end()) {
        *out = it->second;
        *cap_out = cap;
        ctx->pool.erase(it);
        return 0;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess) return fail(ctx, JH_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
    ctx->pool_bytes += cap;
    *out = p;
    *cap_out = cap;
    return 0;
}

void* jh_scratch_get(JhScratch* s, int slot, uint64_t bytes) {
    if (slot < 0 || slot >= JH_SCR_COUNT) return nullptr;
    if (bytes < 256) bytes = 256;
    if (s->cap[slot] >= bytes) return s->ptr[slot];
    // A capture records pointers: growing an array now would leave the graph with a mix of old and new ones, and
    // jh_graph_end would put the "left clean" flag of the NEW, uninitialised memory back up.  The contract --
    // run the recording once eagerly before capturing it -- makes every array big enough; a capture that still has to grow
    // one is refused (the dispatch answers JH_ERR_OOM with a message that says so).
    if (s->ctx->capturing) return nullptr;
    // (what is asked for + 1/16, in whole MiB: these arrays are internal, they do not go through the reference's pool and its
    // size classes -- 2^k and 1.5 * 2^k, up to a third more than asked -- and the sixteenth keeps a slowly growing scene from
    // reallocating every frame)
    uint64_t cap = bytes + bytes / 16;
    cap = cap < (1ull << 20) ? pool_size_class(cap) : (cap + ((1ull << 20) - 1)) & ~((1ull << 20) - 1);
    void* p = nullptr;
    // Every slot starts at its own offset (a multiple of 256 B) into its allocation: the flatten kernels walk up to
    // seven scratch arrays with the same index at once, and with all of them on 2 MiB boundaries k_flatten_lines
    // measured 117-124 us on C3 (4 of 4 processes) against 106-109 us (6 of 8) with the offsets.
    if (hipMalloc(&p, cap + (uint64_t)JH_SCR_COUNT * JH_SCR_SKEW) != hipSuccess) return nullptr;
    if (s->base[slot]) {
        s->retired.push_back(s->base[slot]);
        s->ctx->generation++;  // a captured graph may hold the old pointer
    }
    s->base[slot] = p;
    // new memory holds anything: the slot's "left clean by its kernels" flag goes down (the other slots keep theirs -- with one
    // flag word for all, a frame that grew ANY array late made the next frame fill every counter again, and a graph captured
    // from that frame kept the fills)
    s->clean_flags &= ~clean_flag_of(slot);
    p = (char*)p + (uint64_t)slot * JH_SCR_SKEW;
    s->ptr[slot] = p;
    s->cap[slot] = cap;
    return p;
}

void* jh_scratch_acquire(JhScratch* s, int slot, uint64_t bytes, uint64_t fill_bytes, hipStream_t stream) {
    void* p = jh_scratch_get(s, slot, bytes);
    if (!p) return nullptr;
    const uint32_t flag = clean_flag_of(slot);
    if ((s->clean_flags & flag) == 0u) (void)hipMemsetAsync(p, 0, std::min(fill_bytes, s->cap[slot]), stream);
    s->clean_flags &= ~flag;
    return p;
}
void jh_scratch_left_clean(JhScratch* s, int slot) { s->clean_flags |= clean_flag_of(slot); }
uint64_t jh_scratch_cap(JhScratch* s, int slot) { return (slot >= 0 && slot < JH_SCR_COUNT) ? s->cap[slot] : 0; }

static void scratch_release_retired(JhScratch* s) {
    for (void* p : s->retired) (void)hipFree(p);
    s->retired.clear();
}

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Copies `size` host bytes into the pinned arena and returns the pinned address (valid until the arena wraps, which
// first waits for the stream).  nullptr on allocation failure.
static void* stage_copy(jh_ctx* ctx, const void* data, uint64_t size) {
    Staging& st = ctx->staging;
    uint64_t need = (size + 255u) & ~255ull;
    if (st.used + need > st.cap) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;  // every earlier copy out of the arena is done
        st.used = 0;
        if (need > st.cap) {
            uint64_t cap = st.cap ? st.cap : (8ull << 20);
            while (cap < need) cap *= 2;
            if (st.base) (void)hipHostFree(st.base);
            st.base = nullptr;
            st.cap = 0;
            void* p = nullptr;
            if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
            st.base = (char*)p;
            st.cap = cap;
        }
    }
    void* dst = st.base + st.used;
    std::memcpy(dst, data, size);
    st.used += need;
    return dst;
}

// The stage table, indexed by jh_stage: name, binding contract and launcher, from the list in kcommon.h.
struct StageInfo {
    const char* name;
    int n_min, cfg, bump, indirect;
    bool indirect_only;
    JhResult (*launch)(const JhLaunch&);
};
#define JH_STAGE_ENTRY(name, ...) {#name, __VA_ARGS__, jh_launch_##name},
static const StageInfo kStages[JH_STAGE_COUNT] = {JH_STAGE_LIST(JH_STAGE_ENTRY)};
#undef JH_STAGE_ENTRY

// What every launch gets from the context (the dispatcher adds the command's own: images, indirect count, config shadow, ...)
static JhLaunch make_launch(jh_ctx* ctx, uint32_t gx, uint32_t gy, uint32_t gz, const std::vector<JhBound>& b) {
    JhLaunch L = {};
    L.stream = ctx->stream;
    L.scratch = &ctx->scratch;
    L.gx = gx; L.gy = gy; L.gz = gz;
    L.b = b.data();
    L.nb = (int)b.size();
    L.num_cus = ctx->num_cus;
    L.band_row0 = ctx->band_row0;
    L.band_row1 = ctx->band_row1;
    L.clip_depth_hint = ctx->clip_depth_hint;
    L.hint_overflow = ctx->hint_overflow;
    L.debug_flatten = ctx->debug_flatten;
    return L;
}

// ------------------------------------------------------------------------------------------------
// Held-back commands
// ------------------------------------------------------------------------------------------------
// Six of the recording's commands are 1-thread or trivially small kernels (or a fill) in front of a stage that can do their
// work in passing (render.go:186-197,230-237,369-374,415-420).  The engine holds them back until the next command and lets
// that command absorb them when it is the consumer they were waiting for (same buffers) -- or launches them as recorded before
// anything else happens (any other command, a download, a sync, a buffer that moves, the end of a graph capture: JH_FLUSH).
// What every buffer holds after each command is what the recording says.  The rules, each stated once below:
//   which command may be held         held_kind_of_dispatch, clear_may_be_held
//   what may wait together            hold_back
//   for which consumer, on which of
//   its bindings, what it is told     absorb_one
// Not while profiling: a held-back stage's query would bracket nothing and its work would be charged to the stage that
// absorbs it -- with the profiler on every command is launched as recorded and every query times its own stage.
static HeldKind held_kind_of_dispatch(const jh_ctx* ctx, int stage, uint32_t gx) {
    if (ctx->profiling) return HELD_NONE;
    switch (stage) {
        case JH_BBOX_CLEAR: return HELD_BBOX_CLEAR;
        case JH_PATH_COUNT_SETUP: return HELD_COUNT_SETUP;
        case JH_PATH_TILING_SETUP: return HELD_TILING_SETUP;
        // (the reference always dispatches reduce2 with 256 workgroups, one thread of its consumer per entry of reduced2)
        case JH_PATHTAG_REDUCE2: return gx > 0u && gx <= 256u ? HELD_REDUCE2 : HELD_NONE;
        case JH_PATHTAG_SCAN_SMALL: case JH_PATHTAG_SCAN_LARGE: return gx > 0u ? HELD_LAST_SCAN : HELD_NONE;
        default: return HELD_NONE;
    }
}
// (the recording's Clear(bump) in front of flatten, render.go:237: the whole of a buffer that is a BumpAllocators)
static bool clear_may_be_held(const jh_ctx* ctx, const Alloc& a, uint64_t offset, uint64_t n) {
    return !ctx->profiling && n && offset == 0 && n == a.size && a.size == sizeof(JlBump);
}

// Only one kind of thing waits at a time, except what waits for flatten: the last pathtag scan, bbox_clear and Clear(bump), one of
// each.  Whatever else is waiting is launched first.
static bool waits_for_flatten(HeldKind k) { return k == HELD_BUMP_CLEAR || k == HELD_BBOX_CLEAR || k == HELD_LAST_SCAN; }
static int hold_back(jh_ctx* ctx, Held&& h) {
    for (const Held& d : ctx->held)
        if (!(waits_for_flatten(h.kind) && waits_for_flatten(d.kind) && d.kind != h.kind)) { JH_FLUSH(ctx); break; }
    ctx->held.push_back(std::move(h));
    return JH_OK;
}

static bool same_buffer(const JhBound& x, const JhBound& y) { return x.ptr == y.ptr && x.size == y.size; }
// Is the command being dispatched (stage, gx, indirect count, bindings b) the consumer the held-back command `d` waits for?  If
// so, notes in `a` what its launcher has to do in passing.
static bool absorb_one(int stage, uint32_t gx, const uint32_t* indirect, const std::vector<JhBound>& b, const Held& d, JhAbsorbed& a) {
    // (a dispatch with no workgroups launches nothing that could do the held-back work in passing -- an empty scene's flatten,
    // renderer.cpp: flatten_wgs = 0 -- so what waits for it runs as recorded: ADVICE r03)
    const bool flatten = stage == JH_FLATTEN && gx > 0u;
    switch (d.kind) {
        case HELD_BUMP_CLEAR:  // flatten's first kernel zeroes the bump allocators
            if (!(flatten && same_buffer(d.b[0], b[FL_BUMP]) && b[FL_BUMP].size == sizeof(JlBump))) return false;
            a.bump_clear = true;
            return true;
        case HELD_BBOX_CLEAR:  // ... and resets the path bboxes
            if (!(flatten && d.b[BC_CFG].ptr == b[FL_CFG].ptr && same_buffer(d.b[BC_BBOX], b[FL_BBOX]))) return false;
            a.bbox_clear = true;
            return true;
        case HELD_LAST_SCAN:
            // flatten's classification kernel, which reads every tag word and its monoid back, produces the monoids in passing
            // (k_pathtag_scan_classify): same config and scene, the scan's output is the tag monoids flatten reads, and its
            // threads (one per tag word = four tag bytes) cover flatten's (one per tag byte)
            if (!(flatten && d.b[PSC_CFG].ptr == b[FL_CFG].ptr && same_buffer(d.b[PSC_SCENE], b[FL_SCENE]) && same_buffer(d.b[PSC_TM], b[FL_TM]) &&
                  (uint64_t)d.gx * 4u >= (uint64_t)gx && d.gy <= 1u && d.gz <= 1u))
                return false;
            a.pathtag_scan = true;
            a.scan_reduced = d.b[PSC_REDUCED];
            a.scan_wgs = d.gx;
            a.scan_small = d.stage == JH_PATHTAG_SCAN_SMALL;
            return true;
        case HELD_REDUCE2:
            // pathtag_scan1 redoes reduce2's sums in passing if it runs at most PT_ABSORB_MAX workgroups itself
            if (!(stage == JH_PATHTAG_SCAN1 && gx > 0u && gx <= PT_ABSORB_MAX && gx <= d.gx && same_buffer(d.b[PR2_REDUCED], b[PS1_REDUCED]) &&
                  same_buffer(d.b[PR2_REDUCED2], b[PS1_REDUCED2])))
                return false;
            a.reduce2 = true;
            a.reduce2_entries = d.gx;
            return true;
        case HELD_COUNT_SETUP:  // k_pc_count writes the indirect count it is dispatched with
            if (!(stage == JH_PATH_COUNT && indirect && d.b[PCS_BUMP].ptr == b[PC_BUMP].ptr && d.b[PCS_INDIRECT].ptr == (void*)indirect)) return false;
            a.write_indirect = true;
            return true;
        case HELD_TILING_SETUP:  // k_path_tiling likewise, and marks the ptcl on failure
            if (!(stage == JH_PATH_TILING && indirect && d.b[PTS_BUMP].ptr == b[PT_BUMP].ptr && d.b[PTS_INDIRECT].ptr == (void*)indirect)) return false;
            a.write_indirect = true;
            a.tiling_ptcl = d.b[PTS_PTCL];
            return true;
        default: return false;
    }
}
// Does this command absorb EVERYTHING that is waiting?  Then *out says with what, and nothing waits any more.
static bool absorb_all(jh_ctx* ctx, int stage, uint32_t gx, const uint32_t* indirect, const std::vector<JhBound>& b, JhAbsorbed* out) {
    JhAbsorbed a = {};
    for (const Held& d : ctx->held)
        if (!absorb_one(stage, gx, indirect, b, d, a)) return false;
    *out = a;
    ctx->held.clear();
    return true;
}

// Launches every held-back command as recorded.
static int flush_held(jh_ctx* ctx) {
    if (ctx->held.empty()) return JH_OK;
    std::vector<Held> pending;
    pending.swap(ctx->held);
    for (const Held& d : pending) {
        if (d.kind == HELD_BUMP_CLEAR) {
            HIP_TRY(ctx, hipMemsetAsync(d.b[0].ptr, 0, d.b[0].size, ctx->stream));
            continue;
        }
        if (kStages[d.stage].launch(make_launch(ctx, d.gx, d.gy, d.gz, d.b)) != JH_L_OK)
            return fail(ctx, JH_ERR_INVALID, std::string("deferred stage failed: ") + jh_stage_name(d.stage));
    }
    return JH_OK;
}

extern "C" {

const char* jh_stage_name(int stage) { return (stage >= 0 && stage < JH_STAGE_COUNT) ? kStages[stage].name : "?"; }

int jh_create(jh_ctx** out, int device) {
    if (!out) return JH_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return JH_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return JH_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return JH_ERR_DEVICE;
    jh_ctx* ctx = new jh_ctx();
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        ctx->num_cus = prop.multiProcessorCount;
        ctx->name = prop.name;
        ctx->total_mem = prop.totalGlobalMem;
    }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return JH_ERR_DEVICE;
    }
    ctx->stream = ctx->own_stream;
    ctx->scratch.ctx = ctx;
    // (zeroed on the context's OWN stream: a hipMemset here would be the process's first use of the legacy default stream, and
    // from then on the frames of two contexts no longer overlapped at all -- bench.py's two frames in flight fell from 0.91 to
    // 1.05 ms per frame, found by bisection in round 5)
    if (hipMalloc((void**)&ctx->hint_overflow, 256) != hipSuccess || hipMemsetAsync(ctx->hint_overflow, 0, 256, ctx->own_stream) != hipSuccess ||
        hipStreamSynchronize(ctx->own_stream) != hipSuccess)
        ctx->hint_overflow = nullptr;
    *out = ctx;
    return JH_OK;
}

void jh_destroy(jh_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->buffers)
        if (kv.second.owned && kv.second.ptr) (void)hipFree(kv.second.ptr);
    for (auto& kv : ctx->images)
        if (kv.second.owned && kv.second.ptr) (void)hipFree(kv.second.ptr);
    for (auto& kv : ctx->pool) (void)hipFree(kv.second);
    for (int i = 0; i < JH_SCR_COUNT; i++)
        if (ctx->scratch.base[i]) (void)hipFree(ctx->scratch.base[i]);
    scratch_release_retired(&ctx->scratch);
    if (ctx->staging.base) (void)hipHostFree(ctx->staging.base);
    if (ctx->image_table) (void)hipFree(ctx->image_table);
    if (ctx->hint_overflow) (void)hipFree(ctx->hint_overflow);
    for (auto& p : ctx->prof)
        if (p.kind == JH_PROF_QUERY) { (void)hipEventDestroy(p.start); (void)hipEventDestroy(p.stop); }
    for (auto& e : ctx->free_events) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char* jh_last_error(jh_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int jh_set_stream(jh_ctx* ctx, void* hip_stream) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    if (next != ctx->stream && ctx->staging.used) {  // uploads still in flight on the old stream read the pinned arena
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->staging.used = 0;
    }
    ctx->stream = next;
    return JH_OK;
}

// A stream of the lowest (level < 0), the default (0) or the highest (> 0) launch priority of the context's device, for callers that
// want a stage on a stream of its own (tools/fine_priority.py).  Destroy with jh_stream_destroy.
int jh_stream_create(jh_ctx* ctx, int level, void** hip_stream) {
    if (!ctx || !hip_stream) return JH_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int least = 0, greatest = 0;
    HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t st = nullptr;
    HIP_TRY(ctx, hipStreamCreateWithPriority(&st, hipStreamNonBlocking, level < 0 ? least : (level > 0 ? greatest : 0)));
    *hip_stream = (void*)st;
    return JH_OK;
}
int jh_stream_destroy(jh_ctx* ctx, void* hip_stream) {
    if (!ctx || !hip_stream) return JH_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamDestroy((hipStream_t)hip_stream));
    return JH_OK;
}

int jh_set_band(jh_ctx* ctx, uint32_t bin_row0, uint32_t bin_row1) {
    if (!ctx || bin_row1 < bin_row0) return JH_ERR_INVALID;
    ctx->band_row0 = bin_row0;
    ctx->band_row1 = bin_row1;
    return JH_OK;
}

int jh_sync(jh_ctx* ctx) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    scratch_release_retired(&ctx->scratch);
    ctx->staging.used = 0;
    return JH_OK;
}

// ---- buffers ----
static Alloc* find_alloc(std::unordered_map<uint64_t, Alloc>& map, uint64_t id) {
    auto it = map.find(id);
    return it == map.end() ? nullptr : &it->second;
}
// The allocation behind an id goes away (the caller erases or overwrites the entry).  Memory the context owns goes back to the
// pool and into circulation, so captured graphs that may point to it become stale.  Caller-owned memory stays valid for as long
// as its owner keeps it -- a graph captured while it was bound keeps using it, e.g. double-buffered output images -- unless
// the caller asks for staleness anyway (`stale_if_imported`).
static void retire_alloc(jh_ctx* ctx, const Alloc& a, bool stale_if_imported = false) {
    if (a.owned) ctx->pool.insert({a.capacity, a.ptr});
    if (a.owned || stale_if_imported) ctx->generation++;
}

static int buffer_get_or_create(jh_ctx* ctx, uint64_t id, uint64_t size, Alloc** out) {
    if (Alloc* old = find_alloc(ctx->buffers, id)) {
        if (old->size >= size) {
            *out = old;
            return 0;
        }
        if (!old->owned) return fail(ctx, JH_ERR_INVALID, "imported buffer is smaller than the requested size (the caller owns it: cannot grow)");
        // grow: return the old allocation to the pool (a held-back command may still refer to it: launch those first)
        JH_FLUSH(ctx);
        retire_alloc(ctx, *old);
        ctx->buffers.erase(id);
    }
    Alloc a;
    int rc = pool_get(ctx, size, &a.ptr, &a.capacity);
    if (rc) return rc;
    a.size = size;
    a.owned = true;
    auto ins = ctx->buffers.emplace(id, a);
    *out = &ins.first->second;
    return 0;
}

int jh_buffer_create(jh_ctx* ctx, uint64_t id, uint64_t size) {
    if (!ctx) return JH_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Alloc* a;
    return buffer_get_or_create(ctx, id, size, &a);
}

int jh_buffer_import(jh_ctx* ctx, uint64_t id, void* device_ptr, uint64_t size) {
    if (!ctx || !device_ptr) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    if (const Alloc* old = find_alloc(ctx->buffers, id)) retire_alloc(ctx, *old);  // (re-importing caller-owned memory leaves graphs valid)
    Alloc a;
    a.ptr = device_ptr;
    a.size = size;
    a.capacity = size;
    a.owned = false;
    ctx->buffers[id] = a;
    ctx->config_shadow.erase(id);  // whatever was uploaded under this id is not what the new memory holds
    return JH_OK;
}

int jh_upload(jh_ctx* ctx, uint64_t id, const void* data, uint64_t size) {
    if (!ctx || (!data && size)) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Alloc* a;
    int rc = buffer_get_or_create(ctx, id, size, &a);
    if (rc) return rc;
    // The launchers pick kernel instantiations and grids from the host shadow of the ConfigUniform (clip / no-clip fine and
    // coarse, ...), so a captured frame is only valid for the uniform it was captured with: a different uniform under the
    // same id makes every captured graph stale (jh_graph_launch then answers JH_ERR_INVALID instead of replaying kernels
    // that would stop at the first BEGIN_CLIP).
    {
        auto sh = ctx->config_shadow.find(id);
        const bool had = sh != ctx->config_shadow.end();
        if (size == sizeof(JlConfig)) {
            if (!had || std::memcmp(&sh->second, data, sizeof(JlConfig)) != 0) {
                if (had) ctx->generation++;
                std::memcpy(&ctx->config_shadow[id], data, sizeof(JlConfig));
            }
        } else if (had) {
            ctx->config_shadow.erase(sh);
            ctx->generation++;
        }
    }
    if (size) {
        // The host slice is only valid for the duration of the call (reference: queue.WriteBuffer copies, wgpu.go:360):
        // it is copied into the pinned arena here and the DMA is left in flight -- no stream synchronisation per upload.
        void* src = stage_copy(ctx, data, size);
        if (!src) return fail(ctx, JH_ERR_OOM, "jh_upload: pinned staging allocation failed");
        HIP_TRY(ctx, hipMemcpyAsync(a->ptr, src, size, hipMemcpyHostToDevice, ctx->stream));
    }
    return JH_OK;
}

int jh_clear(jh_ctx* ctx, uint64_t id, uint64_t offset, int64_t size) {
    if (!ctx) return JH_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Alloc* a = find_alloc(ctx->buffers, id);
    if (!a) return fail(ctx, JH_ERR_INVALID, "jh_clear: unknown buffer id (create it first)");
    if (offset > a->size) return fail(ctx, JH_ERR_INVALID, "jh_clear: offset out of range");
    uint64_t n = size < 0 ? a->size - offset : (uint64_t)size;
    if (offset + n > a->size) n = a->size - offset;
    if (clear_may_be_held(ctx, *a, offset, n)) {
        int rc = hold_back(ctx, Held{HELD_BUMP_CLEAR, -1, 0, 0, 0, {JhBound{a->ptr, n, 0, 0, 0}}});
        if (rc) return rc;
    } else {
        JH_FLUSH(ctx);
        if (n) HIP_TRY(ctx, hipMemsetAsync((char*)a->ptr + offset, 0, n, ctx->stream));
    }
    if (n && offset < sizeof(JlConfig) && ctx->config_shadow.erase(id)) ctx->generation++;  // the shadow no longer describes the device copy
    return JH_OK;
}

int jh_download(jh_ctx* ctx, uint64_t id, void* dst, uint64_t offset, uint64_t size) {
    if (!ctx || !dst) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Alloc* a = find_alloc(ctx->buffers, id);
    if (!a) return fail(ctx, JH_ERR_INVALID, "jh_download: unknown buffer id");
    if (offset + size > a->size) return fail(ctx, JH_ERR_INVALID, "jh_download: range out of bounds");
    HIP_TRY(ctx, hipMemcpyAsync(dst, (char*)a->ptr + offset, size, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return JH_OK;
}

int jh_free(jh_ctx* ctx, uint64_t id) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    const Alloc* a = find_alloc(ctx->buffers, id);
    if (!a) return JH_OK;  // the reference ignores frees of unknown ids (wgpu.go:601-603)
    retire_alloc(ctx, *a);
    ctx->buffers.erase(id);
    ctx->config_shadow.erase(id);
    return JH_OK;
}

void* jh_buffer_device_ptr(jh_ctx* ctx, uint64_t id) {
    const Alloc* a = ctx ? find_alloc(ctx->buffers, id) : nullptr;
    return a ? a->ptr : nullptr;
}
uint64_t jh_buffer_size(jh_ctx* ctx, uint64_t id) {
    const Alloc* a = ctx ? find_alloc(ctx->buffers, id) : nullptr;
    return a ? a->size : 0;
}

// ---- images ----
static uint64_t format_bpp(int format) {
    switch (format) {
        case JL_RGBA8: case JL_RGBA8_SRGB: case JL_BGRA8: return 4;
        case JL_RGBA16_FLOAT: return 8;
        default: return 0;
    }
}

int jh_image_create(jh_ctx* ctx, uint64_t id, uint32_t width, uint32_t height, int format) {
    if (!ctx) return JH_ERR_INVALID;
    uint64_t bpp = format_bpp(format);
    if (!bpp) return fail(ctx, JH_ERR_INVALID, "jh_image_create: bad format");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint64_t size = (uint64_t)width * height * bpp;
    if (const Alloc* old = find_alloc(ctx->images, id)) {
        if (old->width == width && old->height == height && old->format == format) return JH_OK;
        JH_FLUSH(ctx);
        retire_alloc(ctx, *old, /*stale_if_imported=*/true);  // (the image changes shape under the id: a graph that binds it is stale either way)
        ctx->images.erase(id);
    }
    Alloc a;
    int rc = pool_get(ctx, size ? size : 8, &a.ptr, &a.capacity);
    if (rc) return rc;
    a.size = size; a.width = width; a.height = height; a.format = format; a.owned = true;
    ctx->images[id] = a;
    return JH_OK;
}

int jh_image_import(jh_ctx* ctx, uint64_t id, void* device_ptr, uint32_t width, uint32_t height, int format) {
    if (!ctx || !device_ptr) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    uint64_t bpp = format_bpp(format);
    if (!bpp) return fail(ctx, JH_ERR_INVALID, "jh_image_import: bad format");
    if (const Alloc* old = find_alloc(ctx->images, id)) retire_alloc(ctx, *old);
    Alloc a;
    a.ptr = device_ptr; a.size = (uint64_t)width * height * bpp; a.capacity = a.size; a.owned = false;
    a.width = width; a.height = height; a.format = format; a.written = true;
    ctx->images[id] = a;
    return JH_OK;
}

int jh_image_upload(jh_ctx* ctx, uint64_t id, uint32_t width, uint32_t height, int format, const void* data, uint64_t size) {
    int rc = jh_image_create(ctx, id, width, height, format);
    if (rc) return rc;
    JH_FLUSH(ctx);
    if (!data && size) return JH_ERR_INVALID;
    Alloc& a = ctx->images[id];
    if (size > a.size) size = a.size;
    if (size) {
        void* src = stage_copy(ctx, data, size);
        if (!src) return fail(ctx, JH_ERR_OOM, "jh_image_upload: pinned staging allocation failed");
        HIP_TRY(ctx, hipMemcpyAsync(a.ptr, src, size, hipMemcpyHostToDevice, ctx->stream));
    }
    // an all-zero image (the 1x1 placeholder of render.go:115-124) contributes zero texels: bind it as absent
    bool nonzero = false;
    const uint8_t* bytes = (const uint8_t*)data;
    for (uint64_t i = 0; i < size && !nonzero; i++) nonzero = bytes[i] != 0;
    if (a.written != nonzero) ctx->generation++;  // fine binds a never-written image as absent: the choice is baked into a graph
    a.written = nonzero;
    return JH_OK;
}

// WriteImage (renderer/recording.go:204-208; wgpu.go:422-452 queue.WriteTexture): rows of `width` texels, tightly
// packed in `data`, into the rectangle (x, y, width, height) of the image.
int jh_image_write(jh_ctx* ctx, uint64_t id, uint32_t x, uint32_t y, uint32_t width, uint32_t height, const void* data, uint64_t size) {
    if (!ctx || (!data && size)) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Alloc* found = find_alloc(ctx->images, id);
    if (!found) return fail(ctx, JH_ERR_INVALID, "jh_image_write: unknown image id (create it first)");
    Alloc& a = *found;
    const uint64_t bpp = format_bpp(a.format);
    if ((uint64_t)x + width > a.width || (uint64_t)y + height > a.height) return fail(ctx, JH_ERR_INVALID, "jh_image_write: rectangle outside the image");
    const uint64_t row = (uint64_t)width * bpp;
    if (size < row * height) return fail(ctx, JH_ERR_INVALID, "jh_image_write: data smaller than the rectangle");
    if (row == 0 || height == 0) return JH_OK;
    void* src = stage_copy(ctx, data, row * height);
    if (!src) return fail(ctx, JH_ERR_OOM, "jh_image_write: pinned staging allocation failed");
    HIP_TRY(ctx, hipMemcpy2DAsync((char*)a.ptr + ((uint64_t)y * a.width + x) * bpp, (uint64_t)a.width * bpp, src, row, row, height,
                                  hipMemcpyHostToDevice, ctx->stream));
    if (!a.written) { a.written = true; ctx->generation++; }
    return JH_OK;
}

int jh_image_download(jh_ctx* ctx, uint64_t id, void* dst, uint64_t size) {
    if (!ctx || !dst) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Alloc* a = find_alloc(ctx->images, id);
    if (!a) return fail(ctx, JH_ERR_INVALID, "jh_image_download: unknown image id");
    if (size > a->size) size = a->size;
    HIP_TRY(ctx, hipMemcpyAsync(dst, a->ptr, size, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return JH_OK;
}

int jh_image_free(jh_ctx* ctx, uint64_t id) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    const Alloc* a = find_alloc(ctx->images, id);
    if (!a) return JH_OK;
    retire_alloc(ctx, *a);
    ctx->images.erase(id);
    return JH_OK;
}

void* jh_image_device_ptr(jh_ctx* ctx, uint64_t id) {
    const Alloc* a = ctx ? find_alloc(ctx->images, id) : nullptr;
    return a ? a->ptr : nullptr;
}
int jh_image_size(jh_ctx* ctx, uint64_t id, uint32_t* width, uint32_t* height) {
    const Alloc* a = ctx ? find_alloc(ctx->images, id) : nullptr;
    if (!a) return JH_ERR_INVALID;
    if (width) *width = a->width;
    if (height) *height = a->height;
    return JH_OK;
}

// ---- dispatch ----
static int resolve_bindings(jh_ctx* ctx, const jh_binding* bindings, int n, std::vector<JhBound>& out, std::vector<JhBound>& images) {
    out.clear();
    images.clear();
    for (int i = 0; i < n; i++) {
        const jh_binding& b = bindings[i];
        JhBound r;
        std::memset(&r, 0, sizeof r);
        if (b.kind == JH_BIND_BUFFER) {
            const Alloc* a = find_alloc(ctx->buffers, b.id);
            if (!a) return fail(ctx, JH_ERR_INVALID, "dispatch: unknown buffer id in binding " + std::to_string(i));
            r.ptr = a->ptr;
            r.size = a->size;
            out.push_back(r);
        } else if (b.kind == JH_BIND_IMAGE) {
            const Alloc* a = find_alloc(ctx->images, b.id);
            if (!a) return fail(ctx, JH_ERR_INVALID, "dispatch: unknown image id in binding " + std::to_string(i));
            r.ptr = a->ptr; r.size = a->size; r.width = a->width; r.height = a->height; r.format = a->format;
            out.push_back(r);
        } else if (b.kind == JH_BIND_IMAGE_ARRAY) {
            for (uint32_t k = 0; k < b.count; k++) {
                const Alloc* a = find_alloc(ctx->images, b.ids[k]);
                if (!a) return fail(ctx, JH_ERR_INVALID, "dispatch: unknown image id in image array");
                JhBound im;
                std::memset(&im, 0, sizeof im);
                // a never-written image samples as transparent black: no pointer, the texel fetch returns zero
                im.ptr = a->written ? a->ptr : nullptr; im.size = a->size; im.width = a->width; im.height = a->height; im.format = a->format;
                images.push_back(im);
            }
            out.push_back(r);  // placeholder keeps binding indices aligned with the WGSL @binding order
        } else {
            return fail(ctx, JH_ERR_INVALID, "dispatch: bad binding kind");
        }
    }
    return 0;
}

// The launchers read these slots as fixed structs: refuses binding lists that are too short and buffers that cannot hold them.
static int check_contract(jh_ctx* ctx, int stage, const std::vector<JhBound>& b, const uint32_t* indirect) {
    const StageInfo& S = kStages[stage];
    if ((int)b.size() < S.n_min) return fail(ctx, JH_ERR_INVALID, std::string("bad bindings for stage ") + S.name + ": too few");
    auto too_small = [&](int slot, uint64_t need) { return slot >= 0 && (b[slot].ptr == nullptr || b[slot].size < need); };
    if (too_small(S.cfg, sizeof(JlConfig)) || too_small(S.bump, sizeof(JlBump)) || too_small(S.indirect, 12))
        return fail(ctx, JH_ERR_INVALID, std::string("bad bindings for stage ") + S.name + ": config / bump / indirect buffer too small");
    if (S.indirect_only && !indirect) return fail(ctx, JH_ERR_INVALID, std::string("bad bindings for stage ") + S.name);
    return JH_OK;
}

// More images than fit in the kernel arguments: fine indexes a device table of descriptors (the reference binds an array of up
// to 2048 textures, wgpu.go:278).  The table is re-uploaded only when the bound set changes.
static int bind_image_table(jh_ctx* ctx, const std::vector<JhBound>& images, const JhImageDesc** out) {
    std::vector<JhImageDesc> t(images.size());
    for (size_t i = 0; i < images.size(); i++) {
        t[i].ptr = images[i].ptr; t[i].width = images[i].width; t[i].height = images[i].height;
        t[i].srgb = images[i].format == JL_RGBA8_SRGB ? 1u : 0u; t[i].pad = 0u;
    }
    const bool same = t.size() == ctx->image_table_host.size() &&
                      std::memcmp(t.data(), ctx->image_table_host.data(), t.size() * sizeof(JhImageDesc)) == 0;
    if (!same) {
        if (ctx->capturing) return fail(ctx, JH_ERR_INVALID, "fine: the image table changed during graph capture (run the recording once eagerly first)");
        const uint64_t bytes = t.size() * sizeof(JhImageDesc);
        if (bytes > ctx->image_table_cap) {
            void* np = nullptr;
            if (hipMalloc(&np, pool_size_class(bytes)) != hipSuccess) return fail(ctx, JH_ERR_OOM, "fine: image table allocation failed");
            if (ctx->image_table) ctx->scratch.retired.push_back(ctx->image_table);
            ctx->image_table = np;
            ctx->image_table_cap = pool_size_class(bytes);
            ctx->generation++;
        }
        void* src = stage_copy(ctx, t.data(), bytes);
        if (!src) return fail(ctx, JH_ERR_OOM, "fine: pinned staging allocation failed");
        HIP_TRY(ctx, hipMemcpyAsync(ctx->image_table, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        ctx->image_table_host = t;
    }
    *out = (const JhImageDesc*)ctx->image_table;
    return JH_OK;
}

// binning and coarse address a bin by its index in a 256-entry table (one per lane of the 256-thread workgroup:
// binning.wgsl:52,131; coarse.wgsl:153-176): a target of more than 256 bins of 256 x 256 px -- beyond 4096 px in a
// direction -- silently loses the bins past the 256th in the reference.  Here the dispatch is refused instead.
static int check_bin_limit(jh_ctx* ctx, int stage, const JlConfig* cfg_host) {
    if ((stage != JH_BINNING && stage != JH_COARSE) || !cfg_host) return JH_OK;
    const uint64_t wb = (cfg_host->width_in_tiles + 15u) / 16u, hb = (cfg_host->height_in_tiles + 15u) / 16u;
    if (wb * hb > 256u)
        return fail(ctx, JH_ERR_INVALID, std::string(jh_stage_name(stage)) + ": the target has " + std::to_string(wb * hb) +
                                             " bins of 256 x 256 px, the pipeline addresses 256 (at most 4096 x 4096 px or any shape of <= 256 bins)");
    return JH_OK;
}

// One GPU query of the profile tree around whatever is enqueued between begin and end; both do nothing with the profiler off.
// stage = -1: a query that is no stage record (the post-render calls).
static int prof_query_begin(jh_ctx* ctx, ProfEntry& pe, int stage, const char* label) {
    if (!ctx->profiling) return JH_OK;
    for (hipEvent_t* e : {&pe.start, &pe.stop}) {
        if (ctx->free_events.empty()) { HIP_TRY(ctx, hipEventCreate(e)); continue; }
        *e = ctx->free_events.back();
        ctx->free_events.pop_back();
    }
    pe.kind = JH_PROF_QUERY;
    pe.parent = ctx->prof_stack.empty() ? -1 : ctx->prof_stack.back();
    pe.stage = stage;
    pe.label = label;
    pe.cpu_start_ms = now_ms();
    HIP_TRY(ctx, hipEventRecord(pe.start, ctx->stream));
    return JH_OK;
}
static int prof_query_end(jh_ctx* ctx, ProfEntry& pe) {
    if (!ctx->profiling) return JH_OK;
    HIP_TRY(ctx, hipEventRecord(pe.stop, ctx->stream));
    pe.cpu_end_ms = now_ms();
    ctx->prof.push_back(pe);
    return JH_OK;
}

// What a scratch array that could not be had is reported as; `remedy`: what to do first when a capture kept it from growing.
static std::string scratch_failure(const jh_ctx* ctx, const char* remedy) {
    return ctx->capturing ? std::string("a scratch array would have to grow during graph capture: ") + remedy : "scratch allocation failed";
}
static int launch_result(jh_ctx* ctx, int stage, JhResult r) {
    switch (r) {
        case JH_L_OK: return JH_OK;
        case JH_L_SCRATCH: return fail(ctx, JH_ERR_OOM, scratch_failure(ctx, "run the recording once eagerly first"));
        default: return fail(ctx, JH_ERR_INVALID, std::string("bad bindings for stage ") + jh_stage_name(stage));
    }
}

static int dispatch_common(jh_ctx* ctx, int stage, uint32_t gx, uint32_t gy, uint32_t gz, const uint32_t* indirect, const jh_binding* bindings,
                           int n_bindings) {
    if (!ctx || stage < 0 || stage >= JH_STAGE_COUNT || (n_bindings && !bindings)) return JH_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<JhBound> b, images;
    int rc = resolve_bindings(ctx, bindings, n_bindings, b, images);
    if (rc) return rc;
    rc = check_contract(ctx, stage, b, indirect);
    if (rc) return rc;
    // held back: launched by the stage it waits for, or as recorded by the next flush
    const HeldKind kind = held_kind_of_dispatch(ctx, stage, gx);
    if (kind != HELD_NONE) return hold_back(ctx, Held{kind, stage, gx, gy, gz, std::move(b)});
    JhLaunch L = make_launch(ctx, gx, gy, gz, b);
    if (!absorb_all(ctx, stage, gx, indirect, b, &L.absorbed)) JH_FLUSH(ctx);
    L.images = images.data();
    L.n_images = (int)images.size();
    L.indirect = indirect;
    if ((int)images.size() > JH_FINE_INLINE_IMAGES && stage >= JH_FINE_AREA) {
        rc = bind_image_table(ctx, images, &L.image_table);
        if (rc) return rc;
    }
    if (n_bindings > 0 && bindings[0].kind == JH_BIND_BUFFER) {
        auto sh = ctx->config_shadow.find(bindings[0].id);
        if (sh != ctx->config_shadow.end()) L.cfg_host = &sh->second;
    }
    rc = check_bin_limit(ctx, stage, L.cfg_host);
    if (rc) return rc;
    ProfEntry pe;
    rc = prof_query_begin(ctx, pe, stage, jh_stage_name(stage));  // ProfilerGroup.Compute(arena, shader.Label), wgpu.go:486,537
    if (rc) return rc;
    const JhResult res = kStages[stage].launch(L);
    rc = prof_query_end(ctx, pe);
    if (rc) return rc;
    rc = launch_result(ctx, stage, res);
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, jh_stage_name(stage));
    for (int i = 0; i < n_bindings; i++)
        if (bindings[i].kind == JH_BIND_IMAGE)
            if (Alloc* im = find_alloc(ctx->images, bindings[i].id)) im->stored = true;
    return JH_OK;
}

int jh_dispatch(jh_ctx* ctx, int stage, uint32_t gx, uint32_t gy, uint32_t gz, const jh_binding* bindings, int n_bindings) {
    return dispatch_common(ctx, stage, gx, gy, gz, nullptr, bindings, n_bindings);
}

int jh_dispatch_indirect(jh_ctx* ctx, int stage, uint64_t indirect_buffer_id, uint64_t offset, const jh_binding* bindings, int n_bindings) {
    if (!ctx) return JH_ERR_INVALID;
    const Alloc* a = find_alloc(ctx->buffers, indirect_buffer_id);
    if (!a) return fail(ctx, JH_ERR_INVALID, "dispatch_indirect: unknown indirect buffer");
    if (offset + 12 > a->size || (offset & 3)) return fail(ctx, JH_ERR_INVALID, "dispatch_indirect: bad offset");
    return dispatch_common(ctx, stage, 0, 1, 1, (const uint32_t*)((char*)a->ptr + offset), bindings, n_bindings);
}

// ---- hipGraph capture ----
int jh_graph_begin(jh_ctx* ctx) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    if (ctx->profiling) return fail(ctx, JH_ERR_INVALID, "jh_graph_begin: disable profiling first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    ctx->clean_at_capture_begin = ctx->scratch.clean_flags;
    return JH_OK;
}
int jh_graph_end(jh_ctx* ctx, void** graph_exec) {
    if (!ctx || !graph_exec) return JH_ERR_INVALID;
    *graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    const int frc = flush_held(ctx);  // held-back commands belong to the captured frame
    ctx->capturing = false;
    // Nothing ran: the device holds what it held when the capture began, and so must the host's picture of it (a launcher that
    // found a flag down recorded its fill INTO the graph and raised the flag -- the fill has not happened).
    ctx->scratch.clean_flags = ctx->clean_at_capture_begin;
    HIP_TRY(ctx, hipStreamEndCapture(ctx->stream, &graph));
    if (frc != JH_OK) { if (graph) (void)hipGraphDestroy(graph); return frc; }
    // the launches of the frame, counted on the captured graph itself
    uint32_t n_kernel = 0u, n_other = 0u;
    {
        size_t n = 0;
        if (hipGraphGetNodes(graph, nullptr, &n) == hipSuccess && n > 0) {
            std::vector<hipGraphNode_t> nodes(n);
            if (hipGraphGetNodes(graph, nodes.data(), &n) == hipSuccess)
                for (size_t i = 0; i < n; i++) {
                    hipGraphNodeType ty = hipGraphNodeTypeEmpty;
                    if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess) continue;
                    if (ty == hipGraphNodeTypeKernel) n_kernel++; else if (ty != hipGraphNodeTypeEmpty) n_other++;
                }
        }
    }
    // (Launch priorities per kernel node -- hipGraphKernelNodeSetAttribute(hipKernelNodeAttributePriority) -- are refused by this ROCm for
    // every node; priorities through streams do not help either: profiles/r04_fine_priority.txt.)
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipGraphInstantiate");
    *graph_exec = (void*)new JhGraph{exec, ctx->generation, n_kernel, n_other, ctx->clean_at_capture_begin};
    return JH_OK;
}
int jh_graph_node_counts(jh_ctx* ctx, void* graph_exec, uint32_t* kernel_nodes, uint32_t* other_nodes) {
    if (!ctx || !graph_exec) return JH_ERR_INVALID;
    const JhGraph* g = (const JhGraph*)graph_exec;
    if (kernel_nodes) *kernel_nodes = g->kernel_nodes;
    if (other_nodes) *other_nodes = g->other_nodes;
    return JH_OK;
}
int jh_graph_launch(jh_ctx* ctx, void* graph_exec) {
    if (!ctx || !graph_exec) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    JhGraph* g = (JhGraph*)graph_exec;
    // The graph holds raw device pointers (buffers, scratch, image table) and the kernel instantiations picked at capture
    // time: it is only valid while none of them has been freed, regrown or re-imported since.
    if (g->generation != ctx->generation)
        return fail(ctx, JH_ERR_INVALID, "jh_graph_launch: stale graph (a buffer, image or scratch array it refers to was freed, regrown or "
                                         "re-imported after the capture) -- capture again");
    // Counters the graph expects zeroed (it has no fill for them) and that are not: the frame before did not run to its end
    // (a stage failed half-way) or the scratch was poisoned.  Zero them here -- the eager path's own remedy -- then replay.
    const uint32_t dirty = g->assumes_clean & ~ctx->scratch.clean_flags;
    if (dirty) {
        for (const auto& k : kSelfCleaned)
            if ((dirty & k.flag) && ctx->scratch.ptr[k.slot] && ctx->scratch.cap[k.slot])
                HIP_TRY(ctx, hipMemsetAsync(ctx->scratch.ptr[k.slot], 0, ctx->scratch.cap[k.slot], ctx->stream));
        ctx->scratch.clean_flags |= dirty;
        ctx->graph_self_cleans++;
    }
    HIP_TRY(ctx, hipGraphLaunch(g->exec, ctx->stream));
    return JH_OK;
}
int jh_graph_destroy(jh_ctx* ctx, void* graph_exec) {
    if (!ctx) return JH_ERR_INVALID;
    if (graph_exec) {
        JhGraph* g = (JhGraph*)graph_exec;
        hipError_t e = hipGraphExecDestroy(g->exec);
        delete g;
        if (e != hipSuccess) return hip_fail(ctx, e, "hipGraphExecDestroy");
    }
    return JH_OK;
}

// ---- profiling ----
int jh_profile_enable(jh_ctx* ctx, int on) {
    if (!ctx) return JH_ERR_INVALID;
    ctx->profiling = on != 0;
    return JH_OK;
}

// Profiler.Start / ProfilerGroup.Nest (profiler.go:49-65, 138-158): opens a group under the innermost open one.
int jh_profile_group_begin(jh_ctx* ctx, const char* label) {
    if (!ctx) return JH_ERR_INVALID;
    if (!ctx->profiling) return JH_OK;  // a nil profiler accepts every call (profiler.go:45-52)
    ProfEntry g;
    g.kind = JH_PROF_GROUP;
    g.parent = ctx->prof_stack.empty() ? -1 : ctx->prof_stack.back();
    g.stage = -1;
    g.label = label ? label : "";
    g.cpu_start_ms = now_ms();
    ctx->prof_stack.push_back((int)ctx->prof.size());
    ctx->prof.push_back(g);
    return JH_OK;
}
// ProfilerGroup.End (profiler.go:113-125); ending a group that was never begun is an error (the reference panics).
int jh_profile_group_end(jh_ctx* ctx) {
    if (!ctx) return JH_ERR_INVALID;
    if (!ctx->profiling && ctx->prof_stack.empty()) return JH_OK;
    if (ctx->prof_stack.empty()) return fail(ctx, JH_ERR_INVALID, "jh_profile_group_end: no open group");
    ctx->prof[ctx->prof_stack.back()].cpu_end_ms = now_ms();
    ctx->prof_stack.pop_back();
    return JH_OK;
}

static void prof_recycle(jh_ctx* ctx) {
    for (auto& p : ctx->prof)
        if (p.kind == JH_PROF_QUERY) { ctx->free_events.push_back(p.start); ctx->free_events.push_back(p.stop); }
    ctx->prof.clear();
    ctx->prof_stack.clear();
}

int jh_profile_collect(jh_ctx* ctx, jh_profile_record* out, int max) {
    if (!ctx) return JH_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int n = 0;
    for (auto& p : ctx->prof) {
        if (p.kind != JH_PROF_QUERY || p.stage < 0) continue;  // (a post-render call is a query of the tree, not a stage record)
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, p.start, p.stop);
        if (out && n < max) {
            out[n].stage = p.stage;
            out[n].pad = 0;
            out[n].ms = ms;
            n++;
        }
    }
    prof_recycle(ctx);
    return n;
}

// Profiler.Collect (profiler.go:337-385): the tree, flattened in creation order (a node's parent always precedes it).
int jh_profile_collect_tree(jh_ctx* ctx, jh_profile_node* out, int max) {
    if (!ctx) return JH_ERR_INVALID;
    if (!ctx->prof_stack.empty()) return fail(ctx, JH_ERR_INVALID, "jh_profile_collect_tree: a group is still open");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    hipEvent_t base = nullptr;
    double cpu0 = 0.0;
    bool have_cpu0 = false;
    for (auto& p : ctx->prof) {
        if (!have_cpu0) { cpu0 = p.cpu_start_ms; have_cpu0 = true; }
        if (p.kind == JH_PROF_QUERY && !base) base = p.start;
    }
    int n = 0;
    for (auto& p : ctx->prof) {
        if (!out || n >= max) break;
        jh_profile_node& o = out[n++];
        std::memset(&o, 0, sizeof o);
        o.kind = p.kind;
        o.parent = p.parent;
        o.stage = p.stage;
        std::strncpy(o.label, p.label.c_str(), sizeof(o.label) - 1);
        o.cpu_start_ms = p.cpu_start_ms - cpu0;
        o.cpu_end_ms = p.cpu_end_ms - cpu0;
        if (p.kind == JH_PROF_QUERY) {
            float a = 0.0f, d = 0.0f;
            (void)hipEventElapsedTime(&a, base, p.start);
            (void)hipEventElapsedTime(&d, p.start, p.stop);
            o.gpu_start_ms = a;
            o.gpu_end_ms = a + d;
        }
    }
    // a group's GPU interval = the hull of the queries below it (filled bottom-up: children follow their parents)
    for (int i = n - 1; i >= 0; i--) {
        if (out[i].kind == JH_PROF_QUERY || (out[i].kind == JH_PROF_GROUP && out[i].gpu_end_ms > out[i].gpu_start_ms)) {
            int par = out[i].parent;
            if (par >= 0 && par < n) {
                if (out[par].gpu_end_ms <= out[par].gpu_start_ms) { out[par].gpu_start_ms = out[i].gpu_start_ms; out[par].gpu_end_ms = out[i].gpu_end_ms; }
                else {
                    if (out[i].gpu_start_ms < out[par].gpu_start_ms) out[par].gpu_start_ms = out[i].gpu_start_ms;
                    if (out[i].gpu_end_ms > out[par].gpu_end_ms) out[par].gpu_end_ms = out[i].gpu_end_ms;
                }
            }
        }
    }
    prof_recycle(ctx);
    return n;
}

// ---- post-render calls: the surface and YUV blits, the tile pack, dashing, blur, composite, resample, colour filter, morphology, warp, convolve, lighting, turbulence, displace, shadow, perspective, distance, load, stats ----
// The words of the context's counter block (hint_overflow: 64 words, zeroed at creation) and who counts in them.
enum {
    kHintOverflowWord = 0,   // fine: blend-stack saves dropped because the clip-depth hint was too small (L.hint_overflow)
    kFineTimingWord = 8,     // fine under FINE_TIMING: six 64-bit counters
    kUnpackRejectWord = 32,  // jh_unpack_tiles: what it ignored
};
// n_words of the block from first_word on into `out` (if non-null), then zeroed if `reset`.  Synchronises the stream.
static int counter_words(jh_ctx* ctx, uint32_t first_word, uint32_t n_words, void* out, int reset) {
    uint32_t* words = ctx->hint_overflow + first_word;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (out) {
        HIP_TRY(ctx, hipMemcpyAsync(out, words, 4u * n_words, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (reset) {
        HIP_TRY(ctx, hipMemsetAsync(words, 0, 4u * n_words, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return JH_OK;
}

extern "C++" {  // (a template cannot have C linkage)
// The frame of a post-render call once its own checks have passed (every check comes before anything is enqueued: a refused call
// touches no memory and flushes nothing): what is held back is launched, the device selected, `prepare` gets what has to be there
// before the query opens (scratch, staging), and `launch` enqueues the call's work -- inside a query of its own when profiling is on
// (the reference's pgroup.Render(arena, "blit")): stage -1, a node of the tree and no stage record.  Both answer a JH_* code and
// have reported their own failure.
template <class Prepare, class Launch>
static int post_render_call(jh_ctx* ctx, const char* label, Prepare&& prepare, Launch&& launch) {
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = prepare();
    if (rc) return rc;
    ProfEntry pe;
    rc = prof_query_begin(ctx, pe, -1, label);
    if (rc) return rc;
    rc = launch();
    const int prc = prof_query_end(ctx, pe);
    return rc ? rc : prc;
}
template <class Launch>
static int post_render_call(jh_ctx* ctx, const char* label, Launch&& launch) {
    return post_render_call(ctx, label, [] { return (int)JH_OK; }, launch);
}
}
// What the launchers of kcommon.h's list answer -- 0, -1 for a frame they refuse, anything else for a failed launch -- as a JH_* code.
static int launch_status(jh_ctx* ctx, const char* who, int rc) {
    if (rc == 0) return JH_OK;
    if (rc == -1) return fail(ctx, JH_ERR_INVALID, std::string(who) + ": image too large for one launch");
    return fail(ctx, JH_ERR_DEVICE, std::string(who) + ": launch failed: " + hipGetErrorString(hipGetLastError()));
}

// The images a call names by id, each in its role ("source" or "destination"): all of them known, then each of them RGBA16F and
// -- where the caller gives one -- of the size size[0] x size[1].
struct ImageRole { uint64_t id; const char* role; Alloc** out; };
static int rgba16f_images(jh_ctx* ctx, const char* who, std::initializer_list<ImageRole> images, const uint32_t* size = nullptr) {
    const std::string w(who);
    for (const ImageRole& i : images)
        if (!(*i.out = find_alloc(ctx->images, i.id))) return fail(ctx, JH_ERR_INVALID, w + ": unknown " + i.role + " image id");
    for (const ImageRole& i : images) {
        const Alloc& a = **i.out;
        if (a.format != JL_RGBA16_FLOAT) return fail(ctx, JH_ERR_INVALID, w + ": the " + i.role + " is not an RGBA16F image");
        if (size && (a.width != size[0] || a.height != size[1])) return fail(ctx, JH_ERR_INVALID, w + ": size differs from the " + i.role + " image");
    }
    return JH_OK;
}
// a source that was never written reads as transparent black, like a fresh texture: the kernels take a null pointer for it
static const void* content_or_null(const Alloc& a) { return (a.written || a.stored) ? a.ptr : nullptr; }
// A call is about to write the width x height rectangle of dst.  If that is dst's first content, the texels outside the rectangle
// go on reading as transparent black.  (Not jh_image_write's condition: a frame's target is stored, never written, and a call
// that writes it must not make captured graphs stale.)
static int first_content(jh_ctx* ctx, Alloc* dst, uint32_t width, uint32_t height) {
    if (!(dst->written || dst->stored)) {
        if (width != dst->width || height != dst->height) HIP_TRY(ctx, hipMemsetAsync(dst->ptr, 0, dst->size, ctx->stream));
        ctx->generation++;  // (fine binds a never-written image as absent: the choice is baked into a graph)
    }
    dst->written = true;
    return JH_OK;
}
// band mode: the pixel rows [*row0, *row1) of the active bin rows only (a bin row = 256 pixel rows: an even cut), so that bands of
// several ranks compose; row1 = row0 when the band lies below the image
static void band_pixel_rows(const jh_ctx* ctx, uint32_t height, uint32_t* row0, uint32_t* row1) {
    *row0 = (uint32_t)std::min<uint64_t>((uint64_t)ctx->band_row0 * 256u, height);
    *row1 = std::max(*row0, (uint32_t)std::min<uint64_t>((uint64_t)ctx->band_row1 * 256u, height));
}

// What a call from one RGBA16F image into another checks first: the context, the descriptor, both ids known, both images RGBA16F (and
// of `size`, where the call takes one), two images where the call cannot run in place (`in_place` says what it would do there), and
// no band set: the call's texels depend on rows outside a band (`band_rows` names them).
static int image_call_images(jh_ctx* ctx, const char* who, const void* desc, uint64_t src_id, uint64_t dst_id, const char* in_place, const char* band_rows,
                             Alloc** src, Alloc** dst, const uint32_t* size = nullptr) {
    if (!ctx) return JH_ERR_INVALID;
    if (!desc) return fail(ctx, JH_ERR_INVALID, std::string(who) + ": null descriptor");
    if (int rc = rgba16f_images(ctx, who, {{src_id, "source", src}, {dst_id, "destination", dst}}, size)) return rc;
    if (in_place && *src == *dst) return fail(ctx, JH_ERR_INVALID, std::string(who) + ": the source is the destination (" + in_place + ")");
    if (ctx->band_row0 == 0u && ctx->band_row1 == 0xffffffffu) return JH_OK;
    return fail(ctx, JH_ERR_INVALID, std::string(who) + ": not in band mode (" + band_rows + ")");
}
// What a call that only writes one RGBA16F image (jh_turbulence generates) checks first: the same, for one image.
static int image_call_image(jh_ctx* ctx, const char* who, const void* desc, uint64_t dst_id, const char* band_rows, Alloc** dst) {
    if (!ctx) return JH_ERR_INVALID;
    if (!desc) return fail(ctx, JH_ERR_INVALID, std::string(who) + ": null descriptor");
    if (int rc = rgba16f_images(ctx, who, {{dst_id, "destination", dst}})) return rc;
    if (ctx->band_row0 == 0u && ctx->band_row1 == 0xffffffffu) return JH_OK;
    return fail(ctx, JH_ERR_INVALID, std::string(who) + ": not in band mode (" + band_rows + ")");
}
// The refusal of a rectangle after jimage_rect_check's answer (`role`: which rectangle of the call and which image: "", "source " or
// "destination "), and the rectangle a descriptor names in `image`, resolved into *out, or its refusal.
static int refuse_rect(jh_ctx* ctx, const char* who, int check, const std::string& role) {
    return fail(ctx, JH_ERR_INVALID, std::string(who) + ": the " + role + "rectangle is " + (check == JIMAGE_RECT_HALF_EMPTY ? "empty in one dimension" : "not inside the " + role + "image"));
}
static int image_call_rect(jh_ctx* ctx, const char* who, jimage_rect named, const Alloc& image, const char* role, jimage_rect* out) {
    *out = jimage_resolve(named, image.width, image.height);
    const int check = jimage_rect_check(named, image.width, image.height);
    return check ? refuse_rect(ctx, who, check, role) : (int)JH_OK;
}
// A call is about to write the rectangle `written` of dst from src, inside its query: the views its launcher takes.  The source pointer
// is taken first: dst may be the same image, and one that was never written reads as transparent black (null), not as its memory.
struct ImageViews { jimage_src from; jimage_dst to; };
static int image_call_views(jh_ctx* ctx, const Alloc* src, Alloc* dst, jimage_rect written, ImageViews* v) {
    v->from = {content_or_null(*src), src->width, src->height};
    if (int rc = first_content(ctx, dst, written.w, written.h)) return rc;
    v->to = {dst->ptr, dst->width, dst->height};
    return JH_OK;
}

// `bytes` of scratch slot `slot` into *out, in a call's `prepare` (`remedy`: scratch_failure's advice).
static int scratch_take(jh_ctx* ctx, const char* who, const char* remedy, int slot, uint64_t bytes, void** out) {
    if ((*out = jh_scratch_get(&ctx->scratch, slot, bytes))) return JH_OK;
    return fail(ctx, JH_ERR_OOM, std::string(who) + ": " + scratch_failure(ctx, remedy));
}
// Bytes that have to be in a scratch slot before a call's launch.  slot_upload_take, in `prepare`: the slot, and a copy in the pinned
// arena (as jh_upload: the DMA is left in flight); slot_upload_send, in `launch`: the asynchronous copy (the query holds the upload too).
struct SlotUpload { char* dev = nullptr; void* staged = nullptr; uint64_t bytes = 0; };
static int slot_upload_take(jh_ctx* ctx, const char* who, const char* remedy, int slot, const void* data, uint64_t bytes, SlotUpload* u) {
    u->bytes = bytes;
    if (int rc = scratch_take(ctx, who, remedy, slot, bytes, (void**)&u->dev)) return rc;
    if ((u->staged = stage_copy(ctx, data, bytes))) return JH_OK;
    return fail(ctx, JH_ERR_OOM, std::string(who) + ": pinned staging allocation failed");
}
static int slot_upload_send(jh_ctx* ctx, const SlotUpload& u) {
    HIP_TRY(ctx, hipMemcpyAsync(u.dev, u.staged, u.bytes, hipMemcpyHostToDevice, ctx->stream));
    return JH_OK;
}
// Tables a call keeps in a scratch slot of their own under a key of the context's (jh_resample: one geometry, jh_color_filter: one
// key): content that a captured call reads on every replay.  `resident`: the slot holds this call's, nothing is uploaded.  A capture
// can neither grow an array nor upload, so its tables have to be resident: the blob is built only where to_build(), tables_take (in
// `prepare`) refuses the capture, and tables_send (in `launch`) invalidates the key, uploads, has set_key(device pointer) note the
// new key and bumps the generation (a graph captured against the tables of another key would read these).
struct ResidentTables {
    bool resident;
    SlotUpload up;
    bool to_build(const jh_ctx* ctx) const { return !resident && !ctx->capturing; }
};
static int tables_take(jh_ctx* ctx, const char* who, const char* remedy, int slot, const std::vector<char>& blob, ResidentTables* t) {
    if (t->resident) return JH_OK;
    if (ctx->capturing) return fail(ctx, JH_ERR_OOM, std::string(who) + ": " + scratch_failure(ctx, remedy));
    return slot_upload_take(ctx, who, remedy, slot, blob.data(), blob.size(), &t->up);
}
extern "C++" template <class SetKey>
static int tables_send(jh_ctx* ctx, const ResidentTables& t, bool* valid, SetKey&& set_key) {
    if (t.resident) return JH_OK;
    *valid = false;
    if (int rc = slot_upload_send(ctx, t.up)) return rc;
    set_key(t.up.dev);
    *valid = true;
    ctx->generation++;
    return JH_OK;
}

// surface blit (RenderToSurface's blit pass, engine/wgpu_engine/lib.go:109-198, 266-333; kernels_surface.hip)
int jh_blit(jh_ctx* ctx, uint64_t src_image_id, void* dst_device_ptr, uint64_t dst_pitch_bytes, uint32_t width, uint32_t height,
            int surface_format) {
    if (!ctx) return JH_ERR_INVALID;
    const uint32_t size[2] = {width, height};
    Alloc* a = nullptr;
    if (int rc = rgba16f_images(ctx, "jh_blit", {{src_image_id, "source", &a}}, size)) return rc;
    if (!dst_device_ptr) return fail(ctx, JH_ERR_INVALID, "jh_blit: null destination");
    if (const char* why = jframe_surface_pitch_error(dst_pitch_bytes, width)) return fail(ctx, JH_ERR_INVALID, std::string("jh_blit: ") + why);
    if (const char* why = jframe_surface_format_error(surface_format)) return fail(ctx, JH_ERR_INVALID, std::string("jh_blit: ") + why);
    return post_render_call(ctx, "blit", [&] {
        uint32_t row0, row1;
        band_pixel_rows(ctx, height, &row0, &row1);
        return launch_status(ctx, "jh_blit", jh_blit_launch(ctx->stream, content_or_null(*a), dst_device_ptr, dst_pitch_bytes, width, row0, row1,
                                                            surface_format, ctx->num_cus));
    });
}

// YUV blit (include/jello_hip.h "YUV blit"; kernels_yuv.hip)
int jh_blit_yuv(jh_ctx* ctx, uint64_t src_image_id, uint32_t width, uint32_t height, const jh_yuv_desc* desc) {
    if (!ctx) return JH_ERR_INVALID;
    if (!desc) return fail(ctx, JH_ERR_INVALID, "jh_blit_yuv: null descriptor");
    const uint32_t size[2] = {width, height};
    Alloc* a = nullptr;
    if (int rc = rgba16f_images(ctx, "jh_blit_yuv", {{src_image_id, "source", &a}}, size)) return rc;
    const char* why = jframe_yuv_enums_error(desc->layout, desc->matrix, desc->range, desc->transfer);
    if (!why) why = jframe_yuv_planes_error(desc->layout, desc->plane, desc->pitch, width, JFRAME_NULL_PLANE | JFRAME_SHORT_PITCH);  // (plane by plane)
    if (why) return fail(ctx, JH_ERR_INVALID, std::string("jh_blit_yuv: ") + why);
    return post_render_call(ctx, "blit_yuv", [&] {
        uint32_t row0, row1;  // the luma rows of the band, and the chroma rows under them
        band_pixel_rows(ctx, height, &row0, &row1);
        if (row1 == row0) return (int)JH_OK;
        return launch_status(ctx, "jh_blit_yuv", jh_blit_yuv_launch(ctx->stream, content_or_null(*a), desc->plane, desc->pitch, width, height, row0, row1,
                                                                    desc->layout, desc->matrix, desc->range, desc->transfer, ctx->num_cus));
    });
}

// tile pack (include/jello_hip.h "tile-packed frame transport"; kernels_pack.hip)
uint64_t jh_pack_bound(uint32_t width, uint32_t height, uint32_t texel_bytes) {
    if (texel_bytes != 4u && texel_bytes != 8u) return 0;
    const uint64_t tiles = (uint64_t)((width + 15ull) / 16u) * ((height + 15ull) / 16u);
    return 32u + ((8u * tiles + 15u) & ~15ull) + tiles * 256u * texel_bytes;  // header, entries, no solid texels, all blocks raw
}

// What both calls ask of a frame: a texel size of 4 or 8, a size that is not empty and whose tile indices fit 31 bits, a pitch
// that holds a row, pointer and pitch multiples of the texel size.  nullptr when it holds, else what is wrong.
static const char* pack_frame_error(const void* p, uint64_t pitch, uint32_t width, uint32_t height, uint32_t texel_bytes) {
    if (texel_bytes != 4u && texel_bytes != 8u) return "texel_bytes is not 4 or 8";
    if (width == 0u || height == 0u) return "empty frame";
    if ((uint64_t)((width + 15ull) / 16u) * ((height + 15ull) / 16u) > 0x7fffffffull) return "more than 2^31 - 1 tiles";
    if (!p) return "null pointer";
    if (pitch < (uint64_t)width * texel_bytes) return "pitch below width * texel_bytes";
    if (((uintptr_t)p | pitch) % texel_bytes) return "pointer or pitch is not a multiple of texel_bytes";
    return nullptr;
}

int jh_pack_tiles(jh_ctx* ctx, const void* src, uint64_t src_pitch, const void* ref, uint64_t ref_pitch, uint32_t width, uint32_t height,
                  uint32_t texel_bytes, void* dst, uint64_t dst_capacity) {
    if (!ctx) return JH_ERR_INVALID;
    if (const char* why = pack_frame_error(src, src_pitch, width, height, texel_bytes)) return fail(ctx, JH_ERR_INVALID, std::string("jh_pack_tiles: source: ") + why);
    if (ref)
        if (const char* why = pack_frame_error(ref, ref_pitch, width, height, texel_bytes))
            return fail(ctx, JH_ERR_INVALID, std::string("jh_pack_tiles: reference: ") + why);
    if (!dst || (uintptr_t)dst % texel_bytes) return fail(ctx, JH_ERR_INVALID, "jh_pack_tiles: null destination, or not a multiple of texel_bytes");
    if (dst_capacity < jh_pack_bound(width, height, texel_bytes)) return fail(ctx, JH_ERR_INVALID, "jh_pack_tiles: dst_capacity below jh_pack_bound");
    void *cls = nullptr, *totals = nullptr;
    return post_render_call(
        ctx, "pack",
        [&] {
            const uint32_t n_tiles = ((width + 15u) / 16u) * ((height + 15u) / 16u);
            cls = jh_scratch_get(&ctx->scratch, JH_SCR_H, n_tiles);
            totals = jh_scratch_get(&ctx->scratch, JH_SCR_J, 8ull * jh_pack_groups(n_tiles, nullptr));
            if (cls && totals) return (int)JH_OK;
            return fail(ctx, JH_ERR_OOM, "jh_pack_tiles: " + scratch_failure(ctx, "pack a frame of this size once eagerly first"));
        },
        [&] { return launch_status(ctx, "jh_pack_tiles", jh_pack_launch(ctx->stream, src, src_pitch, ref, ref_pitch, width, height, texel_bytes, dst, cls, totals)); });
}

int jh_unpack_tiles(jh_ctx* ctx, const void* pack, uint64_t pack_bytes, void* dst, uint64_t dst_pitch, uint32_t width, uint32_t height,
                    uint32_t texel_bytes) {
    if (!ctx || !ctx->hint_overflow) return JH_ERR_INVALID;
    if (const char* why = pack_frame_error(dst, dst_pitch, width, height, texel_bytes)) return fail(ctx, JH_ERR_INVALID, std::string("jh_unpack_tiles: destination: ") + why);
    if (!pack || (uintptr_t)pack % texel_bytes) return fail(ctx, JH_ERR_INVALID, "jh_unpack_tiles: null pack, or not a multiple of texel_bytes");
    if (pack_bytes < 32u) return fail(ctx, JH_ERR_INVALID, "jh_unpack_tiles: pack_bytes below the header's 32");
    return post_render_call(ctx, "unpack", [&] {
        return launch_status(ctx, "jh_unpack_tiles", jh_unpack_launch(ctx->stream, pack, pack_bytes, dst, dst_pitch, width, height, texel_bytes,
                                                                      ctx->hint_overflow + kUnpackRejectWord));
    });
}

// dashing (include/jello_hip.h "dashing"; kernels_dash.hip)
int jh_dash(jh_ctx* ctx, const jh_dash_el* els, uint64_t n_els, const jh_dash_path* paths, uint32_t n_paths, const double* dashes,
            uint64_t n_dashes, void* out_els, uint64_t out_capacity, uint32_t* out_index) {
    if (!ctx) return JH_ERR_INVALID;
    if (!out_index || (!out_els && out_capacity) || (!els && n_els) || (!paths && n_paths) || (!dashes && n_dashes))
        return fail(ctx, JH_ERR_INVALID, "jh_dash: null pointer");
    if (n_paths == 0xffffffffu || out_capacity > 0xffffffffull) return fail(ctx, JH_ERR_INVALID, "jh_dash: too many paths, or a capacity above 2^32 - 1 elements");
    static_assert(sizeof(jh_dash_el) == sizeof(JDashInEl) && sizeof(jh_dash_path) == sizeof(JDashInPath) && sizeof(jh_dash_out_el) == sizeof(JDashEl),
                  "the C ABI's structs are the rule's");
    JDashJob job;
    if (const char* why = jdash_prepare((const JDashInEl*)els, n_els, (const JDashInPath*)paths, n_paths, dashes, n_dashes, &job))
        return fail(ctx, JH_ERR_INVALID, std::string("jh_dash: ") + why);
    if (ctx->capturing) return fail(ctx, JH_ERR_INVALID, "jh_dash: not during graph capture (its grids depend on the job)");
    if (job.segs.empty())  // nothing is drawn: every offset is 0
        return post_render_call(ctx, "dash", [&] {
            HIP_TRY(ctx, hipMemsetAsync(out_index, 0, ((uint64_t)n_paths + 1u) * 4u, ctx->stream));
            return (int)JH_OK;
        });
    // one upload for the whole job: [segs][subs][pats][runs][path_first_seg], each section on a 16-byte boundary
    auto al = [](uint64_t v) { return (v + 15u) & ~15ull; };
    const uint64_t o_subs = al(job.segs.size() * sizeof(JDashSeg)), o_pats = o_subs + al(job.subs.size() * sizeof(JDashSub));
    const uint64_t o_runs = o_pats + al(job.pats.size() * sizeof(JDashPat)), o_first = o_runs + al(job.runs.size() * sizeof(JDashRun));
    const uint64_t bytes = o_first + al(job.path_first_seg.size() * 4u);
    std::vector<char> blob(bytes, 0);
    std::memcpy(blob.data(), job.segs.data(), job.segs.size() * sizeof(JDashSeg));
    std::memcpy(blob.data() + o_subs, job.subs.data(), job.subs.size() * sizeof(JDashSub));
    std::memcpy(blob.data() + o_pats, job.pats.data(), job.pats.size() * sizeof(JDashPat));
    if (!job.runs.empty()) std::memcpy(blob.data() + o_runs, job.runs.data(), job.runs.size() * sizeof(JDashRun));
    std::memcpy(blob.data() + o_first, job.path_first_seg.data(), job.path_first_seg.size() * 4u);
    SlotUpload up;
    return post_render_call(
        ctx, "dash", [&] { return slot_upload_take(ctx, "jh_dash", "dash outside the capture", JH_SCR_A, blob.data(), bytes, &up); },
        [&] {
            if (int rc = slot_upload_send(ctx, up)) return rc;
            JhDashJob dj;
            dj.segs = (const JDashSeg*)up.dev; dj.subs = (const JDashSub*)(up.dev + o_subs); dj.pats = (const JDashPat*)(up.dev + o_pats);
            dj.runs = (const JDashRun*)(up.dev + o_runs); dj.path_first_seg = (const uint32_t*)(up.dev + o_first);
            dj.n_segs = (uint32_t)job.segs.size(); dj.n_subs = (uint32_t)job.subs.size(); dj.n_paths = n_paths;
            const std::vector<JhBound> none;
            const JhResult lr = jh_dash_launch(make_launch(ctx, 0, 0, 0, none), dj, out_els, out_capacity, out_index);
            if (lr == JH_L_SCRATCH) return fail(ctx, JH_ERR_OOM, "jh_dash: scratch allocation failed");
            if (hipGetLastError() != hipSuccess) return fail(ctx, JH_ERR_DEVICE, "jh_dash: launch failed");
            return (int)JH_OK;
        });
}

// The context-free queries of the image calls (include/jello_hip.h, call by call): each is its one body in include/jello_queries.h,
// which the host twin compiles too; the reason of a refusal stays there.
#define JH_QUERY(name, params, args) int jh_##name params { return jq_##name args ? JH_ERR_INVALID : JH_OK; }
JQ_QUERY_LIST(JH_QUERY)
#undef JH_QUERY

// blur (include/jello_hip.h "Gaussian blur"; the taps: include/jello_blur.h; kernels_blur.hip)
int jh_blur(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, uint32_t width, uint32_t height, const jh_blur_desc* desc) {
    Alloc *src = nullptr, *dst = nullptr;
    const uint32_t size[2] = {width, height};
    if (int rc = image_call_images(ctx, "jh_blur", desc, src_image_id, dst_image_id, nullptr, "the rows next to a band belong to another rank", &src, &dst, size)) return rc;
    if (!jblur_sigma_ok(desc->sigma_x) || !jblur_sigma_ok(desc->sigma_y)) return fail(ctx, JH_ERR_INVALID, "jh_blur: sigma is negative, above 64 or NaN");
    if (desc->edge != JH_BLUR_EDGE_ZERO && desc->edge != JH_BLUR_EDGE_CLAMP) return fail(ctx, JH_ERR_INVALID, "jh_blur: unknown edge mode");
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_blur", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    float taps_x[2u * JBLUR_MAX_RADIUS + 1u], taps_y[2u * JBLUR_MAX_RADIUS + 1u];
    const uint32_t radius_x = jblur_taps(desc->sigma_x, taps_x), radius_y = jblur_taps(desc->sigma_y, taps_y);
    void* tmp = nullptr;
    return post_render_call(
        ctx, "blur",
        [&] { return scratch_take(ctx, "jh_blur", "blur a rectangle of this size once eagerly first", JH_SCR_BLUR, jblur_scratch_bytes(r, radius_y, height), &tmp); },
        [&] {
            ImageViews v;
            if (int rc = image_call_views(ctx, src, dst, r, &v)) return rc;
            return launch_status(ctx, "jh_blur", jh_blur_launch(ctx->stream, v.from, v.to, r, desc->edge == JH_BLUR_EDGE_CLAMP, taps_x, radius_x, taps_y,
                                                                radius_y, tmp, ctx->num_cus));
        });
}

// composite (include/jello_hip.h "Composite"; the geometry: include/jello_composite.h; kernels_composite.hip)
int jh_composite(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_composite_desc* desc) {
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_composite", desc, src_image_id, dst_image_id, "a shifted blend in place reads what it writes", "a shifted source row belongs to another rank", &src, &dst)) return rc;
    if (desc->mix > 15u) return fail(ctx, JH_ERR_INVALID, "jh_composite: unknown mix mode (Mix.Clip is not a blend of two images)");
    if (desc->compose > 13u) return fail(ctx, JH_ERR_INVALID, "jh_composite: unknown compose operator");
    if (!(desc->opacity >= 0.0f && desc->opacity <= 1.0f)) return fail(ctx, JH_ERR_INVALID, "jh_composite: opacity is outside [0, 1] or NaN");
    if ((desc->flags & ~(uint32_t)JH_COMPOSITE_TINT) != 0u) return fail(ctx, JH_ERR_INVALID, "jh_composite: unknown flag bits");
    if (desc->flags & JH_COMPOSITE_TINT) {
        if (!std::isfinite(desc->tint[0]) || !std::isfinite(desc->tint[1]) || !std::isfinite(desc->tint[2]))
            return fail(ctx, JH_ERR_INVALID, "jh_composite: the tint colour is not finite");
        if (!(desc->tint[3] >= 0.0f && desc->tint[3] <= 1.0f)) return fail(ctx, JH_ERR_INVALID, "jh_composite: the tint alpha is outside [0, 1] or NaN");
    }
    jcomp_rect rect;
    if (jcomp_clip(src->width, src->height, desc->sx, desc->sy, desc->sw, desc->sh, desc->dx, desc->dy, dst->width, dst->height, &rect))
        return fail(ctx, JH_ERR_INVALID, "jh_composite: the source rectangle is not inside the source image or is empty in one dimension");
    if (rect.w == 0u || rect.h == 0u) return JH_OK;  // placed outside dst: nothing to write, nothing launched
    return post_render_call(ctx, "composite", [&] {
        const bool backdrop = dst->written || dst->stored;
        ImageViews v;
        if (int rc = image_call_views(ctx, src, dst, {rect.dx, rect.dy, rect.w, rect.h}, &v)) return rc;
        return launch_status(ctx, "jh_composite", jh_composite_launch(ctx->stream, v.from, v.to, backdrop, &rect, desc->mix << 8 | desc->compose, desc->flags,
                                                                      desc->opacity, desc->tint, ctx->num_cus));
    });
}

// resample (include/jello_hip.h "Resample"; windows and taps: include/jello_resample.h; kernels_resample.hip)
// The tables of one geometry as kernels_resample.hip reads them (JhResampleTables, kcommon.h), in one blob: [win_x][seg_x][w_x]
// [win_y][w_y], each section on a 16-byte boundary.  false for a window without taps (the rule has none).
struct ResampleBlob {
    std::vector<char> bytes;
    uint64_t o_seg_x = 0, o_w_x = 0, o_win_y = 0, o_w_y = 0;
    uint32_t taps_x = 0, stride_y = 0, region_x = 0;
};
static bool resample_build(int filter, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, ResampleBlob& b) {
    struct Axis { std::vector<uint32_t> first, count; std::vector<float> w; uint32_t most = 0; };
    auto axis = [&](uint32_t n_in, uint32_t n_out, Axis& a) {
        a.first.resize(n_out);
        a.count.resize(n_out);
        a.w.assign((size_t)n_out * JRESAMPLE_MAX_TAPS, 0.0f);
        for (uint32_t i = 0; i < n_out; i++) {
            a.count[i] = jresample_taps(filter, n_in, n_out, i, &a.w[(size_t)i * JRESAMPLE_MAX_TAPS], &a.first[i], nullptr);
            if (a.count[i] == 0u || (uint64_t)a.first[i] + a.count[i] > n_in) return false;
            a.most = std::max(a.most, a.count[i]);
        }
        return true;
    };
    Axis ax, ay;
    if (!axis(sw, dw, ax) || !axis(sh, dh, ay)) return false;
    auto al = [](uint64_t v) { return (v + 15u) & ~15ull; };
    const uint32_t segs = (dw + JH_RESAMPLE_ROW_SEG - 1u) / JH_RESAMPLE_ROW_SEG;
    b.taps_x = ax.most;
    b.stride_y = ay.most;
    b.o_seg_x = al(8ull * dw);
    b.o_w_x = b.o_seg_x + al(16ull * segs);
    b.o_win_y = b.o_w_x + al(4ull * ax.most * dw);
    b.o_w_y = b.o_win_y + al(8ull * dh);
    b.bytes.assign(b.o_w_y + al(4ull * ay.most * dh), 0);
    uint32_t* win_x = (uint32_t*)b.bytes.data();
    uint32_t* seg_x = (uint32_t*)(b.bytes.data() + b.o_seg_x);
    float* w_x = (float*)(b.bytes.data() + b.o_w_x);
    uint32_t* win_y = (uint32_t*)(b.bytes.data() + b.o_win_y);
    float* w_y = (float*)(b.bytes.data() + b.o_w_y);
    uint32_t longest = 1u;
    for (uint32_t s = 0; s < segs; s++) {
        uint32_t lo = 0xffffffffu, hi = 0u, most = 0u;
        for (uint32_t o = s * JH_RESAMPLE_ROW_SEG; o < dw && o < (s + 1u) * JH_RESAMPLE_ROW_SEG; o++) {
            lo = std::min(lo, ax.first[o]);
            hi = std::max(hi, ax.first[o] + ax.count[o]);
            most = std::max(most, ax.count[o]);
        }
        seg_x[4u * s] = lo; seg_x[4u * s + 1u] = hi - lo; seg_x[4u * s + 2u] = most;
        longest = std::max(longest, hi - lo);
    }
    b.region_x = jh_resample_skew(longest - 1u) + 1u;
    for (uint32_t o = 0; o < dw; o++) {
        win_x[2u * o] = ax.first[o]; win_x[2u * o + 1u] = ax.count[o];
        for (uint32_t j = 0; j < ax.count[o]; j++) w_x[(size_t)j * dw + o] = ax.w[(size_t)o * JRESAMPLE_MAX_TAPS + j];
    }
    for (uint32_t o = 0; o < dh; o++) {
        win_y[2u * o] = ay.first[o]; win_y[2u * o + 1u] = ay.count[o];
        for (uint32_t j = 0; j < ay.count[o]; j++) w_y[(size_t)o * ay.most + j] = ay.w[(size_t)o * JRESAMPLE_MAX_TAPS + j];
    }
    return true;
}

int jh_resample(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_resample_desc* desc) {
    static const char* const kRemedy = "resample this geometry once eagerly first";
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_resample", desc, src_image_id, dst_image_id, "a resize in place reads what it writes", "the rows a window reads belong to another rank", &src, &dst)) return rc;
    if (!jresample_filter_ok(desc->filter)) return fail(ctx, JH_ERR_INVALID, "jh_resample: unknown filter");
    if ((desc->flags & ~(uint32_t)JH_RESAMPLE_STRAIGHT) != 0u) return fail(ctx, JH_ERR_INVALID, "jh_resample: unknown flag bits");
    jimage_rect s, d;
    if (int rc = image_call_rect(ctx, "jh_resample", {desc->src_x, desc->src_y, desc->src_width, desc->src_height}, *src, "source ", &s)) return rc;
    if (int rc = image_call_rect(ctx, "jh_resample", {desc->dst_x, desc->dst_y, desc->dst_width, desc->dst_height}, *dst, "destination ", &d)) return rc;
    if (jimage_rect_empty(s) || jimage_rect_empty(d)) return fail(ctx, JH_ERR_INVALID, "jh_resample: an image without texels");
    if (!jresample_sizes_ok(s.w, d.w) || !jresample_sizes_ok(s.h, d.h)) return fail(ctx, JH_ERR_INVALID, "jh_resample: a ratio above 16:1");
    auto& key = ctx->resample;
    ResidentTables tables = {key.valid && key.filter == desc->filter && key.sw == s.w && key.sh == s.h && key.dw == d.w && key.dh == d.h, {}};
    ResampleBlob blob;
    if (tables.to_build(ctx) && !resample_build(desc->filter, s.w, s.h, d.w, d.h, blob)) return fail(ctx, JH_ERR_INVALID, "jh_resample: a window without taps");
    void* tmp = nullptr;
    return post_render_call(
        ctx, "resample",
        [&] {
            if (int rc = scratch_take(ctx, "jh_resample", kRemedy, JH_SCR_RESAMPLE, jresample_scratch_bytes(s, d), &tmp)) return rc;
            return tables_take(ctx, "jh_resample", kRemedy, JH_SCR_RESAMPLE_TAPS, blob.bytes, &tables);
        },
        [&] {
            ImageViews v;
            if (int rc = image_call_views(ctx, src, dst, d, &v)) return rc;
            const int rc = tables_send(ctx, tables, &key.valid, [&](const char* dev) {
                JhResampleTables& t = key.tables;
                t.win_x = (const uint2*)dev; t.seg_x = (const uint4*)(dev + blob.o_seg_x); t.w_x = (const float*)(dev + blob.o_w_x);
                t.win_y = (const uint2*)(dev + blob.o_win_y); t.w_y = (const float*)(dev + blob.o_w_y);
                t.taps_x = blob.taps_x; t.stride_y = blob.stride_y; t.region_x = blob.region_x;
                key.filter = desc->filter; key.sw = s.w; key.sh = s.h; key.dw = d.w; key.dh = d.h;
            });
            if (rc) return rc;
            return launch_status(ctx, "jh_resample", jh_resample_launch(ctx->stream, v.from, s, v.to, d, (desc->flags & JH_RESAMPLE_STRAIGHT) != 0u, &key.tables,
                                                                        tmp, ctx->num_cus));
        });
}

// colour filter (include/jello_hip.h "Colour filter"; the tables: include/jello_color.h; kernels_color.hip)
int jh_color_filter(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_color_desc* desc) {
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_color_filter", desc, src_image_id, dst_image_id, nullptr, "a band's rows are one rank's, the tables and their key the context's", &src, &dst)) return rc;
    if (const char* why = jcolor_desc_error(desc)) return fail(ctx, JH_ERR_INVALID, std::string("jh_color_filter: ") + why);
    for (float m : desc->matrix)
        if (!std::isfinite(m)) return fail(ctx, JH_ERR_INVALID, "jh_color_filter: a matrix entry is not finite");
    jimage_rect r;  // (named in the source, where 0 x 0 is the whole of it, and the same texels of the destination)
    if (int rc = image_call_rect(ctx, "jh_color_filter", {desc->x, desc->y, desc->width, desc->height}, *src, "source ", &r)) return rc;
    if (!jimage_rect_inside(r, dst->width, dst->height)) return refuse_rect(ctx, "jh_color_filter", JIMAGE_RECT_OUTSIDE, "destination ");
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    const uint32_t which = jcolor_which(desc);
    jcolor_key key;
    jcolor_key_of(desc, &key);
    // (a filter without tables does not touch the slot: nothing of it has to be resident)
    ResidentTables tables = {which == 0u || (ctx->color.valid && jcolor_key_equal(&ctx->color.key, &key)), {}};
    const uint64_t pre_bytes = 3ull * JCOLOR_ENTRIES * sizeof(float), all_bytes = pre_bytes + 4ull * JCOLOR_ENTRIES * sizeof(uint16_t);
    std::vector<char> blob;
    if (tables.to_build(ctx)) {
        blob.assign(all_bytes, 0);
        jcolor_tables(desc, (float*)blob.data(), (uint16_t*)(blob.data() + pre_bytes));
    }
    return post_render_call(
        ctx, "color", [&] { return tables_take(ctx, "jh_color_filter", "run this filter once eagerly first", JH_SCR_COLOR_TABLES, blob, &tables); },
        [&] {
            ImageViews v;
            if (int rc = image_call_views(ctx, src, dst, r, &v)) return rc;
            if (int rc = tables_send(ctx, tables, &ctx->color.valid, [&](const char* dev) { ctx->color.key = key; ctx->color.dev = dev; })) return rc;
            const char* dev = ctx->color.dev;
            const float* pre = (which & JCOLOR_PRE(0)) ? (const float*)dev : nullptr;
            const uint16_t* post[4];
            for (uint32_t i = 0; i < 4u; i++) post[i] = (which & JCOLOR_POST(i)) ? (const uint16_t*)(dev + pre_bytes) + (size_t)i * JCOLOR_ENTRIES : nullptr;
            return launch_status(ctx, "jh_color_filter",
                                 jh_color_launch(ctx->stream, v.from, v.to, r, desc->matrix, (desc->flags & JH_COLOR_CLAMP) != 0u, pre, post, ctx->num_cus));
        });
}

// 3D LUT (include/jello_hip.h "3D LUT"; the rule: include/jello_lut3d.h; kernels_lut3d.hip)
int jh_lut3d(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, uint64_t lut_image_id, const jh_lut3d_desc* desc) {
    static_assert(JH_LUT3D_MIN_SIZE == JLUT_MIN_SIZE && JH_LUT3D_MAX_SIZE == JLUT_MAX_SIZE, "the C ABI's values are the rule's");
    if (!ctx) return JH_ERR_INVALID;
    if (!desc) return fail(ctx, JH_ERR_INVALID, "jh_lut3d: null descriptor");
    Alloc *src = nullptr, *dst = nullptr, *lut = nullptr;
    if (int rc = rgba16f_images(ctx, "jh_lut3d", {{src_image_id, "source", &src}, {dst_image_id, "destination", &dst}, {lut_image_id, "LUT", &lut}})) return rc;
    if (const char* why = jlut_check(desc->size, desc->flags)) return fail(ctx, JH_ERR_INVALID, std::string("jh_lut3d: ") + why);
    if (const char* why = jlut_image_error(desc->size, lut->width, lut->height)) return fail(ctx, JH_ERR_INVALID, std::string("jh_lut3d: ") + why);
    if (lut == dst) return fail(ctx, JH_ERR_INVALID, "jh_lut3d: the LUT is the destination (the call would read entries it has written)");
    if (!(ctx->band_row0 == 0u && ctx->band_row1 == 0xffffffffu))
        return fail(ctx, JH_ERR_INVALID, "jh_lut3d: not in band mode (a band's rows are one rank's, the table the context's)");
    jimage_rect r;  // (named in the source, where 0 x 0 is the whole of it, and the same texels of the destination)
    if (int rc = image_call_rect(ctx, "jh_lut3d", {desc->x, desc->y, desc->width, desc->height}, *src, "source ", &r)) return rc;
    if (!jimage_rect_inside(r, dst->width, dst->height)) return refuse_rect(ctx, "jh_lut3d", JIMAGE_RECT_OUTSIDE, "destination ");
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    if (ctx->debug_lut3d == 2 && desc->size > JLUT_STAGED_MAX_SIZE) return fail(ctx, JH_ERR_INVALID, "jh_lut3d: jh_debug_lut3d_variant asks for a table in LDS, and this one does not fit");
    return post_render_call(ctx, "lut3d", [&] {
        const void* table = content_or_null(*lut);  // (taken first: the table may be the source, never the destination)
        ImageViews v;
        if (int rc = image_call_views(ctx, src, dst, r, &v)) return rc;
        return launch_status(ctx, "jh_lut3d", jh_lut3d_launch(ctx->stream, v.from, v.to, r, table, desc->size, ctx->debug_lut3d, ctx->num_cus));
    });
}

// morphology (include/jello_hip.h "Morphology"; the descriptor, the planes and the key: include/jello_morph.h; kernels_morph.hip)
int jh_morphology(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_morph_desc* desc) {
    static_assert(JH_MORPH_ERODE == JMORPH_ERODE && JH_MORPH_DILATE == JMORPH_DILATE && JH_MORPH_EDGE_ZERO == JMORPH_EDGE_ZERO &&
                      JH_MORPH_EDGE_CLAMP == JMORPH_EDGE_CLAMP && JH_MORPH_STRAIGHT == JMORPH_STRAIGHT && JH_MORPH_MAX_RADIUS == JMORPH_MAX_RADIUS,
                  "the C ABI's values are the rule's");
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_morphology", desc, src_image_id, dst_image_id, nullptr, "the rows next to a band belong to another rank", &src, &dst)) return rc;
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, JH_ERR_INVALID, "jh_morphology: the images differ in size");
    if (const char* why = jmorph_desc_error(desc->op, desc->edge, desc->flags, desc->radius_x, desc->radius_y)) return fail(ctx, JH_ERR_INVALID, std::string("jh_morphology: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_morphology", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    void* tmp = nullptr;
    return post_render_call(
        ctx, "morphology",
        [&] {
            return scratch_take(ctx, "jh_morphology", "run a call of this rectangle size and these radii once eagerly first", JH_SCR_MORPH,
                                jmorph_scratch_bytes(r.w, r.h, desc->radius_y), &tmp);
        },
        [&] {
            ImageViews v;
            if (int rc = image_call_views(ctx, src, dst, r, &v)) return rc;
            return launch_status(ctx, "jh_morphology",
                                 jh_morph_launch(ctx->stream, v.from, v.to, r, desc->op == JH_MORPH_DILATE, desc->edge == JH_MORPH_EDGE_CLAMP,
                                                 (desc->flags & JH_MORPH_STRAIGHT) != 0u, desc->radius_x, desc->radius_y, tmp, ctx->num_cus));
        });
}

// distance (include/jello_hip.h "Distance"; the descriptor, the planes and the per-axis pieces: include/jello_distance.h; kernels_distance.hip)
int jh_distance(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_distance_desc* desc) {
    static_assert(JH_DISTANCE_OUTER == JDIST_OUTER && JH_DISTANCE_INNER == JDIST_INNER && JH_DISTANCE_SIGNED == JDIST_SIGNED &&
                      JH_DISTANCE_EDGE_ZERO == JDIST_EDGE_ZERO && JH_DISTANCE_EDGE_CLAMP == JDIST_EDGE_CLAMP && JH_DISTANCE_STRAIGHT == JDIST_STRAIGHT &&
                      JH_DISTANCE_MAX_RADIUS == JDIST_MAX_RADIUS,
                  "the C ABI's values are the rule's");
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_distance", desc, src_image_id, dst_image_id, nullptr, "the rows next to a band belong to another rank", &src, &dst)) return rc;
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, JH_ERR_INVALID, "jh_distance: the images differ in size");
    if (const char* why = jdist_desc_error(desc)) return fail(ctx, JH_ERR_INVALID, std::string("jh_distance: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_distance", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    void* tmp = nullptr;
    return post_render_call(
        ctx, "distance",
        [&] {
            return scratch_take(ctx, "jh_distance", "run a call needing no less scratch (jh_distance_plan) once eagerly first", JH_SCR_DISTANCE,
                                jdist_scratch_bytes(r.w, r.h, desc->max_distance, desc->which), &tmp);
        },
        [&] {
            ImageViews v;
            if (int rc = image_call_views(ctx, src, dst, r, &v)) return rc;
            return launch_status(ctx, "jh_distance", jh_distance_launch(ctx->stream, v.from, v.to, r, desc, tmp, ctx->num_cus));
        });
}

// stats (include/jello_hip.h "Stats"; the descriptor, the plan, the partial and the record: include/jello_stats.h; kernels_stats.hip)
int jh_stats(jh_ctx* ctx, uint64_t src_image_id, const jh_stats_desc* desc, void* out_device_ptr) {
    static_assert(JH_STATS_ALL == JSTATS_ALL && JH_STATS_CONTENT == JSTATS_CONTENT && JH_STATS_LINEAR == JSTATS_LINEAR && JH_STATS_SRGB == JSTATS_SRGB &&
                      JH_STATS_BOUNDS == JSTATS_BOUNDS && JH_STATS_EXTREMES == JSTATS_EXTREMES && JH_STATS_HISTOGRAM == JSTATS_HISTOGRAM &&
                      JH_STATS_MAX_TEXELS == JSTATS_MAX_TEXELS && JH_STATS_MAX_PARTIALS == JSTATS_MAX_PARTIALS,
                  "the C ABI's values are the rule's");
    if (!ctx) return JH_ERR_INVALID;
    if (!desc) return fail(ctx, JH_ERR_INVALID, "jh_stats: null descriptor");
    if (!out_device_ptr) return fail(ctx, JH_ERR_INVALID, "jh_stats: null out pointer");
    if (((uintptr_t)out_device_ptr & 7u) != 0u) return fail(ctx, JH_ERR_INVALID, "jh_stats: the out pointer is not 8-byte aligned");
    Alloc* src = nullptr;
    if (int rc = rgba16f_images(ctx, "jh_stats", {{src_image_id, "source", &src}})) return rc;
    if (const char* why = jstats_desc_error(desc)) return fail(ctx, JH_ERR_INVALID, std::string("jh_stats: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_stats", {desc->x, desc->y, desc->width, desc->height}, *src, "", &r)) return rc;
    if (const char* why = jstats_rect_error(desc, src->width, src->height, &r)) return fail(ctx, JH_ERR_INVALID, std::string("jh_stats: ") + why);
    if (!(ctx->band_row0 == 0u && ctx->band_row1 == 0xffffffffu))
        return fail(ctx, JH_ERR_INVALID, "jh_stats: not in band mode (the rows outside a band belong to another rank)");
    void* tmp = nullptr;
    return post_render_call(
        ctx, "stats",
        [&] {
            if (jimage_rect_empty(r)) return (int)JH_OK;  // (an image without texels: the record's header and zeros, no partials)
            return scratch_take(ctx, "jh_stats", "run one jh_stats call once eagerly first", JH_SCR_STATS, jstats_scratch_bytes(r), &tmp);
        },
        [&] {
            // (the source is only read: nothing is cleared and nothing counts as written)
            const jimage_src from = {content_or_null(*src), src->width, src->height};
            return launch_status(ctx, "jh_stats", jh_stats_launch(ctx->stream, from, r, desc, out_device_ptr, tmp, ctx->num_cus));
        });
}

extern "C++" {  // (a template cannot have C linkage)
// What jh_warp, jh_displace and jh_perspective do alike between their own checks.  warp_family_rects: the source and the destination
// rectangle the descriptor names, resolved into *s and *d, or the refusal.  warp_family_views: image_call_views for the destination
// rectangle d, and a source rectangle without texels reads as transparent black: nothing is loaded, and the launcher gets a texel it
// can name.
template <class Desc>
static int warp_family_rects(jh_ctx* ctx, const char* who, const Desc* desc, const Alloc& src, const Alloc& dst, jimage_rect* s, jimage_rect* d) {
    if (int rc = image_call_rect(ctx, who, {desc->src_x, desc->src_y, desc->src_width, desc->src_height}, src, "source ", s)) return rc;
    return image_call_rect(ctx, who, {desc->dst_x, desc->dst_y, desc->dst_width, desc->dst_height}, dst, "destination ", d);
}
}
static int warp_family_views(jh_ctx* ctx, const Alloc* src, Alloc* dst, jimage_rect* s, jimage_rect d, ImageViews* v) {
    if (int rc = image_call_views(ctx, src, dst, d, v)) return rc;
    if (jimage_rect_empty(*s)) {
        v->from = {nullptr, std::max(src->width, 1u), std::max(src->height, 1u)};
        *s = {s->x, s->y, std::max(s->w, 1u), std::max(s->h, 1u)};
    }
    return JH_OK;
}

// warp (include/jello_hip.h "Warp"; the plan, the bounds and the descriptor: include/jello_warp.h; kernels_warp.hip, warp_taps.h)
int jh_warp(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_warp_desc* desc) {
    static_assert(JH_WARP_NEAREST == JWARP_NEAREST && JH_WARP_BILINEAR == JWARP_BILINEAR && JH_WARP_BICUBIC == JWARP_BICUBIC &&
                      JH_WARP_EDGE_ZERO == JWARP_EDGE_ZERO && JH_WARP_EDGE_CLAMP == JWARP_EDGE_CLAMP && JH_WARP_EDGE_REPEAT == JWARP_EDGE_REPEAT &&
                      JH_WARP_EDGE_MIRROR == JWARP_EDGE_MIRROR && JH_WARP_STRAIGHT == JWARP_STRAIGHT && JH_WARP_MAX_SIDE == JWARP_MAX_SIDE,
                  "the C ABI's values are the rule's");
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_warp", desc, src_image_id, dst_image_id, "a warp in place reads what it writes", "the rows a tap reads belong to another rank", &src, &dst)) return rc;
    if (const char* why = jwarp_desc_error(desc->filter, desc->edge, desc->flags, src->width, src->height, dst->width, dst->height))
        return fail(ctx, JH_ERR_INVALID, std::string("jh_warp: ") + why);
    jimage_rect s, d;
    if (int rc = warp_family_rects(ctx, "jh_warp", desc, *src, *dst, &s, &d)) return rc;
    int64_t plan[6];
    if (const char* why = jwarp_plan(desc->matrix, plan)) return fail(ctx, JH_ERR_INVALID, std::string("jh_warp: illegal matrix: ") + why);
    if (jimage_rect_empty(d)) return JH_OK;  // (an image without texels)
    return post_render_call(ctx, "warp", [&] {
        ImageViews v;
        if (int rc = warp_family_views(ctx, src, dst, &s, d, &v)) return rc;
        return launch_status(ctx, "jh_warp",
                             jh_warp_launch(ctx->stream, v.from, s, v.to, d, plan, desc->filter, desc->edge, (desc->flags & JH_WARP_STRAIGHT) != 0u, ctx->num_cus));
    });
}

// convolve (include/jello_hip.h "Convolve"; the descriptor and the weights: include/jello_convolve.h; kernels_convolve.hip)
int jh_convolve(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_convolve_desc* desc) {
    static_assert(JH_CONVOLVE_EDGE_ZERO == JCONV_EDGE_ZERO && JH_CONVOLVE_EDGE_CLAMP == JCONV_EDGE_CLAMP && JH_CONVOLVE_EDGE_REPEAT == JCONV_EDGE_REPEAT &&
                      JH_CONVOLVE_EDGE_MIRROR == JCONV_EDGE_MIRROR && JH_CONVOLVE_PREMULTIPLIED == JCONV_PREMULTIPLIED &&
                      JH_CONVOLVE_STRAIGHT == JCONV_STRAIGHT && JH_CONVOLVE_PRESERVE_ALPHA == JCONV_PRESERVE_ALPHA &&
                      JH_CONVOLVE_MAX_ORDER == JCONV_MAX_ORDER && JH_CONVOLVE_MAX_TAPS == JCONV_MAX_TAPS &&
                      (int)JH_CONVOLVE_EDGE_ZERO == (int)JH_WARP_EDGE_ZERO && (int)JH_CONVOLVE_EDGE_MIRROR == (int)JH_WARP_EDGE_MIRROR,
                  "the C ABI's values are the rule's");
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_convolve", desc, src_image_id, dst_image_id, "a tile of a convolution in place reads what another tile wrote", "the rows a window reads belong to another rank", &src, &dst)) return rc;
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, JH_ERR_INVALID, "jh_convolve: the images differ in size");
    if (const char* why = jconv_desc_error(desc->order_x, desc->order_y, desc->target_x, desc->target_y, desc->edge, desc->mode, desc->weights, desc->bias))
        return fail(ctx, JH_ERR_INVALID, std::string("jh_convolve: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_convolve", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    return post_render_call(ctx, "convolve", [&] {
        ImageViews v;
        if (int rc = image_call_views(ctx, src, dst, r, &v)) return rc;
        return launch_status(ctx, "jh_convolve",
                             jh_convolve_launch(ctx->stream, v.from, v.to, r, desc->order_x, desc->order_y, desc->target_x, desc->target_y, desc->weights,
                                                desc->edge, desc->mode, desc->bias, ctx->num_cus));
    });
}

// lighting (include/jello_hip.h "Lighting"; the descriptor, the plan, the tables and the key: include/jello_lighting.h; kernels_lighting.hip)
int jh_lighting(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_lighting_desc* desc) {
    static_assert(JH_LIGHTING_DIFFUSE == JLIGHT_DIFFUSE && JH_LIGHTING_SPECULAR == JLIGHT_SPECULAR && JH_LIGHT_DISTANT == JLIGHT_DISTANT &&
                      JH_LIGHT_POINT == JLIGHT_POINT && JH_LIGHT_SPOT == JLIGHT_SPOT && JH_LIGHTING_TABLE_ENTRIES == JLIGHT_ENTRIES &&
                      JH_LIGHTING_TABLE_SPEC == JLIGHT_TABLE_SPEC && JH_LIGHTING_TABLE_SPOT == JLIGHT_TABLE_SPOT && JH_LIGHTING_MAX_EXTENT == JLIGHT_MAX_EXTENT,
                  "the C ABI's values are the rule's");
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_lighting", desc, src_image_id, dst_image_id, "a tile of a lighting in place reads alpha that another tile overwrote", "the rows a normal reads belong to another rank, the tables and their key to the context", &src, &dst)) return rc;
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, JH_ERR_INVALID, "jh_lighting: the images differ in size");
    if (dst->width > JLIGHT_MAX_EXTENT || dst->height > JLIGHT_MAX_EXTENT) return fail(ctx, JH_ERR_INVALID, "jh_lighting: an image extent above 2^23");
    jh_light_plan plan;
    if (const char* why = jlight_plan(desc, &plan)) return fail(ctx, JH_ERR_INVALID, std::string("jh_lighting: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_lighting", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    const uint32_t which = jlight_which(desc);
    jlight_key key;
    jlight_key_of(desc, &key);
    // (a call without tables does not touch the slot: nothing of it has to be resident)
    ResidentTables tables = {which == 0u || (ctx->light.valid && jlight_key_equal(&ctx->light.key, &key)), {}};
    const uint64_t table_bytes = (uint64_t)JLIGHT_ENTRIES * sizeof(float);
    std::vector<char> blob;
    if (tables.to_build(ctx)) {
        blob.assign(2u * table_bytes, 0);
        jlight_tables(desc, (float*)blob.data(), (float*)(blob.data() + table_bytes));
    }
    return post_render_call(
        ctx, "lighting", [&] { return tables_take(ctx, "jh_lighting", "run this lighting once eagerly first", JH_SCR_LIGHT_TABLES, blob, &tables); },
        [&] {
            ImageViews v;
            if (int rc = image_call_views(ctx, src, dst, r, &v)) return rc;
            if (int rc = tables_send(ctx, tables, &ctx->light.valid, [&](const char* dev) { ctx->light.key = key; ctx->light.dev = dev; })) return rc;
            const char* dev = ctx->light.dev;
            const float* spec = (which & JLIGHT_TABLE_SPEC) ? (const float*)dev : nullptr;
            const float* spot = (which & JLIGHT_TABLE_SPOT) ? (const float*)(dev + table_bytes) : nullptr;
            return launch_status(ctx, "jh_lighting",
                                 jh_lighting_launch(ctx->stream, v.from, v.to, r, desc->kind, desc->light, &plan, desc->surface_scale, desc->constant, desc->color, spec,
                                                    spot, ctx->num_cus));
        });
}

// turbulence (include/jello_hip.h "Turbulence"; the descriptor, the generator, the tables, the plan and the key: include/jello_turbulence.h; kernels_turbulence.hip)
int jh_turbulence(jh_ctx* ctx, uint64_t dst_image_id, const jh_turbulence_desc* desc) {
    static_assert(JH_TURBULENCE_FRACTAL_NOISE == JTURB_FRACTAL_NOISE && JH_TURBULENCE_TURBULENCE == JTURB_TURBULENCE && JH_TURBULENCE_MAX_OCTAVES == JTURB_MAX_OCTAVES,
                  "the C ABI's values are the rule's");
    Alloc* dst = nullptr;
    if (int rc = image_call_image(ctx, "jh_turbulence", desc, dst_image_id, "a band's rows are one rank's, the tables and their key the context's", &dst)) return rc;
    jh_turb_plan plan;
    if (const char* why = jturb_plan(desc, &plan)) return fail(ctx, JH_ERR_INVALID, std::string("jh_turbulence: ") + why);
    if (dst->width > plan.max_extent[0] || dst->height > plan.max_extent[1])
        return fail(ctx, JH_ERR_INVALID, "jh_turbulence: the image reaches beyond the position range of this many octaves (max_extent of the plan)");
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_turbulence", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    ResidentTables tables = {ctx->turb.valid && ctx->turb.key == plan.key, {}};
    std::vector<char> blob;
    if (tables.to_build(ctx)) {
        uint8_t P[256];
        std::vector<float> G(JTURB_GRADIENT_FLOATS);
        jturb_tables(desc->seed, P, G.data());
        blob.assign(JTURB_DEVICE_BYTES, 0);
        jturb_device_tables(P, G.data(), blob.data());
    }
    return post_render_call(
        ctx, "turbulence", [&] { return tables_take(ctx, "jh_turbulence", "run this turbulence once eagerly first", JH_SCR_TURB_TABLES, blob, &tables); },
        [&] {
            if (int rc = first_content(ctx, dst, r.w, r.h)) return rc;
            if (int rc = tables_send(ctx, tables, &ctx->turb.valid, [&](const char* dev) { ctx->turb.key = plan.key; ctx->turb.dev = dev; })) return rc;
            return launch_status(ctx, "jh_turbulence",
                                 jh_turbulence_launch(ctx->stream, {dst->ptr, dst->width, dst->height}, r, desc->kind, desc->octaves, &plan, ctx->turb.dev, ctx->num_cus));
        });
}

// displace (include/jello_hip.h "Displace"; the descriptor and the offset: include/jello_displace.h; the plan: include/jello_warp.h; kernels_displace.hip, warp_taps.h)
int jh_displace(jh_ctx* ctx, uint64_t src_image_id, uint64_t map_image_id, uint64_t dst_image_id, const jh_displace_desc* desc) {
    static_assert(JH_DISPLACE_R == JDISP_R && JH_DISPLACE_G == JDISP_G && JH_DISPLACE_B == JDISP_B && JH_DISPLACE_A == JDISP_A &&
                      JH_DISPLACE_STRAIGHT == JDISP_STRAIGHT && JH_DISPLACE_STRAIGHT == JH_WARP_STRAIGHT,
                  "the C ABI's values are the rule's");
    Alloc *src = nullptr, *dst = nullptr, *map = nullptr;
    if (int rc = image_call_images(ctx, "jh_displace", desc, src_image_id, dst_image_id, "a displacement in place reads what it writes", "the rows a tap reads belong to another rank", &src, &dst)) return rc;
    if (int rc = rgba16f_images(ctx, "jh_displace", {{map_image_id, "map", &map}})) return rc;
    if (const char* why = jdisp_desc_error(desc->filter, desc->edge, desc->flags, desc->scale_x, desc->scale_y, desc->x_channel, desc->y_channel, src->width,
                                           src->height, map->width, map->height, dst->width, dst->height))
        return fail(ctx, JH_ERR_INVALID, std::string("jh_displace: ") + why);
    jimage_rect s, d;
    if (int rc = warp_family_rects(ctx, "jh_displace", desc, *src, *dst, &s, &d)) return rc;
    int64_t plan[6];
    if (const char* why = jwarp_plan(desc->matrix, plan)) return fail(ctx, JH_ERR_INVALID, std::string("jh_displace: illegal matrix: ") + why);
    if (jimage_rect_empty(d)) return JH_OK;  // (an image without texels)
    return post_render_call(ctx, "displace", [&] {
        const jimage_src from_map = {content_or_null(*map), map->width, map->height};  // (taken first: the map may be dst, and a never-written one reads 0, not its memory)
        ImageViews v;
        if (int rc = warp_family_views(ctx, src, dst, &s, d, &v)) return rc;
        return launch_status(ctx, "jh_displace",
                             jh_displace_launch(ctx->stream, v.from, s, from_map, v.to, d, plan, desc->scale_x, desc->scale_y, desc->x_channel, desc->y_channel,
                                                desc->filter, desc->edge, (desc->flags & JH_DISPLACE_STRAIGHT) != 0u, ctx->num_cus));
    });
}

// shadow (include/jello_hip.h "Shadow"; the descriptor, the plan and the coverage: include/jello_shadow.h; the matrix: include/jello_warp.h; kernels_shadow.hip)
int jh_shadow(jh_ctx* ctx, uint64_t dst_image_id, const jh_shadow_desc* desc) {
    static_assert(JH_SHADOW_OVER == JSHADOW_OVER && JH_SHADOW_INVERT == JSHADOW_INVERT, "the C ABI's values are the rule's");
    Alloc* dst = nullptr;
    if (int rc = image_call_image(ctx, "jh_shadow", desc, dst_image_id, "a band's rows are one rank's, the call writes its whole rectangle", &dst)) return rc;
    if (const char* why = jshadow_extent_error(dst->width, dst->height)) return fail(ctx, JH_ERR_INVALID, std::string("jh_shadow: ") + why);
    if (const char* why = jshadow_desc_error(desc)) return fail(ctx, JH_ERR_INVALID, std::string("jh_shadow: ") + why);
    jh_shad_plan plan;
    if (const char* why = jshadow_plan(desc, &plan)) return fail(ctx, JH_ERR_INVALID, std::string("jh_shadow: illegal matrix: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_shadow", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    return post_render_call(ctx, "shadow", [&] {
        const bool backdrop = dst->written || dst->stored;  // (taken first: OVER onto a never-written image blends onto transparent black)
        if (int rc = first_content(ctx, dst, r.w, r.h)) return rc;
        return launch_status(ctx, "jh_shadow",
                             jh_shadow_launch(ctx->stream, {dst->ptr, dst->width, dst->height}, backdrop, r, &plan, desc->color, desc->flags, ctx->num_cus));
    });
}

// perspective (include/jello_hip.h "Perspective"; the plan, the position and the bounds: include/jello_perspective.h; kernels_perspective.hip, warp_taps.h)
int jh_perspective(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_perspective_desc* desc) {
    static_assert(JH_PERSPECTIVE_STRAIGHT == JPERSP_STRAIGHT && JH_PERSPECTIVE_STRAIGHT == JH_WARP_STRAIGHT, "the C ABI's values are the rule's");
    Alloc *src = nullptr, *dst = nullptr;
    if (int rc = image_call_images(ctx, "jh_perspective", desc, src_image_id, dst_image_id, "a warp in place reads what it writes", "the rows a tap reads belong to another rank", &src, &dst)) return rc;
    if (const char* why = jpersp_desc_error(desc->filter, desc->edge, desc->flags, src->width, src->height, dst->width, dst->height))
        return fail(ctx, JH_ERR_INVALID, std::string("jh_perspective: ") + why);
    jimage_rect s, d;
    if (int rc = warp_family_rects(ctx, "jh_perspective", desc, *src, *dst, &s, &d)) return rc;
    double plan[9];
    if (const char* why = jpersp_plan(desc->matrix, plan)) return fail(ctx, JH_ERR_INVALID, std::string("jh_perspective: illegal matrix: ") + why);
    if (jimage_rect_empty(d)) return JH_OK;  // (an image without texels)
    return post_render_call(ctx, "perspective", [&] {
        ImageViews v;
        if (int rc = warp_family_views(ctx, src, dst, &s, d, &v)) return rc;
        return launch_status(ctx, "jh_perspective",
                             jh_perspective_launch(ctx->stream, v.from, s, v.to, d, plan, desc->filter, desc->edge, (desc->flags & JH_PERSPECTIVE_STRAIGHT) != 0u, ctx->num_cus));
    });
}

// load (include/jello_hip.h "load"; legality, tables, texel: include/jello_load.h and jello_frame.h; kernels_load.hip): null planes before the rectangle, pitches after it
int jh_load_surface(jh_ctx* ctx, uint64_t dst_image_id, const jh_load_surface_desc* desc) {
    Alloc* dst = nullptr;
    if (int rc = image_call_image(ctx, "jh_load_surface", desc, dst_image_id, "a band's rows are one rank's, the frame is the whole rectangle's", &dst)) return rc;
    if (const char* why = jload_surface_desc_error(desc)) return fail(ctx, JH_ERR_INVALID, std::string("jh_load_surface: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_load_surface", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (const char* why = jframe_surface_pitch_error(desc->pitch, r.w)) return fail(ctx, JH_ERR_INVALID, std::string("jh_load_surface: ") + why);
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    return post_render_call(ctx, "load_surface", [&] {
        if (int rc = first_content(ctx, dst, r.w, r.h)) return rc;
        return launch_status(ctx, "jh_load_surface",
                             jh_load_surface_launch(ctx->stream, desc->src, desc->pitch, {dst->ptr, dst->width, dst->height}, r, desc->format, desc->alpha, ctx->num_cus));
    });
}

int jh_load_yuv(jh_ctx* ctx, uint64_t dst_image_id, const jh_load_yuv_desc* desc) {
    Alloc* dst = nullptr;
    if (int rc = image_call_image(ctx, "jh_load_yuv", desc, dst_image_id, "a band's rows are one rank's, the frame is the whole rectangle's", &dst)) return rc;
    if (const char* why = jload_yuv_desc_error(desc)) return fail(ctx, JH_ERR_INVALID, std::string("jh_load_yuv: ") + why);
    jimage_rect r;
    if (int rc = image_call_rect(ctx, "jh_load_yuv", {desc->x, desc->y, desc->width, desc->height}, *dst, "", &r)) return rc;
    if (const char* why = jframe_yuv_planes_error(desc->layout, desc->plane, desc->pitch, r.w, JFRAME_SHORT_PITCH)) return fail(ctx, JH_ERR_INVALID, std::string("jh_load_yuv: ") + why);
    if (jimage_rect_empty(r)) return JH_OK;  // (an image without texels)
    return post_render_call(ctx, "load_yuv", [&] {
        if (int rc = first_content(ctx, dst, r.w, r.h)) return rc;
        return launch_status(ctx, "jh_load_yuv", jh_load_yuv_launch(ctx->stream, desc->plane, desc->pitch, {dst->ptr, dst->width, dst->height}, r, desc->layout,
                                                                    desc->matrix, desc->range, desc->transfer, desc->chroma, ctx->num_cus));
    });
}

// Entries (or whole packs, counted once) jh_unpack_tiles has ignored since the last reset.  Synchronises the stream.
int jh_debug_unpack_rejects(jh_ctx* ctx, uint32_t* count, int reset) {
    if (!ctx || !ctx->hint_overflow) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    return counter_words(ctx, kUnpackRejectWord, 1, count, reset);
}

int jh_selftest_math(jh_ctx* ctx, int op, const float* a, const float* b, float* out, uint32_t n) {
    if (!ctx || !a || !out) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    size_t bytes = (size_t)n * 4;
    HIP_TRY(ctx, hipMalloc(&da, bytes ? bytes : 4));
    HIP_TRY(ctx, hipMalloc(&dout, bytes ? bytes : 4));
    if (b) HIP_TRY(ctx, hipMalloc(&db, bytes ? bytes : 4));
    HIP_TRY(ctx, hipMemcpyAsync(da, a, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (b) HIP_TRY(ctx, hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, ctx->stream));
    int rc = jh_selftest_math_launch(ctx->stream, op, da, db, dout, n);
    if (rc == 0) {
        HIP_TRY(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    (void)hipFree(da); (void)hipFree(dout);
    if (db) (void)hipFree(db);
    return rc == 0 ? JH_OK : fail(ctx, JH_ERR_DEVICE, "selftest launch failed");
}

int jh_selftest_atomics(jh_ctx* ctx, int form, uint32_t seed, uint32_t n_waves) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = jh_selftest_atomics_launch(ctx->stream, form, seed, n_waves);
    if (rc == -1) return fail(ctx, JH_ERR_INVALID, "selftest_atomics: form 0..2, 1..4096 waves");
    if (rc < 0) return fail(ctx, JH_ERR_DEVICE, "selftest_atomics: runtime error");
    return rc;
}

int jh_debug_poison_scratch(jh_ctx* ctx, int byte) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < JH_SCR_COUNT; i++) {
        if (i == JH_SCR_RESAMPLE_TAPS || i == JH_SCR_COLOR_TABLES || i == JH_SCR_LIGHT_TABLES || i == JH_SCR_TURB_TABLES) continue;  // (uploaded content a captured jh_resample / jh_color_filter / jh_lighting / jh_turbulence reads, not an array a frame fills before it reads it)
        if (ctx->scratch.ptr[i] && ctx->scratch.cap[i]) HIP_TRY(ctx, hipMemsetAsync(ctx->scratch.ptr[i], byte, ctx->scratch.cap[i], ctx->stream));
    }
    ctx->scratch.clean_flags = 0u;
    return JH_OK;
}

int jh_set_clip_depth_hint(jh_ctx* ctx, uint32_t max_depth) {
    if (!ctx) return JH_ERR_INVALID;
    // (a captured graph has the layout of its capture baked in and never looks at the hint again; its scratch pointer stays
    // valid until the array is regrown, which bumps the generation by itself)
    ctx->clip_depth_hint = max_depth;
    return JH_OK;
}
// Tests: flatten's temporary is cut into regions that a frame only fills up (and leaves behind, marking the slots at their ends
// empty) when it comes close to the capacity of its line buffer.  Bit 0: every wave starts in region 0; bit 1: eight regions
// whatever the capacity -- so that ordinary scenes take that path; bit 2: batches allocate their slots job by job (the product does
// above 51 200 lines per batch); bit 3: k_flatten_items runs as one workgroup (four waves, one unit counter: the edges of its work
// distribution at small item counts).  Results never depend on it.
int jh_debug_flatten_regions(jh_ctx* ctx, uint32_t flags) {
    if (!ctx) return JH_ERR_INVALID;
    ctx->debug_flatten = flags;
    ctx->generation++;  // (a captured graph holds the old kernel arguments)
    return JH_OK;
}
// Tests and timing: the instantiation jh_lut3d launches (0: the launcher's choice, 1: gathers from memory, 2: the table in LDS).
int jh_debug_lut3d_variant(jh_ctx* ctx, int variant) {
    if (!ctx || variant < 0 || variant > 2) return JH_ERR_INVALID;
    ctx->debug_lut3d = variant;
    return JH_OK;
}
// Tests: jh_scan_u32 -- the look-back scan has no stage id -- on the context's stream and scratch, on context buffers.  The checks
// are what keeps the kernel inside them: it reads in[(n - 1) * stride] and writes out[n - 1] at most, n <= n_max.
int jh_debug_scan_u32(jh_ctx* ctx, uint64_t in_id, uint64_t out_id, uint32_t stride, uint32_t n_max, uint64_t count_id, uint32_t count_word,
                      uint64_t total_id, uint32_t total_word) {
    if (!ctx) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Alloc* in = find_alloc(ctx->buffers, in_id);
    const Alloc* out = find_alloc(ctx->buffers, out_id);
    const Alloc* count = count_id ? find_alloc(ctx->buffers, count_id) : nullptr;
    const Alloc* total = total_id ? find_alloc(ctx->buffers, total_id) : nullptr;
    if (!in || !out || (count_id && !count) || (total_id && !total)) return fail(ctx, JH_ERR_INVALID, "jh_debug_scan_u32: unknown buffer");
    if (stride == 0u || in->size < (uint64_t)n_max * stride * 4u || out->size < (uint64_t)n_max * 4u || in == out ||
        (count && count->size < ((uint64_t)count_word + 1u) * 4u) || (total && total->size < ((uint64_t)total_word + 1u) * 4u))
        return fail(ctx, JH_ERR_INVALID, "jh_debug_scan_u32: stride 0 or a buffer too small for n_max");
    static const std::vector<JhBound> none;
    const JhResult r = jh_scan_u32(make_launch(ctx, 0, 0, 0, none), (const uint32_t*)in->ptr, stride, (uint32_t*)out->ptr, n_max,
                                   count ? (const uint32_t*)count->ptr + count_word : nullptr, total ? (uint32_t*)total->ptr + total_word : nullptr);
    if (r != JH_L_OK) return launch_result(ctx, -1, r);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? hip_fail(ctx, e, "jh_debug_scan_u32") : (int)JH_OK;
}
// Blend-stack saves the fine stage dropped since the last reset because jh_set_clip_depth_hint promised a shallower scene than
// it got (every one of them is a wrong pixel colour): 0 for every correct hint.  Synchronises the stream.
int jh_debug_clip_hint_overflows(jh_ctx* ctx, uint32_t* count, int reset) {
    if (!ctx || !ctx->hint_overflow) return JH_ERR_INVALID;
    JH_FLUSH(ctx);
    return counter_words(ctx, kHintOverflowWord, 1, count, reset);
}
#ifdef FINE_TIMING
extern "C" int jh_debug_fine_timing(jh_ctx* ctx, unsigned long long* out6, int reset) {
    if (!ctx || !ctx->hint_overflow) return JH_ERR_INVALID;
    return counter_words(ctx, kFineTimingWord, 12, out6, reset);
}
#endif
uint64_t jh_debug_scratch_bytes(jh_ctx* ctx, int slot) {
    if (!ctx) return 0;
    if (slot == -1) {  // all of them
        uint64_t sum = 0;
        for (int i = 0; i < JH_SCR_COUNT; i++) sum += ctx->scratch.cap[i];
        return sum;
    }
    return (slot >= 0 && slot < JH_SCR_COUNT) ? ctx->scratch.cap[slot] : 0;
}
// The scratch arrays only grow; a context that has rendered one much larger frame (or one frame with the estimator's generous
// bump sizes before the regrow loop settled on the real ones) keeps that size.  This gives all of it back: waits for the
// stream, frees every array; the next frame allocates what it needs.  Captured graphs hold the old pointers: they are stale
// afterwards (generation check) and must be captured again.
int jh_scratch_trim(jh_ctx* ctx) {
    if (!ctx) return JH_ERR_INVALID;
    if (ctx->capturing) return fail(ctx, JH_ERR_INVALID, "jh_scratch_trim during a graph capture");
    JH_FLUSH(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    scratch_release_retired(&ctx->scratch);
    for (int i = 0; i < JH_SCR_COUNT; i++) {
        if (ctx->scratch.base[i]) (void)hipFree(ctx->scratch.base[i]);
        ctx->scratch.base[i] = nullptr;
        ctx->scratch.ptr[i] = nullptr;
        ctx->scratch.cap[i] = 0;
    }
    ctx->scratch.clean_flags = 0;  // (new memory holds anything: every self-cleaned array is filled again on its next use)
    ctx->resample.valid = false;   // (jh_resample's tables went with their slot)
    ctx->color.valid = false;      // (jh_color_filter's likewise)
    ctx->light.valid = false;      // (jh_lighting's likewise)
    ctx->turb.valid = false;       // (jh_turbulence's likewise)
    ctx->generation++;
    return JH_OK;
}
uint64_t jh_debug_graph_self_cleans(jh_ctx* ctx) { return ctx ? ctx->graph_self_cleans : 0; }

int jh_device_info(jh_ctx* ctx, char* name, int name_len, int* compute_units, uint64_t* total_mem) {
    if (!ctx) return JH_ERR_INVALID;
    if (name && name_len > 0) {
        std::strncpy(name, ctx->name.c_str(), (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    if (compute_units) *compute_units = ctx->num_cus;
    if (total_mem) *total_mem = ctx->total_mem;
    return JH_OK;
}

uint64_t jh_pool_bytes(jh_ctx* ctx) { return ctx ? ctx->pool_bytes : 0; }

}  // extern "C"
