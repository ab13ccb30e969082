// kernels_pack.hip -- jh_pack_tiles / jh_unpack_tiles: a frame as only the bytes that have to travel, and back.
// The format is in include/jello_hip.h and DESIGN.md 5.4 ("Tile pack: the format"): 16 x 16 tiles classified SKIP (equal to
// the reference frame), SOLID (one colour) or RAW; header, entries in ascending tile order, the solid texels, the raw blocks.
//
// Pack is count -> prefix -> write in a canonical order, two launches and no atomics:
//   k_pack_classify  a wave per tile, each lane four adjacent texels of one tile row (16 B of 4-byte texels, 32 B of 8-byte
//                    ones); SKIP and SOLID are one wave-wide vote each.  A workgroup owns a fixed run of consecutive tiles and
//                    its four waves take neighbouring tiles at the same time, so the two 64-B halves of a 128-B line are asked
//                    for together.  Leaves a class byte per tile and (n_solid, n_raw) per workgroup.
//   k_pack_write     the same runs.  Every workgroup sums the totals in front of it (at most kPackMaxGroups pairs) and all of
//                    them (the section offsets), scans its own class bytes, writes its entries and solid texels with a thread
//                    per tile and copies its RAW tiles with a wave per tile (a second read of those tiles).  Workgroup 0 also
//                    writes the header and the zero padding.
// Unpack is a wave per entry; the pack is untrusted input: the header is checked against the arguments and pack_bytes,
// every entry against the tile count and its section's count, and whatever fails is counted and ignored.
// Texels are opaque bit patterns (u32 / u64 compares).  The 16-B accesses need 16-B aligned pointers and pitches; anything
// else that is a multiple of the texel size goes texel by texel.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kcommon.h"

namespace {

constexpr uint32_t kPackMagic = 0x3150544Au;  // "JTP1"
constexpr uint32_t kPackMaxGroups = 1024u;    // workgroups per pass: what k_pack_write sums to get its prefix
constexpr uint32_t kPackMinRun = 64u;         // tiles per workgroup at least (a multiple of the 4 waves)
enum : uint32_t { PK_SKIP = 0u, PK_SOLID = 1u, PK_RAW = 2u };

struct PackArgs {
    const uint8_t* src;
    const uint8_t* ref;  // or nullptr
    uint8_t* dst;
    uint8_t* cls;        // scratch H: a class byte per tile
    uint2* totals;       // scratch J: (n_solid, n_raw) per workgroup
    uint64_t src_pitch, ref_pitch;
    uint32_t width, height, tiles_x, n_tiles;
    uint32_t run;        // tiles per workgroup
    uint32_t src_vec, ref_vec, dst_vec;  // 1: pointer and pitch are multiples of 16
};

struct UnpackArgs {
    const uint8_t* pack;
    uint8_t* dst;
    uint32_t* rejects;
    uint64_t pack_bytes, dst_pitch;
    uint32_t width, height, tiles_x, n_tiles;
    uint32_t pack_vec, dst_vec;
};

JD uint64_t pack_align16(uint64_t v) { return (v + 15ull) & ~15ull; }

template <typename T>
struct Quad {
    T v[4];
};

// four texels at p: one or two 16-B loads when `vec` (p is then 16-B aligned), else texel by texel; only the first n are read,
// the others are zero
template <typename T>
JD Quad<T> quad_load(const uint8_t* p, bool vec, uint32_t n) {
    Quad<T> q;
    if (vec && n == 4u) {
        if (sizeof(T) == 4) {
            const uint4 a = *(const uint4*)p;
            q.v[0] = (T)a.x; q.v[1] = (T)a.y; q.v[2] = (T)a.z; q.v[3] = (T)a.w;
        } else {
            const uint4 a = *(const uint4*)p, b = *(const uint4*)(p + 16);
            q.v[0] = (T)((uint64_t)a.x | ((uint64_t)a.y << 32)); q.v[1] = (T)((uint64_t)a.z | ((uint64_t)a.w << 32));
            q.v[2] = (T)((uint64_t)b.x | ((uint64_t)b.y << 32)); q.v[3] = (T)((uint64_t)b.z | ((uint64_t)b.w << 32));
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) q.v[k] = k < n ? ((const T*)p)[k] : (T)0;
    }
    return q;
}
// the first n of four texels to p
template <typename T>
JD void quad_store(uint8_t* p, bool vec, uint32_t n, const Quad<T>& q) {
    if (vec && n == 4u) {
        if (sizeof(T) == 4) {
            *(uint4*)p = make_uint4((uint32_t)q.v[0], (uint32_t)q.v[1], (uint32_t)q.v[2], (uint32_t)q.v[3]);
        } else {
            *(uint4*)p = make_uint4((uint32_t)q.v[0], (uint32_t)((uint64_t)q.v[0] >> 32), (uint32_t)q.v[1], (uint32_t)((uint64_t)q.v[1] >> 32));
            *(uint4*)(p + 16) = make_uint4((uint32_t)q.v[2], (uint32_t)((uint64_t)q.v[2] >> 32), (uint32_t)q.v[3], (uint32_t)((uint64_t)q.v[3] >> 32));
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            if (k < n) ((T*)p)[k] = q.v[k];
    }
}

// This lane's part of tile (tx, ty): texels x0 .. x0 + 3 of row y, of which the first n lie inside the frame (0: none)
struct LanePos {
    uint32_t x0, y, n;
};
JD LanePos lane_pos(uint32_t tx, uint32_t ty, uint32_t width, uint32_t height) {
    const uint32_t l = jk::lane_id();
    LanePos p;
    p.x0 = tx * 16u + (l & 3u) * 4u;
    p.y = ty * 16u + (l >> 2);
    p.n = (p.y < height && p.x0 < width) ? (width - p.x0 < 4u ? width - p.x0 : 4u) : 0u;
    return p;
}

template <typename T, bool HAS_REF>
__global__ __launch_bounds__(JL_WG) void k_pack_classify(const PackArgs a) {
    __shared__ uint32_t sh[8];
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t t0 = blockIdx.x * a.run;
    const uint32_t t1 = t0 + a.run < a.n_tiles ? t0 + a.run : a.n_tiles;
    uint32_t n_solid = 0u, n_raw = 0u;
    for (uint32_t t = t0 + wave; t < t1; t += 4u) {
        const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const LanePos p = lane_pos(tx, ty, a.width, a.height);
        const uint64_t xoff = (uint64_t)p.x0 * sizeof(T);
        const Quad<T> q = quad_load<T>(a.src + (uint64_t)p.y * a.src_pitch + xoff, a.src_vec != 0u, p.n);
        bool same_as_ref = HAS_REF;
        if (HAS_REF) {
            const Quad<T> r = quad_load<T>(a.ref + (uint64_t)p.y * a.ref_pitch + xoff, a.ref_vec != 0u, p.n);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) same_as_ref = same_as_ref && (k >= p.n || q.v[k] == r.v[k]);
        }
        const T first = jk::uni(q.v[0]);  // lane 0 holds the tile's texel (0, 0), which is always inside the frame
        bool same_as_first = true;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) same_as_first = same_as_first && (k >= p.n || q.v[k] == first);
        uint32_t c;
        if (HAS_REF && __builtin_amdgcn_ballot_w64(!same_as_ref) == 0ull) c = PK_SKIP;
        else c = __builtin_amdgcn_ballot_w64(!same_as_first) == 0ull ? PK_SOLID : PK_RAW;
        n_solid += c == PK_SOLID ? 1u : 0u;
        n_raw += c == PK_RAW ? 1u : 0u;
        if (jk::lane_id() == 0u) a.cls[t] = (uint8_t)c;
    }
    if (jk::lane_id() == 0u) { sh[wave] = n_solid; sh[4u + wave] = n_raw; }
    __syncthreads();
    if (threadIdx.x == 0u) a.totals[blockIdx.x] = make_uint2(sh[0] + sh[1] + sh[2] + sh[3], sh[4] + sh[5] + sh[6] + sh[7]);
}

template <typename T, bool HAS_REF>
__global__ __launch_bounds__(JL_WG) void k_pack_write(const PackArgs a) {
    __shared__ uint32_t sh[16];
    __shared__ uint32_t raw_tile[JL_WG];
    const uint32_t wave = threadIdx.x >> 6;
    // (solid, raw) of the workgroups in front of this one, and of all of them
    jk::MonoidK<4> m;
    m.v[0] = m.v[1] = m.v[2] = m.v[3] = 0u;
    for (uint32_t g = threadIdx.x; g < gridDim.x; g += JL_WG) {
        const uint2 s = a.totals[g];
        m.v[2] += s.x; m.v[3] += s.y;
        if (g < blockIdx.x) { m.v[0] += s.x; m.v[1] += s.y; }
    }
    m = jk::block_reduce_monoid<4>(m, sh);
    uint32_t base_solid = m.v[0], base_raw = m.v[1];
    const uint32_t n_solid = m.v[2], n_raw = m.v[3], n_entries = n_solid + n_raw;
    const uint64_t off_solid = 32ull + pack_align16(8ull * n_entries);
    const uint64_t off_raw = off_solid + pack_align16((uint64_t)sizeof(T) * n_solid);
    if (blockIdx.x == 0u && threadIdx.x == 0u) {  // header and the zero padding of the two sections that can need any
        uint32_t* d = (uint32_t*)a.dst;
        d[0] = kPackMagic; d[1] = a.width; d[2] = a.height; d[3] = (uint32_t)sizeof(T);
        d[4] = n_entries; d[5] = n_solid; d[6] = n_raw; d[7] = HAS_REF ? 1u : 0u;
        for (uint64_t w = (32ull + 8ull * n_entries) / 4u; w < off_solid / 4u; w++) d[w] = 0u;                    // 0 or 2 words
        for (uint64_t w = (off_solid + (uint64_t)sizeof(T) * n_solid) / 4u; w < off_raw / 4u; w++) d[w] = 0u;  // up to 3 words
    }
    const uint32_t t0 = blockIdx.x * a.run;
    const uint32_t t1 = t0 + a.run < a.n_tiles ? t0 + a.run : a.n_tiles;
    for (uint32_t r0 = t0; r0 < t1; r0 += JL_WG) {  // (uniform: every thread takes part in the scans and barriers)
        const uint32_t t = r0 + threadIdx.x;
        const uint32_t c = t < t1 ? (uint32_t)a.cls[t] : PK_SKIP;
        jk::MonoidK<2> in, tot;
        in.v[0] = c == PK_SOLID ? 1u : 0u;
        in.v[1] = c == PK_RAW ? 1u : 0u;
        const jk::MonoidK<2> ex = jk::block_excl_scan_monoid<2>(in, sh, &tot);
        if (c != PK_SKIP) {
            const uint32_t e = base_solid + base_raw + ex.v[0] + ex.v[1];
            uint32_t* d = (uint32_t*)(a.dst + 32ull + 8ull * e);
            if (c == PK_SOLID) {
                const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
                d[0] = t;
                d[1] = base_solid + ex.v[0];
                *(T*)(a.dst + off_solid + (uint64_t)sizeof(T) * (base_solid + ex.v[0])) =
                    *(const T*)(a.src + (uint64_t)ty * 16u * a.src_pitch + (uint64_t)tx * 16u * sizeof(T));
            } else {
                d[0] = t | 0x80000000u;
                d[1] = base_raw + ex.v[1];
                raw_tile[ex.v[1]] = t;
            }
        }
        __syncthreads();
        for (uint32_t j = wave; j < tot.v[1]; j += 4u) {
            const uint32_t rt = raw_tile[j];
            const uint32_t ty = rt / a.tiles_x, tx = rt - ty * a.tiles_x;
            const LanePos p = lane_pos(tx, ty, a.width, a.height);
            const Quad<T> q = quad_load<T>(a.src + (uint64_t)p.y * a.src_pitch + (uint64_t)p.x0 * sizeof(T), a.src_vec != 0u, p.n);
            // texels outside the frame were loaded as zero; a block is 256 texels, this lane's four are texels 4 * lane ..
            quad_store<T>(a.dst + off_raw + (uint64_t)(base_raw + j) * (256u * sizeof(T)) + (uint64_t)jk::lane_id() * (4u * sizeof(T)),
                          a.dst_vec != 0u, 4u, q);
        }
        base_solid += tot.v[0];
        base_raw += tot.v[1];
        __syncthreads();  // raw_tile and sh are reused by the next round
    }
}

template <typename T>
__global__ __launch_bounds__(JL_WG) void k_unpack(const UnpackArgs a) {
    const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6);  // this wave's entry
    const uint32_t* h = (const uint32_t*)a.pack;              // pack_bytes >= 32 (the launcher's check)
    const uint32_t n_entries = h[4], n_solid = h[5], n_raw = h[6];
    const uint64_t off_solid = 32ull + pack_align16(8ull * n_entries);
    const uint64_t off_raw = off_solid + pack_align16((uint64_t)sizeof(T) * n_solid);
    const uint64_t total = off_raw + (uint64_t)n_raw * (256u * sizeof(T));  // (< 2^45: no overflow)
    const bool header_ok = h[0] == kPackMagic && h[1] == a.width && h[2] == a.height && h[3] == (uint32_t)sizeof(T) &&
                           (uint64_t)n_solid + n_raw == n_entries && n_entries <= a.n_tiles && total <= a.pack_bytes;
    if (!header_ok) {  // the whole pack is ignored: one reject
        if (blockIdx.x == 0u && threadIdx.x == 0u) atomicAdd(a.rejects, 1u);
        return;
    }
    if (e >= n_entries) return;
    const uint2 en = make_uint2(h[8u + 2u * e], h[9u + 2u * e]);  // inside the pack: e < n_entries and total <= pack_bytes
    const bool raw = (en.x >> 31) != 0u;
    const uint32_t t = en.x & 0x7fffffffu;
    if (t >= a.n_tiles || en.y >= (raw ? n_raw : n_solid)) {
        if (jk::lane_id() == 0u) atomicAdd(a.rejects, 1u);
        return;
    }
    const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const LanePos p = lane_pos(tx, ty, a.width, a.height);
    Quad<T> q;
    if (raw) {
        q = quad_load<T>(a.pack + off_raw + (uint64_t)en.y * (256u * sizeof(T)) + (uint64_t)jk::lane_id() * (4u * sizeof(T)), a.pack_vec != 0u, 4u);
    } else {
        const T s = *(const T*)(a.pack + off_solid + (uint64_t)sizeof(T) * en.y);
        q.v[0] = q.v[1] = q.v[2] = q.v[3] = s;
    }
    if (p.n) quad_store<T>(a.dst + (uint64_t)p.y * a.dst_pitch + (uint64_t)p.x0 * sizeof(T), a.dst_vec != 0u, p.n, q);
}

bool aligned16(const void* p, uint64_t pitch) { return (((uintptr_t)p | pitch) & 15u) == 0u; }

}  // namespace

// Enqueues the two kernels of a pack.  The caller (jh_pack_tiles) has checked the arguments; `cls` holds n_tiles bytes and
// `totals` jh_pack_groups(n_tiles) pairs of u32.  Returns 0, -2 on a launch error.
extern "C" uint32_t jh_pack_groups(uint32_t n_tiles, uint32_t* run_out) {
    uint32_t run = (n_tiles + kPackMaxGroups - 1u) / kPackMaxGroups;
    run = run < kPackMinRun ? kPackMinRun : (run + 3u) & ~3u;
    if (run_out) *run_out = run;
    return (n_tiles + run - 1u) / run;
}

extern "C" int jh_pack_launch(hipStream_t stream, const void* src, uint64_t src_pitch, const void* ref, uint64_t ref_pitch, uint32_t width,
                              uint32_t height, uint32_t texel_bytes, void* dst, void* cls, void* totals) {
    PackArgs a;
    a.src = (const uint8_t*)src; a.ref = (const uint8_t*)ref; a.dst = (uint8_t*)dst;
    a.cls = (uint8_t*)cls; a.totals = (uint2*)totals;
    a.src_pitch = src_pitch; a.ref_pitch = ref_pitch;
    a.width = width; a.height = height;
    a.tiles_x = (width + 15u) / 16u;
    a.n_tiles = a.tiles_x * ((height + 15u) / 16u);
    const uint32_t groups = jh_pack_groups(a.n_tiles, &a.run);
    a.src_vec = aligned16(src, src_pitch) ? 1u : 0u;
    a.ref_vec = ref && aligned16(ref, ref_pitch) ? 1u : 0u;
    a.dst_vec = aligned16(dst, 0) ? 1u : 0u;
    const dim3 grid(groups), block(JL_WG);
    if (texel_bytes == 4u) {
        if (ref) {
            hipLaunchKernelGGL((k_pack_classify<uint32_t, true>), grid, block, 0, stream, a);
            hipLaunchKernelGGL((k_pack_write<uint32_t, true>), grid, block, 0, stream, a);
        } else {
            hipLaunchKernelGGL((k_pack_classify<uint32_t, false>), grid, block, 0, stream, a);
            hipLaunchKernelGGL((k_pack_write<uint32_t, false>), grid, block, 0, stream, a);
        }
    } else {
        if (ref) {
            hipLaunchKernelGGL((k_pack_classify<uint64_t, true>), grid, block, 0, stream, a);
            hipLaunchKernelGGL((k_pack_write<uint64_t, true>), grid, block, 0, stream, a);
        } else {
            hipLaunchKernelGGL((k_pack_classify<uint64_t, false>), grid, block, 0, stream, a);
            hipLaunchKernelGGL((k_pack_write<uint64_t, false>), grid, block, 0, stream, a);
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// One kernel, a wave per possible entry (the entry count is on the device: the grid comes from the tile count).
extern "C" int jh_unpack_launch(hipStream_t stream, const void* pack, uint64_t pack_bytes, void* dst, uint64_t dst_pitch, uint32_t width,
                                uint32_t height, uint32_t texel_bytes, uint32_t* rejects) {
    UnpackArgs a;
    a.pack = (const uint8_t*)pack; a.dst = (uint8_t*)dst; a.rejects = rejects;
    a.pack_bytes = pack_bytes; a.dst_pitch = dst_pitch;
    a.width = width; a.height = height;
    a.tiles_x = (width + 15u) / 16u;
    a.n_tiles = a.tiles_x * ((height + 15u) / 16u);
    a.pack_vec = aligned16(pack, 0) ? 1u : 0u;
    a.dst_vec = aligned16(dst, dst_pitch) ? 1u : 0u;
    const dim3 grid((a.n_tiles + 3u) / 4u), block(JL_WG);
    if (texel_bytes == 4u) hipLaunchKernelGGL((k_unpack<uint32_t>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_unpack<uint64_t>), grid, block, 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
