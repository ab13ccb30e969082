// kernels_displace.hip -- jh_displace: feDisplacementMap, a rectangle of one RGBA16F image into a rectangle of another at positions
// that a third image, the map, moves texel by texel; the device half of the rule in include/jello_hip.h ("Displace") and DESIGN.md
// 5.17.  The host half -- what is legal and the offset one map value gives -- is include/jello_displace.h, compiled here too; the plan
// is jh_warp's (include/jello_warp.h).  The kernel, its arguments and its launch are the warp family's (warp_taps.h); this file's own
// is the position of destination texel (X, Y) of the image
//   m = the map's texel (X, Y): the stored f16 of the x channel and of the y channel
//   U = P (2 X + 1) + Q (2 Y + 1) + R + jdisp_offset(scale_x, m_x),  V = S (2 X + 1) + T (2 Y + 1) + W + jdisp_offset(scale_y, m_y)
// The map has the destination's size, so a lane's map texel sits where its destination texel does: one coalesced 8-byte load per
// lane, a 128-byte line per tile row, issued before the plan's part of the position, which does not depend on it.  The channels are
// run-time scalars -- the 64-bit texel shifted by 16 x channel -- so the rule adds no instantiation.  The map may be the destination:
// a lane reads its one map texel before it writes that texel, and no other lane touches it (the map pointer is not __restrict__, so
// the store stays behind the load).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_displace.h"
#include "kcommon.h"
#include "warp_taps.h"

namespace {

struct MapPosition {
    const uint2* map;  // the map image, of the destination's size; may be the destination, and is where there is no map
    int64_t plan[6];   // P, Q, R, S, T, W
    float scale_x, scale_y;
    uint32_t shift_x, shift_y;  // 16 x the channel: where its f16 sits in the 64-bit texel
    uint32_t has_map;           // 0: the map was never written, 0 in every channel
    JD bool operator()(uint32_t X, uint32_t Y, uint64_t at, int64_t* U, int64_t* V) const {
        // (unconditional, so that it is in flight under the plan's part of the position: without a map the lane's own destination
        // texel is loaded and replaced by 0)
        uint2 m = map[at];
        if (!has_map) m = make_uint2(0u, 0u);
        const int64_t U0 = jwarp_position(plan[0], plan[1], plan[2], X, Y), V0 = jwarp_position(plan[3], plan[4], plan[5], X, Y);
        const uint64_t texel = (uint64_t)m.x | ((uint64_t)m.y << 32);
        *U = U0 + jdisp_offset(scale_x, (uint16_t)(texel >> shift_x));
        *V = V0 + jdisp_offset(scale_y, (uint16_t)(texel >> shift_y));
        return true;
    }
};

}  // namespace

// The rectangle d of the RGBA16F image dst = the rectangle s of the image src (null texels: transparent black; another image than
// dst) under the plan (P, Q, R, S, T, W of include/jello_warp.h, host memory, read during the call), every position moved by the
// x_channel and y_channel of the image map (null texels: 0; of dst's size; may be dst or src) times scale_x and scale_y
// (include/jello_displace.h).  One launch on `stream`: one of the 24 instantiations of k_warp<MapPosition>, filter x edge x straight.
// Returns 0, -1 on arguments it refuses (a plan outside a legal one's range among them: the kernel's indices are 32-bit), -2 on a
// launch error.
extern "C" int jh_displace_launch(hipStream_t stream, jimage_src src, jimage_rect s, jimage_src map, jimage_dst dst, jimage_rect d, const int64_t* plan,
                                  float scale_x, float scale_y, int x_channel, int y_channel, int filter, int edge, int straight, int num_cus) {
    TileArgs a;
    if (!plan || !tile_args(src, s, dst, d, &a)) return -1;
    if (jdisp_desc_error(filter, edge, 0u, scale_x, scale_y, x_channel, y_channel, src.width, src.height, map.width, map.height, dst.width, dst.height)) return -1;
    if (!jwarp_plan_in_range(plan)) return -1;
    MapPosition pos;
    pos.map = (const uint2*)(map.texels ? map.texels : dst.texels);
    for (int i = 0; i < 6; i++) pos.plan[i] = plan[i];
    pos.scale_x = scale_x; pos.scale_y = scale_y;
    pos.shift_x = 16u * (uint32_t)x_channel; pos.shift_y = 16u * (uint32_t)y_channel;
    pos.has_map = map.texels != nullptr;
    return tile_launch(stream, a, pos, filter, edge, straight, num_cus);
}
