// kernels_perspective.hip -- jh_perspective: a rectangle of one RGBA16F image into a rectangle of another under a projective
// transform; the device half of the rule in include/jello_hip.h ("Perspective") and DESIGN.md 5.19.  The plan (nine doubles, host
// only) and the source position are include/jello_perspective.h's, compiled here too.  The kernel, its arguments and its launch are
// the warp family's (warp_taps.h); this file's own is the position of destination texel (X, Y) of the image
//   (U, V) = jpersp_position(G, X, Y), or the texel is void: den <= 0 (behind the viewer, or on the horizon) or a NaN position
// The nine doubles travel in the kernel arguments (scalar registers); the position is 14 binary64 products and sums and one IEEE
// division per texel, on the vector unit at the binary64 rate.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/jello_perspective.h"
#include "kcommon.h"
#include "warp_taps.h"

namespace {

struct ProjectivePosition {
    double G[9];  // the plan
    JD bool operator()(uint32_t X, uint32_t Y, uint64_t, int64_t* U, int64_t* V) const { return jpersp_position(G, X, Y, U, V); }
};

}  // namespace

// The rectangle d of the RGBA16F image dst = the rectangle s of the image src (null texels: transparent black; another image than
// dst) under the plan (G[9] of include/jello_perspective.h, host memory, read during the call).  One launch on `stream`: one of the
// 24 instantiations of k_warp<ProjectivePosition>, filter x edge x straight.  Returns 0, -1 on arguments it refuses (a plan outside a
// legal one's range among them: an entry that is not finite or above 1 in magnitude), -2 on a launch error.
extern "C" int jh_perspective_launch(hipStream_t stream, jimage_src src, jimage_rect s, jimage_dst dst, jimage_rect d, const double* plan, int filter, int edge,
                                     int straight, int num_cus) {
    TileArgs a;
    if (!plan || !tile_args(src, s, dst, d, &a)) return -1;
    if (jpersp_desc_error(filter, edge, 0u, src.width, src.height, dst.width, dst.height)) return -1;
    ProjectivePosition pos;
    for (int i = 0; i < 9; i++) {
        if (!(plan[i] >= -1.0 && plan[i] <= 1.0)) return -1;
        pos.G[i] = plan[i];
    }
    return tile_launch(stream, a, pos, filter, edge, straight, num_cus);
}
