// composite_clip_check.cpp -- include/jello_composite.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/composite_clip_check.cpp -o /tmp/composite_clip_check && /tmp/composite_clip_check
//
// Runs jcomp_clip over the corner values of every argument -- int32 offsets at INT32_MIN / INT32_MAX and around the sizes, uint32
// sizes 0, 1, 2 and 0xffffffff, every source rectangle those allow -- so that a sum that wraps or overflows is an
// UndefinedBehaviorSanitizer report, and checks each result against the same clip in 128-bit integers and against what the kernel
// relies on: the rectangle lies inside both images.  Prints "ok" and returns 0.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "jello_composite.h"

typedef __int128 wide;

static int check_axis(uint32_t src, uint32_t s, uint32_t n, int32_t d, uint32_t dst) {
    uint32_t so = 7u, dor = 7u;
    const uint32_t got = jcomp_clip_axis(s, n, d, dst, &so, &dor);
    const wide lo = d < 0 ? (wide)0 : (wide)d, end = (wide)d + n, hi = end < (wide)dst ? end : (wide)dst;
    if (hi <= lo) return (got == 0u && so == 0u && dor == 0u) ? 0 : 1;
    if ((wide)got != hi - lo || (wide)dor != lo || (wide)so != (wide)s + (lo - d)) return 2;
    if ((wide)so + got > src || (wide)dor + got > dst || got == 0u) return 3;  // inside both
    return 0;
}

int main() {
    const uint32_t sizes[] = {0u, 1u, 2u, 3u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    long n = 0;
    for (uint32_t src : sizes)
        for (uint32_t dst : sizes)
            for (uint32_t len : sizes) {
                if (len == 0u || len > src) continue;
                const uint32_t starts[] = {0u, 1u, (src - len) / 2u, src - len};
                for (uint32_t s : starts) {
                    if ((uint64_t)s + len > src) continue;
                    std::vector<int64_t> offs = {INT32_MIN, INT32_MIN + 1, -(int64_t)len - 1, -(int64_t)len, -(int64_t)len + 1, -1, 0, 1,
                                                 (int64_t)dst - 1, (int64_t)dst, (int64_t)dst + 1, INT32_MAX - 1, INT32_MAX};
                    for (int64_t d : offs) {
                        if (d < INT32_MIN || d > INT32_MAX) continue;
                        if (int rc = check_axis(src, s, len, (int32_t)d, dst)) {
                            printf("axis src %u s %u n %u d %lld dst %u: check %d failed\n", src, s, len, (long long)d, dst, rc);
                            return 1;
                        }
                        // the same numbers through the whole function, on x with a trivial y and the other way round
                        jcomp_rect r;
                        if (jcomp_clip(src, 2u, s, 1u, len, 1u, (int32_t)d, 0, dst, 1u, &r) != 0 || jcomp_clip(2u, src, 1u, s, 1u, len, 0, (int32_t)d, 1u, dst, &r) != 0) {
                            printf("a legal rectangle was refused\n");
                            return 1;
                        }
                        if ((r.w == 0u) != (r.h == 0u) || (uint64_t)r.sy + r.h > src || (uint64_t)r.dy + r.h > dst) { printf("clip result outside\n"); return 1; }
                        n++;
                    }
                }
            }
    // the whole image, an image without texels, and what is refused
    jcomp_rect r = {9u, 9u, 9u, 9u, 9u, 9u};
    if (jcomp_clip(5u, 4u, 3u, 3u, 0u, 0u, -2, 1, 4u, 4u, &r) != 0 || r.sx != 2u || r.sy != 0u || r.dx != 0u || r.dy != 1u || r.w != 3u || r.h != 3u) return 2;
    if (jcomp_clip(0u, 0u, 0u, 0u, 0u, 0u, 0, 0, 4u, 4u, &r) != 0 || r.w != 0u || r.h != 0u) return 2;
    const uint32_t bad[][4] = {{0u, 0u, 0u, 2u}, {0u, 0u, 2u, 0u}, {4u, 0u, 2u, 1u}, {0u, 3u, 1u, 2u}, {0xffffffffu, 0u, 2u, 1u}, {0u, 0xffffffffu, 1u, 2u},
                               {1u, 0u, 0xffffffffu, 1u}, {5u, 4u, 1u, 1u}};
    for (const auto& b : bad)
        if (jcomp_clip(5u, 4u, b[0], b[1], b[2], b[3], 0, 0, 8u, 8u, &r) != -1) { printf("accepted a bad rectangle\n"); return 1; }
    printf("ok: %ld placements\n", n);
    return 0;
}
