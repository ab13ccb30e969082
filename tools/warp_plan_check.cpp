// warp_plan_check.cpp -- include/jello_warp.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/warp_plan_check.cpp -o /tmp/warp_plan_check && /tmp/warp_plan_check
//
// Four things.  (1) Legal and illegal matrices: each condition of the rule from both sides, the reason named; every plan jwarp_plan
// makes is inside jwarp_plan_in_range, a plan one unit beyond either limit is not.  (2) The plan against
// __int128 arithmetic: every coefficient is the binary64 inverse coefficient times 2^31 (offsets: 2^32) rounded half to even, worked
// on the double's own integer mantissa; the positions U, V of the corner texels of a 32768 x 32768 destination in __int128 equal the
// int64 ones and stay below 2^58.  (3) The four index rules against a brute-force definition (a walk, no division) for n = 1 .. 5
// and i in [-40, 40], and the fraction and the taps' first index against __int128.  (4) The bounds rectangle against the plan on
// small images: every destination texel that has a tap inside the source rectangle on both axes lies inside the rectangle
// (exactly sized arrays: a read or write past an end is an AddressSanitizer report).  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jello_warp.h"

typedef __int128 i128;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}
static double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

// v 2^shift rounded half to even, on the double's integer mantissa
static i128 scaled_rint(double v, int shift) {
    if (v == 0.0) return 0;
    int e;
    const double m = frexp(fabs(v), &e);          // |v| = m 2^e, 0.5 <= m < 1
    i128 q = (i128)(int64_t)ldexp(m, 53);         // |v| = q 2^(e - 53), exactly
    const int s = e - 53 + shift;
    if (s >= 0) q <<= s;
    else if (-s >= 120) q = 0;
    else {
        const i128 one = (i128)1 << -s, rem = q & (one - 1), half = one >> 1;
        q >>= -s;
        if (rem > half || (rem == half && (q & 1))) q += 1;
    }
    return v < 0.0 ? -q : q;
}

static int check_matrices() {
    const double inf = INFINITY, nan = NAN;
    const double legal[][6] = {{1, 0, 0, 1, 0, 0}, {0, 1, -1, 0, 5, 0}, {1.0 / 64, 0, 0, 1.0 / 64, 0, 0}, {1, 0, 0, 1, 4194304.0, -4194304.0},
                               {1e6, 0, 0, 1e6, 1e9, -1e9}, {0.866, 0.5, -0.5, 0.866, -3.25, 7.5}, {1, 0, 64, 1, 0, 0}};
    const struct { double m[6]; const char* word; } illegal[] = {
        {{nan, 0, 0, 1, 0, 0}, "not finite"}, {{1, 0, 0, 1, inf, 0}, "not finite"}, {{1, 0, 0, 1, 0, -inf}, "not finite"},
        {{0, 0, 0, 0, 0, 0}, "determinant is 0"}, {{1, 2, 2, 4, 0, 0}, "determinant is 0"}, {{1e200, 0, 0, 1e200, 0, 0}, "determinant is not finite"},
        {{1.0 / 65, 0, 0, 1, 0, 0}, "above 64"}, {{1, 0, 0, 0.015, 0, 0}, "above 64"}, {{1, 0, 64.5, 1, 0, 0}, "above 64"}, {{1, -65, 0, 1, 0, 0}, "above 64"},
        {{1, 0, 0, 1, 4194305.0, 0}, "above 2^22"}, {{1, 0, 0, 1, 0, -4194304.5}, "above 2^22"}, {{1e-300, 0, 0, 1e-300, 0, 0}, "determinant is 0"}};
    int64_t plan[6];
    for (const auto& m : legal)
        if (jwarp_plan(m, plan) || !jwarp_plan_in_range(plan)) return 1;
    for (const auto& c : illegal) {
        plan[0] = 77;
        const char* why = jwarp_plan(c.m, plan);
        if (!why || !strstr(why, c.word) || plan[0] != 77) return 2;
    }
    const double id[6] = {1, 0, 0, 1, 0, 0};
    if (jwarp_plan(id, plan) || plan[0] != ((int64_t)1 << 31) || plan[1] != 0 || plan[2] != 0 || plan[3] != 0 || plan[4] != ((int64_t)1 << 31) || plan[5] != 0) return 3;
    // the range a launcher asks of a plan: the legal matrices at each limit are inside it (2^37 = 64 x 2^31, 2^54 = 2^22 x 2^32), a
    // coefficient one unit beyond its limit is not
    const double at_scale[6] = {1.0 / 64, 0, 0, -1.0 / 64, 0, 0}, at_offset[6] = {1, 0, 0, 1, 4194304.0, -4194304.0};
    if (jwarp_plan(at_scale, plan) || plan[0] != ((int64_t)1 << 37) || plan[4] != -((int64_t)1 << 37) || !jwarp_plan_in_range(plan)) return 4;
    if (jwarp_plan(at_offset, plan) || plan[2] != -((int64_t)1 << 54) || plan[5] != ((int64_t)1 << 54) || !jwarp_plan_in_range(plan)) return 5;
    for (int i = 0; i < 6; i++)
        for (int64_t sign : {1, -1}) {
            int64_t edge[6] = {0, 0, 0, 0, 0, 0};
            edge[i] = sign * ((int64_t)1 << (i % 3 == 2 ? 54 : 37));
            if (!jwarp_plan_in_range(edge)) return 6;
            edge[i] += sign;
            if (jwarp_plan_in_range(edge)) return 7;
        }
    return 0;
}

static int check_plans(unsigned* count) {
    const i128 lim = (i128)1 << 58;
    unsigned n = 0;
    for (int it = 0; it < 20000; it++) {
        double m[6];
        const double k = exp(uniform(-4.0, 8.0)), t = uniform(-3.2, 3.2), sh = uniform(-1.0, 1.0);
        m[0] = k * cos(t); m[1] = k * sin(t); m[2] = k * (sh * cos(t) - sin(t)); m[3] = k * (sh * sin(t) + cos(t));
        m[4] = uniform(-40000.0, 40000.0); m[5] = uniform(-40000.0, 40000.0);
        double inv[6];
        int64_t plan[6];
        const char* why = jwarp_inverse(m, inv);
        if ((why != nullptr) != (jwarp_plan(m, plan) != nullptr)) return 1;
        if (why) continue;
        if (!jwarp_plan_in_range(plan)) return 7;
        n++;
        for (int i = 0; i < 6; i++)
            if ((i128)plan[i] != scaled_rint(inv[i], i % 3 == 2 ? 32 : 31)) return 2;
        const uint32_t corner[2] = {0u, JWARP_MAX_SIDE - 1u};
        for (int row = 0; row < 2; row++)
            for (uint32_t X : corner)
                for (uint32_t Y : corner) {
                    const int64_t* p = plan + 3 * row;
                    const i128 U = (i128)p[0] * (2 * (i128)X + 1) + (i128)p[1] * (2 * (i128)Y + 1) + (i128)p[2];
                    if (U >= lim || U <= -lim || (i128)jwarp_position(p[0], p[1], p[2], X, Y) != U) return 3;
                    // the taps: floors of U / 2^32 and of (U - 2^31) / 2^32, the fraction's 16 bits
                    const i128 two32 = (i128)1 << 32;
                    i128 fl = U / two32;
                    if (U % two32 < 0) fl -= 1;
                    if ((i128)jwarp_nearest((int64_t)U) != fl) return 4;
                    const i128 u = U - ((i128)1 << 31);
                    i128 i0 = u / two32, rem = u % two32;
                    if (rem < 0) { i0 -= 1; rem += two32; }
                    float f;
                    if ((i128)jwarp_split((int64_t)U, &f) != i0 || f != (float)(uint32_t)(rem >> 16) / 65536.0f || !(f >= 0.0f && f < 1.0f)) return 5;
                }
    }
    *count = n;
    return n > 5000u ? 0 : 6;
}

static int check_weights() {
    for (uint32_t k = 0; k < 65536u; k++) {
        const float f = (float)k / 65536.0f;
        float w[4];
        jwarp_cubic_weights(f, w);
        const double x = f, e[4] = {((-0.5 * x + 1.0) * x - 0.5) * x, (1.5 * x - 2.5) * x * x + 1.0, ((-1.5 * x + 2.0) * x + 0.5) * x, (0.5 * x - 0.5) * x * x};
        for (int i = 0; i < 4; i++)
            if (fabs((double)w[i] - e[i]) > 5e-7) return 1;
        if (fabs((double)w[0] + w[1] + w[2] + w[3] - 1.0) > 1.5e-6) return 2;
    }
    float w[4];
    jwarp_cubic_weights(0.0f, w);
    return (w[0] == 0.0f && w[1] == 1.0f && w[2] == 0.0f && w[3] == 0.0f) ? 0 : 3;
}

// The index rules by walking: no division, no modulo.
static int32_t brute_index(int edge, int32_t i, int32_t n) {
    if (edge == JWARP_EDGE_ZERO) return (i >= 0 && i < n) ? i : -1;
    if (edge == JWARP_EDGE_CLAMP) { while (i < 0) i++; while (i > n - 1) i--; return i; }
    if (edge == JWARP_EDGE_REPEAT) { while (i < 0) i += n; while (i >= n) i -= n; return i; }
    // MIRROR: the rectangle reflected about each of its edges, ... 1 0 | 0 1 .. n-1 | n-1 .. 1 0 | 0 1 ...: index -1 - i is the
    // reflection of i about the left edge; from 0 walk right, turning round at an end after repeating it
    if (i < 0) i = -1 - i;
    int32_t pos = 0, dir = 1;
    for (int32_t s = 0; s < i; s++) {
        if (pos + dir > n - 1 || pos + dir < 0) dir = -dir; else pos += dir;
    }
    return pos;
}

static int check_indices(unsigned* count) {
    unsigned c = 0;
    for (int edge = 0; edge < JWARP_EDGES; edge++)
        for (int32_t n = 1; n <= 5; n++) {
            std::vector<int> texel((size_t)n, 0);
            for (int32_t i = -40; i <= 40; i++, c++) {
                const int32_t got = jwarp_index(edge, i, n);
                if (got != brute_index(edge, i, n)) return 1 + edge;
                if (got >= 0) texel[(size_t)got]++;  // (inside [0, n), or ASan says so)
                else if (edge != JWARP_EDGE_ZERO) return 10;
            }
        }
    *count = c;
    return 0;
}

static int check_bounds(unsigned* count) {
    const double ms[][6] = {{1, 0, 0, 1, 0, 0}, {1, 0, 0, 1, 3.5, -2.25}, {0.866025, 0.5, -0.5, 0.866025, 4.0, 1.0}, {2, 0, 0, 2, -3, -3}, {0.5, 0, 0, 0.5, 2, 2},
                            {0, 1, -1, 0, 9, 0}, {1, 0.3, 0.5, 1, -2, 1}, {3.7, 0, 0, 3.7, 0.1, 0.2}, {1, 0, 0, 1, 100, 100}, {-1.3, 0.2, 0.4, 1.1, 12, 3},
                            {1.0 / 64, 0, 0, 1.0 / 64, 5, 5}};
    const uint32_t sizes[][4] = {{9, 7, 16, 12}, {1, 1, 5, 5}, {3, 11, 20, 9}, {20, 20, 1, 1}, {5, 2, 31, 17}};
    unsigned inside = 0;
    for (const auto& m : ms)
        for (const auto& sz : sizes)
            for (int filter = 0; filter < JWARP_FILTERS; filter++) {
                const uint32_t sw = sz[0], sh = sz[1], dw = sz[2], dh = sz[3];
                uint32_t r[4];
                int64_t plan[6];
                if (jwarp_bounds(m, sw, sh, filter, dw, dh, r) || jwarp_plan(m, plan)) return 1;
                if ((uint64_t)r[0] + r[2] > dw || (uint64_t)r[1] + r[3] > dh || ((r[2] == 0u) != (r[3] == 0u))) return 2;
                if (r[2] == 0u && (r[0] | r[1] | r[3]) != 0u) return 3;
                std::vector<uint8_t> covered((size_t)dw * dh, 0);
                for (uint32_t y = r[1]; y < r[1] + r[3]; y++)
                    for (uint32_t x = r[0]; x < r[0] + r[2]; x++) covered[(size_t)y * dw + x] = 1;
                const int n_taps = filter == JWARP_NEAREST ? 1 : (filter == JWARP_BILINEAR ? 2 : 4);
                for (uint32_t Y = 0; Y < dh; Y++)
                    for (uint32_t X = 0; X < dw; X++) {
                        bool live[2] = {false, false};
                        for (int axis = 0; axis < 2; axis++) {
                            const int64_t U = jwarp_position(plan[3 * axis], plan[3 * axis + 1], plan[3 * axis + 2], X, Y);
                            float f;
                            const int32_t first = filter == JWARP_NEAREST ? jwarp_nearest(U) : jwarp_split(U, &f) - (filter == JWARP_BICUBIC ? 1 : 0);
                            for (int k = 0; k < n_taps; k++)
                                if (jwarp_index(JWARP_EDGE_ZERO, first + k, (int32_t)(axis ? sh : sw)) >= 0) live[axis] = true;
                        }
                        if (live[0] && live[1]) {
                            inside++;
                            if (!covered[(size_t)Y * dw + X]) return 4;
                        }
                    }
            }
    *count = inside;
    return inside > 1000u ? 0 : 5;
}

int main() {
    unsigned plans = 0, indices = 0, texels = 0;
    if (int rc = check_matrices()) { printf("FAILED: matrices (%d)\n", rc); return 1; }
    if (int rc = check_plans(&plans)) { printf("FAILED: plans (%d)\n", rc); return 1; }
    if (int rc = check_weights()) { printf("FAILED: cubic weights (%d)\n", rc); return 1; }
    if (int rc = check_indices(&indices)) { printf("FAILED: index rules (%d)\n", rc); return 1; }
    if (int rc = check_bounds(&texels)) { printf("FAILED: bounds (%d)\n", rc); return 1; }
    printf("ok: %u plans, %u indices, %u texels inside their bounds\n", plans, indices, texels);
    return 0;
}
