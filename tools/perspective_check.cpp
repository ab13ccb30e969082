// perspective_check.cpp -- include/jello_perspective.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/perspective_check.cpp -o /tmp/perspective_check && /tmp/perspective_check
//
// Four things.  (1) The plan where it is exact: matrices of small integers, the adjugate and the determinant worked in __int128, G
// against sign(det) adj 2^-k with 2^(k-1) < max |adj| <= 2^k decided on the integers; matrices whose inverse is dyadic; every |G| <= 1
// and one above 1/2; den > 0 <=> the forward w of the source position > 0, on the integers.  (2) Legality from both sides: entries,
// adjugate entries and the determinant at the edge of binary64, a determinant of 0 and next to 0, image sides of 32768 and 32769.
// (3) The bounds by brute force on small images: every texel outside the rectangle is void or has all its taps of one axis outside the
// source rectangle, for three filters, a matrix that crosses w = 0 among them (the whole destination).  (4) The position's special
// routes: den = 0, q = Inf with n_u = 0 (void) and n_u != 0 (the clamp), the clamp from both sides, rint half to even.
// Prints "ok" and returns 0.
//
// With arguments -- the nine entries of a matrix, then x y width height of a destination rectangle -- it prints the rectangle's
// positions instead, a line per texel: "U V" in decimal, or "void" (tests/test_perspective_spec.py compares them with the reference).
#include <initializer_list>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jello_perspective.h"

typedef __int128 i128;

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            return 1;                                                \
        }                                                            \
    } while (0)

static bool is(const char* got, const char* want) { return got && strstr(got, want); }

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static int64_t small(int64_t range) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (int64_t)((g_state >> 33) % (uint64_t)(2 * range + 1)) - range;
}

static int check_plan() {
    for (int n = 0; n < 20000; n++) {
        const int64_t range = n % 3 == 0 ? 3 : (n % 3 == 1 ? 1000 : 1000000);
        int64_t m[9];
        double md[9];
        for (int i = 0; i < 9; i++) { m[i] = small(range); md[i] = (double)m[i]; }
        const int64_t a = m[0], b = m[1], p = m[2], c = m[3], d = m[4], q = m[5], e = m[6], f = m[7], s = m[8];
        const int64_t adj[9] = {d * s - f * q, e * q - c * s, c * f - e * d, f * p - b * s, a * s - e * p, e * b - a * f, b * q - d * p, c * p - a * q, a * d - c * b};
        const i128 det = (i128)a * adj[0] + (i128)c * adj[3] + (i128)e * adj[6];
        double G[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
        const char* why = jpersp_plan(md, G);
        if (det == 0) {
            CHECK(is(why, "determinant is 0") && G[0] == 7.0 && G[8] == 7.0);
            continue;
        }
        CHECK(!why);
        int64_t top = 0;
        for (int i = 0; i < 9; i++) top = llabs(adj[i]) > top ? llabs(adj[i]) : top;
        int k = 0;
        while (((int64_t)1 << k) < top) k++;  // 2^(k-1) < top <= 2^k (top >= 1)
        bool above_half = false;
        for (int i = 0; i < 9; i++) {
            const double want = ldexp((double)adj[i], -k) * (det < 0 ? -1.0 : 1.0);  // (|adj| < 2^42: exact)
            CHECK(G[i] == want && fabs(G[i]) <= 1.0);
            above_half = above_half || fabs(G[i]) > 0.5;
        }
        CHECK(above_half);
        // den > 0 <=> forward w > 0: the source position of the destination point (X + 1/2, Y + 1/2) is (nu, nv) / den with integer nu,
        // nv, den' = 2 adj (2X + 1, 2Y + 1, 2)^T; its forward w is (p nu + q nv + s den') / den' = 2 det / den' (M adj = det I)
        for (int64_t X = 0; X < 3; X++)
            for (int64_t Y = 0; Y < 3; Y++) {
                const i128 den2 = (i128)adj[6] * (2 * X + 1) + (i128)adj[7] * (2 * Y + 1) + (i128)adj[8] * 2;
                const i128 nu2 = (i128)adj[0] * (2 * X + 1) + (i128)adj[1] * (2 * Y + 1) + (i128)adj[2] * 2;
                const i128 nv2 = (i128)adj[3] * (2 * X + 1) + (i128)adj[4] * (2 * Y + 1) + (i128)adj[5] * 2;
                CHECK((i128)p * nu2 + (i128)q * nv2 + (i128)s * den2 == 2 * det);  // w den' = 2 det
                int64_t U = 0, V = 0;
                const bool front = jpersp_position(G, (uint32_t)X, (uint32_t)Y, &U, &V);
                const bool w_positive = den2 != 0 && ((den2 > 0) == (det > 0));
                CHECK(front == w_positive);  // (|adj| < 2^42 and x' < 4: every product and sum of den is exact)
            }
    }
    // dyadic inverses stay exact: a translation by (3.5, -2.25), a scale by 4, a quarter turn
    const double t[9] = {1, 0, 0, 0, 1, 0, 3.5, -2.25, 1}, sc[9] = {4, 0, 0, 0, 4, 0, 0, 0, 1}, qt[9] = {0, 1, 0, -1, 0, 0, 8, 0, 1};
    double G[9];
    CHECK(!jpersp_plan(t, G) && G[0] == 0.25 && G[2] == -0.875 && G[4] == 0.25 && G[5] == 0.5625 && G[8] == 0.25 && G[1] == 0 && G[6] == 0);
    CHECK(!jpersp_plan(sc, G) && G[0] == 0.25 && G[4] == 0.25 && G[8] == 1.0);
    CHECK(!jpersp_plan(qt, G) && G[1] == 0.125 && G[3] == -0.125 && G[5] == 1.0 && G[8] == 0.125);
    int64_t U, V;
    CHECK(jpersp_position(G, 2, 5, &U, &V) && U == (int64_t)(5.5 * 4294967296.0) && V == (int64_t)(5.5 * 4294967296.0));  // u = y', v = 8 - x'
    return 0;
}

static int check_legality() {
    double G[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
    uint32_t r[4] = {9, 9, 9, 9};
    const double id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(!jpersp_plan(id, G));
    for (int i = 0; i < 9; i++)
        for (double bad : {(double)INFINITY, -(double)INFINITY, (double)NAN}) {
            double m[9];
            memcpy(m, id, sizeof m);
            m[i] = bad;
            double H[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
            CHECK(is(jpersp_plan(m, H), "matrix entry is not finite") && H[0] == 7.0);
            CHECK(is(jpersp_bounds(m, 4, 4, 1, 8, 8, r), "matrix entry is not finite") && r[0] == 9u);
        }
    // an adjugate entry at the edge: a d = 1e154 1e154 = 1e308 is finite, 1.4e154^2 is not
    const double edge_ok[9] = {1e154, 0, 0, 0, 1e154, 0, 0, 0, 1e-160}, edge_bad[9] = {1.4e154, 0, 0, 0, 1.4e154, 0, 0, 0, 1e-160};
    CHECK(!jpersp_plan(edge_ok, G) && G[8] > 0.5 && G[8] <= 1.0);
    CHECK(is(jpersp_plan(edge_bad, G), "adjugate entry is not finite"));
    // the determinant: finite adjugate, a (d s) beyond binary64; 0; next to 0
    const double det_big[9] = {1e120, 0, 0, 0, 1e120, 0, 0, 0, 1e120}, det_ok[9] = {1e100, 0, 0, 0, 1e100, 0, 0, 0, 1e100};
    CHECK(is(jpersp_plan(det_big, G), "determinant is not finite") && !jpersp_plan(det_ok, G));
    const double sing[9] = {1, 2, 0, 2, 4, 0, 0, 0, 1}, near[9] = {1, 2, 0, 2, nextafter(4.0, 5.0), 0, 0, 0, 1}, flat[9] = {1, 0, 0, 0, 1, 0, 0, 0, 0};
    CHECK(is(jpersp_plan(sing, G), "determinant is 0") && is(jpersp_plan(flat, G), "determinant is 0") && !jpersp_plan(near, G));
    CHECK(is(jpersp_bounds(sing, 4, 4, 1, 8, 8, r), "determinant is 0") && r[1] == 9u);
    // the bounds' own arguments
    CHECK(!jpersp_bounds(id, 32768u, 32768u, 2, 32768u, 32768u, r) && r[0] == 0u && r[2] == 32768u && r[3] == 32768u);
    CHECK(is(jpersp_bounds(id, 32769u, 1u, 0, 8u, 8u, r), "32768") && is(jpersp_bounds(id, 1u, 32769u, 0, 8u, 8u, r), "32768"));
    CHECK(is(jpersp_bounds(id, 1u, 1u, 0, 32769u, 8u, r), "32768") && is(jpersp_bounds(id, 1u, 1u, 0, 8u, 32769u, r), "32768"));
    CHECK(is(jpersp_bounds(id, 4u, 4u, 3, 8u, 8u, r), "filter") && is(jpersp_bounds(id, 4u, 4u, -1, 8u, 8u, r), "filter"));
    CHECK(!jpersp_desc_error(2, 3, 1u, 32768u, 1u, 1u, 32768u) && is(jpersp_desc_error(0, 0, 2u, 1u, 1u, 1u, 1u), "flag"));
    CHECK(is(jpersp_desc_error(0, 4, 0u, 1u, 1u, 1u, 1u), "edge") && is(jpersp_desc_error(0, 0, 0u, 1u, 1u, 32769u, 1u), "32768"));
    return 0;
}

// Whether every tap of the axis at position U is outside [0, n).
static bool axis_dead(int filter, int64_t U, int32_t n) {
    float f;
    const int32_t i0 = filter == JWARP_NEAREST ? jwarp_nearest(U) : jwarp_split(U, &f) - (filter == JWARP_BICUBIC ? 1 : 0);
    const int taps = filter == JWARP_NEAREST ? 1 : (filter == JWARP_BILINEAR ? 2 : 4);
    for (int k = 0; k < taps; k++)
        if (jwarp_index(JWARP_EDGE_ZERO, i0 + k, n) >= 0) return false;
    return true;
}

static int check_bounds() {
    const struct { double m[9]; uint32_t sw, sh, dw, dh; bool whole; } rows[] = {
        {{1.1, 0.05, 1e-3, -0.08, 1.05, 5e-4, 2.25, 1.5, 1.0}, 9, 7, 40, 30, false},
        {{0.9, 0.04, 6.25e-4, 0.0, 1.0, 0.0, 14.0, 9.0, 0.96}, 11, 8, 48, 36, false},
        {{-1.1, 0.05, -1e-3, -0.08, 1.05, 5e-4, 30.0, 1.5, 1.0}, 9, 7, 40, 30, false},  // mirrored
        {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 100.0, 3.0, 1.0}, 9, 7, 40, 30, false},          // wholly outside: 0, 0, 0, 0
        {{1.0, 0.0, -0.2, 0.0, 1.0, 0.0, 5.0, 4.0, 1.0}, 9, 7, 40, 30, true},            // w = 1 - 0.2 x crosses 0 inside the rectangle
        {{2.0, 0.0, 0.0, 0.0, 2.0, 0.0, -3.0, -3.0, 1.0}, 30, 30, 24, 20, false},        // clipped on every side
    };
    for (const auto& r : rows) {
        double G[9];
        CHECK(!jpersp_plan(r.m, G));
        for (int filter = 0; filter < JWARP_FILTERS; filter++) {
            uint32_t b[4];
            CHECK(!jpersp_bounds(r.m, r.sw, r.sh, filter, r.dw, r.dh, b));
            CHECK(b[0] + b[2] <= r.dw && b[1] + b[3] <= r.dh && ((b[2] == 0u) == (b[3] == 0u)));
            if (r.whole) CHECK(b[0] == 0u && b[1] == 0u && b[2] == r.dw && b[3] == r.dh);
            uint32_t live_outside = 0, live = 0;
            for (uint32_t Y = 0; Y < r.dh; Y++)
                for (uint32_t X = 0; X < r.dw; X++) {
                    int64_t U = 0, V = 0;
                    const bool zero = !jpersp_position(G, X, Y, &U, &V) || axis_dead(filter, U, (int32_t)r.sw) || axis_dead(filter, V, (int32_t)r.sh);
                    const bool inside = X >= b[0] && X < b[0] + b[2] && Y >= b[1] && Y < b[1] + b[3];
                    live += !zero;
                    live_outside += !zero && !inside;
                }
            CHECK(live_outside == 0u);
            if (b[2] == 0u) CHECK(live == 0u);
            if (&r == &rows[0]) CHECK(live > 0u && b[2] < r.dw && b[3] < r.dh);
        }
    }
    return 0;
}

static int check_routes() {
    int64_t U = 5, V = 5;
    const int64_t top = (int64_t)1 << 54;
    const double zero[9] = {0.125, 0, 0, 0, 0.125, 0, 0, -0.25, 1.625};  // den = 1.625 - y' / 4: 0 at Y = 6
    CHECK(jpersp_position(zero, 0, 5, &U, &V) && !jpersp_position(zero, 0, 6, &U, &V) && !jpersp_position(zero, 3, 7, &U, &V));
    const double tiny[9] = {0.125, 0, -0.8125, 0, 0.125, 0, 0, 0, ldexp(1.0, -1033)};  // q = Inf; n_u = 0 at X = 6
    U = V = 5;
    CHECK(!jpersp_position(tiny, 6, 0, &U, &V) && U == 5 && V == 5);
    CHECK(jpersp_position(tiny, 7, 0, &U, &V) && U == top && V == top && jpersp_position(tiny, 5, 2, &U, &V) && U == -top && V == top);
    const double nan_den[9] = {1, 0, 0, 0, 1, 0, 0, 0, NAN};
    CHECK(!jpersp_position(nan_den, 0, 0, &U, &V));
    // the clamp from both sides: u = x' + 2^22 - 3.5
    const double reach[9] = {1, 0, 4194304.0 - 3.5, 0, 1, 0, 0, 0, 1};
    CHECK(jpersp_position(reach, 2, 0, &U, &V) && U == top - ((int64_t)1 << 32) && jpersp_position(reach, 3, 0, &U, &V) && U == top);
    CHECK(jpersp_position(reach, 4, 0, &U, &V) && U == top && V == ((int64_t)1 << 31));
    // rint, half to even: u 2^32 = x' is an odd number of halves at every texel centre
    const double half[9] = {ldexp(1.0, -32), 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(jpersp_position(half, 0, 0, &U, &V) && U == 0 && jpersp_position(half, 1, 0, &U, &V) && U == 2 && jpersp_position(half, 2, 0, &U, &V) && U == 2);
    const double neg[9] = {-ldexp(1.0, -32), 0, 0, 0, 1, 0, 0, 0, 1};
    CHECK(jpersp_position(neg, 1, 0, &U, &V) && U == -2 && jpersp_position(neg, 3, 0, &U, &V) && U == -4);
    return 0;
}

static int print_positions(char** argv) {
    double m[9], G[9];
    for (int i = 0; i < 9; i++) m[i] = strtod(argv[1 + i], nullptr);
    const uint32_t x = (uint32_t)strtoul(argv[10], nullptr, 10), y = (uint32_t)strtoul(argv[11], nullptr, 10);
    const uint32_t w = (uint32_t)strtoul(argv[12], nullptr, 10), h = (uint32_t)strtoul(argv[13], nullptr, 10);
    if (const char* why = jpersp_plan(m, G)) { fprintf(stderr, "illegal matrix: %s\n", why); return 2; }
    for (uint32_t Y = y; Y < y + h; Y++)
        for (uint32_t X = x; X < x + w; X++) {
            int64_t U, V;
            if (jpersp_position(G, X, Y, &U, &V)) printf("%lld %lld\n", (long long)U, (long long)V);
            else printf("void\n");
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 14) return print_positions(argv);
    if (argc != 1) { fprintf(stderr, "usage: perspective_check [a b p c d q e f s  x y width height]\n"); return 2; }
    if (check_plan()) { fprintf(stderr, "plan failed\n"); return 1; }
    if (check_legality()) { fprintf(stderr, "legality failed\n"); return 1; }
    if (check_bounds()) { fprintf(stderr, "bounds failed\n"); return 1; }
    if (check_routes()) { fprintf(stderr, "routes failed\n"); return 1; }
    printf("ok: the plan on 20000 integer matrices, legality, the bounds by brute force, the position's routes\n");
    return 0;
}
