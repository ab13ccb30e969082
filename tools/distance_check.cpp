// distance_check.cpp -- include/jello_distance.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/distance_check.cpp -o /tmp/distance_check && /tmp/distance_check
//
// Three things.  (1) jdist_desc_error and jdist_plan over legal descriptors -- every channel, which, edge, flag and radius -- and over a
// set of illegal ones, on both sides of every boundary; the plan's geometry against a count of the plane elements the passes below
// touch.  (2) The decomposition kernels_distance.hip uses, built from the header's pieces -- columns by the clamped run-length counter,
// down and up over segments with an R-row warm-up, into planes of rect_h x (rect_w + 2 R); rows by the walk outwards from dx = 0 with
// the exact stop -- written scalar with exactly sized arrays (a read or write past an end is an AddressSanitizer report), against an
// all-pairs brute force over the SET of features, on images up to 12 x 12 with R = 1..5 and R = 255, in every which x edge, whole
// images and rectangles.  (3) jdist_value: no NaN and a value in [0, 1] for every reachable s under a set of finite ramps, extreme
// ones among them.  Prints "ok" and returns 0.
//
// With arguments -- W H R which edge SEEDS, SEEDS a string of W * H characters, '1' a seed, row by row -- it prints the two-pass D of
// every texel of the image, H lines of W integers: Dout for OUTER, Din for INNER, and for SIGNED Dout on a non-seed and -Din on a seed.
// tests/test_distance_spec.py compares that with tests/distance_ref.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jello_distance.h"

struct Image {
    uint32_t W, H;
    std::vector<uint8_t> seed;  // W * H
};

// The all-pairs definition: min(cap, min over the features of dx^2 + dy^2); inner under ZERO: the positions outside the image too,
// walked over a margin of R + 1 around it (a feature farther than R in x or y is at least cap away).
static uint32_t brute(const Image& im, int64_t X, int64_t Y, uint32_t R, bool inner, bool clamp) {
    const int64_t m = (int64_t)R + 1;
    uint64_t best = jdist_cap(R);
    for (int64_t y = Y - m; y <= Y + m; y++)
        for (int64_t x = X - m; x <= X + m; x++) {
            const bool in_image = x >= 0 && y >= 0 && x < (int64_t)im.W && y < (int64_t)im.H;
            bool feature;
            if (in_image) feature = (im.seed[(size_t)(y * im.W + x)] != 0) != inner;
            else feature = inner && !clamp;
            if (!feature) continue;
            const uint64_t d = (uint64_t)((x - X) * (x - X) + (y - Y) * (y - Y));
            if (d < best) best = d;
        }
    return (uint32_t)best;
}

// The two passes as the kernels make them, for one plane (inner or outer) over the rectangle r; seg_rows: the rows of a column
// segment.  D: r.w * r.h.  *touched: the plane elements written (each once on the way down).
static void two_pass(const Image& im, jimage_rect r, uint32_t R, bool inner, bool clamp, uint32_t seg_rows, std::vector<uint32_t>& D, uint64_t* touched) {
    const uint64_t pc = jdist_plane_cols(r.w, R), pr = jdist_plane_rows(r.h);
    std::vector<uint16_t> plane((size_t)(pc * pr));
    for (uint32_t v0 = 0; v0 < r.h; v0 += seg_rows) {
        const uint32_t v1 = r.h - v0 < seg_rows ? r.h : v0 + seg_rows;
        const uint32_t Y0 = r.y + v0, Y1 = r.y + v1;
        for (uint64_t c = 0; c < pc; c++) {
            const int64_t xs = (int64_t)r.x - R + (int64_t)c;
            const bool in_image = xs >= 0 && xs < (int64_t)im.W;
            auto feature = [&](uint32_t Y) { return in_image ? ((im.seed[(size_t)Y * im.W + (size_t)xs] != 0) != inner) : (inner && !clamp); };
            const uint32_t ys = Y0 > R ? Y0 - R : 0u;
            uint32_t run = jdist_run_start(ys == 0u, inner, clamp, R);
            if (in_image)
                for (uint32_t Y = ys; Y < Y0; Y++) run = jdist_run(run, feature(Y), R);
            for (uint32_t v = v0; v < v1; v++) {
                run = jdist_run(run, feature(r.y + v), R);
                plane.at((size_t)(v * pc + c)) = (uint16_t)run;
                ++*touched;
            }
            const uint32_t ye = (uint64_t)Y1 + R < im.H ? Y1 + R : im.H;
            run = jdist_run_start(ye == im.H, inner, clamp, R);
            if (in_image)
                for (uint32_t Y = ye; Y > Y1; Y--) run = jdist_run(run, feature(Y - 1u), R);
            for (uint32_t v = v1; v > v0; v--) {
                uint16_t& g = plane.at((size_t)((v - 1u) * pc + c));
                run = jdist_run(run, g == 0u, R);
                if (run < g) g = (uint16_t)run;
            }
        }
    }
    D.assign((size_t)r.w * r.h, 0u);
    for (uint32_t v = 0; v < r.h; v++) {
        const uint16_t* g = plane.data() + (size_t)(v * pc);  // element e is plane column e; output o sits at o + R
        for (uint32_t o = 0; o < r.w; o++) {
            const uint32_t i = o + R;
            uint32_t best = jdist_combine(jdist_cap(R), 0u, g[i]);
            for (uint32_t dx = 1u; dx <= R && !jdist_stop(best, dx); dx++) {
                if (i < dx || i + dx >= pc) { printf("the walk leaves the plane row\n"); exit(1); }
                best = jdist_combine(best, dx, g[i - dx]);
                best = jdist_combine(best, dx, g[i + dx]);
            }
            D[(size_t)v * r.w + o] = best;
        }
    }
}

static jh_distance_desc legal_desc() {
    jh_distance_desc d;
    memset(&d, 0, sizeof d);
    d.channel = 3; d.threshold = 0.5f; d.which = JDIST_OUTER; d.edge = JDIST_EDGE_ZERO; d.max_distance = 4u; d.scale = 1.0f; d.offset = 0.0f;
    return d;
}

static int check_descriptors() {
    const uint32_t W = 40, H = 24;
    for (int ch = 0; ch <= 3; ch++)
        for (int which = 0; which <= 2; which++)
            for (int edge = 0; edge <= 1; edge++)
                for (uint32_t flags = 0; flags <= 1u; flags++)
                    for (uint32_t R = 1; R <= JDIST_MAX_RADIUS; R++) {
                        jh_distance_desc d = legal_desc();
                        d.channel = ch; d.which = which; d.edge = edge; d.flags = flags; d.max_distance = R;
                        d.x = 3; d.y = 5; d.width = 30; d.height = 11;
                        jh_dist_plan p;
                        if (jdist_desc_error(&d) || jdist_plan(&d, W, H, &p)) return 1;
                        if (p.x != 3u || p.y != 5u || p.width != 30u || p.height != 11u || p.radius != R || p.cap != (R + 1u) * (R + 1u)) return 2;
                        if (p.planes != (which == 2 ? 2u : 1u) || p.plane_columns != 30u + 2u * R || p.plane_rows != 11u) return 3;
                        if (p.scratch_bytes != (uint64_t)p.planes * p.plane_columns * p.plane_rows * 2u) return 4;
                    }
    jh_distance_desc d = legal_desc();
    jh_dist_plan p;
    if (jdist_plan(&d, W, H, &p) || p.width != W || p.height != H || p.x != 0u) return 5;       // 0 x 0: the whole image
    if (jdist_plan(&d, 0u, 0u, &p) || p.scratch_bytes != 0u) return 6;                             // an image without texels
    struct { int field; double value; } bad[] = {{0, -1}, {0, 4}, {1, -1}, {1, 3}, {2, -1}, {2, 2}, {3, 2}, {3, 0x80000001u}, {4, 0}, {4, 256}, {4, 4294967295.0},
                                                 {5, INFINITY}, {5, NAN}, {6, -INFINITY}, {6, NAN}, {7, INFINITY}, {7, NAN}};
    for (const auto& b : bad) {
        jh_distance_desc e = legal_desc();
        switch (b.field) {
            case 0: e.channel = (int)b.value; break;
            case 1: e.which = (int)b.value; break;
            case 2: e.edge = (int)b.value; break;
            case 3: e.flags = (uint32_t)b.value; break;
            case 4: e.max_distance = (uint32_t)b.value; break;
            case 5: e.threshold = (float)b.value; break;
            case 6: e.scale = (float)b.value; break;
            default: e.offset = (float)b.value; break;
        }
        if (!jdist_desc_error(&e) || !jdist_plan(&e, W, H, &p)) return 10 + b.field;
    }
    for (int k = 0; k < 2; k++) {  // on the legal side of the boundaries
        jh_distance_desc e = legal_desc();
        e.max_distance = k ? 255u : 1u; e.channel = k ? 3 : 0; e.threshold = k ? 3.4e38f : -3.4e38f; e.scale = k ? -3.4e38f : 1e-45f;
        if (jdist_desc_error(&e)) return 20;
    }
    const uint32_t rects[][4] = {{8, 0, 33, 4}, {0, 21, 4, 4}, {0xFFFFFFFFu, 0, 2, 2}, {0, 0xFFFFFFFFu, 2, 2}, {2, 2, 0, 4}, {2, 2, 4, 0}};
    for (const auto& q : rects) {
        jh_distance_desc e = legal_desc();
        e.x = q[0]; e.y = q[1]; e.width = q[2]; e.height = q[3];
        if (jdist_desc_error(&e) || !jdist_plan(&e, W, H, &p)) return 21;
    }
    return 0;
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static int check_passes(uint64_t* cases) {
    const uint32_t radii[] = {1, 2, 3, 4, 5, 255};
    for (uint32_t trial = 0; trial < 60u; trial++) {
        Image im;
        im.W = 1u + rnd() % 12u; im.H = 1u + rnd() % 12u;
        im.seed.resize((size_t)im.W * im.H);
        const uint32_t density = trial % 5u == 0u ? 0u : (trial % 5u == 1u ? 100u : 3u + rnd() % 60u);  // none, all, some
        for (auto& s : im.seed) s = rnd() % 100u < density;
        jimage_rect r = {0, 0, im.W, im.H};
        if (trial % 3u == 2u) {
            r.x = rnd() % im.W; r.y = rnd() % im.H;
            r.w = 1u + rnd() % (im.W - r.x); r.h = 1u + rnd() % (im.H - r.y);
        }
        for (uint32_t R : radii)
            for (int inner = 0; inner <= 1; inner++)
                for (int clamp = 0; clamp <= 1; clamp++) {
                    const uint32_t seg_rows = 1u + rnd() % 5u;
                    std::vector<uint32_t> D;
                    uint64_t touched = 0;
                    two_pass(im, r, R, inner != 0, clamp != 0, seg_rows, D, &touched);
                    if (touched * 2u != jdist_scratch_bytes(r.w, r.h, R, inner ? JDIST_INNER : JDIST_OUTER)) return 1;
                    if (2u * touched * 2u != jdist_scratch_bytes(r.w, r.h, R, JDIST_SIGNED)) return 2;
                    for (uint32_t v = 0; v < r.h; v++)
                        for (uint32_t o = 0; o < r.w; o++)
                            if (D[(size_t)v * r.w + o] != brute(im, r.x + o, r.y + v, R, inner != 0, clamp != 0)) {
                                printf("%ux%u rect %u %u %u %u R %u inner %d clamp %d at (%u, %u): %u, the set gives %u\n", im.W, im.H, r.x, r.y, r.w, r.h, R, inner, clamp,
                                       o, v, D[(size_t)v * r.w + o], brute(im, r.x + o, r.y + v, R, inner != 0, clamp != 0));
                                return 3;
                            }
                    ++*cases;
                }
    }
    return 0;
}

static int check_values() {
    const float ramps[][2] = {{1.0f, 0.0f}, {-1.0f, 3.0f}, {0.0f, 0.25f}, {0.0f, -0.0f}, {3.4e38f, -3.4e38f}, {-3.4e38f, 3.4e38f}, {3.4e38f, 3.4e38f}, {1e-45f, -1e-45f},
                              {1.0f / 510.0f, 0.5f}, {-0.125f, 0.75f}};
    for (const auto& k : ramps)
        for (int which = 0; which <= 2; which++)
            for (uint32_t D = 0; D <= 65536u; D++)
                for (int seed = 0; seed <= (which == 2 ? 1 : 0); seed++) {
                    const float v = jdist_value(D, D, seed != 0, which, k[0], k[1]);
                    if (!(v >= 0.0f && v <= 1.0f)) return 1;  // (a NaN fails both)
                }
    if (jdist_value(9u, 0u, false, JDIST_OUTER, 1.0f, 0.0f) != 1.0f || jdist_value(9u, 4u, true, JDIST_SIGNED, 0.25f, 0.5f) != 0.125f) return 2;
    if (jdist_value(9u, 4u, false, JDIST_SIGNED, 0.25f, 0.0f) != 0.625f || jdist_value(9u, 4u, false, JDIST_INNER, 0.25f, 0.0f) != 0.5f) return 3;
    if (!jdist_is_seed(-0.0f, 0.0f) || !jdist_is_seed(0.0f, -0.0f) || jdist_is_seed(NAN, -1.0f) || !jdist_is_seed(INFINITY, 3.4e38f)) return 4;
    return 0;
}

static int print_image(char** a) {
    Image im;
    im.W = (uint32_t)atoi(a[1]); im.H = (uint32_t)atoi(a[2]);
    const uint32_t R = (uint32_t)atoi(a[3]);
    const int which = atoi(a[4]), clamp = atoi(a[5]);
    if (im.W == 0u || im.H == 0u || im.W > 4096u || im.H > 4096u || R < 1u || R > JDIST_MAX_RADIUS || which < 0 || which > 2 || strlen(a[6]) != (size_t)im.W * im.H) return 2;
    for (const char* p = a[6]; *p; p++) im.seed.push_back(*p == '1');
    const jimage_rect r = {0, 0, im.W, im.H};
    std::vector<uint32_t> Dout, Din;
    uint64_t touched = 0;
    two_pass(im, r, R, false, clamp != 0, 3u, Dout, &touched);
    two_pass(im, r, R, true, clamp != 0, 4u, Din, &touched);
    for (uint32_t y = 0; y < im.H; y++) {
        for (uint32_t x = 0; x < im.W; x++) {
            const size_t i = (size_t)y * im.W + x;
            const long d = which == JDIST_OUTER ? (long)Dout[i] : (which == JDIST_INNER ? (long)Din[i] : (im.seed[i] ? -(long)Din[i] : (long)Dout[i]));
            printf("%ld%c", d, x + 1u == im.W ? '\n' : ' ');
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7) return print_image(argv);
    if (argc != 1) return 2;
    if (int rc = check_descriptors()) { printf("descriptors: %d\n", rc); return 1; }
    uint64_t cases = 0;
    if (int rc = check_passes(&cases)) { printf("passes: %d\n", rc); return 1; }
    if (int rc = check_values()) { printf("values: %d\n", rc); return 1; }
    printf("ok: %llu decompositions against the set\n", (unsigned long long)cases);
    return 0;
}
