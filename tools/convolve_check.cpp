// convolve_check.cpp -- include/jello_convolve.h (and the index rules it takes from include/jello_warp.h) exercised stand-alone, for
// the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/convolve_check.cpp -o /tmp/convolve_check && /tmp/convolve_check
//
// Four things.  (1) jconv_desc_error on every legal (order_x, order_y, target_x, target_y, edge, mode) with a weights array of
// exactly order_x * order_y floats on the heap (a read past it is the sanitizer's to find), and on a set of illegal descriptors, each
// with the text it has to answer.  (2) jconv_weights against long double on small kernels: the flip, the quotient and its single
// rounding.  (3) The default divisor: the sum in ascending order, a sum of 0 (divisor 1), an explicit divisor, and what is refused.
// (4) jwarp_index for n = 1..5 and offsets -14 .. n + 13 -- every index an order-15 window can ask for -- against a walk that steps
// from 0 one texel at a time.  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jello_convolve.h"

static bool says(const char* got, const char* want) { return want ? (got && strstr(got, want)) : got == nullptr; }

static int check_descriptors() {
    for (uint32_t ox = 1; ox <= JCONV_MAX_ORDER; ox++)
        for (uint32_t oy = 1; oy <= JCONV_MAX_ORDER; oy++) {
            std::vector<float> w(ox * oy, 0.5f);  // exactly what is read
            for (uint32_t tx = 0; tx < ox; tx++)
                for (uint32_t ty = 0; ty < oy; ty++)
                    for (int edge = 0; edge < JWARP_EDGES; edge++)
                        for (int mode = 0; mode < JCONV_MODES; mode++)
                            if (jconv_desc_error(ox, oy, tx, ty, edge, mode, w.data(), -0.25f)) return 1;
            if (!says(jconv_desc_error(ox, oy, ox, 0, 0, 0, w.data(), 0.0f), "target")) return 2;
            if (!says(jconv_desc_error(ox, oy, 0, oy, 0, 0, w.data(), 0.0f), "target")) return 3;
            if (!says(jconv_desc_error(ox, oy, 0xffffffffu, 0, 0, 0, w.data(), 0.0f), "target")) return 4;
            w[ox * oy - 1u] = INFINITY;
            if (!says(jconv_desc_error(ox, oy, 0, 0, 0, 0, w.data(), 0.0f), "weight")) return 5;
            w[ox * oy - 1u] = 0.5f;
            w[0] = NAN;
            if (!says(jconv_desc_error(ox, oy, 0, 0, 0, 0, w.data(), 0.0f), "weight")) return 6;
        }
    const float one[1] = {1.0f};
    const uint32_t bad_orders[][2] = {{0, 1}, {1, 0}, {16, 1}, {1, 16}, {0, 0}, {0xffffffffu, 0xffffffffu}, {65536u, 65536u}};
    for (const auto& o : bad_orders)
        if (!says(jconv_desc_error(o[0], o[1], 0, 0, 0, 0, one, 0.0f), "order")) return 7;  // (nothing of the weights is read)
    if (!says(jconv_desc_error(1, 1, 0, 0, 4, 0, one, 0.0f), "edge") || !says(jconv_desc_error(1, 1, 0, 0, -1, 0, one, 0.0f), "edge")) return 8;
    if (!says(jconv_desc_error(1, 1, 0, 0, 0, 3, one, 0.0f), "mode") || !says(jconv_desc_error(1, 1, 0, 0, 0, -1, one, 0.0f), "mode")) return 9;
    if (!says(jconv_desc_error(1, 1, 0, 0, 0, 0, one, NAN), "bias") || !says(jconv_desc_error(1, 1, 0, 0, 0, 0, one, -INFINITY), "bias")) return 10;
    // a weight beyond the ones that are read may be anything
    const float tail[4] = {1.0f, 2.0f, NAN, INFINITY};
    if (jconv_desc_error(2, 1, 1, 0, 3, 2, tail, 0.0f)) return 11;
    return 0;
}

static int check_weights() {
    // small kernels against long double: weights[j ox + i] = (float)(km[(oy - 1 - j) ox + (ox - 1 - i)] / d)
    uint32_t seed = 12345u;
    for (uint32_t ox = 1; ox <= 5u; ox++)
        for (uint32_t oy = 1; oy <= 5u; oy++)
            for (int trial = 0; trial < 8; trial++) {
                std::vector<double> km(ox * oy);
                for (double& v : km) {
                    seed = seed * 1664525u + 1013904223u;
                    v = ((double)(seed >> 8) / 8388608.0 - 1.0) * (trial % 2 ? 1e-3 : 7.0);
                }
                const double divisor = trial < 4 ? 0.0 : (trial % 3 - 1.5) * 3.7;
                long double d = divisor;
                if (divisor == 0.0) {
                    double sum = 0.0;
                    for (double v : km) sum = sum + v;
                    d = sum == 0.0 ? 1.0 : sum;
                }
                std::vector<float> w(ox * oy, -99.0f);
                if (jconv_weights(ox, oy, km.data(), divisor, w.data())) return 20;
                for (uint32_t j = 0; j < oy; j++)
                    for (uint32_t i = 0; i < ox; i++) {
                        // binary64 division is correctly rounded and so is the long double one: the double of the long double quotient
                        // is the binary64 quotient unless a double rounding strikes, which one ULP of slack in binary32 allows for
                        const long double q = (long double)km[(oy - 1u - j) * ox + (ox - 1u - i)] / d;
                        const float want = (float)(double)q, got = w[j * ox + i];
                        if (got != want && got != nextafterf(want, INFINITY) && got != nextafterf(want, -INFINITY)) return 21;
                        if (got != (float)(km[(oy - 1u - j) * ox + (ox - 1u - i)] / (double)d)) return 22;  // (and exactly the binary64 route)
                    }
            }
    return 0;
}

static int check_divisor() {
    float w[9];
    const double asym[6] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0};  // 3 x 2, sum 21
    if (jconv_weights(3, 2, asym, 0.0, w)) return 30;
    for (int k = 0; k < 6; k++)
        if (w[k] != (float)(asym[5 - k] / 21.0)) return 31;
    const double sobel[9] = {-1.0, 0.0, 1.0, -2.0, 0.0, 2.0, -1.0, 0.0, 1.0};  // sum 0: divisor 1
    if (jconv_weights(3, 3, sobel, 0.0, w)) return 32;
    for (int k = 0; k < 9; k++)
        if (w[k] != (float)sobel[8 - k]) return 33;
    if (jconv_weights(3, 3, sobel, -4.0, w) || w[0] != -0.25f || w[2] != 0.25f || w[3] != -0.5f) return 34;
    // the sum is taken in ascending index order: 1e17 + 1 - 1e17 is 0 that way (divisor 1) and 1 in any order that adds 1 last
    const double order[3] = {1e17, 1.0, -1e17};
    if (jconv_weights(3, 1, order, 0.0, w) || w[0] != (float)-1e17 || w[1] != 1.0f || w[2] != (float)1e17) return 35;
    const double one[1] = {1.0};
    if (!says(jconv_weights(0, 1, one, 0.0, w), "order") || !says(jconv_weights(1, 16, one, 0.0, w), "order")) return 36;
    if (!says(jconv_weights(1, 1, one, NAN, w), "divisor") || !says(jconv_weights(1, 1, one, INFINITY, w), "divisor")) return 37;
    const double inf[2] = {1.0, INFINITY}, huge[2] = {1e308, 1e308}, big[1] = {1e300};
    if (!says(jconv_weights(2, 1, inf, 1.0, w), "entry") || !says(jconv_weights(2, 1, huge, 0.0, w), "sum")) return 38;
    if (!says(jconv_weights(1, 1, big, 1.0, w), "finite") || !says(jconv_weights(1, 1, one, 1e-300, w), "finite")) return 39;
    if (jconv_weights(1, 1, one, -0.0, w) || w[0] != 1.0f) return 40;  // (-0 is 0: the default)
    return 0;
}

static int check_index() {
    for (int32_t n = 1; n <= 5; n++) {
        // the walk: position 0 is index 0; REPEAT steps round the n texels, MIRROR walks to the end, repeats the edge texel, walks back
        for (int dir = -1; dir <= 1; dir += 2) {
            int32_t repeat = 0, mirror = 0, mirror_step = 1;  // (going left from 0 too: position -1 is index 0 again, then upwards)
            for (int32_t k = 0; k <= n + 13; k++) {
                const int32_t i = dir * k;
                if (i < -14) break;
                if (jwarp_index(JCONV_EDGE_REPEAT, i, n) != repeat) return 50;
                if (jwarp_index(JCONV_EDGE_MIRROR, i, n) != mirror) return 51;
                if (jwarp_index(JCONV_EDGE_CLAMP, i, n) != (i < 0 ? 0 : (i >= n ? n - 1 : i))) return 52;
                if (jwarp_index(JCONV_EDGE_ZERO, i, n) != ((i >= 0 && i < n) ? i : -1)) return 53;
                // one step further
                repeat = dir > 0 ? (repeat + 1 == n ? 0 : repeat + 1) : (repeat == 0 ? n - 1 : repeat - 1);
                if (dir < 0 && k == 0) continue;  // (-1 mirrors 0: the edge texel is repeated, the index stays)
                const int32_t next = mirror + mirror_step;
                if (next < 0 || next >= n) mirror_step = -mirror_step;  // (the edge texel is repeated, then the walk turns)
                else mirror = next;
            }
        }
    }
    return 0;
}

int main() {
    int rc = check_descriptors();
    if (!rc) rc = check_weights();
    if (!rc) rc = check_divisor();
    if (!rc) rc = check_index();
    if (rc) { printf("FAILED: check %d\n", rc); return 1; }
    printf("ok\n");
    return 0;
}
