// resample_taps_check.cpp -- include/jello_resample.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/resample_taps_check.cpp -o /tmp/resample_taps_check && /tmp/resample_taps_check
//
// Calls jresample_taps into an array of exactly as many floats as the window has taps (so that a write past either end is an
// AddressSanitizer report) for every filter, every n_out up to a limit (default 40; the first argument) and every legal n_in, and
// checks what the rule promises of a window: 1..96 taps inside the axis, S >= 0.48, weights that sum to 1 within their rounding,
// the single tap 1.0f at equal sizes (not LANCZOS3).  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jello_resample.h"

static uint32_t g_most[JRESAMPLE_FILTERS];
static double g_least_sum[JRESAMPLE_FILTERS] = {1e9, 1e9, 1e9, 1e9};

static int check(int filter, uint32_t n_in, uint32_t n_out) {
    for (uint32_t i = 0; i < n_out; i++) {
        uint32_t first = 0xffffffffu;
        double S = 0.0;
        const uint32_t n = jresample_taps(filter, n_in, n_out, i, nullptr, &first, &S);
        if (n == 0u || n > JRESAMPLE_MAX_TAPS) return 1;
        if ((uint64_t)first + n > n_in) return 2;
        if (!(S >= 0.48)) return 3;
        std::vector<float> w(n, -1.0f);
        uint32_t first2 = 0u;
        if (jresample_taps(filter, n_in, n_out, i, w.data(), &first2, nullptr) != n || first2 != first) return 4;
        double sum = 0.0, mag = 0.0;
        for (float v : w) {
            if (!isfinite(v)) return 5;
            sum += (double)v;
            mag += fabs((double)v);
        }
        if (fabs(sum - 1.0) > (n + 1.0) * mag * ldexp(1.0, -24)) return 6;
        if (n_in == n_out && filter != JRESAMPLE_LANCZOS3 && (n != 1u || first != i || w[0] != 1.0f)) return 7;
        if (n > g_most[filter]) g_most[filter] = n;
        if (S < g_least_sum[filter]) g_least_sum[filter] = S;
    }
    return 0;
}

int main(int argc, char** argv) {
    const uint32_t limit = argc > 1 ? (uint32_t)atoi(argv[1]) : 40u;
    if (jresample_filter_ok(-1) || jresample_filter_ok(JRESAMPLE_FILTERS) || jresample_sizes_ok(0u, 1u) || jresample_sizes_ok(1u, 0u) ||
        jresample_sizes_ok(17u, 1u) || !jresample_sizes_ok(16u, 1u) || jresample_sizes_ok(0xffffffffu, 0x0fffffffu) || !jresample_sizes_ok(1u, 0xffffffffu)) {
        printf("the legality checks are wrong\n");
        return 1;
    }
    long long axes = 0;
    for (int filter = 0; filter < JRESAMPLE_FILTERS; filter++) {
        for (uint32_t n_out = 1; n_out <= limit; n_out++)
            for (uint32_t n_in = 1; n_in <= JRESAMPLE_MAX_RATIO * n_out; n_in++) {
                if (int rc = check(filter, n_in, n_out)) { printf("filter %d, %u -> %u: check %d failed\n", filter, n_in, n_out, rc); return 1; }
                axes++;
            }
        // large axes: the arithmetic near 2^32, and the sizes of the frames the call is for
        const uint32_t big[][2] = {{4096u, 2048u}, {4096u, 1080u}, {2048u, 4096u}, {4096u, 256u}, {0xffffffffu, 0x10000000u}, {1u, 70000u}, {65535u, 4096u}};
        for (const auto& b : big) {
            const uint32_t n_out = b[1] > 70000u ? 70000u : b[1];  // (the first outputs of a very long axis are enough)
            for (uint32_t i : {0u, 1u, n_out / 2u, n_out - 1u, b[1] - 1u}) {
                uint32_t first = 0u;
                std::vector<float> w(JRESAMPLE_MAX_TAPS, -1.0f);
                const uint32_t n = jresample_taps(filter, b[0], b[1], i, w.data(), &first, nullptr);
                if (n == 0u || n > JRESAMPLE_MAX_TAPS || (uint64_t)first + n > b[0]) { printf("filter %d, %u -> %u, output %u: bad window\n", filter, b[0], b[1], i); return 1; }
            }
        }
    }
    for (int filter = 0; filter < JRESAMPLE_FILTERS; filter++) printf("filter %d: most taps %u, least S %.6f\n", filter, g_most[filter], g_least_sum[filter]);
    printf("ok: %lld axes\n", axes);
    return 0;
}
