// blur_taps_check.cpp -- include/jello_blur.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/blur_taps_check.cpp -o /tmp/blur_taps_check && /tmp/blur_taps_check
//
// Calls jblur_taps into an array of exactly 2 R + 1 floats (so that a write past either end is an AddressSanitizer report) for
// every R step, its neighbours and a sweep, and checks what the rule promises of the taps.  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jello_blur.h"

static int check(float sigma) {
    if (!jblur_sigma_ok(sigma)) return 0;
    const uint32_t R = jblur_taps(sigma, nullptr);
    if (R != jblur_radius(sigma) || R > JBLUR_MAX_RADIUS || R != (uint32_t)ceil(3.0 * (double)sigma)) return 1;
    std::vector<float> w(2u * R + 1u, -1.0f);
    if (jblur_taps(sigma, w.data()) != R) return 2;
    double sum = 0.0;
    for (uint32_t k = 0; k <= 2u * R; k++) {
        if (!(w[k] >= 0.0f && w[k] <= 1.0f) || w[k] != w[2u * R - k]) return 3;
        if (k > 0 && k <= R && w[k] < w[k - 1]) return 4;
        sum += (double)w[k];
    }
    if (fabs(sum - 1.0) > (2.0 * R + 2.0) * ldexp(1.0, -24)) return 5;
    if (R == 0 && w[0] != 1.0f) return 6;
    return 0;
}

int main() {
    int n = 0;
    const float bad[] = {-1.0f, -1e-30f, nextafterf(64.0f, 100.0f), INFINITY, -INFINITY, NAN};
    for (float s : bad)
        if (jblur_sigma_ok(s)) { printf("accepted %g\n", (double)s); return 1; }
    std::vector<float> sigmas = {0.0f, -0.0f, nextafterf(0.0f, 1.0f), 1e-30f, 0.05f, 0.07f, 0.3f, 64.0f, nextafterf(64.0f, 0.0f)};
    for (uint32_t r = 1; r <= JBLUR_MAX_RADIUS; r++) {
        const float step = (float)(r / 3.0);
        sigmas.push_back(step);
        sigmas.push_back(nextafterf(step, 0.0f));
        if (step < 64.0f) sigmas.push_back(nextafterf(step, 100.0f));
    }
    for (int i = 0; i <= 4096; i++) sigmas.push_back(64.0f * (float)i / 4096.0f);
    for (float s : sigmas) {
        if (int rc = check(s)) { printf("sigma %.9g: check %d failed\n", (double)s, rc); return 1; }
        n++;
    }
    printf("ok: %d sigmas\n", n);
    return 0;
}
