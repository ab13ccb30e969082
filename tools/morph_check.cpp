// morph_check.cpp -- include/jello_morph.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/morph_check.cpp -o /tmp/morph_check && /tmp/morph_check
//
// Three things.  (1) jmorph_desc_error over every legal (op, edge, flags, radius_x, radius_y), with the sizes of the intermediate for a
// set of rectangles, and over a set of illegal descriptors (the rectangles' own check: tools/image_rect_check.cpp).  (2) The order key against a direct comparison of the values -- every f16 bit pattern widened to binary32,
// and the products of a few thousand pairs of them: sorted by key the values ascend in totalOrder, distinct values have distinct
// keys, the inverse gives the value back, a NaN of either sign maps to the operator's extreme and nothing maps to the neutral key.
// (3) The decomposition kernels_morph.hip uses -- rows by doubling in place, columns by block prefix and suffix over planes of
// rect_h + 2 ry rows -- written scalar with exactly sized arrays (a read or write past an end is an AddressSanitizer report),
// against a brute-force walk of every window, on tiny images.  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jello_image.h"
#include "jello_morph.h"

static uint32_t f16_bits_to_f32_bits(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    if (exp == 0x1fu) return sign | 0x7f800000u | (man << 13);
    if (exp == 0u) {
        if (man == 0u) return sign;
        const float v = ldexpf((float)man, -24);
        uint32_t b;
        memcpy(&b, &v, 4);
        return sign | b;
    }
    return sign | ((exp + 112u) << 23) | (man << 13);
}
static float as_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static bool is_nan_bits(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }

// -1, 0, 1: a below, equal to, above b in totalOrder, by comparing the VALUES (both not NaN)
static int direct_compare(uint32_t a, uint32_t b) {
    const float x = as_float(a), y = as_float(b);
    if (x < y) return -1;
    if (x > y) return 1;
    const int sa = (int)(a >> 31), sb = (int)(b >> 31);  // equal values: the same pattern, or the two zeros (-0 below +0)
    return sa == sb ? 0 : (sa ? -1 : 1);
}

static int check_descriptors() {
    const uint32_t W = 40, H = 24;
    const uint32_t rects[][4] = {{0, 0, 0, 0}, {0, 0, W, H}, {3, 5, 1, 1}, {W - 1, H - 1, 1, 1}, {7, 0, W - 7, H}, {99, 99, 0, 0}};
    for (int op = 0; op <= 1; op++)
        for (int edge = 0; edge <= 1; edge++)
            for (uint32_t flags = 0; flags <= 1u; flags++)
                for (uint32_t rx = 0; rx <= JMORPH_MAX_RADIUS; rx++)
                    for (uint32_t ry = 0; ry <= JMORPH_MAX_RADIUS; ry++)
                        for (const auto& r : rects) {
                            if (jmorph_desc_error(op, edge, flags, rx, ry) || jimage_rect_check({r[0], r[1], r[2], r[3]}, W, H) != JIMAGE_RECT_OK) return 1;
                            const jimage_rect q = jimage_resolve({r[0], r[1], r[2], r[3]}, W, H);
                            if (q.w == 0u || q.h == 0u || q.x + q.w > W || q.y + q.h > H) return 2;
                            if (jmorph_plane_rows(q.h, ry) != q.h + 2u * ry || jmorph_scratch_bytes(q.w, q.h, ry) != 32ull * q.w * (q.h + 2u * ry)) return 3;
                        }
    struct Bad { int op, edge; uint32_t flags, rx, ry, x, y, w, h; };
    const Bad bad[] = {
        {2, 0, 0, 1, 1, 0, 0, 0, 0},  {-1, 0, 0, 1, 1, 0, 0, 0, 0}, {0, 2, 0, 1, 1, 0, 0, 0, 0},          {0, -1, 0, 1, 1, 0, 0, 0, 0},
        {0, 0, 2, 1, 1, 0, 0, 0, 0},  {0, 0, 0x80000001u, 1, 1, 0, 0, 0, 0}, {1, 1, 1, 256, 0, 0, 0, 0, 0}, {1, 1, 1, 0, 256, 0, 0, 0, 0},
        {1, 1, 1, 0xffffffffu, 0, 0, 0, 0, 0}, {1, 0, 0, 1, 1, 2, 2, 0, 4}, {1, 0, 0, 1, 1, 2, 2, 4, 0}, {1, 0, 0, 1, 1, 8, 0, W - 7, 4},
        {1, 0, 0, 1, 1, 0, 9, 4, H - 8}, {1, 0, 0, 1, 1, 0xffffffffu, 0, 2, 2}, {1, 0, 0, 1, 1, 0, 0xffffffffu, 2, 2}, {1, 0, 0, 1, 1, 0, 0, W + 1, H},
    };
    for (const Bad& b : bad)
        if (!jmorph_desc_error(b.op, b.edge, b.flags, b.rx, b.ry) && jimage_rect_check({b.x, b.y, b.w, b.h}, W, H) == JIMAGE_RECT_OK) return 4;
    if (jmorph_desc_error(0, 0, 0, 0, 0) || jimage_rect_check({0, 0, 0, 0}, 0, 0) != JIMAGE_RECT_OK) return 5;  // an image without texels: its whole is legal
    return 0;
}

static int check_order(const std::vector<uint32_t>& values) {
    for (int dilate = 0; dilate <= 1; dilate++) {
        std::vector<uint32_t> v;
        for (uint32_t b : values) {
            const int32_t k = jmorph_key(b, dilate);
            if (is_nan_bits(b)) {
                if (k != (dilate ? INT32_MAX : INT32_MIN)) return 1;
                if (!is_nan_bits(jmorph_unkey(k))) return 2;
                continue;
            }
            if (k == jmorph_neutral(dilate) || k == jmorph_neutral(!dilate)) return 3;  // (no value maps to either extreme)
            if (jmorph_unkey(k) != b) return 4;
            v.push_back(b);
        }
        std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return jmorph_key(a, dilate) < jmorph_key(b, dilate); });
        for (size_t i = 1; i < v.size(); i++) {
            const int32_t ka = jmorph_key(v[i - 1], dilate), kb = jmorph_key(v[i], dilate);
            const int d = direct_compare(v[i - 1], v[i]);
            if (d > 0) return 5;                  // sorted by key the values never descend
            if ((d == 0) != (ka == kb)) return 6;  // and equal keys are equal patterns
        }
    }
    if (jmorph_key(0u, 0) != 0 || jmorph_key(0u, 1) != 0 || jmorph_key(0x80000000u, 1) != -1) return 7;  // +0 is key 0, -0 just below
    if (jmorph_pad(0, 0) != 0 || jmorph_pad(1, 0) != 0 || jmorph_pad(0, 1) != INT32_MAX || jmorph_pad(1, 1) != INT32_MIN) return 8;
    return 0;
}

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

// One channel of a tiny image: the decomposition against the brute force.
static int check_image(uint32_t W, uint32_t H, uint32_t rx, uint32_t ry, int dilate, int clamp, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh) {
    static const uint16_t special[] = {0x0000, 0x8000, 0x0001, 0x8001, 0x3c00, 0xbc00, 0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x7bff, 0xfbff};
    std::vector<int32_t> img((size_t)W * H);
    for (int32_t& k : img) {
        const uint32_t r = rnd();
        const uint16_t h = (r & 3u) == 0u ? special[(r >> 8) % 12u] : (uint16_t)(r >> 16);
        k = jmorph_key(f16_bits_to_f32_bits(h), dilate);
    }
    auto pick = [&](int32_t a, int32_t b) { return dilate ? std::max(a, b) : std::min(a, b); };
    const int32_t neutral = jmorph_neutral(dilate), pad = jmorph_pad(dilate, clamp);
    // brute force: every position of every window
    std::vector<int32_t> want((size_t)rw * rh);
    for (uint32_t oy = 0; oy < rh; oy++)
        for (uint32_t ox = 0; ox < rw; ox++) {
            int32_t acc = neutral;
            for (int64_t py = (int64_t)y + oy - ry; py <= (int64_t)y + oy + ry; py++)
                for (int64_t px = (int64_t)x + ox - rx; px <= (int64_t)x + ox + rx; px++)
                    acc = pick(acc, (px < 0 || py < 0 || px >= W || py >= H) ? pad : img[(size_t)py * W + (size_t)px]);
            want[(size_t)oy * rw + ox] = acc;
        }
    // the decomposition: planes of nv rows, of which [vlo, vhi) are rows of the image
    const uint32_t nv = (uint32_t)jmorph_plane_rows(rh, ry), row0 = y > ry ? y - ry : 0u;
    const uint32_t row1 = y + rh + ry < H ? y + rh + ry : H, vlo = row0 + ry - y, vhi = vlo + (row1 - row0);
    std::vector<int32_t> hp((size_t)nv * rw, 0x55555555), pp((size_t)nv * rw, 0x55555555), got((size_t)rw * rh);
    const uint32_t Lx = 2u * rx + 1u, Ly = 2u * ry + 1u;
    for (uint32_t row = row0; row < row1; row++) {  // rows: stage, double in place, two overlapping reads
        std::vector<int32_t> reg((size_t)rw + 2u * rx);
        for (uint32_t e = 0; e < reg.size(); e++) {
            const int64_t px = (int64_t)x + e - rx;
            reg[e] = (px < 0 || px >= W) ? pad : img[(size_t)row * W + (size_t)px];
        }
        uint32_t w = 1u, n = (uint32_t)reg.size();
        while (2u * w <= Lx) {
            n -= w;
            for (uint32_t i = 0; i < n; i++) reg[i] = pick(reg[i], reg[i + w]);
            w *= 2u;
        }
        for (uint32_t o = 0; o < rw; o++) hp[(size_t)(vlo + row - row0) * rw + o] = pick(reg[o], reg[o + Lx - w]);
    }
    auto plane_h = [&](uint32_t v, uint32_t c) { return (v < vlo || v >= vhi) ? pad : hp[(size_t)v * rw + c]; };
    for (uint32_t c = 0; c < rw; c++) {
        for (uint32_t v0 = 0; v0 < nv; v0 += Ly) {  // prefix of every block
            int32_t run = neutral;
            for (uint32_t v = v0; v < std::min(v0 + Ly, nv); v++) pp[(size_t)v * rw + c] = run = pick(run, plane_h(v, c));
        }
        for (uint32_t v0 = 0; v0 < rh; v0 += Ly) {  // suffix of the blocks that hold an output row, and the combination
            int32_t suf = neutral;
            for (uint32_t v = std::min(v0 + Ly, nv); v > v0; v--) {
                suf = pick(suf, plane_h(v - 1u, c));
                if (v - 1u < rh) got[(size_t)(v - 1u) * rw + c] = pick(suf, pp[(size_t)(v - 1u + Ly - 1u) * rw + c]);
            }
        }
    }
    return got == want ? 0 : 1;
}

int main() {
    if (int rc = check_descriptors()) { printf("descriptors: check %d failed\n", rc); return 1; }
    std::vector<uint32_t> widened;
    for (uint32_t h = 0; h < 65536u; h++) widened.push_back(f16_bits_to_f32_bits((uint16_t)h));
    if (int rc = check_order(widened)) { printf("key order over the f16 patterns: check %d failed\n", rc); return 1; }
    std::vector<uint32_t> products;
    for (int i = 0; i < 6000; i++) {  // colour times alpha: exact in binary32, Inf x 0 a NaN
        const uint32_t a = widened[rnd() & 0xffffu], b = widened[rnd() & 0xffffu];
        products.push_back(as_bits(as_float(a) * as_float(b)));
    }
    const uint32_t edge_pairs[][2] = {{0x7c00, 0x0000}, {0xfc00, 0x8000}, {0x0001, 0x0001}, {0x7bff, 0x7bff}, {0x8001, 0x0001}, {0x7bff, 0xfbff}};
    for (const auto& p : edge_pairs) products.push_back(as_bits(as_float(widened[p[0]]) * as_float(widened[p[1]])));
    if (int rc = check_order(products)) { printf("key order over products: check %d failed\n", rc); return 1; }
    int n = 0;
    struct Img { uint32_t W, H, rx, ry, x, y, rw, rh; };
    const Img imgs[] = {
        {1, 1, 0, 0, 0, 0, 1, 1},   {1, 1, 3, 2, 0, 0, 1, 1},    {7, 5, 1, 1, 0, 0, 7, 5},    {7, 5, 2, 0, 0, 0, 7, 5},   {7, 5, 0, 2, 0, 0, 7, 5},
        {7, 5, 9, 9, 0, 0, 7, 5},   {13, 11, 3, 4, 2, 3, 9, 5},  {13, 11, 1, 2, 12, 10, 1, 1}, {13, 29, 2, 3, 0, 0, 13, 29}, {5, 21, 0, 3, 1, 0, 3, 21},
        {5, 22, 1, 3, 0, 1, 5, 20}, {9, 20, 4, 1, 3, 7, 6, 13},  {4, 6, 255, 255, 0, 0, 4, 6}, {17, 9, 7, 8, 5, 2, 11, 6},  {17, 9, 8, 7, 0, 0, 17, 9},
    };
    for (const Img& im : imgs)
        for (int dilate = 0; dilate <= 1; dilate++)
            for (int clamp = 0; clamp <= 1; clamp++) {
                if (check_image(im.W, im.H, im.rx, im.ry, dilate, clamp, im.x, im.y, im.rw, im.rh)) {
                    printf("image %ux%u r %u,%u op %d clamp %d: the decomposition differs from the window\n", im.W, im.H, im.rx, im.ry, dilate, clamp);
                    return 1;
                }
                n++;
            }
    printf("ok: %zu + %zu values, %d images\n", widened.size(), products.size(), n);
    return 0;
}
