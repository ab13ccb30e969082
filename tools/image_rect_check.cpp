// image_rect_check.cpp -- include/jello_image.h and the scratch sizes of include/jello_blur.h and include/jello_resample.h exercised
// stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/image_rect_check.cpp -o /tmp/image_rect_check && /tmp/image_rect_check
//
// Three things.  (1) For every image height <= 12 and every y, rectangle height and radius <= 6 of a rectangle inside it: the row
// window, jblur_scratch_rows and jblur_scratch_bytes against a brute-force count of the image rows within the radius of the
// rectangle's, and against the formula jh_blur used to size the intermediate with before it called them (kept here as the expected
// value).  (2) jresample_scratch_bytes against source rows x destination columns x 16 over small extents.  (3) The rectangle check's
// three answers and the resolved rectangle: 0 x 0 is the whole image (of an image without texels too), a rectangle empty in one
// dimension, ends that touch the image's and pass it by one, and x + w or y + h beyond 32 bits.  Prints "ok" and returns 0.
#include <stdio.h>

#include <algorithm>

#include "jello_blur.h"
#include "jello_image.h"
#include "jello_resample.h"

static int check_rows() {
    long n = 0;
    for (uint32_t height = 0; height <= 12u; height++)
        for (uint32_t y = 0; y <= 6u; y++)
            for (uint32_t rect_h = 0; rect_h <= 6u; rect_h++)
                for (uint32_t radius = 0; radius <= 6u; radius++) {
                    if (y + rect_h > height) continue;  // (the callers have refused it)
                    // an image row counts when it lies within `radius` of a row of the rectangle; an empty rectangle's window is
                    // the rows within the radius of the gap at y, which nobody reads -- the functions are total, not the callers
                    uint32_t first = 0, count = 0;
                    for (uint32_t row = 0; row < height; row++) {
                        const bool near = (int64_t)row >= (int64_t)y - (int64_t)radius && (int64_t)row < (int64_t)y + rect_h + radius;
                        if (near && count++ == 0u) first = row;
                    }
                    const jimage_rows got = jimage_row_window(y, rect_h, radius, height);
                    if (got.n_rows != count || (count != 0u && got.row0 != first)) return 1;
                    const uint64_t old_rows = std::min<uint64_t>(height, (uint64_t)y + rect_h + radius) - (y > radius ? y - radius : 0u);  // jh_blur's own line, before
                    if (got.n_rows != old_rows) return 2;
                    for (uint32_t rect_w = 0; rect_w <= 5u; rect_w++)
                        for (uint32_t x = 0; x <= 2u; x++) {
                            const jimage_rect r = {x, y, rect_w, rect_h};
                            const jimage_rows rows = jblur_scratch_rows(r, radius, height);
                            if (rows.row0 != got.row0 || rows.n_rows != count) return 3;
                            if (jblur_scratch_bytes(r, radius, height) != (uint64_t)count * rect_w * 16u) return 4;
                            if (jblur_scratch_bytes(r, radius, height) != old_rows * rect_w * 16u) return 5;
                            n++;
                        }
                }
    // at the limits nothing wraps: the last row of the tallest image, the largest radius a call has
    const jimage_rows top = jimage_row_window(0xfffffffeu, 1u, 255u, 0xffffffffu);
    if (top.row0 != 0xfffffffeu - 255u || top.n_rows != 256u) return 6;
    if (jblur_scratch_bytes({0u, 0xfffffff0u, 0xffffffffu, 15u}, 192u, 0xffffffffu) != 207ull * 0xffffffffull * 16u) return 7;  // (above 2^32 bytes)
    return n > 0 ? 0 : 8;
}

static int check_resample() {
    for (uint32_t sh = 0; sh <= 9u; sh++)
        for (uint32_t dw = 0; dw <= 9u; dw++)
            for (uint32_t other = 1; other <= 3u; other++) {
                const jimage_rect s = {other, 2u, other + 4u, sh}, d = {1u, other, dw, other + 7u};
                if (jresample_scratch_rows(s) != sh) return 1;
                if (jresample_scratch_bytes(s, d) != (uint64_t)sh * dw * 16u) return 2;
            }
    if (jresample_scratch_bytes({0u, 0u, 1u, 0xffffffffu}, {0u, 0u, 4096u, 1u}) != 0xffffffffull * 4096u * 16u) return 3;  // (above 2^32 bytes)
    return 0;
}

static bool same(jimage_rect a, jimage_rect b) { return a.x == b.x && a.y == b.y && a.w == b.w && a.h == b.h; }

static int check_rects() {
    const uint32_t W = 40u, H = 24u, M = 0xffffffffu;
    struct Case { jimage_rect named; int want; };
    const Case cases[] = {
        {{0, 0, 0, 0}, JIMAGE_RECT_OK},         {{99, 99, 0, 0}, JIMAGE_RECT_OK},       {{M, M, 0, 0}, JIMAGE_RECT_OK},  // 0 x 0: the whole image, x and y ignored
        {{0, 0, W, H}, JIMAGE_RECT_OK},         {{3, 5, 1, 1}, JIMAGE_RECT_OK},         {{W - 1, H - 1, 1, 1}, JIMAGE_RECT_OK},
        {{7, 0, W - 7, H}, JIMAGE_RECT_OK},     {{0, 9, W, H - 9}, JIMAGE_RECT_OK},
        {{2, 2, 0, 4}, JIMAGE_RECT_HALF_EMPTY}, {{2, 2, 4, 0}, JIMAGE_RECT_HALF_EMPTY}, {{M, M, 0, 1}, JIMAGE_RECT_HALF_EMPTY},
        {{8, 0, W - 7, 4}, JIMAGE_RECT_OUTSIDE}, {{0, 9, 4, H - 8}, JIMAGE_RECT_OUTSIDE}, {{0, 0, W + 1, H}, JIMAGE_RECT_OUTSIDE},
        {{0, 0, W, H + 1}, JIMAGE_RECT_OUTSIDE}, {{W, 0, 1, 1}, JIMAGE_RECT_OUTSIDE},     {{0, H, 1, 1}, JIMAGE_RECT_OUTSIDE},
        {{M, 0, 2, 2}, JIMAGE_RECT_OUTSIDE},     {{0, M, 2, 2}, JIMAGE_RECT_OUTSIDE},     {{1, 0, M, 1}, JIMAGE_RECT_OUTSIDE},  // x + w, y + h beyond 32 bits
        {{M, M, M, M}, JIMAGE_RECT_OUTSIDE},
    };
    for (const Case& c : cases) {
        const int got = jimage_rect_check(c.named, W, H);
        if (got != c.want) return 1;
        if (got != JIMAGE_RECT_OK) continue;
        const jimage_rect r = jimage_resolve(c.named, W, H);
        const bool whole = c.named.w == 0u && c.named.h == 0u;
        if (!same(r, whole ? jimage_rect{0u, 0u, W, H} : c.named)) return 3;
        if (jimage_rect_empty(r) || !jimage_rect_inside(r, W, H)) return 4;
    }
    // an image without texels: its whole is legal and empty; a rectangle with texels is outside it
    const uint32_t no_texels[][2] = {{0u, 0u}, {0u, 5u}, {5u, 0u}};
    for (const auto& size : no_texels) {
        if (jimage_rect_check({0, 0, 0, 0}, size[0], size[1]) != JIMAGE_RECT_OK) return 5;
        if (!jimage_rect_empty(jimage_resolve({3, 3, 0, 0}, size[0], size[1]))) return 6;
        if (jimage_rect_check({0, 0, 1, 1}, size[0], size[1]) != JIMAGE_RECT_OUTSIDE) return 7;
    }
    // the largest image: its last texel is inside, nothing wraps
    if (jimage_rect_check({M - 1u, M - 1u, 1, 1}, M, M) != JIMAGE_RECT_OK || jimage_rect_check({M, 0, 1, 1}, M, M) != JIMAGE_RECT_OUTSIDE) return 8;
    if (jimage_rect_inside({M, M, 0, 0}, M, M) != true || jimage_rect_inside({M, M, 1, 0}, M, M) != false) return 9;
    return 0;
}

int main() {
    if (int rc = check_rows()) { printf("row window and blur scratch: check %d failed\n", rc); return 1; }
    if (int rc = check_resample()) { printf("resample scratch: check %d failed\n", rc); return 1; }
    if (int rc = check_rects()) { printf("rectangles: check %d failed\n", rc); return 1; }
    printf("ok\n");
    return 0;
}
