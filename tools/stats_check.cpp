// stats_check.cpp -- include/jello_stats.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/stats_check.cpp -o /tmp/stats_check && /tmp/stats_check
//
// Four things.  (1) jstats_desc_error and jstats_plan over legal descriptors -- every subset of what, channel, population, transfer --
// and over illegal ones, on both sides of every boundary (2^31 texels legal, one more refused), the plan untouched on a refusal.
// (2) The 16-bit key: all 63 490 non-NaN patterns walked in key order see jmorph_key of the widened value rise strictly, under either
// operator; unkey inverts key; no key lies beyond the neutral elements.  The codes: LINEAR against the binary64 product rounded
// half-even, SRGB against a linear count of the thresholds, over all 65 536 patterns.  (3) The record as kernels_stats.hip makes it,
// built from the header's pieces -- the rectangle's texels dealt to P partials, each starting from jstats_word_neutral and taking a
// texel by jstats_word_combine, the partials combined, the words through jstats_record_word / jstats_record_bin -- in exactly sized
// arrays, against a brute-force loop that knows nothing of partials or keys (float comparisons and the sign bit), on images up to
// 12 x 12, whole images and rectangles, every what x population x transfer.  (4) The combine over EVERY split of a list of 8 items
// into 1..5 contiguous partials, combined forwards and backwards: one record.  Prints "ok" and returns 0.
//
// With arguments -- W H what channel threshold population transfer x y w h BITS, BITS a string of W * H * 4 f16 patterns of four hex
// digits, texel by texel -- it prints the record of that rectangle (P = 3), its uint32_t words one to a line.
// tests/test_stats_spec.py compares that with tests/stats_ref.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jello_morph.h"
#include "jello_stats.h"

#define JSRGB_ENCODE_TABLE static const
#include "../jello_amd/csrc/srgb_encode_lut.h"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static const uint32_t kRecordWords = sizeof(jh_stats_record) / 4u;

struct Image {
    uint32_t W, H;
    std::vector<uint16_t> bits;  // W * H * 4
    uint16_t at(uint32_t x, uint32_t y, uint32_t c) const { return bits.at(((size_t)y * W + x) * 4u + c); }
};

// One texel into a partial: its own one-texel partial, word by word, combined in.
static void take(std::vector<uint32_t>& p, const Image& im, const jh_stats_desc& d, uint32_t x, uint32_t y) {
    const bool content = jstats_is_content(im.at(x, y, (uint32_t)d.channel), d.threshold);
    const bool in_pop = d.population == JSTATS_ALL || content;
    std::vector<uint32_t> t(JSTATS_PARTIAL_WORDS);
    for (uint32_t i = 0; i < t.size(); i++) t[i] = jstats_word_neutral(i);
    if (content) {
        t[JSTATS_W_CONTENT] = 1u;
        t[JSTATS_W_X0] = x; t[JSTATS_W_Y0] = y; t[JSTATS_W_X1] = x + 1u; t[JSTATS_W_Y1] = y + 1u;
    }
    if (in_pop) {
        t[JSTATS_W_POP] = 1u;
        for (uint32_t c = 0; c < 4u; c++) {
            const uint16_t h = im.at(x, y, c);
            if (jstats_is_nan(h)) t[JSTATS_W_NAN + c] = 1u;
            else t[JSTATS_W_MIN + c] = t[JSTATS_W_MAX + c] = jstats_key(h);
            t[JSTATS_W_HIST + 256u * c + jstats_code(d.transfer, c, h, kSrgbEncodeThreshold)] = 1u;
        }
    }
    for (uint32_t i = 0; i < p.size(); i++) p[i] = jstats_word_combine(i, p[i], t[i]);
}

static std::vector<uint32_t> neutral() {
    std::vector<uint32_t> p(JSTATS_PARTIAL_WORDS);
    for (uint32_t i = 0; i < p.size(); i++) p[i] = jstats_word_neutral(i);
    return p;
}

static std::vector<uint32_t> finish(const std::vector<std::vector<uint32_t>>& partials, const jstats_head& hd, bool backwards) {
    std::vector<uint32_t> all = neutral();
    for (size_t k = 0; k < partials.size(); k++) {
        const std::vector<uint32_t>& p = partials[backwards ? partials.size() - 1u - k : k];
        for (uint32_t i = 0; i < all.size(); i++) all[i] = jstats_word_combine(i, all[i], p[i]);
    }
    std::vector<uint32_t> rec(kRecordWords);
    for (uint32_t j = 0; j < JSTATS_RECORD_HEAD_WORDS; j++) rec[j] = jstats_record_word(j, hd, all.data());
    for (uint32_t i = 0; i < 1024u; i++) rec[JSTATS_RECORD_HEAD_WORDS + i] = jstats_record_bin(hd, all[JSTATS_W_HIST + i]);
    return rec;
}

// The record of the rectangle r of im, its texels dealt to P partials round robin.
static std::vector<uint32_t> pieces(const Image& im, const jh_stats_desc& d, jimage_rect r, uint32_t P) {
    std::vector<std::vector<uint32_t>> partials(P, neutral());
    uint32_t n = 0;
    for (uint32_t y = r.y; y < r.y + r.h; y++)
        for (uint32_t x = r.x; x < r.x + r.w; x++) take(partials[n++ % P], im, d, x, y);
    const jstats_head hd = {r.x, r.y, r.w, r.h, d.what, (uint32_t)d.population, (uint32_t)d.transfer};
    return finish(partials, hd, false);
}

static bool below(float a, float b) {  // totalOrder on non-NaN values, by comparisons and the sign bit
    if (a < b) return true;
    if (a > b) return false;
    return signbit(a) && !signbit(b);
}
static uint32_t brute_code(int transfer, uint32_t c, uint16_t h) {
    const float v = jstats_f16(h);
    double q = v != v ? 0.0 : (double)v;
    q = q > 0.0 ? q : 0.0;
    q = q < 1.0 ? q : 1.0;
    if (transfer == JSTATS_SRGB && c != 3u) {
        uint32_t n = 0;
        for (uint32_t k = 0; k < 255u; k++) n += (double)kSrgbEncodeThreshold[k] <= q ? 1u : 0u;
        return n;
    }
    return (uint32_t)nearbyint(q * 255.0);  // (the default rounding mode: half-even)
}
static jh_stats_record brute(const Image& im, const jh_stats_desc& d, jimage_rect r) {
    jh_stats_record rec;
    memset(&rec, 0, sizeof rec);
    rec.x = r.x; rec.y = r.y; rec.width = r.w; rec.height = r.h;
    rec.what = d.what; rec.population = (uint32_t)d.population; rec.transfer = (uint32_t)d.transfer;
    if (r.w == 0u || r.h == 0u) return rec;
    const bool counts = (d.what & (JSTATS_EXTREMES | JSTATS_HISTOGRAM)) != 0u;
    bool any[4] = {false, false, false, false};
    float lo[4], hi[4];
    uint16_t lo_bits[4] = {0x7c00, 0x7c00, 0x7c00, 0x7c00}, hi_bits[4] = {0xfc00, 0xfc00, 0xfc00, 0xfc00};
    for (uint32_t y = r.y; y < r.y + r.h; y++)
        for (uint32_t x = r.x; x < r.x + r.w; x++) {
            const float cv = jstats_f16(im.at(x, y, (uint32_t)d.channel));
            const bool content = cv >= d.threshold;
            if (content) {
                if ((d.what & JSTATS_BOUNDS) != 0u) {
                    if (rec.content_count == 0u) { rec.bounds[0] = x; rec.bounds[1] = y; rec.bounds[2] = x + 1u; rec.bounds[3] = y + 1u; }
                    rec.bounds[0] = std::min(rec.bounds[0], x); rec.bounds[1] = std::min(rec.bounds[1], y);
                    rec.bounds[2] = std::max(rec.bounds[2], x + 1u); rec.bounds[3] = std::max(rec.bounds[3], y + 1u);
                }
                rec.content_count++;
            }
            if (!counts || !(d.population == JSTATS_ALL || content)) continue;
            rec.population_count++;
            for (uint32_t c = 0; c < 4u; c++) {
                const uint16_t h = im.at(x, y, c);
                const float v = jstats_f16(h);
                if (v != v) rec.nan_count[c]++;
                else {
                    if (!any[c] || below(v, lo[c])) { lo[c] = v; lo_bits[c] = h; }
                    if (!any[c] || below(hi[c], v)) { hi[c] = v; hi_bits[c] = h; }
                    any[c] = true;
                }
                if ((d.what & JSTATS_HISTOGRAM) != 0u) rec.histogram[c][brute_code(d.transfer, c, h)]++;
            }
        }
    if ((d.what & JSTATS_EXTREMES) != 0u)
        for (uint32_t c = 0; c < 4u; c++) { rec.min_bits[c] = lo_bits[c]; rec.max_bits[c] = hi_bits[c]; }
    return rec;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static const uint16_t kValues[] = {0x0000, 0x8000, 0x0001, 0x8001, 0x3800, 0x3c00, 0x4000, 0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x3400,
                                   0x3bff, 0x3c01, 0x1c04, 0x1804, 0x37ff, 0x3801, 0xbc00, 0x2e66, 0x7bff, 0xfbff};

static Image random_image(uint32_t W, uint32_t H) {
    Image im{W, H, std::vector<uint16_t>((size_t)W * H * 4u)};
    for (uint16_t& b : im.bits) b = (rnd() >> 8) % 3u == 0u ? (uint16_t)(rnd() >> 16) : kValues[(rnd() >> 8) % (sizeof kValues / sizeof kValues[0])];
    return im;
}

static void check_legality() {
    jh_stats_desc d = {JSTATS_BOUNDS, 3, 0.5f, JSTATS_ALL, JSTATS_LINEAR, 0, 0, 0, 0};
    jh_stats_plan_t plan;
    for (uint32_t what = 1; what < 8u; what++)
        for (int ch = 0; ch < 4; ch++)
            for (int pop = 0; pop < 2; pop++)
                for (int tr = 0; tr < 2; tr++) {
                    jh_stats_desc l = d;
                    l.what = what; l.channel = ch; l.population = pop; l.transfer = tr;
                    CHECK(jstats_desc_error(&l) == nullptr);
                    CHECK(jstats_plan(&l, 100, 50, &plan) == nullptr && plan.width == 100u && plan.height == 50u && plan.launches == 2u &&
                          plan.record_bytes == sizeof(jh_stats_record) && plan.scratch_bytes == (uint64_t)JSTATS_MAX_PARTIALS * JSTATS_PARTIAL_BYTES);
                }
    CHECK(jstats_plan(&d, 0, 0, &plan) == nullptr && plan.launches == 1u && plan.scratch_bytes == 0u);
    const jh_stats_plan_t untouched = {1, 2, 3, 4, 5, 6, 7, 8};
    auto refused = [&](jh_stats_desc bad, uint32_t w, uint32_t h) {
        plan = untouched;
        CHECK(jstats_plan(&bad, w, h, &plan) != nullptr);
        CHECK(memcmp(&plan, &untouched, sizeof plan) == 0);
    };
    jh_stats_desc b;
    b = d; b.what = 0u; refused(b, 10, 10);
    b = d; b.what = 8u; refused(b, 10, 10);
    b = d; b.what = 0x80000001u; refused(b, 10, 10);
    b = d; b.channel = -1; refused(b, 10, 10);
    b = d; b.channel = 4; refused(b, 10, 10);
    b = d; b.population = 2; refused(b, 10, 10);
    b = d; b.population = -1; refused(b, 10, 10);
    b = d; b.transfer = 2; refused(b, 10, 10);
    b = d; b.transfer = -1; refused(b, 10, 10);
    b = d; b.threshold = INFINITY; refused(b, 10, 10);
    b = d; b.threshold = -INFINITY; refused(b, 10, 10);
    b = d; b.threshold = NAN; refused(b, 10, 10);
    b = d; b.x = 9; b.y = 9; b.width = 2; b.height = 1; refused(b, 10, 10);
    b = d; b.x = 0; b.y = 0; b.width = 10; b.height = 11; refused(b, 10, 10);
    b = d; b.x = 2; b.y = 2; b.width = 0; b.height = 4; refused(b, 10, 10);
    b = d; b.x = 2; b.y = 2; b.width = 4; b.height = 0; refused(b, 10, 10);
    b = d; b.x = 0xffffffffu; b.width = 2; b.height = 2; refused(b, 10, 10);
    b = d; b.x = 9; b.y = 9; b.width = 1; b.height = 1; CHECK(jstats_plan(&b, 10, 10, &plan) == nullptr && plan.x == 9u);
    b = d; b.threshold = -3.0e38f; CHECK(jstats_plan(&b, 10, 10, &plan) == nullptr);
    // 2^31 texels legal, one more refused: descriptor arithmetic only
    CHECK(jstats_plan(&d, 65536, 32768, &plan) == nullptr && plan.width == 65536u);
    CHECK(jstats_plan(&d, 0x80000000u, 1, &plan) == nullptr);
    refused(d, 0x80000001u, 1);
    refused(d, 1, 0x80000001u);
    refused(d, 65536, 32769);
    b = d; b.width = 0x80000000u; b.height = 1; CHECK(jstats_plan(&b, 0x80000001u, 1, &plan) == nullptr);
}

static void check_keys_and_codes() {
    std::vector<uint32_t> order;
    for (uint32_t h = 0; h < 65536u; h++)
        if (!jstats_is_nan(h)) order.push_back(h);
    CHECK(order.size() == 63490u);
    std::sort(order.begin(), order.end(), [](uint32_t a, uint32_t b) { return jstats_key(a) < jstats_key(b); });
    for (size_t i = 0; i < order.size(); i++) {
        const uint32_t h = order[i];
        CHECK(jstats_unkey(jstats_key(h)) == h && jstats_key(h) <= 0xffffu);
        CHECK(jstats_key(h) <= JSTATS_KEY_MIN_NEUTRAL && jstats_key(h) >= JSTATS_KEY_MAX_NEUTRAL);
        if (i == 0) continue;
        const float a = jstats_f16((uint16_t)order[i - 1]), b = jstats_f16((uint16_t)h);
        uint32_t ab, bb;
        memcpy(&ab, &a, 4);
        memcpy(&bb, &b, 4);
        CHECK(jmorph_key(ab, 0) < jmorph_key(bb, 0) && jmorph_key(ab, 1) < jmorph_key(bb, 1));
        CHECK(below(a, b));
    }
    CHECK(order.front() == 0xfc00u && order.back() == 0x7c00u);
    CHECK(jstats_unkey(JSTATS_KEY_MIN_NEUTRAL) == 0x7c00u && jstats_unkey(JSTATS_KEY_MAX_NEUTRAL) == 0xfc00u);
    CHECK(jstats_key(0x8000u) + 1u == jstats_key(0x0000u));
    for (uint32_t h = 0; h < 65536u; h++)
        for (int tr = 0; tr < 2; tr++)
            for (uint32_t c = 2; c < 4u; c++) {
                const uint32_t code = jstats_code(tr, c, (uint16_t)h, kSrgbEncodeThreshold);
                CHECK(code < 256u && code == brute_code(tr, c, (uint16_t)h));
            }
}

static void check_records() {
    uint32_t n = 0;
    for (uint32_t W = 1; W <= 12u; W += (W < 4u ? 1u : 4u))
        for (uint32_t H = 1; H <= 12u; H += (H < 3u ? 1u : 9u)) {
            const Image im = random_image(W, H);
            const jimage_rect rects[] = {{0, 0, W, H}, {W / 2u, H / 2u, W - W / 2u, H - H / 2u}, {W / 3u, 0, 1, H}, {W - 1u, H - 1u, 1, 1}};
            for (const jimage_rect& r : rects)
                for (uint32_t what = 1; what < 8u; what++)
                    for (int pop = 0; pop < 2; pop++)
                        for (int tr = 0; tr < 2; tr++) {
                            const float thresholds[] = {0.0f, -0.0f, 0.5f, 5.9604645e-8f, 7.0e4f, -1.0f};
                            const jh_stats_desc d = {what, (int)(n % 4u), thresholds[n % 6u], pop, tr, r.x, r.y, r.w, r.h};
                            const jh_stats_record want = brute(im, d, r);
                            for (uint32_t P : {1u, 2u, 5u}) {
                                const std::vector<uint32_t> got = pieces(im, d, r, P);
                                CHECK(got.size() * 4u == sizeof want && memcmp(got.data(), &want, sizeof want) == 0);
                            }
                            n++;
                        }
        }
    // an image without texels: the header and zeros
    const Image none{0, 0, {}};
    const jh_stats_desc d = {7u, 3, 0.5f, JSTATS_CONTENT, JSTATS_SRGB, 0, 0, 0, 0};
    const std::vector<uint32_t> got = pieces(none, d, {0, 0, 0, 0}, 1);
    const jh_stats_record want = brute(none, d, {0, 0, 0, 0});
    CHECK(memcmp(got.data(), &want, sizeof want) == 0 && got[4] == 7u && got[5] == 1u && got[6] == 1u);
    for (uint32_t j = 8; j < kRecordWords; j++) CHECK(got[j] == 0u);
    printf("ok: %u records from the pieces", n);
}

static void check_splits() {
    const Image im = random_image(8, 1);
    const jh_stats_desc d = {7u, 1, 0.0f, JSTATS_CONTENT, JSTATS_SRGB, 0, 0, 0, 0};
    const jstats_head hd = {0, 0, 8, 1, d.what, (uint32_t)d.population, (uint32_t)d.transfer};
    const jh_stats_record want = brute(im, d, {0, 0, 8, 1});
    uint32_t splits = 0;
    for (uint32_t cuts = 0; cuts < 128u; cuts++) {  // bit i: a cut between item i and item i + 1
        const uint32_t parts = (uint32_t)__builtin_popcount(cuts) + 1u;
        if (parts > 5u) continue;
        std::vector<std::vector<uint32_t>> partials(1, neutral());
        for (uint32_t x = 0; x < 8u; x++) {
            take(partials.back(), im, d, x, 0);
            if (x < 7u && (cuts >> x & 1u)) partials.push_back(neutral());
        }
        CHECK(partials.size() == parts);
        for (bool backwards : {false, true}) {
            const std::vector<uint32_t> got = finish(partials, hd, backwards);
            CHECK(memcmp(got.data(), &want, sizeof want) == 0);
        }
        splits++;
    }
    CHECK(splits == 99u);
    printf(", %u splits\n", splits);
}

int main(int argc, char** argv) {
    static_assert(sizeof(jh_stats_record) == 4u * (JSTATS_RECORD_HEAD_WORDS + 1024u), "the record's words");
    if (argc == 13) {
        Image im{(uint32_t)atoi(argv[1]), (uint32_t)atoi(argv[2]), {}};
        const jh_stats_desc d = {(uint32_t)atoi(argv[3]), atoi(argv[4]), strtof(argv[5], nullptr), atoi(argv[6]), atoi(argv[7]),
                                 (uint32_t)atoi(argv[8]), (uint32_t)atoi(argv[9]), (uint32_t)atoi(argv[10]), (uint32_t)atoi(argv[11])};
        const size_t n = (size_t)im.W * im.H * 4u;
        if (strlen(argv[12]) != 4u * n) return 2;
        for (size_t i = 0; i < n; i++) {
            char word[5] = {argv[12][4 * i], argv[12][4 * i + 1], argv[12][4 * i + 2], argv[12][4 * i + 3], 0};
            im.bits.push_back((uint16_t)strtoul(word, nullptr, 16));
        }
        jimage_rect r;
        if (jstats_desc_error(&d) || jstats_rect_error(&d, im.W, im.H, &r)) return 3;
        for (uint32_t word : pieces(im, d, r, 3)) printf("%u\n", word);
        return 0;
    }
    check_legality();
    check_keys_and_codes();
    check_records();
    check_splits();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    return 0;
}
