// lut3d_check.cpp -- include/jello_lut3d.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/lut3d_check.cpp -o /tmp/lut3d_check && /tmp/lut3d_check
//
// Four things.  (1) The position: for every f16 bit pattern and every N = 2..65, k lies in [0, N - 2], f in [0, 1], and k + f is
// the clamped value times N - 1 exactly (in binary64, where every quantity is exact).  (2) The walk against a brute-force
// barycentric solve on N = 2..5: for every texel of a lattice of inputs (sixteenths, ties of every kind among them) the six
// tetrahedra of the cell -- the six orders of the axes -- are tried, the ones with no negative coordinate are the candidates, and the
// header's vertices and weights must be those of the FIRST candidate in the order (r, g, b) < (r, b, g) < (g, r, b) < ... -- the
// stable sort; the weights sum to 1 and sum w_i V_i is the position, exactly.  (3) jlut_texel over tables in heap arrays of exactly
// n^3 entries (a read past an end is an AddressSanitizer report): an identity table of a power-of-two N - 1 returns the clamped input,
// a constant table of powers of two its colour (every partial sum is then exact), alpha is copied.  (4) jlut_check and
// jlut_image_error from both sides of 2 and 65.  Prints "ok ..." and returns 0.
//
// With arguments -- N LUTHEX TEXELHEX, the table's 4 N^3 and the texels' 4 K f16 bit patterns, four hex digits each -- it prints the K
// texels of the rule, one line "rrrr gggg bbbb aaaa" each.  tests/test_lut3d_spec.py compares that with tests/lut3d_ref.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jello_lut3d.h"

static int failures = 0;
#define CHECK(c)                                   \
    do {                                           \
        if (!(c)) {                                \
            failures++;                            \
            if (failures < 20) printf("line %d: %s\n", __LINE__, #c); \
        }                                          \
    } while (0)

static uint64_t check_positions() {
    uint64_t count = 0;
    for (uint32_t n = JLUT_MIN_SIZE; n <= JLUT_MAX_SIZE; n++)
        for (uint32_t h = 0; h < 65536u; h++) {
            uint32_t k;
            float f;
            jlut_position(h, n - 1u, &k, &f);
            double c = jcolor_f16_value(h);
            c = c > 0.0 ? c : 0.0;
            c = c < 1.0 ? c : 1.0;
            CHECK(k <= n - 2u && f >= 0.0f && f <= 1.0f);
            CHECK((double)k + (double)f == c * (double)(n - 1u));  // (both sides exact in binary64)
            CHECK((double)(1.0f - f) == 1.0 - (double)f);
            count++;
        }
    return count;
}

static uint64_t check_walk() {
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    uint64_t count = 0;
    for (uint32_t n = 2u; n <= 5u; n++) {
        const uint32_t steps = 16u * (n - 1u);  // inputs j / steps: every sixteenth of every cell
        for (uint32_t a = 0; a <= steps; a++)
            for (uint32_t b = 0; b <= steps; b++)
                for (uint32_t c = 0; c <= steps; c++) {
                    const uint32_t lattice[3] = {a, b, c};
                    uint16_t h[3];
                    bool exact = true;
                    for (int i = 0; i < 3; i++) {
                        h[i] = jcolor_f16_bits((double)lattice[i] / (double)steps);
                        exact = exact && jcolor_f16_value(h[i]) * (double)steps == (double)lattice[i];
                    }
                    if (!exact) continue;  // (thirds are no f16: N = 4 keeps the inputs that are)
                    uint32_t index[4];
                    float w[4];
                    jlut_vertices((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2], n, index, w);
                    // the position in table coordinates, the cell and the fractions, in binary64
                    double p[3], fr[3];
                    uint32_t k[3];
                    for (int i = 0; i < 3; i++) {
                        p[i] = (double)lattice[i] / 16.0;
                        k[i] = std::min((uint32_t)p[i], n - 2u);
                        fr[i] = p[i] - (double)k[i];
                    }
                    int chosen = -1;
                    for (int q = 0; q < 6 && chosen < 0; q++) {  // barycentric coordinates in the tetrahedron of this order
                        const double bc[4] = {1.0 - fr[perms[q][0]], fr[perms[q][0]] - fr[perms[q][1]], fr[perms[q][1]] - fr[perms[q][2]], fr[perms[q][2]]};
                        if (bc[0] >= 0.0 && bc[1] >= 0.0 && bc[2] >= 0.0 && bc[3] >= 0.0) chosen = q;
                    }
                    CHECK(chosen >= 0);
                    if (chosen < 0) continue;
                    uint32_t v[3] = {k[0], k[1], k[2]};
                    double sum_w = 0.0, sum_p[3] = {0.0, 0.0, 0.0};
                    for (int i = 0; i < 4; i++) {
                        if (i > 0) v[perms[chosen][i - 1]]++;
                        CHECK(index[i] == v[0] + n * (v[1] + n * v[2]));
                        CHECK(index[i] < n * n * n && w[i] >= 0.0f);
                        sum_w += (double)w[i];
                        for (int d = 0; d < 3; d++) sum_p[d] += (double)w[i] * (double)v[d];
                    }
                    CHECK(sum_w == 1.0 && sum_p[0] == p[0] && sum_p[1] == p[1] && sum_p[2] == p[2]);
                    count++;
                }
    }
    return count;
}

static uint64_t check_texels() {
    uint64_t count = 0;
    for (uint32_t n : {2u, 3u, 5u, 9u, 17u, 33u, 65u}) {
        std::vector<uint16_t> table(4u * (size_t)n * n * n), flat(4u * (size_t)n * n * n);  // exactly n^3 entries each
        jlut_identity(n, table.data());
        for (size_t i = 0; i < flat.size(); i += 4u) { flat[i] = 0x3800u; flat[i + 1u] = 0x3400u; flat[i + 2u] = 0x3c00u; flat[i + 3u] = 0x7e00u; }
        for (uint32_t h = 0; h < 65536u; h += (n < 17u ? 1u : 7u)) {
            const uint16_t in[4] = {(uint16_t)h, (uint16_t)(h * 40503u + 12345u), (uint16_t)(h * 25173u + 13849u), (uint16_t)(h * 0x9E37u + 0x79B9u)};
            uint16_t out[4], want[4];
            jlut_texel(n, table.data(), in, out);
            for (int c = 0; c < 3; c++) {
                const double v = jcolor_f16_value(in[c]);
                want[c] = (v != v || v <= 0.0) ? 0u : (v >= 1.0 ? 0x3c00u : in[c]);
            }
            CHECK(out[0] == want[0] && out[1] == want[1] && out[2] == want[2] && out[3] == in[3]);
            jlut_texel(n, flat.data(), in, out);
            CHECK(out[0] == 0x3800u && out[1] == 0x3400u && out[2] == 0x3c00u && out[3] == in[3]);  // (a power of two times 1 - f is exact: every partial sum is)
            count++;
        }
    }
    return count;
}

static void check_legality() {
    CHECK(jlut_check(1u, 0u) && !jlut_check(2u, 0u) && !jlut_check(65u, 0u) && jlut_check(66u, 0u) && jlut_check(0u, 0u) && jlut_check(0xffffffffu, 0u));
    CHECK(jlut_check(17u, 1u) && jlut_check(17u, 0x80000000u) && !jlut_check(17u, 0u));
    CHECK(strcmp(jlut_check(1u, 0u), "size outside 2..65") == 0 && strcmp(jlut_check(2u, 2u), "unknown flag bits") == 0);
    CHECK(!jlut_image_error(2u, 2u, 4u) && jlut_image_error(2u, 2u, 5u) && jlut_image_error(2u, 3u, 4u) && jlut_image_error(2u, 4u, 2u));
    CHECK(!jlut_image_error(65u, 65u, 4225u) && jlut_image_error(65u, 65u, 4224u) && jlut_image_error(65u, 64u, 4225u));
    uint16_t none[4] = {1, 2, 3, 4};
    CHECK(jlut_identity_query(1u, none) && jlut_identity_query(66u, none) && jlut_texels(1u, none, none, 1u, none) && jlut_texels(66u, none, none, 1u, none));
    CHECK(none[0] == 1 && none[1] == 2 && none[2] == 3 && none[3] == 4);
}

static bool parse_hex(const char* s, std::vector<uint16_t>& out) {
    const size_t len = strlen(s);
    if (len % 4u) return false;
    out.resize(len / 4u);  // exactly what was given
    for (size_t i = 0; i < out.size(); i++) {
        unsigned v;
        char four[5] = {s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3], 0};
        if (sscanf(four, "%x", &v) != 1) return false;
        out[i] = (uint16_t)v;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc == 4) {
        const uint32_t n = (uint32_t)strtoul(argv[1], nullptr, 10);
        std::vector<uint16_t> table, in;
        if (jlut_check(n, 0u) || !parse_hex(argv[2], table) || !parse_hex(argv[3], in) || table.size() != 4u * (size_t)n * n * n || in.size() % 4u) {
            printf("usage: lut3d_check N LUTHEX TEXELHEX\n");
            return 2;
        }
        std::vector<uint16_t> out(in.size());
        if (jlut_texels(n, table.data(), in.data(), in.size() / 4u, out.data())) return 2;
        for (size_t i = 0; i < out.size(); i += 4u) printf("%04x %04x %04x %04x\n", out[i], out[i + 1u], out[i + 2u], out[i + 3u]);
        return 0;
    }
    const uint64_t positions = check_positions(), walks = check_walk(), texels = check_texels();
    check_legality();
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok: %llu positions, %llu walks, %llu texels\n", (unsigned long long)positions, (unsigned long long)walks, (unsigned long long)texels);
    return 0;
}
