// turbulence_check.cpp -- include/jello_turbulence.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/turbulence_check.cpp -o /tmp/turbulence_check && /tmp/turbulence_check
//
// Five things.  (1) The generator against Schrage-free 64-bit arithmetic (16807 s mod (2^31 - 1)) over 20 000 steps from several
// seeds, setup_seed on the int32 corners, and the published check value: from seed 1 the 10 000th number is 1043618065.  (2) The tables
// of a set of seeds on heap arrays of exactly 256 bytes and 2048 floats: P is a permutation; every gradient has unit length to a
// binary32 ULP or is exactly (+0, +0); the device layout is a permutation of the same values.  (3) The plan against __int128 and long
// double: step and start within half a unit of the product, max_extent the last extent inside the range and max_extent + 1 outside it.
// (4) Legality from both sides: every boundary of jturb_desc_error and jturb_plan with a descriptor just inside and one just outside,
// each refusal with the text it has to answer.  (5) The masked lattice lookup equals the specification's duplicated-table lookup --
// uLatticeSelector and fGradient of 514 entries, indexed without a mask -- for every (bx0, by0) of the 256 x 256 lattice.
// Prints "ok" and returns 0.
//
//     turbulence_check texels KIND OCTAVES SEED STITCH FX FY TX TY TW TH OX OY X Y W H
//
// prints the binary32 bit patterns (8 hex digits each, r g b a) of jturb_texel for the W x H texels from (X, Y), one texel per line:
// the rule's host half evaluated on the CPU, which tests/test_turbulence_spec.py compares with tests/turbulence_ref.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jello_turbulence.h"

static bool says(const char* got, const char* want) { return want ? (got && strstr(got, want)) : got == nullptr; }
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);               \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static jh_turbulence_desc legal() {
    jh_turbulence_desc d;
    memset(&d, 0, sizeof d);
    d.kind = JTURB_TURBULENCE;
    d.octaves = 4;
    d.seed = 7;
    d.base_frequency[0] = 0.05; d.base_frequency[1] = 0.03;
    d.tile[0] = NAN; d.tile[1] = NAN; d.tile[2] = NAN; d.tile[3] = NAN;  // (not looked at without stitch)
    d.origin[0] = -17.25; d.origin[1] = 1000.5;
    return d;
}

static int check_generator() {
    CHECK(jturb_setup_seed(0) == 1 && jturb_setup_seed(1) == 1 && jturb_setup_seed(-1) == 2 && jturb_setup_seed(5) == 5);
    CHECK(jturb_setup_seed(INT32_MAX) == JTURB_RAND_M - 1 && jturb_setup_seed(INT32_MAX - 1) == JTURB_RAND_M - 1);
    CHECK(jturb_setup_seed(INT32_MIN) == 3 && jturb_setup_seed(-(JTURB_RAND_M - 1)) == 1 && jturb_setup_seed(-(JTURB_RAND_M - 2)) == JTURB_RAND_M - 1);
    const int32_t seeds[] = {1, 2, 3, 127773, 127774, 2147483646, 1043618065, 16807};
    for (int32_t seed : seeds) {
        int32_t s = seed;
        uint64_t t = (uint64_t)seed;
        for (int i = 1; i <= 20000; i++) {
            s = jturb_random(s);
            t = (t * 16807u) % 2147483647u;
            CHECK((uint64_t)s == t && s > 0 && s < JTURB_RAND_M);
            if (seed == 1 && i == 10000) CHECK(s == 1043618065);
        }
    }
    return 0;
}

static int check_tables() {
    const int32_t seeds[] = {0, 1, -1, 2, 12345, -2000000000, INT32_MAX, INT32_MIN};
    for (int32_t seed : seeds) {
        std::vector<uint8_t> P(256);
        std::vector<float> G(JTURB_GRADIENT_FLOATS);
        const uint32_t key = jturb_tables(seed, P.data(), G.data());
        CHECK(key == (uint32_t)jturb_setup_seed(seed) && key == jturb_tables(seed, nullptr, nullptr));
        int seen[256] = {0};
        for (int i = 0; i < 256; i++) seen[P[i]]++;
        for (int i = 0; i < 256; i++) CHECK(seen[i] == 1);
        for (uint32_t i = 0; i < JTURB_GRADIENT_FLOATS; i += 2) {
            const double len = sqrt((double)G[i] * G[i] + (double)G[i + 1] * G[i + 1]);
            const bool zero = G[i] == 0.0f && G[i + 1] == 0.0f && !signbit(G[i]) && !signbit(G[i + 1]);
            CHECK(zero || fabs(len - 1.0) <= 1.2e-7);
        }
        std::vector<char> blob(JTURB_DEVICE_BYTES);
        jturb_device_tables(P.data(), G.data(), blob.data());
        const float* g = (const float*)blob.data();
        for (uint32_t b = 0; b < 256u; b++)
            for (uint32_t c = 0; c < 4u; c++)
                for (uint32_t j = 0; j < 2u; j++) CHECK(memcmp(&g[(b * 4u + c) * 2u + j], &G[(c * 256u + b) * 2u + j], 4) == 0);
        CHECK(memcmp(blob.data() + JTURB_GRADIENT_FLOATS * 4u, P.data(), 256) == 0);
    }
    return 0;
}

static int check_plan() {
    const double freqs[] = {0.0, 0.01, 0.05, 0.25, 1.0, 1.5, 7.3, 1e-9, 1000.0};
    const double origins[] = {0.0, -0.5, 0.25, -1234.75, 1e6, -1e9, 123456789.125};
    for (uint32_t octaves = 0; octaves <= JTURB_MAX_OCTAVES; octaves += 4)
        for (double f : freqs)
            for (double o : origins) {
                jh_turbulence_desc d = legal();
                d.octaves = octaves;
                d.base_frequency[0] = f; d.base_frequency[1] = f * 0.5;
                d.origin[0] = o; d.origin[1] = -o;
                jh_turb_plan p;
                const char* why = jturb_plan(&d, &p);
                const __int128 L = ((((__int128)1) << 62) - 1) >> jturb_shift(octaves);
                if (why) {  // only the range can refuse these
                    CHECK(strstr(why, "position range"));
                    continue;
                }
                for (int a = 0; a < 2; a++) {
                    const long double fs = (long double)d.base_frequency[a] * 4294967296.0L;
                    const long double os = (long double)((d.origin[a] + 0.5) * d.base_frequency[a]) * 4294967296.0L;
                    CHECK(fabsl((long double)p.step[a] - fs) <= 0.5L && fabsl((long double)p.start[a] - os) <= 0.5L);
                    CHECK(p.frequency[a] == d.base_frequency[a] && p.wrap[a] == 0 && p.width[a] == 0);
                    const __int128 start = p.start[a], step = p.step[a], ext = p.max_extent[a];
                    CHECK(ext >= 1 && start <= L && -start <= L);
                    CHECK(start + (ext - 1) * step <= L);
                    CHECK(ext == 0xffffffffu || start + ext * step > L);
                }
                CHECK(p.key == 7u && p.stitched == 0u);
            }
    // stitch: the lo / hi rule, the width and the wrap
    jh_turbulence_desc d = legal();
    d.stitch = 1;
    d.tile[0] = 10.0; d.tile[1] = -30.0; d.tile[2] = 100.0; d.tile[3] = 64.0;
    d.base_frequency[0] = 0.047; d.base_frequency[1] = 0.0;  // 4.7 cells: lo = 0.04, hi = 0.05; 0.047 / 0.04 = 1.175 > 0.05 / 0.047 = 1.064: hi
    jh_turb_plan p;
    CHECK(jturb_plan(&d, &p) == nullptr);
    CHECK(p.frequency[0] == 5.0 / 100.0 && p.width[0] == 5 && p.wrap[0] == 0 + 5 && p.stitched == 1u);
    CHECK(p.frequency[1] == 0.0 && p.width[1] == 0 && p.wrap[1] == 0 && p.step[1] == 0);
    d.base_frequency[0] = 0.043;  // 1.075 < 1.163: lo
    CHECK(jturb_plan(&d, &p) == nullptr && p.frequency[0] == 4.0 / 100.0 && p.width[0] == 4 && p.wrap[0] == 4);
    d.base_frequency[0] = 0.004;  // a tile smaller than a cell: lo = 0, so hi = 1 / 100
    CHECK(jturb_plan(&d, &p) == nullptr && p.frequency[0] == 1.0 / 100.0 && p.width[0] == 1 && p.wrap[0] == 1);
    d.base_frequency[1] = 0.5; d.tile[1] = -30.5;  // floor(-15.25) = -16
    CHECK(jturb_plan(&d, &p) == nullptr && p.width[1] == 32 && p.wrap[1] == -16 + 32);
    return 0;
}

static int check_legality() {
    jh_turb_plan p;
    jh_turbulence_desc d = legal();
    CHECK(jturb_desc_error(&d) == nullptr && jturb_plan(&d, &p) == nullptr);
#define REFUSED(stmt, text)                                  \
    do {                                                     \
        jh_turbulence_desc e = legal();                      \
        stmt;                                                \
        CHECK(says(jturb_plan(&e, &p), text));               \
    } while (0)
    REFUSED(e.kind = 2, "kind"); REFUSED(e.kind = -1, "kind"); REFUSED(e.kind = 0, nullptr); REFUSED(e.kind = 1, nullptr);
    REFUSED(e.octaves = 17, "octaves"); REFUSED(e.octaves = 16, nullptr); REFUSED(e.octaves = 0, nullptr);
    REFUSED(e.stitch = 2, "stitch"); REFUSED(e.stitch = -1, "stitch");
    REFUSED(e.base_frequency[0] = -1e-300, "base_frequency"); REFUSED(e.base_frequency[1] = NAN, "base_frequency");
    REFUSED(e.base_frequency[0] = INFINITY, "base_frequency"); REFUSED(e.base_frequency[0] = -0.0, nullptr);
    REFUSED(e.origin[0] = NAN, "origin"); REFUSED(e.origin[1] = -INFINITY, "origin");
    REFUSED(e.stitch = 1, "tile is not finite");
    REFUSED(e.stitch = 1; e.tile[0] = e.tile[1] = 0.0; e.tile[2] = 0.0; e.tile[3] = 8.0, "tile is empty");
    REFUSED(e.stitch = 1; e.tile[0] = e.tile[1] = 0.0; e.tile[2] = 8.0; e.tile[3] = -8.0, "tile is empty");
    REFUSED(e.stitch = 1; e.tile[0] = e.tile[1] = 0.0; e.tile[2] = 8.0; e.tile[3] = 5e-324, nullptr);
    // the frequency: f 2^32 below 2^62
    REFUSED(e.octaves = 1; e.origin[0] = e.origin[1] = -0.5; e.base_frequency[0] = 1073741824.0, "2^30");
    REFUSED(e.octaves = 1; e.origin[0] = e.origin[1] = -0.5; e.base_frequency[0] = nextafter(1073741824.0, 0.0), nullptr);
    // the origin: |start| <= L, for 1 and for 16 octaves
    REFUSED(e.octaves = 1; e.base_frequency[0] = 1.0; e.origin[0] = 1073741823.5, "position range");   // (o + 0.5) 2^32 = 2^62
    REFUSED(e.octaves = 1; e.base_frequency[0] = 1.0; e.origin[0] = 1073741823.25, nullptr);
    REFUSED(e.octaves = 1; e.base_frequency[0] = 1.0; e.origin[0] = -1073741824.5, "position range");
    REFUSED(e.octaves = 1; e.base_frequency[0] = 1.0; e.origin[0] = -1073741824.25, nullptr);
    REFUSED(e.octaves = 16; e.base_frequency[0] = 1.0; e.origin[0] = 32767.5, "position range");       // 2^15 cells << 15 = 2^30 cells = 2^62
    REFUSED(e.octaves = 16; e.base_frequency[0] = 1.0; e.origin[0] = 32767.25, nullptr);
    // max_extent: the last texel inside the range
    {
        jh_turbulence_desc e = legal();
        e.octaves = 16; e.base_frequency[0] = 1.0; e.base_frequency[1] = 0.0; e.origin[0] = 32000.0;  // L = 2^47 - 1 units = 32768 cells less one unit
        CHECK(jturb_plan(&e, &p) == nullptr);
        CHECK(p.max_extent[0] == 768u && p.max_extent[1] == 0xffffffffu);  // texel 767 sits at 32767.5 cells, texel 768 at 32768.5
    }
    // the stitch pair: width and |wrap| at most (2^31 - 1) >> (octaves - 1)
    REFUSED(e.octaves = 1; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = e.tile[1] = 0.0; e.tile[2] = 2147483647.0;
            e.tile[3] = 4.0, nullptr);  // (tile_w f + 0.5 = 2^31 - 0.5: width = wrap = 2^31 - 1, the last legal pair)
    REFUSED(e.octaves = 1; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = e.tile[1] = 0.0; e.tile[2] = 2147483648.0;
            e.tile[3] = 4.0, "lattice range");
    REFUSED(e.octaves = 16; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = e.tile[1] = 0.0; e.tile[2] = 65536.0;
            e.tile[3] = 4.0, "lattice range of this many octaves");  // 65536 > (2^31 - 1) >> 15 = 65535
    REFUSED(e.octaves = 16; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = e.tile[1] = 0.0; e.tile[2] = 65535.0;
            e.tile[3] = 4.0, nullptr);
    REFUSED(e.octaves = 16; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = 65000.0; e.tile[1] = 0.0; e.tile[2] = 536.0;
            e.tile[3] = 4.0, "lattice range of this many octaves");  // wrap = 65000 + 536 = 65536
    REFUSED(e.octaves = 16; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = 65000.0; e.tile[1] = 0.0; e.tile[2] = 535.0;
            e.tile[3] = 4.0, nullptr);
    REFUSED(e.octaves = 16; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = -65540.0; e.tile[1] = 0.0; e.tile[2] = 4.0;
            e.tile[3] = 4.0, "lattice range of this many octaves");  // wrap = -65536
    REFUSED(e.octaves = 16; e.stitch = 1; e.base_frequency[0] = e.base_frequency[1] = 1.0; e.origin[0] = e.origin[1] = 0.0; e.tile[0] = -65539.0; e.tile[1] = 0.0; e.tile[2] = 4.0;
            e.tile[3] = 4.0, nullptr);
#undef REFUSED
    return 0;
}

// The specification's lookup, literally: tables of BSize + BSize + 2 entries whose upper part repeats the lower one, no mask after
// the first level.
static int check_lattice() {
    const int32_t seeds[] = {0, 1, 99, -77};
    for (int32_t seed : seeds) {
        std::vector<uint8_t> P(256);
        std::vector<float> G(JTURB_GRADIENT_FLOATS);
        jturb_tables(seed, P.data(), G.data());
        std::vector<int> L(514);
        std::vector<float> D(4 * 514 * 2);
        for (int i = 0; i < 514; i++) {
            L[i] = P[i & 255];
            for (int k = 0; k < 4; k++)
                for (int j = 0; j < 2; j++) D[(k * 514 + i) * 2 + j] = G[(k * 256 + (i & 255)) * 2 + j];
        }
        for (int i = 0; i < 258; i++) CHECK(L[256 + i] == L[i]);  // (what init's last loop builds)
        for (uint32_t bx0 = 0; bx0 < 256u; bx0++)
            for (uint32_t by0 = 0; by0 < 256u; by0++) {
                const uint32_t bx1 = (bx0 + 1u) & 255u, by1 = (by0 + 1u) & 255u;
                const int i = L[bx0], j = L[bx1];
                const int spec[4] = {L[i + by0], L[j + by0], L[i + by1], L[j + by1]};  // (indices up to 510)
                uint32_t pi, pj, b[4];
                jturb_lattice_x(P.data(), bx0, bx1, &pi, &pj);
                jturb_lattice_y(P.data(), pi, pj, by0, by1, b);
                for (int q = 0; q < 4; q++) {
                    CHECK((int)b[q] == spec[q]);
                    for (int k = 0; k < 4; k++) CHECK(memcmp(&D[(k * 514 + spec[q]) * 2], &G[(k * 256 + b[q]) * 2], 8) == 0);
                }
            }
    }
    // the pieces on a texel: a lattice point gives exactly 0, the split floors negative positions
    int32_t cell;
    float r0;
    jturb_split(-1, &cell, &r0);
    CHECK(cell == -1 && r0 == 16777215.0f / 16777216.0f);
    jturb_split(-((int64_t)3 << 32), &cell, &r0);
    CHECK(cell == -3 && r0 == 0.0f);
    jturb_split(((int64_t)5 << 32) | 0x80000000u, &cell, &r0);
    CHECK(cell == 5 && r0 == 0.5f);
    CHECK(jturb_s(0.0f) == 0.0f && jturb_s(1.0f) == 1.0f && jturb_s(0.5f) == 0.5f);
    CHECK(jturb_stitch(7, 8, 5) == 7u && jturb_stitch(8, 8, 5) == 3u && (jturb_stitch(-3, -4, 2) & 255u) == 251u);
    return 0;
}

static int texels(char** v) {
    jh_turbulence_desc d;
    memset(&d, 0, sizeof d);
    d.kind = atoi(v[0]); d.octaves = (uint32_t)atoi(v[1]); d.seed = (int32_t)atoll(v[2]); d.stitch = atoi(v[3]);
    d.base_frequency[0] = strtod(v[4], nullptr); d.base_frequency[1] = strtod(v[5], nullptr);
    for (int i = 0; i < 4; i++) d.tile[i] = strtod(v[6 + i], nullptr);
    d.origin[0] = strtod(v[10], nullptr); d.origin[1] = strtod(v[11], nullptr);
    const uint32_t X = (uint32_t)atoll(v[12]), Y = (uint32_t)atoll(v[13]), W = (uint32_t)atoll(v[14]), H = (uint32_t)atoll(v[15]);
    jh_turb_plan p;
    if (const char* why = jturb_plan(&d, &p)) { printf("refused: %s\n", why); return 2; }
    if ((uint64_t)X + W > p.max_extent[0] || (uint64_t)Y + H > p.max_extent[1]) { printf("refused: beyond max_extent\n"); return 2; }
    std::vector<uint8_t> P(256);
    std::vector<float> G(JTURB_GRADIENT_FLOATS);
    jturb_tables(d.seed, P.data(), G.data());
    for (uint32_t y = Y; y < Y + H; y++)
        for (uint32_t x = X; x < X + W; x++) {
            float out[4];
            uint32_t bits[4];
            jturb_texel(&p, d.kind, d.octaves, P.data(), G.data(), x, y, out);
            memcpy(bits, out, 16);
            printf("%08x %08x %08x %08x\n", bits[0], bits[1], bits[2], bits[3]);
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 18 && strcmp(argv[1], "texels") == 0) return texels(argv + 2);
    if (argc != 1) { printf("usage: turbulence_check [texels KIND OCTAVES SEED STITCH FX FY TX TY TW TH OX OY X Y W H]\n"); return 2; }
    if (check_generator() || check_tables() || check_plan() || check_legality() || check_lattice()) return 1;
    printf("ok\n");
    return 0;
}
