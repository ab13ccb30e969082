// lighting_check.cpp -- include/jello_lighting.h exercised stand-alone, for the sanitizers (CPU only; needs no GPU and no library):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//         tools/lighting_check.cpp -o /tmp/lighting_check && /tmp/lighting_check
//
// Four things.  (1) jlight_desc_error on every kind x light with legal fields -- what the kind and the light do not use poisoned with
// NaN -- and on a set of illegal descriptors, each with the text it has to answer.  (2) jlight_plan against long double: the six
// factors, the two unit vectors (within a binary32 half ULP of the long double quotient; exact for lengths that are exact), the
// position and the cone.  (3) jlight_normal on every texel of every image of 1..4 x 1..4 texels against the specification's table
// written out literally -- interior, four edges, four corners, and the forms an image one texel wide or high leaves -- with
// small-integer alpha and surface_scale 3, on which every factor, sum and product is exact; the 3 x 3 neighbourhood is gathered with
// clamped indices as the kernel stages it.  (4) jlight_table on a heap array of exactly 4097 floats, for exponents 1.5, 2, 20 and 128:
// T[0] = 0, T[4096] = 1, never decreasing, and jlight_pw at the ends and on a node.  Prints "ok" and returns 0.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jello_lighting.h"

static bool says(const char* got, const char* want) { return want ? (got && strstr(got, want)) : got == nullptr; }

static jh_lighting_desc legal(int kind, int light) {
    jh_lighting_desc d;
    memset(&d, 0, sizeof d);
    d.kind = kind; d.light = light;
    d.surface_scale = -2.5f; d.constant = 0.0f;
    d.specular_exponent = kind == JLIGHT_SPECULAR ? 128.0f : NAN;
    d.spot_exponent = light == JLIGHT_SPOT ? 1.0f : NAN;
    d.color[0] = 0.0f; d.color[1] = 1.0f; d.color[2] = 7.0f;
    for (int c = 0; c < 3; c++) {
        d.direction[c] = light == JLIGHT_DISTANT ? (double)(c - 1) : (double)NAN;
        d.position[c] = light != JLIGHT_DISTANT ? 1.0e6 * (c - 1) : (double)NAN;
        d.points_at[c] = light == JLIGHT_SPOT ? 3.0 - c : (double)NAN;
    }
    d.cone_cos = light == JLIGHT_SPOT ? -1.0 : (double)NAN;
    return d;
}

static int check_descriptors() {
    for (int kind = 0; kind < JLIGHT_KINDS; kind++)
        for (int light = 0; light < JLIGHT_LIGHTS; light++) {
            jh_lighting_desc d = legal(kind, light);
            if (jlight_desc_error(&d)) return 1;
            d.cone_cos = light == JLIGHT_SPOT ? 1.0 : d.cone_cos;
            if (jlight_desc_error(&d)) return 2;
            jh_lighting_desc b = d;
            b.surface_scale = INFINITY;
            if (!says(jlight_desc_error(&b), "surface_scale")) return 3;
            b = d; b.constant = -0.5f;
            if (!says(jlight_desc_error(&b), "constant")) return 4;
            b = d; b.constant = NAN;
            if (!says(jlight_desc_error(&b), "constant")) return 5;
            b = d; b.color[2] = -1.0f;
            if (!says(jlight_desc_error(&b), "color")) return 6;
            b = d; b.color[0] = INFINITY;
            if (!says(jlight_desc_error(&b), "color")) return 7;
            if (kind == JLIGHT_SPECULAR) {
                const float bad[] = {0.99999994f, 128.00002f, NAN, -1.0f, INFINITY};
                for (float e : bad) {
                    b = d; b.specular_exponent = e;
                    if (!says(jlight_desc_error(&b), "specular_exponent")) return 8;
                }
                b = d; b.specular_exponent = 1.0f;
                if (jlight_desc_error(&b)) return 9;
            }
            if (light == JLIGHT_DISTANT) {
                b = d; b.direction[0] = b.direction[1] = b.direction[2] = 0.0;
                if (!says(jlight_desc_error(&b), "direction")) return 10;
                b = d; b.direction[1] = INFINITY;
                if (!says(jlight_desc_error(&b), "direction")) return 11;
                b = d; b.direction[0] = 1e200;
                if (!says(jlight_desc_error(&b), "direction")) return 12;
                b = d; b.direction[0] = 1e-200; b.direction[1] = 0.0; b.direction[2] = 0.0;
                if (!says(jlight_desc_error(&b), "direction")) return 13;
            } else {
                b = d; b.position[2] = 1e39;
                if (!says(jlight_desc_error(&b), "position")) return 14;
                b = d; b.position[0] = NAN;
                if (!says(jlight_desc_error(&b), "position")) return 15;
            }
            if (light == JLIGHT_SPOT) {
                b = d;
                for (int c = 0; c < 3; c++) b.points_at[c] = b.position[c];
                if (!says(jlight_desc_error(&b), "points_at")) return 16;
                b = d; b.points_at[1] = NAN;
                if (!says(jlight_desc_error(&b), "points_at")) return 17;
                b = d; b.spot_exponent = 0.5f;
                if (!says(jlight_desc_error(&b), "spot_exponent")) return 18;
                b = d; b.spot_exponent = 129.0f;
                if (!says(jlight_desc_error(&b), "spot_exponent")) return 19;
                b = d; b.cone_cos = 1.0000000000000002;
                if (!says(jlight_desc_error(&b), "cone_cos")) return 20;
                b = d; b.cone_cos = NAN;
                if (!says(jlight_desc_error(&b), "cone_cos")) return 21;
            }
            jh_light_plan untouched, p;
            memset(&untouched, 0x5a, sizeof untouched);
            p = untouched;
            b = d; b.constant = -1.0f;
            if (!jlight_plan(&b, &p) || memcmp(&p, &untouched, sizeof p) != 0) return 22;  // (a refused plan is not written)
        }
    jh_lighting_desc d = legal(0, 0);
    d.kind = 2;
    if (!says(jlight_desc_error(&d), "kind")) return 23;
    d.kind = -1;
    if (!says(jlight_desc_error(&d), "kind")) return 24;
    d = legal(0, 0);
    d.light = 3;
    if (!says(jlight_desc_error(&d), "light")) return 25;
    d.light = -1;
    if (!says(jlight_desc_error(&d), "light")) return 26;
    return 0;
}

static bool near32(float got, long double want) {  // within half a binary32 ULP of `want`, and a little for the binary64 quotient under it
    const long double ulp = ldexpl(1.0L, ilogbl(fabsl(want) > 0 ? fabsl(want) : 1.0L) - 23);
    return fabsl((long double)got - want) <= 0.5L * ulp * (1.0L + 1e-6L);
}

static int check_plan() {
    const float scales[] = {0.0f, -0.0f, 1.0f, 3.0f, -2.5f, 1000.0f, 1e-30f, 0.1f};
    for (float ss : scales) {
        jh_lighting_desc d = legal(JLIGHT_DIFFUSE, JLIGHT_DISTANT);
        d.surface_scale = ss;
        jh_light_plan p;
        if (jlight_plan(&d, &p)) return 30;
        for (uint32_t span = 1; span <= 2; span++)
            for (uint32_t wsum = 2; wsum <= 4; wsum++) {
                const long double want = -(long double)ss * 2.0L / (long double)(span * wsum);
                if (!near32(p.s[span - 1][wsum - 2], want)) return 31;
                if (p.s[span - 1][wsum - 2] != jlight_s(&p.s[0][0], span, wsum)) return 32;
            }
        if (signbit(p.s[0][0]) == signbit(ss) && ss == 0.0f) return 33;  // (-(+0) is -0)
    }
    const double dirs[][3] = {{0, 0, 1}, {3, 4, 0}, {1, 2, 2}, {-1, 1, 1}, {0.3, -0.7, 0.2}, {1e-3, 1e3, -1}, {2, 3, 6}, {1e150, 1e150, 0}};
    for (const auto& v : dirs) {
        jh_lighting_desc d = legal(JLIGHT_SPECULAR, JLIGHT_DISTANT);
        for (int c = 0; c < 3; c++) d.direction[c] = v[c];
        jh_light_plan p;
        if (jlight_plan(&d, &p)) return 34;
        const long double len = sqrtl((long double)v[0] * v[0] + (long double)v[1] * v[1] + (long double)v[2] * v[2]);
        for (int c = 0; c < 3; c++)
            if (!near32(p.ldir[c], (long double)v[c] / len)) return 35;
        if (p.p[0] != 0.0f || p.sdir[2] != 0.0f || p.cone != 0.0f) return 36;
        // the same vector as a spot's axis, from a position that keeps the difference exact
        d = legal(JLIGHT_DIFFUSE, JLIGHT_SPOT);
        for (int c = 0; c < 3; c++) { d.position[c] = 0.0; d.points_at[c] = v[c]; }
        d.position[2] = 0.0;
        d.cone_cos = 0.30000000000000004;
        jh_light_plan q;
        if (jlight_plan(&d, &q)) return 37;
        if (memcmp(q.sdir, p.ldir, sizeof q.sdir) != 0 || q.cone != (float)0.30000000000000004 || q.ldir[2] != 0.0f) return 38;
    }
    {  // exact lengths give exact components
        jh_lighting_desc d = legal(JLIGHT_DIFFUSE, JLIGHT_DISTANT);
        d.direction[0] = 3; d.direction[1] = 4; d.direction[2] = 0;
        jh_light_plan p;
        if (jlight_plan(&d, &p) || p.ldir[0] != (float)(3.0 / 5.0) || p.ldir[1] != (float)(4.0 / 5.0) || p.ldir[2] != 0.0f) return 39;
        d = legal(JLIGHT_DIFFUSE, JLIGHT_POINT);
        d.position[0] = 0.1; d.position[1] = -1e30; d.position[2] = 16777217.0;
        if (jlight_plan(&d, &p) || p.p[0] != 0.1f || p.p[1] != -1e30f || p.p[2] != 16777216.0f) return 40;
    }
    return 0;
}

// The specification's table, literally, on an image I of W x H (row-major) with surface_scale ss -- and, for an image one texel wide
// or high, the forms the rule leaves: no gradient along the axis of one texel, the weights (2) of the one row or column that exists
// along the other.
struct Img {
    int W, H;
    const double* v;
    double operator()(int x, int y) const { return v[y * W + x]; }
};
static void spec_normal(const Img& I, double ss, int x, int y, double* nx, double* ny) {
    const int W = I.W, H = I.H;
    const bool l = x == 0, r = x == W - 1, t = y == 0, b = y == H - 1;
    if (W == 1) *nx = 0.0;
    if (H == 1) *ny = 0.0;
    if (W == 1 && H > 1) {
        *ny = t ? -ss * 1.0 * (2 * I(x, y + 1) - 2 * I(x, y)) : b ? -ss * 1.0 * (2 * I(x, y) - 2 * I(x, y - 1)) : -ss * 1.0 / 2.0 * (2 * I(x, y + 1) - 2 * I(x, y - 1));
        return;
    }
    if (H == 1 && W > 1) {
        *nx = l ? -ss * 1.0 * (2 * I(x + 1, y) - 2 * I(x, y)) : r ? -ss * 1.0 * (2 * I(x, y) - 2 * I(x - 1, y)) : -ss * 1.0 / 2.0 * (2 * I(x + 1, y) - 2 * I(x - 1, y));
        return;
    }
    if (W == 1 || H == 1) return;
    if (t && l) {  // top/left corner
        *nx = -ss * 2.0 / 3.0 * ((2 * I(x + 1, y) + I(x + 1, y + 1)) - (2 * I(x, y) + I(x, y + 1)));
        *ny = -ss * 2.0 / 3.0 * ((2 * I(x, y + 1) + I(x + 1, y + 1)) - (2 * I(x, y) + I(x + 1, y)));
    } else if (t && r) {  // top/right corner
        *nx = -ss * 2.0 / 3.0 * ((2 * I(x, y) + I(x, y + 1)) - (2 * I(x - 1, y) + I(x - 1, y + 1)));
        *ny = -ss * 2.0 / 3.0 * ((I(x - 1, y + 1) + 2 * I(x, y + 1)) - (I(x - 1, y) + 2 * I(x, y)));
    } else if (b && l) {  // bottom/left corner
        *nx = -ss * 2.0 / 3.0 * ((I(x + 1, y - 1) + 2 * I(x + 1, y)) - (I(x, y - 1) + 2 * I(x, y)));
        *ny = -ss * 2.0 / 3.0 * ((2 * I(x, y) + I(x + 1, y)) - (2 * I(x, y - 1) + I(x + 1, y - 1)));
    } else if (b && r) {  // bottom/right corner
        *nx = -ss * 2.0 / 3.0 * ((I(x, y - 1) + 2 * I(x, y)) - (I(x - 1, y - 1) + 2 * I(x - 1, y)));
        *ny = -ss * 2.0 / 3.0 * ((I(x - 1, y) + 2 * I(x, y)) - (I(x - 1, y - 1) + 2 * I(x, y - 1)));
    } else if (t) {  // top row
        *nx = -ss * 1.0 / 3.0 * ((2 * I(x + 1, y) + I(x + 1, y + 1)) - (2 * I(x - 1, y) + I(x - 1, y + 1)));
        *ny = -ss * 1.0 / 2.0 * ((I(x - 1, y + 1) + 2 * I(x, y + 1) + I(x + 1, y + 1)) - (I(x - 1, y) + 2 * I(x, y) + I(x + 1, y)));
    } else if (b) {  // bottom row
        *nx = -ss * 1.0 / 3.0 * ((I(x + 1, y - 1) + 2 * I(x + 1, y)) - (I(x - 1, y - 1) + 2 * I(x - 1, y)));
        *ny = -ss * 1.0 / 2.0 * ((I(x - 1, y) + 2 * I(x, y) + I(x + 1, y)) - (I(x - 1, y - 1) + 2 * I(x, y - 1) + I(x + 1, y - 1)));
    } else if (l) {  // left column
        *nx = -ss * 1.0 / 2.0 * ((I(x + 1, y - 1) + 2 * I(x + 1, y) + I(x + 1, y + 1)) - (I(x, y - 1) + 2 * I(x, y) + I(x, y + 1)));
        *ny = -ss * 1.0 / 3.0 * ((2 * I(x, y + 1) + I(x + 1, y + 1)) - (2 * I(x, y - 1) + I(x + 1, y - 1)));
    } else if (r) {  // right column
        *nx = -ss * 1.0 / 2.0 * ((I(x, y - 1) + 2 * I(x, y) + I(x, y + 1)) - (I(x - 1, y - 1) + 2 * I(x - 1, y) + I(x - 1, y + 1)));
        *ny = -ss * 1.0 / 3.0 * ((I(x - 1, y + 1) + 2 * I(x, y + 1)) - (I(x - 1, y - 1) + 2 * I(x, y - 1)));
    } else {  // interior
        *nx = -ss * 1.0 / 4.0 * ((I(x + 1, y - 1) + 2 * I(x + 1, y) + I(x + 1, y + 1)) - (I(x - 1, y - 1) + 2 * I(x - 1, y) + I(x - 1, y + 1)));
        *ny = -ss * 1.0 / 4.0 * ((I(x - 1, y + 1) + 2 * I(x, y + 1) + I(x + 1, y + 1)) - (I(x - 1, y - 1) + 2 * I(x, y - 1) + I(x + 1, y - 1)));
    }
}

static int check_normals() {
    jh_lighting_desc d = legal(JLIGHT_DIFFUSE, JLIGHT_DISTANT);
    d.surface_scale = 3.0f;  // every factor -3 * 2 / (span wsum) is exact
    jh_light_plan p;
    if (jlight_plan(&d, &p)) return 50;
    const float want_s[2][3] = {{-3.0f, -2.0f, -1.5f}, {-1.5f, -1.0f, -0.75f}};
    if (memcmp(p.s, want_s, sizeof want_s) != 0) return 51;
    uint32_t seed = 12345u;
    int cases_seen = 0;
    for (int W = 1; W <= 4; W++)
        for (int H = 1; H <= 4; H++) {
            std::vector<double> v((size_t)W * H);
            for (double& e : v) { seed = seed * 1664525u + 1013904223u; e = (double)((int)(seed >> 24) % 17 - 8); }
            const Img I = {W, H, v.data()};
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    float a[3][3];
                    for (int j = 0; j < 3; j++)
                        for (int i = 0; i < 3; i++) {
                            const int cx = x - 1 + i < 0 ? 0 : (x - 1 + i > W - 1 ? W - 1 : x - 1 + i), cy = y - 1 + j < 0 ? 0 : (y - 1 + j > H - 1 ? H - 1 : y - 1 + j);
                            a[j][i] = (float)I(cx, cy);
                        }
                    float nx, ny;
                    jlight_normal(&p.s[0][0], (uint32_t)x, (uint32_t)y, (uint32_t)W, (uint32_t)H, a, &nx, &ny);
                    double wx = 0.0, wy = 0.0;
                    spec_normal(I, 3.0, x, y, &wx, &wy);
                    if ((double)nx != wx || (double)ny != wy) { fprintf(stderr, "normal at (%d, %d) of %d x %d: (%g, %g), want (%g, %g)\n", x, y, W, H, nx, ny, wx, wy); return 52; }
                    if (W >= 3 && H >= 3) cases_seen |= 1 << ((x == 0 ? 0 : x == W - 1 ? 2 : 1) + 3 * (y == 0 ? 0 : y == H - 1 ? 2 : 1));
                }
        }
    return cases_seen == 0x1ff ? 0 : 53;  // all nine
}

static int check_tables() {
    const float exps[] = {1.5f, 2.0f, 20.0f, 128.0f};
    for (float e : exps) {
        std::vector<float> T(JLIGHT_ENTRIES);  // exactly what is written
        jlight_table(e, T.data());
        if (T[0] != 0.0f || T[JLIGHT_STEPS] != 1.0f) return 60;
        for (uint32_t i = 1; i < JLIGHT_ENTRIES; i++)
            if (!(T[i] >= T[i - 1])) return 61;
        if (T[2048] != (float)pow(0.5, (double)e)) return 62;
        if (jlight_pw(T.data(), 0.0f) != 0.0f || jlight_pw(T.data(), 1.0f) != 1.0f || jlight_pw(T.data(), 0.5f) != T[2048]) return 63;
        float f;
        if (jlight_segment(1.0f, &f) != JLIGHT_STEPS - 1 || f != 1.0f || jlight_segment(0.99999994f, &f) != JLIGHT_STEPS - 1) return 64;
        if (jlight_segment(0.25f, &f) != 1024 || f != 0.0f || jlight_segment(ldexpf(3.0f, -14), &f) != 0 || f != 0.75f) return 65;
    }
    jh_lighting_desc d = legal(JLIGHT_SPECULAR, JLIGHT_SPOT);
    jlight_key k;
    jlight_key_of(&d, &k);
    uint32_t bits;
    memcpy(&bits, &d.specular_exponent, 4);
    if (jlight_which(&d) != JLIGHT_TABLE_SPEC || k.spec_bits != bits || k.spot_bits != 0u) return 66;
    d.spot_exponent = 8.0f; d.specular_exponent = 1.0f;
    jlight_key_of(&d, &k);
    if (jlight_which(&d) != JLIGHT_TABLE_SPOT || k.spec_bits != 0u || k.spot_bits != 0x41000000u) return 67;
    std::vector<float> spot(JLIGHT_ENTRIES, -1.0f);
    if (jlight_tables(&d, nullptr, spot.data()) != JLIGHT_TABLE_SPOT || spot[JLIGHT_STEPS] != 1.0f || spot[0] != 0.0f) return 68;
    d = legal(JLIGHT_DIFFUSE, JLIGHT_POINT);
    if (jlight_which(&d) != 0u || jlight_tables(&d, nullptr, nullptr) != 0u) return 69;
    return 0;
}

int main() {
    int (*const checks[])() = {check_descriptors, check_plan, check_normals, check_tables};
    for (auto check : checks)
        if (int rc = check()) {
            fprintf(stderr, "lighting_check: failed with %d\n", rc);
            return rc;
        }
    printf("ok\n");
    return 0;
}
