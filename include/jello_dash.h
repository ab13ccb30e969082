// jello_dash.h -- the dash rule, stated once for its two users: the host route (jello_amd/host/dash.cpp,
// g++) and the device stage jh_dash (jello_amd/csrc/kernels_dash.hip, hipcc).  tests/dash_ref.py restates it independently;
// all three must agree byte for byte.
//
// Everything here is a pure function of its arguments: integer arithmetic, and fixed sequences of binary64 + - * / sqrt with
// no contraction (both Makefiles build without it, see dmath.h).  Positions along a subpath are 64-bit integers on a grid of
// 2^-20 user units; the lengths of a curve's panels are integers on 2^-32 units, so a segment's length is the same word in
// whatever order its panels are summed.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JDASH_FN __host__ __device__ inline
#else
#define JDASH_FN inline
#endif

#define JDASH_MAX_PATTERN 64      // entries of a pattern
#define JDASH_COARSE 32           // coarse sums per segment (the first level of the cumulative table)
#define JDASH_MAX_PANELS 4096     // K is held to this; the accuracy bound is stated for control points in [0, 4096]^2, where K <= 2508
#define JDASH_SOLVE_ITERATIONS 8  // safeguarded Newton steps of the inverse, always all of them
#define JDASH_COORD_LIMIT 1048576.0         // |coordinate| <= 2^20, else the input is rejected
#define JDASH_ENTRY_LIMIT 1073741824.0      // pattern entry <= 2^30
#define JDASH_OFFSET_LIMIT 1099511627776.0  // |offset| <= 2^40
#define JDASH_MAX_STARTS 0x20000000         // dashes counted per segment are held to 2^29 (memory safety only: such a job never fits)

// PathElKind values (host/gfx.h); the device element is {u32 kind, f32 p[6]}
enum { JDASH_MOVE = 0, JDASH_LINE = 1, JDASH_QUAD = 2, JDASH_CUBIC = 3, JDASH_CLOSE = 4 };

struct JDashEl {  // 28 bytes
    uint32_t kind;
    float p[6];
};
struct JDashSeg {  // one drawn segment: its kind (LINE / QUAD / CUBIC) and control points p0 .. p3 (x, y pairs; unused ones 0)
    double p[8];
    uint32_t kind;
    uint32_t sub;  // index of its subpath
};
struct JDashRun {  // one maximal "on" run of a pattern's period: [start, start + len) in phase units, 0 <= start < period
    int64_t start, len;
};
struct JDashPat {  // a quantised pattern: period, phase at position 0, its runs (sorted by start)
    int64_t period, phase;
    uint32_t first_run, n_runs;
    uint32_t solid;  // 1: on everywhere (n_runs == 0 then; n_runs == 0 without it: on nowhere)
    uint32_t pad;
};
struct JDashSub {  // one subpath
    uint32_t first_seg, n_segs;
    uint32_t pat;     // index of its path's pattern
    uint32_t closed;  // ended by ClosePath
};
struct JDashSegLen {  // what the lengths pass knows about a segment
    int64_t coarse[JDASH_COARSE];  // 2^-32 units: the sum of the panels of coarse block c
    int64_t q;                     // length, 2^-20 units
    int64_t start;                 // position of its start along the subpath, 2^-20 units
    uint32_t panels;               // K (0 for a line)
    uint32_t pad;
};
struct JDashSubInfo {
    int64_t total;   // the subpath's length, 2^-20 units
    int64_t bfirst;  // merged: where the dash that holds position 0 ends
    uint32_t whole;  // closed and one dash covers it all
    uint32_t merged; // closed, not whole, the first dash starts at 0 and the last one ends at `total`: they are one dash
};

// ---- integer helpers ----
JDASH_FN int64_t jdash_floordiv(int64_t a, int64_t b) {  // b > 0
    int64_t d = a / b;
    return (a % b < 0) ? d - 1 : d;
}
JDASH_FN int64_t jdash_quantise(double x, double scale) { return (int64_t)llrint(x * scale); }  // rint: ties to even
JDASH_FN int64_t jdash_q20_of_q32(int64_t s32) { return (s32 + 2048) >> 12; }

// ---- the pattern as an "on" set ----
// Position s of a subpath has phase y = s + pat.phase; the period index is floor(y / period), the remainder r in [0, period).
// s is on iff r or r + period lies in a run (a run may reach past the period's end: the one merged across it).
JDASH_FN bool jdash_run_at(const JDashPat& pat, const JDashRun* runs, int64_t s, int64_t* a, int64_t* b) {
    if (pat.solid) {
        *a = INT64_MIN / 2;
        *b = INT64_MAX / 2;
        return true;
    }
    const int64_t y = s + pat.phase;
    const int64_t per = jdash_floordiv(y, pat.period);
    const int64_t r = y - per * pat.period;
    for (uint32_t k = 0; k < pat.n_runs; k++) {
        const JDashRun run = runs[pat.first_run + k];
        if (r >= run.start && r < run.start + run.len) {
            *a = per * pat.period + run.start - pat.phase;
            *b = *a + run.len;
            return true;
        }
        if (r + pat.period < run.start + run.len) {  // (run.start <= r + period always)
            *a = (per - 1) * pat.period + run.start - pat.phase;
            *b = *a + run.len;
            return true;
        }
    }
    return false;
}
// The number of run starts at positions below x, up to a constant that is the same for every x (only differences are used).
JDASH_FN int64_t jdash_starts_below(const JDashPat& pat, const JDashRun* runs, int64_t x) {
    const int64_t y = x + pat.phase;
    const int64_t per = jdash_floordiv(y, pat.period);
    const int64_t r = y - per * pat.period;
    int64_t n = 0;
    for (uint32_t k = 0; k < pat.n_runs; k++) n += (runs[pat.first_run + k].start < r) ? 1 : 0;
    return per * (int64_t)pat.n_runs + n;
}
// The run whose start has index idx in the numbering of jdash_starts_below.
JDASH_FN void jdash_run_by_index(const JDashPat& pat, const JDashRun* runs, int64_t idx, int64_t* a, int64_t* b) {
    const int64_t per = jdash_floordiv(idx, (int64_t)pat.n_runs);
    const JDashRun run = runs[pat.first_run + (uint32_t)(idx - per * (int64_t)pat.n_runs)];
    *a = per * pat.period + run.start - pat.phase;
    *b = *a + run.len;
}

// ---- segment lengths ----
// K uniform panels, K = ceil(sqrt(64 * D2)) held to [1, JDASH_MAX_PANELS]: D2 bounds |B''| (6 x the largest second difference
// of a cubic's control points in the 1-norm, 2 x a quad's); 64 = c / 2^-10 with c = 1/16.
JDASH_FN double jdash_abs(double x) { return x < 0.0 ? -x : x; }
JDASH_FN uint32_t jdash_panels(const JDashSeg& g) {
    if (g.kind == JDASH_LINE) return 0u;
    const double* p = g.p;
    double d2 = jdash_abs((p[0] - 2.0 * p[2]) + p[4]) + jdash_abs((p[1] - 2.0 * p[3]) + p[5]);
    if (g.kind == JDASH_CUBIC) {
        const double e = jdash_abs((p[2] - 2.0 * p[4]) + p[6]) + jdash_abs((p[3] - 2.0 * p[5]) + p[7]);
        d2 = 6.0 * (e > d2 ? e : d2);
    } else {
        d2 = 2.0 * d2;
    }
    const double k = ceil(sqrt(64.0 * d2));
    if (!(k >= 1.0)) return 1u;
    if (!(k < (double)JDASH_MAX_PANELS)) return JDASH_MAX_PANELS;
    return (uint32_t)k;
}
// |B'(t)|
JDASH_FN double jdash_speed(const JDashSeg& g, double t) {
    const double* p = g.p;
    const double mt = 1.0 - t;
    if (g.kind == JDASH_CUBIC) {
        const double a = mt * mt, b = (mt * t) * 2.0, c = t * t;
        const double dx = (a * (p[2] - p[0]) + b * (p[4] - p[2])) + c * (p[6] - p[4]);
        const double dy = (a * (p[3] - p[1]) + b * (p[5] - p[3])) + c * (p[7] - p[5]);
        return 3.0 * sqrt(dx * dx + dy * dy);
    }
    const double dx = mt * (p[2] - p[0]) + t * (p[4] - p[2]);
    const double dy = mt * (p[3] - p[1]) + t * (p[5] - p[3]);
    return 2.0 * sqrt(dx * dx + dy * dy);
}
// The length of [t0, t0 + u h] by the 4-point Gauss-Legendre rule on that interval, summed in this order.
JDASH_FN double jdash_panel_length(const JDashSeg& g, double t0, double h, double u) {
    const double X0 = 0.06943184420297371, X1 = 0.33000947820757187, X2 = 0.6699905217924281, X3 = 0.9305681557970262;
    const double W0 = 0.17392742256872692, W1 = 0.3260725774312731;
    const double hu = u * h;
    const double s0 = jdash_speed(g, t0 + hu * X0), s1 = jdash_speed(g, t0 + hu * X1);
    const double s2 = jdash_speed(g, t0 + hu * X2), s3 = jdash_speed(g, t0 + hu * X3);
    return hu * (((W0 * s0 + W1 * s1) + W1 * s2) + W0 * s3);
}
JDASH_FN int64_t jdash_panel_q32(const JDashSeg& g, uint32_t panels, uint32_t k) {
    const double h = 1.0 / (double)panels;
    return jdash_quantise(jdash_panel_length(g, (double)k * h, h, 1.0), 4294967296.0);
}
JDASH_FN int64_t jdash_line_q32(const JDashSeg& g) {
    const double dx = g.p[2] - g.p[0], dy = g.p[3] - g.p[1];
    return jdash_quantise(sqrt(dx * dx + dy * dy), 4294967296.0);
}
JDASH_FN uint32_t jdash_block_panels(uint32_t panels) { return (panels + JDASH_COARSE - 1u) / JDASH_COARSE; }  // panels per coarse block
// Sequential form of the lengths pass for one segment (the device sums the same integers in parallel); `start` is left alone.
JDASH_FN void jdash_measure(const JDashSeg& g, JDashSegLen* out) {
    for (int c = 0; c < JDASH_COARSE; c++) out->coarse[c] = 0;
    out->panels = jdash_panels(g);
    int64_t s32 = 0;
    if (out->panels == 0u) {
        s32 = jdash_line_q32(g);
    } else {
        const uint32_t bp = jdash_block_panels(out->panels);
        for (uint32_t k = 0; k < out->panels; k++) {
            const int64_t v = jdash_panel_q32(g, out->panels, k);
            out->coarse[k / bp] += v;
            s32 += v;
        }
    }
    out->q = jdash_q20_of_q32(s32);
    out->pad = 0u;
}
// The parameter at which the segment has run `s` of its q units, 0 < s < q.
JDASH_FN double jdash_inverse(const JDashSeg& g, const JDashSegLen& len, int64_t s) {
    if (len.panels == 0u) return (double)s / (double)len.q;
    const int64_t target = s << 12;  // 2^-32 units; below the sum of the panels because s <= q - 1
    const uint32_t bp = jdash_block_panels(len.panels);
    int64_t acc = 0;
    uint32_t c = 0;
    while (c + 1u < JDASH_COARSE && acc + len.coarse[c] <= target) acc += len.coarse[c++];
    uint32_t k = c * bp;
    int64_t pk = jdash_panel_q32(g, len.panels, k);
    while (k + 1u < len.panels && acc + pk <= target) {
        acc += pk;
        k++;
        pk = jdash_panel_q32(g, len.panels, k);
    }
    const double h = 1.0 / (double)len.panels;
    const double t0 = (double)k * h;
    const double tau = (double)(target - acc) / 4294967296.0;
    const double full = jdash_panel_length(g, t0, h, 1.0);
    double lo = 0.0, hi = 1.0;
    double u = tau / full;
    for (int it = 0; it < JDASH_SOLVE_ITERATIONS; it++) {
        if (!(u >= lo && u <= hi)) u = 0.5 * (lo + hi);
        const double r = jdash_panel_length(g, t0, h, u) - tau;
        if (r > 0.0) hi = u; else lo = u;
        const double sp = jdash_speed(g, t0 + u * h) * h;
        u = (sp > 0.0) ? u - r / sp : 2.0;  // (2: outside every bracket, the next step bisects)
    }
    if (!(u >= lo && u <= hi)) u = 0.5 * (lo + hi);
    const double t = t0 + u * h;
    return t < 1.0 ? t : 1.0;
}

// ---- sub-curves: the blossom of the control polygon, one de Casteljau level per argument ----
JDASH_FN double jdash_lerp(double a, double b, double t) { return t == 1.0 ? b : a + (b - a) * t; }
JDASH_FN void jdash_blossom(const JDashSeg& g, double t1, double t2, double t3, double* x, double* y) {
    const double* p = g.p;
    for (int d = 0; d < 2; d++) {
        double v;
        if (g.kind == JDASH_CUBIC) {
            const double a = jdash_lerp(p[d], p[2 + d], t1), b = jdash_lerp(p[2 + d], p[4 + d], t1), c = jdash_lerp(p[4 + d], p[6 + d], t1);
            v = jdash_lerp(jdash_lerp(a, b, t2), jdash_lerp(b, c, t2), t3);
        } else if (g.kind == JDASH_QUAD) {
            v = jdash_lerp(jdash_lerp(p[d], p[2 + d], t1), jdash_lerp(p[2 + d], p[4 + d], t1), t2);
        } else {
            v = jdash_lerp(p[d], p[2 + d], t1);
        }
        *(d ? y : x) = v;
    }
}
JDASH_FN JDashEl jdash_el_zero(uint32_t kind) {
    JDashEl e;
    e.kind = kind;
    for (int i = 0; i < 6; i++) e.p[i] = 0.0f;
    return e;
}
JDASH_FN JDashEl jdash_move_el(const JDashSeg& g, double ta) {
    JDashEl e = jdash_el_zero(JDASH_MOVE);
    double x, y;
    jdash_blossom(g, ta, ta, ta, &x, &y);
    e.p[0] = (float)x; e.p[1] = (float)y;
    return e;
}
JDASH_FN JDashEl jdash_curve_el(const JDashSeg& g, double ta, double tb) {
    JDashEl e = jdash_el_zero(g.kind);
    double x, y;
    if (g.kind == JDASH_CUBIC) {
        jdash_blossom(g, ta, ta, tb, &x, &y); e.p[0] = (float)x; e.p[1] = (float)y;
        jdash_blossom(g, ta, tb, tb, &x, &y); e.p[2] = (float)x; e.p[3] = (float)y;
        jdash_blossom(g, tb, tb, tb, &x, &y); e.p[4] = (float)x; e.p[5] = (float)y;
    } else if (g.kind == JDASH_QUAD) {
        jdash_blossom(g, ta, tb, tb, &x, &y); e.p[0] = (float)x; e.p[1] = (float)y;
        jdash_blossom(g, tb, tb, tb, &x, &y); e.p[2] = (float)x; e.p[3] = (float)y;
    } else {
        jdash_blossom(g, tb, tb, tb, &x, &y); e.p[0] = (float)x; e.p[1] = (float)y;
    }
    return e;
}

// ---- what a segment emits ----
// Segment [S, E) of a subpath (S = len.start, E = S + len.q, q > 0) emits, in this order:
//   the lead piece, if S is on: the dash that holds S, from parameter 0 -- preceded by a MoveTo when that dash starts at S
//   (S == 0 included, unless the subpath is merged: then the piece continues the last dash);
//   for every run start a in (S, E): MoveTo(point at a), piece from a to min(run end, E);
//   ClosePath, if the subpath is whole and this is its last segment.
struct JDashSegPlan {
    int64_t first_idx;  // index (jdash_run_by_index) of the first run start in (S, E)
    uint32_t starts;    // run starts in (S, E)
    uint32_t lead;      // 1: there is a lead piece
    uint32_t lead_move; // 1: with a MoveTo
    uint32_t close;     // 1: a ClosePath at the end
    uint32_t relocated; // 1: the lead piece belongs to the merged dash (emitted at the end of the subpath)
    int64_t lead_end;   // lead: where its dash ends
};
JDASH_FN JDashSubInfo jdash_sub_info(const JDashPat& pat, const JDashRun* runs, uint32_t closed, int64_t total) {
    JDashSubInfo si;
    si.total = total; si.bfirst = 0; si.whole = 0u; si.merged = 0u;
    int64_t a, b;
    if (closed && total > 0 && jdash_run_at(pat, runs, 0, &a, &b)) {
        if (b >= total) {
            si.whole = 1u;
        } else {
            int64_t a2, b2;
            if (jdash_run_at(pat, runs, total - 1, &a2, &b2)) {  // the last dash reaches the end
                si.merged = 1u;
                si.bfirst = b;
            }
        }
    }
    return si;
}
JDASH_FN JDashSegPlan jdash_plan(const JDashPat& pat, const JDashRun* runs, const JDashSubInfo& si, const JDashSegLen& len) {
    JDashSegPlan pl;
    pl.first_idx = 0; pl.starts = 0u; pl.lead = 0u; pl.lead_move = 0u; pl.close = 0u; pl.relocated = 0u; pl.lead_end = 0;
    if (len.q <= 0) return pl;
    const int64_t S = len.start, E = len.start + len.q;
    int64_t a, b;
    if (jdash_run_at(pat, runs, S, &a, &b)) {
        pl.lead = 1u;
        pl.lead_end = b;
        pl.lead_move = ((a == S || S == 0) && !(si.merged && S == 0)) ? 1u : 0u;
        pl.relocated = (si.merged && S < si.bfirst) ? 1u : 0u;
    }
    if (pat.n_runs) {
        pl.first_idx = jdash_starts_below(pat, runs, S + 1);
        const int64_t n = jdash_starts_below(pat, runs, E) - pl.first_idx;
        pl.starts = (uint32_t)(n > JDASH_MAX_STARTS ? JDASH_MAX_STARTS : n);
    }
    pl.close = (si.whole && E == si.total) ? 1u : 0u;
    return pl;
}
JDASH_FN uint32_t jdash_plan_count(const JDashSegPlan& pl) { return pl.lead * (1u + pl.lead_move) + 2u * pl.starts + pl.close; }
// Element r (0 <= r < jdash_plan_count) of the segment.
JDASH_FN JDashEl jdash_emit(const JDashSeg& g, const JDashSegLen& len, const JDashPat& pat, const JDashRun* runs, const JDashSegPlan& pl,
                            uint32_t r) {
    const int64_t S = len.start, E = len.start + len.q;
    const uint32_t n_lead = pl.lead * (1u + pl.lead_move);
    if (r < n_lead) {
        if (pl.lead_move && r == 0u) return jdash_move_el(g, 0.0);
        return jdash_curve_el(g, 0.0, pl.lead_end >= E ? 1.0 : jdash_inverse(g, len, pl.lead_end - S));
    }
    r -= n_lead;
    if (r < 2u * pl.starts) {
        int64_t a, b;
        jdash_run_by_index(pat, runs, pl.first_idx + (int64_t)(r >> 1), &a, &b);
        const double ta = jdash_inverse(g, len, a - S);
        if ((r & 1u) == 0u) return jdash_move_el(g, ta);
        return jdash_curve_el(g, ta, b >= E ? 1.0 : jdash_inverse(g, len, b - S));
    }
    return jdash_el_zero(JDASH_CLOSE);
}
// Where element r of a segment goes inside its subpath's output [0, n_sub): `before` = elements of the subpath's earlier
// segments, `reloc_before` = how many of those segments have a relocated lead piece, `reloc_total` = how many the subpath has.
JDASH_FN uint32_t jdash_place(const JDashSegPlan& pl, uint32_t r, uint32_t before, uint32_t reloc_before, uint32_t reloc_total, uint32_t n_sub) {
    if (pl.relocated && r == 0u) return n_sub - reloc_total + reloc_before;
    return before + r - reloc_before - pl.relocated;
}
