// jello_dash_host.h -- the host half of the dash rule: validation, the walk from path elements to drawn
// segments and subpaths, and a pattern's quantised "on" runs.  Integer work and copies only -- every length and every split
// comes from jello_dash.h.  Used by the host route (jello_amd/host/dash.cpp) and by jh_dash (jello_amd/csrc/jello_hip.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "jello_dash.h"

struct JDashInEl {  // = jh_dash_el = capi.cpp's jl_path_el
    int32_t kind, pad;
    double pts[6];
};
struct JDashInPath {  // = jh_dash_path
    uint32_t first_el, n_els, first_dash, n_dash;
    double offset;
};

struct JDashJob {
    std::vector<JDashSeg> segs;
    std::vector<JDashSub> subs;
    std::vector<JDashPat> pats;  // one per path
    std::vector<JDashRun> runs;
    std::vector<uint32_t> path_first_seg;  // n_paths + 1
};

// One pattern + offset -> period, phase and runs (appended to `runs`).  nullptr, or why the input is rejected.
inline const char* jdash_make_pattern(const double* d, uint32_t n, double offset, std::vector<JDashRun>* runs, JDashPat* out) {
    if (n == 0u || n > JDASH_MAX_PATTERN) return "a dash pattern has 1 to 64 entries";
    if (!std::isfinite(offset) || std::fabs(offset) > JDASH_OFFSET_LIMIT) return "dash offset is not finite, or beyond 2^40";
    int64_t q[2 * JDASH_MAX_PATTERN];
    for (uint32_t i = 0; i < n; i++) {
        if (!std::isfinite(d[i]) || d[i] < 0.0 || d[i] > JDASH_ENTRY_LIMIT) return "a dash pattern entry is negative, not finite, or above 2^30";
        q[i] = jdash_quantise(d[i], 1048576.0);
    }
    uint32_t m = n;
    if (n & 1u) {  // an odd pattern keeps alternating: two cycles make its period
        for (uint32_t i = 0; i < n; i++) q[n + i] = q[i];
        m = 2u * n;
    }
    int64_t period = 0;
    for (uint32_t i = 0; i < m; i++) period += q[i];
    if (period == 0) return "the dash pattern's quantised period is 0";
    out->period = period;
    out->phase = jdash_quantise(offset, 1048576.0) - jdash_floordiv(jdash_quantise(offset, 1048576.0), period) * period;
    out->first_run = (uint32_t)runs->size();
    out->solid = 0u;
    out->pad = 0u;
    int64_t pos = 0;
    for (uint32_t i = 0; i < m; i += 2u) {
        if (q[i] > 0) {
            if (runs->size() > out->first_run && runs->back().start + runs->back().len == pos) runs->back().len += q[i];
            else runs->push_back(JDashRun{pos, q[i]});
        }
        pos += q[i] + q[i + 1];
    }
    uint32_t nr = (uint32_t)runs->size() - out->first_run;
    if (nr >= 1u) {
        JDashRun& first = (*runs)[out->first_run];
        JDashRun& last = runs->back();
        if (first.start == 0 && last.start + last.len == period) {
            if (nr == 1u) {  // on everywhere
                out->solid = 1u;
                runs->pop_back();
            } else {  // the run across the period's end is one run
                last.len += first.len;
                runs->erase(runs->begin() + out->first_run);
            }
        }
    }
    out->n_runs = (uint32_t)runs->size() - out->first_run;
    return nullptr;
}

// The elements of one path -> drawn segments and subpaths (appended).  MoveTo begins a subpath; a drawing element before the
// first MoveTo, and a ClosePath with no subpath open, are ignored; after a ClosePath the next drawing element begins a subpath
// at the closed one's start.  ClosePath adds the closing line when end != start.  nullptr, or why the input is rejected.
inline const char* jdash_walk_path(const JDashInEl* els, uint32_t n, uint32_t pat, JDashJob* job) {
    bool have_point = false, open = false;
    double start[2] = {0, 0}, cur[2] = {0, 0};
    auto begin_sub = [&]() {
        job->subs.push_back(JDashSub{(uint32_t)job->segs.size(), 0u, pat, 0u});
        open = true;
    };
    auto add_seg = [&](uint32_t kind, const double* pts, int n_pts) {
        if (!open) begin_sub();
        JDashSeg g;
        for (int i = 0; i < 8; i++) g.p[i] = 0.0;
        g.p[0] = cur[0]; g.p[1] = cur[1];
        for (int i = 0; i < 2 * n_pts; i++) g.p[2 + i] = pts[i];
        g.kind = kind;
        g.sub = (uint32_t)job->subs.size() - 1u;
        job->segs.push_back(g);
        job->subs.back().n_segs++;
        cur[0] = pts[2 * n_pts - 2]; cur[1] = pts[2 * n_pts - 1];
    };
    for (uint32_t i = 0; i < n; i++) {
        const JDashInEl& e = els[i];
        const int n_pts = e.kind == JDASH_MOVE || e.kind == JDASH_LINE ? 1 : e.kind == JDASH_QUAD ? 2 : e.kind == JDASH_CUBIC ? 3 : 0;
        if (e.kind < JDASH_MOVE || e.kind > JDASH_CLOSE) return "unknown path element kind";
        for (int k = 0; k < 2 * n_pts; k++)
            if (!std::isfinite(e.pts[k]) || std::fabs(e.pts[k]) > JDASH_COORD_LIMIT) return "a path coordinate is not finite, or beyond 2^20";
        if (e.kind == JDASH_MOVE) {
            start[0] = cur[0] = e.pts[0]; start[1] = cur[1] = e.pts[1];
            have_point = true;
            open = false;
        } else if (e.kind == JDASH_CLOSE) {
            if (open) {
                if (cur[0] != start[0] || cur[1] != start[1]) add_seg(JDASH_LINE, start, 1);
                job->subs.back().closed = 1u;
                open = false;
            }
            cur[0] = start[0]; cur[1] = start[1];
        } else if (have_point) {
            if (!open) { start[0] = cur[0]; start[1] = cur[1]; }
            add_seg((uint32_t)e.kind, e.pts, n_pts);
        }
    }
    return nullptr;
}

// A whole batch.  On rejection `job` is left in an unspecified state and nothing must be done with it.
inline const char* jdash_prepare(const JDashInEl* els, uint64_t n_els, const JDashInPath* paths, uint32_t n_paths, const double* dashes,
                                 uint64_t n_dashes, JDashJob* job) {
    job->segs.clear(); job->subs.clear(); job->pats.clear(); job->runs.clear(); job->path_first_seg.clear();
    for (uint32_t p = 0; p < n_paths; p++) {
        const JDashInPath& d = paths[p];
        if ((uint64_t)d.first_el + d.n_els > n_els) return "a path's elements lie outside the element array";
        if ((uint64_t)d.first_dash + d.n_dash > n_dashes) return "a path's pattern lies outside the pattern array";
        JDashPat pat;
        if (const char* why = jdash_make_pattern(dashes + d.first_dash, d.n_dash, d.offset, &job->runs, &pat)) return why;
        job->pats.push_back(pat);
        job->path_first_seg.push_back((uint32_t)job->segs.size());
        if (const char* why = jdash_walk_path(els + d.first_el, d.n_els, p, job)) return why;
        if (job->segs.size() > 0x7fffffffull) return "more than 2^31 - 1 segments";
    }
    job->path_first_seg.push_back((uint32_t)job->segs.size());
    return nullptr;
}
