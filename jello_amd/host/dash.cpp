// dash.cpp -- the host route of the dash rule: the sequential driver over include/jello_dash.h.  It runs the
// passes of the device stage (jh_dash, csrc/kernels_dash.hip) one after the other -- lengths, positions, per-segment plans,
// one call of jdash_emit per output element -- so both produce the same words; tests/dash_ref.py is the independent restatement.
#include "dash.h"

#include <stdexcept>
#include <string>

#include "jello_dash_host.h"

namespace jello {

std::vector<JDashEl> dash_job(const JDashJob& job, std::vector<uint32_t>* index) {
    const size_t n_segs = job.segs.size();
    std::vector<JDashSegLen> lens(n_segs);
    std::vector<JDashSegPlan> plans(n_segs);
    std::vector<uint32_t> base(n_segs + 1, 0u);
    std::vector<JDashSubInfo> infos(job.subs.size());
    for (size_t i = 0; i < n_segs; i++) jdash_measure(job.segs[i], &lens[i]);
    for (size_t s = 0; s < job.subs.size(); s++) {
        const JDashSub& sub = job.subs[s];
        int64_t pos = 0;
        for (uint32_t i = sub.first_seg; i < sub.first_seg + sub.n_segs; i++) {
            lens[i].start = pos;
            pos += lens[i].q;
        }
        infos[s] = jdash_sub_info(job.pats[sub.pat], job.runs.data(), sub.closed, pos);
    }
    for (size_t i = 0; i < n_segs; i++) {
        const JDashSub& sub = job.subs[job.segs[i].sub];
        plans[i] = jdash_plan(job.pats[sub.pat], job.runs.data(), infos[job.segs[i].sub], lens[i]);
        base[i + 1] = base[i] + jdash_plan_count(plans[i]);
    }
    std::vector<JDashEl> out(base[n_segs]);
    for (size_t s = 0; s < job.subs.size(); s++) {
        const JDashSub& sub = job.subs[s];
        const uint32_t first = sub.first_seg, end = sub.first_seg + sub.n_segs;
        uint32_t reloc_total = 0u;
        for (uint32_t i = first; i < end; i++) reloc_total += plans[i].relocated;
        uint32_t reloc_before = 0u;
        for (uint32_t i = first; i < end; i++) {
            const uint32_t n = base[i + 1] - base[i];
            for (uint32_t r = 0; r < n; r++)
                out[base[first] + jdash_place(plans[i], r, base[i] - base[first], reloc_before, reloc_total, base[end] - base[first])] =
                    jdash_emit(job.segs[i], lens[i], job.pats[sub.pat], job.runs.data(), plans[i], r);
            reloc_before += plans[i].relocated;
        }
    }
    if (index) {
        index->clear();
        for (uint32_t f : job.path_first_seg) index->push_back(base[f]);
    }
    return out;
}

static JDashInEl to_in(const PathEl& e) {
    JDashInEl r;
    r.kind = (int32_t)e.kind; r.pad = 0;
    r.pts[0] = e.p0[0]; r.pts[1] = e.p0[1]; r.pts[2] = e.p1[0]; r.pts[3] = e.p1[1]; r.pts[4] = e.p2[0]; r.pts[5] = e.p2[1];
    return r;
}

BezPath dash(const BezPath& path, const std::vector<double>& pattern, double offset) {
    std::vector<JDashInEl> els;
    els.reserve(path.size());
    for (const PathEl& e : path) els.push_back(to_in(e));
    JDashInPath d{0u, (uint32_t)els.size(), 0u, (uint32_t)pattern.size(), offset};
    JDashJob job;
    if (pattern.size() > JDASH_MAX_PATTERN) throw std::invalid_argument("dash: a dash pattern has 1 to 64 entries");
    if (const char* why = jdash_prepare(els.data(), els.size(), &d, 1u, pattern.data(), pattern.size(), &job))
        throw std::invalid_argument(std::string("dash: ") + why);
    std::vector<JDashEl> out = dash_job(job, nullptr);
    BezPath r;
    r.reserve(out.size());
    for (const JDashEl& e : out)
        r.push_back(PathEl{(PathElKind)e.kind, {(double)e.p[0], (double)e.p[1]}, {(double)e.p[2], (double)e.p[3]}, {(double)e.p[4], (double)e.p[5]}});
    return r;
}

}  // namespace jello
