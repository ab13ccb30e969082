// dash.h -- dashing a path on the host (DESIGN.md 5.6 "Dash rule"; the reference calls the third-party curve.Dash at
// scene.go:169-177, this project defines the result itself).
#pragma once
#include <cstdint>
#include <vector>

#include "gfx.h"
#include "jello_dash_host.h"

namespace jello {

// The dashes of `path` as one path of MoveTo + sub-curves per dash (coordinates exactly representable in binary32).
// Throws std::invalid_argument for every input the rule rejects; an empty pattern is one of them (it is not dashing).
BezPath dash(const BezPath& path, const std::vector<double>& pattern, double offset);

// The same for a prepared batch (jdash_prepare): all elements, and optionally the n_paths + 1 exclusive offsets per path.
std::vector<JDashEl> dash_job(const JDashJob& job, std::vector<uint32_t>* index);

}  // namespace jello
