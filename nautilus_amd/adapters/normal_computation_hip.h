// normal_computation_hip.h -- drop-in for src/input/normal_computation.h as nautilus uses it:
//   std::vector<Eigen::Vector2f> nautilus::NormalComputation::GetNormals(const std::vector<Eigen::Vector2f>& points)
// (called from KDTree::EigenToKD, kdtree.cc:152-163, for every cloud and every feature cloud).  Header-only; link with
// -lnautilus_hip.  The estimate runs on the MI355X through the C ABI (nhip_normals_estimate, nautilus_hip.h); there is no
// CPU path: a failure throws std::runtime_error carrying nhip_last_error().
//
// The method is the reference's randomised Hough vote, stated deterministically ("Scan normals"):
// the same cloud and the same seed give the same normals, whatever else is in the call.  GetNormals is ONE scan per call --
// an upload, a launch and a download each time; a host that has its clouds at hand should call GetNormalsBatch once.
// The nc_* values of the config file go into Spec() before the first call (the defaults are default_config.lua's).
#ifndef NAUTILUS_HIP_NORMAL_COMPUTATION_H_
#define NAUTILUS_HIP_NORMAL_COMPUTATION_H_

#include <vector>

#include "CorrelativeScanMatcher.h"  // (Vec2f, Check, ScansHandle)

namespace nautilus {
namespace NormalComputation {

using Vector2f = nautilus_hip::Vec2f;

// the spec every call uses: neighborhood_size, neighborhood_step_size, mean_distance, bin_number, max_growth_steps, seed
inline nhip_normals_spec_t &Spec() {
  static nhip_normals_spec_t spec = [] {
    nhip_normals_spec_t s;
    nautilus_hip::Check(nhip_normals_spec_default(&s), "nhip_normals_spec_default");
    return s;
  }();
  return spec;
}

// the normals of every cloud, in one launch
inline std::vector<std::vector<Vector2f>> GetNormalsBatch(const std::vector<std::vector<Vector2f>> &clouds) {
  std::vector<const std::vector<Vector2f> *> ptrs;
  size_t total = 0;
  for (const auto &c : clouds) {
    ptrs.push_back(&c);
    total += c.size();
  }
  std::vector<std::vector<Vector2f>> out(clouds.size());
  if (total == 0) return out;
  const nautilus_hip::ScansHandle scans(ptrs);
  std::vector<float> flat(2 * total);
  nautilus_hip::Check(nhip_normals_estimate(scans.h, &Spec(), flat.data(), nullptr), "nhip_normals_estimate");
  size_t at = 0;
  for (size_t i = 0; i < clouds.size(); i++) {
    out[i].reserve(clouds[i].size());
    for (size_t p = 0; p < clouds[i].size(); p++, at++) out[i].push_back(Vector2f(flat[2 * at], flat[2 * at + 1]));
  }
  return out;
}

// Returns a list of normals for the corresponding list of points (the reference's signature)
inline std::vector<Vector2f> GetNormals(const std::vector<Vector2f> &points) {
  return GetNormalsBatch(std::vector<std::vector<Vector2f>>(1, points))[0];
}

}  // namespace NormalComputation
}  // namespace nautilus

#endif  // NAUTILUS_HIP_NORMAL_COMPUTATION_H_
