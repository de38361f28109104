// vectorize_hip.h -- the vector map of Solver::Vectorize (solver.cc:581-624) from the clouds and the solved poses:
//   std::vector<LineSegment> nautilus_hip::VectorizeMap(scans, poses, spec)
// in place of the merge of every TransformPointcloud(...) and VectorMaps::ExtractLines (third_party/vector_maps: absent from
// the reference tree).  Header-only; link with -lnautilus_hip.  The whole step runs on the MI355X through the C ABI
// (nhip_vectorize, the handle form; nautilus_hip.h); there is no CPU path: a failure throws std::runtime_error carrying
// nhip_last_error().  The method is build-defined ("Map vectorisation"): an exhaustive integer Hough
// transform over the occupied cells of a world raster, deterministic.  The segments are what io::WriteMapLines takes.
#ifndef NAUTILUS_HIP_VECTORIZE_H_
#define NAUTILUS_HIP_VECTORIZE_H_

#include <algorithm>
#include <array>
#include <cmath>
#include <stdexcept>
#include <vector>

#include "CorrelativeScanMatcher.h"  // (Vec2f, Check, ScansHandle)
#include "nautilus_hip_io.h"         // (io::LineSegment)

namespace nautilus_hip {

using LineSegment = io::LineSegment;

// the defaults (res 0.05, band 1.5 cells, min_hits 2, 360 directions, ...) on the smallest window that holds every pose
// +- range metres (the scanner's range): what a caller without wishes of its own passes as `spec`
inline nhip_vectorize_spec_t VectorizeSpec(const std::vector<std::array<double, 3>> &poses, double range = 30.0) {
  nhip_vectorize_spec_t s;
  Check(nhip_vectorize_spec_default(&s), "nhip_vectorize_spec_default");
  if (poses.empty()) {
    s.width = s.height = 1;
    return s;
  }
  double lo[2] = {poses[0][0], poses[0][1]}, hi[2] = {poses[0][0], poses[0][1]};
  for (const auto &p : poses)
    for (int k = 0; k < 2; k++) {
      lo[k] = std::min(lo[k], p[k]);
      hi[k] = std::max(hi[k], p[k]);
    }
  const double x0 = std::floor((lo[0] - range) / s.res), y0 = std::floor((lo[1] - range) / s.res);
  s.cell_x0 = (int32_t)x0;
  s.cell_y0 = (int32_t)y0;
  s.width = (int32_t)(std::floor((hi[0] + range) / s.res) - x0) + 1;
  s.height = (int32_t)(std::floor((hi[1] + range) / s.res) - y0) + 1;
  return s;
}

// scans[i] is node i's cloud in its own frame, poses[i] its (x, y, theta).  stats (may be null): the call's 8 counters
// {cells, segments, rounds, flag, cells emitted, cells retired, n_rho, 0}; flag 2: max_segments was too small
inline std::vector<LineSegment> VectorizeMap(const std::vector<std::vector<Vec2f>> &scans,
                                             const std::vector<std::array<double, 3>> &poses, const nhip_vectorize_spec_t &spec,
                                             int32_t *stats = nullptr) {
  if (scans.size() != poses.size()) throw std::runtime_error("VectorizeMap: one pose per scan");
  std::vector<const std::vector<Vec2f> *> ptrs;
  for (const auto &c : scans) ptrs.push_back(&c);
  const ScansHandle handle(ptrs);
  std::vector<double> flat(3 * poses.size() + 3);
  for (size_t i = 0; i < poses.size(); i++)
    for (int k = 0; k < 3; k++) flat[3 * i + k] = poses[i][k];
  const int64_t window = (int64_t)spec.width * spec.height;
  const int32_t max_cells = (int32_t)std::min<int64_t>(window, (int64_t)1 << 26);
  std::vector<int64_t> records(10 * (size_t)std::max(spec.max_segments, 1));
  int32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  Check(nhip_vectorize(handle.h, flat.data(), &spec, max_cells, INT32_MAX, 8, records.data(), st), "nhip_vectorize");
  if (stats) std::copy(st, st + 8, stats);
  if (st[3] == 3) throw std::runtime_error("VectorizeMap: more occupied cells than the window was given room for");
  std::vector<float> lines(4 * (size_t)std::max(st[1], 1));
  Check(nhip_vectorize_endpoints(&spec, records.data(), st[1], lines.data()), "nhip_vectorize_endpoints");
  std::vector<LineSegment> out((size_t)st[1]);
  for (size_t i = 0; i < out.size(); i++) out[i] = LineSegment{lines[4 * i], lines[4 * i + 1], lines[4 * i + 2], lines[4 * i + 3]};
  return out;
}

}  // namespace nautilus_hip

#endif  // NAUTILUS_HIP_VECTORIZE_H_
