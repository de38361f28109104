// nhip_host_occupancy.hip -- the occupancy-grid entry points of the C ABI (kernels: nhip_occupancy.hip, K14): the spec's
// defaults and its check, the form on the caller's buffers and stream, and the handle form with host poses and host outputs.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

// the accepted ranges of include/nautilus_hip.h
int occupancy_spec_check(const nhip_occupancy_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(std::isfinite(s->res) && s->res > 0, "%s: res must be finite and > 0", who);
  NHIP_REQUIRE(s->width >= 1 && s->width <= 16384 && s->height >= 1 && s->height <= 16384,
               "%s: window of %d x %d cells outside 1..16384", who, s->width, s->height);
  NHIP_REQUIRE(s->max_ray_cells >= 1 && s->max_ray_cells <= 4096, "%s: max_ray_cells %d outside 1..4096", who, s->max_ray_cells);
  NHIP_REQUIRE(s->min_obs >= 1 && s->min_obs <= (1 << 30), "%s: min_obs %d outside 1..2^30", who, s->min_obs);
  NHIP_REQUIRE(s->occ_permille >= 1 && s->occ_permille <= 1000, "%s: occ_permille %d outside 1..1000", who, s->occ_permille);
  NHIP_REQUIRE(s->free_permille >= 0 && s->free_permille < s->occ_permille, "%s: free_permille %d outside 0..occ_permille - 1 = %d",
               who, s->free_permille, s->occ_permille - 1);
  NHIP_REQUIRE(s->flags == 0 || s->flags == NHIP_OCC_ACCUMULATE, "%s: flags %d: 0 or NHIP_OCC_ACCUMULATE", who, s->flags);
  NHIP_REQUIRE(s->reserved == 0, "%s: reserved %d must be 0", who, s->reserved);
  return NHIP_OK;
}

// the arguments have been checked
int occupancy_run(const float *d_xy, const int32_t *d_offsets, const float *d_affines, int32_t n_scans,
                  const nhip_occupancy_spec_t &spec, int32_t *d_hits, int32_t *d_misses, int8_t *d_grid, int64_t *d_stats,
                  hipStream_t s) {
  OccParams P;
  P.width = spec.width, P.height = spec.height, P.cell_x0 = spec.cell_x0, P.cell_y0 = spec.cell_y0;
  P.max_ray_cells = spec.max_ray_cells, P.min_obs = spec.min_obs, P.occ_permille = spec.occ_permille, P.free_permille = spec.free_permille;
  P.n_scans = n_scans;
  P.res = spec.res, P.inv_res = 1.0 / spec.res;
  P.hits = d_hits, P.misses = d_misses, P.grid = d_grid;
  P.stats = reinterpret_cast<long long *>(d_stats);
  P.status = dev_status();
  return launch_occupancy(P, !(spec.flags & NHIP_OCC_ACCUMULATE), d_xy, d_offsets, d_affines, s);
}

}  // namespace

extern "C" {

int nhip_occupancy_spec_default(nhip_occupancy_spec_t *out) {
  NHIP_REQUIRE(out, "occupancy_spec_default: null pointer");
  *out = nhip_occupancy_spec_t{};
  out->res = 0.05;
  out->max_ray_cells = 640;
  out->min_obs = 1;
  out->occ_permille = 650;
  out->free_permille = 196;
  return NHIP_OK;
}

int nhip_occupancy_dev(const float *d_xy, const int32_t *d_offsets, const float *d_affines, int32_t n_scans,
                       const nhip_occupancy_spec_t *spec, int32_t *d_hits, int32_t *d_misses, int8_t *d_grid, int64_t *d_stats,
                       void *stream) {
  int rc = occupancy_spec_check(spec, "occupancy_dev");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0, "occupancy_dev: n_scans %d must be >= 0", n_scans);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_hits && d_misses && d_grid && d_stats && (n_scans == 0 || (d_xy && d_offsets && d_affines)),
               "occupancy_dev: null pointer");
  NHIP_REQUIRE(aligned(d_hits, 16) && aligned(d_misses, 16) && aligned(d_grid, 4) && aligned(d_stats, 8),
               "occupancy_dev: d_hits and d_misses must be 16-byte aligned, d_grid 4-byte, d_stats 8-byte");
  return occupancy_run(d_xy, d_offsets, d_affines, n_scans, *spec, d_hits, d_misses, d_grid, d_stats, static_cast<hipStream_t>(stream));
}

int nhip_occupancy(const nhip_scans_t *scans, const double *poses, const nhip_occupancy_spec_t *spec, int32_t *hits,
                   int32_t *misses, int8_t *grid, int64_t *stats) {
  int rc = occupancy_spec_check(spec, "occupancy");
  if (rc || (rc = require_device())) return rc;
  NHIP_REQUIRE(scans && hits && misses && grid && stats && (scans->n_scans == 0 || poses), "occupancy: bad arguments");
  const int32_t n = scans->n_scans;
  const size_t cells = (size_t)spec->width * (size_t)spec->height;
  const bool keep = spec->flags & NHIP_OCC_ACCUMULATE;  // (the planes given are uploaded and added to)
  std::vector<float> aff(4 * (size_t)n);
  if ((rc = nhip_map_pose_affines(poses, n, aff.data()))) return rc;
  Staged st;
  const float *da = st.in(aff.data(), aff.size());
  int32_t *dh = st.inout(keep ? hits : nullptr, cells), *dm = st.inout(keep ? misses : nullptr, cells);
  int8_t *dg = st.out<int8_t>(cells + 4);  // (the kernel writes the grid in words)
  int64_t *ds = st.out<int64_t>(STATS_WORDS);
  if (st.ok())
    st.launched(occupancy_run(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), da, n, *spec, dh, dm, dg, ds, nullptr));
  st.fetch(hits, dh, cells);
  st.fetch(misses, dm, cells);
  st.fetch(grid, dg, cells);
  st.fetch(stats, ds, STATS_WORDS);
  return st.finish();
}

}  // extern "C"
