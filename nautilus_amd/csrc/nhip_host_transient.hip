// nhip_host_transient.hip -- the transient-returns entry points of the C ABI (kernels: nhip_transient.hip, K19): the spec's
// defaults and its check, the form on the caller's buffers and stream, and the handle form with host poses, host planes and
// host outputs.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

// the accepted ranges of include/nautilus_hip.h
int transient_spec_check(const nhip_transient_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(std::isfinite(s->res) && s->res > 0, "%s: res must be finite and > 0", who);
  NHIP_REQUIRE(s->width >= 1 && s->width <= 16384 && s->height >= 1 && s->height <= 16384,
               "%s: window of %d x %d cells outside 1..16384", who, s->width, s->height);
  NHIP_REQUIRE(s->support_radius >= 0 && s->support_radius <= 4, "%s: support_radius %d outside 0..4", who, s->support_radius);
  NHIP_REQUIRE(s->min_through >= 1 && s->min_through <= (1 << 30), "%s: min_through %d outside 1..2^30", who, s->min_through);
  NHIP_REQUIRE(s->transient_permille >= 0 && s->transient_permille <= 1000, "%s: transient_permille %d outside 0..1000", who,
               s->transient_permille);
  NHIP_REQUIRE(s->flags == 0, "%s: flags %d must be 0", who, s->flags);
  NHIP_REQUIRE(s->reserved == 0, "%s: reserved %d must be 0", who, s->reserved);
  return NHIP_OK;
}

// the arguments have been checked
int transient_run(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, int32_t n_points, const float *d_affines,
                  const nhip_transient_spec_t &spec, const int32_t *d_hits, const int32_t *d_misses, uint8_t *d_labels,
                  float *d_out_xy, int32_t *d_out_offsets, int32_t *d_out_index, int64_t *d_stats, hipStream_t s) {
  TransientParams P;
  P.width = spec.width, P.height = spec.height, P.cell_x0 = spec.cell_x0, P.cell_y0 = spec.cell_y0;
  P.support_radius = spec.support_radius, P.min_through = spec.min_through, P.transient_permille = spec.transient_permille;
  P.n_scans = n_scans, P.n_points = n_points;
  P.res = spec.res, P.inv_res = 1.0 / spec.res;
  P.hits = d_hits, P.misses = d_misses;
  P.labels = d_labels, P.out_xy = reinterpret_cast<float2 *>(d_out_xy), P.out_offsets = d_out_offsets, P.out_index = d_out_index;
  P.stats = reinterpret_cast<long long *>(d_stats);
  P.status = dev_status();
  return launch_transient(P, d_xy, d_offsets, d_affines, s);
}

}  // namespace

extern "C" {

int nhip_transient_spec_default(nhip_transient_spec_t *out) {
  NHIP_REQUIRE(out, "transient_spec_default: null pointer");
  *out = nhip_transient_spec_t{};
  out->res = 0.05;
  out->support_radius = 1;
  out->min_through = 2;
  out->transient_permille = 500;
  return NHIP_OK;
}

int nhip_transient_filter_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, int32_t n_points, const float *d_affines,
                              const nhip_transient_spec_t *spec, const int32_t *d_hits, const int32_t *d_misses, uint8_t *d_labels,
                              float *d_out_xy, int32_t *d_out_offsets, int32_t *d_out_index, int64_t *d_stats, void *stream) {
  int rc = transient_spec_check(spec, "transient_filter_dev");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0, "transient_filter_dev: n_scans %d must be >= 0", n_scans);
  NHIP_REQUIRE(n_points >= 0, "transient_filter_dev: n_points %d must be >= 0", n_points);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_hits && d_misses && d_out_offsets && d_stats && (n_scans == 0 || (d_offsets && d_affines)) &&
                   (n_points == 0 || (d_xy && d_labels && d_out_xy && d_out_index)),
               "transient_filter_dev: null pointer");
  NHIP_REQUIRE(aligned(d_xy, 8) && aligned(d_out_xy, 8) && aligned(d_stats, 8),
               "transient_filter_dev: d_xy, d_out_xy and d_stats must be 8-byte aligned");
  return transient_run(d_xy, d_offsets, n_scans, n_points, d_affines, *spec, d_hits, d_misses, d_labels, d_out_xy, d_out_offsets,
                       d_out_index, d_stats, static_cast<hipStream_t>(stream));
}

int nhip_transient_filter(const nhip_scans_t *scans, const double *poses, const nhip_transient_spec_t *spec, const int32_t *hits,
                          const int32_t *misses, uint8_t *labels, float *out_xy, int32_t *out_offsets, int32_t *out_index,
                          int64_t *stats) {
  int rc = transient_spec_check(spec, "transient_filter");
  if (rc || (rc = require_device())) return rc;
  NHIP_REQUIRE(scans && hits && misses && out_offsets && stats && (scans->n_scans == 0 || poses), "transient_filter: bad arguments");
  NHIP_REQUIRE(scans->n_points >= 0 && scans->n_points <= INT32_MAX, "transient_filter: the handle holds more than 2^31 - 1 points");
  const int32_t n = scans->n_scans, np = (int32_t)scans->n_points;
  NHIP_REQUIRE(np == 0 || (labels && out_xy && out_index), "transient_filter: null output");
  const size_t cells = (size_t)spec->width * (size_t)spec->height;
  std::vector<float> aff(4 * (size_t)n);
  if ((rc = nhip_map_pose_affines(poses, n, aff.data()))) return rc;
  Staged st;
  const float *da = st.in(aff.data(), aff.size());
  const int32_t *dh = st.in(hits, cells), *dm = st.in(misses, cells);
  uint8_t *dl = st.out<uint8_t>((size_t)np);
  float *dx = st.out<float>(2 * (size_t)np);
  int32_t *doff = st.out<int32_t>((size_t)n + 1), *di = st.out<int32_t>((size_t)np);
  int64_t *ds = st.out<int64_t>(STATS_WORDS);
  if (st.ok())
    st.launched(transient_run(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), n, np, da, *spec, dh, dm, dl, dx, doff,
                              di, ds, nullptr));
  st.fetch(out_offsets, doff, (size_t)n + 1);
  st.fetch(stats, ds, STATS_WORDS);
  const size_t kept = st.ok() && out_offsets[n] > 0 ? (size_t)out_offsets[n] : 0;  // (<= np: the offsets kernel cuts it there)
  st.fetch(labels, dl, (size_t)np);
  st.fetch(out_xy, dx, 2 * kept);
  st.fetch(out_index, di, kept);
  return st.finish();
}

}  // extern "C"
