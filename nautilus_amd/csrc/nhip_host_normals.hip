// nhip_host_normals.hip -- the scan-normal entry points of the C ABI (kernels: nhip_normals.hip): the spec's defaults and
// its check, the `_dev` form, the handle form.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

// the accepted ranges of include/nautilus_hip.h; *limit: the sample limit's second term, SampleLimit (normal_computation.cc:39-41)
static int normals_spec_check(const nhip_normals_spec_t *s, const char *who, int32_t *limit) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(std::isfinite(s->neighborhood_size) && s->neighborhood_size > 0, "%s: neighborhood_size must be finite and > 0", who);
  NHIP_REQUIRE(std::isfinite(s->neighborhood_step_size) && s->neighborhood_step_size > 0,
               "%s: neighborhood_step_size must be finite and > 0", who);
  NHIP_REQUIRE(std::isfinite(s->mean_distance) && s->mean_distance > 0, "%s: mean_distance must be finite and > 0", who);
  NHIP_REQUIRE(s->bin_number >= 2 && s->bin_number <= NHIP_NORMALS_MAX_BINS, "%s: bin_number %d outside 2..%d", who, s->bin_number,
               NHIP_NORMALS_MAX_BINS);
  NHIP_REQUIRE(s->max_growth_steps >= 0 && s->max_growth_steps <= 1024, "%s: max_growth_steps %d outside 0..1024", who,
               s->max_growth_steps);
  const double term = 1 / (2.0 * s->mean_distance * s->mean_distance);  // (as the reference writes it: 49.99.. for 0.1)
  NHIP_REQUIRE(term >= 1.0 && term < (double)NHIP_NORMALS_MAX_SAMPLES + 1.0,
               "%s: mean_distance %g gives a sample limit of %g, outside 1..%d", who, s->mean_distance, std::floor(term),
               NHIP_NORMALS_MAX_SAMPLES);
  *limit = (int32_t)(size_t)term;
  return NHIP_OK;
}

extern "C" {

int nhip_normals_spec_default(nhip_normals_spec_t *out) {
  NHIP_REQUIRE(out, "normals_spec_default: null pointer");
  // nc_neighborhood_size, nc_neighborhood_step_size, nc_mean_distance, nc_bin_number (config/default_config.lua:147-156)
  out->neighborhood_size = 0.15;
  out->neighborhood_step_size = 0.1;
  out->mean_distance = 0.1;
  out->bin_number = 32;
  out->max_growth_steps = 32;
  out->seed = 1u;
  out->flags = 0;
  return NHIP_OK;
}

int nhip_normals_estimate_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_normals_spec_t *spec,
                              float *d_normals, int32_t *d_info, void *stream) {
  int32_t limit = 0;
  int rc = normals_spec_check(spec, "normals_estimate_dev", &limit);  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0, "normals_estimate_dev: n_scans < 0");
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(n_scans == 0 || (d_xy && d_offsets && d_normals), "normals_estimate_dev: null pointer");
  return launch_normals_estimate(d_xy, d_offsets, n_scans, *spec, limit, d_normals, d_info, static_cast<hipStream_t>(stream));
}

int nhip_normals_estimate(const nhip_scans_t *scans, const nhip_normals_spec_t *spec, float *normals, int32_t *info) {
  int32_t limit = 0;
  int rc = normals_spec_check(spec, "normals_estimate", &limit);
  if (rc) return rc;
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(scans && (scans->n_points == 0 || normals), "normals_estimate: bad arguments");
  if (scans->n_scans == 0 || scans->n_points == 0) return NHIP_OK;
  const size_t np = (size_t)scans->n_points;
  Staged st;
  float *dn = st.out<float>(2 * np);
  int32_t *di = info ? st.out<int32_t>(4 * np) : nullptr;  // (null: the kernel keeps no info)
  if (st.ok())
    st.launched(launch_normals_estimate(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), scans->n_scans, *spec, limit,
                                        dn, di, nullptr));
  st.fetch(normals, dn, 2 * np);
  st.fetch(info, di, 4 * np);
  return st.finish();
}

}  // extern "C"
