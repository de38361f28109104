// nhip_host_refine.hip -- the match refinement's entry points of the C ABI (kernel: nhip_refine.hip, K22): the spec's defaults
// and its check, the start poses, the form on the caller's buffers and stream, the form on host arrays, the transform.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

// thr[k] = (float)max(thr_min, thr0 * shrink^k), the power by repeated products in double (refine.py fills the same values)
void fill_thresholds(nhip_refine_spec_t *s) {
  double v = s->thr0;
  for (int k = 0; k < NHIP_REFINE_THRESHOLDS; k++) {
    s->thr[k] = (float)(v > s->thr_min ? v : s->thr_min);
    v = v * s->shrink;
  }
}

// the accepted ranges of include/nautilus_hip.h
int refine_spec_check(const nhip_refine_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null refine spec", who);
  NHIP_REQUIRE(s->max_iterations >= 1 && s->max_iterations <= NHIP_REFINE_THRESHOLDS, "%s: max_iterations %d outside 1..%d", who,
               s->max_iterations, NHIP_REFINE_THRESHOLDS);
  NHIP_REQUIRE(s->min_corr >= 3, "%s: min_corr %d < 3", who, s->min_corr);
  NHIP_REQUIRE(s->flags == 0 && s->reserved == 0, "%s: flags %d and reserved %d must be 0", who, s->flags, s->reserved);
  NHIP_REQUIRE(s->thr[0] > 0.f && s->thr[0] < 1.0e6f, "%s: thr[0] %g must be positive and below 1e6", who, (double)s->thr[0]);
  for (int k = 1; k < s->max_iterations; k++)
    NHIP_REQUIRE(s->thr[k] > 0.f && s->thr[k] <= s->thr[0], "%s: thr[%d] %g outside (0, thr[0] = %g]: the bucket grid's cells are thr[0]'s",
                 who, k, (double)s->thr[k], (double)s->thr[0]);
  NHIP_REQUIRE(s->step_tol_m >= 0 && s->step_tol_rad >= 0, "%s: negative or NaN step tolerance", who);
  NHIP_REQUIRE(s->min_spread >= 0 && s->max_shift_m >= 0 && s->max_turn_sin >= 0, "%s: negative or NaN min_spread / max_shift_m / max_turn_sin", who);
  return NHIP_OK;
}

RefineParams refine_params(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                           const int32_t *d_pair_src, const int32_t *d_pair_tgt, const double *d_pose0, int32_t n_pairs,
                           const nhip_refine_spec_t &spec, nhip_refined_t *d_out, double *d_trace) {
  RefineParams P;
  memset(&P, 0, sizeof(P));
  P.xy = reinterpret_cast<const float2 *>(d_xy), P.normals = reinterpret_cast<const float2 *>(d_normals);
  P.offsets = d_offsets, P.pair_src = d_pair_src, P.pair_tgt = d_pair_tgt;
  P.pose0 = d_pose0;
  P.out = d_out, P.trace = d_trace;
  P.n_scans = n_scans, P.n_pairs = n_pairs;
  P.status = dev_status();
  P.spec = spec;
  return P;
}

}  // namespace

extern "C" {

int nhip_refine_spec_default(nhip_refine_spec_t *out) {
  NHIP_REQUIRE(out, "refine_spec_default: null pointer");
  *out = nhip_refine_spec_t{};
  out->thr0 = 0.25, out->shrink = 0.5, out->thr_min = 0.05;
  out->step_tol_m = 1e-5, out->step_tol_rad = 1e-5;
  out->min_spread = 0.02, out->max_shift_m = 0.5;
  out->max_turn_sin = sin(5.0 * M_PI / 180.0);
  out->max_iterations = 8, out->min_corr = 30;
  fill_thresholds(out);
  return NHIP_OK;
}

int nhip_refine_start_poses(const nhip_match_t *records, const double *theta0, const int32_t *pair_origin, int32_t n_pairs,
                            const nhip_grid_spec_t *grid_spec, const nhip_search_t *search, double *pose0) {
  NHIP_REQUIRE(grid_spec && search && n_pairs >= 0, "refine_start_poses: bad arguments");
  NHIP_REQUIRE(n_pairs == 0 || (records && theta0 && pose0), "refine_start_poses: null array");
  for (int32_t i = 0; i < n_pairs; i++) {
    const nhip_match_t &m = records[i];
    double *p = pose0 + 4 * (size_t)i;
    if (m.itheta < 0) {
      p[0] = p[1] = p[2] = p[3] = NAN;
      continue;
    }
    const int32_t ox = pair_origin ? pair_origin[2 * (size_t)i] : 0, oy = pair_origin ? pair_origin[2 * (size_t)i + 1] : 0;
    const double theta = theta0[i] + (double)(m.itheta - (search->n_theta - 1) / 2) * search->theta_step;
    p[0] = cos(theta);
    p[1] = sin(theta);
    p[2] = (double)(ox + m.ix - (search->nx - 1) / 2) * grid_spec->res;
    p[3] = (double)(oy + m.iy - (search->ny - 1) / 2) * grid_spec->res;
  }
  return NHIP_OK;
}

int nhip_refine_icp_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                        const int32_t *d_pair_src, const int32_t *d_pair_tgt, const double *d_pose0, int32_t n_pairs,
                        const nhip_refine_spec_t *spec, nhip_refined_t *d_out, double *d_trace, void *stream) {
  int rc = refine_spec_check(spec, "refine_icp_dev");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(n_pairs >= 0 && n_scans >= 0, "refine_icp_dev: n_pairs %d / n_scans %d < 0", n_pairs, n_scans);
  if ((rc = require_device())) return rc;
  if (n_pairs == 0) return NHIP_OK;
  NHIP_REQUIRE(d_xy && d_normals && d_offsets && d_pair_src && d_pair_tgt && d_pose0 && d_out, "refine_icp_dev: null pointer");
  NHIP_REQUIRE(aligned(d_xy, 8) && aligned(d_normals, 8) && aligned(d_pose0, 8) && aligned(d_out, 8) && aligned(d_trace, 8),
               "refine_icp_dev: d_xy, d_normals, d_pose0, d_out and d_trace must be 8-byte aligned");
  return launch_refine_icp(refine_params(d_xy, d_normals, d_offsets, n_scans, d_pair_src, d_pair_tgt, d_pose0, n_pairs, *spec, d_out, d_trace),
                           static_cast<hipStream_t>(stream));
}

int nhip_refine_icp(const float *xy, const float *normals, const int32_t *offsets, int32_t n_scans, const int32_t *pair_src,
                    const int32_t *pair_tgt, const double *pose0, int32_t n_pairs, const nhip_refine_spec_t *spec,
                    nhip_refined_t *out, double *trace) {
  int rc = refine_spec_check(spec, "refine_icp");
  if (rc) return rc;
  NHIP_REQUIRE(n_pairs >= 0 && n_scans >= 0 && offsets, "refine_icp: bad arguments");
  NHIP_REQUIRE(n_pairs == 0 || (pair_src && pair_tgt && pose0 && out), "refine_icp: null array");
  NHIP_REQUIRE(offsets[0] == 0, "refine_icp: offsets[0] = %d", offsets[0]);
  for (int32_t i = 0; i < n_scans; i++)
    NHIP_REQUIRE(offsets[i + 1] >= offsets[i], "refine_icp: offsets decrease at scan %d", i);
  const size_t n_points = (size_t)offsets[n_scans];
  NHIP_REQUIRE(n_points == 0 || (xy && normals), "refine_icp: null cloud");
  for (int32_t i = 0; i < n_pairs; i++)
    NHIP_REQUIRE(pair_src[i] >= 0 && pair_src[i] < n_scans && pair_tgt[i] >= 0 && pair_tgt[i] < n_scans,
                 "refine_icp: pair %d (%d, %d) names a scan outside the %d scans", i, pair_src[i], pair_tgt[i], n_scans);
  if ((rc = require_device())) return rc;
  if (n_pairs == 0) return NHIP_OK;
  const size_t N = (size_t)n_pairs;
  Staged st;
  const float *d_xy = st.in(xy, 2 * n_points), *d_nrm = st.in(normals, 2 * n_points);
  const int32_t *d_off = st.in(offsets, (size_t)n_scans + 1), *d_src = st.in(pair_src, N), *d_tgt = st.in(pair_tgt, N);
  const double *d_pose0 = st.in(pose0, 4 * N);
  nhip_refined_t *d_out = st.out<nhip_refined_t>(N);
  double *d_trace = trace ? st.out<double>(NHIP_REFINE_TRACE_DOUBLES * N) : nullptr;
  if (st.ok())
    st.launched(launch_refine_icp(refine_params(d_xy, d_nrm, d_off, n_scans, d_src, d_tgt, d_pose0, n_pairs, *spec, d_out, d_trace), nullptr));
  st.fetch(out, d_out, N);
  if (trace) st.fetch(trace, d_trace, NHIP_REFINE_TRACE_DOUBLES * N);
  return st.finish();
}

int nhip_refined_to_transform(const nhip_refined_t *r, double *tx, double *ty, double *theta) {
  NHIP_REQUIRE(r, "refined_to_transform: null record");
  if (tx) *tx = r->tx;
  if (ty) *ty = r->ty;
  if (theta) *theta = atan2(r->s, r->c);
  return NHIP_OK;
}

}  // extern "C"
