// nhip_host_features.hip -- the scan-feature entry points of the C ABI (kernels: nhip_feat.hip): the spec's defaults and
// its check, the `_dev` forms, the handle form.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

// the accepted ranges of include/nautilus_hip.h; everything the kernel sizes an array or a loop by
static int feature_spec_check(const nhip_feature_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(s->neighbors_per_side >= 1 && s->neighbors_per_side <= NHIP_FEATURE_MAX, "%s: neighbors_per_side %d outside 1..%d",
               who, s->neighbors_per_side, NHIP_FEATURE_MAX);
  NHIP_REQUIRE(s->min_neighbors >= 1 && s->min_neighbors <= 2 * s->neighbors_per_side - 1,
               "%s: min_neighbors %d outside 1..%d (a point has at most 2 * neighbors_per_side - 1 neighbours)", who, s->min_neighbors,
               2 * s->neighbors_per_side - 1);
  NHIP_REQUIRE(s->max_planar >= 1 && s->max_planar <= NHIP_FEATURE_MAX, "%s: max_planar %d outside 1..%d", who, s->max_planar,
               NHIP_FEATURE_MAX);
  NHIP_REQUIRE(s->max_edge >= 1 && s->max_edge <= NHIP_FEATURE_MAX, "%s: max_edge %d outside 1..%d", who, s->max_edge, NHIP_FEATURE_MAX);
  NHIP_REQUIRE(std::isfinite(s->threshold), "%s: threshold is not finite", who);
  NHIP_REQUIRE(std::isfinite(s->distance_threshold) && s->distance_threshold >= 0, "%s: distance_threshold must be finite and >= 0", who);
  NHIP_REQUIRE(std::isfinite(s->max_neighbor_distance) && s->max_neighbor_distance >= 0,
               "%s: max_neighbor_distance must be finite and >= 0", who);
  return NHIP_OK;
}

extern "C" {

int nhip_feature_spec_default(nhip_feature_spec_t *out) {
  NHIP_REQUIRE(out, "feature_spec_default: null pointer");
  // FeatureExtractor(pointcloud, 0.008, 2.0, 10, 10, 20, 10): threshold, distance_threshold, neighbor_num, max_edge_num,
  // max_planar_num, min_neighbor_num (slam_types.h:66-67); max_neighbor_distance_ = 0.8 (feature_extracter.h:28)
  out->threshold = 0.008;
  out->distance_threshold = 2.0;
  out->max_neighbor_distance = 0.8;
  out->neighbors_per_side = 10;
  out->min_neighbors = 10;
  out->max_planar = 20;
  out->max_edge = 10;
  return NHIP_OK;
}

int nhip_features_extract_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_feature_spec_t *spec,
                              int32_t *d_planar_idx, int32_t *d_planar_count, int32_t *d_edge_idx, int32_t *d_edge_count,
                              double *d_scores, void *stream) {
  int rc = feature_spec_check(spec, "features_extract_dev");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(n_scans >= 0, "features_extract_dev: n_scans < 0");
  NHIP_REQUIRE(n_scans == 0 || (d_xy && d_offsets && d_planar_idx && d_planar_count && d_edge_idx && d_edge_count),
               "features_extract_dev: null pointer");
  return launch_feat_extract(d_xy, d_offsets, n_scans, *spec, d_planar_idx, d_planar_count, d_edge_idx, d_edge_count, d_scores,
                             static_cast<hipStream_t>(stream));
}

int nhip_features_pack_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                           const int32_t *d_idx, const int32_t *d_count, int32_t cap, float *d_xy_out, float *d_normals_out,
                           int32_t *d_offsets_out, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0 && n_scans <= 0x7fffffff / NHIP_FEATURE_MAX, "features_pack_dev: n_scans %d outside 0..%d", n_scans,
               0x7fffffff / NHIP_FEATURE_MAX);
  NHIP_REQUIRE(cap >= 1 && cap <= NHIP_FEATURE_MAX, "features_pack_dev: cap %d outside 1..%d", cap, NHIP_FEATURE_MAX);
  NHIP_REQUIRE(d_offsets_out && (n_scans == 0 || (d_xy && d_offsets && d_idx && d_count && d_xy_out)), "features_pack_dev: null pointer");
  NHIP_REQUIRE(!d_normals || d_normals_out, "features_pack_dev: d_normals without d_normals_out");
  return launch_feat_pack(d_xy, d_normals, d_offsets, n_scans, d_idx, d_count, cap, d_xy_out, d_normals_out, d_offsets_out,
                          static_cast<hipStream_t>(stream));
}

int nhip_features_extract(const nhip_scans_t *scans, const nhip_feature_spec_t *spec, int32_t *planar_idx, int32_t *planar_count,
                          int32_t *edge_idx, int32_t *edge_count, double *scores) {
  int rc = feature_spec_check(spec, "features_extract");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(scans && (scans->n_scans == 0 || (planar_idx && planar_count && edge_idx && edge_count)), "features_extract: bad arguments");
  if (scans->n_scans == 0) return NHIP_OK;
  const size_t N = (size_t)scans->n_scans, np = N * (size_t)spec->max_planar, ne = N * (size_t)spec->max_edge;
  const size_t pts = (size_t)scans->n_points;
  Staged st;
  int32_t *dpi = st.out<int32_t>(np), *dpc = st.out<int32_t>(N), *dei = st.out<int32_t>(ne), *dec = st.out<int32_t>(N);
  double *dsc = scores && pts ? st.out<double>(pts) : nullptr;  // (null: the kernel keeps no scores)
  if (st.ok())
    st.launched(launch_feat_extract(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), scans->n_scans, *spec, dpi, dpc,
                                    dei, dec, dsc, nullptr));
  st.fetch(planar_idx, dpi, np);
  st.fetch(planar_count, dpc, N);
  st.fetch(edge_idx, dei, ne);
  st.fetch(edge_count, dec, N);
  st.fetch(scores, dsc, pts);
  return st.finish();
}

}  // extern "C"
