// nhip_host_solver.hip -- the solver-side entry points of the C ABI: residuals, correspondences, HITL point selection and
// loop-closure gates in their `_dev` and host-buffer forms, the residual batch handle, the all-gather of match records (RCCL, bound at run time).
#include <dlfcn.h>

#include "nhip_common.h"
#include "nhip_host.h"

// the residual batch handle (this unit's alone; the scan and grid handles are in nhip_host.h)
struct nhip_resid_batch {
  nhip::DevBuf corr, corr_block, block_src, block_tgt, consts, poses, res, jsrc, jtgt, jtt;  // (jtt also holds q: nhip_resid_batch_eval_q)
  nhip::DevBuf one_poses, one_consts, one_idx;  // single-block evaluation: 2 poses, 8 constants, {0, 1}
  std::vector<int32_t> h_offsets;
  std::mutex one_mu;
  int kind = 0;
  int32_t n_blocks = 0, n_poses = 0;
  int64_t n_corr = 0;
};

using namespace nhip;

extern "C" {

// ---------------------------------------------------------------- residuals and correspondences, device pointers
int nhip_resid_lidar_dev(int kind, const float *d_corr, const int32_t *d_corr_block,
                         int64_t n_corr, const int32_t *d_block_src, const int32_t *d_block_tgt,
                         int32_t n_blocks, const double *d_poses, int32_t n_poses,
                         double *d_block_consts, double *d_residuals, double *d_jac_src,
                         double *d_jac_tgt, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_corr && d_corr_block && d_block_src && d_block_tgt && d_poses && d_block_consts &&
                   d_residuals,
               "resid_lidar_dev: null pointer");
  return launch_resid_lidar(kind, d_corr, d_corr_block, n_corr, d_block_src, d_block_tgt, n_blocks,
                            d_poses, n_poses, d_block_consts, d_residuals, d_jac_src, d_jac_tgt,
                            static_cast<hipStream_t>(stream));
}

int nhip_resid_lidar_normal_eq_dev(int kind, const float *d_corr, const int32_t *d_block_offsets,
                                   const int32_t *d_block_src, const int32_t *d_block_tgt,
                                   int32_t n_blocks, const double *d_poses, int32_t n_poses,
                                   double *d_block_consts, double *d_out, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_corr && d_block_offsets && d_block_src && d_block_tgt && d_poses && d_block_consts && d_out,
               "resid_lidar_normal_eq_dev: null pointer");
  NHIP_REQUIRE(n_poses >= 0, "resid_lidar_normal_eq_dev: negative size");
  return launch_resid_normal_eq(kind, d_corr, d_block_offsets, d_block_src, d_block_tgt, n_blocks, d_poses, n_poses,
                                d_block_consts, d_out, static_cast<hipStream_t>(stream));
}

int nhip_pose_affines(const double *poses, int32_t n, float *out) {
  NHIP_REQUIRE(poses && out && n >= 0, "pose_affines: bad arguments");
  for (int32_t i = 0; i < n; i++) {
    // entries of PoseArrayToAffine<double>(pose).cast<float>() (slam_util.h:20-28, 37-40)
    out[4 * i + 0] = (float)cos(poses[3 * i + 2]);
    out[4 * i + 1] = (float)sin(poses[3 * i + 2]);
    out[4 * i + 2] = (float)poses[3 * i + 0];
    out[4 * i + 3] = (float)poses[3 * i + 1];
  }
  return NHIP_OK;
}

int nhip_corr_search_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                         const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                         const float *d_pose_aff, float outlier_threshold,
                         const int64_t *d_cap_offsets, float *d_corr_padded, int32_t *d_counts,
                         void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_xy && d_normals && d_offsets && d_block_src && d_block_tgt && d_pose_aff && d_cap_offsets &&
                   d_corr_padded && d_counts,
               "corr_search_dev: null pointer");
  NHIP_REQUIRE(n_blocks >= 0 && n_scans >= 0 && outlier_threshold > 0, "corr_search_dev: bad size or threshold");
  return launch_corr_search(d_xy, d_normals, d_offsets, n_scans, d_block_src, d_block_tgt, n_blocks, d_pose_aff,
                            outlier_threshold, 0.f, false, d_cap_offsets, d_corr_padded, d_counts,
                            static_cast<hipStream_t>(stream));
}

int nhip_corr_search_normals_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                                 const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                                 const float *d_pose_aff, float outlier_threshold, float min_abs_cosine,
                                 const int64_t *d_cap_offsets, float *d_corr_padded, int32_t *d_counts,
                                 void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_xy && d_normals && d_offsets && d_block_src && d_block_tgt && d_pose_aff && d_cap_offsets &&
                   d_corr_padded && d_counts,
               "corr_search_normals_dev: null pointer");
  NHIP_REQUIRE(n_blocks >= 0 && n_scans >= 0 && outlier_threshold > 0, "corr_search_normals_dev: bad size or threshold");
  NHIP_REQUIRE(min_abs_cosine >= 0.f && min_abs_cosine <= 1.f, "corr_search_normals_dev: min_abs_cosine outside [0, 1]");
  return launch_corr_search(d_xy, d_normals, d_offsets, n_scans, d_block_src, d_block_tgt, n_blocks, d_pose_aff,
                            outlier_threshold, min_abs_cosine, true, d_cap_offsets, d_corr_padded, d_counts,
                            static_cast<hipStream_t>(stream));
}

int nhip_corr_compact_dev(const float *d_corr_padded, const int64_t *d_cap_offsets,
                          const int32_t *d_counts, int32_t n_blocks, int32_t *d_block_offsets,
                          float *d_corr, int32_t *d_corr_block, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_corr_padded && d_cap_offsets && d_counts && d_block_offsets && d_corr && d_corr_block,
               "corr_compact_dev: null pointer");
  NHIP_REQUIRE(n_blocks >= 0, "corr_compact_dev: n_blocks < 0");
  return launch_corr_compact(d_corr_padded, d_cap_offsets, d_counts, n_blocks, d_block_offsets, d_corr,
                             d_corr_block, static_cast<hipStream_t>(stream));
}

int nhip_resid_point_to_line_dev(const float *d_segments, const float *d_points,
                                 const int32_t *d_point_block, int64_t n_points,
                                 const int32_t *d_block_pose, const int32_t *d_block_line,
                                 int32_t n_blocks, const double *d_poses, int32_t n_poses,
                                 const double *d_line_poses, int32_t n_line_poses, double *d_residuals,
                                 double *d_jac_pose, double *d_jac_line, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_segments && d_points && d_point_block && d_block_pose && d_block_line && d_poses &&
                   d_line_poses && d_residuals,
               "resid_point_to_line_dev: null pointer");
  return launch_resid_point_to_line(d_segments, d_points, d_point_block, n_points, d_block_pose,
                                    d_block_line, n_blocks, d_poses, n_poses, d_line_poses, n_line_poses, d_residuals,
                                    d_jac_pose, d_jac_line, static_cast<hipStream_t>(stream));
}

int nhip_resid_point_to_line_normal_eq_dev(const float *d_segments, const float *d_points, const int32_t *d_block_offsets,
                                           const int32_t *d_block_pose, const int32_t *d_block_line, int32_t n_blocks,
                                           const double *d_poses, int32_t n_poses, const double *d_line_poses,
                                           int32_t n_line_poses, double *d_out, void *stream) {
  // (sizes are an argument error with or without a device)
  NHIP_REQUIRE(n_blocks >= 0 && n_poses >= 0 && n_line_poses >= 0, "resid_point_to_line_normal_eq_dev: negative size");
  int rc = require_device();
  if (rc) return rc;
  if (n_blocks == 0) return NHIP_OK;
  NHIP_REQUIRE(d_segments && d_points && d_block_offsets && d_block_pose && d_block_line && d_poses && d_line_poses && d_out,
               "resid_point_to_line_normal_eq_dev: null pointer");
  return launch_resid_point_to_line_normal_eq(d_segments, d_points, d_block_offsets, d_block_pose, d_block_line, n_blocks, d_poses,
                                              n_poses, d_line_poses, n_line_poses, d_out, static_cast<hipStream_t>(stream));
}

int nhip_resid_odometry_dev(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                            const int32_t *d_pose_j, int32_t n_factors, double translation_weight,
                            double rotation_weight, const double *d_poses, int32_t n_poses, double *d_residuals,
                            double *d_jac_i, double *d_jac_j, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_t_odom && d_r_odom && d_pose_i && d_pose_j && d_poses && d_residuals,
               "resid_odometry_dev: null pointer");
  return launch_resid_odometry(d_t_odom, d_r_odom, d_pose_i, d_pose_j, n_factors,
                               translation_weight, rotation_weight, d_poses, n_poses, d_residuals, d_jac_i,
                               d_jac_j, static_cast<hipStream_t>(stream));
}

int nhip_resid_odometry_normal_eq_dev(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                                      const int32_t *d_pose_j, int32_t n_factors, double translation_weight,
                                      double rotation_weight, const double *d_poses, int32_t n_poses, double *d_out,
                                      void *stream) {
  NHIP_REQUIRE(n_factors >= 0 && n_poses >= 0, "resid_odometry_normal_eq_dev: negative size");
  int rc = require_device();
  if (rc) return rc;
  if (n_factors == 0) return NHIP_OK;
  NHIP_REQUIRE(d_t_odom && d_r_odom && d_pose_i && d_pose_j && d_poses && d_out, "resid_odometry_normal_eq_dev: null pointer");
  return launch_resid_odometry_normal_eq(d_t_odom, d_r_odom, d_pose_i, d_pose_j, n_factors, translation_weight, rotation_weight,
                                         d_poses, n_poses, d_out, static_cast<hipStream_t>(stream));
}

int nhip_resid_odometry_robust_normal_eq_dev(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                                             const int32_t *d_pose_j, int32_t n_factors, double translation_weight,
                                             double rotation_weight, const nhip_loss_spec_t *loss, const double *d_poses,
                                             int32_t n_poses, double *d_out, double *d_weights, void *stream) {
  // (the spec, the sizes and the pointers are an argument error with or without a device)
  int rc = loss_spec_check(loss, "resid_odometry_robust_normal_eq_dev");
  if (rc) return rc;
  NHIP_REQUIRE(n_factors >= 0 && n_poses >= 0, "resid_odometry_robust_normal_eq_dev: negative size (n_factors %d, n_poses %d)",
               n_factors, n_poses);
  NHIP_REQUIRE(d_t_odom && d_r_odom && d_pose_i && d_pose_j && d_poses && d_out,
               "resid_odometry_robust_normal_eq_dev: null pointer (only d_weights may be null)");
  if ((rc = require_device())) return rc;
  return launch_resid_odometry_robust_normal_eq(d_t_odom, d_r_odom, d_pose_i, d_pose_j, n_factors, translation_weight,
                                                rotation_weight, loss->kind, loss->scale, d_poses, n_poses, d_out, d_weights,
                                                static_cast<hipStream_t>(stream));
}

int nhip_resid_relpose_dev(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                           int32_t n_factors, const double *d_poses, int32_t n_poses, double *d_residuals, double *d_jac_i,
                           double *d_jac_j, double *d_parts, int32_t *d_flags, void *stream) {
  // (the sizes and the pointers are an argument error with or without a device)
  int rc = relpose_args_check(d_z, d_info, d_pose_i, d_pose_j, n_factors, d_poses, n_poses, d_residuals, "resid_relpose_dev");
  if (rc) return rc;
  if ((rc = require_device())) return rc;
  return launch_resid_relpose(d_z, d_info, d_pose_i, d_pose_j, n_factors, d_poses, n_poses, d_residuals, d_jac_i, d_jac_j,
                              d_parts, d_flags, static_cast<hipStream_t>(stream));
}

int nhip_resid_relpose_normal_eq_dev(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                                     int32_t n_factors, const nhip_loss_spec_t *loss, const double *d_poses, int32_t n_poses,
                                     double *d_out, double *d_weights, int32_t *d_flags, void *stream) {
  // (the spec, the sizes and the pointers are an argument error with or without a device)
  const nhip_loss_spec_t none = {NHIP_LOSS_NONE, 0, 1.0};
  if (!loss) loss = &none;
  int rc = loss_spec_check(loss, "resid_relpose_normal_eq_dev");
  if (rc) return rc;
  if ((rc = relpose_args_check(d_z, d_info, d_pose_i, d_pose_j, n_factors, d_poses, n_poses, d_out, "resid_relpose_normal_eq_dev")))
    return rc;
  if ((rc = require_device())) return rc;
  return launch_resid_relpose_normal_eq(d_z, d_info, d_pose_i, d_pose_j, n_factors, loss->kind, loss->scale, d_poses, n_poses,
                                        d_out, d_weights, d_flags, static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------- HITL point selection
// the accepted ranges of include/nautilus_hip.h
static int hitl_spec_check(const nhip_hitl_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(std::isfinite(s->line_width) && s->line_width >= 0, "%s: line_width must be finite and >= 0", who);
  NHIP_REQUIRE(s->point_threshold >= 1, "%s: point_threshold %d below 1", who, s->point_threshold);
  return NHIP_OK;
}

int nhip_hitl_spec_default(nhip_hitl_spec_t *out) {
  NHIP_REQUIRE(out, "hitl_spec_default: null pointer");
  memset(out, 0, sizeof(*out));
  out->line_width = 0.05;     // hitl_line_width, default_config.lua:88
  out->point_threshold = 10;  // hitl_pose_point_threshold, default_config.lua:91
  return NHIP_OK;
}

int nhip_hitl_select_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const float *d_pose_f32,
                         const nhip_hitl_spec_t *spec, uint8_t *d_class, int32_t *d_counts, int32_t *d_scan_block,
                         int32_t *d_scan_offset, int32_t *d_totals, void *stream) {
  int rc = hitl_spec_check(spec, "hitl_select_dev");  // (a bad spec or size is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0, "hitl_select_dev: n_scans < 0");
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_totals && (n_scans == 0 || (d_xy && d_offsets && d_pose_f32 && d_class && d_counts && d_scan_block && d_scan_offset)),
               "hitl_select_dev: null pointer");
  NHIP_REQUIRE(aligned(d_pose_f32, 16), "hitl_select_dev: d_pose_f32 must be 16-byte aligned");
  return launch_hitl_select(d_xy, d_offsets, n_scans, d_pose_f32, *spec, d_class, d_counts, d_scan_block, d_scan_offset, d_totals,
                            static_cast<hipStream_t>(stream));
}

int nhip_hitl_pack_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_class,
                       const int32_t *d_counts, const int32_t *d_scan_block, const int32_t *d_scan_offset,
                       const int32_t *d_totals, int32_t n_blocks, int32_t n_points, float *d_points,
                       int32_t *d_block_offsets, int32_t *d_block_pose, void *stream) {
  NHIP_REQUIRE(n_scans >= 0 && n_blocks >= 0 && n_points >= 0, "hitl_pack_dev: negative size");
  NHIP_REQUIRE(n_blocks <= n_scans, "hitl_pack_dev: %d blocks of %d scans", n_blocks, n_scans);
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_totals && d_block_offsets && (n_scans == 0 || (d_xy && d_offsets && d_class && d_counts && d_scan_block && d_scan_offset)) &&
                   (n_blocks == 0 || d_block_pose) && (n_points == 0 || d_points),
               "hitl_pack_dev: null pointer");
  return launch_hitl_pack(d_xy, d_offsets, n_scans, d_class, d_counts, d_scan_block, d_scan_offset, d_totals, n_blocks, n_points, d_points,
                          d_block_offsets, d_block_pose, static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------- loop-closure gates
int nhip_lc_scatter_scores_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, double *d_scores,
                               void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0 && (n_scans == 0 || (d_xy && d_offsets && d_scores)), "lc_scatter_scores_dev: bad arguments");
  return launch_lc_scatter_scores(d_xy, d_offsets, n_scans, d_scores, static_cast<hipStream_t>(stream));
}

int nhip_lc_pair_gate_dev(const double *d_poses, int32_t n_poses, const int32_t *d_candidates, int32_t n_candidates,
                          double max_range, int32_t min_separation, uint8_t *d_flags, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n_candidates >= 0 && n_poses >= 0 && (n_candidates == 0 || (d_poses && d_candidates && d_flags)),
               "lc_pair_gate_dev: bad arguments");
  return launch_lc_pair_gate(d_poses, n_poses, d_candidates, n_candidates, max_range, min_separation, d_flags,
                             static_cast<hipStream_t>(stream));
}

int nhip_round_norm_dev(const float *d_dx, const float *d_dy, int64_t n, int32_t root_only, float *d_out, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n >= 0 && (n == 0 || (d_dx && d_out && (root_only || d_dy))), "round_norm_dev: bad arguments");
  return launch_round_norm(d_dx, d_dy, n, root_only, d_out, static_cast<hipStream_t>(stream));
}

int nhip_lc_chi_square_gate_dev(const double *d_poses, int32_t n_poses, const int32_t *d_pair_src, const int32_t *d_pair_tgt,
                                const float *d_cov, int32_t n_pairs, double max_score, double *d_scores,
                                uint8_t *d_flags, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n_pairs >= 0 && n_poses >= 0 && (n_pairs == 0 || (d_poses && d_pair_src && d_pair_tgt && d_cov && d_scores && d_flags)),
               "lc_chi_square_gate_dev: bad arguments");
  NHIP_REQUIRE(aligned(d_cov, 16), "lc_chi_square_gate_dev: d_cov must be 16-byte aligned");
  return launch_lc_chi_square(d_poses, n_poses, d_pair_src, d_pair_tgt, d_cov, n_pairs, max_score, d_scores, d_flags,
                              static_cast<hipStream_t>(stream));
}

int nhip_lc_chi_square_gate(const double *poses, int32_t n_poses, const int32_t *pair_src, const int32_t *pair_tgt,
                            const float *cov, int32_t n, double max_score, double *scores, uint8_t *flags) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n >= 0 && n_poses >= 0 && (n == 0 || (poses && pair_src && pair_tgt && cov && scores && flags)),
               "lc_chi_square_gate: bad arguments");
  for (int32_t i = 0; i < n; i++)
    NHIP_REQUIRE(pair_src[i] >= 0 && pair_src[i] < n_poses && pair_tgt[i] >= 0 && pair_tgt[i] < n_poses,
                 "lc_chi_square_gate: pair %d (%d, %d) out of range", i, pair_src[i], pair_tgt[i]);
  if (n == 0) return NHIP_OK;
  const size_t N = (size_t)n;
  Staged st;
  const double *dp = st.in(poses, 3 * (size_t)n_poses);
  const int32_t *ds = st.in(pair_src, N), *dt = st.in(pair_tgt, N);
  const float *dc = st.in(cov, 4 * N);
  double *dsc = st.out<double>(N);
  uint8_t *df = st.out<uint8_t>(N);
  if (st.ok()) st.launched(launch_lc_chi_square(dp, n_poses, ds, dt, dc, n, max_score, dsc, df, nullptr));
  st.fetch(scores, dsc, N);
  st.fetch(flags, df, N);
  return st.finish();
}

int nhip_lc_scatter_scores(const nhip_scans_t *scans, double *scores) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(scans && (scores || scans->n_scans == 0), "lc_scatter_scores: bad arguments");
  if (scans->n_scans == 0) return NHIP_OK;
  Staged st;
  double *d = st.out<double>((size_t)scans->n_scans);
  if (st.ok())
    st.launched(launch_lc_scatter_scores(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), scans->n_scans, d, nullptr));
  st.fetch(scores, d, (size_t)scans->n_scans);
  return st.finish();
}

int nhip_lc_pair_gate(const double *poses, int32_t n_poses, const int32_t *candidates, int32_t n, double max_range,
                      int32_t min_separation, uint8_t *flags) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n >= 0 && n_poses >= 0 && (n == 0 || (poses && candidates && flags)), "lc_pair_gate: bad arguments");
  for (int32_t i = 0; i < n; i++)
    NHIP_REQUIRE(candidates[i] >= 0 && candidates[i] < n_poses, "lc_pair_gate: candidate %d out of range", candidates[i]);
  if (n == 0) return NHIP_OK;
  Staged st;
  const double *dp = st.in(poses, 3 * (size_t)n_poses);
  const int32_t *dc = st.in(candidates, (size_t)n);
  uint8_t *df = st.out<uint8_t>((size_t)n * n);
  if (st.ok()) st.launched(launch_lc_pair_gate(dp, n_poses, dc, n, max_range, min_separation, df, nullptr));
  st.fetch(flags, df, (size_t)n * n);
  return st.finish();
}

// ---------------------------------------------------------------- residual batches and the host-buffer residual forms
int nhip_resid_batch_create(int kind, const float *corr, const int32_t *block_offsets,
                            const int32_t *block_src, const int32_t *block_tgt, int32_t n_blocks,
                            int32_t n_poses, nhip_resid_batch_t **out) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(kind == NHIP_LIDAR_NORMAL || kind == NHIP_LIDAR_POINT, "resid_batch_create: bad kind %d", kind);
  NHIP_REQUIRE(block_offsets && block_src && block_tgt && out && n_blocks >= 0 && n_poses >= 0,
               "resid_batch_create: bad arguments");
  NHIP_REQUIRE(block_offsets[0] == 0, "resid_batch_create: block_offsets[0] must be 0");
  for (int32_t b = 0; b < n_blocks; b++) {
    // slam_residuals.h:109 CHECK_GT(source_points.size(), 0)
    NHIP_REQUIRE(block_offsets[b + 1] > block_offsets[b], "resid_batch_create: block %d is empty", b);
    NHIP_REQUIRE(block_src[b] >= 0 && block_src[b] < n_poses && block_tgt[b] >= 0 && block_tgt[b] < n_poses,
                 "resid_batch_create: block %d pose index out of range", b);
  }
  const int64_t n_corr = block_offsets[n_blocks];
  NHIP_REQUIRE(n_corr == 0 || corr, "resid_batch_create: null corr");
  std::vector<int32_t> cb((size_t)n_corr);
  for (int32_t b = 0; b < n_blocks; b++)
    for (int32_t i = block_offsets[b]; i < block_offsets[b + 1]; i++) cb[i] = b;
  nhip_resid_batch *B = new nhip_resid_batch();
  B->kind = kind;
  B->n_blocks = n_blocks;
  B->n_poses = n_poses;
  B->n_corr = n_corr;
  B->h_offsets.assign(block_offsets, block_offsets + n_blocks + 1);
  if ((rc = B->jtt.alloc(sizeof(double) * 2 * (size_t)n_corr)) || (rc = B->one_poses.alloc(sizeof(double) * 6)) ||
      (rc = B->one_consts.alloc(sizeof(double) * 8)) || (rc = B->one_idx.alloc(sizeof(int32_t) * 2))) {
    delete B;
    return rc;
  }
  {
    const int32_t idx[2] = {0, 1};
    hipError_t e0 = hipMemcpy(B->one_idx.p, idx, sizeof(idx), hipMemcpyHostToDevice);
    if (e0 != hipSuccess) {
      delete B;
      return hip_fail(e0, "resid_batch_create memcpy", __FILE__, __LINE__);
    }
  }
  if ((rc = B->corr.alloc(sizeof(float) * 8 * (size_t)n_corr)) || (rc = B->corr_block.alloc(sizeof(int32_t) * (size_t)n_corr)) ||
      (rc = B->block_src.alloc(sizeof(int32_t) * (size_t)n_blocks)) || (rc = B->block_tgt.alloc(sizeof(int32_t) * (size_t)n_blocks)) ||
      (rc = B->consts.alloc(sizeof(double) * 8 * (size_t)n_blocks)) || (rc = B->poses.alloc(sizeof(double) * 3 * (size_t)n_poses)) ||
      (rc = B->res.alloc(sizeof(double) * 2 * (size_t)n_corr)) || (rc = B->jsrc.alloc(sizeof(double) * 6 * (size_t)n_corr)) ||
      (rc = B->jtgt.alloc(sizeof(double) * 6 * (size_t)n_corr))) {
    delete B;
    return rc;
  }
  hipError_t e = hipSuccess;
  if (n_corr) {
    e = hipMemcpy(B->corr.p, corr, sizeof(float) * 8 * (size_t)n_corr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(B->corr_block.p, cb.data(), sizeof(int32_t) * (size_t)n_corr, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && n_blocks) {
    e = hipMemcpy(B->block_src.p, block_src, sizeof(int32_t) * (size_t)n_blocks, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(B->block_tgt.p, block_tgt, sizeof(int32_t) * (size_t)n_blocks, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    delete B;
    return hip_fail(e, "resid_batch_create memcpy", __FILE__, __LINE__);
  }
  *out = B;
  return NHIP_OK;
}

// the whole batch at `poses`, on the null stream: the pose upload and the launch the three evaluations share.  jsrc, jtgt,
// jtt, q: which of the outputs beside the residuals the kernel writes (jtt and q into B->jtt, one of them at a time)
static int batch_launch(nhip_resid_batch_t *B, const double *poses, bool jsrc, bool jtgt, bool jtt, bool q) {
  NHIP_TRY_HIP(hipMemcpy(B->poses.p, poses, sizeof(double) * 3 * (size_t)B->n_poses, hipMemcpyHostToDevice));
  return launch_resid_lidar(B->kind, B->corr.as<const float>(), B->corr_block.as<const int32_t>(), B->n_corr,
                            B->block_src.as<const int32_t>(), B->block_tgt.as<const int32_t>(), B->n_blocks, B->poses.as<const double>(),
                            B->n_poses, B->consts.as<double>(), B->res.as<double>(), jsrc ? B->jsrc.as<double>() : nullptr,
                            jtgt ? B->jtgt.as<double>() : nullptr, nullptr, jtt ? B->jtt.as<double>() : nullptr, 0,
                            q ? B->jtt.as<double>() : nullptr);
}

int nhip_resid_batch_eval(nhip_resid_batch_t *B, const double *poses, double *residuals,
                          double *jac_src, double *jac_tgt) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(B && poses && residuals, "resid_batch_eval: bad arguments");
  if (B->n_corr == 0) return NHIP_OK;
  if ((rc = batch_launch(B, poses, jac_src != nullptr, jac_tgt != nullptr, false, false))) return rc;
  NHIP_TRY_HIP(hipMemcpy(residuals, B->res.p, sizeof(double) * 2 * (size_t)B->n_corr, hipMemcpyDeviceToHost));
  if (jac_src) NHIP_TRY_HIP(hipMemcpy(jac_src, B->jsrc.p, sizeof(double) * 6 * (size_t)B->n_corr, hipMemcpyDeviceToHost));
  if (jac_tgt) NHIP_TRY_HIP(hipMemcpy(jac_tgt, B->jtgt.p, sizeof(double) * 6 * (size_t)B->n_corr, hipMemcpyDeviceToHost));
  return NHIP_OK;
}

int nhip_resid_batch_eval_compact(nhip_resid_batch_t *B, const double *poses, double *residuals, double *jac_src,
                                  double *jac_tgt_theta) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(B && poses && residuals && jac_src && jac_tgt_theta, "resid_batch_eval_compact: bad arguments");
  if (B->n_corr == 0) return NHIP_OK;
  if ((rc = batch_launch(B, poses, true, false, true, false))) return rc;
  // three copies on the stream the kernel ran on; into pinned memory (nhip_host_alloc) they run at the PCIe rate
  NHIP_TRY_HIP(hipMemcpyAsync(residuals, B->res.p, sizeof(double) * 2 * (size_t)B->n_corr, hipMemcpyDeviceToHost, nullptr));
  NHIP_TRY_HIP(hipMemcpyAsync(jac_src, B->jsrc.p, sizeof(double) * 6 * (size_t)B->n_corr, hipMemcpyDeviceToHost, nullptr));
  NHIP_TRY_HIP(hipMemcpyAsync(jac_tgt_theta, B->jtt.p, sizeof(double) * 2 * (size_t)B->n_corr, hipMemcpyDeviceToHost, nullptr));
  NHIP_TRY_HIP(hipStreamSynchronize(nullptr));
  return NHIP_OK;
}

int nhip_resid_batch_eval_q(nhip_resid_batch_t *B, const double *poses, double *residuals, double *q, double *block_consts) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(B && poses && residuals && q && block_consts, "resid_batch_eval_q: bad arguments");
  if (B->n_corr == 0) return NHIP_OK;
  // (residual-only instantiation + one more 16-byte store per correspondence; q goes where the compact form keeps J_tgt's
  //  theta column: the two forms of one batch are not in flight together -- the handle's calls synchronise)
  if ((rc = batch_launch(B, poses, false, false, false, true))) return rc;
  NHIP_TRY_HIP(hipMemcpyAsync(residuals, B->res.p, sizeof(double) * 2 * (size_t)B->n_corr, hipMemcpyDeviceToHost, nullptr));
  NHIP_TRY_HIP(hipMemcpyAsync(q, B->jtt.p, sizeof(double) * 2 * (size_t)B->n_corr, hipMemcpyDeviceToHost, nullptr));
  NHIP_TRY_HIP(hipMemcpyAsync(block_consts, B->consts.p, sizeof(double) * 8 * (size_t)B->n_blocks, hipMemcpyDeviceToHost, nullptr));
  NHIP_TRY_HIP(hipStreamSynchronize(nullptr));
  return NHIP_OK;
}

int nhip_resid_jacobians_from_q(int kind, const float *corr, const double *q, const double *block_consts, int64_t n,
                                double *jac_src, double *jac_tgt) {
  NHIP_REQUIRE(kind == NHIP_LIDAR_NORMAL || kind == NHIP_LIDAR_POINT, "resid_jacobians_from_q: bad kind %d", kind);
  NHIP_REQUIRE(n >= 0 && (n == 0 || (corr && q && block_consts)), "resid_jacobians_from_q: bad arguments");
  // the closed forms of resid_lidar_kernel (nhip_resid.hip); consts = {l00, l01, l10, l11, tx, ty, i00, i01}.  u = L p_s is
  // formed as the kernel forms it, from the source point the caller holds: q - t would leave it with the rounding of q, which
  // beside a point near its scanner's origin is hundreds of ulps of u
  const double l00 = block_consts[0], l01 = block_consts[1], l10 = block_consts[2], l11 = block_consts[3];
  const double i00 = block_consts[6], i01 = block_consts[7], i10 = -i01, i11 = i00;
  for (int64_t i = 0; i < n; i++) {
    const double px = corr[8 * i], py = corr[8 * i + 1];
    const double qx = q[2 * i], qy = q[2 * i + 1], ux = l00 * px + l01 * py, uy = l10 * px + l11 * py;
    double js[6], jt[6];
    if (kind == NHIP_LIDAR_NORMAL) {
      const double nsx = corr[8 * i + 4], nsy = corr[8 * i + 5], ntx = corr[8 * i + 6], nty = corr[8 * i + 7];
      js[0] = ntx * i00 + nty * i10;
      js[1] = ntx * i01 + nty * i11;
      js[2] = ntx * (-uy) + nty * ux;
      js[3] = -(nsx * i00 + nsy * i10);
      js[4] = -(nsx * i01 + nsy * i11);
      js[5] = -(nsx * (-uy) + nsy * ux);
      jt[0] = -js[0];
      jt[1] = -js[1];
      jt[2] = ntx * qy - nty * qx;
      jt[3] = -js[3];
      jt[4] = -js[4];
      jt[5] = -(nsx * qy - nsy * qx);
    } else {
      js[0] = -i00; js[1] = -i01; js[2] = uy;
      js[3] = -i10; js[4] = -i11; js[5] = -ux;
      jt[0] = i00;  jt[1] = i01;  jt[2] = -qy;
      jt[3] = i10;  jt[4] = i11;  jt[5] = qx;
    }
    if (jac_src) memcpy(jac_src + 6 * i, js, sizeof(js));
    if (jac_tgt) memcpy(jac_tgt + 6 * i, jt, sizeof(jt));
  }
  return NHIP_OK;
}

int nhip_resid_batch_eval_block(nhip_resid_batch_t *B, int32_t block, const double *source_pose,
                                const double *target_pose, double *residuals, double *jac_src, double *jac_tgt) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(B && source_pose && target_pose && residuals, "resid_batch_eval_block: bad arguments");
  NHIP_REQUIRE(block >= 0 && block < B->n_blocks, "resid_batch_eval_block: block %d out of range", block);
  const int64_t o = B->h_offsets[block], n = B->h_offsets[block + 1] - o;
  double two[6];
  memcpy(two, source_pose, 3 * sizeof(double));
  memcpy(two + 3, target_pose, 3 * sizeof(double));
  std::lock_guard<std::mutex> lk(B->one_mu);  // one scratch set per batch: callers on several threads take turns
  NHIP_TRY_HIP(hipMemcpy(B->one_poses.p, two, sizeof(two), hipMemcpyHostToDevice));
  // the block's slice of the batch; its rows carry block id `block`, the one set of constants sits at index 0
  rc = launch_resid_lidar(B->kind, B->corr.as<const float>() + 8 * o, B->corr_block.as<const int32_t>() + o, n,
                          B->one_idx.as<const int32_t>(), B->one_idx.as<const int32_t>() + 1, 1, B->one_poses.as<const double>(), 2,
                          B->one_consts.as<double>(), B->res.as<double>() + 2 * o, jac_src ? B->jsrc.as<double>() + 6 * o : nullptr,
                          jac_tgt ? B->jtgt.as<double>() + 6 * o : nullptr, nullptr, nullptr, block);
  if (rc) return rc;
  NHIP_TRY_HIP(hipMemcpy(residuals, B->res.as<double>() + 2 * o, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost));
  if (jac_src) NHIP_TRY_HIP(hipMemcpy(jac_src, B->jsrc.as<double>() + 6 * o, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost));
  if (jac_tgt) NHIP_TRY_HIP(hipMemcpy(jac_tgt, B->jtgt.as<double>() + 6 * o, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost));
  return NHIP_OK;
}

int nhip_resid_batch_free(nhip_resid_batch_t *batch) {
  delete batch;
  return NHIP_OK;
}

int nhip_resid_odometry(const float *t_odom, const float *r_odom, const int32_t *pose_i,
                        const int32_t *pose_j, int32_t n, double tw, double rw, const double *poses,
                        int32_t n_poses, double *residuals, double *jac_i, double *jac_j) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n >= 0 && n_poses >= 0, "resid_odometry: negative size");
  if (n == 0) return NHIP_OK;
  NHIP_REQUIRE(t_odom && r_odom && pose_i && pose_j && poses && residuals, "resid_odometry: null pointer");
  for (int32_t f = 0; f < n; f++)
    NHIP_REQUIRE(pose_i[f] >= 0 && pose_i[f] < n_poses && pose_j[f] >= 0 && pose_j[f] < n_poses,
                 "resid_odometry: factor %d pose index out of range", f);
  const size_t N = (size_t)n;
  Staged st;
  const float *dt = st.in(t_odom, 2 * N), *dr = st.in(r_odom, N);
  const int32_t *di = st.in(pose_i, N), *dj = st.in(pose_j, N);
  const double *dp = st.in(poses, 3 * (size_t)n_poses);
  double *res = st.out<double>(3 * N), *ji = st.out<double>(9 * N), *jj = st.out<double>(9 * N);
  if (st.ok())
    st.launched(launch_resid_odometry(dt, dr, di, dj, n, tw, rw, dp, n_poses, res, jac_i ? ji : nullptr, jac_j ? jj : nullptr, nullptr));
  st.fetch(residuals, res, 3 * N);
  st.fetch(jac_i, ji, 9 * N);
  st.fetch(jac_j, jj, 9 * N);
  return st.finish();
}

int nhip_resid_relpose(const double *z, const double *info, const int32_t *pose_i, const int32_t *pose_j, int32_t n,
                       const double *poses, int32_t n_poses, double *residuals, double *jac_i, double *jac_j, double *parts,
                       int32_t *flags) {
  int rc = relpose_args_check(z, info, pose_i, pose_j, n, poses, n_poses, residuals, "resid_relpose");
  if (rc) return rc;
  for (int32_t f = 0; f < n; f++)
    NHIP_REQUIRE(pose_i[f] >= 0 && pose_i[f] < n_poses && pose_j[f] >= 0 && pose_j[f] < n_poses,
                 "resid_relpose: factor %d pose index out of range", f);
  if ((rc = require_device())) return rc;
  if (n == 0) return NHIP_OK;
  const size_t N = (size_t)n;
  Staged st;
  const double *dz = st.in(z, 4 * N), *dl = st.in(info, 6 * N);
  const int32_t *di = st.in(pose_i, N), *dj = st.in(pose_j, N);
  const double *dp = st.in(poses, 3 * (size_t)n_poses);
  double *res = st.out<double>(3 * N), *ji = st.out<double>(9 * N), *jj = st.out<double>(9 * N), *pt = st.out<double>(8 * N);
  int32_t *fl = st.out<int32_t>(N);
  if (st.ok())
    st.launched(launch_resid_relpose(dz, dl, di, dj, n, dp, n_poses, res, jac_i ? ji : nullptr, jac_j ? jj : nullptr,
                                     parts ? pt : nullptr, flags ? fl : nullptr, nullptr));
  st.fetch(residuals, res, 3 * N);
  st.fetch(jac_i, ji, 9 * N);
  st.fetch(jac_j, jj, 9 * N);
  st.fetch(parts, pt, 8 * N);
  st.fetch(flags, fl, N);
  return st.finish();
}

int nhip_resid_point_to_line(const float *segments, const float *points, const int32_t *point_block,
                             int64_t n_points, const int32_t *block_pose, const int32_t *block_line,
                             int32_t n_blocks, const double *poses, int32_t n_poses,
                             const double *line_poses, int32_t n_line_poses, double *residuals,
                             double *jac_pose, double *jac_line) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n_points >= 0 && n_blocks >= 0 && n_poses >= 0 && n_line_poses >= 0, "resid_point_to_line: negative size");
  if (n_points == 0) return NHIP_OK;
  NHIP_REQUIRE(segments && points && point_block && block_pose && block_line && poses && line_poses && residuals,
               "resid_point_to_line: null pointer");
  for (int32_t b = 0; b < n_blocks; b++)
    NHIP_REQUIRE(block_pose[b] >= 0 && block_pose[b] < n_poses && block_line[b] >= 0 && block_line[b] < n_line_poses,
                 "resid_point_to_line: block %d parameter index out of range", b);
  for (int64_t i = 0; i < n_points; i++)
    NHIP_REQUIRE(point_block[i] >= 0 && point_block[i] < n_blocks, "resid_point_to_line: point %lld block out of range",
                 (long long)i);
  const size_t NP = (size_t)n_points, NB = (size_t)n_blocks;
  Staged st;
  const float *ds = st.in(segments, 4 * NB), *dpt = st.in(points, 2 * NP);
  const int32_t *dpb = st.in(point_block, NP), *dbp = st.in(block_pose, NB), *dbl = st.in(block_line, NB);
  const double *dp = st.in(poses, 3 * (size_t)n_poses), *dl = st.in(line_poses, 3 * (size_t)n_line_poses);
  double *res = st.out<double>(NP), *j0 = st.out<double>(3 * NP), *j1 = st.out<double>(3 * NP);
  if (st.ok())
    st.launched(launch_resid_point_to_line(ds, dpt, dpb, n_points, dbp, dbl, n_blocks, dp, n_poses, dl, n_line_poses, res,
                                           jac_pose ? j0 : nullptr, jac_line ? j1 : nullptr, nullptr));
  st.fetch(residuals, res, NP);
  st.fetch(jac_pose, j0, 3 * NP);
  st.fetch(jac_line, j1, 3 * NP);
  return st.finish();
}

// ---------------------------------------------------------------- multi-GPU all-gather
namespace {
// ncclAllGather(sendbuff, recvbuff, sendcount, datatype, comm, stream); ncclInt8 = 0 (rccl.h)
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
typedef const char *(*nccl_errstr_fn)(int);
nccl_allgather_fn g_allgather = nullptr;
nccl_errstr_fn g_errstr = nullptr;
std::once_flag g_rccl_once;

void bind_rccl() {
  // RTLD_NOLOAD first: a process that already holds an RCCL (PyTorch ships its own copy) must
  // keep using that one, since the communicator came from it
  void *h = nullptr;
  for (const char *name : {"librccl.so.1", "librccl.so"}) {
    h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
    if (h) break;
  }
  for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    if (h) break;
    h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
  }
  if (!h) return;
  g_allgather = reinterpret_cast<nccl_allgather_fn>(dlsym(h, "ncclAllGather"));
  g_errstr = reinterpret_cast<nccl_errstr_fn>(dlsym(h, "ncclGetErrorString"));
}
}  // namespace

int nhip_allgather_matches(void *comm, const nhip_match_t *d_local, int32_t n_local, nhip_match_t *d_all,
                           void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(n_local >= 0, "allgather_matches: negative count");
  if (n_local == 0) return NHIP_OK;
  NHIP_REQUIRE(comm && d_local && d_all, "allgather_matches: null pointer");
  std::call_once(g_rccl_once, bind_rccl);
  if (!g_allgather) {
    const char *why = dlerror();
    set_error("allgather_matches: librccl.so could not be loaded (%s)", why ? why : "no ncclAllGather symbol");
    return NHIP_ERR_STATE;
  }
  const int st = g_allgather(d_local, d_all, sizeof(nhip_match_t) * (size_t)n_local, /*ncclInt8=*/0, comm,
                             static_cast<hipStream_t>(stream));
  if (st != 0) {
    set_error("allgather_matches: ncclAllGather failed: %s", g_errstr ? g_errstr(st) : "unknown");
    return NHIP_ERR_HIP;
  }
  return NHIP_OK;
}


}  // extern "C"
