// nhip_host_csm.hip -- the grid and matcher entry points of the C ABI: the `_dev` forms on the caller's buffers and
// stream, and the scan / grid handles with the searches that run on them.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

// digest of what a table buffer's layout and build depend on: the spec as handed in, the number of targets
static uint64_t grids_shape(const nhip_grid_spec_t *spec, int32_t n_targets) {
  uint64_t h = 0xcbf29ce484222325ull;
  const unsigned char *b = reinterpret_cast<const unsigned char *>(spec);
  for (size_t i = 0; i < sizeof(*spec); i++) h = (h ^ b[i]) * 0x100000001b3ull;
  for (int i = 0; i < 4; i++) h = (h ^ (uint64_t)((uint32_t)n_targets >> (8 * i) & 0xffu)) * 0x100000001b3ull;
  return h >> 1;  // (the low bit is the pool's: which buffer of the pair)
}

int nhip::ensure_skip_maps(const nhip_grids_t *grids, const MatchPlan &plan) {
  // (writes to the handle -- the maps, then the flag -- under the handle's mutex, which is taken before the flag is looked
  //  at: concurrent nhip_csm_match calls on one handle are ordered, the loser finds the maps built.  L and n never change.)
  nhip_grids *g = const_cast<nhip_grids *>(grids);
  if (plan.form != MATCH_STRIPS16 || g->n == 0 || !g->L.has_image) return NHIP_OK;
  std::lock_guard<std::mutex> lock(g->mu);
  if (g->spec.flags & NHIP_GRID_SKIP_MAP) return NHIP_OK;
  g->dirty = true;  // (maps the build's tile list does not know of)
  int rc = launch_skipmap_build(g->grids.as<uint8_t>(), g->n, g->L, nullptr);
  if (rc) return rc;
  NHIP_TRY_HIP(hipStreamSynchronize(nullptr));
  g->spec.flags |= NHIP_GRID_SKIP_MAP;
  return NHIP_OK;
}

int nhip::spec_under_lock(nhip_grids_t *g, nhip_grid_spec_t *out) {
  std::lock_guard<std::mutex> lock(g->mu);
  *out = g->spec;
  return NHIP_OK;
}

// ---------------------------------------------------------------- device-pointer API
// nhip_grid_build_dev / nhip_grid_rebuild_dev (`name`, for the messages): the build, from zeroed slots or incrementally
static int grid_build_dev(const char *name, bool incremental, const float *d_xy, const int32_t *d_offsets, int32_t n_scans,
                          const int32_t *d_target_ids, int32_t n_targets, const nhip_grid_spec_t *spec, uint8_t *d_grids,
                          void *d_workspace, int64_t workspace_bytes, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_xy && d_offsets && d_target_ids && d_grids && d_workspace, "%s: null pointer", name);
  NHIP_REQUIRE(n_targets >= 0 && n_scans >= 0, "%s: n_targets %d / n_scans %d < 0", name, n_targets, n_scans);
  GridLayout L;
  rc = make_layout(spec, &L);
  if (rc) return rc;
  if (n_targets == 0) return NHIP_OK;
  return launch_grid_build(d_xy, d_offsets, n_scans, d_target_ids, n_targets, spec, L, d_grids, d_workspace,
                           workspace_bytes, static_cast<hipStream_t>(stream), incremental);
}

extern "C" {

int nhip_grid_build_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids,
                        int32_t n_targets, const nhip_grid_spec_t *spec, uint8_t *d_grids,
                        void *d_workspace, int64_t workspace_bytes, void *stream) {
  return grid_build_dev("grid_build_dev", false, d_xy, d_offsets, n_scans, d_target_ids, n_targets, spec, d_grids, d_workspace, workspace_bytes, stream);
}

int nhip_grid_rebuild_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids,
                          int32_t n_targets, const nhip_grid_spec_t *spec, uint8_t *d_grids,
                          void *d_workspace, int64_t workspace_bytes, void *stream) {
  return grid_build_dev("grid_rebuild_dev", true, d_xy, d_offsets, n_scans, d_target_ids, n_targets, spec, d_grids, d_workspace, workspace_bytes, stream);
}

int nhip_submap_member_affines(const double *poses, int32_t n_poses, const int32_t *anchor_of_member, const int32_t *member_scan,
                               int32_t n_members, float *out) {
  NHIP_REQUIRE(n_poses >= 0 && n_members >= 0, "submap_member_affines: negative count");
  NHIP_REQUIRE(n_members == 0 || (poses && anchor_of_member && member_scan && out), "submap_member_affines: null pointer");
  for (int32_t m = 0; m < n_members; m++)
    NHIP_REQUIRE(anchor_of_member[m] >= 0 && anchor_of_member[m] < n_poses && member_scan[m] >= 0 && member_scan[m] < n_poses,
                 "submap_member_affines: member %d: anchor %d / scan %d outside the %d poses", m, anchor_of_member[m],
                 member_scan[m], n_poses);
  for (int32_t m = 0; m < n_members; m++) {
    // entries of inverse(A(anchor)) * A(member) in double (A: PoseArrayToAffine, slam_util.h:20-28; the rigid inverse), then
    // the cast of TransformPointcloud (slam_util.h:55-63).  Compiled without contraction: products and sums round singly.
    const double *a = poses + 3 * (size_t)anchor_of_member[m], *b = poses + 3 * (size_t)member_scan[m];
    const double ca = cos(a[2]), sa = sin(a[2]), cm = cos(b[2]), sm = sin(b[2]);
    const double dx = b[0] - a[0], dy = b[1] - a[1];
    out[4 * (size_t)m + 0] = (float)(ca * cm + sa * sm);
    out[4 * (size_t)m + 1] = (float)(ca * sm - sa * cm);
    out[4 * (size_t)m + 2] = (float)(ca * dx + sa * dy);
    out[4 * (size_t)m + 3] = (float)(ca * dy - sa * dx);
  }
  return NHIP_OK;
}

int nhip_submaps_gather_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_member_scan,
                            const float *d_member_affine, const int32_t *d_member_offsets, int32_t n_targets, float *d_out_xy,
                            int64_t out_capacity, int32_t *d_out_offsets, void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_offsets && d_member_offsets && d_out_offsets && (d_member_scan || n_targets == 0), "submaps_gather_dev: null pointer");
  NHIP_REQUIRE(n_targets >= 0 && n_scans >= 0 && out_capacity >= 0, "submaps_gather_dev: n_targets %d / n_scans %d / out_capacity %lld < 0",
               n_targets, n_scans, (long long)out_capacity);
  // (without room nothing reads the points or the affines: a caller that only wants the error may pass null for them)
  NHIP_REQUIRE(out_capacity == 0 || (d_xy && d_member_affine && d_out_xy), "submaps_gather_dev: null pointer");
  return launch_submap_gather(d_xy, d_offsets, n_scans, d_member_scan, d_member_affine, d_member_offsets, n_targets, d_out_xy,
                              out_capacity, d_out_offsets, static_cast<hipStream_t>(stream));
}

int nhip_csm_match_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                       int32_t n_grids, const nhip_grid_spec_t *spec, const int32_t *d_pair_src,
                       const int32_t *d_pair_slot, const double *d_rot0_cs,
                       const double *d_delta_cs, const int32_t *d_pair_origin, int32_t n_pairs,
                       const nhip_search_t *search, uint64_t *d_keys, nhip_match_t *d_out,
                       int32_t *d_sums, void *d_workspace, int64_t workspace_bytes, void *stream) {
  return nhip_csm_match_gated_dev(d_xy, d_offsets, n_scans, d_grids, n_grids, spec, d_pair_src, d_pair_slot, d_rot0_cs, d_delta_cs,
                                  d_pair_origin, n_pairs, search, d_keys, d_out, d_sums, d_workspace, workspace_bytes, stream,
                                  -INFINITY);
}

int nhip_csm_match_gated_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                             int32_t n_grids, const nhip_grid_spec_t *spec, const int32_t *d_pair_src,
                             const int32_t *d_pair_slot, const double *d_rot0_cs,
                             const double *d_delta_cs, const int32_t *d_pair_origin, int32_t n_pairs,
                             const nhip_search_t *search, uint64_t *d_keys, nhip_match_t *d_out,
                             int32_t *d_sums, void *d_workspace, int64_t workspace_bytes, void *stream, double min_score) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(!std::isnan(min_score), "csm_match_dev: min_score is NaN");
  NHIP_REQUIRE(d_xy && d_offsets && d_grids && d_pair_src && d_pair_slot && d_rot0_cs && d_delta_cs &&
                   d_keys && d_out && search,
               "csm_match_dev: null pointer");
  NHIP_REQUIRE(workspace_bytes >= 0 && (d_workspace || workspace_bytes == 0), "csm_match_dev: bad workspace");
  NHIP_REQUIRE(n_pairs >= 0 && n_scans >= 0 && n_grids >= 0, "csm_match_dev: negative count (n_pairs %d, n_scans %d, n_grids %d)",
               n_pairs, n_scans, n_grids);
  GridLayout L;
  rc = make_layout(spec, &L);
  if (rc) return rc;
  MatchJob job;
  job.xy = d_xy;
  job.offsets = d_offsets;
  job.ids = {n_scans, n_grids, dev_status()};
  job.grids = d_grids;
  job.spec = spec;
  job.L = &L;
  job.pair_src = d_pair_src;
  job.pair_slot = d_pair_slot;
  job.rot0_cs = d_rot0_cs;
  job.delta_cs = d_delta_cs;
  job.pair_origin = d_pair_origin;
  job.n_pairs = n_pairs;
  job.search = search;
  job.min_score = min_score;
  job.keys = d_keys;
  job.out = d_out;
  job.sums = d_sums;
  job.stream = static_cast<hipStream_t>(stream);
  job.workspace = d_workspace;
  job.workspace_bytes = workspace_bytes;
  return launch_csm_match(job, csm_plan(L, search, n_pairs));
}

int64_t nhip_csm_workspace_bytes(int32_t n_pairs) { return bnb_workspace_bytes(n_pairs); }

int nhip_csm_last_launch(int32_t out[8]) {
  NHIP_REQUIRE(out != nullptr, "csm_last_launch: null out");
  bnb_last_launch(out);
  return NHIP_OK;
}

int nhip_csm_scores_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                        int32_t n_grids, const nhip_grid_spec_t *spec, int32_t src, int32_t slot,
                        const double *d_rot0_cs, const double *d_delta_cs, int32_t origin_x,
                        int32_t origin_y, const nhip_search_t *search, int32_t *d_sums,
                        void *stream) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_xy && d_offsets && d_grids && d_rot0_cs && d_delta_cs && d_sums && search,
               "csm_scores_dev: null pointer");
  NHIP_REQUIRE(src >= 0 && src < n_scans && slot >= 0 && slot < n_grids, "csm_scores_dev: scan %d of %d / grid slot %d of %d out of range",
               src, n_scans, slot, n_grids);
  GridLayout L;
  rc = make_layout(spec, &L);
  if (rc) return rc;
  MatchJob job;  // (a score volume is of one pair, passed by value below: no pair arrays, ids, keys or records)
  job.xy = d_xy;
  job.offsets = d_offsets;
  job.grids = d_grids;
  job.spec = spec;
  job.L = &L;
  job.rot0_cs = d_rot0_cs;
  job.delta_cs = d_delta_cs;
  job.search = search;
  job.stream = static_cast<hipStream_t>(stream);
  return launch_csm_scores(job, src, slot, origin_x, origin_y, d_sums);
}

// ---------------------------------------------------------------- handle API
int nhip_scans_upload(const float *xy, const int32_t *offsets, int32_t n_scans, nhip_scans_t **out) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(offsets && out && n_scans >= 0, "scans_upload: bad arguments");
  phases_reset();
  NHIP_REQUIRE(offsets[0] == 0, "scans_upload: offsets[0] must be 0");
  for (int32_t i = 0; i < n_scans; i++)
    NHIP_REQUIRE(offsets[i + 1] >= offsets[i], "scans_upload: offsets not monotone at scan %d", i);
  const int64_t n_points = offsets[n_scans];
  NHIP_REQUIRE(n_points == 0 || xy, "scans_upload: null xy");
  nhip_scans *s = new nhip_scans();
  s->n_scans = n_scans;
  s->n_points = n_points;
  s->h_offsets.assign(offsets, offsets + n_scans + 1);
  if ((rc = s->xy.alloc(sizeof(float) * 2 * (size_t)n_points)) ||
      (rc = s->offsets.alloc(sizeof(int32_t) * (size_t)(n_scans + 1)))) {
    delete s;
    return rc;
  }
  hipError_t e = hipSuccess;
  {
    PhaseClock pc(PH_UPLOAD);
    if (n_points) e = hipMemcpy(s->xy.p, xy, sizeof(float) * 2 * (size_t)n_points, hipMemcpyHostToDevice);
    if (e == hipSuccess)
      e = hipMemcpy(s->offsets.p, offsets, sizeof(int32_t) * (size_t)(n_scans + 1), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    delete s;
    return hip_fail(e, "scans_upload memcpy", __FILE__, __LINE__);
  }
  *out = s;
  return NHIP_OK;
}

int nhip_scans_free(nhip_scans_t *scans) {
  phases_reset();
  delete scans;
  return NHIP_OK;
}

// the handle builds: the tables of scans `target_ids` (checked by the caller) of the device cloud (d_xy, d_offsets), after
// whatever the caller enqueued on the null stream; returns with the device idle
static int grids_build_on(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *target_ids,
                          int32_t n_targets, const nhip_grid_spec_t *spec, nhip_grids_t **out) {
  GridLayout L;
  int rc = make_layout(spec, &L);
  if (rc) return rc;
  nhip_grids *g = new nhip_grids();
  g->spec = *spec;
  g->L = L;
  g->n = n_targets;
  g->target_ids.assign(target_ids, target_ids + n_targets);
  g->shape = grids_shape(spec, n_targets);
  DevBuf ids;
  DevBuf &ws = g->ws;
  const int32_t chunk = n_targets > 0 ? n_targets : 1;  // workspace is ~25 bytes per 64x64 tile: all targets in one pass
  const int64_t ws_bytes = nhip_grid_workspace_bytes(spec, chunk);
  const size_t grid_bytes = (size_t)n_targets * L.slot_bytes + 256;
  // the buffers of the last build of this shape, if a handle released them and nobody has touched them since: the build
  // clears what that build wrote (its tile list and line masks are in the workspace, vouched for by a tag the clearing
  // kernel checks on the device) instead of zero-filling the slots -- 1.3 ms per 1000 targets at 1200 x 1200
  {
    void *pg = nullptr, *pw = nullptr;
    size_t bg = 0, bw = 0;
    if (n_targets > 0 && pool_take_pair(g->shape << 1, (g->shape << 1) | 1u, grid_bytes, (size_t)ws_bytes, &pg, &bg, &pw, &bw)) {
      g->grids.adopt(pg, bg);
      ws.adopt(pw, bw);
      g->rebuilt = true;
    }
  }
  if ((!g->rebuilt && ((rc = g->grids.alloc(grid_bytes)) || (rc = ws.alloc((size_t)ws_bytes)))) ||
      (rc = ids.alloc(sizeof(int32_t) * (size_t)(n_targets > 0 ? n_targets : 1)))) {
    delete g;
    return rc;
  }
  hipError_t e = hipSuccess;
  {
    PhaseClock pc(PH_UPLOAD);
    // (a fresh build zero-fills its n_targets slots itself, on its stream: launch_grid_build; what it does not reach is the
    //  256-byte tail past the last slot, which loads of the last slot's planes may run into)
    if (!g->rebuilt) e = hipMemset(g->grids.as<uint8_t>() + (size_t)n_targets * L.slot_bytes, 0, 256);
    if (e == hipSuccess && n_targets)
      e = hipMemcpy(ids.p, target_ids, sizeof(int32_t) * (size_t)n_targets, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    delete g;
    return hip_fail(e, "grids_build setup", __FILE__, __LINE__);
  }
  if (n_targets) {
    InFlight inflight;
    {
      PhaseClock pc(PH_ENQUEUE);
      rc = launch_grid_build(d_xy, d_offsets, n_scans, ids.as<const int32_t>(), n_targets, spec, L, g->grids.as<uint8_t>(), ws.p,
                             ws_bytes, nullptr, g->rebuilt);
    }
    if (rc == NHIP_OK) {
      PhaseClock pc(PH_WAIT);
      e = hipDeviceSynchronize();
      if (e != hipSuccess) rc = hip_fail(e, "grids_build sync", __FILE__, __LINE__);
      InFlight::done();
    }
    if (rc) {
      g->dirty = true;  // (a failed build: contents unknown)
      delete g;
      return rc;
    }
  }
  *out = g;
  return NHIP_OK;
}

int nhip_grids_build(const nhip_scans_t *scans, const int32_t *target_ids, int32_t n_targets,
                     const nhip_grid_spec_t *spec, nhip_grids_t **out) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(scans && out && n_targets >= 0 && (target_ids || n_targets == 0), "grids_build: bad arguments");
  phases_reset();
  for (int32_t i = 0; i < n_targets; i++)
    NHIP_REQUIRE(target_ids[i] >= 0 && target_ids[i] < scans->n_scans,
                 "grids_build: target id %d out of range", target_ids[i]);
  return grids_build_on(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), scans->n_scans, target_ids, n_targets,
                        spec, out);
}

int nhip_grids_build_submaps(const nhip_scans_t *scans, const int32_t *member_scan, const float *member_affine,
                             const int32_t *member_offsets, int32_t n_targets, const nhip_grid_spec_t *spec,
                             nhip_grids_t **out) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(scans && out && n_targets >= 0 && member_offsets, "grids_build_submaps: bad arguments");
  phases_reset();
  NHIP_REQUIRE(member_offsets[0] == 0, "grids_build_submaps: member_offsets[0] must be 0");
  for (int32_t t = 0; t < n_targets; t++)
    NHIP_REQUIRE(member_offsets[t + 1] >= member_offsets[t], "grids_build_submaps: member_offsets not monotone at target %d", t);
  const int32_t n_members = member_offsets[n_targets];
  NHIP_REQUIRE(n_members == 0 || (member_scan && member_affine), "grids_build_submaps: null member array");
  int64_t total = 0;  // points of all merged clouds: the host knows the scans' lengths
  for (int32_t m = 0; m < n_members; m++) {
    NHIP_REQUIRE(member_scan[m] >= 0 && member_scan[m] < scans->n_scans, "grids_build_submaps: member %d: scan id %d out of range",
                 m, member_scan[m]);
    total += scans->h_offsets[member_scan[m] + 1] - scans->h_offsets[member_scan[m]];
  }
  NHIP_REQUIRE(total <= 0x7fffffffll, "grids_build_submaps: the merged clouds hold %lld points; offsets are int32", (long long)total);
  {
    GridLayout L;  // (a bad spec fails before anything is allocated)
    if ((rc = make_layout(spec, &L))) return rc;
  }
  DevBuf d_scan, d_aff, d_moff, d_xy, d_off;
  if ((rc = d_scan.alloc(sizeof(int32_t) * (size_t)(n_members > 0 ? n_members : 1))) ||
      (rc = d_aff.alloc(sizeof(float) * 4 * (size_t)(n_members > 0 ? n_members : 1))) ||
      (rc = d_moff.alloc(sizeof(int32_t) * (size_t)(n_targets + 1))) ||
      (rc = d_xy.alloc(sizeof(float) * 2 * (size_t)(total > 0 ? total : 1))) ||
      (rc = d_off.alloc(sizeof(int32_t) * (size_t)(n_targets + 1))))
    return rc;
  {
    PhaseClock pc(PH_UPLOAD);
    if (n_members) {
      NHIP_TRY_HIP(hipMemcpy(d_scan.p, member_scan, sizeof(int32_t) * (size_t)n_members, hipMemcpyHostToDevice));
      NHIP_TRY_HIP(hipMemcpy(d_aff.p, member_affine, sizeof(float) * 4 * (size_t)n_members, hipMemcpyHostToDevice));
    }
    NHIP_TRY_HIP(hipMemcpy(d_moff.p, member_offsets, sizeof(int32_t) * (size_t)(n_targets + 1), hipMemcpyHostToDevice));
  }
  std::vector<int32_t> ids((size_t)n_targets);
  for (int32_t t = 0; t < n_targets; t++) ids[(size_t)t] = t;
  InFlight inflight;  // (the buffers above outlive the gather: grids_build_on returns with the device idle; a failure waits)
  {
    PhaseClock pc(PH_ENQUEUE);
    rc = launch_submap_gather(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), scans->n_scans,
                              d_scan.as<const int32_t>(), d_aff.as<const float>(), d_moff.as<const int32_t>(), n_targets,
                              d_xy.as<float>(), total, d_off.as<int32_t>(), nullptr);
  }
  if (rc) return rc;
  rc = grids_build_on(d_xy.as<const float>(), d_off.as<const int32_t>(), n_targets, ids.data(), n_targets, spec, out);
  if (rc) return rc;
  (*out)->submaps = true;
  if (n_targets == 0) {
    NHIP_TRY_HIP(hipStreamSynchronize(nullptr));  // (nothing was built: the offsets kernel alone ran)
    InFlight::done();
  }
  return NHIP_OK;
}

int nhip_grids_free(nhip_grids_t *grids) {
  phases_reset();
  if (grids && grids->n > 0 && !grids->dirty && grids->grids.p && grids->ws.p) {
    // the pair goes back with its contents known (see PoolEntry): the next build of this shape may rebuild into it
    const uint64_t key = g_pool_key.fetch_add(1);
    grids->grids.free(key, grids->shape << 1);
    grids->ws.free(key, (grids->shape << 1) | 1u);
  }
  delete grids;
  return NHIP_OK;
}

int nhip_grids_was_rebuilt(const nhip_grids_t *grids) { return grids && grids->rebuilt ? 1 : 0; }

// The plane downloads: the arguments each of them checks (`name`, for the message), then -- after the plane's own
// preconditions -- `bytes` at `offset` of the slot to the host.
static int plane_args(const nhip_grids_t *grids, int32_t slot, const void *out, const char *name, bool more = true) {
  NHIP_REQUIRE(grids && out && slot >= 0 && slot < grids->n && more, "%s: bad arguments", name);
  return NHIP_OK;
}
static int plane_fetch(const nhip_grids_t *grids, int32_t slot, int64_t offset, int64_t bytes, void *out) {
  NHIP_TRY_HIP(hipMemcpy(out, grids->grids.as<const uint8_t>() + (size_t)slot * grids->L.slot_bytes + offset, (size_t)bytes,
                         hipMemcpyDeviceToHost));
  return NHIP_OK;
}

int nhip_grids_download(const nhip_grids_t *grids, int32_t slot, uint8_t *out) {
  if (int rc = plane_args(grids, slot, out, "grids_download")) return rc;
  NHIP_REQUIRE(grids->L.has_image, "grids_download: the grids were built with NHIP_GRID_NO_IMAGE (nhip_grids_download_tiled16 / "
               "_hi_plane return the matcher's copies of the cells)");
  return plane_fetch(grids, slot, 0, grids->L.grid_bytes, out);
}

int nhip_grids_download_hi_plane_copy(const nhip_grids_t *grids, int32_t slot, int32_t copy, uint8_t *out) {
  if (int rc = plane_args(grids, slot, out, "grids_download_hi_plane", copy == 0 || copy == 1)) return rc;
  const GridLayout &L = grids->L;
  std::vector<uint8_t> raw((size_t)L.hi_bytes);
  if (int rc = plane_fetch(grids, slot, L.hi_offset, L.hi_bytes, raw.data())) return rc;
  const int32_t rows = L.S + 2 * L.pad;
  for (int32_t r = 0; r < rows; r++)
    for (int32_t c = 0; c < L.hi_pitch; c++)
      out[(size_t)r * L.hi_pitch + c] = raw[hi_tiled((uint32_t)r, (uint32_t)c, (uint32_t)copy, (uint32_t)L.hi_tpr, (uint32_t)L.hi_copy_bytes)];
  return NHIP_OK;
}

int nhip_grids_download_tiled16(const nhip_grids_t *grids, int32_t slot, uint8_t *out) {
  if (int rc = plane_args(grids, slot, out, "grids_download_tiled16")) return rc;
  const GridLayout &L = grids->L;
  NHIP_REQUIRE(L.t16_bytes > 0, "grids_download_tiled16: 8-bit grids have no tiled 16-bit copy");
  std::vector<uint8_t> raw((size_t)L.t16_bytes);
  if (int rc = plane_fetch(grids, slot, L.t16_offset, L.t16_bytes, raw.data())) return rc;
  const int32_t rows = L.S + 2 * L.pad;
  memset(out, 0, (size_t)L.plain_bytes);
  for (int32_t r = 0; r < rows; r++)
    for (int32_t c = 0; c < rows; c++)  // (square image: `rows` cells per row; the plain pitch may end before hi_pitch cells)
      memcpy(out + (size_t)r * L.pitch + 2 * (size_t)c, raw.data() + t16_tiled((uint32_t)r, (uint32_t)c, (uint32_t)L.t16_tpr), 2);
  return NHIP_OK;
}

int nhip_grids_download_hi_plane(const nhip_grids_t *grids, int32_t slot, uint8_t *out) {
  return nhip_grids_download_hi_plane_copy(grids, slot, 0, out);
}

int nhip_grids_download_skip_map(const nhip_grids_t *grids, int32_t slot, uint8_t *out) {
  if (int rc = plane_args(grids, slot, out, "grids_download_skip_map")) return rc;
  NHIP_REQUIRE(grids->L.has_image, "grids_download_skip_map: grids built with NHIP_GRID_NO_IMAGE carry no skip map");
  return plane_fetch(grids, slot, grids->L.skip_offset, grids->L.skip_bytes, out);
}

int nhip_grids_download_pool(const nhip_grids_t *grids, int32_t slot, uint8_t *out) {
  if (int rc = plane_args(grids, slot, out, "grids_download_pool")) return rc;
  return plane_fetch(grids, slot, grids->L.pool_offset, grids->L.pool_bytes, out);
}

int nhip_grids_download_hits(const nhip_grids_t *grids, int32_t slot, uint8_t *out) {
  if (int rc = plane_args(grids, slot, out, "grids_download_hits")) return rc;
  return plane_fetch(grids, slot, grids->L.hits_offset, grids->L.hits_bytes, out);
}

int nhip_grids_download_pool4(const nhip_grids_t *grids, int32_t slot, uint8_t *out) {
  if (int rc = plane_args(grids, slot, out, "grids_download_pool4")) return rc;
  // (rows x pitch: pool4_bytes may hold padding behind the table)
  return plane_fetch(grids, slot, grids->L.pool4_offset, (int64_t)grids->L.pool4_rows * grids->L.pool4_pitch, out);
}

int nhip_csm_match(const nhip_scans_t *scans, const nhip_grids_t *grids, const int32_t *pair_src,
                   const int32_t *pair_slot, const double *theta0, const int32_t *pair_origin,
                   int32_t n_pairs, const nhip_search_t *search, nhip_match_t *out,
                   int32_t *out_sums) {
  return nhip_csm_match_gated(scans, grids, pair_src, pair_slot, theta0, pair_origin, n_pairs, search, out, out_sums, -INFINITY);
}

int nhip_csm_match_gated(const nhip_scans_t *scans, const nhip_grids_t *grids, const int32_t *pair_src,
                         const int32_t *pair_slot, const double *theta0, const int32_t *pair_origin,
                         int32_t n_pairs, const nhip_search_t *search, nhip_match_t *out,
                         int32_t *out_sums, double min_score) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(!std::isnan(min_score), "csm_match: min_score is NaN");
  NHIP_REQUIRE(scans && grids && search && n_pairs >= 0, "csm_match: bad arguments");
  NHIP_REQUIRE(n_pairs == 0 || (pair_src && pair_slot && theta0 && out), "csm_match: null array");
  phases_reset();
  PhaseClock pc_host(PH_HOST);  // (the whole call; the phases below are inside it)
  for (int32_t i = 0; i < n_pairs; i++) {
    NHIP_REQUIRE(pair_src[i] >= 0 && pair_src[i] < scans->n_scans, "csm_match: pair %d source %d out of range", i, pair_src[i]);
    NHIP_REQUIRE(pair_slot[i] >= 0 && pair_slot[i] < grids->n, "csm_match: pair %d grid slot %d out of range", i, pair_slot[i]);
    if (pair_origin)
      NHIP_REQUIRE(abs(pair_origin[2 * i]) + (search->nx - 1) / 2 <= grids->spec.max_shift &&
                       abs(pair_origin[2 * i + 1]) + (search->ny - 1) / 2 <= grids->spec.max_shift,
                   "csm_match: pair %d search centre (%d, %d) exceeds the grids' max_shift %d", i,
                   pair_origin[2 * i], pair_origin[2 * i + 1], grids->spec.max_shift);
  }
  if (n_pairs == 0) return NHIP_OK;
  // sums are reported as int32: the longest scan whose largest possible sum fits
  const int64_t max_pts = 0x7fffffffll / (grids->L.cb == 2 ? 65535 : 255);
  for (int32_t i = 0; i < n_pairs; i++) {
    const int64_t n_i = (int64_t)scans->h_offsets[pair_src[i] + 1] - scans->h_offsets[pair_src[i]];
    NHIP_REQUIRE(n_i <= max_pts, "csm_match: pair %d: scan %d has %lld points; with %d-bit cells at most %lld fit the "
                 "int32 sums", i, pair_src[i], (long long)n_i, 8 * grids->L.cb, (long long)max_pts);
  }
  // the host knows the scan lengths: when every source fits the by-rotation form the general kernel is not launched
  nhip_search_t search_now = *search;
  {
    bool all_short = true;
    for (int32_t i = 0; i < n_pairs && all_short; i++)
      all_short = scans->h_offsets[pair_src[i] + 1] - scans->h_offsets[pair_src[i]] <= NHIP_SHORT_SCAN_POINTS;
    if (all_short) search_now.flags |= NHIP_SEARCH_SHORT_SCANS;
  }
  search = &search_now;
  const MatchPlan plan = csm_plan(grids->L, search, n_pairs);
  if ((rc = ensure_skip_maps(grids, plan))) return rc;
  nhip_grid_spec_t spec_now;
  spec_under_lock(const_cast<nhip_grids *>(grids), &spec_now);
  std::vector<double> rot0(2 * (size_t)n_pairs), delta(2 * (size_t)search->n_theta);
  if ((rc = nhip_csm_rot0(theta0, nullptr, n_pairs, rot0.data()))) return rc;
  if ((rc = nhip_csm_delta_table(search, delta.data()))) return rc;
  DevBuf d_src, d_slot, d_rot0, d_delta, d_keys, d_out, d_sums, d_org, d_ws;
  // The split form's workspace is 32 KB per pair (4.3 GB at 131,072 pairs, 8.6 GB beyond): on a GPU that cannot spare
  // it the list still matches -- with the hand-over lists alone, in the one-kernel form (same records).
  int64_t ws_bytes = bnb_workspace_bytes(n_pairs);
  if (d_ws.alloc((size_t)ws_bytes) != NHIP_OK) {
    (void)hipGetLastError();
    ws_bytes = bnb_workspace_bytes_lists(n_pairs);
    if ((rc = d_ws.alloc((size_t)ws_bytes))) return rc;
  }
  if (pair_origin) {
    if ((rc = d_org.alloc(sizeof(int32_t) * 2 * (size_t)n_pairs))) return rc;
    NHIP_TRY_HIP(hipMemcpy(d_org.p, pair_origin, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice));
  }
  if ((rc = d_src.alloc(sizeof(int32_t) * (size_t)n_pairs)) || (rc = d_slot.alloc(sizeof(int32_t) * (size_t)n_pairs)) ||
      (rc = d_rot0.alloc(sizeof(double) * rot0.size())) || (rc = d_delta.alloc(sizeof(double) * delta.size())) ||
      (rc = d_keys.alloc(sizeof(uint64_t) * (size_t)n_pairs)) || (rc = d_out.alloc(sizeof(nhip_match_t) * (size_t)n_pairs)) ||
      (rc = d_sums.alloc(sizeof(int32_t) * (size_t)n_pairs)))
    return rc;
  {
    PhaseClock pc(PH_UPLOAD);
    NHIP_TRY_HIP(hipMemcpy(d_src.p, pair_src, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice));
    NHIP_TRY_HIP(hipMemcpy(d_slot.p, pair_slot, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice));
    NHIP_TRY_HIP(hipMemcpy(d_rot0.p, rot0.data(), sizeof(double) * rot0.size(), hipMemcpyHostToDevice));
    NHIP_TRY_HIP(hipMemcpy(d_delta.p, delta.data(), sizeof(double) * delta.size(), hipMemcpyHostToDevice));
  }
  MatchJob job = job_on(scans->xy, scans->offsets, *grids, spec_now);
  job.ids = {scans->n_scans, grids->n, dev_status()};  // (checked on the host above; the kernels check again)
  job.pair_src = d_src.as<const int32_t>();
  job.pair_slot = d_slot.as<const int32_t>();
  job.rot0_cs = d_rot0.as<const double>();
  job.delta_cs = d_delta.as<const double>();
  job.pair_origin = pair_origin ? d_org.as<const int32_t>() : nullptr;
  job.n_pairs = n_pairs;
  job.search = search;
  job.min_score = min_score;
  job.keys = d_keys.as<uint64_t>();
  job.out = d_out.as<nhip_match_t>();
  job.sums = d_sums.as<int32_t>();
  job.workspace = d_ws.p;
  job.workspace_bytes = ws_bytes;
  PhaseClock pc_enq(PH_ENQUEUE);  // (to the end of the call minus the phases inside it; nhip_host_phases subtracts nothing:
                                  //  read it as "enqueue + wait + download + frees")
  InFlight inflight;  // (a failure from here on: the DevBufs above wait for the device before they return to the pool)
  rc = launch_csm_match(job, plan);
  if (rc) return rc;
  {
    PhaseClock pc(PH_WAIT);  // (the kernels; the downloads below find them done)
    NHIP_TRY_HIP(hipStreamSynchronize(nullptr));
    InFlight::done();
  }
  {
    PhaseClock pc(PH_DOWNLOAD);
    NHIP_TRY_HIP(hipMemcpy(out, d_out.p, sizeof(nhip_match_t) * (size_t)n_pairs, hipMemcpyDeviceToHost));
    if (out_sums) NHIP_TRY_HIP(hipMemcpy(out_sums, d_sums.p, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost));
  }
  return NHIP_OK;
}

int nhip_csm_scores(const nhip_scans_t *scans, const nhip_grids_t *grids, int32_t src, int32_t slot,
                    double theta0, int32_t origin_x, int32_t origin_y, const nhip_search_t *search,
                    int32_t *out_sums) {
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(scans && grids && search && out_sums, "csm_scores: bad arguments");
  NHIP_REQUIRE(src >= 0 && src < scans->n_scans && slot >= 0 && slot < grids->n, "csm_scores: index out of range");
  {
    // (the volume comes from the strip kernels, which read skip maps where they exist: built for the lattices an exhaustive
    //  search of a list takes the strip kernels for)
    nhip_search_t ex = *search;
    ex.flags = (ex.flags | NHIP_SEARCH_EXHAUSTIVE) & ~NHIP_SEARCH_LATENCY;
    if ((rc = ensure_skip_maps(grids, csm_plan(grids->L, &ex, 1)))) return rc;
  }
  double rot0[2];
  std::vector<double> delta(2 * (size_t)search->n_theta);
  if ((rc = nhip_csm_rot0(&theta0, nullptr, 1, rot0))) return rc;
  if ((rc = nhip_csm_delta_table(search, delta.data()))) return rc;
  const size_t vol = (size_t)search->n_theta * search->nx * search->ny;
  Staged st;
  MatchJob job = job_on(scans->xy, scans->offsets, *grids, grids->spec);  // (one pair, passed by value below: no pair arrays, ids, keys or records)
  job.rot0_cs = st.in(rot0, 2);
  job.delta_cs = st.in(delta.data(), delta.size());
  job.search = search;
  int32_t *d_vol = st.out<int32_t>(vol);
  if (st.ok()) st.launched(launch_csm_scores(job, src, slot, origin_x, origin_y, d_vol));
  st.fetch(out_sums, d_vol, vol);
  return st.finish();
}

int nhip_bnb_stats_per_pair(uint64_t *evaluated, int32_t n_pairs) {
  NHIP_REQUIRE(evaluated && n_pairs >= 0, "bnb_stats_per_pair: bad arguments");
  return bnb_stats_per_pair(reinterpret_cast<unsigned long long *>(evaluated), n_pairs);
}

int nhip_bnb_timeline(uint64_t *ticks, int32_t n_pairs) {
  NHIP_REQUIRE(ticks && n_pairs >= 0, "bnb_timeline: bad arguments");
  return bnb_timeline_read(reinterpret_cast<unsigned long long *>(ticks), n_pairs);
}

int nhip_bnb_timeline_candidates(uint64_t *ticks, int32_t n_pairs) {
  NHIP_REQUIRE(ticks && n_pairs >= 0, "bnb_timeline_candidates: bad arguments");
  return bnb_timeline_cand_read(reinterpret_cast<unsigned long long *>(ticks), n_pairs);
}

int nhip_bnb_stats(uint64_t *evaluated, uint64_t *total) {
  unsigned long long v[24];
  int rc = bnb_stats_read(v);
  if (rc) return rc;
  if (evaluated) *evaluated = v[0] + (v[3] + 3) / 4;  // in blocks: four sub-blocks = one block
  if (total) *total = v[1];
  return NHIP_OK;
}

int nhip_bnb_stats_levels(uint64_t out[24]) {
  NHIP_REQUIRE(out != nullptr, "bnb_stats_levels: null out");
  unsigned long long v[24];
  int rc = bnb_stats_read(v);
  if (rc) return rc;
  for (int i = 0; i < 24; i++) out[i] = v[i];
  return NHIP_OK;
}

int nhip_bnb_stats_chunks(uint64_t out[4]) {
  NHIP_REQUIRE(out != nullptr, "bnb_stats_chunks: null out");
  unsigned long long v[4];
  int rc = bnb_stats_chunks_read(v);
  if (rc) return rc;
  for (int i = 0; i < 4; i++) out[i] = v[i];
  return NHIP_OK;
}

int nhip_bnb_stats_seeds(uint64_t out[8]) {
  NHIP_REQUIRE(out != nullptr, "bnb_stats_seeds: null out");
  unsigned long long v[8];
  int rc = bnb_stats_seeds_read(v);
  if (rc) return rc;
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return NHIP_OK;
}

}  // extern "C"
