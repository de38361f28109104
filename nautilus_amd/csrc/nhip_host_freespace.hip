// nhip_host_freespace.hip -- the free-space check's entry points of the C ABI (kernels: nhip_freespace.hip, K15): the spec's
// defaults and its check, the two forms on the caller's buffers and stream, and the handle form that keeps a handle's planes.
#include "nhip_common.h"
#include "nhip_host.h"
#include "nhip_ray.h"

using namespace nhip;

namespace {

constexpr size_t FS_COUNTS = 8;  // int32 counts per pair (include/nautilus_hip.h)

// the accepted ranges of include/nautilus_hip.h
int freespace_spec_check(const nhip_freespace_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null free-space spec", who);
  NHIP_REQUIRE(s->hit_radius >= 0 && s->hit_radius <= 16, "%s: hit_radius %d outside 0..16 (the raster's zero border is %d cells)",
               who, s->hit_radius, HIT_PAD);
  NHIP_REQUIRE(s->end_margin >= 0 && s->end_margin <= 64, "%s: end_margin %d outside 0..64", who, s->end_margin);
  NHIP_REQUIRE(s->flags == 0, "%s: flags %d must be 0", who, s->flags);
  NHIP_REQUIRE(s->reserved == 0, "%s: reserved %d must be 0", who, s->reserved);
  return NHIP_OK;
}

// the layout of grids the check takes: every layout keeps the hit raster; the ray's int32 bound limits the side
int freespace_layout(const nhip_grid_spec_t *grid_spec, const char *who, GridLayout *L) {
  NHIP_REQUIRE(grid_spec, "%s: null grid spec", who);
  int rc = make_layout(grid_spec, L);
  if (rc) return rc;
  NHIP_REQUIRE(L->S / 2 <= RAY_MAX_CELLS, "%s: a grid of side %d: side / 2 exceeds %d, the ray's int32 bound", who, L->S, RAY_MAX_CELLS);
  NHIP_REQUIRE(L->hits_bytes > 0 && L->hits_pitch > 0, "%s: the grids keep no hit raster", who);
  return NHIP_OK;
}

int search_check(const nhip_search_t *search, const char *who) {
  NHIP_REQUIRE(search, "%s: null search", who);
  NHIP_REQUIRE(search->n_theta >= 1 && search->nx >= 1 && search->ny >= 1, "%s: lattice %d x %d x %d", who, search->n_theta,
               search->nx, search->ny);
  return NHIP_OK;
}

FsParams fs_params(const GridLayout &L, const nhip_grid_spec_t &grid_spec, const float *d_xy, const int32_t *d_offsets,
                   int32_t n_scans, const uint8_t *d_grids, int32_t n_slots, uint8_t *d_free) {
  FsParams P;
  memset(&P, 0, sizeof(P));
  P.xy = reinterpret_cast<const float2 *>(d_xy);
  P.offsets = d_offsets;
  P.grids = d_grids;
  P.free_planes = d_free;
  P.S = L.S, P.hits_pitch = L.hits_pitch;
  P.slot_bytes = L.slot_bytes, P.hits_offset = L.hits_offset, P.hits_bytes = L.hits_bytes;
  P.res = grid_spec.res, P.inv_res = 1.0 / grid_spec.res;
  P.ids = {n_scans, n_slots, dev_status()};
  return P;
}

// the fields of a check beside fs_params': the pair arrays, the lattice, the spec, the counts
void fs_check_fields(FsParams &P, const int32_t *d_pair_src, const int32_t *d_pair_slot, const int32_t *d_pair_origin,
                     const double *d_rot0_cs, const double *d_delta_cs, const nhip_match_t *d_matches, int32_t n_pairs,
                     const nhip_search_t &search, const nhip_freespace_spec_t &fs_spec, int32_t *d_counts) {
  P.pair_src = d_pair_src, P.pair_slot = d_pair_slot, P.pair_origin = d_pair_origin;
  P.rot0_cs = d_rot0_cs, P.delta_cs = d_delta_cs;
  P.matches = d_matches;
  P.counts = d_counts;
  P.n_pairs = n_pairs;
  P.n_theta = search.n_theta, P.nx = search.nx, P.ny = search.ny;
  P.hx = (search.nx - 1) / 2, P.hy = (search.ny - 1) / 2;
  P.hit_radius = fs_spec.hit_radius, P.end_margin = fs_spec.end_margin;
}

}  // namespace

extern "C" {

int nhip_freespace_spec_default(nhip_freespace_spec_t *out) {
  NHIP_REQUIRE(out, "freespace_spec_default: null pointer");
  *out = nhip_freespace_spec_t{};
  out->hit_radius = 2;
  out->end_margin = 3;
  return NHIP_OK;
}

int64_t nhip_freespace_planes_bytes(const nhip_grid_spec_t *grid_spec, int64_t n_slots) {
  GridLayout L;
  if (freespace_layout(grid_spec, "freespace_planes_bytes", &L)) return -1;
  return (n_slots > 0 ? n_slots : 0) * L.hits_bytes;
}

int nhip_freespace_trace_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids,
                             int32_t n_targets, const nhip_grid_spec_t *grid_spec, const uint8_t *d_grids, uint8_t *d_free,
                             void *stream) {
  GridLayout L;
  int rc = freespace_layout(grid_spec, "freespace_trace_dev", &L);  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(n_targets >= 0 && n_scans >= 0, "freespace_trace_dev: n_targets %d / n_scans %d < 0", n_targets, n_scans);
  if ((rc = require_device())) return rc;
  if (n_targets == 0) return NHIP_OK;
  NHIP_REQUIRE(d_xy && d_offsets && d_target_ids && d_grids && d_free, "freespace_trace_dev: null pointer");
  NHIP_REQUIRE(aligned(d_grids, 4) && aligned(d_free, 16), "freespace_trace_dev: d_grids must be 4-byte aligned, d_free 16-byte");
  FsParams P = fs_params(L, *grid_spec, d_xy, d_offsets, n_scans, d_grids, n_targets, d_free);
  P.target_ids = d_target_ids;
  P.n_targets = n_targets;
  return launch_fs_trace(P, static_cast<hipStream_t>(stream));
}

int nhip_freespace_check_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                             int32_t n_grids, const nhip_grid_spec_t *grid_spec, const int32_t *d_pair_src,
                             const int32_t *d_pair_slot, const double *d_rot0_cs, const double *d_delta_cs,
                             const int32_t *d_pair_origin, int32_t n_pairs, const nhip_search_t *search, const uint8_t *d_free,
                             const nhip_match_t *d_matches, const nhip_freespace_spec_t *fs_spec, int32_t *d_counts,
                             void *stream) {
  int rc = freespace_spec_check(fs_spec, "freespace_check_dev");
  if (rc || (rc = search_check(search, "freespace_check_dev"))) return rc;
  GridLayout L;
  if ((rc = freespace_layout(grid_spec, "freespace_check_dev", &L))) return rc;
  NHIP_REQUIRE(n_pairs >= 0 && n_scans >= 0 && n_grids >= 0, "freespace_check_dev: negative count (n_pairs %d, n_scans %d, n_grids %d)",
               n_pairs, n_scans, n_grids);
  if ((rc = require_device())) return rc;
  if (n_pairs == 0) return NHIP_OK;
  NHIP_REQUIRE(d_xy && d_offsets && d_grids && d_pair_src && d_pair_slot && d_rot0_cs && d_delta_cs && d_free && d_matches && d_counts,
               "freespace_check_dev: null pointer");
  NHIP_REQUIRE(aligned(d_grids, 4) && aligned(d_free, 4) && aligned(d_matches, 4) && aligned(d_counts, 4),
               "freespace_check_dev: d_grids, d_free, d_matches and d_counts must be 4-byte aligned");
  FsParams P = fs_params(L, *grid_spec, d_xy, d_offsets, n_scans, d_grids, n_grids, const_cast<uint8_t *>(d_free));
  fs_check_fields(P, d_pair_src, d_pair_slot, d_pair_origin, d_rot0_cs, d_delta_cs, d_matches, n_pairs, *search, *fs_spec, d_counts);
  return launch_fs_check(P, static_cast<hipStream_t>(stream));
}

int nhip_csm_freespace(const nhip_scans_t *scans, const nhip_grids_t *grids, const int32_t *pair_src, const int32_t *pair_slot,
                       const double *theta0, const int32_t *pair_origin, int32_t n_pairs, const nhip_search_t *search,
                       const nhip_match_t *matches, const nhip_freespace_spec_t *fs_spec, int32_t *counts) {
  int rc = freespace_spec_check(fs_spec, "csm_freespace");
  if (rc || (rc = search_check(search, "csm_freespace")) || (rc = require_device())) return rc;
  NHIP_REQUIRE(scans && grids && n_pairs >= 0, "csm_freespace: bad arguments");
  NHIP_REQUIRE(n_pairs == 0 || (pair_src && pair_slot && theta0 && matches && counts), "csm_freespace: null array");
  if (grids->submaps) {
    set_error("csm_freespace: the grids are submaps (nhip_grids_build_submaps): a submap's free space needs one ray origin per member");
    return NHIP_ERR_STATE;
  }
  nhip_grids *g = const_cast<nhip_grids *>(grids);
  GridLayout L;
  if ((rc = freespace_layout(&g->spec, "csm_freespace", &L))) return rc;
  for (int32_t i = 0; i < n_pairs; i++) {
    NHIP_REQUIRE(pair_src[i] >= 0 && pair_src[i] < scans->n_scans, "csm_freespace: pair %d source %d out of range", i, pair_src[i]);
    NHIP_REQUIRE(pair_slot[i] >= 0 && pair_slot[i] < g->n, "csm_freespace: pair %d grid slot %d out of range", i, pair_slot[i]);
    NHIP_REQUIRE(matches[i].itheta < search->n_theta && (matches[i].itheta < 0 || (matches[i].ix >= 0 && matches[i].ix < search->nx &&
                                                                                 matches[i].iy >= 0 && matches[i].iy < search->ny)),
                 "csm_freespace: pair %d: record (%d, %d, %d) outside the lattice", i, matches[i].itheta, matches[i].ix, matches[i].iy);
  }
  for (int32_t t = 0; t < g->n; t++)
    NHIP_REQUIRE(g->target_ids[(size_t)t] < scans->n_scans, "csm_freespace: slot %d was built from scan %d; these scans hold %d", t,
                 g->target_ids[(size_t)t], scans->n_scans);
  if (n_pairs == 0) return NHIP_OK;
  const size_t N = (size_t)n_pairs;
  {
    // the handle's planes: traced by the first check, under the handle's mutex (concurrent calls are ordered, the loser finds
    // them traced).  A staged call of its own: it has finished, and its list is back in the pool, before the lock is released.
    std::lock_guard<std::mutex> lock(g->mu);
    if (!g->free_traced) {
      if ((rc = g->free_planes.alloc((size_t)g->n * (size_t)L.hits_bytes))) return rc;
      Staged tr;
      FsParams T = fs_params(L, g->spec, scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), scans->n_scans,
                             g->grids.as<const uint8_t>(), g->n, g->free_planes.as<uint8_t>());
      T.target_ids = tr.in(g->target_ids.data(), (size_t)g->n);
      T.n_targets = g->n;
      if (tr.ok()) tr.launched(launch_fs_trace(T, nullptr));
      if ((rc = tr.finish())) return rc;  // (waits for the null stream)
      g->free_traced = true;
    }
  }
  std::vector<double> rot0(2 * N), delta(2 * (size_t)search->n_theta);
  if ((rc = nhip_csm_rot0(theta0, nullptr, n_pairs, rot0.data()))) return rc;
  if ((rc = nhip_csm_delta_table(search, delta.data()))) return rc;
  Staged st;
  const int32_t *d_src = st.in(pair_src, N), *d_slot = st.in(pair_slot, N);
  const double *d_rot0 = st.in(rot0.data(), rot0.size()), *d_delta = st.in(delta.data(), delta.size());
  const nhip_match_t *d_m = st.in(matches, N);
  int32_t *d_counts = st.out<int32_t>(FS_COUNTS * N);
  const int32_t *d_org = pair_origin ? st.in(pair_origin, 2 * N) : nullptr;  // (null: every pair's window at the slot's origin)
  FsParams P = fs_params(L, g->spec, scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), scans->n_scans,
                         g->grids.as<const uint8_t>(), g->n, g->free_planes.as<uint8_t>());
  fs_check_fields(P, d_src, d_slot, d_org, d_rot0, d_delta, d_m, n_pairs, *search, *fs_spec, d_counts);
  if (st.ok()) st.launched(launch_fs_check(P, nullptr));
  st.fetch(counts, d_counts, FS_COUNTS * N);
  return st.finish();
}

}  // extern "C"
