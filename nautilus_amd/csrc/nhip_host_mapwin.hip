// nhip_host_mapwin.hip -- the map-window entry points of the C ABI (kernels: nhip_mapwin.hip, K20): the spec's defaults and its
// check, the origins of priors (pure host), the workspace's size, the two forms on the caller's buffers and stream, and the
// host form with a host grid, host origins and host outputs.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

// the accepted ranges of include/nautilus_hip.h
int mapwin_spec_check(const nhip_mapwin_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(std::isfinite(s->res) && s->res > 0, "%s: res must be finite and > 0", who);
  NHIP_REQUIRE(s->width >= 1 && s->width <= 16384 && s->height >= 1 && s->height <= 16384,
               "%s: window of %d x %d cells outside 1..16384", who, s->width, s->height);
  NHIP_REQUIRE(s->side >= 2 && s->side <= 8192, "%s: side %d outside 2..8192", who, s->side);
  NHIP_REQUIRE(s->occ_min >= 1 && s->occ_min <= 100, "%s: occ_min %d outside 1..100", who, s->occ_min);
  NHIP_REQUIRE(s->flags == 0, "%s: flags %d must be 0", who, s->flags);
  NHIP_REQUIRE(s->reserved == 0, "%s: reserved %d must be 0", who, s->reserved);
  return NHIP_OK;
}

MapwinParams params_of(const nhip_mapwin_spec_t &spec, int64_t *d_stats) {
  MapwinParams P;
  P.width = spec.width, P.height = spec.height, P.cell_x0 = spec.cell_x0, P.cell_y0 = spec.cell_y0;
  P.side = spec.side, P.occ_min = spec.occ_min;
  P.res = spec.res;
  P.stats = reinterpret_cast<long long *>(d_stats);
  P.status = dev_status();
  return P;
}

constexpr int64_t MAPWIN_WS_ALIGN = 256;

}  // namespace

extern "C" {

int nhip_mapwin_spec_default(nhip_mapwin_spec_t *out) {
  NHIP_REQUIRE(out, "mapwin_spec_default: null pointer");
  *out = nhip_mapwin_spec_t{};
  out->res = 0.05;
  out->occ_min = 100;
  return NHIP_OK;
}

int nhip_mapwin_origins(const double *poses, int32_t n, double res, int32_t *origins, double *theta0) {
  NHIP_REQUIRE(n >= 0, "mapwin_origins: n %d must be >= 0", n);
  NHIP_REQUIRE(std::isfinite(res) && res > 0, "mapwin_origins: res must be finite and > 0");
  NHIP_REQUIRE(n == 0 || (poses && origins), "mapwin_origins: null pointer");
  for (int32_t i = 0; i < n; i++) {
    const double x = poses[3 * (size_t)i], y = poses[3 * (size_t)i + 1], th = poses[3 * (size_t)i + 2];
    NHIP_REQUIRE(std::isfinite(x) && std::isfinite(y) && std::isfinite(th), "mapwin_origins: pose %d is not finite", i);
    const double fx = std::floor(x / res), fy = std::floor(y / res);
    NHIP_REQUIRE(std::fabs(fx) < 0x1p30 && std::fabs(fy) < 0x1p30, "mapwin_origins: pose %d lies 2^30 cells or more from the origin", i);
    origins[2 * (size_t)i] = (int32_t)fx, origins[2 * (size_t)i + 1] = (int32_t)fy;
    if (theta0) theta0[i] = th;
  }
  return NHIP_OK;
}

int64_t nhip_mapwin_workspace_bytes(int32_t n_queries) {
  if (n_queries < 0) return 0;
  return (4 * (int64_t)n_queries + MAPWIN_WS_ALIGN) / MAPWIN_WS_ALIGN * MAPWIN_WS_ALIGN;
}

int nhip_mapwin_cells_dev(const int8_t *d_grid, const nhip_mapwin_spec_t *spec, int32_t max_cells, int32_t *d_row_ptr,
                          int32_t *d_cols, int64_t *d_stats, void *stream) {
  int rc = mapwin_spec_check(spec, "mapwin_cells_dev");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(max_cells >= 0, "mapwin_cells_dev: max_cells %d must be >= 0", max_cells);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_grid && d_row_ptr && d_stats && (max_cells == 0 || d_cols), "mapwin_cells_dev: null pointer");
  NHIP_REQUIRE(aligned(d_row_ptr, 4) && aligned(d_cols, 4) && aligned(d_stats, 8),
               "mapwin_cells_dev: d_row_ptr and d_cols must be 4-byte aligned, d_stats 8-byte aligned");
  return launch_mapwin_cells(params_of(*spec, d_stats), d_grid, max_cells, d_row_ptr, d_cols, static_cast<hipStream_t>(stream));
}

int nhip_mapwin_gather_dev(const int32_t *d_row_ptr, const int32_t *d_cols, const nhip_mapwin_spec_t *spec, const int32_t *d_origins,
                           int32_t n_queries, float *d_out_xy, int64_t out_capacity, int32_t *d_out_offsets, int64_t *d_stats,
                           void *d_workspace, int64_t workspace_bytes, void *stream) {
  int rc = mapwin_spec_check(spec, "mapwin_gather_dev");
  if (rc) return rc;
  NHIP_REQUIRE(n_queries >= 0, "mapwin_gather_dev: n_queries %d must be >= 0", n_queries);
  NHIP_REQUIRE(out_capacity >= 0, "mapwin_gather_dev: out_capacity %lld must be >= 0", (long long)out_capacity);
  NHIP_REQUIRE(workspace_bytes >= nhip_mapwin_workspace_bytes(n_queries), "mapwin_gather_dev: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)nhip_mapwin_workspace_bytes(n_queries));
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_row_ptr && d_out_offsets && d_stats && d_workspace && (n_queries == 0 || d_origins) && (out_capacity == 0 || d_out_xy),
               "mapwin_gather_dev: null pointer");
  NHIP_REQUIRE(aligned(d_out_xy, 8) && aligned(d_stats, 8) && aligned(d_workspace, 4) && aligned(d_row_ptr, 4) && aligned(d_cols, 4) &&
                   aligned(d_origins, 4) && aligned(d_out_offsets, 4),
               "mapwin_gather_dev: d_out_xy and d_stats must be 8-byte aligned, the int32 arrays and the workspace 4-byte aligned");
  return launch_mapwin_gather(params_of(*spec, d_stats), d_row_ptr, d_cols, d_origins, n_queries, d_out_xy, out_capacity, d_out_offsets,
                              static_cast<int32_t *>(d_workspace), static_cast<hipStream_t>(stream));
}

int nhip_map_windows(const int8_t *grid, const nhip_mapwin_spec_t *spec, const int32_t *origins, int32_t n_queries, float *out_xy,
                     int64_t capacity, int32_t *out_offsets, int64_t *stats) {
  int rc = mapwin_spec_check(spec, "map_windows");
  if (rc) return rc;
  NHIP_REQUIRE(n_queries >= 0, "map_windows: n_queries %d must be >= 0", n_queries);
  NHIP_REQUIRE(capacity >= 0, "map_windows: capacity %lld must be >= 0", (long long)capacity);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(grid && out_offsets && stats && (n_queries == 0 || origins) && (capacity == 0 || out_xy), "map_windows: null pointer");
  const size_t cells = (size_t)spec->width * (size_t)spec->height;
  int64_t n_occ = 0;  // (<= 2^28)
  for (size_t i = 0; i < cells; i++) n_occ += (int32_t)grid[i] >= spec->occ_min;
  const int64_t ws_bytes = nhip_mapwin_workspace_bytes(n_queries);
  Staged st;
  const int8_t *dg = st.in(grid, cells);
  const int32_t *dorg = st.in(origins, 2 * (size_t)n_queries);
  int32_t *drow = st.out<int32_t>((size_t)spec->height + 1), *dcols = st.out<int32_t>((size_t)n_occ);
  float *dxy = st.out<float>(2 * (size_t)capacity);
  int32_t *doff = st.out<int32_t>((size_t)n_queries + 1);
  int64_t *ds = st.out<int64_t>(STATS_WORDS);
  uint8_t *dws = st.out<uint8_t>((size_t)ws_bytes);
  if (st.ok()) {
    const MapwinParams P = params_of(*spec, ds);
    st.launched(launch_mapwin_cells(P, dg, (int32_t)n_occ, drow, dcols, nullptr));
    if (st.ok())
      st.launched(launch_mapwin_gather(P, drow, dcols, dorg, n_queries, dxy, capacity, doff, reinterpret_cast<int32_t *>(dws), nullptr));
  }
  st.fetch(out_offsets, doff, (size_t)n_queries + 1);
  st.fetch(stats, ds, STATS_WORDS);
  const size_t stored = st.ok() && out_offsets[n_queries] > 0 ? (size_t)out_offsets[n_queries] : 0;  // (<= capacity: the scan kernel's decision)
  st.fetch(out_xy, dxy, 2 * stored);
  return st.finish();
}

}  // extern "C"
