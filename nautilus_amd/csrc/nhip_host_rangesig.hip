// nhip_host_rangesig.hip -- the range-signature entry points of the C ABI (kernels: nhip_rangesig.hip, K21): the spec's
// defaults and its check, the ray and edge tables (pure host), the workspace rule, the four forms on the caller's buffers and
// stream, and the host form with a host grid, host scans and host outputs.
#include "nhip_common.h"
#include "nhip_host.h"
#include "nhip_ray.h"  // (RAY_MAX_CELLS)

using namespace nhip;

namespace {

constexpr int64_t RANGESIG_WS_MIN = 4 * ((int64_t)RANGESIG_MAX_NODES_PER_AXIS + 1) / 256 * 256 + 256;  // the anchors' row counts
constexpr int32_t RANGESIG_MAX_CHUNK_ROWS = 1 << 18;  // (a launch's grid: chunk rows / RANGESIG_QT workgroups along y)
constexpr double TWO_PI = 6.283185307179586476925286766559;

// the accepted ranges of include/nautilus_hip.h
int rangesig_spec_check(const nhip_rangesig_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(std::isfinite(s->res) && s->res > 0, "%s: res must be finite and > 0", who);
  NHIP_REQUIRE(std::isfinite(s->unit) && s->unit > 0, "%s: unit must be finite and > 0", who);
  NHIP_REQUIRE(s->width >= 1 && s->width <= 16384 && s->height >= 1 && s->height <= 16384,
               "%s: window of %d x %d cells outside 1..16384", who, s->width, s->height);
  NHIP_REQUIRE(s->occ_min >= 1 && s->occ_min <= 127, "%s: occ_min %d outside 1..127", who, s->occ_min);
  NHIP_REQUIRE(s->free_max >= 0 && s->free_max < s->occ_min, "%s: free_max %d outside 0..occ_min - 1 = %d", who, s->free_max, s->occ_min - 1);
  NHIP_REQUIRE(s->stride >= 1 && s->stride <= 1024, "%s: stride %d outside 1..1024", who, s->stride);
  NHIP_REQUIRE(s->max_ray_cells >= 1 && s->max_ray_cells <= RAY_MAX_CELLS, "%s: max_ray_cells %d outside 1..%d", who, s->max_ray_cells,
               RAY_MAX_CELLS);
  NHIP_REQUIRE(s->rays_per_sector == 1 || s->rays_per_sector == 2 || s->rays_per_sector == 4 || s->rays_per_sector == 8,
               "%s: rays_per_sector %d is not 1, 2, 4 or 8", who, s->rays_per_sector);
  NHIP_REQUIRE(s->top_k >= 1 && s->top_k <= 16, "%s: top_k %d outside 1..16", who, s->top_k);
  NHIP_REQUIRE(s->min_sep >= 0 && s->min_sep <= 64, "%s: min_sep %d outside 0..64", who, s->min_sep);
  NHIP_REQUIRE(s->min_sectors >= 1 && s->min_sectors <= 64, "%s: min_sectors %d outside 1..64", who, s->min_sectors);
  NHIP_REQUIRE(s->flags == 0 || s->flags == NHIP_RANGESIG_UNKNOWN_STOPS, "%s: flags %d: 0 or NHIP_RANGESIG_UNKNOWN_STOPS", who, s->flags);
  NHIP_REQUIRE(s->reserved == 0, "%s: reserved %d must be 0", who, s->reserved);
  return NHIP_OK;
}

// item 2 of the spec; either output may be null (the check of n scale < 2^31 is made either way)
int rangesig_tables(const nhip_rangesig_spec_t &s, int32_t *rays, float *edge2, const char *who) {
  const int32_t m = s.rays_per_sector, L = s.max_ray_cells;
  const double w = TWO_PI / 64;
  for (int32_t t = 0; t < 64 * m; t++) {
    const double phi = (t + 0.5) * w / m;
    const long dx = std::lrint(L * std::cos(phi)), dy = std::lrint(L * std::sin(phi));
    const long n = std::labs(dx) > std::labs(dy) ? std::labs(dx) : std::labs(dy);
    NHIP_REQUIRE(n >= 1, "%s: ray %d has no step", who, t);
    const double sc = 65536.0 * std::sqrt((double)(dx * dx + dy * dy)) * s.res / ((double)n * s.unit);
    NHIP_REQUIRE(std::isfinite(sc) && sc * (double)n < 2147483647.0,
                 "%s: res / unit = %g is too large for rays of %d cells: a range in units times 2^16 must stay below 2^31", who,
                 s.res / s.unit, L);
    const long scale = std::lrint(sc);
    NHIP_REQUIRE((long long)n * (long long)scale < 0x80000000ll, "%s: res / unit = %g is too large for rays of %d cells", who,
                 s.res / s.unit, L);
    if (rays) rays[4 * t] = (int32_t)dx, rays[4 * t + 1] = (int32_t)dy, rays[4 * t + 2] = (int32_t)n, rays[4 * t + 3] = (int32_t)scale;
  }
  if (edge2) {
    edge2[0] = 0.0f;
    for (int k = 1; k <= 254; k++) {
      const float e = (float)(s.unit * k);
      edge2[k] = e * e;
    }
  }
  return NHIP_OK;
}

// spec and tables: what every compute entry point asks before it looks for a device
int rangesig_check(const nhip_rangesig_spec_t *s, const char *who) {
  int rc = rangesig_spec_check(s, who);
  return rc ? rc : rangesig_tables(*s, nullptr, nullptr, who);
}

RangesigParams params_of(const nhip_rangesig_spec_t &spec, int64_t *d_stats) {
  RangesigParams P;
  P.width = spec.width, P.height = spec.height, P.occ_min = spec.occ_min, P.free_max = spec.free_max, P.stride = spec.stride;
  P.rays_per_sector = spec.rays_per_sector, P.top_k = spec.top_k, P.min_sep = spec.min_sep, P.min_sectors = spec.min_sectors, P.flags = spec.flags;
  P.stats = reinterpret_cast<long long *>(d_stats);
  P.status = dev_status();
  return P;
}

RangesigScanTables scan_tables_of(const nhip_rangesig_spec_t &spec) {
  RangesigScanTables T;
  std::memset(&T, 0, sizeof(T));
  (void)rangesig_tables(spec, nullptr, T.edge2, "rangesig");  // (checked before)
  for (int j = 0; j < 32; j++) T.dir[2 * j] = (float)std::cos(TWO_PI * j / 64), T.dir[2 * j + 1] = (float)std::sin(TWO_PI * j / 64);
  return T;
}

int64_t key_row_bytes(int32_t n_anchors) { return 4 * (((int64_t)(n_anchors > 0 ? n_anchors : 1) + 63) & ~63ll); }

// the arguments have been checked
int rangesig_match_run(const uint8_t *d_qsig, int32_t n_queries, const uint8_t *d_asig, const int32_t *d_anchors, int32_t n_anchors,
                       const nhip_rangesig_spec_t &spec, int32_t *d_records, int64_t *d_stats, void *d_ws, int64_t ws_bytes,
                       hipStream_t s) {
  const int64_t row = key_row_bytes(n_anchors);
  int64_t rows = ws_bytes / row;
  NHIP_REQUIRE(rows >= 1, "rangesig_match: a workspace of %lld bytes holds no row of %lld bytes", (long long)ws_bytes, (long long)row);
  if (rows > RANGESIG_MAX_CHUNK_ROWS) rows = RANGESIG_MAX_CHUNK_ROWS;
  return launch_rangesig_match(params_of(spec, d_stats), d_qsig, n_queries, d_asig, d_anchors, n_anchors, d_records,
                               static_cast<uint32_t *>(d_ws), (int32_t)(row / 4), (int32_t)rows, s);
}

}  // namespace

extern "C" {

int nhip_rangesig_spec_default(nhip_rangesig_spec_t *out) {
  NHIP_REQUIRE(out, "rangesig_spec_default: null pointer");
  *out = nhip_rangesig_spec_t{};
  out->res = 0.05;
  out->unit = 0.125;
  out->occ_min = 100;
  out->free_max = 0;
  out->stride = 10;
  out->max_ray_cells = 600;
  out->rays_per_sector = 4;
  out->top_k = 5;
  out->min_sep = 2;
  out->min_sectors = 8;
  return NHIP_OK;
}

int nhip_rangesig_tables(const nhip_rangesig_spec_t *spec, int32_t *rays, float *edge2) {
  int rc = rangesig_spec_check(spec, "rangesig_tables");
  return rc ? rc : rangesig_tables(*spec, rays, edge2, "rangesig_tables");
}

int64_t nhip_rangesig_workspace_bytes(const nhip_rangesig_spec_t *spec, int32_t n_anchors, int32_t n_queries) {
  if (rangesig_spec_check(spec, "rangesig_workspace_bytes")) return -1;
  if (n_anchors < 0 || n_anchors > RANGESIG_MAX_ANCHORS || n_queries < 0) {
    set_error("rangesig_workspace_bytes: n_anchors %d outside 0..%d or n_queries %d below 0", n_anchors, RANGESIG_MAX_ANCHORS, n_queries);
    return -1;
  }
  const int64_t row = key_row_bytes(n_anchors), fit = NHIP_RANGESIG_WORKSPACE_MAX / row;
  const int64_t rows = n_queries < 1 ? 1 : n_queries <= fit ? n_queries : fit < 1 ? 1 : fit;
  const int64_t bytes = rows * row;
  return bytes < RANGESIG_WS_MIN ? RANGESIG_WS_MIN : bytes;
}

int nhip_rangesig_anchors_dev(const int8_t *d_grid, const nhip_rangesig_spec_t *spec, int32_t max_anchors, int32_t *d_anchors,
                              int64_t *d_stats, void *d_workspace, int64_t workspace_bytes, void *stream) {
  int rc = rangesig_check(spec, "rangesig_anchors_dev");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(max_anchors >= 0 && max_anchors <= RANGESIG_MAX_ANCHORS, "rangesig_anchors_dev: max_anchors %d outside 0..%d", max_anchors,
               RANGESIG_MAX_ANCHORS);
  NHIP_REQUIRE(workspace_bytes >= RANGESIG_WS_MIN, "rangesig_anchors_dev: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)RANGESIG_WS_MIN);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_grid && d_stats && d_workspace && (max_anchors == 0 || d_anchors), "rangesig_anchors_dev: null pointer");
  NHIP_REQUIRE(aligned(d_anchors, 16) && aligned(d_stats, 8) && aligned(d_workspace, 4),
               "rangesig_anchors_dev: d_anchors must be 16-byte aligned, d_stats 8-byte, d_workspace 4-byte");
  return launch_rangesig_anchors(params_of(*spec, d_stats), d_grid, max_anchors, d_anchors, static_cast<int32_t *>(d_workspace),
                                 static_cast<hipStream_t>(stream));
}

int nhip_rangesig_map_dev(const int8_t *d_grid, const nhip_rangesig_spec_t *spec, const int32_t *d_rays, const int32_t *d_anchors,
                          int32_t n_anchors, uint8_t *d_sig, int64_t *d_stats, void *stream) {
  int rc = rangesig_check(spec, "rangesig_map_dev");
  if (rc) return rc;
  NHIP_REQUIRE(n_anchors >= 0 && n_anchors <= RANGESIG_MAX_ANCHORS, "rangesig_map_dev: n_anchors %d outside 0..%d", n_anchors,
               RANGESIG_MAX_ANCHORS);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_grid && d_rays && d_stats && (n_anchors == 0 || (d_anchors && d_sig)), "rangesig_map_dev: null pointer");
  NHIP_REQUIRE(aligned(d_rays, 16) && aligned(d_anchors, 16) && aligned(d_stats, 8) && aligned(d_sig, 4),
               "rangesig_map_dev: d_rays and d_anchors must be 16-byte aligned, d_stats 8-byte, d_sig 4-byte");
  return launch_rangesig_map(params_of(*spec, d_stats), d_grid, d_rays, d_anchors, n_anchors, d_sig, static_cast<hipStream_t>(stream));
}

int nhip_rangesig_scans_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_rangesig_spec_t *spec,
                            uint8_t *d_sig, void *stream) {
  int rc = rangesig_check(spec, "rangesig_scans_dev");
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0, "rangesig_scans_dev: n_scans %d must be >= 0", n_scans);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(n_scans == 0 || (d_xy && d_offsets && d_sig), "rangesig_scans_dev: null pointer");
  NHIP_REQUIRE(aligned(d_xy, 8) && aligned(d_offsets, 4) && aligned(d_sig, 4),
               "rangesig_scans_dev: d_xy must be 8-byte aligned, d_offsets and d_sig 4-byte");
  return launch_rangesig_scans(scan_tables_of(*spec), d_xy, d_offsets, n_scans, d_sig, static_cast<hipStream_t>(stream));
}

int nhip_rangesig_match_dev(const uint8_t *d_query_sig, int32_t n_queries, const uint8_t *d_map_sig, const int32_t *d_anchors,
                            int32_t n_anchors, const nhip_rangesig_spec_t *spec, int32_t *d_records, int64_t *d_stats,
                            void *d_workspace, int64_t workspace_bytes, void *stream) {
  int rc = rangesig_check(spec, "rangesig_match_dev");
  if (rc) return rc;
  NHIP_REQUIRE(n_queries >= 0 && n_anchors >= 0 && n_anchors <= RANGESIG_MAX_ANCHORS,
               "rangesig_match_dev: n_queries %d must be >= 0, n_anchors %d in 0..%d", n_queries, n_anchors, RANGESIG_MAX_ANCHORS);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_stats && (n_queries == 0 || (d_query_sig && d_records && d_workspace)) && (n_anchors == 0 || (d_map_sig && d_anchors)),
               "rangesig_match_dev: null pointer");
  NHIP_REQUIRE(aligned(d_query_sig, 4) && aligned(d_map_sig, 4) && aligned(d_anchors, 16) && aligned(d_records, 4) && aligned(d_stats, 8) &&
                   aligned(d_workspace, 4),
               "rangesig_match_dev: d_anchors must be 16-byte aligned, d_stats 8-byte, the signatures, records and workspace 4-byte");
  return rangesig_match_run(d_query_sig, n_queries, d_map_sig, d_anchors, n_anchors, *spec, d_records, d_stats, d_workspace,
                            workspace_bytes, static_cast<hipStream_t>(stream));
}

int nhip_rangesig_candidates(const int8_t *grid, const nhip_rangesig_spec_t *spec, const float *xy, const int32_t *offsets,
                             int32_t n_scans, int32_t max_anchors, int32_t *records, int32_t *anchors, int32_t *n_anchors,
                             int64_t *stats, uint8_t *map_sig, uint8_t *scan_sig) {
  int rc = rangesig_check(spec, "rangesig_candidates");
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0 && max_anchors >= 0 && max_anchors <= RANGESIG_MAX_ANCHORS,
               "rangesig_candidates: n_scans %d must be >= 0, max_anchors %d in 0..%d", n_scans, max_anchors, RANGESIG_MAX_ANCHORS);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(grid && offsets && n_anchors && stats && (n_scans == 0 || records) && (max_anchors == 0 || anchors),
               "rangesig_candidates: null pointer");
  NHIP_REQUIRE(offsets[0] == 0, "rangesig_candidates: offsets[0] = %d must be 0", offsets[0]);
  for (int32_t i = 0; i < n_scans; i++)
    NHIP_REQUIRE(offsets[i + 1] >= offsets[i], "rangesig_candidates: offsets[%d] = %d after %d: the offsets must ascend", i + 1,
                 offsets[i + 1], offsets[i]);
  const size_t n_points = (size_t)offsets[n_scans];
  NHIP_REQUIRE(n_points == 0 || xy, "rangesig_candidates: null points");
  const size_t cells = (size_t)spec->width * (size_t)spec->height;
  const int32_t h = spec->stride / 2;
  int64_t found = 0;  // (<= 2^28)
  for (int32_t y = h; y < spec->height; y += spec->stride)
    for (int32_t x = h; x < spec->width; x += spec->stride) {
      const int32_t v = grid[(size_t)y * (size_t)spec->width + (size_t)x];
      found += v >= 0 && v <= spec->free_max;
    }
  const int32_t held = (int32_t)(found < max_anchors ? found : max_anchors);
  *n_anchors = held;
  const int32_t n_rays = 64 * spec->rays_per_sector;
  std::vector<int32_t> rays(4 * (size_t)n_rays);
  (void)rangesig_tables(*spec, rays.data(), nullptr, "rangesig_candidates");  // (checked above)
  const int64_t ws_bytes = nhip_rangesig_workspace_bytes(spec, held, n_scans);
  const size_t n_rec = 4 * (size_t)spec->top_k * (size_t)n_scans;
  Staged st;
  const int8_t *dg = st.in(grid, cells);
  const float *dxy = st.in(xy, 2 * n_points);
  const int32_t *doff = st.in(offsets, (size_t)n_scans + 1);
  const int32_t *drays = st.in(rays.data(), rays.size());
  int32_t *dan = st.out<int32_t>(4 * (size_t)held);
  uint8_t *dasig = st.out<uint8_t>(64 * (size_t)held), *dqsig = st.out<uint8_t>(64 * (size_t)n_scans);
  int32_t *drec = st.out<int32_t>(n_rec);
  int64_t *ds = st.out<int64_t>(STATS_WORDS);
  uint8_t *dws = st.out<uint8_t>((size_t)ws_bytes);
  if (st.ok()) {
    const RangesigParams P = params_of(*spec, ds);
    st.launched(launch_rangesig_anchors(P, dg, held, dan, reinterpret_cast<int32_t *>(dws), nullptr));
    if (st.ok()) st.launched(launch_rangesig_map(P, dg, drays, dan, held, dasig, nullptr));
    if (st.ok()) st.launched(launch_rangesig_scans(scan_tables_of(*spec), dxy, doff, n_scans, dqsig, nullptr));
    if (st.ok()) st.launched(rangesig_match_run(dqsig, n_scans, dasig, dan, held, *spec, drec, ds, dws, ws_bytes, nullptr));
  }
  st.fetch(records, drec, n_rec);
  st.fetch(stats, ds, STATS_WORDS);
  st.fetch(anchors, dan, 4 * (size_t)held);
  st.fetch(map_sig, dasig, 64 * (size_t)held);
  st.fetch(scan_sig, dqsig, 64 * (size_t)n_scans);
  return st.finish();
}

}  // extern "C"
