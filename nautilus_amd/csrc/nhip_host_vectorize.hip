// nhip_host_vectorize.hip -- the map-vectorisation entry points of the C ABI (kernels: nhip_vectorize.hip, K13): the spec's
// defaults and its check, the tables, the pose affines, the workspace's layout, the host loop over the rounds (drive_pcg's
// pattern, nhip_host_linsolve.hip: rounds are enqueued check_every at a time, one look at the end word between two batches),
// the handle form, and the endpoints of the records -- in double, on the host.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

constexpr int VQ = 14;
constexpr size_t REC_WORDS = 10;  // a segment record: ten int64 words (include/nautilus_hip.h)

// the accepted ranges of include/nautilus_hip.h
int vectorize_spec_check(const nhip_vectorize_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  NHIP_REQUIRE(std::isfinite(s->res) && s->res > 0, "%s: res must be finite and > 0", who);
  NHIP_REQUIRE(s->width >= 1 && s->width <= 16384 && s->height >= 1 && s->height <= 16384,
               "%s: window of %d x %d cells outside 1..16384", who, s->width, s->height);
  NHIP_REQUIRE(s->min_hits >= 1 && s->min_hits <= (1 << 30), "%s: min_hits %d outside 1..2^30", who, s->min_hits);
  NHIP_REQUIRE(s->n_theta >= 2 && s->n_theta <= 1024, "%s: n_theta %d outside 2..1024", who, s->n_theta);
  NHIP_REQUIRE(s->min_votes >= 1, "%s: min_votes %d must be >= 1", who, s->min_votes);
  NHIP_REQUIRE(std::isfinite(s->band) && s->band >= 0.5 && s->band <= 65536.0, "%s: band must be finite and in 0.5..65536 cells", who);
  NHIP_REQUIRE(s->max_gap >= 0, "%s: max_gap %d must be >= 0", who, s->max_gap);
  NHIP_REQUIRE(s->min_length >= 1, "%s: min_length %d must be >= 1", who, s->min_length);
  NHIP_REQUIRE(s->max_segments >= 0, "%s: max_segments %d must be >= 0", who, s->max_segments);
  return NHIP_OK;
}

void tables_of(const nhip_vectorize_spec_t &s, int32_t *C, int32_t *S) {
  for (int32_t t = 0; t < s.n_theta; t++) {
    const double a = M_PI * (double)t / (double)s.n_theta;
    C[t] = (int32_t)lrint(16384.0 * cos(a));
    S[t] = (int32_t)lrint(16384.0 * sin(a));
  }
}

int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

// the steps nhip_vectorize_dev and the handle form share; the arguments have been checked
int vectorize_run(const float *d_xy, const int32_t *d_offsets, const float *d_affines, int32_t n_scans,
                  const nhip_vectorize_spec_t &spec, int32_t max_cells, int32_t max_rounds, int32_t check_every,
                  int64_t *d_records, int32_t *d_stats, void *d_ws, hipStream_t s) {
  VecLayout L;
  vec_layout(spec, max_cells, &L);
  uint8_t *base = static_cast<uint8_t *>(d_ws);
  VecParams P;
  P.width = spec.width, P.height = spec.height, P.cell_x0 = spec.cell_x0, P.cell_y0 = spec.cell_y0;
  P.n_theta = spec.n_theta, P.n_rho = L.n_rho, P.n_along = L.n_along, P.min_hits = spec.min_hits, P.min_votes = spec.min_votes;
  P.band_q = (int32_t)lrint(spec.band * 16384.0);
  P.gap1 = (spec.max_gap < (1 << 20) ? spec.max_gap : (1 << 20)) + 1;  // (no two bins lie further apart than n_along < 2^16)
  P.min_length = spec.min_length, P.max_segments = spec.max_segments, P.max_cells = max_cells, P.max_rounds = max_rounds;
  P.n_scans = n_scans;
  P.res = spec.res, P.inv_res = 1.0 / spec.res;
  P.st = reinterpret_cast<VecState *>(base + L.state);
  auto i32 = [&](int64_t off) { return reinterpret_cast<int32_t *>(base + off); };
  P.counts = i32(L.counts), P.cells = i32(L.cells), P.votes = i32(L.votes), P.row_off = i32(L.row_off);
  P.run_of_bin = i32(L.run_of_bin), P.run_lo = i32(L.run_lo), P.run_hi = i32(L.run_hi), P.run_slot = i32(L.run_slot);
  P.band_list = i32(L.band_list);
  P.C = i32(L.tables), P.S = i32(L.tables) + spec.n_theta;
  P.live = base + L.live;
  P.partial = reinterpret_cast<unsigned long long *>(base + L.partial);
  P.bits = reinterpret_cast<uint32_t *>(base + L.bits);
  P.records = reinterpret_cast<long long *>(d_records);
  P.status = dev_status();
  std::vector<int32_t> tab(2 * (size_t)spec.n_theta);  // (lives until the stream has drained below)
  tables_of(spec, tab.data(), tab.data() + spec.n_theta);
  NHIP_TRY_HIP(hipMemcpyAsync(base + L.tables, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, s));
  int rc = launch_vec_front(P, d_xy, d_offsets, d_affines, s);
  if (rc) return rc;
  // Round max_rounds + 1 can only end the call (flag 0 or 1 at its peak), so the loop below always finds the end word set.
  // Kernels enqueued behind the end return at once: nothing depends on check_every.
  int32_t end = 0;
  for (int64_t done = 0, all = (int64_t)max_rounds + 1; done < all && !end;) {
    const int32_t n = (int32_t)(all - done < check_every ? all - done : check_every);
    if ((rc = launch_vec_rounds(P, n, s))) return rc;
    done += n;
    NHIP_TRY_HIP(hipMemcpyAsync(&end, &P.st->end, sizeof(end), hipMemcpyDeviceToHost, s));
    NHIP_TRY_HIP(hipStreamSynchronize(s));
  }
  NHIP_TRY_HIP(hipMemcpyAsync(d_stats, P.st->stats, STATS_WORDS * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  NHIP_TRY_HIP(hipStreamSynchronize(s));
  return NHIP_OK;
}

int vectorize_call_check(const char *who, int32_t n_scans, int32_t max_cells, int32_t max_rounds, int32_t check_every) {
  NHIP_REQUIRE(n_scans >= 0 && max_cells >= 0 && max_rounds >= 0 && check_every >= 1,
               "%s: n_scans %d, max_cells %d and max_rounds %d must be >= 0, check_every %d >= 1", who, n_scans, max_cells,
               max_rounds, check_every);
  return NHIP_OK;
}

}  // namespace

namespace nhip {

void vec_layout(const nhip_vectorize_spec_t &s, int32_t max_cells, VecLayout *L) {
  L->n_rho = 2 * s.width + s.height + 1;
  L->n_along = s.width + 2 * s.height + 1;
  L->bit_words = (L->n_along + 31) / 32;
  L->max_runs = L->n_along / 2 + 1;
  const int64_t cells = max_cells > 0 ? max_cells : 1;
  int64_t at = 0;
  auto take = [&](int64_t bytes) {
    const int64_t here = at;
    at = up256(at + bytes);
    return here;
  };
  L->state = take(sizeof(VecState));
  L->counts = take(4 * (int64_t)s.width * s.height);
  L->cells = take(8 * cells);
  L->votes = take(4 * (int64_t)s.n_theta * L->n_rho);
  L->live = take(cells);
  L->row_off = take(4 * ((int64_t)s.height + 1));
  L->tables = take(8 * (int64_t)s.n_theta);
  L->partial = take(8 * 256);
  L->bits = take(4 * (int64_t)L->bit_words);
  L->run_of_bin = take(4 * (int64_t)L->n_along);
  L->run_lo = take(4 * (int64_t)L->max_runs);
  L->run_hi = take(4 * (int64_t)L->max_runs);
  L->run_slot = take(4 * (int64_t)L->max_runs);
  L->band_list = take(4 * cells);
  L->bytes = at;
}

}  // namespace nhip

extern "C" {

int nhip_vectorize_spec_default(nhip_vectorize_spec_t *out) {
  NHIP_REQUIRE(out, "vectorize_spec_default: null pointer");
  *out = nhip_vectorize_spec_t{};
  out->res = 0.05;
  out->band = 1.5;
  out->min_hits = 2;
  out->n_theta = 360;
  out->min_votes = 20;
  out->max_gap = 4;
  out->min_length = 10;
  out->max_segments = 4096;
  return NHIP_OK;
}

int nhip_vectorize_tables(const nhip_vectorize_spec_t *spec, int32_t *c_table, int32_t *s_table) {
  int rc = vectorize_spec_check(spec, "vectorize_tables");
  if (rc) return rc;
  NHIP_REQUIRE(c_table && s_table, "vectorize_tables: null pointer");
  tables_of(*spec, c_table, s_table);
  return NHIP_OK;
}

int nhip_map_pose_affines(const double *poses, int32_t n_poses, float *out) {
  NHIP_REQUIRE(n_poses >= 0 && (n_poses == 0 || (poses && out)), "map_pose_affines: bad arguments");
  for (int32_t i = 0; i < n_poses; i++) {
    // the cast of TransformPointcloud (slam_util.h:55-63)
    out[4 * (size_t)i + 0] = (float)cos(poses[3 * (size_t)i + 2]);
    out[4 * (size_t)i + 1] = (float)sin(poses[3 * (size_t)i + 2]);
    out[4 * (size_t)i + 2] = (float)poses[3 * (size_t)i + 0];
    out[4 * (size_t)i + 3] = (float)poses[3 * (size_t)i + 1];
  }
  return NHIP_OK;
}

int nhip_vectorize_workspace_layout(const nhip_vectorize_spec_t *spec, int32_t max_cells, nhip_vectorize_layout_t *out) {
  int rc = vectorize_spec_check(spec, "vectorize_workspace_layout");
  if (rc) return rc;
  NHIP_REQUIRE(out && max_cells >= 0, "vectorize_workspace_layout: null pointer or max_cells %d < 0", max_cells);
  VecLayout L;
  vec_layout(*spec, max_cells, &L);
  *out = nhip_vectorize_layout_t{L.counts, L.cells, L.votes, L.live, L.bytes, L.n_rho, L.n_along};
  return NHIP_OK;
}

int64_t nhip_vectorize_workspace_bytes(const nhip_vectorize_spec_t *spec, int32_t max_cells) {
  nhip_vectorize_layout_t L;
  return nhip_vectorize_workspace_layout(spec, max_cells, &L) == NHIP_OK ? L.bytes : -1;
}

int nhip_vectorize_dev(const float *d_xy, const int32_t *d_offsets, const float *d_affines, int32_t n_scans,
                       const nhip_vectorize_spec_t *spec, int32_t max_cells, int32_t max_rounds, int32_t check_every,
                       int64_t *d_records, int32_t *d_stats, void *d_workspace, int64_t workspace_bytes, void *stream) {
  int rc = vectorize_spec_check(spec, "vectorize_dev");  // (a bad spec is an argument error with or without a device)
  if (rc || (rc = vectorize_call_check("vectorize_dev", n_scans, max_cells, max_rounds, check_every))) return rc;
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_stats && d_workspace && (spec->max_segments == 0 || d_records) && (n_scans == 0 || (d_xy && d_offsets && d_affines)),
               "vectorize_dev: null pointer");
  VecLayout L;
  vec_layout(*spec, max_cells, &L);
  NHIP_REQUIRE(workspace_bytes >= L.bytes, "vectorize_dev: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)L.bytes);
  NHIP_REQUIRE(aligned(d_workspace, 256), "vectorize_dev: d_workspace must be 256-byte aligned");
  return vectorize_run(d_xy, d_offsets, d_affines, n_scans, *spec, max_cells, max_rounds, check_every, d_records, d_stats,
                       d_workspace, static_cast<hipStream_t>(stream));
}

int nhip_vectorize(const nhip_scans_t *scans, const double *poses, const nhip_vectorize_spec_t *spec, int32_t max_cells,
                   int32_t max_rounds, int32_t check_every, int64_t *records, int32_t *stats) {
  int rc = vectorize_spec_check(spec, "vectorize");
  if (rc || (rc = vectorize_call_check("vectorize", 0, max_cells, max_rounds, check_every))) return rc;
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(scans && stats && (spec->max_segments == 0 || records) && (scans->n_scans == 0 || poses), "vectorize: bad arguments");
  const int32_t n = scans->n_scans;
  std::vector<float> aff(4 * (size_t)n);
  if ((rc = nhip_map_pose_affines(poses, n, aff.data()))) return rc;
  VecLayout L;
  vec_layout(*spec, max_cells, &L);
  Staged st;
  const float *da = st.in(aff.data(), aff.size());
  int64_t *dr = st.out<int64_t>(REC_WORDS * (size_t)spec->max_segments);
  int32_t *ds = st.out<int32_t>(STATS_WORDS);
  uint8_t *dw = st.out<uint8_t>((size_t)L.bytes);
  if (st.ok())
    st.launched(vectorize_run(scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), da, n, *spec, max_cells, max_rounds,
                              check_every, dr, ds, dw, nullptr));
  st.fetch(stats, ds, STATS_WORDS);
  st.fetch(records, dr, st.ok() && stats[1] > 0 ? REC_WORDS * (size_t)stats[1] : 0);
  return st.finish();
}

int nhip_vectorize_endpoints(const nhip_vectorize_spec_t *spec, const int64_t *records, int32_t n, float *lines) {
  int rc = vectorize_spec_check(spec, "vectorize_endpoints");
  if (rc) return rc;
  NHIP_REQUIRE(n >= 0 && (n == 0 || (records && lines)), "vectorize_endpoints: bad arguments");
  for (int32_t i = 0; i < n; i++)
    NHIP_REQUIRE(records[10 * (size_t)i] >= 0 && records[10 * (size_t)i] < spec->n_theta, "vectorize_endpoints: record %d: row %lld outside the %d rows",
                 i, (long long)records[10 * (size_t)i], spec->n_theta);
  std::vector<int32_t> tab(2 * (size_t)spec->n_theta);
  tables_of(*spec, tab.data(), tab.data() + spec->n_theta);
  const int64_t w_q = (int64_t)spec->width << VQ;
  for (int32_t i = 0; i < n; i++) {
    // compiled without contraction: every product, sum and quotient rounds on its own (the spec's order)
    const int64_t *r = records + 10 * (size_t)i;
    const double cnt = (double)r[4], sx = (double)r[5], sy = (double)r[6];
    const double mx = sx / cnt, my = sy / cnt;
    const double cxx = (double)r[7] - sx * mx, cxy = (double)r[8] - sx * my, cyy = (double)r[9] - sy * my;
    const double phi = 0.5 * atan2(2.0 * cxy, cxx - cyy);
    const double dx = cos(phi), dy = sin(phi);
    const double c = (double)tab[(size_t)r[0]] / 16384.0, s = (double)tab[(size_t)spec->n_theta + (size_t)r[0]] / 16384.0;
    const double rho = (double)((r[1] << VQ) + (1 << (VQ - 1)) - w_q) / 16384.0;
    for (int e = 0; e < 2; e++) {
      const double alpha = (double)(r[2 + e] + e - spec->width);  // a_lo, then a_hi + 1
      const double px = rho * c - alpha * s, py = rho * s + alpha * c;
      const double u = (px - mx) * dx + (py - my) * dy;
      const double qx = mx + u * dx, qy = my + u * dy;
      lines[4 * (size_t)i + 2 * e] = (float)((((double)spec->cell_x0 + qx) + 0.5) * spec->res);
      lines[4 * (size_t)i + 2 * e + 1] = (float)((((double)spec->cell_y0 + qy) + 0.5) * spec->res);
    }
  }
  return NHIP_OK;
}

}  // extern "C"
