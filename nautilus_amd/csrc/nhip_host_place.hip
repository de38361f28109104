// nhip_host_place.hip -- the place-descriptor entry points of the C ABI (kernels: nhip_place.hip, K16, and nhip_place_seq.hip,
// K16b): the specs' defaults and their checks, the tables, the workspace rules, the forms on the caller's buffers and stream,
// and the handle forms with a host list and host outputs.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

constexpr int32_t PLACE_MAX_IDS = 1 << 20;
constexpr int32_t PLACE_MAX_CHUNK_ROWS = 1 << 19;  // (a launch's grid: chunk rows / PLACE_QT workgroups along y)

// the accepted ranges of include/nautilus_hip.h; `match`: the call compares descriptors
int place_spec_check(const nhip_place_spec_t *s, bool match, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  const int max_rings = match ? PLACE_MATCH_MAX_RINGS : PLACE_MAX_RINGS;
  NHIP_REQUIRE(s->n_rings >= 1 && s->n_rings <= max_rings, "%s: n_rings %d outside 1..%d%s", who, s->n_rings, max_rings,
               match ? " (the 16-bit key of a pair holds dist <= 1022)" : "");
  NHIP_REQUIRE(std::isfinite(s->range_max) && s->range_max > 0, "%s: range_max must be finite and > 0", who);
  NHIP_REQUIRE(s->top_k >= 1 && s->top_k <= 32, "%s: top_k %d outside 1..32", who, s->top_k);
  NHIP_REQUIRE(s->min_separation >= 0, "%s: min_separation %d must be >= 0", who, s->min_separation);
  NHIP_REQUIRE(s->max_permille >= 0 && s->max_permille <= 1000, "%s: max_permille %d outside 0..1000", who, s->max_permille);
  NHIP_REQUIRE(s->flags == 0 || s->flags == NHIP_PLACE_PAST_ONLY, "%s: flags %d: 0 or NHIP_PLACE_PAST_ONLY", who, s->flags);
  return NHIP_OK;
}

void place_tables(const nhip_place_spec_t &s, float *edge2, float *dir) {
  for (int k = 0; k <= s.n_rings; k++) {
    const float e = (float)((double)s.range_max * k / s.n_rings);
    edge2[k] = e * e;
  }
  const double two_pi = 6.283185307179586476925286766559;
  for (int j = 0; j < 32; j++) dir[2 * j] = (float)std::cos(two_pi * j / 64), dir[2 * j + 1] = (float)std::sin(two_pi * j / 64);
}

PlaceTables place_tables_of(const nhip_place_spec_t &s) {
  PlaceTables T;
  T.n_rings = s.n_rings;
  place_tables(s, T.edge2, T.dir);
  return T;
}

int64_t place_row_bytes(int32_t n_ids) { return 2 * (((int64_t)n_ids + 63) & ~63ll); }

// the arguments have been checked
int place_match_run(const uint64_t *d_desc, const int32_t *d_bits, int32_t n_scans, const int32_t *d_ids, int32_t n_ids,
                    const nhip_place_spec_t &spec, int32_t *d_records, int64_t *d_stats, void *d_ws, int64_t ws_bytes, hipStream_t s) {
  PlaceMatch P;
  P.desc = reinterpret_cast<const unsigned long long *>(d_desc), P.bits = d_bits, P.ids = d_ids;
  P.keys = static_cast<uint16_t *>(d_ws), P.records = d_records, P.stats = reinterpret_cast<long long *>(d_stats);
  P.status = dev_status();
  P.n_scans = n_scans, P.n_ids = n_ids, P.pitch = (int32_t)(place_row_bytes(n_ids) / 2);
  P.n_rings = spec.n_rings, P.top_k = spec.top_k, P.min_separation = spec.min_separation, P.max_permille = spec.max_permille;
  P.flags = spec.flags;
  int64_t rows = n_ids > 0 ? ws_bytes / place_row_bytes(n_ids) / PLACE_QT * PLACE_QT : PLACE_QT;
  NHIP_REQUIRE(rows >= PLACE_QT, "place_match: a workspace of %lld bytes holds fewer than %d rows of %lld bytes", (long long)ws_bytes,
               PLACE_QT, (long long)place_row_bytes(n_ids));
  if (rows > PLACE_MAX_CHUNK_ROWS) rows = PLACE_MAX_CHUNK_ROWS;
  return launch_place_match(P, (int32_t)rows, s);
}

// ---- place sequences (K16b) ----
constexpr int32_t SEQ_MIN_CHUNK = 16;  // query scans a chunk holds at least (beside its halo)

int place_seq_spec_check(const nhip_place_spec_t *s, const nhip_place_seq_spec_t *q, const char *who) {
  int rc = place_spec_check(s, true, who);
  if (rc) return rc;
  NHIP_REQUIRE(q, "%s: null sequence spec", who);
  NHIP_REQUIRE(q->half_window >= 0 && q->half_window <= 8, "%s: half_window %d outside 0..8", who, q->half_window);
  NHIP_REQUIRE(q->step >= 1 && q->step <= 16, "%s: step %d outside 1..16", who, q->step);
  NHIP_REQUIRE(s->min_separation >= 2 * q->half_window * q->step,
               "%s: min_separation %d below 2 half_window step = %d: the two windows of a pair would touch", who, s->min_separation,
               2 * q->half_window * q->step);
  return NHIP_OK;
}

// the workspace of a chunk of S query scans: S + halo rows of the plane (all scans' rows without a halo when S covers them),
// then S rows of keys
struct SeqLayout {
  int64_t row_s, row_i, halo_bytes, per_scan, full;
  int32_t all;  // query scans when nothing is chunked: n_scans, at least 1
};
SeqLayout seq_layout(const nhip_place_seq_spec_t &q, int32_t n_scans, int32_t n_ids) {
  SeqLayout L;
  L.row_s = place_row_bytes(n_scans > 0 ? n_scans : 1), L.row_i = place_row_bytes(n_ids > 0 ? n_ids : 1);
  L.halo_bytes = 2ll * q.half_window * q.step * L.row_s, L.per_scan = L.row_s + L.row_i;
  L.all = n_scans > 0 ? n_scans : 1;
  L.full = L.all * L.per_scan;
  return L;
}

// the arguments have been checked
int place_seq_run(const uint64_t *d_desc, const int32_t *d_bits, int32_t n_scans, const int32_t *d_ids, int32_t n_ids,
                  const nhip_place_spec_t &spec, const nhip_place_seq_spec_t &seq, int32_t *d_records, int64_t *d_stats, void *d_ws,
                  int64_t ws_bytes, hipStream_t s) {
  const SeqLayout L = seq_layout(seq, n_scans, n_ids);
  int64_t S = L.all, plane_rows = L.all;
  if (ws_bytes < L.full) {
    S = ws_bytes >= L.halo_bytes ? (ws_bytes - L.halo_bytes) / L.per_scan : 0;
    NHIP_REQUIRE(S >= SEQ_MIN_CHUNK, "place_seq_match: a workspace of %lld bytes holds fewer than %d query scans (%lld bytes each) beside a halo of %lld bytes",
                 (long long)ws_bytes, SEQ_MIN_CHUNK, (long long)L.per_scan, (long long)L.halo_bytes);
    if (S > PLACE_MAX_CHUNK_ROWS / 2) S = PLACE_MAX_CHUNK_ROWS / 2;  // (a launch's grid: plane rows / PLACE_QT workgroups along y)
    plane_rows = S + 2ll * seq.half_window * seq.step;
  }
  PlaceSeq P;
  P.desc = reinterpret_cast<const unsigned long long *>(d_desc), P.bits = d_bits, P.ids = d_ids;
  P.plane = static_cast<uint16_t *>(d_ws), P.keys = P.plane + plane_rows * (L.row_s / 2);
  P.records = d_records, P.stats = reinterpret_cast<long long *>(d_stats), P.status = dev_status();
  P.n_scans = n_scans, P.n_ids = n_ids, P.pitch_s = (int32_t)(L.row_s / 2), P.pitch = (int32_t)(L.row_i / 2);
  P.n_rings = spec.n_rings, P.top_k = spec.top_k, P.min_separation = spec.min_separation, P.max_permille = spec.max_permille;
  P.flags = spec.flags, P.half_window = seq.half_window, P.step = seq.step;
  return launch_place_seq_match(P, (int32_t)S, s);
}

// ---- the handle forms ----
// what they ask of their list: ids of the handle's scans, strictly ascending
int place_ids_check(const int32_t *ids, int32_t n_ids, int32_t n_scans, const char *who) {
  for (int32_t b = 0; b < n_ids; b++) {
    NHIP_REQUIRE(ids[b] >= 0 && ids[b] < n_scans, "%s: ids[%d] = %d outside the %d scans", who, b, ids[b], n_scans);
    NHIP_REQUIRE(b == 0 || ids[b] > ids[b - 1], "%s: ids[%d] = %d after %d: the list must ascend strictly", who, b, ids[b], ids[b - 1]);
  }
  return NHIP_OK;
}

// on checked arguments: describe every scan, then match the list -- window sums where `seq` is given, single scans otherwise
int place_candidates_run(const nhip_scans_t *scans, const int32_t *ids, int32_t n_ids, const nhip_place_spec_t &spec,
                         const nhip_place_seq_spec_t *seq, int32_t *records, int64_t *stats, uint64_t *desc, int32_t *bits) {
  const int32_t n = scans->n_scans;
  const size_t n_desc = (size_t)spec.n_rings * (size_t)n;
  const size_t n_rec = (seq ? 8 : 4) * (size_t)spec.top_k * (size_t)n_ids;  // (int32 words: a sequence record is twice a single one)
  const int64_t ws_bytes = seq ? nhip_place_seq_workspace_bytes(&spec, seq, n, n_ids) : nhip_place_workspace_bytes(&spec, n_ids);
  Staged st;
  uint64_t *dd = st.out<uint64_t>(n_desc);
  int32_t *db = st.out<int32_t>((size_t)n);
  const int32_t *di = st.in(ids, (size_t)n_ids);
  int32_t *dr = st.out<int32_t>(n_rec);
  int64_t *ds = st.out<int64_t>(STATS_WORDS);
  uint8_t *dw = st.out<uint8_t>((size_t)ws_bytes);
  if (st.ok())
    st.launched(launch_place_describe(place_tables_of(spec), scans->xy.as<const float>(), scans->offsets.as<const int32_t>(), n, dd, db, nullptr));
  if (st.ok())
    st.launched(seq ? place_seq_run(dd, db, n, di, n_ids, spec, *seq, dr, ds, dw, ws_bytes, nullptr)
                    : place_match_run(dd, db, n, di, n_ids, spec, dr, ds, dw, ws_bytes, nullptr));
  st.fetch(records, dr, n_rec);
  st.fetch(stats, ds, STATS_WORDS);
  st.fetch(desc, dd, n_desc);
  st.fetch(bits, db, (size_t)n);
  return st.finish();
}

}  // namespace

extern "C" {

int nhip_place_spec_default(nhip_place_spec_t *out) {
  NHIP_REQUIRE(out, "place_spec_default: null pointer");
  *out = nhip_place_spec_t{};
  out->n_rings = 10;
  out->range_max = 30.0f;
  out->top_k = 5;
  out->min_separation = 20;
  out->max_permille = 1000;
  return NHIP_OK;
}

int nhip_place_tables(const nhip_place_spec_t *spec, float *edge2, float *dir) {
  int rc = place_spec_check(spec, false, "place_tables");
  if (rc) return rc;
  NHIP_REQUIRE(edge2 && dir, "place_tables: null pointer");
  place_tables(*spec, edge2, dir);
  return NHIP_OK;
}

int64_t nhip_place_workspace_bytes(const nhip_place_spec_t *spec, int32_t n_ids) {
  if (place_spec_check(spec, true, "place_workspace_bytes")) return -1;
  if (n_ids < 0 || n_ids > PLACE_MAX_IDS) {
    set_error("place_workspace_bytes: n_ids %d outside 0..%d", n_ids, PLACE_MAX_IDS);
    return -1;
  }
  const int64_t tile = PLACE_QT * place_row_bytes(n_ids > 0 ? n_ids : 1), tiles = ((int64_t)n_ids + PLACE_QT - 1) / PLACE_QT;
  const int64_t fit = NHIP_PLACE_WORKSPACE_MAX / tile;
  return tile * (tiles < 1 ? 1 : tiles <= fit ? tiles : fit < 1 ? 1 : fit);
}

int nhip_place_describe_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_place_spec_t *spec,
                            uint64_t *d_desc, int32_t *d_bits, void *stream) {
  int rc = place_spec_check(spec, false, "place_describe_dev");  // (a bad spec is an argument error with or without a device)
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0, "place_describe_dev: n_scans %d must be >= 0", n_scans);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(n_scans == 0 || (d_xy && d_offsets && d_desc && d_bits), "place_describe_dev: null pointer");
  NHIP_REQUIRE(aligned(d_desc, 8), "place_describe_dev: d_desc must be 8-byte aligned");
  return launch_place_describe(place_tables_of(*spec), d_xy, d_offsets, n_scans, d_desc, d_bits, static_cast<hipStream_t>(stream));
}

int nhip_place_match_dev(const uint64_t *d_desc, const int32_t *d_bits, int32_t n_scans, const int32_t *d_ids, int32_t n_ids,
                         const nhip_place_spec_t *spec, int32_t *d_records, int64_t *d_stats, void *d_workspace,
                         int64_t workspace_bytes, void *stream) {
  int rc = place_spec_check(spec, true, "place_match_dev");
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0 && n_ids >= 0 && n_ids <= PLACE_MAX_IDS, "place_match_dev: n_scans %d must be >= 0, n_ids %d in 0..%d", n_scans,
               n_ids, PLACE_MAX_IDS);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_stats && (n_ids == 0 || (d_desc && d_bits && d_ids && d_records && d_workspace)), "place_match_dev: null pointer");
  NHIP_REQUIRE(aligned(d_desc, 8) && aligned(d_stats, 8) && aligned(d_workspace, 2),
               "place_match_dev: d_desc and d_stats must be 8-byte aligned, d_workspace 2-byte");
  return place_match_run(d_desc, d_bits, n_scans, d_ids, n_ids, *spec, d_records, d_stats, d_workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream));
}

int nhip_place_candidates(const nhip_scans_t *scans, const int32_t *ids, int32_t n_ids, const nhip_place_spec_t *spec,
                          int32_t *records, int64_t *stats, uint64_t *desc, int32_t *bits) {
  int rc = place_spec_check(spec, true, "place_candidates");
  if (rc || (rc = require_device())) return rc;
  NHIP_REQUIRE(scans && stats && n_ids >= 0 && n_ids <= PLACE_MAX_IDS && (n_ids == 0 || (ids && records)), "place_candidates: bad arguments");
  if ((rc = place_ids_check(ids, n_ids, scans->n_scans, "place_candidates"))) return rc;
  return place_candidates_run(scans, ids, n_ids, *spec, nullptr, records, stats, desc, bits);
}

int nhip_place_seq_spec_default(nhip_place_seq_spec_t *out) {
  NHIP_REQUIRE(out, "place_seq_spec_default: null pointer");
  *out = nhip_place_seq_spec_t{};
  out->half_window = 2;
  out->step = 1;
  return NHIP_OK;
}

int64_t nhip_place_seq_workspace_bytes(const nhip_place_spec_t *spec, const nhip_place_seq_spec_t *seq, int32_t n_scans, int32_t n_ids) {
  if (place_seq_spec_check(spec, seq, "place_seq_workspace_bytes")) return -1;
  if (n_scans < 0 || n_ids < 0 || n_ids > PLACE_MAX_IDS) {
    set_error("place_seq_workspace_bytes: n_scans %d must be >= 0, n_ids %d in 0..%d", n_scans, n_ids, PLACE_MAX_IDS);
    return -1;
  }
  const SeqLayout L = seq_layout(*seq, n_scans, n_ids);
  if (L.full <= NHIP_PLACE_WORKSPACE_MAX) return L.full;
  int64_t S = NHIP_PLACE_WORKSPACE_MAX >= L.halo_bytes ? (NHIP_PLACE_WORKSPACE_MAX - L.halo_bytes) / L.per_scan : 0;
  if (S < SEQ_MIN_CHUNK) S = SEQ_MIN_CHUNK;
  const int64_t bytes = S * L.per_scan + L.halo_bytes;
  return bytes < L.full ? bytes : L.full;
}

int nhip_place_seq_match_dev(const uint64_t *d_desc, const int32_t *d_bits, int32_t n_scans, const int32_t *d_ids, int32_t n_ids,
                             const nhip_place_spec_t *spec, const nhip_place_seq_spec_t *seq, int32_t *d_records, int64_t *d_stats,
                             void *d_workspace, int64_t workspace_bytes, void *stream) {
  int rc = place_seq_spec_check(spec, seq, "place_seq_match_dev");
  if (rc) return rc;
  NHIP_REQUIRE(n_scans >= 0 && n_ids >= 0 && n_ids <= PLACE_MAX_IDS, "place_seq_match_dev: n_scans %d must be >= 0, n_ids %d in 0..%d",
               n_scans, n_ids, PLACE_MAX_IDS);
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_stats && (n_ids == 0 || (d_ids && d_records && d_workspace && (n_scans == 0 || (d_desc && d_bits)))),
               "place_seq_match_dev: null pointer");
  NHIP_REQUIRE(aligned(d_desc, 8) && aligned(d_stats, 8) && aligned(d_workspace, 2),
               "place_seq_match_dev: d_desc and d_stats must be 8-byte aligned, d_workspace 2-byte");
  return place_seq_run(d_desc, d_bits, n_scans, d_ids, n_ids, *spec, *seq, d_records, d_stats, d_workspace, workspace_bytes,
                       static_cast<hipStream_t>(stream));
}

int nhip_place_seq_candidates(const nhip_scans_t *scans, const int32_t *ids, int32_t n_ids, const nhip_place_spec_t *spec,
                              const nhip_place_seq_spec_t *seq, int32_t *records, int64_t *stats) {
  int rc = place_seq_spec_check(spec, seq, "place_seq_candidates");
  if (rc || (rc = require_device())) return rc;
  NHIP_REQUIRE(scans && stats && n_ids >= 0 && n_ids <= PLACE_MAX_IDS && (n_ids == 0 || (ids && records)), "place_seq_candidates: bad arguments");
  if ((rc = place_ids_check(ids, n_ids, scans->n_scans, "place_seq_candidates"))) return rc;
  return place_candidates_run(scans, ids, n_ids, *spec, seq, records, stats, nullptr, nullptr);
}

}  // extern "C"
