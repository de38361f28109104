// nhip_host_consistency.hip -- the loop-closure consistency entry points of the C ABI (kernels: nhip_consistency.hip, K17): the
// spec's defaults and its check, the one-buffer workspace rule, the forms on the caller's buffers and stream -- the set with the
// host loop over the steps (vectorize_run's pattern, nhip_host_vectorize.hip: steps are enqueued check_every at a time, one look
// at the done word between two batches) -- and the host-memory form.
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

constexpr int32_t CHECK_EVERY_DEFAULT = 8;  // (nhip_vectorize's default)
constexpr size_t RECORD_DOUBLES = 8;        // a match record as the adjacency kernel reads it (include/nautilus_hip.h)

int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
int64_t words_of(int32_t M) { return ((int64_t)M + 63) / 64; }
int64_t adj_offset() { return NHIP_CONSISTENCY_STATE_BYTES; }
int64_t deg_offset(int32_t M) { return adj_offset() + 8 * (int64_t)M * words_of(M); }
int64_t workspace_bytes(int32_t M) { return up256(deg_offset(M) + 4 * (int64_t)M); }

// the accepted ranges of include/nautilus_hip.h
int consistency_spec_check(const nhip_consistency_spec_t *s, const char *who) {
  NHIP_REQUIRE(s, "%s: null spec", who);
  const double tol[6] = {s->t0, s->t_rate, s->t_max, s->r0, s->r_rate, s->r_max};
  static const char *const name[6] = {"t0", "t_rate", "t_max", "r0", "r_rate", "r_max"};
  for (int k = 0; k < 6; k++)
    NHIP_REQUIRE(std::isfinite(tol[k]) && tol[k] >= 0.0, "%s: %s must be finite and >= 0", who, name[k]);
  NHIP_REQUIRE(s->t_max >= s->t0, "%s: t_max %g below t0 %g", who, s->t_max, s->t0);
  NHIP_REQUIRE(s->r_max >= s->r0, "%s: r_max %g below r0 %g", who, s->r_max, s->r0);
  NHIP_REQUIRE(s->max_steps >= 1, "%s: max_steps %d must be >= 1", who, s->max_steps);
  NHIP_REQUIRE(s->flags == 0, "%s: flags %d: none is defined", who, s->flags);
  return NHIP_OK;
}

int count_check(int32_t M, const char *who) {
  NHIP_REQUIRE(M >= 0 && M <= CONSISTENCY_MAX_RECORDS, "%s: M %d outside 0..%d", who, M, CONSISTENCY_MAX_RECORDS);
  return NHIP_OK;
}

ConsistencyTol tol_of(const nhip_consistency_spec_t &s) { return ConsistencyTol{s.t0, s.t_rate, s.t_max, s.r0, s.r_rate, s.r_max}; }

// the set on checked arguments: begin, then the steps in batches; waits for the stream
int consistency_set_run(const uint64_t *d_adj, const int32_t *d_deg, int32_t M, const nhip_consistency_spec_t &spec, int32_t check_every,
                        int32_t *d_members, int32_t *d_n_members, int64_t *d_stats, void *d_ws, hipStream_t s) {
  uint8_t *base = static_cast<uint8_t *>(d_ws);
  ConsistencySet P;
  P.adj = reinterpret_cast<const unsigned long long *>(d_adj), P.deg = d_deg;
  P.st = reinterpret_cast<ConsistencyState *>(base);
  P.C = reinterpret_cast<unsigned long long *>(base + 256);
  P.members = d_members, P.n_members = d_n_members, P.stats = reinterpret_cast<long long *>(d_stats);
  P.status = dev_status();
  P.M = M, P.W = (int32_t)words_of(M), P.max_steps = spec.max_steps < M ? spec.max_steps : M;
  int rc = launch_consistency_begin(P, s);
  if (rc) return rc;
  // Every step appends one member, and step max_steps sets the done word if none before it did: the loop below always finds
  // it set.  Kernels enqueued behind the end return at once: nothing depends on check_every.
  int32_t done = 0;
  for (int32_t at = 0; at < P.max_steps && !done;) {
    const int32_t n = P.max_steps - at < check_every ? P.max_steps - at : check_every;
    if ((rc = launch_consistency_steps(P, n, s))) return rc;
    at += n;
    NHIP_TRY_HIP(hipMemcpyAsync(&done, &P.st->done, sizeof(done), hipMemcpyDeviceToHost, s));
    NHIP_TRY_HIP(hipStreamSynchronize(s));
  }
  NHIP_TRY_HIP(hipStreamSynchronize(s));
  return NHIP_OK;
}

}  // namespace

extern "C" {

int nhip_consistency_spec_default(nhip_consistency_spec_t *out) {
  NHIP_REQUIRE(out, "consistency_spec_default: null pointer");
  *out = nhip_consistency_spec_t{};
  // chosen by the study of DESIGN.md section 3, "Loop-closure consistency"
  out->t0 = 0.8, out->t_rate = 0.1, out->t_max = 16.0;
  out->r0 = 0.1, out->r_rate = 0.005, out->r_max = 0.5;
  out->max_steps = CONSISTENCY_MAX_RECORDS;
  return NHIP_OK;
}

int64_t nhip_consistency_workspace_bytes(int32_t M) {
  if (count_check(M, "consistency_workspace_bytes")) return -1;
  return workspace_bytes(M);
}

int nhip_consistency_adjacency_dev(const double *d_records, int32_t M, const nhip_consistency_spec_t *spec, uint64_t *d_adj,
                                   int32_t *d_deg, int64_t *d_stats, void *stream) {
  int rc = consistency_spec_check(spec, "consistency_adjacency_dev");  // (a bad spec is an argument error with or without a device)
  if (rc || (rc = count_check(M, "consistency_adjacency_dev"))) return rc;
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_stats && (M == 0 || (d_records && d_adj && d_deg)), "consistency_adjacency_dev: null pointer");
  NHIP_REQUIRE(aligned(d_records, 8) && aligned(d_adj, 8) && aligned(d_stats, 8) && aligned(d_deg, 4),
               "consistency_adjacency_dev: d_records, d_adj and d_stats must be 8-byte aligned, d_deg 4-byte");
  return launch_consistency_adjacency(d_records, M, tol_of(*spec), reinterpret_cast<unsigned long long *>(d_adj), d_deg,
                                      reinterpret_cast<long long *>(d_stats), static_cast<hipStream_t>(stream));
}

int nhip_consistency_set_dev(const uint64_t *d_adj, const int32_t *d_deg, int32_t M, const nhip_consistency_spec_t *spec,
                             int32_t check_every, int32_t *d_members, int32_t *d_n_members, int64_t *d_stats, void *d_workspace,
                             int64_t workspace_bytes_given, void *stream) {
  int rc = consistency_spec_check(spec, "consistency_set_dev");
  if (rc || (rc = count_check(M, "consistency_set_dev"))) return rc;
  NHIP_REQUIRE(check_every >= 0, "consistency_set_dev: check_every %d must be >= 0 (0: the default, %d)", check_every, CHECK_EVERY_DEFAULT);
  NHIP_REQUIRE(workspace_bytes_given >= workspace_bytes(M), "consistency_set_dev: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes_given, (long long)workspace_bytes(M));
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(d_n_members && d_stats && d_workspace && (M == 0 || (d_adj && d_deg && d_members)), "consistency_set_dev: null pointer");
  NHIP_REQUIRE(aligned(d_adj, 8) && aligned(d_stats, 8) && aligned(d_workspace, 256),
               "consistency_set_dev: d_adj and d_stats must be 8-byte aligned, d_workspace 256-byte");
  return consistency_set_run(d_adj, d_deg, M, *spec, check_every ? check_every : CHECK_EVERY_DEFAULT, d_members, d_n_members, d_stats,
                             d_workspace, static_cast<hipStream_t>(stream));
}

int nhip_consistency(const double *records, int32_t M, const nhip_consistency_spec_t *spec, int32_t *members, int32_t *n_members,
                     int64_t *stats) {
  int rc = consistency_spec_check(spec, "consistency");
  if (rc || (rc = count_check(M, "consistency"))) return rc;
  if ((rc = require_device())) return rc;
  NHIP_REQUIRE(n_members && stats && (M == 0 || (records && members)), "consistency: null pointer");
  Staged st;
  const double *dr = st.in(records, RECORD_DOUBLES * (size_t)M);
  int32_t *dm = st.out<int32_t>((size_t)M), *dn = st.out<int32_t>(1);
  int64_t *ds = st.out<int64_t>(STATS_WORDS);
  uint8_t *base = st.out<uint8_t>((size_t)workspace_bytes(M));
  if (st.ok()) {
    unsigned long long *d_adj = reinterpret_cast<unsigned long long *>(base + adj_offset());
    int32_t *d_deg = reinterpret_cast<int32_t *>(base + deg_offset(M));
    st.launched(launch_consistency_adjacency(dr, M, tol_of(*spec), d_adj, d_deg, reinterpret_cast<long long *>(ds), nullptr));
    if (st.ok())
      st.launched(consistency_set_run(reinterpret_cast<const uint64_t *>(d_adj), d_deg, M, *spec, CHECK_EVERY_DEFAULT, dm, dn, ds, base, nullptr));
  }
  st.fetch(members, dm, (size_t)M);
  st.fetch(n_members, dn, 1);
  st.fetch(stats, ds, STATS_WORDS);
  return st.finish();
}

}  // extern "C"
