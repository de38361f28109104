// nhip_host_linsolve.hip -- the linear-solve entry points of the C ABI (kernels: nhip_linsolve.hip, nhip_linsolve_columns.hip):
// argument checks, the workspace's size, and the one host loop of the library that looks at the device between launches --
// the PCG's convergence word, once per `check_every` iterations (one system, or many on one matrix).
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

namespace {

// The checks nhip_bsr_pcg_dev (one system) and nhip_bsr_pcg_columns_dev share; `who` names the entry point in the message.
struct PcgCall {
  const char *who;
  int32_t n_blocks, nnzb, n_systems, max_iters, check_every;
  int sizes() const {  // (an argument error with or without a device)
    NHIP_REQUIRE(n_blocks >= 0 && nnzb >= 0 && n_systems >= 0 && n_blocks <= (1 << 29), "%s: bad size", who);
    // (the kernels index a vector's 3 n_blocks n_systems doubles with 64 bits; the bound keeps every such vector below 16 GiB)
    NHIP_REQUIRE(3 * (int64_t)n_blocks * (int64_t)n_systems <= INT32_MAX,
                 "%s: 3 * %d blocks * %d systems is more than 2^31 - 1 doubles per vector: solve in chunks", who, n_blocks, n_systems);
    NHIP_REQUIRE(max_iters >= 0 && check_every >= 1, "%s: max_iters %d must be >= 0 and check_every %d >= 1", who, max_iters,
                 check_every);
    return NHIP_OK;
  }
  int workspace(const void *d_ws, int64_t bytes, int64_t need) const {
    NHIP_REQUIRE(bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)bytes, (long long)need);
    NHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_ws) & 15) == 0, "%s: d_workspace must be 16-byte aligned", who);
    return NHIP_OK;
  }
};

// The host loop of both solvers.  enqueue(first, last, final): the kernels of iterations first .. last - 1 (first == 0: the
// set-up in front of them; final: the closing check behind them).  Iterations are enqueued `check_every` at a time; between
// two batches still_running(&running) reads the end words once.  Kernels enqueued behind the end of a solve do not touch
// it, so x, the counts and the flags do not depend on check_every.  The closing launch (after max_iters iterations:
// converged or flag 1; nothing behind an earlier end) follows the set-up alone if max_iters is 0.
template <class Enqueue, class StillRunning>
int drive_pcg(int32_t max_iters, int32_t check_every, Enqueue enqueue, StillRunning still_running) {
  int rc;
  bool running = true;
  for (int32_t first = 0; first < max_iters && running;) {
    const int32_t last = max_iters - first > check_every ? first + check_every : max_iters;
    if ((rc = enqueue(first, last, false))) return rc;
    first = last;
    if (first < max_iters && (rc = still_running(&running))) return rc;
  }
  return enqueue(max_iters, max_iters, true);
}

}  // namespace

extern "C" {

int nhip_bsr_assemble_dev(const double *d_rows, int32_t n_rows, const int32_t *d_row_ptr, const int32_t *d_col,
                          const int32_t *d_contrib_ptr, const int32_t *d_contrib, int32_t n_blocks, int32_t nnzb,
                          int32_t n_contrib, double *d_values, double *d_grad, double *d_cost, void *stream) {
  // (sizes are an argument error with or without a device)
  NHIP_REQUIRE(n_rows >= 0 && n_blocks >= 0 && nnzb >= 0 && n_contrib >= 0, "bsr_assemble_dev: negative size");
  NHIP_REQUIRE(n_rows <= (1 << 29) && n_blocks <= (1 << 29), "bsr_assemble_dev: more than 2^29 rows or blocks");
  NHIP_REQUIRE(nnzb == 0 || n_blocks > 0, "bsr_assemble_dev: %d stored blocks of 0 unknown blocks", nnzb);
  int rc = require_device();
  if (rc) return rc;
  NHIP_REQUIRE(d_cost && (n_rows == 0 || d_rows) && (n_blocks == 0 || (d_row_ptr && d_grad)) &&
                   (nnzb == 0 || (d_col && d_contrib_ptr && d_values)) && (n_contrib == 0 || d_contrib),
               "bsr_assemble_dev: null pointer");
  return launch_bsr_assemble(d_rows, n_rows, d_row_ptr, d_col, d_contrib_ptr, d_contrib, n_blocks, nnzb, n_contrib, d_values,
                             d_grad, d_cost, static_cast<hipStream_t>(stream));
}

int64_t nhip_bsr_pcg_workspace_bytes(int32_t n_blocks, int32_t nnzb) { return bsr_pcg_workspace_bytes(n_blocks, nnzb); }

int nhip_bsr_pcg_dev(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const double *d_grad,
                     const uint8_t *d_fixed, int32_t n_blocks, int32_t nnzb, double lambda, double diag_floor, double tol,
                     int32_t max_iters, int32_t check_every, double *d_x, void *d_workspace, int64_t workspace_bytes,
                     nhip_pcg_stats_t *stats, void *stream) {
  const PcgCall call{"bsr_pcg_dev", n_blocks, nnzb, 1, max_iters, check_every};
  int rc = call.sizes();
  if (rc) return rc;
  NHIP_REQUIRE(std::isfinite(lambda) && lambda >= 0 && std::isfinite(diag_floor) && diag_floor >= 0 && tol >= 0,
               "bsr_pcg_dev: lambda and diag_floor must be finite and >= 0, tol >= 0");
  NHIP_REQUIRE(stats, "bsr_pcg_dev: null stats");
  if ((rc = require_device())) return rc;
  *stats = nhip_pcg_stats_t{0, 0, 0.0};
  if (n_blocks == 0) return NHIP_OK;
  NHIP_REQUIRE(d_row_ptr && d_grad && d_fixed && d_x && d_workspace && (nnzb == 0 || (d_col && d_values)),
               "bsr_pcg_dev: null pointer");
  if ((rc = call.workspace(d_workspace, workspace_bytes, bsr_pcg_workspace_bytes(n_blocks, nnzb)))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PcgStats st;  // the state in the workspace's first bytes
  auto read_state = [&](bool *running) {
    NHIP_TRY_HIP(hipMemcpyAsync(&st, d_workspace, sizeof(st), hipMemcpyDeviceToHost, s));
    NHIP_TRY_HIP(hipStreamSynchronize(s));
    *running = (st.done_a | st.done_b) == 0;
    return NHIP_OK;
  };
  auto enqueue = [&](int32_t first, int32_t last, bool final) {
    return launch_bsr_pcg(d_row_ptr, d_col, d_values, d_grad, d_fixed, n_blocks, nnzb, lambda, diag_floor, tol, first, last, final,
                          d_x, d_workspace, s);
  };
  bool running;
  if ((rc = drive_pcg(max_iters, check_every, enqueue, read_state)) || (rc = read_state(&running))) return rc;
  *stats = nhip_pcg_stats_t{st.iterations, st.flag, st.relres};
  return NHIP_OK;
}

int64_t nhip_bsr_pcg_columns_workspace_bytes(int32_t n_blocks, int32_t nnzb, int32_t n_systems) {
  return bsr_pcg_columns_workspace_bytes(n_blocks, nnzb, n_systems);
}

int nhip_bsr_pcg_columns_dev(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const uint8_t *d_fixed,
                             int32_t n_blocks, int32_t nnzb, const int32_t *d_gauge, const int32_t *d_rhs_index,
                             int32_t n_systems, double ridge, double tol, int32_t max_iters, int32_t check_every, double *d_x,
                             void *d_workspace, int64_t workspace_bytes, nhip_pcg_stats_t *stats, void *stream) {
  const PcgCall call{"bsr_pcg_columns_dev", n_blocks, nnzb, n_systems, max_iters, check_every};
  int rc = call.sizes();
  if (rc) return rc;
  NHIP_REQUIRE(std::isfinite(ridge) && ridge >= 0 && tol >= 0, "bsr_pcg_columns_dev: ridge must be finite and >= 0, tol >= 0");
  NHIP_REQUIRE(stats || n_systems == 0, "bsr_pcg_columns_dev: null stats");
  if ((rc = require_device())) return rc;
  for (int32_t i = 0; i < n_systems; i++) stats[i] = nhip_pcg_stats_t{0, 0, 0.0};
  if (n_blocks == 0 || n_systems == 0) return NHIP_OK;
  NHIP_REQUIRE(d_row_ptr && d_fixed && d_gauge && d_rhs_index && d_x && d_workspace && (nnzb == 0 || (d_col && d_values)),
               "bsr_pcg_columns_dev: null pointer");
  if ((rc = call.workspace(d_workspace, workspace_bytes, bsr_pcg_columns_workspace_bytes(n_blocks, nnzb, n_systems)))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t n_active = 0;  // the ONE word the host reads between two batches: the number of systems not yet ended
  auto still_running = [&](bool *running) {
    const int r = bsr_pcg_columns_read(d_workspace, n_blocks, n_systems, &n_active, nullptr, nullptr, nullptr, s);
    *running = n_active > 0;
    return r;
  };
  auto enqueue = [&](int32_t first, int32_t last, bool final) {
    return launch_bsr_pcg_columns(d_row_ptr, d_col, d_values, d_fixed, n_blocks, nnzb, d_gauge, d_rhs_index, n_systems, ridge, tol,
                                  first, last, final, d_x, d_workspace, s);
  };
  if ((rc = drive_pcg(max_iters, check_every, enqueue, still_running))) return rc;
  std::vector<int32_t> iters((size_t)n_systems), flag((size_t)n_systems);
  std::vector<double> relres((size_t)n_systems);
  if ((rc = bsr_pcg_columns_read(d_workspace, n_blocks, n_systems, &n_active, iters.data(), flag.data(), relres.data(), s)))
    return rc;
  for (int32_t i = 0; i < n_systems; i++) stats[i] = nhip_pcg_stats_t{iters[(size_t)i], flag[(size_t)i], relres[(size_t)i]};
  return NHIP_OK;
}

}  // extern "C"
