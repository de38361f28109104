// nhip_host_linsolve.hip -- the linear-solve entry points of the C ABI (kernels: nhip_linsolve.hip, nhip_linsolve_columns.hip): argument checks, the
// workspace's size, and the one host loop of the library that looks at the device between launches -- the PCG's
// convergence word, once per `check_every` iterations (one system, or many on one matrix).
#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

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
  NHIP_REQUIRE(n_blocks >= 0 && nnzb >= 0 && n_blocks <= (1 << 29), "bsr_pcg_dev: bad size");
  NHIP_REQUIRE(max_iters >= 0 && check_every >= 1, "bsr_pcg_dev: max_iters %d must be >= 0 and check_every %d >= 1", max_iters,
               check_every);
  NHIP_REQUIRE(std::isfinite(lambda) && lambda >= 0 && std::isfinite(diag_floor) && diag_floor >= 0 && tol >= 0,
               "bsr_pcg_dev: lambda and diag_floor must be finite and >= 0, tol >= 0");
  NHIP_REQUIRE(stats, "bsr_pcg_dev: null stats");
  int rc = require_device();
  if (rc) return rc;
  stats->iterations = 0;
  stats->flag = 0;
  stats->relative_residual = 0.0;
  if (n_blocks == 0) return NHIP_OK;
  NHIP_REQUIRE(d_row_ptr && d_grad && d_fixed && d_x && d_workspace && (nnzb == 0 || (d_col && d_values)),
               "bsr_pcg_dev: null pointer");
  NHIP_REQUIRE(workspace_bytes >= bsr_pcg_workspace_bytes(n_blocks, nnzb), "bsr_pcg_dev: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)bsr_pcg_workspace_bytes(n_blocks, nnzb));
  NHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "bsr_pcg_dev: d_workspace must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // Iterations are enqueued `check_every` at a time; between two batches the host reads the end words once.  Kernels
  // enqueued after the end are no-ops, so x, the count and the flag do not depend on check_every.
  PcgStats st;
  bool ended = false;
  for (int32_t first = 0; first < max_iters && !ended;) {
    const int32_t last = max_iters - first > check_every ? first + check_every : max_iters;
    if ((rc = launch_bsr_pcg(d_row_ptr, d_col, d_values, d_grad, d_fixed, n_blocks, nnzb, lambda, diag_floor, tol, first, last,
                             false, d_x, d_workspace, s)))
      return rc;
    first = last;
    if (first < max_iters) {
      NHIP_TRY_HIP(hipMemcpyAsync(&st, d_workspace, sizeof(st), hipMemcpyDeviceToHost, s));
      NHIP_TRY_HIP(hipStreamSynchronize(s));
      ended = (st.done_a | st.done_b) != 0;
    }
  }
  // the closing check (after max_iters iterations: converged or flag 1; a no-op behind an earlier end); with max_iters 0
  // it follows the set-up alone (first == 0 enqueues it)
  if ((rc = launch_bsr_pcg(d_row_ptr, d_col, d_values, d_grad, d_fixed, n_blocks, nnzb, lambda, diag_floor, tol, max_iters,
                           max_iters, true, d_x, d_workspace, s)))
    return rc;
  NHIP_TRY_HIP(hipMemcpyAsync(&st, d_workspace, sizeof(st), hipMemcpyDeviceToHost, s));
  NHIP_TRY_HIP(hipStreamSynchronize(s));
  stats->iterations = st.iterations;
  stats->flag = st.flag;
  stats->relative_residual = st.relres;
  return NHIP_OK;
}

int64_t nhip_bsr_pcg_columns_workspace_bytes(int32_t n_blocks, int32_t nnzb, int32_t n_systems) {
  return bsr_pcg_columns_workspace_bytes(n_blocks, nnzb, n_systems);
}

int nhip_bsr_pcg_columns_dev(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const uint8_t *d_fixed,
                             int32_t n_blocks, int32_t nnzb, const int32_t *d_gauge, const int32_t *d_rhs_index,
                             int32_t n_systems, double ridge, double tol, int32_t max_iters, int32_t check_every, double *d_x,
                             void *d_workspace, int64_t workspace_bytes, nhip_pcg_stats_t *stats, void *stream) {
  NHIP_REQUIRE(n_blocks >= 0 && nnzb >= 0 && n_systems >= 0 && n_blocks <= (1 << 29), "bsr_pcg_columns_dev: bad size");
  // (the kernels index a vector's 3 n_blocks n_systems doubles with 64 bits; the bound keeps every such vector below 16 GiB)
  NHIP_REQUIRE(3 * (int64_t)n_blocks * (int64_t)n_systems <= INT32_MAX,
               "bsr_pcg_columns_dev: 3 * %d blocks * %d systems is more than 2^31 - 1 doubles per vector: solve in chunks", n_blocks,
               n_systems);
  NHIP_REQUIRE(max_iters >= 0 && check_every >= 1, "bsr_pcg_columns_dev: max_iters %d must be >= 0 and check_every %d >= 1",
               max_iters, check_every);
  NHIP_REQUIRE(std::isfinite(ridge) && ridge >= 0 && tol >= 0, "bsr_pcg_columns_dev: ridge must be finite and >= 0, tol >= 0");
  NHIP_REQUIRE(stats || n_systems == 0, "bsr_pcg_columns_dev: null stats");
  int rc = require_device();
  if (rc) return rc;
  for (int32_t i = 0; i < n_systems; i++) stats[i] = nhip_pcg_stats_t{0, 0, 0.0};
  if (n_blocks == 0 || n_systems == 0) return NHIP_OK;
  NHIP_REQUIRE(d_row_ptr && d_fixed && d_gauge && d_rhs_index && d_x && d_workspace && (nnzb == 0 || (d_col && d_values)),
               "bsr_pcg_columns_dev: null pointer");
  const int64_t need = bsr_pcg_columns_workspace_bytes(n_blocks, nnzb, n_systems);
  NHIP_REQUIRE(workspace_bytes >= need, "bsr_pcg_columns_dev: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)need);
  NHIP_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "bsr_pcg_columns_dev: d_workspace must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto enqueue = [&](int32_t first, int32_t last, bool final) {
    return launch_bsr_pcg_columns(d_row_ptr, d_col, d_values, d_fixed, n_blocks, nnzb, d_gauge, d_rhs_index, n_systems, ridge, tol,
                                  first, last, final, d_x, d_workspace, s);
  };
  // nhip_bsr_pcg_dev's loop: `check_every` iterations are enqueued at a time; between two batches the host reads ONE word,
  // the number of systems not yet ended.  Kernels enqueued behind a system's end do not touch it.
  int32_t running = 1;
  for (int32_t first = 0; first < max_iters && running > 0;) {
    const int32_t last = max_iters - first > check_every ? first + check_every : max_iters;
    if ((rc = enqueue(first, last, false))) return rc;
    first = last;
    if (first < max_iters && (rc = bsr_pcg_columns_read(d_workspace, n_blocks, n_systems, &running, nullptr, nullptr, nullptr, s)))
      return rc;
  }
  // the closing check (after max_iters iterations: converged or flag 1; nothing for a system that ended earlier); with
  // max_iters 0 it follows the set-up alone (first == 0 enqueues it)
  if ((rc = enqueue(max_iters, max_iters, true))) return rc;
  std::vector<int32_t> iters((size_t)n_systems), flag((size_t)n_systems);
  std::vector<double> relres((size_t)n_systems);
  if ((rc = bsr_pcg_columns_read(d_workspace, n_blocks, n_systems, &running, iters.data(), flag.data(), relres.data(), s)))
    return rc;
  for (int32_t i = 0; i < n_systems; i++) stats[i] = nhip_pcg_stats_t{iters[(size_t)i], flag[(size_t)i], relres[(size_t)i]};
  return NHIP_OK;
}

}  // extern "C"
