// nhip_pcg.h -- the block-Jacobi preconditioned CG step, defined ONCE for the two solvers of DESIGN.md section 3, "Block-sparse
// system": K11, one damped system (nhip_linsolve.hip), and K12, many ridged, gauged systems on one matrix
// (nhip_linsolve_columns.hip).  The flags: converged (||r|| <= tol ||b||), ended by the closing launch behind max_iters
// iterations, breakdown (a non-finite scalar, or p . q <= 0: decided before x is touched, so x stays the last iterate).
// NOT here, on purpose: each unit keeps its loads and stores of the state (K11: one owner thread; K12: per system) and
//   * its reduction shape: K11 sums 256 lanes by an LDS tree and gives long rows to workgroups of their own; K12 adds four
//     waves in wave order, system-minor.  The bit-level tests pin both;
//   * its matrix-vector body: K11 adds (lambda (a_ii + floor)) p as a term of its own, K12 multiplies (a_ii + ridge) p; the
//     two round differently and the numpy restatements specify both;
//   * its kernels: solve() is not the S = 1 case of the columns kernels -- that would change its bits and its speed.
#pragma once
#include "nhip_common.h"

namespace nhip {

constexpr int32_t PCG_CONVERGED = 0, PCG_MAX_ITERS = 1, PCG_BREAKDOWN = 2;  // nhip_pcg_stats_t.flag
__host__ __device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }  // (false for NaN)
__host__ __device__ __forceinline__ int32_t clamp_end(int32_t v, int32_t nnzb) { return v < 0 ? 0 : v > nnzb ? nnzb : v; }

// d = the diagonal block of row b: columns ascend within a row; a row without one has a zero diagonal block.  The damping
// goes between this and invert3, at the call site: K11 d_ii += lambda (d_ii + floor), K12 d_ii += ridge.
__host__ __device__ __forceinline__ void diag_block(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                    const double *__restrict__ values, int32_t b, int32_t nnzb, double (&d)[9]) {
#pragma unroll
  for (int e = 0; e < 9; e++) d[e] = 0.0;
  int32_t lo = clamp_end(row_ptr[b], nnzb), hi = clamp_end(row_ptr[b + 1], nnzb) - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (col[mid] < b) lo = mid + 1; else hi = mid;
  }
  if (lo == hi && col[lo] == b) {
#pragma unroll
    for (int e = 0; e < 9; e++) d[e] = values[9 * (size_t)lo + e];
  }
}

// m = d^-1 by cofactors (row-major 3 x 3); the order of every product and sum is part of the solvers' bits
__host__ __device__ __forceinline__ void invert3(const double (&d)[9], double (&m)[9]) {
  const double c00 = d[4] * d[8] - d[5] * d[7], c01 = d[5] * d[6] - d[3] * d[8], c02 = d[3] * d[7] - d[4] * d[6];
  const double inv = 1.0 / (d[0] * c00 + d[1] * c01 + d[2] * c02);
  m[0] = c00 * inv; m[1] = (d[2] * d[7] - d[1] * d[8]) * inv; m[2] = (d[1] * d[5] - d[2] * d[4]) * inv;
  m[3] = c01 * inv; m[4] = (d[0] * d[8] - d[2] * d[6]) * inv; m[5] = (d[2] * d[3] - d[0] * d[5]) * inv;
  m[6] = c02 * inv; m[7] = (d[1] * d[6] - d[0] * d[7]) * inv; m[8] = (d[0] * d[4] - d[1] * d[3]) * inv;
}

// z = M^-1 r of one block and the block's terms of r . r and r . z.  Entry i of z is written to z[i * stride], a row of m at
// a time: z may be the solver's vector in memory, which m may overlap for all the compiler knows, and the loads of m and
// the stores of z then keep the order they always had.
__host__ __device__ __forceinline__ void precondition(const double *m, const double (&r)[3], double *z, size_t stride, double *rr,
                                                      double *rz) {
  double v[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    v[i] = m[3 * i] * r[0] + m[3 * i + 1] * r[1] + m[3 * i + 2] * r[2];
    z[i * stride] = v[i];
  }
  *rr = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  *rz = r[0] * v[0] + r[1] * v[1] + r[2] * v[2];
}

// Iteration k's first kernel, `k` iterations complete: from r . r and r . z of the current residual, ||b||^2 and the r . z of
// iteration k - 1 (both ignored at k == 0, where bb is rr), the relative residual (of a zero right-hand side: 0 for a zero
// residual, else r . r), beta, and whether the solve ends here -- `final` is the closing launch -- with which flag.
struct DirectionStep { double relres, beta, bb; bool ended; int32_t flag; };
__host__ __device__ __forceinline__ DirectionStep direction_step(double rr, double rz, double bb_prev, double rz_prev, int32_t k,
                                                                 double tol, bool final) {
  const double bb = k == 0 ? rr : bb_prev, beta = k > 0 ? rz / rz_prev : 0.0;
  const double relres = bb > 0.0 ? sqrt(rr) / sqrt(bb) : (rr == 0.0 ? 0.0 : rr);
  const bool broke = !finite(rr) || !finite(rz) || !finite(beta);
  const bool converged = !broke && sqrt(rr) <= tol * sqrt(bb);
  return {relres, beta, bb, broke || converged || final, broke ? PCG_BREAKDOWN : converged ? PCG_CONVERGED : PCG_MAX_ITERS};
}

// Iteration k's second kernel: alpha = r . z / p . q; p . q <= 0 or a non-finite scalar is a breakdown, and the caller ends the
// solve with PCG_BREAKDOWN before it touches x.
struct UpdateStep { double alpha; bool broke; };
__host__ __device__ __forceinline__ UpdateStep update_step(double rz, double pq) {
  const double alpha = rz / pq;
  return {alpha, !(pq > 0.0) || !finite(pq) || !finite(alpha)};
}

// The pieces of a workspace, one behind the other from byte `o` of `base`, each ending at a multiple of `granule` bytes (a
// power of two).  With a null base it only measures: `o` ends as the workspace's size.
struct WsCarver {
  char *base;
  size_t o, granule;
  template <class T> T *take(size_t n) {
    T *p = reinterpret_cast<T *>(base + o);
    o += (n * sizeof(T) + granule - 1) & ~(granule - 1);
    return p;
  }
};

}  // namespace nhip
