// nhip_linsolve_columns.hip -- K12: columns of the inverse of the pose graph's matrix, MANY systems on ONE matrix (DESIGN.md
// section 3, "Block-sparse system"; section 8 item 13).  System s solves (H + ridge I) x = e_j, j = rhs_index[s], over the
// blocks that are neither in the shared `fixed` mask nor block gauge[s], by nhip_linsolve.hip's block-Jacobi PCG, with its own
// alpha, beta, end words, count and residual.
//
//   columns_setup_kernel      the inverse of every ridged diagonal block (shared by the systems), x = 0, r = b = e_j, z = M^-1 r
//   columns_direction_kernel  per system: beta and the end tests from the update kernel's partials; p = z + beta p_old formed on
//                             the load side of q = A p (p double-buffered); the partials of p . q
//   columns_update_kernel     per system: alpha from those partials; x += alpha p, r -= alpha q, z = M^-1 r; the partials of
//                             r . r and r . z
//
// Layout: x and every work vector are system-minor, element e of system s at [e * S + s].  A workgroup is CT systems x CB
// block rows: the 64 lanes of a wave hold 64 adjacent systems of ONE block row, so row_ptr, col, the nine doubles of a stored
// block and the fixed mask are the same address across the wave (read once per wave for 64 systems) and every load of z and p
// is 512 contiguous bytes.  A wave takes block rows w, w + 4, ... of the workgroup's CB; a lane owns the three scalar rows of a
// block for one system.
//
// The reduction shape of every dot product depends on n_blocks alone: a lane adds its blocks' terms in row order, the four
// waves' sums are added in wave order (one partial per workgroup of rows, at [g * S + s]), and the next kernel adds the
// partials g = w, w + 4, ... in each wave and the four waves' sums in wave order.  Nothing a system computes depends on the
// lane it sits in, on S or on the other systems: its bits are the same alone and in any batch.  No floating-point atomics.
// A system that has ended is never written again; its lanes idle through the barriers.  A workgroup returns early only when
// all its systems had ended before the launch -- decided from ONE read of the end words, shared through LDS, so that the
// four waves decide alike.
// The method's step (the preconditioner, the scalars, the flags) is nhip_pcg.h's, shared with nhip_linsolve.hip.
#include "nhip_pcg.h"

namespace nhip {

namespace {

constexpr int CT = 64;        // systems per workgroup: one wave's lanes
constexpr int CW = 4;         // waves per workgroup
constexpr int CLT = CT * CW;  // threads per workgroup
constexpr int CB = 32;        // block rows per workgroup (CB / CW per wave)

// The workspace: 256 bytes of header (byte 0: the number of systems not yet ended), the per-system state, then the vectors.
struct ColWs {
  int32_t *n_active;
  int32_t *ended, *iters, *flag;  // S each
  double *relres, *bb;            // S each
  double *rz_at, *rel_at;         // 2 S each: r . z and the relative residual of iteration k at [(k & 1) * S + s]
  double *minv;                   // 9 per block: the inverse of the ridged diagonal block (zero for a block of the mask)
  double *r, *z, *q, *p[2];       // 3 nb S each, system-minor
  double *pq, *rr, *rz;           // g S each: the partials, [g * S + s]
  int32_t g;                      // workgroups over the block rows
  size_t bytes;
};
ColWs col_ws(void *ws, int32_t nb, int32_t S) {
  ColWs W;
  W.n_active = static_cast<int32_t *>(ws);
  const size_t s = (size_t)S, v = 3 * (size_t)nb * s;
  W.g = (nb + CB - 1) / CB;
  WsCarver c{static_cast<char *>(ws), 256, 16};
  W.ended = c.take<int32_t>(s);
  W.iters = c.take<int32_t>(s);
  W.flag = c.take<int32_t>(s);
  W.relres = c.take<double>(s);
  W.bb = c.take<double>(s);
  W.rz_at = c.take<double>(2 * s);
  W.rel_at = c.take<double>(2 * s);
  W.minv = c.take<double>(9 * (size_t)nb);
  W.r = c.take<double>(v);
  W.z = c.take<double>(v);
  W.q = c.take<double>(v);
  W.p[0] = c.take<double>(v);
  W.p[1] = c.take<double>(v);
  W.pq = c.take<double>((size_t)W.g * s);
  W.rr = c.take<double>((size_t)W.g * s);
  W.rz = c.take<double>((size_t)W.g * s);
  W.bytes = c.o;
  return W;
}

// the wave's index as a value the compiler knows to be the same in every lane (what is loaded by it is loaded once per wave)
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// The four waves' values of every system, added in wave order; every lane gets its system's sum.
__device__ __forceinline__ double waves_sum(double v, double (*s_part)[CT], int w, int lane) {
  s_part[w][lane] = v;
  __syncthreads();
  const double total = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
  __syncthreads();
  return total;
}
// The prologue of a kernel: the n per-workgroup partials of system s that the kernel before it left, in a fixed order.
__device__ __forceinline__ double sum_partials(const double *__restrict__ part, int32_t n, size_t S, size_t s, bool on,
                                               double (*s_part)[CT], int w, int lane) {
  double v = 0.0;
  if (on)
    for (int32_t g = w; g < n; g += CW) v += part[(size_t)g * S + s];
  return waves_sum(v, s_part, w, lane);
}
// The workgroup's one look at the end words: true if a system of it is still running; `live` is this lane's system's state.
__device__ __forceinline__ bool any_live(const int32_t *ended, int32_t S, int32_t s, int32_t *s_end, bool *live) {
  if (threadIdx.x < CT) s_end[threadIdx.x] = s < S ? reinterpret_cast<const volatile int32_t *>(ended)[s] : 1;
  __syncthreads();
  *live = s_end[threadIdx.x & 63] == 0;
  return __syncthreads_or(*live) != 0;
}
__device__ __forceinline__ void end_system(const ColWs &W, int32_t s, int32_t k, int32_t flag, double relres) {
  W.iters[s] = k;
  W.flag[s] = flag;
  W.relres[s] = relres;
  __threadfence();
  W.ended[s] = 1;
  atomicSub(W.n_active, 1);
}

// grid (g, ceil(S / CT)).  A gauge or a right-hand side outside its range is compared, never used as an index: the system is
// zero, ended with flag 2, and reported.  Workgroup row 0 owns the systems' state and the count of running systems (zeroed by
// the launcher in front of this kernel); system tile 0 writes the shared preconditioner.
__global__ __launch_bounds__(CLT) void columns_setup_kernel(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                            const double *__restrict__ values, const uint8_t *__restrict__ fixed,
                                                            int32_t nb, int32_t nnzb, const int32_t *__restrict__ gauge,
                                                            const int32_t *__restrict__ rhs_index, int32_t S, double ridge,
                                                            double *__restrict__ x, ColWs W, uint32_t *__restrict__ status) {
  __shared__ double s_part[CW][CT];
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int32_t s = blockIdx.y * CT + lane;
  const bool on = s < S;
  const int32_t gs = on ? gauge[s] : -1, js = on ? rhs_index[s] : 0;
  const bool good = gs >= -1 && gs < nb && js >= 0 && (int64_t)js < 3 * (int64_t)nb;
  const int32_t jb = js / 3, ji = js - 3 * jb;
  double vrr = 0.0, vrz = 0.0;
  for (int32_t b = blockIdx.x * CB + w; b < nb && b < (int32_t)(blockIdx.x + 1) * CB; b += CW) {
    const bool fx = fixed[b] != 0;
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!fx) {
      double d[9];
      diag_block(row_ptr, col, values, b, nnzb, d);
#pragma unroll
      for (int i = 0; i < 3; i++) d[4 * i] += ridge;
      invert3(d, m);
    }
    if (blockIdx.y == 0 && lane == 0) {
#pragma unroll
      for (int e = 0; e < 9; e++) W.minv[9 * (size_t)b + e] = m[e];
    }
    if (!on) continue;
    double r[3] = {0, 0, 0}, z[3] = {0, 0, 0};
    if (good && !fx && b != gs && b == jb) {
#pragma unroll
      for (int i = 0; i < 3; i++) r[i] = i == ji ? 1.0 : 0.0;
      double trr, trz;
      precondition(m, r, z, 1, &trr, &trz);
      vrr += trr;
      vrz += trz;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t e = (3 * (size_t)b + i) * (size_t)S + s;
      x[e] = 0.0;
      W.r[e] = r[i];
      W.z[e] = z[i];
      W.p[0][e] = 0.0;
      W.p[1][e] = 0.0;
      W.q[e] = 0.0;
    }
  }
  vrr = waves_sum(vrr, s_part, w, lane);
  vrz = waves_sum(vrz, s_part, w, lane);
  if (w == 0 && on) {
    W.rr[(size_t)blockIdx.x * S + s] = vrr;
    W.rz[(size_t)blockIdx.x * S + s] = vrz;
    if (blockIdx.x == 0) {
      W.ended[s] = good ? 0 : 1;
      W.iters[s] = 0;
      W.flag[s] = good ? PCG_CONVERGED : PCG_BREAKDOWN;
      W.relres[s] = 0.0;
      W.bb[s] = 0.0;
      if (good) atomicAdd(W.n_active, 1);
      else flag_bad_id(status, BAD_SYSTEM_ID, (gs < -1 || gs >= nb) ? gs : js, s);
    }
  }
}

// Iteration k's first kernel; `k` iterations are complete when it starts.  Every workgroup of a system tile forms the same
// scalars per system from the update kernel's partials (direction_step): the end of the solve or beta.  Then q = A p with
// p = z + beta p_old formed where it is loaded.  (The end words of a system are written by workgroup row 0 alone, and only
// where every workgroup of this launch decides alike -- they all evaluate the same partials -- so a workgroup that already
// reads a system as ended does what it would do.)
__global__ __launch_bounds__(CLT) void columns_direction_kernel(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                                const double *__restrict__ values,
                                                                const uint8_t *__restrict__ fixed, int32_t nb, int32_t nnzb,
                                                                const int32_t *__restrict__ gauge, int32_t S, double ridge,
                                                                double tol, int32_t k, int32_t final, ColWs W,
                                                                uint32_t *__restrict__ status) {
  __shared__ double s_part[CW][CT];
  __shared__ int32_t s_end[CT];
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int32_t s = blockIdx.y * CT + lane;
  bool live;
  if (!any_live(W.ended, S, s, s_end, &live)) return;
  const size_t Ss = (size_t)S;
  const double rr = sum_partials(W.rr, W.g, Ss, s, live, s_part, w, lane);
  const double rz = sum_partials(W.rz, W.g, Ss, s, live, s_part, w, lane);
  double beta = 0.0;
  if (live) {
    // (the first iteration has none before it: nothing is loaded, and the step ignores both)
    const double bb_prev = k == 0 ? 0.0 : W.bb[s], rz_prev = k > 0 ? W.rz_at[(size_t)((k - 1) & 1) * Ss + s] : 0.0;
    const DirectionStep d = direction_step(rr, rz, bb_prev, rz_prev, k, tol, final != 0);
    const bool owner = blockIdx.x == 0 && w == 0;
    beta = d.beta;
    if (d.ended) {
      if (owner) end_system(W, s, k, d.flag, d.relres);
      live = false;
    } else if (owner) {
      W.rz_at[(size_t)(k & 1) * Ss + s] = rz;
      W.rel_at[(size_t)(k & 1) * Ss + s] = d.relres;
      if (k == 0) W.bb[s] = d.bb;
    }
  }
  const int32_t gs = live ? gauge[s] : -1;  // (a running system's gauge is in [-1, nb): the set-up ended the others)
  const double *__restrict__ z = W.z;
  const double *__restrict__ pold = W.p[(k + 1) & 1];
  double *__restrict__ pnew = W.p[k & 1];
  // the direction's entry e of this lane's system, the same bits wherever it is formed
  auto pv = [&](size_t e) { return k == 0 ? z[e * Ss + s] : z[e * Ss + s] + beta * pold[e * Ss + s]; };
  double dot = 0.0;
  for (int32_t b = blockIdx.x * CB + w; b < nb && b < (int32_t)(blockIdx.x + 1) * CB; b += CW) {
    if (fixed[b]) continue;  // (wave-uniform; x, r, z, p and q of a block of the mask stay the zeros of the set-up)
    if (!live || b == gs) continue;
    const size_t e0 = 3 * (size_t)b;
    const double pn0 = pv(e0), pn1 = pv(e0 + 1), pn2 = pv(e0 + 2);
    pnew[e0 * Ss + s] = pn0;
    pnew[(e0 + 1) * Ss + s] = pn1;
    pnew[(e0 + 2) * Ss + s] = pn2;
    const int32_t beg = clamp_end(row_ptr[b], nnzb), end = clamp_end(row_ptr[b + 1], nnzb);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int32_t kk = beg; kk < end; kk++) {
      const int32_t c = col[kk];
      if (!id_in(c, nb)) {  // (a column from device memory: reported, the block skipped)
        flag_bad_id(status, BAD_BLOCK_COLUMN, c, kk);
        continue;
      }
      if (fixed[c] || c == gs) continue;
      const double *a = values + 9 * (size_t)kk;
      const bool dg = c == b;
      const double p0 = dg ? pn0 : pv(3 * (size_t)c), p1 = dg ? pn1 : pv(3 * (size_t)c + 1), p2 = dg ? pn2 : pv(3 * (size_t)c + 2);
      const double r0 = dg ? ridge : 0.0;  // (H + ridge I: the entry is ridged, then multiplied)
      a0 += (a[0] + r0) * p0; a0 += a[1] * p1; a0 += a[2] * p2;
      a1 += a[3] * p0; a1 += (a[4] + r0) * p1; a1 += a[5] * p2;
      a2 += a[6] * p0; a2 += a[7] * p1; a2 += (a[8] + r0) * p2;
    }
    W.q[e0 * Ss + s] = a0;
    W.q[(e0 + 1) * Ss + s] = a1;
    W.q[(e0 + 2) * Ss + s] = a2;
    dot += pn0 * a0;
    dot += pn1 * a1;
    dot += pn2 * a2;
  }
  dot = waves_sum(dot, s_part, w, lane);
  if (w == 0 && live) W.pq[(size_t)blockIdx.x * Ss + s] = dot;
}

// Iteration k's second kernel: alpha or a breakdown per system (update_step; x stays the last iterate); x += alpha p,
// r -= alpha q, z = M^-1 r; the partials of r . r and r . z.
__global__ __launch_bounds__(CLT) void columns_update_kernel(const uint8_t *__restrict__ fixed, int32_t nb,
                                                             const int32_t *__restrict__ gauge, int32_t S, int32_t k,
                                                             double *__restrict__ x, ColWs W) {
  __shared__ double s_part[CW][CT];
  __shared__ int32_t s_end[CT];
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int32_t s = blockIdx.y * CT + lane;
  bool live;
  if (!any_live(W.ended, S, s, s_end, &live)) return;
  const size_t Ss = (size_t)S;
  const double pq = sum_partials(W.pq, W.g, Ss, s, live, s_part, w, lane);
  double alpha = 0.0;
  if (live) {
    const UpdateStep u = update_step(W.rz_at[(size_t)(k & 1) * Ss + s], pq);
    alpha = u.alpha;
    if (u.broke) {
      if (blockIdx.x == 0 && w == 0) end_system(W, s, k, PCG_BREAKDOWN, W.rel_at[(size_t)(k & 1) * Ss + s]);
      live = false;
    }
  }
  const int32_t gs = live ? gauge[s] : -1;
  const double *__restrict__ p = W.p[k & 1];
  double vrr = 0.0, vrz = 0.0;
  for (int32_t b = blockIdx.x * CB + w; b < nb && b < (int32_t)(blockIdx.x + 1) * CB; b += CW) {
    if (fixed[b]) continue;
    if (!live || b == gs) continue;
    const double *m = W.minv + 9 * (size_t)b;
    double r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t e = (3 * (size_t)b + i) * Ss + s;
      x[e] += alpha * p[e];
      r[i] = W.r[e] - alpha * W.q[e];
      W.r[e] = r[i];
    }
    double trr, trz;
    precondition(m, r, W.z + 3 * (size_t)b * Ss + s, Ss, &trr, &trz);
    vrr += trr;
    vrz += trz;
  }
  vrr = waves_sum(vrr, s_part, w, lane);
  vrz = waves_sum(vrz, s_part, w, lane);
  if (w == 0 && live) {
    W.rr[(size_t)blockIdx.x * Ss + s] = vrr;
    W.rz[(size_t)blockIdx.x * Ss + s] = vrz;
  }
}

}  // namespace

int64_t bsr_pcg_columns_workspace_bytes(int32_t nb, int32_t nnzb, int32_t S) {
  (void)nnzb;  // (nothing in the workspace is per stored block)
  return (int64_t)col_ws(nullptr, nb < 0 ? 0 : nb, S < 0 ? 0 : S).bytes;
}

int launch_bsr_pcg_columns(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const uint8_t *d_fixed,
                           int32_t nb, int32_t nnzb, const int32_t *d_gauge, const int32_t *d_rhs_index, int32_t S, double ridge,
                           double tol, int32_t first, int32_t last, bool final, double *d_x, void *d_ws, hipStream_t s) {
  const ColWs W = col_ws(d_ws, nb, S);
  const dim3 grid((uint32_t)W.g, (uint32_t)((S + CT - 1) / CT));
  if (first == 0) {
    NHIP_TRY_HIP(hipMemsetAsync(d_ws, 0, 256, s));
    hipLaunchKernelGGL(columns_setup_kernel, grid, dim3(CLT), 0, s, d_row_ptr, d_col, d_values, d_fixed, nb, nnzb, d_gauge,
                       d_rhs_index, S, ridge, d_x, W, dev_status());
  }
  for (int32_t k = first; k < last; k++) {
    hipLaunchKernelGGL(columns_direction_kernel, grid, dim3(CLT), 0, s, d_row_ptr, d_col, d_values, d_fixed, nb, nnzb, d_gauge, S,
                       ridge, tol, k, 0, W, dev_status());
    hipLaunchKernelGGL(columns_update_kernel, grid, dim3(CLT), 0, s, d_fixed, nb, d_gauge, S, k, d_x, W);
  }
  if (final)
    hipLaunchKernelGGL(columns_direction_kernel, dim3(1, grid.y), dim3(CLT), 0, s, d_row_ptr, d_col, d_values, d_fixed, nb, nnzb,
                       d_gauge, S, ridge, tol, last, 1, W, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int bsr_pcg_columns_read(const void *d_ws, int32_t nb, int32_t S, int32_t *n_active, int32_t *iters, int32_t *flag,
                         double *relres, hipStream_t s) {
  const ColWs W = col_ws(const_cast<void *>(d_ws), nb, S);
  NHIP_TRY_HIP(hipMemcpyAsync(n_active, W.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (iters) {
    NHIP_TRY_HIP(hipMemcpyAsync(iters, W.iters, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, s));
    NHIP_TRY_HIP(hipMemcpyAsync(flag, W.flag, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, s));
    NHIP_TRY_HIP(hipMemcpyAsync(relres, W.relres, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, s));
  }
  NHIP_TRY_HIP(hipStreamSynchronize(s));
  return NHIP_OK;
}

}  // namespace nhip
