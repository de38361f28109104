// nhip_linsolve.hip -- K11: the linear step of the pose-graph solve on gfx950 ("Block-sparse system").
//
//   bsr_assemble_kernel    28-double rows (upper triangle of a 6 x 6 J^T J over [u | v], J^T r, r^T r) -> the 3 x 3 blocks of
//                          a block-sparse H, the gradient and the cost, every sum in ONE pinned order, no atomics
//   pcg_setup_kernel       the inverse of every damped diagonal block, x = 0, r = b = -g, z = M^-1 r, the list of long rows
//   pcg_direction_kernel   beta and the convergence test from the update kernel's partials; p = z + beta p formed on the
//                          load side of q = A p (p double-buffered); the partials of p . q
//   pcg_update_kernel      alpha from those partials; x += alpha p, r -= alpha q, z = M^-1 r; the partials of r . r, r . z
//
// Two launches per iteration.  Kernel boundaries are the only grid-wide synchronisation: every dot product leaves one
// partial per workgroup, written at a fixed index, and the NEXT kernel's prologue sums them in a fixed order, redundantly in
// every workgroup.  No floating-point atomics anywhere: the same input gives the same bits.  alpha, beta and the end-of-solve
// words live in the workspace; kernels enqueued after the end read the words and return.
// The method's step (the preconditioner, the scalars, the flags) is nhip_pcg.h's, shared with nhip_linsolve_columns.hip.
#include "nhip_pcg.h"

namespace nhip {

namespace {

constexpr int LT = 256;       // threads per workgroup
constexpr int LONG_ROW = 64;  // a block row of more blocks than this is a LONG row: a workgroup's, not a lane's
constexpr int LONG_WGS = 8;   // workgroups of the direction kernel that take the long rows in turn (a HITL line block's row
                              // holds one block per selected pose; there is one such row per constraint)

// index of (p, q), p <= q, in the row-major upper triangle of a 6 x 6
__host__ __device__ constexpr int tri(int p, int q) { return p * 6 - (p * (p - 1)) / 2 + (q - p); }

// entry (i, j) of quadrant Q of a row's 6 x 6: 0 (u,u), 1 (u,v), 2 (v,u) = quadrant 1 transposed, 3 (v,v)
template <int Q>
__device__ __forceinline__ void add_quadrant(double (&acc)[9], const double *__restrict__ row) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      const int e = Q == 0 ? tri(lo, hi) : Q == 3 ? tri(3 + lo, 3 + hi) : Q == 1 ? tri(i, 3 + j) : tri(j, 3 + i);
      acc[3 * i + j] += row[e];
    }
}

// The pinned sum's second half: partial[l] += partial[l + s] for s = 32, 16, ..., 1 over the 64 partials the lanes of a
// wave hold; lane 0 ends with the sum (the lanes above the step's reach hold values nobody reads).
__device__ __forceinline__ double wave_tree(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s, 64);
  return v;
}

// One wave per stored block (task k < nnzb), one more for the cost (task nnzb).  Lane l keeps partial l of the pinned sum:
// it adds the block's contributors l, l + 64, ... one by one from +0.0; wave_tree adds the partials.
__global__ __launch_bounds__(LT) void bsr_assemble_kernel(const double *__restrict__ rows, int32_t n_rows,
                                                          const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                          const int32_t *__restrict__ contrib_ptr,
                                                          const int32_t *__restrict__ contrib, int32_t nb, int32_t nnzb,
                                                          int32_t n_contrib, double *__restrict__ values,
                                                          double *__restrict__ grad, double *__restrict__ cost,
                                                          uint32_t *__restrict__ status) {
  const int64_t task = ((int64_t)blockIdx.x * LT + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (task > nnzb) return;
  if (task == nnzb) {
    double acc = 0.0;
    constexpr int LOADS = 8;  // (the adds of a partial are a chain; the loads in front of them need not be)
    for (int64_t r0 = lane; r0 < n_rows; r0 += 64 * LOADS) {
      double v[LOADS];
#pragma unroll
      for (int u = 0; u < LOADS; u++) {
        const int64_t r = r0 + 64 * u;
        v[u] = r < n_rows ? rows[28 * r + 27] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < LOADS; u++)
        if (r0 + 64 * u < n_rows) acc += v[u];
    }
    acc = wave_tree(acc);
    if (lane == 0) cost[0] = 0.5 * acc;
    return;
  }
  const int32_t k = (int32_t)task;
  // the block row: the last b with row_ptr[b] <= k (row_ptr is the caller's: non-decreasing, from 0 to nnzb)
  int32_t lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (row_ptr[mid] <= k) lo = mid; else hi = mid - 1;
  }
  const int32_t b = lo, c = col[k];
  const bool diag = c == b;
  int32_t o0 = contrib_ptr[k], o1 = contrib_ptr[k + 1];
  if (o0 < 0) o0 = 0;
  if (o1 > n_contrib) o1 = n_contrib;
  double acc[9], g[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int e = 0; e < 9; e++) acc[e] = 0.0;
  int32_t bad_id = 0;
  bool bad = false;
  for (int32_t t = o0 + lane; t < o1; t += 64) {
    const int32_t id = contrib[t];
    // (an id from device memory: one outside [0, 4 R) is reported, never dereferenced, and the block is zero)
    if (id < 0 || (int64_t)id >= 4 * (int64_t)n_rows) {
      bad = true;
      bad_id = id;
      continue;
    }
    const double *row = rows + 28 * (size_t)(id >> 2);
    const int q = id & 3;
    if (q == 0) add_quadrant<0>(acc, row);
    else if (q == 1) add_quadrant<1>(acc, row);
    else if (q == 2) add_quadrant<2>(acc, row);
    else add_quadrant<3>(acc, row);
    if (diag && (q == 0 || q == 3)) {
      const double *gr = row + (q == 0 ? 21 : 24);
      g[0] += gr[0];
      g[1] += gr[1];
      g[2] += gr[2];
    }
  }
  const bool bad_col = !id_in(c, nb);
  const unsigned long long bad_lanes = __ballot(bad);
  if (bad_lanes != 0ull || bad_col) {
    if (bad_col) {
      if (lane == 0) flag_bad_id(status, BAD_BLOCK_COLUMN, c, k);
    } else if (lane == __ffsll((long long)bad_lanes) - 1) {
      flag_bad_id(status, BAD_CONTRIB_ID, bad_id, k);
    }
    if (lane < 9) values[9 * (size_t)k + lane] = 0.0;
    if (diag && lane < 3) grad[3 * (size_t)b + lane] = 0.0;
    return;
  }
#pragma unroll
  for (int e = 0; e < 9; e++) acc[e] = wave_tree(acc[e]);
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < 9; e++) values[9 * (size_t)k + e] = acc[e];
  }
  if (diag) {  // (wave-uniform)
#pragma unroll
    for (int e = 0; e < 3; e++) g[e] = wave_tree(g[e]);
    if (lane == 0) {
      grad[3 * (size_t)b] = g[0];
      grad[3 * (size_t)b + 1] = g[1];
      grad[3 * (size_t)b + 2] = g[2];
    }
  }
}

// ---------------------------------------------------------------- preconditioned CG
// The workspace: 256 bytes of state, then the vectors.
struct PcgScalars {  // what the direction kernel of iteration k leaves for the update kernel of k and the direction kernel of k + 1
  double rz, relres;
};
struct PcgWs {
  PcgStats *st;        // byte 0
  PcgScalars *sc;      // byte 64: two entries, by the parity of the iteration
  int32_t *n_long;     // byte 128
  double *minv;        // 9 per block: the inverse of the damped diagonal block (zero for a fixed block)
  double *r, *z, *q;   // 3 per block
  double *p[2];        // the direction of iteration k is p[k & 1]
  int32_t *longs;      // the long rows, ascending (nb entries of room)
  double *pq, *rr, *rz;  // per-workgroup partials: p . q (ga + LONG_WGS), r . r and r . z (gb each)
  int32_t ga, gb;      // workgroups over the 3 nb scalar rows / over the nb blocks
  size_t bytes;
};
PcgWs pcg_ws(void *ws, int32_t nb) {
  PcgWs W;
  char *base = static_cast<char *>(ws);
  W.st = reinterpret_cast<PcgStats *>(base);
  W.sc = reinterpret_cast<PcgScalars *>(base + 64);
  W.n_long = reinterpret_cast<int32_t *>(base + 128);
  const size_t n3 = 3 * (size_t)nb;
  W.ga = (int32_t)((n3 + LT - 1) / LT);
  W.gb = (nb + LT - 1) / LT;
  WsCarver c{base, 256, 8};
  W.minv = c.take<double>(3 * n3);
  W.r = c.take<double>(n3);
  W.z = c.take<double>(n3);
  W.q = c.take<double>(n3);
  W.p[0] = c.take<double>(n3);
  W.p[1] = c.take<double>(n3);
  W.longs = c.take<int32_t>((size_t)nb);
  W.pq = c.take<double>((size_t)W.ga + LONG_WGS);
  W.rr = c.take<double>((size_t)W.gb);
  W.rz = c.take<double>((size_t)W.gb);
  W.bytes = c.o;
  return W;
}

// the sum of a workgroup's values in a fixed order (an LDS tree); every lane calls it and gets the sum
__device__ __forceinline__ double block_sum(double v, double *s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int st = LT / 2; st > 0; st >>= 1) {
    if (tid < st) s[tid] += s[tid + st];
    __syncthreads();
  }
  const double total = s[0];
  __syncthreads();
  return total;
}
// the prologue of a kernel: the per-workgroup partials the kernel before it left, summed in a fixed order
__device__ __forceinline__ double sum_partials(const double *__restrict__ part, int32_t n, double *s) {
  double v = 0.0;
  for (int32_t i = threadIdx.x; i < n; i += LT) v += part[i];
  return block_sum(v, s);
}

// the end of the solve, written by its one owner thread: `done` is the end word of the kernel that saw it
__device__ __forceinline__ void end_solve(PcgStats *st, int32_t k, int32_t flag, double relres, int32_t *done) {
  st->iterations = k;
  st->flag = flag;
  st->relres = relres;
  __threadfence();
  *done = 1;
}

// Workgroups 0 .. gb - 1: one lane per block.  Workgroup gb: the list of long rows, ascending.
__global__ __launch_bounds__(LT) void pcg_setup_kernel(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ values, const double *__restrict__ grad,
                                                       const uint8_t *__restrict__ fixed, int32_t nb, int32_t nnzb,
                                                       double lambda, double diag_floor, double *__restrict__ x, PcgWs W) {
  __shared__ double s_sum[LT];
  __shared__ int32_t s_cnt[LT / 64], s_base;
  const int tid = threadIdx.x;
  if ((int32_t)blockIdx.x == W.gb) {
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int32_t base = 0; base < nb; base += LT) {
      const int32_t b = base + tid;
      const bool is = b < nb && clamp_end(row_ptr[b + 1], nnzb) - clamp_end(row_ptr[b], nnzb) > LONG_ROW;
      const unsigned long long m = __ballot(is);
      if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(m);
      __syncthreads();
      int32_t off = s_base;
      for (int w = 0; w < (tid >> 6); w++) off += s_cnt[w];
      if (is) W.longs[off + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = b;
      __syncthreads();
      if (tid == 0) s_base += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      __syncthreads();
    }
    if (tid == 0) *W.n_long = s_base;
    return;
  }
  const int32_t b = blockIdx.x * LT + tid;
  double vrr = 0.0, vrz = 0.0;
  if (b < nb) {
    const bool fx = fixed[b] != 0;
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, r[3] = {0, 0, 0}, z[3] = {0, 0, 0};
    if (!fx) {
      double d[9];
      diag_block(row_ptr, col, values, b, nnzb, d);
#pragma unroll
      for (int i = 0; i < 3; i++) d[4 * i] += lambda * (d[4 * i] + diag_floor);
      invert3(d, m);
#pragma unroll
      for (int i = 0; i < 3; i++) r[i] = -grad[3 * (size_t)b + i];
      precondition(m, r, z, 1, &vrr, &vrz);
    }
#pragma unroll
    for (int e = 0; e < 9; e++) W.minv[9 * (size_t)b + e] = m[e];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t e = 3 * (size_t)b + i;
      x[e] = 0.0;
      W.r[e] = r[i];
      W.z[e] = z[i];
      W.p[0][e] = 0.0;
      W.p[1][e] = 0.0;
      W.q[e] = 0.0;
    }
  }
  vrr = block_sum(vrr, s_sum);
  vrz = block_sum(vrz, s_sum);
  if (tid == 0) {
    W.rr[blockIdx.x] = vrr;
    W.rz[blockIdx.x] = vrz;
    if (blockIdx.x == 0) {
      W.st->done_a = 0;
      W.st->done_b = 0;
      W.st->iterations = 0;
      W.st->flag = 0;
      W.st->relres = 0.0;
      W.st->bb = 0.0;
    }
  }
}

// Iteration k's first kernel; `k` iterations are complete when it starts.  Every workgroup forms the same scalars from the
// update kernel's partials (direction_step): the end of the solve or beta.  Then q = A p with p = z + beta p_old formed where
// it is loaded.  Workgroups 0 .. ga - 1: one lane per scalar row (a lane of a long row only writes its p); workgroups ga ..:
// the long rows in turn, a row's blocks dealt over the lanes, summed in a fixed order.
// (The end words: done_a is written here by workgroup 0 alone and only when every workgroup of this launch has decided to
//  return anyway -- they all evaluate the same partials -- so a workgroup that already reads it as set does what it would do.)
__global__ __launch_bounds__(LT) void pcg_direction_kernel(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                           const double *__restrict__ values,
                                                           const uint8_t *__restrict__ fixed, int32_t nb, int32_t nnzb,
                                                           double lambda, double diag_floor, double tol, int32_t k,
                                                           int32_t final, PcgWs W, uint32_t *__restrict__ status) {
  __shared__ double s_sum[LT];
  const int tid = threadIdx.x;
  {
    const volatile PcgStats *st = W.st;
    if (st->done_a | st->done_b) return;
  }
  const double rr = sum_partials(W.rr, W.gb, s_sum), rz = sum_partials(W.rz, W.gb, s_sum);
  // (the first iteration has none before it: nothing is loaded, and the step ignores both)
  const double bb_prev = k == 0 ? 0.0 : W.st->bb, rz_prev = k > 0 ? W.sc[(k - 1) & 1].rz : 0.0;
  const DirectionStep d = direction_step(rr, rz, bb_prev, rz_prev, k, tol, final != 0);
  if (d.ended) {
    if (blockIdx.x == 0 && tid == 0) end_solve(W.st, k, d.flag, d.relres, &W.st->done_a);
    return;
  }
  if (blockIdx.x == 0 && tid == 0) {
    W.sc[k & 1].rz = rz;
    W.sc[k & 1].relres = d.relres;
    if (k == 0) W.st->bb = d.bb;
  }
  const double beta = d.beta;
  const double *__restrict__ z = W.z;
  const double *__restrict__ pold = W.p[(k + 1) & 1];
  double *__restrict__ pnew = W.p[k & 1];
  // the direction's entry e, the same bits wherever it is formed
  auto pv = [&](size_t e) { return k == 0 ? z[e] : z[e] + beta * pold[e]; };
  if ((int32_t)blockIdx.x < W.ga) {
    const int64_t row = (int64_t)blockIdx.x * LT + tid;
    double v = 0.0;
    if (row < 3 * (int64_t)nb) {
      const int32_t b = (int32_t)(row / 3), i = (int32_t)(row - 3 * (int64_t)b);
      const bool fx = fixed[b] != 0;
      const double pn = fx ? 0.0 : pv((size_t)row);
      pnew[row] = pn;
      const int32_t beg = clamp_end(row_ptr[b], nnzb), end = clamp_end(row_ptr[b + 1], nnzb);
      if (fx) {
        W.q[row] = 0.0;
      } else if (end - beg <= LONG_ROW) {
        double acc = 0.0;
        for (int32_t kk = beg; kk < end; kk++) {
          const int32_t c = col[kk];
          if (!id_in(c, nb)) {  // (a column from device memory: reported, the block skipped)
            flag_bad_id(status, BAD_BLOCK_COLUMN, c, kk);
            continue;
          }
          if (fixed[c]) continue;
          const double *a = values + 9 * (size_t)kk + 3 * i;
          const double p0 = pv(3 * (size_t)c), p1 = pv(3 * (size_t)c + 1), p2 = pv(3 * (size_t)c + 2);
          acc += a[0] * p0;
          acc += a[1] * p1;
          acc += a[2] * p2;
          if (c == b) acc += (lambda * (a[i] + diag_floor)) * pn;
        }
        W.q[row] = acc;
        v = pn * acc;
      }
    }
    v = block_sum(v, s_sum);
    if (tid == 0) W.pq[blockIdx.x] = v;
    return;
  }
  double dot = 0.0;
  const int32_t n_long = *W.n_long;
  for (int32_t j = (int32_t)blockIdx.x - W.ga; j < n_long; j += LONG_WGS) {
    const int32_t b = W.longs[j];
    if (fixed[b]) continue;  // (its lanes above wrote q = 0)
    const int32_t beg = clamp_end(row_ptr[b], nnzb), end = clamp_end(row_ptr[b + 1], nnzb);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int32_t kk = beg + tid; kk < end; kk += LT) {
      const int32_t c = col[kk];
      if (!id_in(c, nb)) {
        flag_bad_id(status, BAD_BLOCK_COLUMN, c, kk);
        continue;
      }
      if (fixed[c]) continue;
      const double *a = values + 9 * (size_t)kk;
      const double p0 = pv(3 * (size_t)c), p1 = pv(3 * (size_t)c + 1), p2 = pv(3 * (size_t)c + 2);
      s0 += a[0] * p0; s0 += a[1] * p1; s0 += a[2] * p2;
      s1 += a[3] * p0; s1 += a[4] * p1; s1 += a[5] * p2;
      s2 += a[6] * p0; s2 += a[7] * p1; s2 += a[8] * p2;
      if (c == b) {
        s0 += (lambda * (a[0] + diag_floor)) * p0;
        s1 += (lambda * (a[4] + diag_floor)) * p1;
        s2 += (lambda * (a[8] + diag_floor)) * p2;
      }
    }
    s0 = block_sum(s0, s_sum);
    s1 = block_sum(s1, s_sum);
    s2 = block_sum(s2, s_sum);
    if (tid == 0) {
      const size_t e = 3 * (size_t)b;
      W.q[e] = s0;
      W.q[e + 1] = s1;
      W.q[e + 2] = s2;
      dot += pv(e) * s0;
      dot += pv(e + 1) * s1;
      dot += pv(e + 2) * s2;
    }
  }
  if (tid == 0) W.pq[blockIdx.x] = dot;
}

// Iteration k's second kernel, one lane per block: alpha or a breakdown (update_step; x stays the last iterate); x += alpha p,
// r -= alpha q, z = M^-1 r; the partials of r . r and r . z.
// (done_b: written by workgroup 0 alone, under the same rule as the direction kernel's done_a.)
__global__ __launch_bounds__(LT) void pcg_update_kernel(const uint8_t *__restrict__ fixed, int32_t nb, int32_t k,
                                                        double *__restrict__ x, PcgWs W) {
  __shared__ double s_sum[LT];
  const int tid = threadIdx.x;
  {
    const volatile PcgStats *st = W.st;
    if (st->done_a | st->done_b) return;
  }
  const double pq = sum_partials(W.pq, W.ga + LONG_WGS, s_sum);
  const UpdateStep u = update_step(W.sc[k & 1].rz, pq);
  const double alpha = u.alpha;
  if (u.broke) {
    if (blockIdx.x == 0 && tid == 0) end_solve(W.st, k, PCG_BREAKDOWN, W.sc[k & 1].relres, &W.st->done_b);
    return;
  }
  const int32_t b = blockIdx.x * LT + tid;
  double vrr = 0.0, vrz = 0.0;
  if (b < nb && !fixed[b]) {  // (a fixed block's x, r and z stay the zeros of the set-up)
    const double *p = W.p[k & 1] + 3 * (size_t)b, *q = W.q + 3 * (size_t)b, *m = W.minv + 9 * (size_t)b;
    double r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const size_t e = 3 * (size_t)b + i;
      x[e] += alpha * p[i];
      r[i] = W.r[e] - alpha * q[i];
      W.r[e] = r[i];
    }
    precondition(m, r, W.z + 3 * (size_t)b, 1, &vrr, &vrz);
  }
  vrr = block_sum(vrr, s_sum);
  vrz = block_sum(vrz, s_sum);
  if (tid == 0) {
    W.rr[blockIdx.x] = vrr;
    W.rz[blockIdx.x] = vrz;
  }
}

}  // namespace

int launch_bsr_assemble(const double *d_rows, int32_t n_rows, const int32_t *d_row_ptr, const int32_t *d_col,
                        const int32_t *d_contrib_ptr, const int32_t *d_contrib, int32_t nb, int32_t nnzb, int32_t n_contrib,
                        double *d_values, double *d_grad, double *d_cost, hipStream_t s) {
  // (a block row without a stored diagonal block -- the builder always stores one -- has no gradient written by the kernel)
  if (nb > 0) NHIP_TRY_HIP(hipMemsetAsync(d_grad, 0, sizeof(double) * 3 * (size_t)nb, s));
  const int64_t waves = (int64_t)nnzb + 1;
  hipLaunchKernelGGL(bsr_assemble_kernel, dim3((uint32_t)((waves * 64 + LT - 1) / LT)), dim3(LT), 0, s, d_rows, n_rows, d_row_ptr,
                     d_col, d_contrib_ptr, d_contrib, nb, nnzb, n_contrib, d_values, d_grad, d_cost, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int64_t bsr_pcg_workspace_bytes(int32_t nb, int32_t nnzb) {
  (void)nnzb;  // (nothing in the workspace is per stored block)
  return (int64_t)pcg_ws(nullptr, nb < 0 ? 0 : nb).bytes;
}

int launch_bsr_pcg(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const double *d_grad,
                   const uint8_t *d_fixed, int32_t nb, int32_t nnzb, double lambda, double diag_floor, double tol,
                   int32_t first, int32_t last, bool final, double *d_x, void *d_ws, hipStream_t s) {
  const PcgWs W = pcg_ws(d_ws, nb);
  if (first == 0)
    hipLaunchKernelGGL(pcg_setup_kernel, dim3(W.gb + 1), dim3(LT), 0, s, d_row_ptr, d_col, d_values, d_grad, d_fixed, nb, nnzb,
                       lambda, diag_floor, d_x, W);
  for (int32_t k = first; k < last; k++) {
    hipLaunchKernelGGL(pcg_direction_kernel, dim3(W.ga + LONG_WGS), dim3(LT), 0, s, d_row_ptr, d_col, d_values, d_fixed, nb, nnzb,
                       lambda, diag_floor, tol, k, 0, W, dev_status());
    hipLaunchKernelGGL(pcg_update_kernel, dim3(W.gb), dim3(LT), 0, s, d_fixed, nb, k, d_x, W);
  }
  if (final)
    hipLaunchKernelGGL(pcg_direction_kernel, dim3(1), dim3(LT), 0, s, d_row_ptr, d_col, d_values, d_fixed, nb, nnzb, lambda,
                       diag_floor, tol, last, 1, W, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
