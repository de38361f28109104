// nhip_vectorize.hip -- K13: the vector map.  Every scan at its pose, rasterised into one world window, the occupied cells
// reduced to wall segments by an exhaustive, deterministic Hough transform with greedy peak extraction.  The spec is
// DESIGN.md section 3, "Map vectorisation"; tests/vectorize_reference.py restates it in numpy.  After the point transform
// everything is integer, so sums by atomics are order-free and the results are the reference's bit for bit.
//
//   map_raster_kernel      a workgroup per scan: the float affine of §3 "Submaps", the cell by floor_quotient, integer
//                          atomicAdd on counts.  A scan whose offsets are not a scan is empty and reported (kind 16384).
//   cells_row_count_kernel a workgroup per raster row: its cells with counts >= min_hits.
//   cells_offsets_kernel   one workgroup: the exclusive scan over the rows, M, the capacity rule (flag 3).
//   cells_pack_kernel      a workgroup per row: its cells in ascending cx behind the row's offset -- the row-major order
//                          is part of the contract, so no atomically claimed slots.
//   hough_votes_kernel     the hot path, M x n_theta votes.  A workgroup per (rho slab, theta row): VOTE_SLAB bins of the
//                          row in LDS, the cell list streamed with 8-byte loads (L2-resident after the first row), LDS
//                          integer atomics, the slab written with plain stores: no global atomics, no zero-fill pass.
//   a round                vec_peak_kernel (the key max over votes, PEAK_BLOCKS partial keys), vec_peak_final_kernel (the
//                          peak, the two ways a call ends at a round's start), vec_band_kernel (band cells into a list --
//                          its order is never observable -- and their along-line bits), vec_runs_kernel (one workgroup: runs,
//                          kept runs, record slots, retire / commit / stop), vec_commit_kernel (deaths, moments, the bits
//                          cleared), vec_unvote_kernel (n_theta votes of every dead cell subtracted, a lane per vote).
// A round boundary is a launch boundary; every kernel of a round returns at once when VecState::end is set.
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int VEC_T = 256;
constexpr int VOTE_SLAB = 8192;    // bins of a theta row a votes workgroup holds in LDS (32 KB)
constexpr int PEAK_BLOCKS = 256;   // partial keys of the peak reduction
constexpr int ROUND_BLOCKS = 512;  // workgroups of the grid-stride kernels of a round
constexpr int Q = 14;

__device__ __forceinline__ int32_t rho_q(int32_t cx, int32_t cy, int32_t c, int32_t s, int32_t width) {
  return cx * c + cy * s + (width << Q);
}
// index of the along-line bin in the bit row: a + height, a the floor (arithmetic shift: a_q is negative where c < 0)
__device__ __forceinline__ int32_t along_index(int32_t cx, int32_t cy, int32_t c, int32_t s, int32_t width, int32_t height) {
  return ((cy * c - cx * s + (width << Q)) >> Q) + height;
}

__global__ __launch_bounds__(VEC_T) void map_raster_kernel(VecParams P, const float2 *__restrict__ xy,
                                                           const int32_t *__restrict__ offsets,
                                                           const float *__restrict__ affines) {
  for (int32_t s = blockIdx.x; s < P.n_scans; s += gridDim.x) {
    const int32_t beg = offsets[s], end = offsets[s + 1];
    if (!(beg >= 0 && end >= beg)) {  // (treated as empty: nothing is read)
      if (threadIdx.x == 0) flag_bad_id(P.status, BAD_MAP_SCAN_OFFSETS, beg < 0 ? beg : end, beg < 0 ? s : s + 1);
      continue;
    }
    const float c = affines[4 * (size_t)s], sn = affines[4 * (size_t)s + 1], tx = affines[4 * (size_t)s + 2],
                ty = affines[4 * (size_t)s + 3];
    for (int32_t i = beg + (int32_t)threadIdx.x; i < end; i += VEC_T) {
      const float2 p = xy[i];
      const float x = __fadd_rn(__fadd_rn(__fmul_rn(c, p.x), __fmul_rn(-sn, p.y)), tx);
      const float y = __fadd_rn(__fadd_rn(__fmul_rn(sn, p.x), __fmul_rn(c, p.y)), ty);
      if (!isfinite(x) || !isfinite(y)) continue;
      const double fx = floor_quotient((double)x, P.res, P.inv_res), fy = floor_quotient((double)y, P.res, P.inv_res);
      if (!(fabs(fx) < 0x1p63) || !(fabs(fy) < 0x1p63)) continue;  // (does not fit an int64: dropped, as SetPointValue's test would)
      const long long lx = (long long)fx, ly = (long long)fy;
      // (compared before the subtraction, which then cannot wrap)
      if (lx < (long long)P.cell_x0 || lx >= (long long)P.cell_x0 + P.width) continue;
      if (ly < (long long)P.cell_y0 || ly >= (long long)P.cell_y0 + P.height) continue;
      const long long cx = lx - P.cell_x0, cy = ly - P.cell_y0;
      atomicAdd(&P.counts[(size_t)cy * (size_t)P.width + (size_t)cx], 1);
    }
  }
}

__global__ __launch_bounds__(VEC_T) void cells_row_count_kernel(VecParams P) {
  __shared__ int32_t total;
  for (int32_t row = blockIdx.x; row < P.height; row += gridDim.x) {
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int32_t n = 0;
    const int32_t *r = P.counts + (size_t)row * (size_t)P.width;
    for (int32_t x = threadIdx.x; x < P.width; x += VEC_T) n += r[x] >= P.min_hits;
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) P.row_off[row] = total;
    __syncthreads();
  }
}

// inclusive scan over the 1024 lanes of a workgroup (sum, or max); leaves the inclusive values in sh
template <bool IS_MAX>
__device__ __forceinline__ int32_t scan1024(int32_t v, int32_t *sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int32_t u = t >= off ? sh[t - off] : (IS_MAX ? INT32_MIN : 0);
    __syncthreads();
    sh[t] = IS_MAX ? (u > sh[t] ? u : sh[t]) : sh[t] + u;
    __syncthreads();
  }
  return sh[t];
}

__global__ __launch_bounds__(1024) void cells_offsets_kernel(VecParams P) {
  __shared__ int32_t sh[1024];
  __shared__ long long carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int32_t base = 0; base < P.height; base += 1024) {
    const int32_t row = base + t;
    const int32_t n = row < P.height ? P.row_off[row] : 0;
    const int32_t inc = scan1024<false>(n, sh);
    if (row < P.height) P.row_off[row] = (int32_t)carry + inc - n;  // (M <= 2^28 cells: int32 holds every offset)
    __syncthreads();
    if (t == 0) carry += sh[1023];
    __syncthreads();
  }
  if (t == 0) {
    VecState *st = P.st;
    const int32_t M = (int32_t)carry;
    P.row_off[P.height] = M;
    st->stats[0] = M;
    st->stats[6] = P.n_rho;
    if (M > P.max_cells) {  // the capacity rule: nothing is packed, voted or vectorised
      st->stats[3] = 3;
      st->end = 1;
    }
  }
}

__global__ __launch_bounds__(VEC_T) void cells_pack_kernel(VecParams P) {
  __shared__ int32_t wave_n[VEC_T / 64];
  if (P.st->end) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int32_t row = blockIdx.x; row < P.height; row += gridDim.x) {
    int32_t base = P.row_off[row];
    const int32_t *r = P.counts + (size_t)row * (size_t)P.width;
    for (int32_t x0 = 0; x0 < P.width; x0 += VEC_T) {
      const int32_t x = x0 + tid;
      const bool occ = x < P.width && r[x] >= P.min_hits;
      const unsigned long long m = __ballot(occ);
      if (lane == 0) wave_n[wv] = __popcll(m);
      __syncthreads();
      int32_t before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < VEC_T / 64; w++) {
        const int32_t c = wave_n[w];
        if (w < wv) before += c;
        all += c;
      }
      if (occ) {
        const int32_t at = base + before + __popcll(m & ((1ull << lane) - 1ull));  // (< M <= max_cells)
        P.cells[2 * (size_t)at] = x;
        P.cells[2 * (size_t)at + 1] = row;
        P.live[at] = 1;
      }
      base += all;
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(VEC_T) void hough_votes_kernel(VecParams P) {
  __shared__ int32_t slab[VOTE_SLAB];
  if (P.st->end) return;
  const int32_t t = blockIdx.y, b0 = blockIdx.x * VOTE_SLAB, M = P.st->stats[0];
  for (int j = threadIdx.x; j < VOTE_SLAB; j += VEC_T) slab[j] = 0;
  __syncthreads();
  const int32_t c = P.C[t], s = P.S[t];
  const int2 *cells = reinterpret_cast<const int2 *>(P.cells);
  for (int32_t i = threadIdx.x; i < M; i += VEC_T) {
    const int2 cell = cells[i];
    const int32_t b = (rho_q(cell.x, cell.y, c, s, P.width) >> Q) - b0;
    if ((uint32_t)b < (uint32_t)VOTE_SLAB) atomicAdd(&slab[b], 1);
  }
  __syncthreads();
  int32_t *row = P.votes + (size_t)t * (size_t)P.n_rho;
  for (int j = threadIdx.x; j < VOTE_SLAB && b0 + j < P.n_rho; j += VEC_T) row[b0 + j] = slab[j];
}

// votes << 32 | ~index: max takes the largest votes and among equals the smallest index (§3 item 5's device)
__device__ __forceinline__ unsigned long long block_max_key(unsigned long long key, unsigned long long *sh) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long u = __shfl_xor(key, d, 64);
    key = u > key ? u : key;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = key;
  __syncthreads();
  unsigned long long best = sh[0];
#pragma unroll
  for (int w = 1; w < VEC_T / 64; w++) best = sh[w] > best ? sh[w] : best;
  return best;
}

__global__ __launch_bounds__(VEC_T) void vec_peak_kernel(VecParams P) {
  __shared__ unsigned long long sh[VEC_T / 64];
  if (P.st->end) return;
  const uint32_t total = (uint32_t)P.n_theta * (uint32_t)P.n_rho;  // (<= 1024 * 49153)
  unsigned long long key = 0;
  for (uint32_t i = blockIdx.x * VEC_T + threadIdx.x; i < total; i += PEAK_BLOCKS * VEC_T) {
    const unsigned long long k = ((unsigned long long)(uint32_t)P.votes[i] << 32) | (uint32_t)~i;
    key = k > key ? k : key;
  }
  key = block_max_key(key, sh);
  if (threadIdx.x == 0) P.partial[blockIdx.x] = key;
}

__global__ __launch_bounds__(VEC_T) void vec_peak_final_kernel(VecParams P) {
  __shared__ unsigned long long sh[VEC_T / 64];
  VecState *st = P.st;
  if (st->end) return;
  static_assert(PEAK_BLOCKS == VEC_T, "a lane per partial key");
  const unsigned long long key = block_max_key(P.partial[threadIdx.x], sh);
  if (threadIdx.x != 0) return;
  const int32_t votes = (int32_t)(key >> 32);
  const uint32_t idx = ~(uint32_t)key;
  if (votes < P.min_votes) {
    st->stats[3] = 0;
    st->end = 1;
  } else if (st->stats[2] >= P.max_rounds) {
    st->stats[3] = 1;
    st->end = 1;
  } else {
    st->peak_t = (int32_t)(idx / (uint32_t)P.n_rho);
    st->peak_b = (int32_t)(idx % (uint32_t)P.n_rho);
    st->peak_votes = votes;
    st->n_band = 0;
  }
}

__global__ __launch_bounds__(VEC_T) void vec_band_kernel(VecParams P) {
  VecState *st = P.st;
  if (st->end) return;
  const int32_t M = st->stats[0], t = st->peak_t, c = P.C[t], s = P.S[t];
  const int32_t centre = (st->peak_b << Q) + (1 << (Q - 1));
  const int2 *cells = reinterpret_cast<const int2 *>(P.cells);
  for (int32_t i = blockIdx.x * VEC_T + threadIdx.x; i < M; i += ROUND_BLOCKS * VEC_T) {
    if (!P.live[i]) continue;
    const int2 cell = cells[i];
    const int32_t d = rho_q(cell.x, cell.y, c, s, P.width) - centre;
    if ((d < 0 ? -d : d) > P.band_q) continue;
    const int32_t a = along_index(cell.x, cell.y, c, s, P.width, P.height);  // (0 <= a < n_along)
    atomicOr(&P.bits[a >> 5], 1u << (a & 31));
    P.band_list[atomicAdd(&st->n_band, 1)] = i;  // (at most M entries; their order is never observable)
  }
}

// One workgroup, a chunk of consecutive along-line bins per lane.  A set bin starts a run iff the set bin before it lies
// more than gap1 = max_gap + 1 back (or there is none): the last set bin before every chunk comes from a max-scan, the
// number of runs started before it from a sum-scan.  Then the same two steps over the runs for the kept ones.
__global__ __launch_bounds__(1024) void vec_runs_kernel(VecParams P) {
  __shared__ int32_t sh[1024];
  VecState *st = P.st;
  if (st->end) return;
  const int t = threadIdx.x, n = P.n_along;
  const int chunk = (n + 1023) / 1024;
  const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  const uint32_t *bits = P.bits;
  int32_t last = -1;
  for (int j = lo; j < hi; j++)
    if ((bits[j >> 5] >> (j & 31)) & 1u) last = j;
  scan1024<true>(last, sh);
  const int32_t prev0 = t ? sh[t - 1] : -1, last_all = sh[1023];
  __syncthreads();
  int32_t prev = prev0, starts = 0;
  for (int j = lo; j < hi; j++)
    if ((bits[j >> 5] >> (j & 31)) & 1u) {
      starts += prev < 0 || j - prev > P.gap1;
      prev = j;
    }
  const int32_t started = scan1024<false>(starts, sh) - starts;  // runs started before this chunk
  const int32_t R = sh[1023];
  __syncthreads();
  prev = prev0;
  int32_t rid = started - 1;
  for (int j = lo; j < hi; j++)
    if ((bits[j >> 5] >> (j & 31)) & 1u) {
      if (prev < 0 || j - prev > P.gap1) {
        rid++;  // (< R <= max_runs)
        P.run_lo[rid] = j;
        if (prev >= 0) P.run_hi[rid - 1] = prev;
      }
      P.run_of_bin[j] = rid;
      prev = j;
    }
  if (t == 0 && R > 0) P.run_hi[R - 1] = last_all;
  __syncthreads();  // (run_lo, run_hi: written above by other lanes of this workgroup)
  const int rchunk = (R + 1023) / 1024;
  const int rlo = t * rchunk < R ? t * rchunk : R, rhi = rlo + rchunk < R ? rlo + rchunk : R;
  int32_t kept = 0;
  for (int r = rlo; r < rhi; r++) kept += P.run_hi[r] - P.run_lo[r] + 1 >= P.min_length;
  int32_t slot = scan1024<false>(kept, sh) - kept;
  const int32_t K = sh[1023], segments = st->stats[1];
  const bool fits = K <= P.max_segments - segments;
  if (K > 0 && fits)
    for (int r = rlo; r < rhi; r++) {
      const int32_t a_lo = P.run_lo[r], a_hi = P.run_hi[r];
      if (a_hi - a_lo + 1 < P.min_length) {
        P.run_slot[r] = -1;
        continue;
      }
      const int32_t at = segments + slot++;  // (< max_segments)
      P.run_slot[r] = at;
      long long *rec = P.records + 10 * (size_t)at;
      rec[0] = st->peak_t;
      rec[1] = st->peak_b;
      rec[2] = a_lo - P.height;
      rec[3] = a_hi - P.height;
      for (int k = 4; k < 10; k++) rec[k] = 0;
    }
  __syncthreads();  // (every lane has read `segments`)
  if (t != 0) return;
  if (K > 0 && !fits) {  // nothing of this round is committed
    st->stats[3] = 2;
    st->end = 1;
    return;
  }
  st->action = K > 0 ? VEC_COMMIT : VEC_RETIRE;
  st->stats[1] = segments + K;
  st->stats[2] += 1;
}

__global__ __launch_bounds__(VEC_T) void vec_commit_kernel(VecParams P) {
  VecState *st = P.st;
  if (st->end) return;
  const int32_t nb = st->n_band, t = st->peak_t, c = P.C[t], s = P.S[t];
  const bool retire = st->action == VEC_RETIRE;
  for (int32_t k = blockIdx.x * VEC_T + threadIdx.x; k < nb; k += ROUND_BLOCKS * VEC_T) {
    const int32_t i = P.band_list[k];
    const int32_t cx = P.cells[2 * (size_t)i], cy = P.cells[2 * (size_t)i + 1];
    const int32_t a = along_index(cx, cy, c, s, P.width, P.height);
    P.bits[a >> 5] = 0u;  // (nobody reads the bits here; every writer of the word stores 0)
    if (retire) {
      P.live[i] = 0;
      atomicAdd(&st->stats[5], 1);
      continue;
    }
    const int32_t slot = P.run_slot[P.run_of_bin[a]];
    if (slot < 0) {
      P.band_list[k] = -1;  // stays live: no votes to subtract
      continue;
    }
    P.live[i] = 0;
    atomicAdd(&st->stats[4], 1);
    unsigned long long *rec = reinterpret_cast<unsigned long long *>(P.records + 10 * (size_t)slot);
    const unsigned long long x = (unsigned long long)cx, y = (unsigned long long)cy;
    atomicAdd(rec + 4, 1ull);
    atomicAdd(rec + 5, x);
    atomicAdd(rec + 6, y);
    atomicAdd(rec + 7, x * x);
    atomicAdd(rec + 8, x * y);
    atomicAdd(rec + 9, y * y);
  }
}

__global__ __launch_bounds__(VEC_T) void vec_unvote_kernel(VecParams P) {
  VecState *st = P.st;
  if (st->end) return;
  const long long total = (long long)st->n_band * P.n_theta;
  for (long long k = (long long)blockIdx.x * VEC_T + threadIdx.x; k < total; k += (long long)ROUND_BLOCKS * VEC_T) {
    const int32_t e = (int32_t)(k / P.n_theta), t = (int32_t)(k - (long long)e * P.n_theta);
    const int32_t i = P.band_list[e];
    if (i < 0) continue;
    const int32_t b = rho_q(P.cells[2 * (size_t)i], P.cells[2 * (size_t)i + 1], P.C[t], P.S[t], P.width) >> Q;
    atomicSub(&P.votes[(size_t)t * (size_t)P.n_rho + (size_t)b], 1);
  }
}

}  // namespace

int launch_vec_front(const VecParams &P, const float *d_xy, const int32_t *d_offsets, const float *d_affines, hipStream_t s) {
  timer_begin(NHIP_TIMER_VEC_RASTER, s);
  NHIP_TRY_HIP(hipMemsetAsync(P.st, 0, sizeof(VecState), s));
  NHIP_TRY_HIP(hipMemsetAsync(P.counts, 0, sizeof(int32_t) * (size_t)P.width * (size_t)P.height, s));
  NHIP_TRY_HIP(hipMemsetAsync(P.bits, 0, sizeof(uint32_t) * (size_t)((P.n_along + 31) / 32), s));
  if (P.n_scans > 0)
    hipLaunchKernelGGL(map_raster_kernel, dim3((uint32_t)(P.n_scans < 65536 ? P.n_scans : 65536)), dim3(VEC_T), 0, s, P,
                       reinterpret_cast<const float2 *>(d_xy), d_offsets, d_affines);
  const dim3 rows((uint32_t)(P.height < 4096 ? P.height : 4096));
  hipLaunchKernelGGL(cells_row_count_kernel, rows, dim3(VEC_T), 0, s, P);
  hipLaunchKernelGGL(cells_offsets_kernel, dim3(1), dim3(1024), 0, s, P);
  hipLaunchKernelGGL(cells_pack_kernel, rows, dim3(VEC_T), 0, s, P);
  timer_end(NHIP_TIMER_VEC_RASTER, s);
  timer_begin(NHIP_TIMER_VEC_VOTES, s);
  hipLaunchKernelGGL(hough_votes_kernel, dim3((uint32_t)((P.n_rho + VOTE_SLAB - 1) / VOTE_SLAB), (uint32_t)P.n_theta), dim3(VEC_T),
                     0, s, P);
  timer_end(NHIP_TIMER_VEC_VOTES, s);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_vec_rounds(const VecParams &P, int32_t n, hipStream_t s) {
  timer_begin(NHIP_TIMER_VEC_ROUNDS, s);
  for (int32_t r = 0; r < n; r++) {
    hipLaunchKernelGGL(vec_peak_kernel, dim3(PEAK_BLOCKS), dim3(VEC_T), 0, s, P);
    hipLaunchKernelGGL(vec_peak_final_kernel, dim3(1), dim3(VEC_T), 0, s, P);
    hipLaunchKernelGGL(vec_band_kernel, dim3(ROUND_BLOCKS), dim3(VEC_T), 0, s, P);
    hipLaunchKernelGGL(vec_runs_kernel, dim3(1), dim3(1024), 0, s, P);
    hipLaunchKernelGGL(vec_commit_kernel, dim3(ROUND_BLOCKS), dim3(VEC_T), 0, s, P);
    hipLaunchKernelGGL(vec_unvote_kernel, dim3(ROUND_BLOCKS), dim3(VEC_T), 0, s, P);
  }
  timer_end(NHIP_TIMER_VEC_ROUNDS, s);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
