// nhip_transient.hip -- K19: transient returns.  Every return of every scan, at the scan's pose, is classified by the two
// planes of the occupancy grid (K14) under it -- how many scans stopped around its cell, how many saw through the cell --
// and the returns that are not transient are packed into clouds of the layout every other entry point takes.  The spec is
// DESIGN.md section 3, "Transient returns"; tests/transient_reference.py restates it in numpy.  After the cells everything
// is integer, and the packing is a stable compaction: the results are the reference's bit for bit, the same every run.
//
//   transient_classify_kernel  a workgroup per scan, a wave per 64 consecutive beams of it, a lane per point: neighbouring
//                              beams end in neighbouring cells, so the (2 r + 1)^2 hit cells a wave gathers per step lie in a
//                              few cache lines of a few rows.  The point's cell as the occupancy grid forms it, S = the hits of
//                              the neighbourhood inside the window, m = the misses of the cell itself, the label byte.  The
//                              scan's kept count and its four label counts from wave ballots: one LDS add per wave, one plain
//                              store (the count, into out_offsets[s]) and four stats atomics per SCAN.
//   transient_offsets_kernel   one workgroup, 1024 scans per step, any number of steps: the exclusive scan of the kept counts
//                              in place (cut at n_points: see below), the three per-scan stats, and the report of the FIRST scan
//                              whose offsets are not a scan -- in scan order, so the record is the same every run.
//   transient_pack_kernel      a workgroup per scan: a lane's rank is the popcount of its wave's ballot below it plus the kept
//                              counts of the waves in front; the kept points and their indices go through LDS and leave as
//                              whole runs, lane t to out[o + t].
//
// Offsets are checked before they become addresses: a scan with a negative start, an end before its start or an end beyond
// n_points is empty in all three kernels.  Scans that are scans one by one may still overlap in the cloud; their kept counts
// can then sum to more than n_points, the capacity of the outputs: the offsets are cut at n_points and the pack kernel
// stores only below a scan's cut end, so the outputs stay inside their buffers (the labels of shared points are those of
// whichever scan wrote last).
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int TR_T = 256;
constexpr int TR_WAVES = TR_T / 64;
constexpr int TR_MAX_SCAN_BLOCKS = 4096;  // workgroups along the scans; more scans than that: grid-stride
constexpr int TR_OFF_T = 1024;
enum { TR_STATIC = 0, TR_TRANSIENT = 1, TR_UNOBSERVED = 2, TR_INVALID = 3 };

// the scan's [beg, end) if its offsets are a scan; else false and (value, index) of the offset at fault
__device__ __forceinline__ bool scan_range(const int32_t *__restrict__ offsets, int32_t s, int32_t n_points, int32_t *beg,
                                           int32_t *end, int32_t *bad_value, int32_t *bad_index) {
  const int32_t b = offsets[s], e = offsets[s + 1];
  *beg = b, *end = e;
  if (b < 0) {
    *bad_value = b, *bad_index = s;
    return false;
  }
  if (e < b || e > n_points) {
    *bad_value = e, *bad_index = s + 1;
    return false;
  }
  return true;
}

__device__ __forceinline__ int label_of(const TransientParams &P, float c, float sn, float tx, float ty, const float2 p) {
  const float x = __fadd_rn(__fadd_rn(__fmul_rn(c, p.x), __fmul_rn(-sn, p.y)), tx);
  const float y = __fadd_rn(__fadd_rn(__fmul_rn(sn, p.x), __fmul_rn(c, p.y)), ty);
  if (!isfinite(p.x) || !isfinite(p.y) || !isfinite(x) || !isfinite(y)) return TR_INVALID;
  const double fx = floor_quotient((double)x, P.res, P.inv_res), fy = floor_quotient((double)y, P.res, P.inv_res);
  if (!(fabs(fx) < 0x1p62) || !(fabs(fy) < 0x1p62)) return TR_INVALID;
  // int64 from here: |fx|, |fy| < 2^62 and the window's terms are int32, so no difference wraps
  const long long wx = (long long)fx - (long long)P.cell_x0, wy = (long long)fy - (long long)P.cell_y0;
  if (wx < 0 || wx >= (long long)P.width || wy < 0 || wy >= (long long)P.height) return TR_UNOBSERVED;
  const int32_t cx = (int32_t)wx, cy = (int32_t)wy, r = P.support_radius;
  const int32_t x_lo = cx - r > 0 ? cx - r : 0, x_hi = cx + r < P.width - 1 ? cx + r : P.width - 1;
  const int32_t y_lo = cy - r > 0 ? cy - r : 0, y_hi = cy + r < P.height - 1 ? cy + r : P.height - 1;
  long long S = 0;
  for (int32_t yy = y_lo; yy <= y_hi; yy++) {
    const int32_t *row = P.hits + (size_t)yy * (size_t)P.width;
    for (int32_t xx = x_lo; xx <= x_hi; xx++) S += (long long)row[xx];
  }
  const long long m = (long long)P.misses[(size_t)cy * (size_t)P.width + (size_t)cx];
  return (m >= (long long)P.min_through && 1000ll * S <= (long long)P.transient_permille * (S + m)) ? TR_TRANSIENT : TR_STATIC;
}

__global__ __launch_bounds__(TR_T) void transient_classify_kernel(TransientParams P, const float2 *__restrict__ xy,
                                                                  const int32_t *__restrict__ offsets,
                                                                  const float *__restrict__ affines) {
  __shared__ int32_t tally[4];  // of the scan: points of each label
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (long long ss = blockIdx.x; ss < P.n_scans; ss += gridDim.x) {
    const int32_t s = (int32_t)ss;
    int32_t beg, end, bv, bi;
    if (!scan_range(offsets, s, P.n_points, &beg, &end, &bv, &bi)) {  // (treated as empty: nothing is read; the offsets kernel reports it)
      if (tid == 0) P.out_offsets[s] = 0;
      continue;
    }
    if (tid < 4) tally[tid] = 0;
    __syncthreads();
    const float c = affines[4 * (size_t)s], sn = affines[4 * (size_t)s + 1], tx = affines[4 * (size_t)s + 2], ty = affines[4 * (size_t)s + 3];
    int32_t n[4] = {0, 0, 0, 0};  // of this wave (uniform)
    for (long long base = (long long)beg + wv * 64; base < end; base += TR_T) {
      const long long i = base + lane;
      int k = -1;
      if (i < end) {
        k = label_of(P, c, sn, tx, ty, xy[i]);
        P.labels[i] = (uint8_t)k;
      }
#pragma unroll
      for (int q = 0; q < 4; q++) n[q] += __builtin_popcountll(__ballot(k == q));
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (n[q]) atomicAdd(&tally[q], n[q]);
    }
    __syncthreads();
    if (tid == 0) P.out_offsets[s] = tally[TR_STATIC] + tally[TR_UNOBSERVED];  // (the count: the offsets kernel scans it in place)
    if (tid < 4 && tally[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(P.stats) + tid, (unsigned long long)tally[tid]);
    __syncthreads();  // (the tally is cleared for the workgroup's next scan)
  }
}

// One workgroup.  In: out_offsets[s] = the kept count of scan s.  Out: out_offsets[s] = the index of its first kept point,
// out_offsets[n_scans] = their number, both cut at n_points; stats[4..7].
__global__ __launch_bounds__(TR_OFF_T) void transient_offsets_kernel(TransientParams P, const int32_t *__restrict__ offsets) {
  __shared__ long long wave_sum[TR_OFF_T / 64];
  __shared__ int32_t first_bad;  // the lowest scan of the step whose offsets are not a scan
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  long long carry = 0;           // kept points of the steps before (uniform)
  int32_t n_bad = 0, n_emptied = 0;  // of this thread
  bool reported = false;             // (uniform)
  for (long long base = 0; base < P.n_scans; base += TR_OFF_T) {
    const int32_t s = (int32_t)(base + t < (long long)P.n_scans ? base + t : (long long)P.n_scans);
    if (t == 0) first_bad = INT32_MAX;
    __syncthreads();
    long long v = 0;
    int32_t bv = 0, bi = 0;
    bool bad = false;
    if (s < P.n_scans) {
      int32_t beg, end;
      bad = !scan_range(offsets, s, P.n_points, &beg, &end, &bv, &bi);
      v = (long long)P.out_offsets[s];
      n_bad += bad;
      n_emptied += !bad && end > beg && v == 0;
      if (bad) atomicMin(&first_bad, s);
    }
    long long inc = v;  // inclusive scan of the wave, then of the waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long u = __shfl_up(inc, d, 64);
      if (lane >= d) inc += u;
    }
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    long long before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < TR_OFF_T / 64; w++) {
      const long long q = wave_sum[w];
      if (w < wv) before += q;
      all += q;
    }
    if (s < P.n_scans) {
      const long long o = before + inc - v;
      P.out_offsets[s] = (int32_t)(o < (long long)P.n_points ? o : (long long)P.n_points);
    }
    if (!reported && first_bad != INT32_MAX) {
      if (s == first_bad) flag_bad_id(P.status, BAD_MAP_SCAN_OFFSETS, bv, bi);
      reported = true;
    }
    carry += all;
    __syncthreads();  // (wave_sum and first_bad are rewritten by the next step)
  }
  if (t == 0) P.out_offsets[P.n_scans] = (int32_t)(carry < (long long)P.n_points ? carry : (long long)P.n_points);
  // the per-scan stats: one add per wave
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_bad += __shfl_xor(n_bad, d, 64);
    n_emptied += __shfl_xor(n_emptied, d, 64);
  }
  unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
  if (lane == 0 && n_bad) atomicAdd(stats + 5, (unsigned long long)n_bad);
  if (lane == 0 && n_emptied) atomicAdd(stats + 6, (unsigned long long)n_emptied);
  if (t == 0) atomicAdd(stats + 4, (unsigned long long)P.n_scans);  // (bad ones included: they were processed as empty scans)
}

__global__ __launch_bounds__(TR_T) void transient_pack_kernel(TransientParams P, const float2 *__restrict__ xy,
                                                              const int32_t *__restrict__ offsets) {
  __shared__ float2 run_xy[TR_T];
  __shared__ int32_t run_index[TR_T];
  __shared__ int32_t wave_kept[TR_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (long long ss = blockIdx.x; ss < P.n_scans; ss += gridDim.x) {
    const int32_t s = (int32_t)ss;
    int32_t beg, end, bv, bi;
    if (!scan_range(offsets, s, P.n_points, &beg, &end, &bv, &bi)) continue;
    const int32_t o = P.out_offsets[s], o_end = P.out_offsets[s + 1];  // (0 <= o <= o_end <= n_points: the offsets kernel's)
    int32_t done = 0;  // points of this scan packed by the chunks before (uniform)
    for (long long base = beg; base < end; base += TR_T) {
      const long long i = base + tid;
      const bool keep = i < end && (P.labels[i] & 1u) == 0u;  // static or unobserved
      const unsigned long long m = __ballot(keep);
      if (lane == 0) wave_kept[wv] = __builtin_popcountll(m);
      __syncthreads();  // (also: every lane has read the runs of the chunk before)
      int32_t before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < TR_WAVES; w++) {
        const int32_t q = wave_kept[w];
        if (w < wv) before += q;
        all += q;
      }
      if (keep) {
        const int32_t rank = before + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        run_xy[rank] = xy[i];
        run_index[rank] = (int32_t)i;
      }
      __syncthreads();  // (and every lane has read the waves' counts)
      const long long at = (long long)o + done + tid;
      if (tid < all && at < (long long)o_end) {
        P.out_xy[at] = run_xy[tid];
        P.out_index[at] = run_index[tid];
      }
      done += all;
    }
    __syncthreads();  // (the runs and the counts are rewritten by the workgroup's next scan)
  }
}

}  // namespace

int launch_transient(const TransientParams &P, const float *d_xy, const int32_t *d_offsets, const float *d_affines, hipStream_t s) {
  NHIP_TRY_HIP(hipMemsetAsync(P.stats, 0, 8 * sizeof(long long), s));
  if (P.n_points > 0) NHIP_TRY_HIP(hipMemsetAsync(P.labels, TR_INVALID, (size_t)P.n_points, s));  // (a point of no scan keeps it)
  const uint32_t blocks = (uint32_t)(P.n_scans < TR_MAX_SCAN_BLOCKS ? P.n_scans : TR_MAX_SCAN_BLOCKS);
  const float2 *xy = reinterpret_cast<const float2 *>(d_xy);
  if (P.n_scans > 0) hipLaunchKernelGGL(transient_classify_kernel, dim3(blocks), dim3(TR_T), 0, s, P, xy, d_offsets, d_affines);
  hipLaunchKernelGGL(transient_offsets_kernel, dim3(1), dim3(TR_OFF_T), 0, s, P, d_offsets);
  if (P.n_scans > 0) hipLaunchKernelGGL(transient_pack_kernel, dim3(blocks), dim3(TR_T), 0, s, P, xy, d_offsets);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
