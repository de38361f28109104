// nhip_corr.hip -- K5: correspondence search on gfx950.
//
// Replaces, batched over all (source, target) residual blocks of a problem build,
//   Solver::GetPointToPointMatching          src/optimization/solver.cc:132-172
//   FindClosestPoint                         src/optimization/solver.cc:80-90
//   KDTree<float,2>::FindNearestPoint        src/util/kdtree.cc:253-305
// which the reference runs from scratch for every (i, j) block and every window size
// (solver.cc:321-356): three tree descents per matched point.
//
// Per block one workgroup: the target cloud is staged in LDS (8 B per point) in the order of its buckets; every lane owns
// a contiguous range of source points, transforms them into the target frame with the float affine
// inverse(T_target) * T_source (Eigen Affine2f semantics, individually rounded products) and visits the 3 x 3 cells
// around each, so the kept rows equal an exhaustive scan's (exact nearest neighbour, ties to the lowest index, kept if
// within the threshold).  The search itself -- cells, buckets, the walk, the tie rule, and why they find the exhaustive
// scan's answer -- is nhip_corr_shared.h, which the match refinement (nhip_refine.hip) uses too.
// Target clouds larger than the LDS stage, or coordinates so large that float cell indices are
// no longer exact, take the exhaustive scan (LDS broadcast reads).  Kept rows are written in
// source order (block-wide exclusive scan of the per-lane counts) as the 8-float rows K4 consumes.
// ~25 candidates per source point instead of 1081.  Where the time goes (tools/corr_phase_probe.py, 9,945 blocks of
// 1081-point scans, 0.58 ms): staging, sort and the rows' output 0.06 ms; the walk 0.52 ms, and it is its per-candidate
// iterations under divergent trip counts (a wave runs a bucket run as long as its fullest lane needs: ~40 % of the lanes
// work) -- not the point reads (0.02 ms), not the index indirection (points in bucket order: -3 %), not the per-run
// setup (runs of three cells instead of nine single cells: -1.5 %); one loop per lane over all nine cells, which would
// iterate max-over-lanes of the totals, was measured slower (0.68 ms: its cell-advance test runs every iteration).
#include "nhip_corr_shared.h"

namespace nhip {

namespace {

using namespace corr;

constexpr int TGT_CHUNK = 2048;  // target points staged per pass (16 KB)
constexpr int MAX_PER_LANE = 8;  // source points a lane owns per pass (2048 per pass)

struct Aff2f {
  float m00, m01, m10, m11, tx, ty;
};

__device__ __forceinline__ Aff2f pose_affine(const float *a) {  // cos sin x y
  return {a[0], -a[1], a[1], a[0], a[2], a[3]};
}

__device__ __forceinline__ Aff2f inverse_f(const Aff2f &A) {
  const float det = __fsub_rn(__fmul_rn(A.m00, A.m11), __fmul_rn(A.m10, A.m01));
  const float invdet = __fdiv_rn(1.0f, det);
  Aff2f R;
  R.m00 = __fmul_rn(A.m11, invdet);
  R.m10 = __fmul_rn(-A.m10, invdet);
  R.m01 = __fmul_rn(-A.m01, invdet);
  R.m11 = __fmul_rn(A.m00, invdet);
  R.tx = -__fadd_rn(__fmul_rn(R.m00, A.tx), __fmul_rn(R.m01, A.ty));
  R.ty = -__fadd_rn(__fmul_rn(R.m10, A.tx), __fmul_rn(R.m11, A.ty));
  return R;
}

__device__ __forceinline__ Aff2f mul_f(const Aff2f &A, const Aff2f &B) {
  Aff2f C;
  C.m00 = dot2(A.m00, B.m00, A.m01, B.m10);
  C.m01 = dot2(A.m00, B.m01, A.m01, B.m11);
  C.m10 = dot2(A.m10, B.m00, A.m11, B.m10);
  C.m11 = dot2(A.m10, B.m01, A.m11, B.m11);
  C.tx = __fadd_rn(dot2(A.m00, B.tx, A.m01, B.ty), A.tx);
  C.ty = __fadd_rn(dot2(A.m10, B.tx, A.m11, B.ty), A.ty);
  return C;
}

// GATE: the normal gate of Solver::GetPointToNormalMatching / FindClosestPointWithSimilarNormal
// (solver.cc:177-260): candidates are the targets within the threshold whose normal satisfies
// |n_target . n_source| > min_cos (NormalsSimilar, math_util.h:46-49; n_source stays in the source
// frame, as in the reference); the nearest candidate wins, ties to the lowest index.
template <bool GATE>
__global__ __launch_bounds__(CT) void corr_search_kernel(
    const float2 *__restrict__ xy, const float2 *__restrict__ normals,
    const int32_t *__restrict__ offsets, const int32_t *__restrict__ block_src,
    const int32_t *__restrict__ block_tgt, const float *__restrict__ pose_aff, float thr, float min_cos,
    const int64_t *__restrict__ cap_offsets, float4 *__restrict__ corr,
    int32_t *__restrict__ counts, int32_t n_scans, uint32_t *__restrict__ status) {
  __shared__ float2 s_tgt[TGT_CHUNK];
  __shared__ float2 s_tgn[GATE ? TGT_CHUNK : 1];  // target normals (gate only)
  __shared__ uint16_t s_sorted[TGT_CHUNK];  // target indices grouped by bucket
  __shared__ uint32_t s_start[NB + 1];      // bucket h = s_sorted[s_start[h] .. s_start[h + 1])
  __shared__ uint32_t s_cur[NB];
  __shared__ int32_t s_scan[CT];
  const int b = blockIdx.x, tid = threadIdx.x;
  int32_t s = block_src[b], t = block_tgt[b];
  // (scan ids from device memory: a block with one outside [0, n_scans) is reported and matches nothing -- count 0)
  const bool ids_ok = id_in(s, n_scans) && id_in(t, n_scans);
  if (!ids_ok) {
    if (tid == 0) flag_bad_id(status, BAD_SCAN_ID, id_in(s, n_scans) ? t : s, b);
    s = t = 0;
  }
  const int32_t sb = ids_ok ? offsets[s] : 0, ns = ids_ok ? offsets[s + 1] - sb : 0;
  const int32_t tb = ids_ok ? offsets[t] : 0, nt = ids_ok ? offsets[t + 1] - tb : 0;
  const Aff2f C = mul_f(inverse_f(pose_affine(pose_aff + 4 * (size_t)t)), pose_affine(pose_aff + 4 * (size_t)s));
  float4 *out = corr + 2 * (size_t)cap_offsets[b];
  int32_t written = 0;  // rows already emitted by earlier source passes (uniform)

  const Staged S{s_tgt, s_tgn, s_sorted, s_start, s_cur, s_scan};
  const float inv_cell = inv_cell_of(thr);
  // stage + bucket the whole target cloud once; a point outside the cell limit, or not finite, sends the block to the scan
  const bool hashed = nt <= TGT_CHUNK && thr > 0.f && inv_cell < 3.0e38f &&
                      stage_buckets<TGT_CHUNK / CT, GATE>(S, xy + tb, normals + tb, nt, inv_cell, tid, [](float2) { return true; });

  for (int32_t s0 = 0; s0 < ns; s0 += CT * MAX_PER_LANE) {
    const int32_t n_pass = min(ns - s0, CT * MAX_PER_LANE);
    // lane t owns points s0 + t, s0 + t + CT, ...: consecutive lanes hold consecutive points, so loads
    // and the kept rows of one round are contiguous across the wave
    const int32_t hi = s0 + n_pass;
#define SRC_INDEX(k) (s0 + (k) * CT + tid)
    float qx[MAX_PER_LANE], qy[MAX_PER_LANE], best[MAX_PER_LANE];
    float snx[GATE ? MAX_PER_LANE : 1], sny[GATE ? MAX_PER_LANE : 1];
    int32_t bi[MAX_PER_LANE];
    int big = 0;
#pragma unroll
    for (int k = 0; k < MAX_PER_LANE; k++) {
      bi[k] = -1;
      best[k] = 3.0e38f;
      qx[k] = qy[k] = 0.f;
      if (SRC_INDEX(k) < hi) {
        const float2 p = xy[sb + SRC_INDEX(k)];
        if (GATE) {
          const float2 sn = normals[sb + SRC_INDEX(k)];
          snx[k] = sn.x;
          sny[k] = sn.y;
        }
        qx[k] = __fadd_rn(dot2(C.m00, p.x, C.m01, p.y), C.tx);
        qy[k] = __fadd_rn(dot2(C.m10, p.x, C.m11, p.y), C.ty);
        // (a non-finite query matches nothing on either path; only a huge finite one needs the scan)
        if (fabsf(__fmul_rn(qx[k], inv_cell)) >= CELL_LIMIT || fabsf(__fmul_rn(qy[k], inv_cell)) >= CELL_LIMIT) big = 1;
      }
    }
    const bool scan_all = !hashed || __syncthreads_or(hashed ? big : 0);
    // the normal gate of round k on the target at LDS position i (no gate: every candidate passes)
    auto gate = [&](int k, uint32_t i, float d2) {
      return !GATE || (float_norm_root(d2) < thr && fabsf(dot2(s_tgn[i].x, snx[GATE ? k : 0], s_tgn[i].y, sny[GATE ? k : 0])) > min_cos);
    };
    if (!scan_all) {
#pragma unroll
      for (int k = 0; k < MAX_PER_LANE; k++) {
        if (SRC_INDEX(k) >= hi) continue;
        const float fx = __fmul_rn(qx[k], inv_cell), fy = __fmul_rn(qy[k], inv_cell);
        if (!(fabsf(fx) < CELL_LIMIT) || !(fabsf(fy) < CELL_LIMIT)) continue;  // NaN / inf: no match
        walk_3x3(S, qx[k], qy[k], inv_cell, best[k], bi[k], [&](uint32_t i, float d2) { return gate(k, i, d2); });  // bi[k]: a SLOT
        if (bi[k] >= 0) bi[k] = (int32_t)s_sorted[bi[k]];  // slot -> index of the target point
      }
    } else {
      for (int32_t t0 = 0; t0 < nt; t0 += TGT_CHUNK) {
        const int32_t nc = min(nt - t0, TGT_CHUNK);
        if (!hashed) {  // (a hashed block already holds the whole target cloud in s_tgt)
          __syncthreads();
          for (int32_t i = tid; i < nc; i += CT) {
            s_tgt[i] = xy[tb + t0 + i];
            if (GATE) s_tgn[i] = normals[tb + t0 + i];
          }
          __syncthreads();
        }
        for (int32_t i = 0; i < nc; i++) {
          const float2 g = s_tgt[i];  // same address in every lane: LDS broadcast
          // (a hashed block holds its cloud in bucket order: position i is point s_sorted[i], and ties go by index)
          const int32_t idx = hashed ? (int32_t)s_sorted[i] : t0 + i;
#pragma unroll
          for (int k = 0; k < MAX_PER_LANE; k++)
            consider(g, qx[k], qy[k], idx, best[k], bi[k], [&](float d2) { return gate(k, i, d2); }, true,
                     [](int32_t c, int32_t at) { return (uint32_t)c < (uint32_t)at; });  // (bi[k]: an INDEX here; over -1 any wins)
        }
      }
    }
    // keep = nearest within the threshold (kdtree.cc:253-305 + solver.cc:84-89).  Source order is
    // round-major (round k holds points s0 + k*CT ..): per round a wave ballot gives the in-wave rank,
    // one LDS table of (round, wave) counts and ONE barrier give the rest.
    bool keep[MAX_PER_LANE];
    int32_t rank[MAX_PER_LANE];
    const int lane = tid & 63, wv = tid >> 6;
    __syncthreads();  // s_scan is free again (previous pass / bucket scan)
#pragma unroll
    for (int k = 0; k < MAX_PER_LANE; k++) {
      keep[k] = (SRC_INDEX(k) < hi) && bi[k] >= 0 && (float_norm_root(best[k]) < thr);
      const unsigned long long m = __ballot(keep[k]);
      rank[k] = __builtin_popcountll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_scan[k * (CT / 64) + wv] = __builtin_popcountll(m);
    }
    __syncthreads();
    int32_t pos = written;
#pragma unroll
    for (int k = 0; k < MAX_PER_LANE; k++) {
      int32_t before = 0, round_total = 0;
#pragma unroll
      for (int w = 0; w < CT / 64; w++) {
        const int32_t c = s_scan[k * (CT / 64) + w];
        before += (w < wv) ? c : 0;
        round_total += c;
      }
      if (keep[k]) {
        const int32_t at = pos + before + rank[k];
        const float2 p = xy[sb + SRC_INDEX(k)], ps = normals[sb + SRC_INDEX(k)];
        const float2 g = xy[tb + bi[k]], gn = normals[tb + bi[k]];
        out[2 * (size_t)at] = make_float4(p.x, p.y, g.x, g.y);
        out[2 * (size_t)at + 1] = make_float4(ps.x, ps.y, gn.x, gn.y);
      }
      pos += round_total;
    }
    written = pos;
#undef SRC_INDEX
  }
  if (tid == 0) counts[b] = written;
}

// ---- compaction into the contiguous layout of the residual batch --------------------------
// block_offsets = exclusive scan of counts (one workgroup; n_blocks is ~1e4)
__global__ __launch_bounds__(1024) void corr_scan_kernel(const int32_t *__restrict__ counts,
                                                         int32_t n_blocks,
                                                         int32_t *__restrict__ block_offsets) {
  __shared__ int32_t s[1024];
  __shared__ int32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int32_t base = 0; base < n_blocks; base += 1024) {
    const int32_t i = base + threadIdx.x;
    const int32_t v = i < n_blocks ? counts[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int32_t u = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += u;
      __syncthreads();
    }
    if (i < n_blocks) block_offsets[i] = carry + s[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) block_offsets[n_blocks] = carry;
}

__global__ __launch_bounds__(CT) void corr_compact_kernel(const float4 *__restrict__ padded,
                                                          const int64_t *__restrict__ cap_offsets,
                                                          const int32_t *__restrict__ block_offsets,
                                                          float4 *__restrict__ corr,
                                                          int32_t *__restrict__ corr_block) {
  const int b = blockIdx.x;
  const int32_t o = block_offsets[b], n = block_offsets[b + 1] - o;
  const float4 *src = padded + 2 * (size_t)cap_offsets[b];
  for (int32_t i = threadIdx.x; i < 2 * n; i += CT) corr[2 * (size_t)o + i] = src[i];
  for (int32_t i = threadIdx.x; i < n; i += CT) corr_block[o + i] = b;
}

}  // namespace

int launch_corr_search(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                       const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                       const float *d_pose_aff, float thr, float min_cos, bool gate,
                       const int64_t *d_cap_offsets, float *d_corr_padded, int32_t *d_counts, hipStream_t s) {
  if (n_blocks == 0) return NHIP_OK;
  timer_begin(NHIP_TIMER_CORR, s);
  if (gate)
    hipLaunchKernelGGL(corr_search_kernel<true>, dim3(n_blocks), dim3(CT), 0, s,
                       reinterpret_cast<const float2 *>(d_xy), reinterpret_cast<const float2 *>(d_normals),
                       d_offsets, d_block_src, d_block_tgt, d_pose_aff, thr, min_cos, d_cap_offsets,
                       reinterpret_cast<float4 *>(d_corr_padded), d_counts, n_scans, dev_status());
  else
    hipLaunchKernelGGL(corr_search_kernel<false>, dim3(n_blocks), dim3(CT), 0, s,
                       reinterpret_cast<const float2 *>(d_xy), reinterpret_cast<const float2 *>(d_normals),
                       d_offsets, d_block_src, d_block_tgt, d_pose_aff, thr, 0.f, d_cap_offsets,
                       reinterpret_cast<float4 *>(d_corr_padded), d_counts, n_scans, dev_status());
  timer_end(NHIP_TIMER_CORR, s);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_corr_compact(const float *d_corr_padded, const int64_t *d_cap_offsets,
                        const int32_t *d_counts, int32_t n_blocks, int32_t *d_block_offsets,
                        float *d_corr, int32_t *d_corr_block, hipStream_t s) {
  hipLaunchKernelGGL(corr_scan_kernel, dim3(1), dim3(1024), 0, s, d_counts, n_blocks, d_block_offsets);
  if (n_blocks > 0)
    hipLaunchKernelGGL(corr_compact_kernel, dim3(n_blocks), dim3(CT), 0, s,
                       reinterpret_cast<const float4 *>(d_corr_padded), d_cap_offsets, d_block_offsets,
                       reinterpret_cast<float4 *>(d_corr), d_corr_block);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
