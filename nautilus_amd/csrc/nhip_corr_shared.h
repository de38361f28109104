// nhip_corr_shared.h -- the bucketed nearest-neighbour search that the correspondence search (nhip_corr.hip, K5) and the match
// refinement (nhip_refine.hip, K22) share: exact nearest neighbour of a query among the points of one target cloud, ties to
// the lowest index.  A workgroup of CT threads stages the cloud in LDS IN THE ORDER OF ITS BUCKETS (stage_buckets: a uniform
// grid of cells a shade wider than the threshold, counting sort on NB hashed buckets) and every lane visits the 3 x 3 cells
// around its query (walk_3x3): a target within the threshold lies in one of them, and so does the global nearest neighbour
// whenever any target is within it, so what a caller keeps under `sqrt(d2) < thr` equals an exhaustive scan's.  A cloud or a
// query whose cell coordinates leave the exact float range takes that scan instead, candidate by candidate through the same
// compare (consider).  The arrays are the caller's (Staged): K5 keeps normals only under its gate and re-stages clouds longer
// than a stage chunk by chunk; K22 holds more beside them.  Units that include this are compiled with -ffp-contract=off.
#pragma once
#include "nhip_common.h"

namespace nhip {
namespace corr {

constexpr int CT = 256;   // threads of a workgroup
constexpr int NB = 1024;  // hash buckets of the target grid, in groups of four
// float cell coordinates are exact enough below it (inv_cell_of); a point or a query at or beyond it takes the exhaustive scan
constexpr float CELL_LIMIT = 4096.0f;

// Cells 0.1 % wider than the threshold: two points closer than thr are less than 0.999 cells apart per axis.  A
// float cell coordinate fx = g * inv_cell carries a relative error of ~1.2e-7 (inv_cell and the product are each
// rounded), so the computed coordinates of such a pair differ by less than 0.999 + 2.4e-7 |fx|: below 1 -- the
// pair lands in the same or in adjacent cells and the 3 x 3 visit finds it -- as long as |fx| < 4166.
// Larger coordinates (beyond 4096 cells = 1 km at the 0.25 m threshold) take the exhaustive scan.
__device__ __forceinline__ float inv_cell_of(float thr) { return __fdiv_rn(1.0f, __fmul_rn(thr, 1.001f)); }

__device__ __forceinline__ float dot2(float a, float b, float c, float d) {
  return __fadd_rn(__fmul_rn(a, b), __fmul_rn(c, d));
}

// Buckets come in groups of four: the cells (4g .. 4g + 3, cy) of a row occupy four CONSECUTIVE buckets (the group is
// hashed, the cell's place in it is cx & 3), so the three cells cx - 1 .. cx + 1 a query visits in a row are one run of
// consecutive buckets -- or two, when they straddle a group -- instead of three separate ones: 4.5 bucket ranges per
// point instead of 9, each with its hash, its two dependent LDS reads and its short loop (the walk is bound by that
// per-range overhead: tools/corr_phase_probe.py).  Cells that share a bucket only add candidates the distance test drops.
__device__ __forceinline__ uint32_t group_hash(int32_t gx, int32_t cy) {
  return ((((uint32_t)gx * 73856093u) ^ ((uint32_t)cy * 19349663u)) & (uint32_t)(NB / 4 - 1)) << 2;
}
__device__ __forceinline__ uint32_t cell_hash(int32_t cx, int32_t cy) {
  return group_hash(cx >> 2, cy) | ((uint32_t)cx & 3u);
}

// block-wide inclusive scan of one int per thread: wave scans by shuffles, wave totals through LDS
// (s_scan: at least CT / 64 ints), two barriers
__device__ __forceinline__ int32_t block_scan_incl(int32_t v, int32_t *s_scan, int tid) {
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  __syncthreads();  // s_scan may still be read by the previous user
  if (lane == 63) s_scan[wv] = v;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < CT / 64; w++) v += (w < wv) ? s_scan[w] : 0;
  return v;
}

// a target cloud in LDS: the caller's arrays (its LDS footprint stays its own)
struct Staged {
  float2 *tgt;       // the points, in bucket order once stage_buckets has returned true
  float2 *tgn;       // their normals (callers that keep none never read it)
  uint16_t *sorted;  // slot -> index of the point in its cloud
  uint32_t *start;   // NB + 1: bucket h = slots [start[h], start[h + 1])
  uint32_t *cur;     // NB
  int32_t *scan;     // CT
};

// Stages the cloud xy[0 .. nt), nt <= TPL * CT, in bucket order: counted, scanned, scattered; true when it is (a barrier
// has then made it visible; start[NB] points are staged).  A point that `keep` refuses is left out.  False, with nothing
// staged, when a kept point's cell coordinate is at or beyond CELL_LIMIT or not finite.  Uniform; every thread calls.
template <int TPL, bool NORMALS, class Keep>
__device__ __forceinline__ bool stage_buckets(const Staged &S, const float2 *__restrict__ xy,
                                              const float2 *__restrict__ normals, int32_t nt, float inv_cell, int tid,
                                              Keep keep) {
  int big = 0;
  for (int32_t i = tid; i < NB; i += CT) S.start[i] = 0u;
  __syncthreads();
  // (all of a thread's points -- up to TPL -- are requested before the first is used)
  {
    float2 tg[TPL];
#pragma unroll
    for (int k = 0; k < TPL; k++) {
      const int32_t i = tid + k * CT;
      if (i < nt) tg[k] = xy[i];
    }
#pragma unroll
    for (int k = 0; k < TPL; k++) {
      const int32_t i = tid + k * CT;
      if (i >= nt || !keep(tg[k])) continue;
      const float fx = __fmul_rn(tg[k].x, inv_cell), fy = __fmul_rn(tg[k].y, inv_cell);
      if (!(fabsf(fx) < CELL_LIMIT) || !(fabsf(fy) < CELL_LIMIT)) big = 1;
      else atomicAdd(&S.start[cell_hash((int32_t)floorf(fx), (int32_t)floorf(fy))], 1u);
    }
  }
  if (__syncthreads_or(big)) return false;
  // exclusive scan of the NB bucket counts (NB / CT per thread), then scatter
  uint32_t c[NB / CT], tot = 0;
#pragma unroll
  for (int k = 0; k < NB / CT; k++) {
    c[k] = S.start[tid * (NB / CT) + k];
    tot += c[k];
  }
  uint32_t run = (uint32_t)block_scan_incl((int32_t)tot, S.scan, tid) - tot;
#pragma unroll
  for (int k = 0; k < NB / CT; k++) {
    S.start[tid * (NB / CT) + k] = run;
    S.cur[tid * (NB / CT) + k] = run;
    run += c[k];
  }
  if (tid == CT - 1) S.start[NB] = run;
  __syncthreads();
  // The points themselves go to LDS IN BUCKET ORDER (tgt[slot], tgn[slot]; sorted[slot] = the point's index): the walk
  // then reads a bucket's points at consecutive addresses, with no index to fetch and follow first.  (Read again from
  // global memory -- the L2 has them -- rather than held in registers across the scan: 16 more registers would cost
  // K5 its fifth wave per SIMD.)
  float2 tg[TPL], tn[NORMALS ? TPL : 1];
#pragma unroll
  for (int k = 0; k < TPL; k++) {
    const int32_t i = tid + k * CT;
    if (i < nt) {
      tg[k] = xy[i];
      if (NORMALS) tn[NORMALS ? k : 0] = normals[i];
    }
  }
#pragma unroll
  for (int k = 0; k < TPL; k++) {
    const int32_t i = tid + k * CT;
    if (i >= nt || !keep(tg[k])) continue;
    const float2 g = tg[k];
    const uint32_t h = cell_hash((int32_t)floorf(__fmul_rn(g.x, inv_cell)), (int32_t)floorf(__fmul_rn(g.y, inv_cell)));
    const uint32_t slot = atomicAdd(&S.cur[h], 1u);
    S.tgt[slot] = g;
    if (NORMALS) S.tgn[slot] = tn[NORMALS ? k : 0];
    S.sorted[slot] = (uint16_t)i;
  }
  __syncthreads();
  return true;
}

// One candidate g, named `cand`, against the best so far of the query (qx, qy): (best, at), at < 0 while there is none.
// accept(d2) may refuse it.  The order of visits is arbitrary: (d2, index) lexicographic = "the lowest index wins ties".
// Only on an exact tie of the squared distances, and only where the caller lets a tie count (where `at` names a slot there
// is no index to fetch while there is none: at >= 0), before(cand, at) is asked whether cand's index is the lower one.
// (ONE condition guards the fetch: with the caller's test nested inside the tie's branch K22 measured 6.00 ms against 5.78.)
template <class Accept, class Before>
__device__ __forceinline__ void consider(const float2 g, float qx, float qy, int32_t cand, float &best, int32_t &at,
                                         Accept accept, bool tie_counts, Before before) {
  const float dx = __fsub_rn(g.x, qx), dy = __fsub_rn(g.y, qy);
  const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
  const bool ok = accept(d2);
  bool better = ok && d2 < best;
  if (ok && d2 == best && tie_counts) better = before(cand, at);
  best = better ? d2 : best;
  at = better ? cand : at;
}

// consider() for a candidate and a best so far that are SLOTS of a staged cloud: their indices are fetched only on a tie
template <class Accept>
__device__ __forceinline__ void consider_slot(const Staged &S, int32_t slot, float qx, float qy, float &best, int32_t &at,
                                              Accept accept) {
  consider(S.tgt[slot], qx, qy, slot, best, at, accept, at >= 0,
           [&S](int32_t cand, int32_t a) { return S.sorted[cand] < S.sorted[a]; });
}

// The 3 x 3 cells around the query (qx, qy) of a bucketed cloud, its cell coordinates below CELL_LIMIT: (best, at) is
// updated with the nearest staged point that accept(slot, d2) does not refuse; `at` is its SLOT.
template <class Accept>
__device__ __forceinline__ void walk_3x3(const Staged &S, float qx, float qy, float inv_cell, float &best, int32_t &at,
                                         Accept accept) {
  const int32_t icx = (int32_t)floorf(__fmul_rn(qx, inv_cell)), icy = (int32_t)floorf(__fmul_rn(qy, inv_cell));
  const int32_t lo = icx - 1, hi2 = icx + 1;
  const bool two = (lo >> 2) != (hi2 >> 2);  // the three cells straddle a group of four
  for (int32_t oy = -1; oy <= 1; oy++)
    for (int32_t r = 0; r < 2; r++) {
      if (r == 1 && !two) break;
      // first run: from cell lo to cell hi2 or the end of lo's group; second run: the cells of hi2's group
      const uint32_t b0 = r == 0 ? cell_hash(lo, icy + oy) : group_hash(hi2 >> 2, icy + oy);
      const uint32_t b1 = r == 0 ? (two ? (b0 | 3u) : b0 + 2u) : b0 + ((uint32_t)hi2 & 3u);
      const uint32_t e = S.start[b1 + 1];
      for (uint32_t i = S.start[b0]; i < e; i++)  // (bucket order: consecutive addresses)
        consider_slot(S, (int32_t)i, qx, qy, best, at, [&](float d2) { return accept(i, d2); });
    }
}

}  // namespace corr
}  // namespace nhip
