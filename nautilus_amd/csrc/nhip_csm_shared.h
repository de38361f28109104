// nhip_csm_shared.h -- what the kernels that perform every add of the (theta, x, y) correlation share with each other
// (the strip kernels of nhip_csm_strip.h, csm_small_plane_kernel) and with the kernels that turn keys into records
// (nhip_csm_score.hip): the score gate, the parameter block, a point's window cell, the rotation, the key.
#pragma once
#include "nhip_common.h"

namespace nhip {

// ---- the score gate of nhip_csm_match_gated -------------------------------------------
// A record is kept when (double)score >= min_score; otherwise it is the rejected record {-1, -1, -1, -inf}, sum -1.
// For a scan of n points, every pose whose sum is below
//     floor(n) = max(0, floor(n * ((min_score - Lf) / step - 1)))
// scores below min_score: its quantised score is more than one step below it, and its exact score (NHIP_SEARCH_EXACT_SCORE)
// at most half a step above the quantised one.  Branch and bound starts its best there and prunes every block whose
// bound is below it; the host helper nhip_csm_gate_floor and the kernels evaluate this one expression.
struct ScoreGate {
  double min_score;  // -INFINITY: the gate is off (floor 0 for every scan, every record kept)
  double Lf, step;   // the grids' floor score and quantisation step (GridLayout)
};
__host__ __device__ inline int32_t gate_floor(const ScoreGate &G, int32_t n_pts) {
  if (n_pts <= 0) return 0;
  const double f = floor((double)n_pts * ((G.min_score - G.Lf) / G.step - 1.0));
  if (!(f > 0.0)) return 0;                                   // (min_score -INFINITY, or at most Lf + step)
  return f >= 2147483647.0 ? 0x7fffffff : (int32_t)f;       // (above every sum an int32 holds: every pose is rejected)
}
// The best key a search starts from: below every pose of sum >= floor, above every pose of a smaller sum.  Floor 0 and 1
// give key0 = pose 0 with sum 0, where an ungated search starts.
__host__ __device__ inline unsigned long long gate_floor_key(int32_t floor_sum) {
  return floor_sum <= 0 ? 0xffffffffull : ((unsigned long long)(uint32_t)(floor_sum - 1) << 32) | 0xffffffffull;
}
// The one decision "rejected": a sum below the floor (what branch and bound leaves behind for a pair it gave up on), or a
// record score below min_score.  `score` = +INFINITY when the score is decided later (the exact-score pass).
__host__ __device__ inline bool gate_rejects(const ScoreGate &G, uint32_t sum, int32_t n_pts, float score) {
  return (int64_t)sum < (int64_t)gate_floor(G, n_pts) || (double)score < G.min_score;
}
__host__ __device__ inline nhip_match_t gate_rejected_record() {
  nhip_match_t m;
  m.itheta = m.ix = m.iy = -1;
  m.score = -INFINITY;
  return m;
}

// A key is (sum << 32) | ~lin with lin = (itheta * nx + ix) * ny + iy, so that the maximum key is the largest sum at the
// smallest linear index.  The indices of the record a key stands for:
__device__ __forceinline__ void decode_key(unsigned long long key, int32_t nx, int32_t ny, nhip_match_t &m) {
  const uint32_t lin = 0xffffffffu - (uint32_t)key;
  m.iy = (int32_t)(lin % (uint32_t)ny);
  m.ix = (int32_t)((lin / (uint32_t)ny) % (uint32_t)nx);
  m.itheta = (int32_t)(lin / ((uint32_t)ny * (uint32_t)nx));
}

inline ScoreGate job_gate(const MatchJob &job) { return {job.min_score, job.L->Lf, job.L->step}; }

// ---- what the kernels' parameter blocks share (CsmParams below, bnb::BnbParams, ExactParams of nhip_csm_score.hip), from a job:
// the fields have one name in all three.  What differs per kernel -- keys, the blocks of the plane, the dense rule, the
// plan's fields -- its launcher sets after these.
// What all three hold (the block is zeroed first): the scans, the grids, the per-pair arrays and their counts, the plane
// of translations, what places a point's window in a slot
template <class Params>
void fill_job_common(Params &P, const MatchJob &job) {
  memset(&P, 0, sizeof(P));
  P.xy = reinterpret_cast<const float2 *>(job.xy);
  P.offsets = job.offsets;
  P.grids = job.grids;
  P.pair_src = job.pair_src;
  P.pair_slot = job.pair_slot;
  P.ids = job.ids;
  P.rot0_cs = job.rot0_cs;
  P.delta_cs = job.delta_cs;
  P.pair_origin = job.pair_origin;
  P.n_pairs = job.n_pairs;
  P.nx = job.search->nx;
  P.ny = job.search->ny;
  P.hx = (job.search->nx - 1) / 2;
  P.hy = (job.search->ny - 1) / 2;
  P.S = job.L->S;
  P.max_shift = job.spec->max_shift;
  P.slot_bytes = job.L->slot_bytes;
  P.res = job.spec->res;
  P.inv_res = 1.0 / job.spec->res;
}
// ... and what the kernels that search add: the rotations and the stored image's geometry
template <class Params>
void fill_job_params(Params &P, const MatchJob &job) {
  fill_job_common(P, job);
  P.n_theta = job.search->n_theta;
  P.pad = job.L->pad;
  P.pitch = job.L->pitch;
  P.rows = job.L->S + 2 * job.L->pad;
  P.grid_bytes = job.L->grid_bytes;
}

namespace csm {

struct CsmParams {
  const float2 *xy;
  const int32_t *offsets;
  const uint8_t *grids;
  const int32_t *pair_src;
  const int32_t *pair_slot;
  const double *rot0_cs;
  const double *delta_cs;
  const int32_t *pair_origin;  // optional (x, y) cell offset of each pair's search centre
  unsigned long long *keys;
  int32_t *volume;  // full score volume (scores kernel only)
  int32_t n_pairs, n_theta, nx, ny, hx, hy, npbx, npby;
  int32_t S, pad, pitch, rows, max_shift;
  int32_t single_src, single_slot;  // scores kernel: the one pair
  int32_t single_ox, single_oy;
  int32_t dense;  // 1: ignore the skip maps (every strip is added, zero or not)
  int32_t tile_rows, n_tiles;  // csm_small_plane_kernel: rows of the plane of translations per workgroup, workgroups per rotation
  IdBounds ids;   // counts the pairs' scan ids and grid slots are checked against (nhip_common.h)
  int64_t grid_bytes, slot_bytes;
  double res, inv_res;
};

// The strip kernels of one cell width (nhip_csm_strip.h), as their launchers take them (nhip_csm_plan.hip)
struct StripKernels {
  void (*match[2])(CsmParams);   // the keys of a list of pairs; [1]: DENSE
  void (*scores[2])(CsmParams);  // the score volume of one pair (VOLUME); [1]: DENSE
  int32_t threads;               // per workgroup
  int32_t pb_nx, pb_ny;          // translations per plane block
};
const StripKernels &strip_kernels8();   // nhip_csm.hip
const StripKernels &strip_kernels16();  // nhip_csm16.hip

// Stored-grid coordinates (row, col) of the top-left cell of point q's window under rotation
// (cf, sf), packed (row << 16) | col.  Spec: rotate in float with individually rounded
// products (Eigen Affine2f * Vector2f on baseline x86-64: no FMA), cell = S/2 +
// floor(double(v) / res) (cimg_debug.h:31-37).  Cells are clamped to [-h-1, S+h]: beyond that
// range every lookup of the window falls on the zero border, and so does the clamped window.
__device__ __forceinline__ uint32_t window_cell(float2 q, float cf, float sf, const CsmParams &P,
                                                int32_t ox, int32_t oy, int32_t cx, int32_t cy) {
  const float xr = __fsub_rn(__fmul_rn(cf, q.x), __fmul_rn(sf, q.y));
  const float yr = __fadd_rn(__fmul_rn(sf, q.x), __fmul_rn(cf, q.y));
  long col = -P.hx - 1, row = -P.hy - 1;  // non-finite points score nothing
  if ((fabsf(xr) < 1e9f) && (fabsf(yr) < 1e9f)) {
    const long half = P.S / 2;
    col = half + (long)floor_quotient((double)xr, P.res, P.inv_res) + cx;
    row = half + (long)floor_quotient((double)yr, P.res, P.inv_res) + cy;
    col = col < -P.hx - 1 ? -P.hx - 1 : (col > P.S + P.hx ? P.S + P.hx : col);
    row = row < -P.hy - 1 ? -P.hy - 1 : (row > P.S + P.hy ? P.S + P.hy : row);
  }
  const uint32_t pcol = (uint32_t)(col - P.hx + ox + P.pad);
  const uint32_t prow = (uint32_t)(row - P.hy + oy + P.pad);
  return (prow << 16) | pcol;
}

// Rotation k of a pair: R(theta0) * R(delta_k), composed in double with individually rounded ops.  (cos, sin) of theta0
// is entry `pair` of rot0_cs, of delta_k entry k of delta_cs.
__device__ __forceinline__ void compose_rotation(const double *rot0_cs, const double *delta_cs, int32_t pair, int32_t k,
                                                 float &cf, float &sf) {
  const double c0 = rot0_cs[2 * pair], s0 = rot0_cs[2 * pair + 1];
  const double cd = delta_cs[2 * k], sd = delta_cs[2 * k + 1];
  cf = __double2float_rn(__dsub_rn(__dmul_rn(c0, cd), __dmul_rn(s0, sd)));
  sf = __double2float_rn(__dadd_rn(__dmul_rn(s0, cd), __dmul_rn(c0, sd)));
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  lo = __shfl_xor(lo, m, 64);
  hi = __shfl_xor(hi, m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// K3: argmax with deterministic tie-break (smallest linear index wins).  `best` is the largest of the lane's keys
// (sum << 32) | ~lin; the wave's largest goes to the pair's key.
__device__ __forceinline__ unsigned long long pose_key(uint32_t sum, uint32_t lin) {
  return ((unsigned long long)sum << 32) | (0xffffffffu - lin);
}
__device__ __forceinline__ void wave_max_to_key(unsigned long long best, int lane, unsigned long long *key) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = shfl_xor_u64(best, m);
    best = o > best ? o : best;
  }
  if (lane == 0) atomicMax(key, best);
}

// Where to put point j inside a fresh tile: ahead of the direction the beam sweep is moving.
__device__ __forceinline__ int32_t place(int32_t here, int32_t ahead, int32_t span) {
  const int32_t d = ahead - here;
  const int32_t off = d > 2 ? span / 8 : (d < -2 ? span - span / 8 : span / 2);
  const int32_t a = here - off;
  return a < 0 ? 0 : a;
}

}  // namespace csm
}  // namespace nhip
