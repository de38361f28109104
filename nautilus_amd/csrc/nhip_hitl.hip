// nhip_hitl.hip -- K8: the point selection of a human-in-the-loop constraint, GetRelevantPosesForHITL
// (src/optimization/solver.cc:479-513) for every scan at once: which points of which nodes lie on the user's line a, which
// on line b, and the packed blocks AddHITLResiduals (solver.cc:515-532) builds its PointToLineResidual blocks from.
// The spec is DESIGN.md section 8, "HITL on the device".
//
//   hitl_classify_kernel  one scan per workgroup, lanes are points.  A point goes to the world under its node's pose as an
//                         Affine2f (float, every operation rounded on its own), then DistanceToLineSegment<float>
//                         (slam_util.h:92-110) against line a and, if it is not on a, against line b; the float distance is
//                         compared AS A DOUBLE with the double line width (CONFIG_DOUBLE hitl_line_width), which rejects
//                         d == float(0.05) (0.05f > 0.05).  A class byte per point (0 none, 1 a, 2 b), the scan's two counts
//                         from wave ballots.
//   hitl_offsets_kernel   the membership of every scan (count_a >= threshold: an a-node with its a-points; else count_b >=
//                         threshold: a b-node with its b-points), the exclusive scans that give every node its block id --
//                         all a-nodes in node order, then all b-nodes -- and the offset of its first point, the totals.
//   hitl_pack_kernel      one workgroup per selected scan: stable compaction of its points of the node's class by ballot and
//                         popcount prefix into the packed arrays nhip_resid_point_to_line_normal_eq_dev takes.
//
// Non-finite points fail every comparison and belong to no class.  The square roots are sqrtf, which this file is compiled
// to round correctly (a bare v_sqrt_f32 is an ulp off); nothing here may be contracted into an fma (Makefile:
// -ffp-contract=off, and the pragma below).
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int HT = 256;  // threads of a workgroup

struct HitlLine {
  float x0, y0, x1, y1, nx, ny, off;  // the ends; Hyperplane::Through(start, end): unit normal and offset
};
struct HitlParams {
  HitlLine a, b;
  double width;
  int32_t threshold;
};

__device__ __forceinline__ bool between_f(float v, float a, float b) {  // IsBetween, slam_util.h:87-89 (closed)
  return (v >= a && v <= b) || (v >= b && v <= a);
}

// DistanceToLineSegment<float> of the world point (wx, wy); NaN wherever the reference's floats give NaN
__device__ __forceinline__ float hitl_distance(float wx, float wy, const HitlLine &L) {
  const float sd = __fadd_rn(__fadd_rn(__fmul_rn(wx, L.nx), __fmul_rn(wy, L.ny)), L.off);
  const float prx = __fsub_rn(wx, __fmul_rn(sd, L.nx)), pry = __fsub_rn(wy, __fmul_rn(sd, L.ny));
  if (between_f(prx, L.x0, L.x1) && between_f(pry, L.y0, L.y1)) return fabsf(sd);
  const float ax = __fsub_rn(wx, L.x0), ay = __fsub_rn(wy, L.y0), bx = __fsub_rn(wx, L.x1), by = __fsub_rn(wy, L.y1);
  const float d0 = sqrtf(__fadd_rn(__fmul_rn(ax, ax), __fmul_rn(ay, ay)));
  const float d1 = sqrtf(__fadd_rn(__fmul_rn(bx, bx), __fmul_rn(by, by)));
  float m = d1 < d0 ? d1 : d0;  // the smaller; NaN if either is
  if (d1 != d1) m = d1;
  return m;
}

__global__ __launch_bounds__(HT) void hitl_classify_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ offsets,
                                                           const float4 *__restrict__ pose_f32, const HitlParams P,
                                                           uint8_t *__restrict__ cls, int32_t *__restrict__ counts) {
  __shared__ int32_t s_cnt[HT / 64][2];
  const int32_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t beg = offsets[s];
  int32_t n = offsets[s + 1] - beg;
  if (n < 0) n = 0;
  const float4 T = pose_f32[s];  // cos, sin, x, y: PoseArrayToAffine(...).cast<float>()
  int32_t ca = 0, cb = 0;        // of this wave (uniform)
  for (int64_t base = 0; base < n; base += HT) {
    const int64_t i = base + tid;
    uint32_t k = 0;
    if (i < n) {
      const float2 p = xy[(size_t)beg + i];
      const float wx = __fadd_rn(__fsub_rn(__fmul_rn(T.x, p.x), __fmul_rn(T.y, p.y)), T.z);
      const float wy = __fadd_rn(__fadd_rn(__fmul_rn(T.y, p.x), __fmul_rn(T.x, p.y)), T.w);
      if ((double)hitl_distance(wx, wy, P.a) <= P.width) k = 1;
      else if ((double)hitl_distance(wx, wy, P.b) <= P.width) k = 2;  // (a point on a is not tested against b, solver.cc:497-503)
      cls[(size_t)beg + i] = (uint8_t)k;
    }
    ca += __builtin_popcountll(__ballot(k == 1));
    cb += __builtin_popcountll(__ballot(k == 2));
  }
  if (lane == 0) {
    s_cnt[wv][0] = ca;
    s_cnt[wv][1] = cb;
  }
  __syncthreads();
  if (tid < 2) {
    int32_t v = 0;
#pragma unroll
    for (int w = 0; w < HT / 64; w++) v += s_cnt[w][tid];
    counts[2 * (size_t)s + tid] = v;
  }
}

// One workgroup, 1024 scans per step.  scan_block[s]: the block of scan s, -1 for a scan that joins neither line;
// scan_offset[s]: the index of its first packed point; totals = {n_a, n_b, n_points}.
__global__ __launch_bounds__(1024) void hitl_offsets_kernel(const int32_t *__restrict__ counts, int32_t n_scans, int32_t threshold,
                                                            int32_t *__restrict__ scan_block, int32_t *__restrict__ scan_offset,
                                                            int32_t *__restrict__ totals) {
  __shared__ int32_t sc[4][1024];  // inclusive scans of: a-nodes, b-nodes, points of a-nodes, points of b-nodes
  __shared__ int32_t carry[4];
  const int t = threadIdx.x;
  if (t < 4) carry[t] = 0;
  __syncthreads();
  for (int32_t base = 0; base < n_scans; base += 1024) {
    const int32_t s = base + t;
    int32_t v[4] = {0, 0, 0, 0};
    int m = 0;
    if (s < n_scans) {
      const int32_t ca = counts[2 * (size_t)s], cb = counts[2 * (size_t)s + 1];
      m = ca >= threshold ? 1 : (cb >= threshold ? 2 : 0);
      if (m == 1) { v[0] = 1; v[2] = ca; }
      if (m == 2) { v[1] = 1; v[3] = cb; }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) sc[q][t] = v[q];
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      int32_t u[4];
#pragma unroll
      for (int q = 0; q < 4; q++) u[q] = t >= off ? sc[q][t - off] : 0;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; q++) sc[q][t] += u[q];
      __syncthreads();
    }
    if (s < n_scans) {
      // (a b-node's rank among the b-nodes as -2 - rank until the number of a-nodes is known: the second pass)
      scan_block[s] = m == 1 ? carry[0] + sc[0][t] - 1 : (m == 2 ? -2 - (carry[1] + sc[1][t] - 1) : -1);
      scan_offset[s] = m == 1 ? carry[2] + sc[2][t] - v[2] : (m == 2 ? carry[3] + sc[3][t] - v[3] : 0);
    }
    __syncthreads();
    if (t < 4) carry[t] += sc[t][1023];
    __syncthreads();
  }
  const int32_t n_a = carry[0], pts_a = carry[2];
  for (int32_t s = t; s < n_scans; s += 1024) {  // (scan s was written by this thread)
    const int32_t blk = scan_block[s];
    if (blk <= -2) {
      scan_block[s] = n_a + (-2 - blk);
      scan_offset[s] += pts_a;
    }
  }
  if (t == 0) {
    totals[0] = n_a;
    totals[1] = carry[1];
    totals[2] = pts_a + carry[3];
  }
}

// One workgroup per scan.  The outputs were sized by the caller from the totals it downloaded: n_blocks and n_points must be
// those totals, every block and every point offset is checked against them before it becomes an address (reported once).
__global__ __launch_bounds__(HT) void hitl_pack_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ offsets,
                                                       int32_t n_scans, const uint8_t *__restrict__ cls,
                                                       const int32_t *__restrict__ counts, const int32_t *__restrict__ scan_block,
                                                       const int32_t *__restrict__ scan_offset, const int32_t *__restrict__ totals,
                                                       int32_t n_blocks, int32_t n_points, float2 *__restrict__ points,
                                                       int32_t *__restrict__ block_offsets, int32_t *__restrict__ block_pose,
                                                       uint32_t *__restrict__ status) {
  __shared__ int32_t s_w[2][HT / 64];
  const int32_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t n_a = totals[0], n_b = totals[1];
  const bool fits = n_a >= 0 && n_b >= 0 && n_a + n_b == n_blocks && totals[2] == n_points;
  if (s == 0 && tid == 0) {
    if (fits) block_offsets[n_blocks] = n_points;
    else flag_bad_id(status, BAD_BLOCK_ID, n_blocks, 0);
  }
  if (!fits || s >= n_scans) return;
  const int32_t blk = scan_block[s];
  if (blk == -1) return;
  const uint32_t want = blk < n_a ? 1u : 2u;
  const int32_t cnt = counts[2 * (size_t)s + (want - 1u)], o = scan_offset[s];
  if (!id_in(blk, n_blocks) || cnt < 0 || o < 0 || o > n_points - cnt) {
    if (tid == 0) flag_bad_id(status, BAD_BLOCK_ID, blk, s);
    return;
  }
  if (tid == 0) {
    block_offsets[blk] = o;
    block_pose[blk] = s;
  }
  const int32_t beg = offsets[s];
  int32_t n = offsets[s + 1] - beg;
  if (n < 0) n = 0;
  int32_t done = 0;  // points of this scan packed by the chunks before (uniform)
  int par = 0;
  for (int64_t base = 0; base < n; base += HT, par ^= 1) {
    const int64_t i = base + tid;
    const bool keep = i < n && cls[(size_t)beg + i] == want;
    const unsigned long long m = __ballot(keep);
    // rows alternate by chunk: a wave writes chunk c + 2's only after the barrier of chunk c + 1, which every wave passes
    // after reading chunk c's
    if (lane == 0) s_w[par][wv] = __builtin_popcountll(m);
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < HT / 64; w++) {
      const int32_t c = s_w[par][w];
      if (w < wv) before += c;
      all += c;
    }
    const int32_t pos = done + before + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (keep && pos < cnt) points[(size_t)o + pos] = xy[(size_t)beg + i];
    done += all;
  }
}

}  // namespace

int launch_hitl_select(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const float *d_pose_f32,
                       const nhip_hitl_spec_t &spec, uint8_t *d_class, int32_t *d_counts, int32_t *d_scan_block,
                       int32_t *d_scan_offset, int32_t *d_totals, hipStream_t s) {
  // Hyperplane<float, 2>::Through(start, end) on the host, in float, one rounding per operation (this unit is compiled
  // without contraction): normal = unitOrthogonal(end - start), offset = -normal . start
  auto line = [](const float *l) {
    HitlLine L;
    L.x0 = l[0]; L.y0 = l[1]; L.x1 = l[2]; L.y1 = l[3];
    const float dx = L.x1 - L.x0, dy = L.y1 - L.y0;
    float nx = -dy, ny = dx;
    const float xx = nx * nx, yy = ny * ny;
    const float ln = sqrtf(xx + yy);
    nx = nx / ln;
    ny = ny / ln;
    const float ox = L.x0 * nx, oy = L.y0 * ny;
    L.nx = nx; L.ny = ny;
    L.off = -(ox + oy);
    return L;
  };
  HitlParams P;
  P.a = line(spec.line_a);
  P.b = line(spec.line_b);
  P.width = spec.line_width;
  P.threshold = spec.point_threshold;
  if (n_scans > 0)
    hipLaunchKernelGGL(hitl_classify_kernel, dim3((uint32_t)n_scans), dim3(HT), 0, s, reinterpret_cast<const float2 *>(d_xy), d_offsets,
                       reinterpret_cast<const float4 *>(d_pose_f32), P, d_class, d_counts);
  hipLaunchKernelGGL(hitl_offsets_kernel, dim3(1), dim3(1024), 0, s, d_counts, n_scans, P.threshold, d_scan_block, d_scan_offset,
                     d_totals);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_hitl_pack(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_class, const int32_t *d_counts,
                     const int32_t *d_scan_block, const int32_t *d_scan_offset, const int32_t *d_totals, int32_t n_blocks,
                     int32_t n_points, float *d_points, int32_t *d_block_offsets, int32_t *d_block_pose, hipStream_t s) {
  hipLaunchKernelGGL(hitl_pack_kernel, dim3((uint32_t)(n_scans > 0 ? n_scans : 1)), dim3(HT), 0, s,
                     reinterpret_cast<const float2 *>(d_xy), d_offsets, n_scans, d_class, d_counts, d_scan_block, d_scan_offset, d_totals,
                     n_blocks, n_points, reinterpret_cast<float2 *>(d_points), d_block_offsets, d_block_pose, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
