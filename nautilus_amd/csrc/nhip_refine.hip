// nhip_refine.hip -- K22: match refinement on gfx950: point-to-line ICP from the lattice pose of every match record.
//
// The rule is DESIGN.md section 3, "Match refinement"; tests/refine_reference.py restates it point by point and this kernel
// equals it bit for bit.  One workgroup of 256 threads per pair, resident for all of the pair's iterations:
//   * the target scan's points and normals are staged in LDS once, in the order of their buckets (the counting sort on
//     hashed cell groups of nhip_corr_shared.h, cells a shade wider than thr[0]): 2048 points, 44 KB, three workgroups per CU;
//   * a lane owns the source points i = lane (mod 256), at most 8 per pass of 2048, in registers across the iterations
//     when the scan is one pass long; longer scans read their points again per pass, the lane sums carry on;
//   * an evaluation at a pose: float transform, exact nearest target (ties to the lowest index), the acceptance test of the
//     correspondence search against this iteration's threshold, then H, g, the cost and the count in double, every lane
//     adding its points in ascending order; the 256 lane sums go through an xor butterfly (1 .. 32 inside the wave, then
//     (w0 + w1) + (w2 + w3) through LDS), which gives every lane the same bits;
//   * the 3 x 3 solve, the update and every decision run redundantly on every lane from those sums: the iteration loop is
//     uniform, nothing is atomically accumulated, no trigonometry, exp or log runs here.
// Target points that are not finite or lie at 1e6 m or beyond are never staged; the same source points are never queried.
// A target whose cell coordinates leave the exact float range (4096 cells), or a pose that takes a query there, is
// searched exhaustively over the staged points: same nearest neighbour.  The search is nhip_corr_shared.h's, shared with the
// correspondence search (nhip_corr.hip): this unit adds which points take part (point_ok) and what is summed over the matches.
#include "nhip_corr_shared.h"

namespace nhip {

namespace {

using namespace corr;

constexpr int TGT_MAX = NHIP_REFINE_TARGET_MAX;
constexpr int PER_LANE = 8;            // source points a lane owns per pass
constexpr int PASS = CT * PER_LANE;    // 2048
constexpr int NSUM = 10;               // H00 H01 H02 H11 H12 H22 g0 g1 g2 cost
constexpr float COORD_LIMIT = 1.0e6f;  // a point at or beyond it (or not finite) never matches

__device__ __forceinline__ bool point_ok(const float2 p) { return fabsf(p.x) < COORD_LIMIT && fabsf(p.y) < COORD_LIMIT; }

struct RefineLds {
  float2 tgt[TGT_MAX];         // the target's points, bucket order (plain order when not hashed; NaN: never matches)
  float2 tgn[TGT_MAX];         // their normals
  uint16_t sorted[TGT_MAX];    // slot -> index of the point in its scan
  uint32_t start[NB + 1];      // bucket h = slots [start[h], start[h + 1])
  uint32_t cur[NB];
  int32_t scan[CT];
  double red[CT / 64][NSUM];   // wave sums
  int32_t red_n[CT / 64];
  double trace[NHIP_REFINE_TRACE_DOUBLES];
  __device__ __forceinline__ Staged staged() { return {tgt, tgn, sorted, start, cur, scan}; }
};

struct Sums {
  double v[NSUM];
  int32_t n;
};

// one evaluation at (c, s, tx, ty) under the threshold thr: uniform result on every lane
__device__ __forceinline__ Sums evaluate(RefineLds &L, const float2 *__restrict__ src, int32_t ns, float (&px)[PER_LANE],
                                         float (&py)[PER_LANE], double c, double s, double tx, double ty, float thr,
                                         float inv_cell, bool hashed, int32_t n_staged, int tid) {
  const float cf = (float)c, sf = (float)s, txf = (float)tx, tyf = (float)ty;
  const Staged T = L.staged();
  double acc[NSUM];
#pragma unroll
  for (int j = 0; j < NSUM; j++) acc[j] = 0.0;
  int32_t cnt = 0;
  for (int32_t s0 = 0; s0 < ns; s0 += PASS) {
    if (ns > PASS) {  // (a scan of one pass keeps its points in registers across the iterations)
#pragma unroll
      for (int k = 0; k < PER_LANE; k++) {
        const int32_t i = s0 + k * CT + tid;
        float2 p = make_float2(NAN, NAN);
        if (i < ns) p = src[i];
        if (!point_ok(p)) p = make_float2(NAN, NAN);
        px[k] = p.x, py[k] = p.y;
      }
    }
    float qx[PER_LANE], qy[PER_LANE], best[PER_LANE];
    int32_t bs[PER_LANE];  // the SLOT of the best so far
    int big = 0;
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
      best[k] = 3.0e38f;
      bs[k] = -1;
      qx[k] = __fadd_rn(dot2(cf, px[k], -sf, py[k]), txf);
      qy[k] = __fadd_rn(dot2(sf, px[k], cf, py[k]), tyf);
      if (px[k] == px[k] && (fabsf(__fmul_rn(qx[k], inv_cell)) >= CELL_LIMIT || fabsf(__fmul_rn(qy[k], inv_cell)) >= CELL_LIMIT)) big = 1;
    }
    const bool scan_all = !hashed || __syncthreads_or(big);
    if (!scan_all) {
#pragma unroll
      for (int k = 0; k < PER_LANE; k++) {
        if (!(px[k] == px[k])) continue;  // (no point, or one that never matches)
        walk_3x3(T, qx[k], qy[k], inv_cell, best[k], bs[k], [](uint32_t, float) { return true; });
      }
    } else {
      for (int32_t i = 0; i < n_staged; i++) {  // (the same slot in every lane: LDS broadcast)
#pragma unroll
        for (int k = 0; k < PER_LANE; k++) consider_slot(T, i, qx[k], qy[k], best[k], bs[k], [](float) { return true; });
      }
    }
    // a lane adds its points in ascending order
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
      if (bs[k] < 0 || !(float_norm_root(best[k]) < thr)) continue;
      const float2 g = L.tgt[bs[k]], gn = L.tgn[bs[k]];
      if (!(fabsf(gn.x) < INFINITY) || !(fabsf(gn.y) < INFINITY)) continue;  // the target's normal is not finite
      const double nx = (double)gn.x, ny = (double)gn.y, dpx = (double)px[k], dpy = (double)py[k];
      const double ex = (double)qx[k] - (double)g.x, ey = (double)qy[k] - (double)g.y;
      const double r = nx * ex + ny * ey;
      const double a = -(s * dpx) - c * dpy, bb = c * dpx - s * dpy;
      const double jt = nx * a + ny * bb;
      acc[0] = acc[0] + nx * nx;
      acc[1] = acc[1] + nx * ny;
      acc[2] = acc[2] + nx * jt;
      acc[3] = acc[3] + ny * ny;
      acc[4] = acc[4] + ny * jt;
      acc[5] = acc[5] + jt * jt;
      acc[6] = acc[6] + nx * r;
      acc[7] = acc[7] + ny * r;
      acc[8] = acc[8] + jt * r;
      acc[9] = acc[9] + r * r;
      cnt++;
    }
  }
  // adjacent-pair halving, eight levels: an xor butterfly gives the same tree on every lane
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int j = 0; j < NSUM; j++) acc[j] = acc[j] + __shfl_xor(acc[j], m, 64);
    cnt += __shfl_xor(cnt, m, 64);
  }
  const int lane = tid & 63, wv = tid >> 6;
  __syncthreads();  // (the previous evaluation's readers are done)
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NSUM; j++) L.red[wv][j] = acc[j];
    L.red_n[wv] = cnt;
  }
  __syncthreads();
  Sums S;
#pragma unroll
  for (int j = 0; j < NSUM; j++) S.v[j] = (L.red[0][j] + L.red[1][j]) + (L.red[2][j] + L.red[3][j]);
  S.n = (L.red_n[0] + L.red_n[1]) + (L.red_n[2] + L.red_n[3]);
  return S;
}

__global__ __launch_bounds__(CT) void refine_icp_kernel(const RefineParams P) {
  __shared__ RefineLds L;
  const int b = blockIdx.x, tid = threadIdx.x;
  const nhip_refine_spec_t &sp = P.spec;
  const double c0 = P.pose0[4 * (size_t)b], s0p = P.pose0[4 * (size_t)b + 1], tx0 = P.pose0[4 * (size_t)b + 2],
               ty0 = P.pose0[4 * (size_t)b + 3];
  nhip_refined_t R;
  R.c = c0, R.s = s0p, R.tx = tx0, R.ty = ty0;
#pragma unroll
  for (int j = 0; j < 6; j++) R.info[j] = 0.0;
  R.cost = 0.0;
  R.n_corr = 0, R.iterations = 0, R.flags = 0u, R.pad = 0u;
  if (tid < NHIP_REFINE_TRACE_DOUBLES) L.trace[tid] = 0.0;

  int32_t s = P.pair_src[b], t = P.pair_tgt[b];
  const bool ids_ok = id_in(s, P.n_scans) && id_in(t, P.n_scans);
  if (!ids_ok && tid == 0) flag_bad_id(P.status, BAD_REFINE_ID, id_in(s, P.n_scans) ? t : s, b);
  if (!ids_ok) s = t = 0;
  const int32_t sb = ids_ok ? P.offsets[s] : 0, ns = ids_ok ? P.offsets[s + 1] - sb : 0;
  const int32_t tb = ids_ok ? P.offsets[t] : 0, nt = ids_ok ? P.offsets[t + 1] - tb : 0;

  const bool start_ok = isfinite(c0) && isfinite(s0p) && isfinite(tx0) && isfinite(ty0);
  if (!start_ok) {
    R.c = R.s = R.tx = R.ty = NAN;
    R.flags = NHIP_REFINE_SKIPPED;
  } else if (nt > TGT_MAX) {
    R.flags = NHIP_REFINE_TARGET_TOO_LONG;
  }
  if (R.flags != 0u) {  // (uniform: decided from the pair's own words)
    if (tid == 0) P.out[b] = R;
    if (P.trace && tid < NHIP_REFINE_TRACE_DOUBLES) P.trace[(size_t)b * NHIP_REFINE_TRACE_DOUBLES + tid] = 0.0;
    return;
  }

  // ---- the target, once: counted, scanned, scattered in bucket order ----
  // (points that fail point_ok are left out; a valid one beyond the cell limit leaves the cloud in plain order, NaN for the
  // left-out ones, and every search exhaustive)
  const float inv_cell = inv_cell_of(sp.thr[0]);
  constexpr int TPL = TGT_MAX / CT;
  const bool hashed = stage_buckets<TPL, true>(L.staged(), P.xy + tb, P.normals + tb, nt, inv_cell, tid, [](float2 p) { return point_ok(p); });
  const int32_t n_staged = hashed ? (int32_t)L.start[NB] : nt;
  if (!hashed) {
#pragma unroll
    for (int k = 0; k < TPL; k++) {
      const int32_t i = tid + k * CT;
      if (i >= nt) continue;
      const float2 g = P.xy[tb + i];
      L.tgt[i] = point_ok(g) ? g : make_float2(NAN, NAN);
      L.tgn[i] = P.normals[tb + i];
      L.sorted[i] = (uint16_t)i;
    }
    __syncthreads();
  }

  // ---- the source's first pass: in registers for every iteration when it is the only one ----
  const float2 *src = P.xy + sb;
  float px[PER_LANE], py[PER_LANE];
#pragma unroll
  for (int k = 0; k < PER_LANE; k++) {
    const int32_t i = k * CT + tid;
    float2 p = make_float2(NAN, NAN);
    if (i < ns) p = src[i];
    if (!point_ok(p)) p = make_float2(NAN, NAN);
    px[k] = p.x, py[k] = p.y;
  }

  double c = c0, sn = s0p, tx = tx0, ty = ty0;
  const int32_t max_it = sp.max_iterations;
  uint32_t flags = 0u;
  int32_t it = 0;
  bool converged = false;
  while (it < max_it) {
    const Sums E = evaluate(L, src, ns, px, py, c, sn, tx, ty, sp.thr[it], inv_cell, hashed, n_staged, tid);
    // every lane holds the same sums: the decisions below are uniform (readfirstlane tells the compiler so)
    uint32_t stop = 0u;
    double dx = 0.0, dy = 0.0, dth = 0.0;
    if (E.n < sp.min_corr) {
      stop = NHIP_REFINE_FEW;
    } else {
      const double H00 = E.v[0], H01 = E.v[1], H02 = E.v[2], H11 = E.v[3], H12 = E.v[4], H22 = E.v[5];
      const double hm = (H00 + H11) * 0.5, hd = (H00 - H11) * 0.5;
      const double lam = hm - sqrt(hd * hd + H01 * H01);
      const double d0 = H00;
      const double l10 = H01 / d0, l20 = H02 / d0;
      const double d1 = H11 - l10 * H01;
      const double u = H12 - l20 * H01;
      const double l21 = u / d1;
      const double d2 = (H22 - l20 * H02) - l21 * u;
      if (!(lam / (double)E.n >= sp.min_spread) || !(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) {
        stop = NHIP_REFINE_SINGULAR;
      } else {
        const double y0 = -E.v[6];
        const double y1 = -E.v[7] - l10 * y0;
        const double y2 = (-E.v[8] - l20 * y0) - l21 * y1;
        dth = y2 / d2;
        dy = y1 / d1 - l21 * dth;
        dx = (y0 / d0 - l10 * dy) - l20 * dth;
        tx = tx + dx;
        ty = ty + dy;
        const double hu = dth * 0.5, u2 = hu * hu;
        const double den = 1.0 + u2;
        const double cd = (1.0 - u2) / den, sd = (2.0 * hu) / den;
        const double cn = c * cd - sn * sd, snn = sn * cd + c * sd;
        c = cn, sn = snn;
        const double mx = tx - tx0, my = ty - ty0;
        if (!(sqrt(mx * mx + my * my) <= sp.max_shift_m) || !(fabs(sn * c0 - c * s0p) <= sp.max_turn_sin)) stop = NHIP_REFINE_RUNAWAY;
      }
    }
    stop = (uint32_t)__builtin_amdgcn_readfirstlane((int)stop);
    if (stop != 0u) {
      flags = stop;
      break;
    }
    if (tid == 0) {
      L.trace[4 * it] = c, L.trace[4 * it + 1] = sn, L.trace[4 * it + 2] = tx, L.trace[4 * it + 3] = ty;
    }
    it++;
    const int done = (sqrt(dx * dx + dy * dy) < sp.step_tol_m && fabs(dth) < sp.step_tol_rad) ? 1 : 0;
    if (__builtin_amdgcn_readfirstlane(done)) {
      converged = true;
      break;
    }
  }
  if (flags == 0u) {
    if (!converged) flags = NHIP_REFINE_NOT_CONVERGED;
    const Sums E = evaluate(L, src, ns, px, py, c, sn, tx, ty, sp.thr[max_it - 1], inv_cell, hashed, n_staged, tid);
    const int few = __builtin_amdgcn_readfirstlane(E.n < sp.min_corr ? 1 : 0);
    if (few) {
      flags = NHIP_REFINE_FEW;
    } else {
      R.c = c, R.s = sn, R.tx = tx, R.ty = ty;
#pragma unroll
      for (int j = 0; j < 6; j++) R.info[j] = E.v[j];
      R.cost = E.v[9];
      R.n_corr = E.n;
    }
  }
  R.iterations = it;
  R.flags = flags;
  if (tid == 0) P.out[b] = R;
  __syncthreads();  // (lane 0's trace entries)
  if (P.trace && tid < NHIP_REFINE_TRACE_DOUBLES) P.trace[(size_t)b * NHIP_REFINE_TRACE_DOUBLES + tid] = L.trace[tid];
}

}  // namespace

int launch_refine_icp(const RefineParams &P, hipStream_t s) {
  if (P.n_pairs == 0) return NHIP_OK;
  hipLaunchKernelGGL(refine_icp_kernel, dim3(P.n_pairs), dim3(CT), 0, s, P);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
