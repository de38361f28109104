// nhip_loss.hip -- odometry-style factors under a robust loss, reduced to their normal equations (DESIGN.md section 3,
// "Robust loss"; K18).  One lane per factor: r (3) and J = [J_i | J_j] (3 x 6) exactly as resid_odometry_kernel forms them
// (nhip_resid.hip), s = r0 r0 + r1 r1 + r2 r2 (products rounded, added in that order), the loss' rho(s) and rho'(s), and
// Ceres' first-order correction (Corrector with alpha = 0, which is the branch it takes for every loss with rho'' <= 0):
// w = sqrt(rho'), r~ = w r, J~ = w J, every entry one rounded product.  The row is the 28 doubles of the other *_normal_eq
// kernels formed from r~ and J~ in resid_odometry_normal_eq_kernel's order -- except slot 27, which holds rho(s), so that
// half the sum of the slots 27 is the robust cost.  Compiled with -ffp-contract=off like its neighbours.
//
// The loss (kind, scale a, b = a a as one rounded product), in this operation order (nautilus_amd/loss.py restates it):
//   NONE      rho = s                        rho' = 1
//   HUBER     s <= b: rho = s, rho' = 1      else q = sqrt(s): rho = ((2 a) q) - b, rho' = a / q
//   SOFT_L1   x = s / b, q = sqrt(1 + x):    rho = (2 s) / (q + 1), rho' = 1 / q
//   CAUCHY    x = s / b:                     rho = x < 2^-54 ? s : b log1p(x), rho' = 1 / (1 + x)
// SOFT_L1's rho is 2 b (sqrt(1 + x) - 1) with the difference written as x / (sqrt(1 + x) + 1): the same function, without
// the cancellation that returns 0 for every s below 2^-53 b.  CAUCHY takes log1p in place of log(1 + x) for the same
// reason, and below x = 2^-54 the series' first term, b x = s, which is b log1p(x) to within 2^-55 of itself: evaluated on the
// device, b log1p(s / b) came back 0 for the smallest subnormal s (tests/test_loss_gpu.py found it), and a subnormal quotient
// has no relative accuracy to hand on.  These choices are build-defined (Ceres writes the plain forms).
//
// Two forms of the row store, the same bytes from either:
//   direct   every lane writes its 28 doubles, lanes 224 bytes apart, as the plain kernel does;
//   staged   the workgroup's rows -- one contiguous span of 256 x 224 bytes -- go through LDS (a lane's row 29 doubles apart:
//            the pad keeps the 8-byte writes of a wave off each other's banks) and leave as whole lines, consecutive lanes
//            writing consecutive doubles.
// The staged form ships: at 100,000 factors it takes 0.67-0.70 of the direct form's time, at 1,000 the two are equal within
// their spread (tools/loss_bench.py).  A process with NHIP_TUNABLES=1 picks either with
// NHIP_LOSS_STORE=direct|staged.
#include "nhip_loss_shared.h"  // loss_value, and the row's shape: shared with nhip_relpose.hip

namespace nhip {
namespace {

constexpr int LT = LOSS_LT, ROW = LOSS_ROW, ROW_PITCH = LOSS_ROW_PITCH;

// the factor's row into o[0 .. 27] (o: registers, or the lane's row in LDS) and its four weights; false: a pose index is
// outside [0, n_poses) -- reported, and the caller writes zeros
__device__ __forceinline__ bool robust_row(const float2 *__restrict__ t_odom, const float *__restrict__ r_odom,
                                           const int32_t *__restrict__ pose_i, const int32_t *__restrict__ pose_j, int32_t f,
                                           double tw, double rw, int32_t kind, double a, const double *__restrict__ poses,
                                           int32_t n_poses, uint32_t *__restrict__ status, double *o, double *wt) {
  const int32_t ii = pose_i[f], ij = pose_j[f];
  if (!id_in(ii, n_poses) || !id_in(ij, n_poses)) {
    flag_bad_id(status, BAD_POSE_ID, id_in(ii, n_poses) ? ij : ii, f);
    return false;
  }
  const double *pi = poses + 3 * (size_t)ii;
  const double *pj = poses + 3 * (size_t)ij;
  const float2 t = t_odom[f];
  const double ex = pi[0] + (double)t.x - pj[0];
  const double ey = pi[1] + (double)t.y - pj[1];
  const double d = pi[2] + (double)r_odom[f] - pj[2];
  const double sd = sin(d), cd = cos(d);
  const double r0[3] = {tw * ex, tw * ey, rw * atan2(sd, cd)};
  const double g = rw * ((sd * sd + cd * cd) / (cd * cd + sd * sd));
  const double s = r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2];
  const LossValue L = loss_value(kind, a, s);
  const double w = sqrt(L.rho1);  // (NONE, and HUBER's inliers: exactly 1, and the products below are their factors)
  const double r[3] = {w * r0[0], w * r0[1], w * r0[2]};
  const double wtw = w * tw, wg = w * g, z = w * 0.0, mtw = w * -tw, mg = w * -g;
  const double J[3][6] = {{wtw, z, z, mtw, z, z}, {z, wtw, z, z, mtw, z}, {z, z, wg, z, z, mg}};
  int k = 0;
#pragma unroll
  for (int p = 0; p < 6; p++)
#pragma unroll
    for (int q = p; q < 6; q++) o[k++] = J[0][p] * J[0][q] + J[1][p] * J[1][q] + J[2][p] * J[2][q];
#pragma unroll
  for (int p = 0; p < 6; p++) o[21 + p] = J[0][p] * r[0] + J[1][p] * r[1] + J[2][p] * r[2];
  o[27] = L.rho;
  wt[0] = s, wt[1] = L.rho, wt[2] = L.rho1, wt[3] = w;
  return true;
}

template <bool STAGED>
__global__ __launch_bounds__(LT) void resid_odometry_robust_normal_eq_kernel(
    const float2 *__restrict__ t_odom, const float *__restrict__ r_odom, const int32_t *__restrict__ pose_i,
    const int32_t *__restrict__ pose_j, int32_t n, double tw, double rw, int32_t kind, double a,
    const double *__restrict__ poses, double *__restrict__ out, double *__restrict__ weights, int32_t n_poses,
    uint32_t *__restrict__ status) {
  const int32_t f0 = blockIdx.x * LT, f = f0 + threadIdx.x;
  double wt[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (STAGED) {
    __shared__ double s_rows[LT * ROW_PITCH];
    if (f < n) {
      double *o = s_rows + ROW_PITCH * threadIdx.x;
      if (!robust_row(t_odom, r_odom, pose_i, pose_j, f, tw, rw, kind, a, poses, n_poses, status, o, wt))
        for (int q = 0; q < ROW; q++) o[q] = 0.0;
    }
    __syncthreads();
    // the rows of this workgroup's factors that exist (the last workgroup may be partial): element e of the span is slot
    // e % 28 of row e / 28
    const int32_t count = (n - f0 < LT ? n - f0 : LT) * ROW;
    double *span = out + (size_t)f0 * ROW;
    for (int32_t e = threadIdx.x; e < count; e += LT) span[e] = s_rows[e + e / ROW];
  } else if (f < n) {
    double o[ROW];
    if (!robust_row(t_odom, r_odom, pose_i, pose_j, f, tw, rw, kind, a, poses, n_poses, status, o, wt))
      for (int q = 0; q < ROW; q++) o[q] = 0.0;
    double *dst = out + (size_t)f * ROW;
#pragma unroll
    for (int q = 0; q < ROW; q++) dst[q] = o[q];
  }
  if (weights && f < n) {
    double *dst = weights + 4 * (size_t)f;
    dst[0] = wt[0], dst[1] = wt[1], dst[2] = wt[2], dst[3] = wt[3];
  }
}

// the form that ships; NHIP_LOSS_STORE (a process with NHIP_TUNABLES=1 only) picks one by name
constexpr bool STAGED_BY_DEFAULT = true;
bool staged_store() {
  const char *v = tunable("NHIP_LOSS_STORE");
  if (v && !strcmp(v, "staged")) return true;
  if (v && !strcmp(v, "direct")) return false;
  return STAGED_BY_DEFAULT;
}

}  // namespace

int launch_resid_odometry_robust_normal_eq(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                                           const int32_t *d_pose_j, int32_t n_factors, double tw, double rw, int32_t kind,
                                           double scale, const double *d_poses, int32_t n_poses, double *d_out,
                                           double *d_weights, hipStream_t s) {
  NHIP_REQUIRE(n_factors >= 0 && n_poses >= 0, "resid_odometry_robust_normal_eq: negative size");
  if (n_factors == 0) return NHIP_OK;
  const dim3 grid((n_factors + LT - 1) / LT), block(LT);
  const float2 *t = reinterpret_cast<const float2 *>(d_t_odom);
  if (staged_store())
    hipLaunchKernelGGL(resid_odometry_robust_normal_eq_kernel<true>, grid, block, 0, s, t, d_r_odom, d_pose_i, d_pose_j, n_factors,
                       tw, rw, kind, scale, d_poses, d_out, d_weights, n_poses, dev_status());
  else
    hipLaunchKernelGGL(resid_odometry_robust_normal_eq_kernel<false>, grid, block, 0, s, t, d_r_odom, d_pose_i, d_pose_j, n_factors,
                       tw, rw, kind, scale, d_poses, d_out, d_weights, n_poses, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
