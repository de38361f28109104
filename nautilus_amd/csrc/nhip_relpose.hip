// nhip_relpose.hip -- relative-pose factors ("Relative-pose factors"; K23).  Factor f couples the poses
// a = pose_i[f] (the target scan's) and b = pose_j[f] (the source's) with a measurement z = (z_x, z_y, c_z, s_z) -- b in a's
// frame, K22's (tx, ty, c, s) -- and an information Lambda = (L00 L01 L02 L11 L12 L22) over (x, y, theta).  One lane per
// factor, all in double, every product and sum rounded on its own (-ffp-contract=off), sums in the order written:
//   trig    (c_a, s_a), (c_b, s_b) = cos / sin of the headings;  D = t_b - t_a;
//           d_x = c_a D_x + s_a D_y,  d_y = (-s_a) D_x + c_a D_y;  c_r = c_a c_b + s_a s_b,  s_r = c_a s_b - s_a c_b;
//           c_e = c_r c_z + s_r s_z,  s_e = s_r c_z - c_r s_z
//   error   e = (d_x - z_x, d_y - z_y, atan2(s_e, c_e))
//   E       row 0 (-c_a, -s_a, d_y, c_a, s_a, 0), row 1 (s_a, -c_a, -d_x, -s_a, c_a, 0), row 2 (0, 0, -1, 0, 0, 1)
//   W       D0 = L00, l10 = L01 / D0, l20 = L02 / D0, D1 = L11 - l10 L01, u = L12 - l20 L01, l21 = u / D1,
//           D2 = (L22 - l20 L02) - l21 u;  q_k = sqrt(D_k);  W = [q0, q0 l10, q0 l20; 0, q1, q1 l21; 0, 0, q2]: W^T W = Lambda
//   r, J    r_k = sum_{m >= k} W_km e_m,  J_kp = sum_{m >= k} W_km E_mp, ascending m, every term formed
//   row     s = r0 r0 + r1 r1 + r2 r2, the loss of nhip_loss_shared.h (loss_value_pinned: CAUCHY's log1p written out in IEEE
//           operations, so that rho is the host form's in every bit), w = sqrt(rho'), r~ = w r, J~ = w J, and the 28 doubles
//           of resid_odometry_normal_eq_kernel's order with rho(s) in slot 27
// Flags, one int32 per factor, any of them a zero row and zero weights: 1 an entry of Lambda not finite or a pivot not > 0,
// 2 an entry of z not finite, 4 pose_i == pose_j.  A pose id outside [0, n_poses) is never dereferenced: zeros, and reported
// through the status words (BAD_POSE_ID).
//
// No array is indexed at run time: every loop below has a compile-time trip count and is unrolled, so the factor lives in
// registers (the code object's metadata: no private segment, no spilled VGPR -- DESIGN.md section 5, K23).  The rows leave as
// nhip_loss.hip's do: through LDS, a lane's row 29 doubles apart, consecutive lanes writing consecutive doubles of the
// workgroup's contiguous span.  A process with NHIP_TUNABLES=1 picks the form with NHIP_RELPOSE_STORE=direct|staged
// (tools/relpose_bench.py times both); the bytes are the same.
#include "nhip_loss_shared.h"

namespace nhip {
namespace {

constexpr int LT = LOSS_LT, ROW = LOSS_ROW, ROW_PITCH = LOSS_ROW_PITCH;

struct RelposeFactor {
  double r[3];     // the whitened residual
  double J[3][6];  // ... and its Jacobian over [a | b]
  double ca, sa, cb, sb, e[3];
};

__device__ __forceinline__ bool finite4(double a, double b, double c, double d) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

// the flags of factor f, and -- if it has none and both ids are in range -- the factor itself; false: nothing to write but zeros
__device__ __forceinline__ bool relpose_factor(const double *__restrict__ z, const double *__restrict__ info,
                                               const int32_t *__restrict__ pose_i, const int32_t *__restrict__ pose_j, int32_t f,
                                               const double *__restrict__ poses, int32_t n_poses, uint32_t *__restrict__ status,
                                               RelposeFactor &F, int32_t &flags) {
  const int32_t ia = pose_i[f], ib = pose_j[f];
  const double *zf = z + 4 * (size_t)f, *lf = info + 6 * (size_t)f;
  const double zx = zf[0], zy = zf[1], cz = zf[2], sz = zf[3];
  const double L00 = lf[0], L01 = lf[1], L02 = lf[2], L11 = lf[3], L12 = lf[4], L22 = lf[5];
  // the square-root-free Cholesky of K22's solve
  const double D0 = L00;
  const double l10 = L01 / D0, l20 = L02 / D0;
  const double D1 = L11 - l10 * L01;
  const double u = L12 - l20 * L01;
  const double l21 = u / D1;
  const double D2 = (L22 - l20 * L02) - l21 * u;
  flags = 0;
  if (!(finite4(L00, L01, L02, L11) && isfinite(L12) && isfinite(L22)) || !(D0 > 0.0) || !(D1 > 0.0) || !(D2 > 0.0))
    flags |= NHIP_RELPOSE_BAD_INFO;
  if (!finite4(zx, zy, cz, sz)) flags |= NHIP_RELPOSE_BAD_MEASUREMENT;
  if (ia == ib) flags |= NHIP_RELPOSE_SAME_POSE;
  if (!id_in(ia, n_poses) || !id_in(ib, n_poses)) {
    flag_bad_id(status, BAD_POSE_ID, id_in(ia, n_poses) ? ib : ia, f);
    return false;
  }
  if (flags) return false;
  const double *pa = poses + 3 * (size_t)ia, *pb = poses + 3 * (size_t)ib;
  double sa, ca, sb, cb;
  sincos(pa[2], &sa, &ca);
  sincos(pb[2], &sb, &cb);
  const double Dx = pb[0] - pa[0], Dy = pb[1] - pa[1];
  const double dx = ca * Dx + sa * Dy, dy = (-sa) * Dx + ca * Dy;
  const double cr = ca * cb + sa * sb, sr = ca * sb - sa * cb;
  const double ce = cr * cz + sr * sz, se = sr * cz - cr * sz;
  const double e[3] = {dx - zx, dy - zy, atan2(se, ce)};
  const double E[3][6] = {{-ca, -sa, dy, ca, sa, 0.0}, {sa, -ca, -dx, -sa, ca, 0.0}, {0.0, 0.0, -1.0, 0.0, 0.0, 1.0}};
  const double q0 = sqrt(D0), q1 = sqrt(D1), q2 = sqrt(D2);
  const double W00 = q0, W01 = q0 * l10, W02 = q0 * l20, W11 = q1, W12 = q1 * l21, W22 = q2;
  F.r[0] = W00 * e[0] + W01 * e[1] + W02 * e[2];
  F.r[1] = W11 * e[1] + W12 * e[2];
  F.r[2] = W22 * e[2];
#pragma unroll
  for (int p = 0; p < 6; p++) {
    F.J[0][p] = W00 * E[0][p] + W01 * E[1][p] + W02 * E[2][p];
    F.J[1][p] = W11 * E[1][p] + W12 * E[2][p];
    F.J[2][p] = W22 * E[2][p];
  }
  F.ca = ca, F.sa = sa, F.cb = cb, F.sb = sb;
  F.e[0] = e[0], F.e[1] = e[1], F.e[2] = e[2];
  return true;
}

__global__ __launch_bounds__(LT) void resid_relpose_kernel(const double *__restrict__ z, const double *__restrict__ info,
                                                           const int32_t *__restrict__ pose_i, const int32_t *__restrict__ pose_j,
                                                           int32_t n, const double *__restrict__ poses, int32_t n_poses,
                                                           double *__restrict__ residuals, double *__restrict__ jac_i,
                                                           double *__restrict__ jac_j, double *__restrict__ parts,
                                                           int32_t *__restrict__ flags_out, uint32_t *__restrict__ status) {
  const int32_t f = blockIdx.x * LT + threadIdx.x;
  if (f >= n) return;
  RelposeFactor F;
  int32_t flags;
  const bool ok = relpose_factor(z, info, pose_i, pose_j, f, poses, n_poses, status, F, flags);
  double *res = residuals + 3 * (size_t)f;
#pragma unroll
  for (int k = 0; k < 3; k++) res[k] = ok ? F.r[k] : 0.0;
  if (jac_i) {
    double *dst = jac_i + 9 * (size_t)f;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int p = 0; p < 3; p++) dst[3 * k + p] = ok ? F.J[k][p] : 0.0;
  }
  if (jac_j) {
    double *dst = jac_j + 9 * (size_t)f;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int p = 0; p < 3; p++) dst[3 * k + p] = ok ? F.J[k][3 + p] : 0.0;
  }
  if (parts) {
    double *dst = parts + 8 * (size_t)f;
    dst[0] = ok ? F.ca : 0.0, dst[1] = ok ? F.sa : 0.0, dst[2] = ok ? F.cb : 0.0, dst[3] = ok ? F.sb : 0.0;
    dst[4] = ok ? F.e[0] : 0.0, dst[5] = ok ? F.e[1] : 0.0, dst[6] = ok ? F.e[2] : 0.0, dst[7] = 0.0;
  }
  if (flags_out) flags_out[f] = flags;
}

// the factor's row into o[0 .. 27] (o: registers, or the lane's row in LDS) and its four weights; false: zeros are the caller's
__device__ __forceinline__ bool relpose_row(const double *__restrict__ z, const double *__restrict__ info,
                                            const int32_t *__restrict__ pose_i, const int32_t *__restrict__ pose_j, int32_t f,
                                            int32_t kind, double a, const double *__restrict__ poses, int32_t n_poses,
                                            uint32_t *__restrict__ status, double *o, double *wt, int32_t &flags) {
  RelposeFactor F;
  if (!relpose_factor(z, info, pose_i, pose_j, f, poses, n_poses, status, F, flags)) return false;
  const double s = F.r[0] * F.r[0] + F.r[1] * F.r[1] + F.r[2] * F.r[2];
  const LossValue L = loss_value_pinned(kind, a, s);  // (CAUCHY: log1p in IEEE operations, the host form's bits)
  const double w = sqrt(L.rho1);  // (NONE, and HUBER's inliers: exactly 1, and the products below are their factors)
  const double r[3] = {w * F.r[0], w * F.r[1], w * F.r[2]};
  double J[3][6];
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int p = 0; p < 6; p++) J[k][p] = w * F.J[k][p];
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
__global__ __launch_bounds__(LT) void resid_relpose_normal_eq_kernel(
    const double *__restrict__ z, const double *__restrict__ info, const int32_t *__restrict__ pose_i,
    const int32_t *__restrict__ pose_j, int32_t n, int32_t kind, double a, const double *__restrict__ poses, int32_t n_poses,
    double *__restrict__ out, double *__restrict__ weights, int32_t *__restrict__ flags_out, uint32_t *__restrict__ status) {
  const int32_t f0 = blockIdx.x * LT, f = f0 + threadIdx.x;
  double wt[4] = {0.0, 0.0, 0.0, 0.0};
  int32_t flags = 0;
  if constexpr (STAGED) {
    __shared__ double s_rows[LT * ROW_PITCH];
    if (f < n) {
      double *o = s_rows + ROW_PITCH * threadIdx.x;
      if (!relpose_row(z, info, pose_i, pose_j, f, kind, a, poses, n_poses, status, o, wt, flags))
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
    const bool ok = relpose_row(z, info, pose_i, pose_j, f, kind, a, poses, n_poses, status, o, wt, flags);
    double *dst = out + (size_t)f * ROW;
#pragma unroll
    for (int q = 0; q < ROW; q++) dst[q] = ok ? o[q] : 0.0;
  }
  if (f < n) {
    if (weights) {
      double *dst = weights + 4 * (size_t)f;
      dst[0] = wt[0], dst[1] = wt[1], dst[2] = wt[2], dst[3] = wt[3];
    }
    if (flags_out) flags_out[f] = flags;
  }
}

// the form that ships; NHIP_RELPOSE_STORE (a process with NHIP_TUNABLES=1 only) picks one by name
constexpr bool STAGED_BY_DEFAULT = true;
bool staged_store() {
  const char *v = tunable("NHIP_RELPOSE_STORE");
  if (v && !strcmp(v, "staged")) return true;
  if (v && !strcmp(v, "direct")) return false;
  return STAGED_BY_DEFAULT;
}

}  // namespace

int launch_resid_relpose(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                         int32_t n_factors, const double *d_poses, int32_t n_poses, double *d_residuals, double *d_jac_i,
                         double *d_jac_j, double *d_parts, int32_t *d_flags, hipStream_t s) {
  NHIP_REQUIRE(n_factors >= 0 && n_poses >= 0, "resid_relpose: negative size");
  if (n_factors == 0) return NHIP_OK;
  hipLaunchKernelGGL(resid_relpose_kernel, dim3((n_factors + LT - 1) / LT), dim3(LT), 0, s, d_z, d_info, d_pose_i, d_pose_j,
                     n_factors, d_poses, n_poses, d_residuals, d_jac_i, d_jac_j, d_parts, d_flags, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_resid_relpose_normal_eq(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                                   int32_t n_factors, int32_t kind, double scale, const double *d_poses, int32_t n_poses,
                                   double *d_out, double *d_weights, int32_t *d_flags, hipStream_t s) {
  NHIP_REQUIRE(n_factors >= 0 && n_poses >= 0, "resid_relpose_normal_eq: negative size");
  if (n_factors == 0) return NHIP_OK;
  const dim3 grid((n_factors + LT - 1) / LT), block(LT);
  if (staged_store())
    hipLaunchKernelGGL(resid_relpose_normal_eq_kernel<true>, grid, block, 0, s, d_z, d_info, d_pose_i, d_pose_j, n_factors, kind,
                       scale, d_poses, n_poses, d_out, d_weights, d_flags, dev_status());
  else
    hipLaunchKernelGGL(resid_relpose_normal_eq_kernel<false>, grid, block, 0, s, d_z, d_info, d_pose_i, d_pose_j, n_factors, kind,
                       scale, d_poses, n_poses, d_out, d_weights, d_flags, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
