// nhip_loss_shared.h -- what the kernels that put factors under a robust loss have in common (nhip_loss.hip: odometry-style
// factors, K18; nhip_relpose.hip: relative-pose factors, K23): the loss itself and the shape of a row and of its staged store.
// The operation order of loss_value is nhip_loss.hip's header and nautilus_amd/loss.py; units that include this are compiled
// with -ffp-contract=off.
#pragma once
#include "nhip_common.h"

namespace nhip {

constexpr int LOSS_LT = 256;        // lanes per workgroup
constexpr int LOSS_ROW = 28;        // doubles per row
constexpr int LOSS_ROW_PITCH = 29;  // ... and per row in LDS: the pad keeps the 8-byte writes of a wave off each other's banks

#ifdef __HIPCC__
struct LossValue {
  double rho, rho1;
};

// kind and a are wave-uniform: one branch for the whole wave
__device__ __forceinline__ LossValue loss_value(int32_t kind, double a, double s) {
  const double b = a * a;
  switch (kind) {
    case NHIP_LOSS_HUBER: {
      if (s <= b) return {s, 1.0};
      const double q = sqrt(s);
      return {(2.0 * a) * q - b, a / q};
    }
    case NHIP_LOSS_SOFT_L1: {
      const double x = s / b;
      const double q = sqrt(1.0 + x);
      return {(2.0 * s) / (q + 1.0), 1.0 / q};
    }
    case NHIP_LOSS_CAUCHY: {
      const double x = s / b;
      return {x < 0x1p-54 ? s : b * log1p(x), 1.0 / (1.0 + x)};
    }
    default:
      return {s, 1.0};
  }
}

// log1p(x) for x >= 0 written out in IEEE operations -- fdlibm's s_log1p.c, its branches for x >= 0: additions, products,
// quotients and moves of the exponent field only, every one rounded on its own, so the same doubles come out of any IEEE machine
// (nautilus_amd/loss.py: log1p_pinned restates it in numpy, bit for bit).  Its error stays below 1 ulp.  The device library's
// log1p and numpy's differ from each other in the last bit on a few values in a hundred; K18 keeps the library's.
__host__ __device__ inline int32_t f64_hi(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof(b));
  return (int32_t)(b >> 32);
}
__host__ __device__ inline double f64_with_hi(double x, int32_t hi) {
  uint64_t b;
  memcpy(&b, &x, sizeof(b));
  b = ((uint64_t)(uint32_t)hi << 32) | (b & 0xffffffffull);
  memcpy(&x, &b, sizeof(b));
  return x;
}
// (host and device: nhip_loss_log1p_pinned hands the host's compilation of the same text to the CPU tests)
__host__ __device__ inline double log1p_pinned(double x) {
  constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  constexpr double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                   Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                   Lp7 = 1.479819860511658591e-01;
  const int hx = f64_hi(x);
  if (!(x >= 0.0) || hx >= 0x7ff00000) return x + x;  // NaN, inf (a negative x is not this function's: NaN-like garbage in, x + x out)
  if (hx < 0x3e200000) return hx < 0x3c900000 ? x : x - x * x * 0.5;  // x < 2^-29 (2^-54)
  int k = 0, hu = 1;
  double f = x, c = 0.0;
  if (hx >= 0x3FDA827A) {  // x >= 0.41422: 1 + x = 2^k (1 + f), sqrt(2) / 2 < 1 + f < sqrt(2), c the rounding of 1 + x over u
    double u;
    if (hx < 0x43400000) {
      u = 1.0 + x;
      hu = f64_hi(u);
      k = (hu >> 20) - 1023;
      c = k > 0 ? 1.0 - (u - x) : x - (u - 1.0);
      c = c / u;
    } else {
      u = x;
      hu = f64_hi(u);
      k = (hu >> 20) - 1023;
    }
    hu &= 0x000fffff;
    if (hu < 0x6a09e) {
      u = f64_with_hi(u, hu | 0x3ff00000);
    } else {
      k += 1;
      u = f64_with_hi(u, hu | 0x3fe00000);
      hu = (0x00100000 - hu) >> 2;
    }
    f = u - 1.0;
  }
  const double hfsq = 0.5 * f * f, kd = (double)k;
  if (hu == 0) {  // |f| < 2^-20
    if (f == 0.0) return k == 0 ? 0.0 : kd * ln2_hi + (c + kd * ln2_lo);
    const double R = hfsq * (1.0 - 0.66666666666666666 * f);
    return k == 0 ? f - R : kd * ln2_hi - ((R - (kd * ln2_lo + c)) - f);
  }
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double R = z * (Lp1 + z * (Lp2 + z * (Lp3 + z * (Lp4 + z * (Lp5 + z * (Lp6 + z * Lp7))))));
  return k == 0 ? f - (hfsq - s * (hfsq + R)) : kd * ln2_hi - ((hfsq - (s * (hfsq + R) + (kd * ln2_lo + c))) - f);
}

// loss_value with CAUCHY's logarithm pinned: what the relative-pose rows take (nhip_relpose.hip), so that their rho is the
// host form's in every bit; every other kind is loss_value itself
__device__ __forceinline__ LossValue loss_value_pinned(int32_t kind, double a, double s) {
  if (kind != NHIP_LOSS_CAUCHY) return loss_value(kind, a, s);
  const double b = a * a, x = s / b;
  return {x < 0x1p-54 ? s : b * log1p_pinned(x), 1.0 / (1.0 + x)};
}
#endif

}  // namespace nhip
