// nhip_ray.h -- the ray of the occupancy grid ("Occupancy grid", item 3), shared by the units that trace
// it: nhip_occupancy.hip (K14) and nhip_freespace.hip (K15).  Step k of the beam to an end cell (dx, dy) away, n = max(|dx|,
// |dy|), is (rdiv(k dx, n), rdiv(k dy, n)): closed per k, so any lane computes any step.
#pragma once
#include "nhip_common.h"

namespace nhip {

constexpr int32_t RAY_MAX_CELLS = 4096;  // |dx|, |dy| <= this keeps 2 k |d| + n below 2^26: everything is int32

#ifdef __HIPCC__
// floor((2 a + n) / (2 n)), n >= 1, |a| < 2^24: the estimate by the reciprocal is off by at most a step or two, the remainder
// says by how many (C's / would truncate)
__device__ __forceinline__ int32_t rdiv(int32_t a, int32_t n, float inv_den) {
  const int32_t num = 2 * a + n, den = 2 * n;
  int32_t q = (int32_t)floorf(__fmul_rn((float)num, inv_den));
  int32_t r = num - q * den;
  while (r < 0) {
    q--;
    r += den;
  }
  while (r >= den) {
    q++;
    r -= den;
  }
  return q;
}
// The same value in straight-line code, for a caller that wants several steps' loads in flight at once (K15's check).  With
// |a| <= RAY_MAX_CELLS^2 and n <= RAY_MAX_CELLS the quotient is at most 4096.5 in magnitude; the conversion of 2 a + n is
// inexact only beyond 2^24, where 2 n > 4096, so the estimate lies within 2e-3 of the quotient and its floor is off by at most
// one either way.  Two corrections each way are made.
__device__ __forceinline__ int32_t rdiv_straight(int32_t a, int32_t n, float inv_den) {
  const int32_t num = 2 * a + n, den = 2 * n;
  int32_t q = (int32_t)floorf(__fmul_rn((float)num, inv_den));
  int32_t r = num - q * den;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const bool under = r < 0;
    q -= under ? 1 : 0;
    r += under ? den : 0;
    const bool over = r >= den;
    q += over ? 1 : 0;
    r -= over ? den : 0;
  }
  return q;
}
#endif

}  // namespace nhip
