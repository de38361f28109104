// nhip_normals.hip -- the normals of every point of every scan: NormalComputation::GetNormals
// (src/input/normal_computation.{h,cc}, called from KDTree::EigenToKD, kdtree.cc:152-163), the randomised Hough estimate
// of Boulch & Marlet, stated deterministically.  The spec, and where it leaves the reference on purpose, is DESIGN.md
// section 3, "Scan normals"; include/nautilus_hip.h carries the summary.
//
//   normals_lds_kernel      scans of at most NORMALS_LDS_N points with a sample limit of at most NORMALS_LDS_TAKEN.  A
//                           workgroup stages its scan in LDS and takes tiles of 256 consecutive points, one point per lane.
//                           A lane's neighbour set is a bit mask over the scan (one word per 32 points, in LDS), so "the
//                           a-th neighbour in scan order" is a popcount rank-select; its vote counts per bin and the list of
//                           pairs it has taken are LDS columns too.
//   normals_general_kernel  everything else (longer scans, longer sample lists): nothing per point but the lane's private
//                           arrays; the a-th neighbour is found by testing the scan's points again.  Slow, same results.
//
// Both run the same hough_point(): the draws, the votes, AddVote's two leading bins, the stop rule, and the mean angle of
// the winning bin.  A bin does not keep a running sum of its angles: the list of taken pairs records every sample's bin,
// and the winning bin's angles are formed again, in vote order, once the winner is known.
//
// The radius growth does not rebuild the neighbour list at every step: the count reaches two exactly when (float)r passes
// the point's second smallest distance (its own, 0, included), so one pass finds that distance, a scalar loop finds the
// step, and the list is rebuilt once, at that radius.
//
// The square roots are sqrtf, correctly rounded as nhip_common.h's float_norm promises; nothing may be contracted into an
// fma (Makefile: -ffp-contract=off, and the pragma below).
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int NT = 256;                  // threads of a workgroup: points of a tile
constexpr int NORMALS_LDS_N = 1088;      // points of a scan the LDS form holds (NHIP_SHORT_SCAN_POINTS)
constexpr int NORMALS_LDS_WORDS = NORMALS_LDS_N / 32;
constexpr int NORMALS_LDS_TAKEN = 64;    // taken pairs per lane the LDS form holds (the default limit is 49)
constexpr int NORMALS_MAX_TAKEN = 128;   // NHIP_NORMALS_MAX_SAMPLES
constexpr int NORMALS_BINS = 34;         // live bins after the fold: 0 .. bin_number / 2 (+ 1 for a quotient that rounds up)
constexpr int NORMALS_TILES_Y = 5;       // workgroups per scan: the tiles of a scan of NORMALS_LDS_N points

struct NormalsParams {
  double r0, r_step;     // neighborhood_size, neighborhood_step_size
  double angle_step;     // 2 pi / bin_number
  double stop_bound;     // 2 sqrt(1 / bin_number)
  int32_t bins;          // bin_number
  int32_t max_growth;
  int32_t limit;         // the sample limit's second term
  uint32_t seed;
  int32_t lds_form;      // the general kernel: 1 = the LDS kernel takes the scans it can hold
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {  // lowbias32
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// sqrtf(dx * dx + dy * dy) < rf, every operation rounded on its own (FindNeighborPoints, kdtree.cc:234-251); d: the distance
__device__ __forceinline__ float nb_distance(float2 p, float2 q) {
  return float_norm(__fsub_rn(p.x, q.x), __fsub_rn(p.y, q.y));
}

// The vote of the ordered pair (pa, pb): unitOrthogonal(pb - pa) folded onto the upper half plane, its angle with the x
// axis, the angle's bin.  -1: no vote (a pair of zero length, or one whose length is not a finite float).
__device__ __forceinline__ int32_t vote_of(float2 pa, float2 pb, double angle_step, double &angle) {
  const float dx = __fsub_rn(pb.x, pa.x), dy = __fsub_rn(pb.y, pa.y);
  const float len = float_norm(dx, dy);
  if (!(len > 0.f) || len == INFINITY) return -1;
  float nx = __fdiv_rn(-dy, len), ny = __fdiv_rn(dx, len);
  if (ny < 0.f || (ny == 0.f && nx < 0.f)) {
    nx = -nx;
    ny = -ny;
  }
  double c = (double)nx;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  angle = acos(c);
  const int32_t bin = (int32_t)floor(__dadd_rn(__ddiv_rn(angle, angle_step), 0.5));
  return bin < NORMALS_BINS ? bin : -1;  // (never: angle <= pi)
}

// Point i (scan-local) with m >= 2 neighbours.  pt(j): point j of the scan; pick(a): the scan index of the a-th neighbour;
// cnt: the votes per bin (zeroed here); tk: the taken pairs.  Returns the normal; winner / packed: words 2 and 3 of d_info.
template <class PT, class PICK, class CNT, class TK>
__device__ __forceinline__ float2 hough_point(const NormalsParams &P, uint32_t i, uint32_t m, PT pt, PICK pick, CNT &cnt, TK &tk,
                                              int32_t &winner, int32_t &packed) {
  for (int32_t b = 0; b < NORMALS_BINS; b++) cnt.set(b, 0);
  const uint64_t pairs = (uint64_t)m * (uint64_t)(m - 1u);
  const int32_t limit = pairs < (uint64_t)P.limit ? (int32_t)pairs : P.limit;
  const uint32_t s0 = mix32(P.seed ^ mix32(i));
  uint32_t draws = 0;
  int32_t most = 0, second = 0, samples = 0, n_taken = 0, votes = 0;
  while (samples < limit) {
    // an ordered pair that was not taken yet.  limit <= m (m - 1): there is one, and the mixer is a bijection of the
    // counter, so the draws reach it
    uint32_t ja, jb;
    for (;;) {
      const uint32_t a = (uint32_t)(((uint64_t)mix32(s0 + draws) * m) >> 32);
      const uint32_t b = (uint32_t)(((uint64_t)mix32(s0 + draws + 1u) * m) >> 32);
      draws += 2u;
      if (a == b) continue;
      ja = pick(a);
      jb = pick(b);
      bool dup = false;
      for (int32_t k = 0; k < n_taken && !dup; k++) dup = tk.is(k, ja, jb);
      if (!dup) break;
    }
    double angle;
    const int32_t bin = vote_of(pt(ja), pt(jb), P.angle_step, angle);
    tk.set(n_taken++, ja, jb, bin);
    if (bin >= 0) {
      const int32_t c = cnt.get(bin) + 1;
      cnt.set(bin, c);
      votes++;
      // CircularHoughAccumulator::AddVote (normal_computation.h:45-50), to the letter: `second` can become `most`
      if (cnt.get(most) < c) {
        second = most;
        most = bin;
      } else if (cnt.get(second) < c) {
        second = bin;
      }
      // MeansDontIntersect with BinMean's integer quotients (normal_computation.cc:43-53)
      if ((double)(cnt.get(most) / P.bins) - (double)(cnt.get(second) / P.bins) >= P.stop_bound) break;
    }
    samples++;
  }
  if (votes == 0) {
    winner = -1;
    packed = samples << 16;
    return make_float2(0.f, 0.f);
  }
  double sum = 0.0;
  for (int32_t k = 0; k < n_taken; k++) {
    uint32_t ja, jb;
    if (tk.get(k, ja, jb) != most) continue;
    double angle;
    vote_of(pt(ja), pt(jb), P.angle_step, angle);
    sum = __dadd_rn(sum, angle);
  }
  const int32_t vm = cnt.get(most);
  const double a = __ddiv_rn(sum, (double)vm);
  winner = most;
  packed = vm | (samples << 16);
  return make_float2((float)cos(a), (float)sin(a));
}

// the first radius (float) at which a point with second smallest distance d2 has two neighbours, and the growths it took;
// false: none within max_growth growths
__device__ __forceinline__ bool grow_radius(const NormalsParams &P, float d2, float &rf, int32_t &steps) {
  double r = P.r0;
  steps = 0;
  rf = (float)r;
  while (!(d2 < rf)) {
    if (steps >= P.max_growth) return false;
    r = __dadd_rn(r, P.r_step);
    steps++;
    rf = (float)r;
  }
  return true;
}

// the two smallest of the distances seen so far (NaN never enters)
__device__ __forceinline__ void two_smallest(float d, float &d1, float &d2) {
  if (d < d1) {
    d2 = d1;
    d1 = d;
  } else if (d < d2) {
    d2 = d;
  }
}

// a scan's bounds from the device's offsets: false (and reported, once per scan) if they are no scan
__device__ __forceinline__ bool scan_bounds(const int32_t *__restrict__ offsets, int32_t s, uint32_t *status, int32_t &beg, int32_t &n) {
  beg = offsets[s];
  const int32_t end = offsets[s + 1];
  n = end - beg;
  if (beg >= 0 && end >= beg) return true;
  if (threadIdx.x == 0 && blockIdx.y == 0) flag_bad_id(status, BAD_SCAN_OFFSETS, beg < 0 ? beg : end, beg < 0 ? s : s + 1);
  return false;
}

__device__ __forceinline__ void normals_store(float2 *__restrict__ normals, int32_t *__restrict__ info, size_t at, float2 nrm, int32_t m,
                                              int32_t steps, int32_t winner, int32_t packed) {
  normals[at] = nrm;
  if (info) {  // (four words: the caller's pointer is an int32_t *, nothing says it is aligned to 16 bytes)
    info[4 * at] = m;
    info[4 * at + 1] = steps;
    info[4 * at + 2] = winner;
    info[4 * at + 3] = packed;
  }
}

struct NormalsShared {
  float2 xy[NORMALS_LDS_N];
  uint32_t mask[NORMALS_LDS_WORDS][NT];    // bit j & 31 of word j >> 5 of column `lane`: point j is a neighbour
  uint32_t taken[NORMALS_LDS_TAKEN][NT];   // scan index a | scan index b << 11 | (bin + 1) << 22
  uint8_t cnt[NORMALS_BINS][NT];
};

struct LdsCounts {
  NormalsShared &sh;
  int lane;
  __device__ __forceinline__ int32_t get(int32_t b) const { return sh.cnt[b][lane]; }
  __device__ __forceinline__ void set(int32_t b, int32_t v) { sh.cnt[b][lane] = (uint8_t)v; }
};
struct LdsTaken {
  NormalsShared &sh;
  int lane;
  __device__ __forceinline__ bool is(int32_t k, uint32_t ja, uint32_t jb) const {
    return (sh.taken[k][lane] & 0x3fffffu) == (ja | (jb << 11));
  }
  __device__ __forceinline__ void set(int32_t k, uint32_t ja, uint32_t jb, int32_t bin) {
    sh.taken[k][lane] = ja | (jb << 11) | ((uint32_t)(bin + 1) << 22);
  }
  __device__ __forceinline__ int32_t get(int32_t k, uint32_t &ja, uint32_t &jb) const {
    const uint32_t v = sh.taken[k][lane];
    ja = v & 0x7ffu;
    jb = (v >> 11) & 0x7ffu;
    return (int32_t)(v >> 22) - 1;
  }
};

// the neighbour mask of the lane's point p at radius rf; returns the count.  d1, d2: the two smallest distances (may be null)
__device__ __forceinline__ int32_t lds_build_mask(NormalsShared &sh, int lane, float2 p, int32_t n, float rf, float *d1, float *d2) {
  int32_t m = 0;
  for (int32_t w = 0; w * 32 < n; w++) {
    uint32_t bits = 0;
    const int32_t jend = n - w * 32 < 32 ? n - w * 32 : 32;
    for (int32_t b = 0; b < jend; b++) {
      const float d = nb_distance(p, sh.xy[w * 32 + b]);
      if (d < rf) bits |= 1u << b;
      if (d1) two_smallest(d, *d1, *d2);
    }
    sh.mask[w][lane] = bits;
    m += __builtin_popcount(bits);
  }
  return m;
}

// the scan index of the lane's rank-th neighbour (rank < the mask's count)
__device__ __forceinline__ uint32_t lds_pick(const NormalsShared &sh, int lane, uint32_t rank) {
  int32_t w = 0;
  uint32_t bits = sh.mask[0][lane];
  for (uint32_t c = __builtin_popcount(bits); rank >= c; c = __builtin_popcount(bits)) {
    rank -= c;
    bits = sh.mask[++w][lane];
  }
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t span = 16; span >= 1; span >>= 1) {
    const uint32_t c = __builtin_popcount((bits >> pos) & ((1u << span) - 1u));
    if (rank >= c) {
      rank -= c;
      pos += span;
    }
  }
  return (uint32_t)w * 32u + pos;
}

__global__ __launch_bounds__(NT) void normals_lds_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ offsets,
                                                         const NormalsParams P, float2 *__restrict__ normals,
                                                         int32_t *__restrict__ info, uint32_t *__restrict__ status) {
  __shared__ NormalsShared sh;
  const int32_t s = blockIdx.x;
  const int lane = threadIdx.x;
  int32_t beg, n;
  if (!scan_bounds(offsets, s, status, beg, n)) return;
  if (n > NORMALS_LDS_N || (int32_t)blockIdx.y * NT >= n) return;  // (uniform; a longer scan is the general kernel's)
  for (int32_t j = lane; j < n; j += NT) sh.xy[j] = xy[(size_t)beg + j];
  __syncthreads();
  // the columns of mask / taken / cnt are the lane's own: the tiles need no further barrier
  for (int32_t i = (int32_t)blockIdx.y * NT + lane; i < n; i += NORMALS_TILES_Y * NT) {
    const float2 p = sh.xy[i];
    float d1 = INFINITY, d2 = INFINITY, rf = (float)P.r0;
    int32_t steps = 0;
    int32_t m = lds_build_mask(sh, lane, p, n, rf, &d1, &d2);
    if (m < 2 && grow_radius(P, d2, rf, steps)) m = lds_build_mask(sh, lane, p, n, rf, nullptr, nullptr);
    float2 nrm = make_float2(0.f, 0.f);
    int32_t winner = -1, packed = 0;
    if (m >= 2) {
      LdsCounts cnt{sh, lane};
      LdsTaken tk{sh, lane};
      nrm = hough_point(P, (uint32_t)i, (uint32_t)m, [&](uint32_t j) { return sh.xy[j]; },
                        [&](uint32_t a) { return lds_pick(sh, lane, a); }, cnt, tk, winner, packed);
    }
    normals_store(normals, info, (size_t)beg + i, nrm, m, steps, winner, packed);
  }
}

struct PrivateCounts {
  uint8_t c[NORMALS_BINS];
  __device__ __forceinline__ int32_t get(int32_t b) const { return c[b]; }
  __device__ __forceinline__ void set(int32_t b, int32_t v) { c[b] = (uint8_t)v; }
};
struct PrivateTaken {
  uint32_t a[NORMALS_MAX_TAKEN], b[NORMALS_MAX_TAKEN];
  int8_t bin[NORMALS_MAX_TAKEN];
  __device__ __forceinline__ bool is(int32_t k, uint32_t ja, uint32_t jb) const { return a[k] == ja && b[k] == jb; }
  __device__ __forceinline__ void set(int32_t k, uint32_t ja, uint32_t jb, int32_t bn) {
    a[k] = ja;
    b[k] = jb;
    bin[k] = (int8_t)bn;
  }
  __device__ __forceinline__ int32_t get(int32_t k, uint32_t &ja, uint32_t &jb) const {
    ja = a[k];
    jb = b[k];
    return bin[k];
  }
};

__global__ __launch_bounds__(NT) void normals_general_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ offsets,
                                                             const NormalsParams P, float2 *__restrict__ normals,
                                                             int32_t *__restrict__ info, uint32_t *__restrict__ status) {
  const int32_t s = blockIdx.x;
  int32_t beg, n;
  // (with the LDS kernel in the launch, that one reports the scan)
  if (!scan_bounds(offsets, s, P.lds_form ? nullptr : status, beg, n)) return;
  if (P.lds_form && n <= NORMALS_LDS_N) return;
  const float2 *__restrict__ sxy = xy + beg;
  for (int64_t i = (int64_t)blockIdx.y * NT + threadIdx.x; i < n; i += NORMALS_TILES_Y * NT) {
    const float2 p = sxy[i];
    float d1 = INFINITY, d2 = INFINITY, rf = (float)P.r0;
    int32_t steps = 0, m = 0;
    for (int32_t j = 0; j < n; j++) {
      const float d = nb_distance(p, sxy[j]);
      m += d < rf ? 1 : 0;
      two_smallest(d, d1, d2);
    }
    if (m < 2 && grow_radius(P, d2, rf, steps)) {
      m = 0;
      for (int32_t j = 0; j < n; j++) m += nb_distance(p, sxy[j]) < rf ? 1 : 0;
    }
    float2 nrm = make_float2(0.f, 0.f);
    int32_t winner = -1, packed = 0;
    if (m >= 2) {
      PrivateCounts cnt;
      PrivateTaken tk;
      auto pick = [&](uint32_t a) {  // the a-th point of the scan that passes the test (a < m: there is one)
        int32_t j = 0;
        for (;; j++) {
          if (nb_distance(p, sxy[j]) < rf && a-- == 0u) break;
        }
        return (uint32_t)j;
      };
      nrm = hough_point(P, (uint32_t)i, (uint32_t)m, [&](uint32_t j) { return sxy[j]; }, pick, cnt, tk, winner, packed);
    }
    normals_store(normals, info, (size_t)beg + (size_t)i, nrm, m, steps, winner, packed);
  }
}

}  // namespace

int launch_normals_estimate(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_normals_spec_t &spec,
                            int32_t sample_limit, float *d_normals, int32_t *d_info, hipStream_t s) {
  if (n_scans == 0) return NHIP_OK;
  static_assert(NORMALS_LDS_N == NHIP_SHORT_SCAN_POINTS && NORMALS_LDS_N % 32 == 0 && NORMALS_LDS_N < 2048,
                "the LDS form's masks and its packed pairs");
  static_assert(NORMALS_MAX_TAKEN == NHIP_NORMALS_MAX_SAMPLES && NORMALS_MAX_TAKEN < 256, "the taken lists and the contract's limit");
  static_assert(NORMALS_BINS >= NHIP_NORMALS_MAX_BINS / 2 + 2 && NORMALS_BINS <= 63, "the live bins and the contract's limit");
  NormalsParams P;
  P.r0 = spec.neighborhood_size;
  P.r_step = spec.neighborhood_step_size;
  P.angle_step = (2.0 * M_PI) / (double)spec.bin_number;
  P.stop_bound = 2.0 * sqrt(1.0 / (double)spec.bin_number);
  P.bins = spec.bin_number;
  P.max_growth = spec.max_growth_steps;
  P.limit = sample_limit;
  P.seed = spec.seed;
  P.lds_form = sample_limit <= NORMALS_LDS_TAKEN ? 1 : 0;
  const dim3 grid((uint32_t)n_scans, NORMALS_TILES_Y);
  auto *xy = reinterpret_cast<const float2 *>(d_xy);
  auto *nrm = reinterpret_cast<float2 *>(d_normals);
  if (P.lds_form) hipLaunchKernelGGL(normals_lds_kernel, grid, dim3(NT), 0, s, xy, d_offsets, P, nrm, d_info, dev_status());
  hipLaunchKernelGGL(normals_general_kernel, grid, dim3(NT), 0, s, xy, d_offsets, P, nrm, d_info, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
