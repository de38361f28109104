// nhip_csm16.hip -- K2 + K3 for 16-bit cells: every add of the exhaustive (theta, x, y) correlation.
//
// Replaces CorrelativeScanMatcher::GetTransformation (call site src/optimization/solver.cc:633-638), batched over
// candidate pairs, at the cell width that keeps reported scores within 1e-5 of an unquantised table (DESIGN.md
// section 3).  It is the cross-check of the branch-and-bound matcher at that width (nhip_bnb.hip: same records, bit
// for bit), the path of lattices that matcher does not hold (more than 88 x 88 translations, more rotations than its
// bounds fit in LDS) and the kernel that performs the work SURVEY.md section 8(d) prices.
//
// Formulation: the strip skeleton of nhip_csm_strip.h -- accumulator-stationary, LDS-tiled, one wave per
// 21-row strip of the (nx x ny) plane of one rotation of one pair, three lanes per plane row with 28 consecutive
// x-shifts each, points visited in beam order as runs that share one staged tile of the target grid, grouped by
// the aligned LDS address their windows start at -- with what two-byte cells change:
//  * a lane's 28 cells are 56 bytes: seven 8-BYTE reads (ds_read_b64, 256 B/clk/CU; the same bytes as ds_read_b32
//    or ds_read2_b64 would take twice the LDS cycles).  8-byte reads must be 8-byte aligned (an unaligned one is
//    replayed at 64 cycles), so windows are grouped by their 8-byte-aligned start and there are again FOUR
//    alignment classes: s = (window start column) & 3 cells;
//  * tile pitch 53 qwords (424 bytes): lane l = 3 * row + segment reads qword slot 53 * row + 7 * segment = 7 l
//    (mod 32) -- a permutation of the 32 slots for each 32-lane group, conflict-free;
//  * no packed fields: a dword w holds two cells; `raw += w; hi += w >> 16` -- three plain VOP2 operations per two
//    lookups -- and sum(lo) = raw - (sum(hi) << 16) modulo 2^32 at the end, exact while a sum stays below 2^32
//    (scans of up to 65,536 points; the API admits 32,768, whose sums fit the int32 it reports).  Nothing overflows in
//    between, so there is no periodic unpack;
//  * cells pair up inside a dword: for odd s a lane's x-shift pairs straddle dwords, so the accumulators come in two
//    PARITY sets of 15 (raw, hi) pairs -- 60 registers; classes 2 and 3 shift the pair index by one, and their
//    first dword (like the low cell of class 1's) belongs to the left neighbour lane's last x-shifts: it is added
//    into pair 14 of the lane's own set and travels there with a wave shuffle at the end.
// LDS is what limits the waves here: a tile of 48 rows x 424 bytes per one-wave workgroup (the 8-bit kernel's shape)
// is 20 KB -- 8 waves per CU.  Four waves (84 plane rows: one 81 x 81 plane) sharing ONE 96-row tile (40.7 KB) put
// 16 waves on a CU, and the shared fills more than pay for the barriers: measured on 3,000 config #2 pairs
// (profiles/r03_csm16_variants.jsonl, tools/c16_variants.sh) 49.6 ms with one wave per 48-row tile, 45.0 / 43.5 with two
// per 64 / 72 rows, 41.1 / 43.0 / 46.4 with four per 120 / 112 / 104 rows (12 waves per CU), 37.9 with four per 96 rows;
// letting hipcc fold the high-half shift into SDWA adds: 40.6.
#include "nhip_csm_strip.h"

namespace nhip {

namespace {

using namespace csm;

#ifndef NHIP_C16_WG_WAVES
#define NHIP_C16_WG_WAVES 4
#endif
#ifndef NHIP_C16_SDWA
#define NHIP_C16_SDWA 0  // 1: let hipcc fold the high-half shift into SDWA adds (measurement)
#endif
#ifndef NHIP_C16_TILE_ROWS
#define NHIP_C16_TILE_ROWS (24 * NHIP_C16_WG_WAVES)
#endif
#ifndef NHIP_C16_FILL_INFLIGHT
#define NHIP_C16_FILL_INFLIGHT 4
#endif
#ifndef NHIP_C16_WAVES_PER_SIMD
#define NHIP_C16_WAVES_PER_SIMD 4
#endif
constexpr int SEG_QW = 7;           // aligned qwords a lane reads per point
constexpr int SEG_DW = 2 * SEG_QW;  // 14 dwords = 28 cells
constexpr int PAIRS = SEG_DW + 1;   // (raw, hi) pairs per parity set: 14 + the left neighbour's

// Accumulators of one lane.  Parity 0 (classes 0, 2): pair j < 14 = x-shifts (2j, 2j + 1) of the lane's 28;
// pair 14 = x-shifts (26, 27) of the left neighbour.  Parity 1 (classes 1, 3): pair j < 14 = x-shifts
// (2j - 1, 2j) -- the low half of pair 0 is the left neighbour's x-shift 27; pair 14 = its x-shifts (25, 26).
struct Acc16 {
  uint32_t raw[2][PAIRS], hi[2][PAIRS];
};

__device__ __forceinline__ void acc_clear(Acc16 &A) {
#pragma unroll
  for (int p = 0; p < 2; p++)
#pragma unroll
    for (int j = 0; j < PAIRS; j++) A.raw[p][j] = A.hi[p][j] = 0u;
}

// One point of class S: dword i of the lane's 14 goes to pair i - (S >> 1) of parity set S & 1 (28 full-rate adds).
template <int S>
__device__ __forceinline__ void acc_add(Acc16 &A, const uint32_t (&w)[SEG_DW], const uint32_t (&h)[SEG_DW]) {
  constexpr int PAR = S & 1, SH = S >> 1;
#pragma unroll
  for (int i = 0; i < SEG_DW; i++) {
    constexpr int LEFT = PAIRS - 1;
    const int j = i - SH < 0 ? LEFT : i - SH;
    A.raw[PAR][j] += w[i];
    A.hi[PAR][j] += h[i];
  }
}

// n members of the group share class S.  (The empty asm keeps the loop a loop of plain adds: hipcc would rewrite it
// as acc += n * w with v_mad_u32_u24, a half-rate VOP3 -- twice the cost in the common n == 1 case.)
template <int S>
__device__ __forceinline__ void acc_add_n(Acc16 &A, const uint32_t (&w)[SEG_DW], const uint32_t (&h)[SEG_DW], int n) {
#pragma nounroll
  for (int r = 0; r < n; r++) {
    asm volatile("" ::: "memory");
    acc_add<S>(A, w, h);
  }
}

// The lane's seven qwords of one group.  One asm statement: hipcc would merge neighbouring 8-byte reads into
// ds_read2_b64 (half the bytes per LDS cycle, and banked like 4-byte reads: the pitch is chosen for ds_read_b64).
__device__ __forceinline__ void read_qwords(uint32_t addr, uint32_t (&w)[SEG_DW]) {
  unsigned long long q0, q1, q2, q3, q4, q5, q6;
  asm volatile(
      "ds_read_b64 %0, %7\n\t"
      "ds_read_b64 %1, %7 offset:8\n\t"
      "ds_read_b64 %2, %7 offset:16\n\t"
      "ds_read_b64 %3, %7 offset:24\n\t"
      "ds_read_b64 %4, %7 offset:32\n\t"
      "ds_read_b64 %5, %7 offset:40\n\t"
      "ds_read_b64 %6, %7 offset:48\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3), "=&v"(q4), "=&v"(q5), "=&v"(q6)
      : "v"(addr)
      : "memory");
  const unsigned long long q[SEG_QW] = {q0, q1, q2, q3, q4, q5, q6};
#pragma unroll
  for (int i = 0; i < SEG_QW; i++) {
    w[2 * i] = (uint32_t)q[i];
    w[2 * i + 1] = (uint32_t)(q[i] >> 32);
  }
}

// All points of the current run segment (lanes in seg_mask), grouped by the 8-byte-aligned LDS offset their windows
// start at: the members of a group read the very same seven qwords and differ only in their class.
__device__ __forceinline__ void acc_segment(Acc16 &A, uint32_t tile_addr, uint32_t lane_off, uint32_t vorg,
                                            unsigned long long seg_mask) {
  const uint32_t vbase = vorg & ~7u, vcls = (vorg >> 1) & 3u;
  const unsigned long long cm0 = __ballot(vcls == 0u), cm1 = __ballot(vcls == 1u), cm2 = __ballot(vcls == 2u);
  unsigned long long m = seg_mask;
#pragma nounroll
  while (m) {
    const int jj = (int)__builtin_ctzll(m);
    const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int32_t)vbase, jj);
    const unsigned long long same = __ballot(vbase == base) & m;  // includes lane jj
    m &= ~same;
    uint32_t w[SEG_DW], h[SEG_DW];
    read_qwords(tile_addr + base + lane_off, w);
#pragma unroll
    for (int i = 0; i < SEG_DW; i++) {
      h[i] = w[i] >> 16;
#if !NHIP_C16_SDWA
      // (opaque: hipcc would fold the shift into every add as an SDWA operand select -- v_add_u32_sdwa issues at
      //  ~4.2 clocks against ~2.3 for the plain add, tools/ubench_valu.hip -- 14 shifts per group are cheaper)
      asm volatile("" : "+v"(h[i]));
#endif
    }
    const int n0 = __builtin_popcountll(same & cm0), n1 = __builtin_popcountll(same & cm1);
    const int n2 = __builtin_popcountll(same & cm2);
    const int n3 = __builtin_popcountll(same) - n0 - n1 - n2;
    acc_add_n<0>(A, w, h, n0);
    acc_add_n<1>(A, w, h, n1);
    acc_add_n<2>(A, w, h, n2);
    acc_add_n<3>(A, w, h, n3);
  }
}

// The lane's 28 sums (x-shifts 28 * segment + i) from the two parity sets; what belongs to the left neighbour comes
// from lane + 1 (same plane row: rows never straddle waves; segment-2 lanes have no right neighbour).
__device__ __forceinline__ void acc_finish(const Acc16 &A, uint32_t (&acc)[SEG_COLS], bool has_right) {
  constexpr int LEFT = PAIRS - 1;
#pragma unroll
  for (int i = 0; i < SEG_COLS; i++) acc[i] = 0u;
#pragma unroll
  for (int j = 0; j < PAIRS; j++) {
    const uint32_t lo0 = A.raw[0][j] - (A.hi[0][j] << 16), hi0 = A.hi[0][j];
    const uint32_t lo1 = A.raw[1][j] - (A.hi[1][j] << 16), hi1 = A.hi[1][j];
    if (j < LEFT) {
      acc[2 * j] += lo0;
      acc[2 * j + 1] += hi0;
      acc[2 * j] += hi1;
      if (j > 0) {
        acc[2 * j - 1] += lo1;
      } else {
        const uint32_t r = (uint32_t)__shfl_down((int)lo1, 1, 64);  // the right neighbour's x-shift -1 = my 27
        acc[SEG_COLS - 1] += has_right ? r : 0u;
      }
    } else {
      const uint32_t r0 = (uint32_t)__shfl_down((int)lo0, 1, 64), r1 = (uint32_t)__shfl_down((int)hi0, 1, 64);
      const uint32_t r2 = (uint32_t)__shfl_down((int)lo1, 1, 64), r3 = (uint32_t)__shfl_down((int)hi1, 1, 64);
      acc[SEG_COLS - 2] += has_right ? r0 : 0u;  // parity 0: x-shifts (-2, -1) of the right neighbour
      acc[SEG_COLS - 1] += has_right ? r1 : 0u;
      acc[SEG_COLS - 3] += has_right ? r2 : 0u;  // parity 1: x-shifts (-3, -2)
      acc[SEG_COLS - 2] += has_right ? r3 : 0u;
    }
  }
}

struct Cells16 {
  static constexpr int CB = 2;
  static constexpr int WG_WAVES = NHIP_C16_WG_WAVES;
  static constexpr int TILE_ROWS = NHIP_C16_TILE_ROWS, FILL_INFLIGHT = NHIP_C16_FILL_INFLIGHT, WAVES_PER_SIMD = NHIP_C16_WAVES_PER_SIMD;
  using Word = unsigned long long;
  using Acc = Acc16;
  static constexpr bool UNPACKS = false;  // (nothing overflows before the end)
  static constexpr int FLUSH_START_MAX = 0;
  static constexpr auto &clear = acc_clear;
  static constexpr auto &segment = acc_segment;
  static constexpr auto &finish = acc_finish;
  static __device__ __forceinline__ uint32_t tile_base(const unsigned long long *s_tile) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)s_tile;
  }
  // 8-byte LDS stores: rows of the 424-byte pitch start on 8-byte boundaries
  static __device__ __forceinline__ void store_head(unsigned long long *dst, const uint4 &v) { dst[0] = ((unsigned long long)v.y << 32) | v.x; }
  static __device__ __forceinline__ void store_tail(unsigned long long *dst, const uint4 &v) { dst[1] = ((unsigned long long)v.w << 32) | v.z; }
};

template <bool VOLUME, bool DENSE>
__global__ __launch_bounds__(Strip<Cells16>::THREADS, Cells16::WAVES_PER_SIMD) void csm_correlate16_kernel(CsmParams P) {
  __shared__ __align__(16) unsigned long long s_tile[Cells16::TILE_ROWS * LP_W];
  using C = Cells16;
#include "nhip_csm_strip_body.h"
}

}  // namespace

const StripKernels &csm::strip_kernels16() {
  static const StripKernels K = {{csm_correlate16_kernel<false, false>, csm_correlate16_kernel<false, true>},
                                 {csm_correlate16_kernel<true, false>, csm_correlate16_kernel<true, true>},
                                 Strip<Cells16>::THREADS, PB_NX, Strip<Cells16>::PB_NY};
  return K;
}

}  // namespace nhip
