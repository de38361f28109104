// nhip_csm.hip -- K2 + K3, every add, 8-bit cells: csm_correlate_kernel is the strip skeleton of nhip_csm_strip.h (the
// formulation is described there) with what one-byte cells bring: a lane's 28 cells are seven dwords, accumulated
// SWAR-style in packed 16-bit fields that are unpacked before they overflow; one wave per workgroup, which never waits
// for another (a shared tile made a 4-wave workgroup as slow as its busiest strip) while the dispatcher balances the
// unequal strips across the SIMDs; a 48-row x 212-byte tile.
#include "nhip_csm_strip.h"

namespace nhip {

namespace {

using namespace csm;

#ifndef NHIP_WG_WAVES
#define NHIP_WG_WAVES 1
#endif
#ifndef NHIP_TILE_ROWS
#define NHIP_TILE_ROWS (48 * NHIP_WG_WAVES)
#endif
#ifndef NHIP_FILL_INFLIGHT
#define NHIP_FILL_INFLIGHT 4
#endif
#ifndef NHIP_WAVES_PER_SIMD
#define NHIP_WAVES_PER_SIMD 4
#endif
constexpr int SEG_DW = 7;  // aligned dwords a lane reads and accumulates per point

// ---- SWAR byte accumulation -------------------------------------------------------------
// gfx950 issues plain VOP2 integer ops (v_add_u32, v_and_b32, v_lshrrev_b32) at 2 clk per
// wave64 but every SDWA / VOP3 form (byte-select adds, v_alignbyte, v_bfe, v_perm, v_add3) at
// ~4.2 clk (tools/ubench_valu.hip).  So a lane never extracts bytes per point.  The three lanes
// of a plane row read the 21 ALIGNED dwords that start at (window start & ~3) -- 84 bytes, enough
// for the 81 window columns under any alignment -- 7 dwords each, and do per dword w:
//     even += w & 0x00FF00FF      (two 16-bit fields: sum b0 | sum b2)
//     odd  += w >> 8              (= sum b1 + 256 sum b2 + 65536 sum b3, no overflow <= 255 pts)
// i.e. 4 full-rate ops per 4 lookups.  The byte alignment s = (window start) & 3 is
// wave-uniform, so points are accumulated into one of four register sets (one class-filtered
// sub-loop each) and the sets are unpacked (before any class reaches 255 points) into the lane's 28 window-relative
// 32-bit sums: byte p of a class-s lane is window column 28*seg + p - s, so bytes p < s belong
// to the left neighbour lane and travel there with one wave shuffle each (6 per unpack).
constexpr int FLUSH_POINTS = 255;  // a 16-bit field holds 255 byte values
// Every alignment class has its own register set, so what must stay <= 255 is the number of points
// ADDED PER CLASS since the last unpack (skipped points do not count): a lane-chunk of 64 points is
// started only while no class has more than this many, so a field never exceeds 191 + 64 values.
// With ~600 points added per wave and four classes, most waves unpack once, at the end.
constexpr int SWAR_START_MAX = FLUSH_POINTS - 64;

struct Swar {
  uint32_t e[4][SEG_DW], o[4][SEG_DW];
};

// Add one point's pre-split dwords into register set SH (14 full-rate adds).
template <int SH>
__device__ __forceinline__ void swar_add(Swar &A, const uint32_t (&te)[SEG_DW], const uint32_t (&to)[SEG_DW]) {
#pragma unroll
  for (int i = 0; i < SEG_DW; i++) {
    A.e[SH][i] += te[i];
    A.o[SH][i] += to[i];
  }
}

// n members of the group share class SH: the 14 plain (full-rate) adds, n times.  The empty
// volatile asm keeps the loop a loop: without it hipcc rewrites it as acc += n * t with
// v_mad_u32_u24, a half-rate VOP3 that costs twice as much in the common n == 1 case
// (and an explicit n == 1 / n > 1 branch pair blows the register allocation: 44 B of scratch).
template <int SH>
__device__ __forceinline__ void swar_add_n(Swar &A, const uint32_t (&te)[SEG_DW], const uint32_t (&to)[SEG_DW], int n) {
#pragma nounroll
  for (int r = 0; r < n; r++) {
    asm volatile("" ::: "memory");
    swar_add<SH>(A, te, to);
  }
}

// All points of the current run segment (lanes in seg_mask), grouped by ALIGNED BASE.
// Points whose window starts fall in the same aligned dword of the same tile row read the very
// same 7 dwords and differ only in their alignment class -- and consecutive beams land in
// neighbouring cells, so on the 1081-beam scans only ~47 % of the points have a base of their
// own.  One ballot finds every lane of the segment that shares the lowest live lane's base; the
// dwords are read and split (w & 0x00FF00FF, w >> 8) ONCE per group and then added into each
// member's class set.  Measured alternatives: one point per iteration
// (no grouping) 79k pairs/s; reading 2-4 points together or a two-buffer software pipeline were
// 0-12 % slower than that (registers cost occupancy; the 4 resident waves already overlap).
__device__ __forceinline__ void swar_segment(Swar &A, const uint8_t *tile_bytes, uint32_t lane_off,
                                             uint32_t vorg, unsigned long long seg_mask) {
  const uint32_t vbase = vorg & ~3u, vcls = vorg & 3u;
  const unsigned long long cm0 = __ballot(vcls == 0u), cm1 = __ballot(vcls == 1u), cm2 = __ballot(vcls == 2u);
  unsigned long long m = seg_mask;
#pragma nounroll
  while (m) {
    const int jj = (int)__builtin_ctzll(m);
    const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int32_t)vbase, jj);
    const unsigned long long same = __ballot(vbase == base) & m;  // includes lane jj
    m &= ~same;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(tile_bytes + base + lane_off);
    uint32_t te[SEG_DW], to[SEG_DW];
#pragma unroll
    for (int i = 0; i < SEG_DW; i++) {
      const uint32_t w = p[i];
      te[i] = w & 0x00ff00ffu;
      to[i] = w >> 8;
    }
    const int n0 = __builtin_popcountll(same & cm0), n1 = __builtin_popcountll(same & cm1);
    const int n2 = __builtin_popcountll(same & cm2);
    const int n3 = __builtin_popcountll(same) - n0 - n1 - n2;
    swar_add_n<0>(A, te, to, n0);
    swar_add_n<1>(A, te, to, n1);
    swar_add_n<2>(A, te, to, n2);
    swar_add_n<3>(A, te, to, n3);
  }
}

__device__ __forceinline__ void swar_clear(Swar &A) {
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int i = 0; i < SEG_DW; i++) A.e[s][i] = A.o[s][i] = 0;
}

// acc[j] += byte sums.  Byte p = 4*i + k of a class-s lane is window column 28*seg + p - s:
// p >= s lands in this lane's acc[p - s]; p < s (at most 3 bytes per class) is column
// 28*seg - (s - p), i.e. acc[28 - (s - p)] of lane - 1, which reads it with a shuffle from
// lane + 1 (same plane row: rows never straddle waves; segment-2 lanes have no right neighbour).
__device__ __forceinline__ void swar_flush(Swar &A, uint32_t (&acc)[SEG_COLS], bool has_right) {
#pragma unroll
  for (int s = 0; s < 4; s++) {
#pragma unroll
    for (int i = 0; i < SEG_DW; i++) {
      const uint32_t ev = A.e[s][i];
      const uint32_t b0 = ev & 0xffffu, b2 = ev >> 16;
      const uint32_t od = A.o[s][i] - (b2 << 8);
      const uint32_t b1 = od & 0xffffu, b3 = od >> 16;
      const uint32_t b[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int p = 4 * i + k;
        if (p >= s) {
          acc[p - s] += b[k];
        } else {
          const uint32_t from_right = (uint32_t)__shfl_down((int)b[k], 1, 64);
          acc[SEG_COLS - (s - p)] += has_right ? from_right : 0u;
        }
      }
    }
  }
  swar_clear(A);
}

struct Cells8 {
  static constexpr int CB = 1;
  static constexpr int WG_WAVES = NHIP_WG_WAVES;  // 1: waves never wait for each other
  static constexpr int TILE_ROWS = NHIP_TILE_ROWS, FILL_INFLIGHT = NHIP_FILL_INFLIGHT, WAVES_PER_SIMD = NHIP_WAVES_PER_SIMD;
  using Word = uint32_t;
  using Acc = Swar;
  static constexpr bool UNPACKS = true;
  static constexpr int FLUSH_START_MAX = SWAR_START_MAX;
  static constexpr auto &clear = swar_clear;
  static constexpr auto &segment = swar_segment;
  static constexpr auto &finish = swar_flush;
  static __device__ __forceinline__ const uint8_t *tile_base(const uint32_t *s_tile) { return reinterpret_cast<const uint8_t *>(s_tile); }
  // 4-byte LDS stores: the 212-byte pitch is no multiple of 16
  static __device__ __forceinline__ void store_head(uint32_t *dst, const uint4 &v) { dst[0] = v.x; }
  static __device__ __forceinline__ void store_tail(uint32_t *dst, const uint4 &v) {
    dst[1] = v.y;
    dst[2] = v.z;
    dst[3] = v.w;
  }
};

template <bool VOLUME, bool DENSE>
__global__ __launch_bounds__(Strip<Cells8>::THREADS, Cells8::WAVES_PER_SIMD) void csm_correlate_kernel(CsmParams P) {
  __shared__ uint32_t s_tile[Cells8::TILE_ROWS * LP_W];
  using C = Cells8;
#include "nhip_csm_strip_body.h"
}

}  // namespace

const StripKernels &csm::strip_kernels8() {
  static const StripKernels K = {{csm_correlate_kernel<false, false>, csm_correlate_kernel<false, true>},
                                 {csm_correlate_kernel<true, false>, csm_correlate_kernel<true, true>},
                                 Strip<Cells8>::THREADS, PB_NX, Strip<Cells8>::PB_NY};
  return K;
}

}  // namespace nhip
