// nhip_bnb_exact.h -- the exact sums of the branch-and-bound matcher's kernels (nhip_bnb.hip): integer sums of the
// stored cells over a scan's points, for the poses of a block or sub-block, and the key of the best of them.
//
// Owns four kinds: eval_block / eval_sub -- from the points, on the stored image (the general kernel and the seeds of
// long scans); block_sums8 / sub_sums8 / pair_sums8 -- from the origins a wave holds, on the tiled 8-bit plane (the cells
// of 8-bit grids, the high bytes of 16-bit ones: a whole block, one sub-block, two sub-blocks side by side), and their
// *_masked forms over the chunks of the list a mask names (the candidates' kernels); pose_sum16 / refine16 -- single poses of 16-bit grids that the high-byte bound
// admits, from the tiled 16-bit image; and best_key / best_sum / best_sum_cached -- the pair's running best,
// key = sum << 32 | ~linear index, so that the maximum key is the maximum sum at the smallest index.
// Assumes: the slot layout of nhip_layout.hip (every offset an evaluation forms lies inside the descriptor it is given),
// hi_tiled / t16_tiled of nhip_common.h, scans of at most 65,536 points (32-bit sums of 16-bit cells).
// Included by nhip_bnb.hip only.
#pragma once
#include "nhip_bnb_origin.h"

namespace nhip {
namespace {

constexpr int SEG_CHUNKS = 32;        // 64-point chunks between reductions: 32 * 255 * 8 lanes < 65536 (16-bit fields); even
constexpr int EVAL_CHUNKS = 2;  // 64-point chunks whose row loads a block evaluation keeps in flight

// ---- the pair's running best
template <bool GLOBAL>
__device__ __forceinline__ uint32_t best_sum(unsigned long long *best) {
  unsigned long long b;
  if (GLOBAL) b = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else b = *(volatile unsigned long long *)best;
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));  // one value for the whole wave
}
// The pair's own workgroup keeps its best in LDS (GLOBAL = false: csm_bnb_kernel); the takers of handed-over
// rotations share it through keys[pair] (GLOBAL = true: csm_bnb_rot_kernel).  Between two looks at a best that
// lives in global memory (a device-scope atomic load: microseconds under load) a taker works with its copy, raised
// by its own finds; a stale copy only costs pruning, never the result.
template <bool GLOBAL>
__device__ __forceinline__ uint32_t best_sum_cached(unsigned long long *best, uint32_t copy) {
  return GLOBAL ? copy : best_sum<false>(best);
}

// the best key (sum << 32 | ~linear index) over the lanes' poses (ix, iy) of rotation k, the same in every lane
__device__ __forceinline__ unsigned long long best_key(const BnbParams &P, int32_t k, int32_t ix, int32_t iy, uint32_t total,
                                                       int top) {
  unsigned long long key = 0ull;
  if (ix < P.nx && iy < P.ny) {
    const uint32_t lin = (uint32_t)((k * P.nx + ix) * P.ny + iy);
    key = ((unsigned long long)total << 32) | (0xffffffffu - lin);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    if (m > top) continue;
    const unsigned long long o = shfl_xor_u64b(key, m);
    key = o > key ? o : key;
  }
  return key;
}

// ---- the lattice inside a block ----------------------------------------------------------------------------------
// Of the 8 pose columns (rows) of block column (row) B, the first block_extent(n, B) are poses of a lattice of n columns
// (rows): 8 everywhere but in the last block column (row) of a lattice that is no multiple of 8.  4 x 4 sub-block (sy, sx) of
// a block with extents (vy, vx) holds a pose iff 4 sx < vx and 4 sy < vy.  Wave-uniform wherever the block is.
__device__ __forceinline__ int32_t block_extent(int32_t n, int32_t B) { return min(max(n - BNB_B * B, 0), BNB_B); }
__device__ __forceinline__ bool sub_valid(int32_t vy, int32_t vx, int32_t sy, int32_t sx) {
  return BNB_B4 * sx < vx && BNB_B4 * sy < vy;
}

// ---- exact sums of one 8 x 8 block -----------------------------------------------------------------------
// Returns the block's best key (sum << 32 | ~linear index) over its valid poses, the same in every lane.
template <int CB>
__device__ __forceinline__ unsigned long long eval_block(const BnbParams &P, const uint8_t *grid, const float2 *pts,
                                                         int32_t n_pts, float cf, float sf, int32_t cx, int32_t cy,
                                                         int32_t k, int32_t Y, int32_t X, int lane) {
  uint32_t total = 0u;  // this lane's pose: (dy, dx) below
  int dy, dx;
  // (stored image + skip map: every offset the evaluation can form lies inside; see nhip_layout.hip make_layout)
  const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(grid, P.grid_bytes + P.skip_bytes);
  if (CB == 1) {
    const float2 none = make_float2(0.f, 0.f);
    for (int32_t c0 = 0; c0 < n_pts; c0 += 64 * SEG_CHUNKS) {
      uint32_t E[8][2], O[8][2];
#pragma unroll
      for (int y = 0; y < 8; y++) E[y][0] = E[y][1] = O[y][0] = O[y][1] = 0u;
      const int32_t c1 = min(n_pts, c0 + 64 * SEG_CHUNKS);
      // EVAL_CHUNKS 64-point chunks per iteration, their row loads issued together, and the points of the next
      // iteration fetched before this one's rows are consumed (the dependent chain is point -> window origin -> rows).
      float qx[EVAL_CHUNKS], qy[EVAL_CHUNKS];  // (plain floats: arrays of float2 end up in scratch)
#pragma unroll
      for (int u = 0; u < EVAL_CHUNKS; u++) {
        const float2 q = c0 + 64 * u + lane < c1 ? pts[c0 + 64 * u + lane] : none;
        qx[u] = q.x;
        qy[u] = q.y;
      }
      for (int32_t c = c0; c < c1; c += 64 * EVAL_CHUNKS) {
        float nx[EVAL_CHUNKS], ny[EVAL_CHUNKS];
#pragma unroll
        for (int u = 0; u < EVAL_CHUNKS; u++) {
          const int32_t idx = c + 64 * (EVAL_CHUNKS + u) + lane;
          const float2 q = idx < c1 ? pts[idx] : none;
          nx[u] = q.x;
          ny[u] = q.y;
        }
        uint32_t g[EVAL_CHUNKS], sh[EVAL_CHUNKS], w[EVAL_CHUNKS][8][3];
#pragma unroll
        for (int u = 0; u < EVAL_CHUNKS; u++) {
          const int32_t idx = c + 64 * u + lane;
          patch_origin(P, idx < c1, make_float2(qx[u], qy[u]), cf, sf, cx, cy, Y, X, &g[u], &sh[u]);
#pragma unroll
          for (int y = 0; y < 8; y++) {
            const u32x3 r = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)(g[u] + (uint32_t)(y * P.pitch)), 0, 0);
            w[u][y][0] = r.x; w[u][y][1] = r.y; w[u][y][2] = r.z;
          }
        }
#pragma unroll
        for (int u = 0; u < EVAL_CHUNKS; u++) {
#pragma unroll
          for (int y = 0; y < 8; y++) {
            const uint32_t n0 = __builtin_amdgcn_alignbit(w[u][y][1], w[u][y][0], sh[u]);
            const uint32_t n1 = __builtin_amdgcn_alignbit(w[u][y][2], w[u][y][1], sh[u]);
            E[y][0] += n0 & M8; O[y][0] += n0 >> 8;
            E[y][1] += n1 & M8; O[y][1] += n1 >> 8;
          }
          qx[u] = nx[u];
          qy[u] = ny[u];
        }
      }
      uint32_t R[32];  // R[4 y + d]: d = 0: dx 0, 2; 1: dx 1, 3; 2: dx 4, 6; 3: dx 5, 7
#pragma unroll
      for (int y = 0; y < 8; y++) {
        R[4 * y + 0] = E[y][0];
        R[4 * y + 1] = O[y][0] - ((E[y][0] >> 16) << 8);
        R[4 * y + 2] = E[y][1];
        R[4 * y + 3] = O[y][1] - ((E[y][1] >> 16) << 8);
      }
      rs_step<32, 1>(R, lane & 1);
      rs_step<16, 2>(R, lane & 2);
      rs_step<8, 4>(R, lane & 4);
      uint32_t V[8];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        V[2 * i] = R[i] & 0xffffu;
        V[2 * i + 1] = R[i] >> 16;
      }
      rs_step<8, 8>(V, lane & 8);
      rs_step<4, 16>(V, lane & 16);
      rs_step<2, 32>(V, lane & 32);
      total += V[0];
    }
    const int r = 8 * (2 * ((lane >> 5) & 1) + ((lane >> 4) & 1)) + 4 * ((lane >> 2) & 1) + 2 * ((lane >> 1) & 1) + (lane & 1);
    const int f = (lane >> 3) & 1, d = r & 3;
    dy = r >> 2;
    dx = 4 * (d >> 1) + (d & 1) + 2 * f;
  } else {
    uint32_t A[64];  // A[8 y + x]: 32-bit sums (n_pts * 65535 < 2^32 for n_pts <= 65536)
#pragma unroll
    for (int i = 0; i < 64; i++) A[i] = 0u;
    float2 qn = lane < n_pts ? pts[lane] : make_float2(0.f, 0.f);
    for (int32_t c = 0; c < n_pts; c += 64) {
      const float2 q = qn;
      if (c + 64 + lane < n_pts) qn = pts[c + 64 + lane];  // next chunk's point: in flight while this one's rows load
      uint32_t g = 0u, sh = 0u;
      if (c + lane < n_pts) {
        int32_t prow, pcol;
        window_origin(q, cf, sf, P, cx, cy, &prow, &pcol);
        const int32_t col = pcol + BNB_B * X;
        g = (uint32_t)((prow + BNB_B * Y) * P.pitch + ((2 * col) & ~3));
        sh = (uint32_t)(col & 1) * 16u;
      }
#pragma unroll
      for (int y = 0; y < 8; y++) {
        const u32x4 r4 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(g + (uint32_t)(y * P.pitch)), 0, 0);
        const uint32_t w[5] = {r4.x, r4.y, r4.z, r4.w,
                               __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)(g + (uint32_t)(y * P.pitch) + 16u), 0, 0)};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t nj = __builtin_amdgcn_alignbit(w[j + 1], w[j], sh);
          A[8 * y + 2 * j] += nj & 0xffffu;
          A[8 * y + 2 * j + 1] += nj >> 16;
        }
      }
    }
    rs_step<64, 1>(A, lane & 1);
    rs_step<32, 2>(A, lane & 2);
    rs_step<16, 4>(A, lane & 4);
    rs_step<8, 8>(A, lane & 8);
    rs_step<4, 16>(A, lane & 16);
    rs_step<2, 32>(A, lane & 32);
    total = A[0];  // lane l holds A[l]: bit s of the register index was selected by bit s of the lane
    dy = lane >> 3;
    dx = lane & 7;
  }
  const int32_t ix = BNB_B * X + dx, iy = BNB_B * Y + dy;
  unsigned long long key = 0ull;
  if (ix < P.nx && iy < P.ny) {
    const uint32_t lin = (uint32_t)((k * P.nx + ix) * P.ny + iy);
    key = ((unsigned long long)total << 32) | (0xffffffffu - lin);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = shfl_xor_u64b(key, m);
    key = o > key ? o : key;
  }
  return key;
}

// ---- exact sums of one 4 x 4 sub-block ----------------------------------------------------------------------
// As eval_block on rows [4 sy, 4 sy + 4) and columns [4 sx, 4 sx + 4) of block (Y, X): four loads per point.
template <int CB>
__device__ __forceinline__ unsigned long long eval_sub(const BnbParams &P, __amdgpu_buffer_rsrc_t rsrc, const float2 *pts,
                                                       int32_t n_pts, float cf, float sf, int32_t cx, int32_t cy,
                                                       int32_t k, int32_t Y, int32_t X, int32_t sy, int32_t sx, int lane) {
  uint32_t total = 0u;
  int dy, dx;
  const float2 none = make_float2(0.f, 0.f);
  constexpr int U = 4;  // chunks whose loads are in flight together
  if (CB == 1) {
    static_assert(SEG_CHUNKS % U == 0, "segments are whole iterations");
    for (int32_t c0 = 0; c0 < n_pts; c0 += 64 * SEG_CHUNKS) {
      uint32_t E[4], O[4];
#pragma unroll
      for (int y = 0; y < 4; y++) E[y] = O[y] = 0u;
      const int32_t c1 = min(n_pts, c0 + 64 * SEG_CHUNKS);
      for (int32_t c = c0; c < c1; c += 64 * U) {
        uint32_t sh[U];
        u32x2 w[U][4];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int32_t idx = c + 64 * u + lane;
          uint32_t g;
          patch_origin(P, idx < c1, idx < c1 ? pts[idx] : none, cf, sf, cx, cy, Y, X, &g, &sh[u]);
          if (idx < c1) g += (uint32_t)(BNB_B4 * sy * P.pitch + BNB_B4 * sx);
#pragma unroll
          for (int y = 0; y < 4; y++) w[u][y] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(g + (uint32_t)(y * P.pitch)), 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
          for (int y = 0; y < 4; y++) {
            const uint32_t n = __builtin_amdgcn_alignbit(w[u][y].y, w[u][y].x, sh[u]);
            E[y] += n & M8;
            O[y] += n >> 8;
          }
      }
      uint32_t R[8];  // R[2 y + d]: d = 0: dx 0, 2; d = 1: dx 1, 3
#pragma unroll
      for (int y = 0; y < 4; y++) {
        R[2 * y] = E[y];
        R[2 * y + 1] = O[y] - ((E[y] >> 16) << 8);
      }
      rs_step<8, 1>(R, lane & 1);
      rs_step<4, 2>(R, lane & 2);
      rs_step<2, 4>(R, lane & 4);
      uint32_t V[2] = {R[0] & 0xffffu, R[0] >> 16};
      rs_step<2, 8>(V, lane & 8);
      V[0] = add_xor<16>(V[0]);
      V[0] = add_xor<32>(V[0]);
      total += V[0];
    }
    dy = ((lane >> 1) & 1) + 2 * ((lane >> 2) & 1);
    dx = (lane & 1) + 2 * ((lane >> 3) & 1);
  } else {
    uint32_t A[16];  // A[4 y + x]
#pragma unroll
    for (int i = 0; i < 16; i++) A[i] = 0u;
    for (int32_t c = 0; c < n_pts; c += 64 * U) {
      uint32_t sh[U];
      u32x3 w[U][4];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int32_t idx = c + 64 * u + lane;
        uint32_t g = 0u;
        sh[u] = 0u;
        if (idx < n_pts) {
          int32_t prow, pcol;
          window_origin(pts[idx], cf, sf, P, cx, cy, &prow, &pcol);
          const int32_t col = pcol + BNB_B * X + BNB_B4 * sx;
          g = (uint32_t)((prow + BNB_B * Y + BNB_B4 * sy) * P.pitch + ((2 * col) & ~3));
          sh[u] = (uint32_t)(col & 1) * 16u;
        }
#pragma unroll
        for (int y = 0; y < 4; y++) w[u][y] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)(g + (uint32_t)(y * P.pitch)), 0, 0);
      }
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int y = 0; y < 4; y++) {
          const uint32_t n0 = __builtin_amdgcn_alignbit(w[u][y].y, w[u][y].x, sh[u]);
          const uint32_t n1 = __builtin_amdgcn_alignbit(w[u][y].z, w[u][y].y, sh[u]);
          A[4 * y + 0] += n0 & 0xffffu;
          A[4 * y + 1] += n0 >> 16;
          A[4 * y + 2] += n1 & 0xffffu;
          A[4 * y + 3] += n1 >> 16;
        }
    }
    rs_step<16, 1>(A, lane & 1);
    rs_step<8, 2>(A, lane & 2);
    rs_step<4, 4>(A, lane & 4);
    rs_step<2, 8>(A, lane & 8);
    A[0] = add_xor<16>(A[0]);
    A[0] = add_xor<32>(A[0]);
    total = A[0];  // lane l holds A[l & 15]
    dy = (lane >> 2) & 3;
    dx = lane & 3;
  }
  const int32_t ix = BNB_B * X + BNB_B4 * sx + dx, iy = BNB_B * Y + BNB_B4 * sy + dy;
  unsigned long long key = 0ull;
  if (ix < P.nx && iy < P.ny) {
    const uint32_t lin = (uint32_t)((k * P.nx + ix) * P.ny + iy);
    key = ((unsigned long long)total << 32) | (0xffffffffu - lin);
  }
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {  // (lanes 16.. hold copies)
    const unsigned long long o = shfl_xor_u64b(key, m);
    key = o > key ? o : key;
  }
  return key;
}

// Exact sums on the matcher's 8-BIT plane (the cells of 8-bit grids; the high bytes of 16-bit cells), for the rotation
// whose origins the wave holds.  The plane is tiled, two copies (nhip_common.h hi_tiled; `pitch` = tiles per tile row,
// `copy_bytes` = bytes of a copy): a row's bytes come from the copy in which they start in a tile's first half, so no
// read crosses a tile, and the rows of a point's window are 16 bytes apart inside a tile and (tiles per row - 1) * 128
// + 16 further at its end.
// 4 x 4 sub-block (sy, sx) of block (Y, X): four 8-byte row loads per point.  Returns the sum of this lane's pose
// (*dy, *dx inside the sub-block; lanes 16.. hold copies of lanes 0..15).
// (A sub-block at the lattice's upper edge holds poses in its first rows or columns only, and still reads all 4 x 8 bytes:
//  reading only those rows, and 4 bytes of a single column, under wave-uniform branches was measured and lost -- the
//  candidates' kernel 2.35 -> 2.42 ms, its code 4 KB longer; profiles/r16_lattice_edge.txt.)
__device__ __forceinline__ uint32_t sub_sums8(__amdgpu_buffer_rsrc_t rsrc, uint32_t pitch, uint32_t copy_bytes, const uint32_t *org,
                                              int32_t nch, int32_t Y, int32_t X, int32_t sy, int32_t sx, int lane, int *dy, int *dx) {
  const uint32_t roff = (uint32_t)(BNB_B * Y + BNB_B4 * sy), coff = (uint32_t)(BNB_B * X + BNB_B4 * sx);
  const uint32_t wrap = pitch * HI_TILE_BYTES - HI_TILE_BYTES;  // from a tile's last row to the next tile's first
  // chunks per round: 4 U row loads in flight.  (6 -> 2 together with block_sums8's rows in two groups of four: the same
  // speed within the run-to-run spread -- profiles/r03_bnb_ab_scratch_free.log -- and the by-rotation kernels fit their 128
  // registers: no scratch memory at all, where each launch used to write 225-370 MB of spills for 160 KB of records.)
  constexpr int U = 2;
  static_assert(OC % U == 0, "whole rounds");
  // (18 chunks * 255 * 8 lanes < 65536: the packed fields hold a whole scan)
  uint32_t E[4] = {0u, 0u, 0u, 0u}, O[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int r = 0; r < OC / U; r++) {
    if (U * r >= nch) continue;
    u32x2 w[U][4];
    uint32_t sh[U], cn[U];
#pragma unroll
    for (int j = 0; j < U; j++) {
      const uint32_t o = origin_of(org, U * r + j);
      cn[j] = org_cnt(o);
      const uint32_t row0 = org_row(o) + roff, col0 = org_col(o) + coff, col4 = col0 & ~3u;
      const uint32_t cp = (col4 >> 3) & 1u, q = row0 & 7u;
      const uint32_t v0 = hi_tiled(row0, col4, cp, pitch, copy_bytes);
      sh[j] = (col0 & 3u) * 8u;
#pragma unroll
      for (int y = 0; y < 4; y++)
        w[j][y] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(v0 + (q + (uint32_t)y >= 8u ? wrap : 0u) + 16u * (uint32_t)y), 0, 0);
    }
#pragma unroll
    for (int j = 0; j < U; j++)
#pragma unroll
      for (int y = 0; y < 4; y++) {
        const uint32_t n = __builtin_amdgcn_alignbit(w[j][y].y, w[j][y].x, sh[j]);
        E[y] += __umul24(n & M8, cn[j]);
        O[y] += __umul24(n >> 8, cn[j]);
      }
  }
  uint32_t R[8];  // R[2 y + d]: d = 0: dx 0, 2; d = 1: dx 1, 3
#pragma unroll
  for (int y = 0; y < 4; y++) {
    R[2 * y] = E[y];
    R[2 * y + 1] = O[y] - ((E[y] >> 16) << 8);
  }
  rs_step<8, 1>(R, lane & 1);
  rs_step<4, 2>(R, lane & 2);
  rs_step<2, 4>(R, lane & 4);
  uint32_t V[2] = {R[0] & 0xffffu, R[0] >> 16};
  rs_step<2, 8>(V, lane & 8);
  V[0] = add_xor<16>(V[0]);
  V[0] = add_xor<32>(V[0]);
  *dy = ((lane >> 1) & 1) + 2 * ((lane >> 2) & 1);
  *dx = (lane & 1) + 2 * ((lane >> 3) & 1);
  return V[0];
}

// whole 8 x 8 block (Y, X): eight 12-byte row loads per point; lane l holds the sum of pose (*dy, *dx) of the block
__device__ __forceinline__ uint32_t block_sums8(__amdgpu_buffer_rsrc_t rsrc, uint32_t pitch, uint32_t copy_bytes, const uint32_t *org,
                                                int32_t nch, int32_t Y, int32_t X, int lane, int *dy, int *dx) {
  const uint32_t roff = (uint32_t)(BNB_B * Y), coff = (uint32_t)(BNB_B * X);
  const uint32_t wrap = pitch * HI_TILE_BYTES - HI_TILE_BYTES;  // from a tile's last row to the next tile's first
  // (one chunk's eight row loads in flight: with two the 32 accumulators + 48 row registers spill, measured 5 % slower)
  constexpr int U = 1;
  uint32_t E[8][2], O[8][2];
#pragma unroll
  for (int y = 0; y < 8; y++) E[y][0] = E[y][1] = O[y][0] = O[y][1] = 0u;
#pragma unroll
  for (int r = 0; r < OC / U; r++) {
    if (U * r >= nch) continue;
    // rows in groups of ROWS per chunk: 8 -> all eight 12-byte loads of a chunk in flight (24 registers), 4 -> two
    // groups of four (12 registers: with the 32 accumulators the kernel then stays inside its 128 registers)
    constexpr int ROWS = 4;
    uint32_t gg[U], sh[U], cn[U], qq[U];
#pragma unroll
    for (int j = 0; j < U; j++) {
      const uint32_t o = origin_of(org, U * r + j);
      cn[j] = org_cnt(o);
      // (12 bytes from a 4-aligned column: the copy in which they start in a tile's first half)
      const uint32_t row0 = org_row(o) + roff, col0 = org_col(o) + coff, col4 = col0 & ~3u;
      qq[j] = row0 & 7u;
      gg[j] = hi_tiled(row0, col4, (col4 >> 3) & 1u, pitch, copy_bytes);
      sh[j] = (col0 & 3u) * 8u;
    }
#pragma unroll
    for (int y0 = 0; y0 < 8; y0 += ROWS) {
      u32x3 w[U][ROWS];
#pragma unroll
      for (int j = 0; j < U; j++)
#pragma unroll
        for (int y = 0; y < ROWS; y++)
          w[j][y] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)(gg[j] + (qq[j] + (uint32_t)(y0 + y) >= 8u ? wrap : 0u) + 16u * (uint32_t)(y0 + y)), 0, 0);
#pragma unroll
      for (int j = 0; j < U; j++)
#pragma unroll
        for (int y = 0; y < ROWS; y++) {
          const uint32_t n0 = __builtin_amdgcn_alignbit(w[j][y].y, w[j][y].x, sh[j]);
          const uint32_t n1 = __builtin_amdgcn_alignbit(w[j][y].z, w[j][y].y, sh[j]);
          E[y0 + y][0] += __umul24(n0 & M8, cn[j]); O[y0 + y][0] += __umul24(n0 >> 8, cn[j]);
          E[y0 + y][1] += __umul24(n1 & M8, cn[j]); O[y0 + y][1] += __umul24(n1 >> 8, cn[j]);
        }
    }
  }
  uint32_t R[32];  // R[4 y + d]: d = 0: dx 0, 2; 1: dx 1, 3; 2: dx 4, 6; 3: dx 5, 7
#pragma unroll
  for (int y = 0; y < 8; y++) {
    R[4 * y + 0] = E[y][0];
    R[4 * y + 1] = O[y][0] - ((E[y][0] >> 16) << 8);
    R[4 * y + 2] = E[y][1];
    R[4 * y + 3] = O[y][1] - ((E[y][1] >> 16) << 8);
  }
  rs_step<32, 1>(R, lane & 1);
  rs_step<16, 2>(R, lane & 2);
  rs_step<8, 4>(R, lane & 4);
  uint32_t V[8];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    V[2 * i] = R[i] & 0xffffu;
    V[2 * i + 1] = R[i] >> 16;
  }
  rs_step<8, 8>(V, lane & 8);
  rs_step<4, 16>(V, lane & 16);
  rs_step<2, 32>(V, lane & 32);
  const int r = 8 * (2 * ((lane >> 5) & 1) + ((lane >> 4) & 1)) + 4 * ((lane >> 2) & 1) + 2 * ((lane >> 1) & 1) + (lane & 1);
  const int f = (lane >> 3) & 1, d = r & 3;
  *dy = r >> 2;
  *dx = 4 * (d >> 1) + (d & 1) + 2 * f;
  return V[0];
}

// Two 4 x 4 sub-blocks side by side in ONE pass: the 4 rows x 8 pose columns from row 8 Y + 4 sy, column 8 X + 4 sx0 on --
// sub-blocks (sy, 0) and (sy, 1) of block (Y, X) for sx0 = 0, or (sy, 1) of it and (sy, 0) of block (Y, X + 1) for sx0 = 1.
// The 12-byte row load block_sums8 issues covers both (sub_sums8's 8 bytes: one), so the pair costs four row loads per
// chunk, one origin decode and one reduction where two passes of sub_sums8 cost eight, two and two.  One group of four rows
// exactly as block_sums8's (the same choice of copy: 12 bytes from a 4-aligned column start in a tile's first half in one
// of the two), 16 packed accumulators, 12 row registers.  Lane l holds the sum of pose (*dy in 0..3, *dx in 0..7) of the
// window; lanes 32.. hold copies of lanes 0..31.
__device__ __forceinline__ uint32_t pair_sums8(__amdgpu_buffer_rsrc_t rsrc, uint32_t pitch, uint32_t copy_bytes, const uint32_t *org,
                                               int32_t nch, int32_t Y, int32_t X, int32_t sy, int32_t sx0, int lane, int *dy, int *dx) {
  const uint32_t roff = (uint32_t)(BNB_B * Y + BNB_B4 * sy), coff = (uint32_t)(BNB_B * X + BNB_B4 * sx0);
  const uint32_t wrap = pitch * HI_TILE_BYTES - HI_TILE_BYTES;  // from a tile's last row to the next tile's first
  // (the fields of block_sums8: a byte sum per 16-bit field through the three packed steps, i.e. over 8 lanes, which hold
  //  at most 257 points -- cache_origins -- of at most 255 each; 32 bits from the unpack on)
  static_assert(257u * 255u <= 0xffffu, "a packed field holds the byte sums of the 8 lanes it is reduced over");
  uint32_t E[4][2], O[4][2];
#pragma unroll
  for (int y = 0; y < 4; y++) E[y][0] = E[y][1] = O[y][0] = O[y][1] = 0u;
#pragma unroll
  for (int r = 0; r < OC; r++) {
    if (r >= nch) continue;
    const uint32_t o = origin_of(org, r);
    const uint32_t cn = org_cnt(o);
    const uint32_t row0 = org_row(o) + roff, col0 = org_col(o) + coff, col4 = col0 & ~3u;
    const uint32_t q = row0 & 7u, sh = (col0 & 3u) * 8u;
    const uint32_t g = hi_tiled(row0, col4, (col4 >> 3) & 1u, pitch, copy_bytes);
    u32x3 w[4];
#pragma unroll
    for (int y = 0; y < 4; y++)
      w[y] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)(g + (q + (uint32_t)y >= 8u ? wrap : 0u) + 16u * (uint32_t)y), 0, 0);
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const uint32_t n0 = __builtin_amdgcn_alignbit(w[y].y, w[y].x, sh);
      const uint32_t n1 = __builtin_amdgcn_alignbit(w[y].z, w[y].y, sh);
      E[y][0] += __umul24(n0 & M8, cn); O[y][0] += __umul24(n0 >> 8, cn);
      E[y][1] += __umul24(n1 & M8, cn); O[y][1] += __umul24(n1 >> 8, cn);
    }
  }
  uint32_t R[16];  // R[4 y + d]: d = 0: dx 0, 2; 1: dx 1, 3; 2: dx 4, 6; 3: dx 5, 7
#pragma unroll
  for (int y = 0; y < 4; y++) {
    R[4 * y + 0] = E[y][0];
    R[4 * y + 1] = O[y][0] - ((E[y][0] >> 16) << 8);
    R[4 * y + 2] = E[y][1];
    R[4 * y + 3] = O[y][1] - ((E[y][1] >> 16) << 8);
  }
  rs_step<16, 1>(R, lane & 1);
  rs_step<8, 2>(R, lane & 2);
  rs_step<4, 4>(R, lane & 4);
  uint32_t V[4] = {R[0] & 0xffffu, R[0] >> 16, R[1] & 0xffffu, R[1] >> 16};
  rs_step<4, 8>(V, lane & 8);
  rs_step<2, 16>(V, lane & 16);
  V[0] = add_xor<32>(V[0]);
  const int r = 8 * ((lane >> 4) & 1) + 4 * ((lane >> 2) & 1) + 2 * ((lane >> 1) & 1) + (lane & 1);
  const int f = (lane >> 3) & 1, d = r & 3;
  *dy = r >> 2;
  *dx = 4 * (d >> 1) + (d & 1) + 2 * f;
  return V[0];
}

// ---- the same three sums over SOME chunks of the list (the candidates' kernels) ----------------------------------
// `mask` (wave-uniform): bit c set = chunk c of the cell list is visited.  The caller leaves out only chunks whose every
// entry reads nothing but zero cells for the poses of the pass (nhip_bnb.hip chunk_mask), so each sum is what the functions
// above return over chunks 0 .. nch - 1, bit for bit.  The loops are rolled walks over the set bits -- lowest bit, clear it,
// the entry at org + 64 c -- where those are unrolled over OC chunks with static offsets: a third of their code.
// sub_sums8 keeps its two chunks in flight per turn (an odd last chunk has a turn of its own: no load is issued for a
// chunk that is not there), pair_sums8 takes two as well, block_sums8 its one chunk in two groups of four rows.
__device__ __forceinline__ int next_chunk(uint32_t &mask) {
  const int c = (int)__builtin_ctz(mask);
  mask &= mask - 1u;
  return c;
}

__device__ __forceinline__ uint32_t sub_sums8_masked(__amdgpu_buffer_rsrc_t rsrc, uint32_t pitch, uint32_t copy_bytes, const uint32_t *org,
                                                     uint32_t mask, int32_t Y, int32_t X, int32_t sy, int32_t sx, int lane, int *dy, int *dx) {
  const uint32_t roff = (uint32_t)(BNB_B * Y + BNB_B4 * sy), coff = (uint32_t)(BNB_B * X + BNB_B4 * sx);
  const uint32_t wrap = pitch * HI_TILE_BYTES - HI_TILE_BYTES;  // from a tile's last row to the next tile's first
  uint32_t E[4] = {0u, 0u, 0u, 0u}, O[4] = {0u, 0u, 0u, 0u};
  auto load = [&](int c, u32x2 (&w)[4], uint32_t &sh, uint32_t &cn) {
    const uint32_t o = org[64 * c];
    cn = org_cnt(o);
    const uint32_t row0 = org_row(o) + roff, col0 = org_col(o) + coff, col4 = col0 & ~3u;
    const uint32_t cp = (col4 >> 3) & 1u, q = row0 & 7u;
    const uint32_t v0 = hi_tiled(row0, col4, cp, pitch, copy_bytes);
    sh = (col0 & 3u) * 8u;
#pragma unroll
    for (int y = 0; y < 4; y++)
      w[y] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(v0 + (q + (uint32_t)y >= 8u ? wrap : 0u) + 16u * (uint32_t)y), 0, 0);
  };
  auto add = [&](const u32x2 (&w)[4], uint32_t sh, uint32_t cn) {
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const uint32_t n = __builtin_amdgcn_alignbit(w[y].y, w[y].x, sh);
      E[y] += __umul24(n & M8, cn);
      O[y] += __umul24(n >> 8, cn);
    }
  };
#pragma unroll 1
  while ((mask & (mask - 1u)) != 0u) {  // two chunks or more are left
    u32x2 wa[4], wb[4];
    uint32_t sa, sb, ca, cb;
    load(next_chunk(mask), wa, sa, ca);
    load(next_chunk(mask), wb, sb, cb);
    add(wa, sa, ca);
    add(wb, sb, cb);
  }
  if (mask != 0u) {
    u32x2 wa[4];
    uint32_t sa, ca;
    load(next_chunk(mask), wa, sa, ca);
    add(wa, sa, ca);
  }
  uint32_t R[8];  // R[2 y + d]: d = 0: dx 0, 2; d = 1: dx 1, 3
#pragma unroll
  for (int y = 0; y < 4; y++) {
    R[2 * y] = E[y];
    R[2 * y + 1] = O[y] - ((E[y] >> 16) << 8);
  }
  rs_step<8, 1>(R, lane & 1);
  rs_step<4, 2>(R, lane & 2);
  rs_step<2, 4>(R, lane & 4);
  uint32_t V[2] = {R[0] & 0xffffu, R[0] >> 16};
  rs_step<2, 8>(V, lane & 8);
  V[0] = add_xor<16>(V[0]);
  V[0] = add_xor<32>(V[0]);
  *dy = ((lane >> 1) & 1) + 2 * ((lane >> 2) & 1);
  *dx = (lane & 1) + 2 * ((lane >> 3) & 1);
  return V[0];
}

__device__ __forceinline__ uint32_t block_sums8_masked(__amdgpu_buffer_rsrc_t rsrc, uint32_t pitch, uint32_t copy_bytes, const uint32_t *org,
                                                       uint32_t mask, int32_t Y, int32_t X, int lane, int *dy, int *dx) {
  const uint32_t roff = (uint32_t)(BNB_B * Y), coff = (uint32_t)(BNB_B * X);
  const uint32_t wrap = pitch * HI_TILE_BYTES - HI_TILE_BYTES;  // from a tile's last row to the next tile's first
  uint32_t E[8][2], O[8][2];
#pragma unroll
  for (int y = 0; y < 8; y++) E[y][0] = E[y][1] = O[y][0] = O[y][1] = 0u;
#pragma unroll 1
  while (mask != 0u) {
    constexpr int ROWS = 4;  // (as block_sums8: two groups of four rows)
    const uint32_t o = org[64 * next_chunk(mask)];
    const uint32_t cn = org_cnt(o);
    const uint32_t row0 = org_row(o) + roff, col0 = org_col(o) + coff, col4 = col0 & ~3u;
    const uint32_t q = row0 & 7u, sh = (col0 & 3u) * 8u;
    const uint32_t g = hi_tiled(row0, col4, (col4 >> 3) & 1u, pitch, copy_bytes);
#pragma unroll
    for (int y0 = 0; y0 < 8; y0 += ROWS) {
      u32x3 w[ROWS];
#pragma unroll
      for (int y = 0; y < ROWS; y++)
        w[y] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)(g + (q + (uint32_t)(y0 + y) >= 8u ? wrap : 0u) + 16u * (uint32_t)(y0 + y)), 0, 0);
#pragma unroll
      for (int y = 0; y < ROWS; y++) {
        const uint32_t n0 = __builtin_amdgcn_alignbit(w[y].y, w[y].x, sh);
        const uint32_t n1 = __builtin_amdgcn_alignbit(w[y].z, w[y].y, sh);
        E[y0 + y][0] += __umul24(n0 & M8, cn); O[y0 + y][0] += __umul24(n0 >> 8, cn);
        E[y0 + y][1] += __umul24(n1 & M8, cn); O[y0 + y][1] += __umul24(n1 >> 8, cn);
      }
    }
  }
  uint32_t R[32];  // R[4 y + d]: d = 0: dx 0, 2; 1: dx 1, 3; 2: dx 4, 6; 3: dx 5, 7
#pragma unroll
  for (int y = 0; y < 8; y++) {
    R[4 * y + 0] = E[y][0];
    R[4 * y + 1] = O[y][0] - ((E[y][0] >> 16) << 8);
    R[4 * y + 2] = E[y][1];
    R[4 * y + 3] = O[y][1] - ((E[y][1] >> 16) << 8);
  }
  rs_step<32, 1>(R, lane & 1);
  rs_step<16, 2>(R, lane & 2);
  rs_step<8, 4>(R, lane & 4);
  uint32_t V[8];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    V[2 * i] = R[i] & 0xffffu;
    V[2 * i + 1] = R[i] >> 16;
  }
  rs_step<8, 8>(V, lane & 8);
  rs_step<4, 16>(V, lane & 16);
  rs_step<2, 32>(V, lane & 32);
  const int r = 8 * (2 * ((lane >> 5) & 1) + ((lane >> 4) & 1)) + 4 * ((lane >> 2) & 1) + 2 * ((lane >> 1) & 1) + (lane & 1);
  const int f = (lane >> 3) & 1, d = r & 3;
  *dy = r >> 2;
  *dx = 4 * (d >> 1) + (d & 1) + 2 * f;
  return V[0];
}

__device__ __forceinline__ uint32_t pair_sums8_masked(__amdgpu_buffer_rsrc_t rsrc, uint32_t pitch, uint32_t copy_bytes, const uint32_t *org,
                                                      uint32_t mask, int32_t Y, int32_t X, int32_t sy, int32_t sx0, int lane, int *dy, int *dx) {
  const uint32_t roff = (uint32_t)(BNB_B * Y + BNB_B4 * sy), coff = (uint32_t)(BNB_B * X + BNB_B4 * sx0);
  const uint32_t wrap = pitch * HI_TILE_BYTES - HI_TILE_BYTES;  // from a tile's last row to the next tile's first
  uint32_t E[4][2], O[4][2];
#pragma unroll
  for (int y = 0; y < 4; y++) E[y][0] = E[y][1] = O[y][0] = O[y][1] = 0u;
  auto load = [&](int c, u32x3 (&w)[4], uint32_t &sh, uint32_t &cn) {
    const uint32_t o = org[64 * c];
    cn = org_cnt(o);
    const uint32_t row0 = org_row(o) + roff, col0 = org_col(o) + coff, col4 = col0 & ~3u;
    const uint32_t q = row0 & 7u;
    sh = (col0 & 3u) * 8u;
    const uint32_t g = hi_tiled(row0, col4, (col4 >> 3) & 1u, pitch, copy_bytes);
#pragma unroll
    for (int y = 0; y < 4; y++)
      w[y] = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)(g + (q + (uint32_t)y >= 8u ? wrap : 0u) + 16u * (uint32_t)y), 0, 0);
  };
  auto add = [&](const u32x3 (&w)[4], uint32_t sh, uint32_t cn) {
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const uint32_t n0 = __builtin_amdgcn_alignbit(w[y].y, w[y].x, sh);
      const uint32_t n1 = __builtin_amdgcn_alignbit(w[y].z, w[y].y, sh);
      E[y][0] += __umul24(n0 & M8, cn); O[y][0] += __umul24(n0 >> 8, cn);
      E[y][1] += __umul24(n1 & M8, cn); O[y][1] += __umul24(n1 >> 8, cn);
    }
  };
#pragma unroll 1
  while ((mask & (mask - 1u)) != 0u) {  // two chunks or more are left
    u32x3 wa[4], wb[4];
    uint32_t sa, sb, ca, cb;
    load(next_chunk(mask), wa, sa, ca);
    load(next_chunk(mask), wb, sb, cb);
    add(wa, sa, ca);
    add(wb, sb, cb);
  }
  if (mask != 0u) {
    u32x3 wa[4];
    uint32_t sa, ca;
    load(next_chunk(mask), wa, sa, ca);
    add(wa, sa, ca);
  }
  uint32_t R[16];  // R[4 y + d]: d = 0: dx 0, 2; 1: dx 1, 3; 2: dx 4, 6; 3: dx 5, 7
#pragma unroll
  for (int y = 0; y < 4; y++) {
    R[4 * y + 0] = E[y][0];
    R[4 * y + 1] = O[y][0] - ((E[y][0] >> 16) << 8);
    R[4 * y + 2] = E[y][1];
    R[4 * y + 3] = O[y][1] - ((E[y][1] >> 16) << 8);
  }
  rs_step<16, 1>(R, lane & 1);
  rs_step<8, 2>(R, lane & 2);
  rs_step<4, 4>(R, lane & 4);
  uint32_t V[4] = {R[0] & 0xffffu, R[0] >> 16, R[1] & 0xffffu, R[1] >> 16};
  rs_step<4, 8>(V, lane & 8);
  rs_step<2, 16>(V, lane & 16);
  V[0] = add_xor<32>(V[0]);
  const int r = 8 * ((lane >> 4) & 1) + 4 * ((lane >> 2) & 1) + 2 * ((lane >> 1) & 1) + (lane & 1);
  const int f = (lane >> 3) & 1, d = r & 3;
  *dy = r >> 2;
  *dx = 4 * (d >> 1) + (d & 1) + 2 * f;
  return V[0];
}

// ---- 16-bit cells: a pose's exact sum from the stored image -------------------------------------------------
// sum over the scan's points of the 16-bit cell that pose (ix, iy) of the rotation reads: one 2-byte load per point
__device__ __forceinline__ uint32_t pose_sum16(const BnbParams &P, __amdgpu_buffer_rsrc_t rsrc16, const uint32_t *org,
                                               int32_t nch, int32_t ix, int32_t iy) {
  // (rsrc16: the tiled copy of the 16-bit image -- one cell per point, neighbours along a wall in the same lines)
  uint32_t acc = 0u;  // (17 chunks * 65535 fits)
#pragma unroll
  for (int c = 0; c < OCL; c++) {
    if (c >= nch) continue;
    const uint32_t o = origin_of(org, c);
    acc += org_cnt(o) * (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(
                            rsrc16, (int)t16_tiled(org_row(o) + (uint32_t)iy, org_col(o) + (uint32_t)ix, (uint32_t)P.t16_tpr), 0, 0);
  }
  return wave_sum(acc);
}
// ... over the chunks of `mask` (as above: a chunk left out adds 0; the loads stay unrolled, all in flight at once)
__device__ __forceinline__ uint32_t pose_sum16_masked(const BnbParams &P, __amdgpu_buffer_rsrc_t rsrc16, const uint32_t *org,
                                                      uint32_t mask, int32_t ix, int32_t iy) {
  uint32_t acc = 0u;
#pragma unroll
  for (int c = 0; c < OCL; c++) {
    if (((mask >> c) & 1u) == 0u) continue;
    const uint32_t o = origin_of(org, c);
    acc += org_cnt(o) * (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(
                            rsrc16, (int)t16_tiled(org_row(o) + (uint32_t)iy, org_col(o) + (uint32_t)ix, (uint32_t)P.t16_tpr), 0, 0);
  }
  return wave_sum(acc);
}

// Two stages for 16-bit cells. `hsum` is the lane's pose sum over the plane of HIGH bytes (what sub_sums8 /
// block_sums8 return on that plane, at the cost of 8-bit cells); a cell is 256 * high + low with low <= 255, so
//     256 * hsum + 255 * points  >=  the pose's 16-bit sum.
// Only poses whose bound reaches the best sum found so far can hold the optimum or a tie with it; their exact sums
// are read from the 16-bit image, highest bound first (it raises the best fastest), until no pose of the block is
// left above it.  Near the optimum that is a handful of poses; elsewhere none.  Returns the number evaluated.
// MASKED: the poses' sums are taken over the chunks of `mask`, the mask of the pass that gave `hsum` -- it keeps every
// chunk that holds a cell that is not zero for any pose of the pass, 16-bit cell or high byte alike (the level-2 byte of a
// 16-bit grid is ceil(max / 257): zero only where every cell is).  The bound keeps the scan's point count.
template <bool GLOBAL, bool MASKED = false>
__device__ __forceinline__ uint32_t refine16(const BnbParams &P, __amdgpu_buffer_rsrc_t rsrc16, const uint32_t *org,
                                             int32_t nch, int32_t n_pts, int32_t k, int32_t ix, int32_t iy, uint32_t hsum,
                                             bool mine, int lane, unsigned long long *best, uint32_t &bcopy,
                                             uint32_t mask = 0u) {
  const bool valid = mine && ix < P.nx && iy < P.ny;
  uint32_t ub = valid ? 256u * hsum + 255u * (uint32_t)n_pts : 0u;  // (points <= 1088: no overflow)
  uint32_t n_eval = 0u;
  for (;;) {
    const uint32_t top = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max(ub));
    if (top == 0u || top < best_sum_cached<GLOBAL>(best, bcopy)) break;
    const int j = (int)__builtin_ctzll(__ballot(ub == top));  // (top != 0: a lane holds it)
    const int32_t jx = __builtin_amdgcn_readlane(ix, j), jy = __builtin_amdgcn_readlane(iy, j);
    const uint32_t sum = MASKED ? pose_sum16_masked(P, rsrc16, org, mask, jx, jy) : pose_sum16(P, rsrc16, org, nch, jx, jy);
    const uint32_t lin = (uint32_t)((k * P.nx + jx) * P.ny + jy);
    const unsigned long long key = ((unsigned long long)sum << 32) | (0xffffffffu - lin);
    wave_atomic_max(best, key, lane);  // (generic address: LDS or global)
    if (GLOBAL) bcopy = max(bcopy, sum);
    if (lane == j) ub = 0u;
    n_eval++;
  }
  return n_eval;
}

}  // namespace
}  // namespace nhip
