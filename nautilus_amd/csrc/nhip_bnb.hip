// nhip_bnb.hip -- K2 + K3 by branch and bound: the argmax (and its sum) of the exhaustive (theta, x, y)
// correlation, without performing most of its adds.
//
// Replaces CorrelativeScanMatcher::GetTransformation (call site src/optimization/solver.cc:633-638), batched
// over candidate pairs, with exactly the result of csm_correlate_kernel (nhip_csm.hip): maximum integer sum,
// ties to the smallest linear index (k * nx + ix) * ny + iy.
//
// Bound: the plane of translations of one rotation is cut into 8 x 8 blocks (Y, X).  A point whose window origin
// (top-left lookup cell) is (r, c) reads, for the 64 poses of block (Y, X), stored cells in rows
// [r + 8Y, r + 8Y + 8) and columns [c + 8X, c + 8X + 8), all inside the 15 x 15 cells that the pooled entry
// pool[(r >> 3) + Y][(c >> 3) + X] covers (nhip_grid_tables.hip).  So U(k, Y, X) = sum over points of that entry is an
// upper bound of every sum in the block (16-bit cells: 257 * U, the pool holds ceil(max / 257)).
// Search: (1) U for all blocks of all rotations -- a gather of 11 x 11 bytes per RUN of points that share a pooled
// entry (consecutive beams do: run-length compression cuts the gathers ~5x) from the LDS-resident pooled table;
// (2) every wave evaluates its highest-bound block exactly, which gives a lower bound `best` of the optimum;
// (3) rotation by rotation, best first: every block with U >= best's sum is refined through the bounds of its four
// 4 x 4 sub-blocks (second table, pooled over 7 x 7 cells at stride 4: one 16-byte read per point serves a strip of
// three neighbouring blocks) and exact sums are gathered from the stored grid only for the sub-blocks whose bound
// still reaches `best`, which rises as it goes.  Blocks and sub-blocks with a bound below best's sum cannot hold the
// optimum, nor a tie with it, and are never touched.  Nor are the sub-blocks that hold no pose of the lattice: a side that
// is no multiple of 8 (81 = 8 * 10 + 1) leaves the last block column / row with 1 .. 7 pose columns / rows, and the sub-blocks
// beyond them -- 43 of a rotation's 484 at 81 x 81 -- carry the HIGHEST bounds of a landscape that rises towards the window's
// edge while nothing in them can raise `best`; they are neither counted as alive nor evaluated (block_extent, sub_valid).
// On the 1081-beam workload 0.36 % of the poses are evaluated.
//
// Parallelisation is the transpose of the exhaustive kernel's: LANES ARE POINTS (one point per lane and
// 64-point chunk), REGISTERS ARE POSES -- byte sums SWAR-packed two per register -- and one transposing
// reduction (reduce-scatter over the 64 lanes) per rotation / block turns 64 partial sums per pose into one
// total per lane.  All sums are integers: order-independent, bit-exact against the oracle.
//
// One 512-thread workgroup per pair; waves take rotations k = wave, wave + 8, ...; LDS holds the target's
// pooled table (36 KB at 1200 x 1200) and the bounds (n_theta x 128 dwords).
//
// Kernels.  csm_bnb_kernel<CB, POOL_LDS, BY_ROT, SPLIT>: steps (1)-(3) for one pair (the fused form), or with SPLIT
// steps (1)-(2) only, leaving the pair's rows of bounds in the caller's workspace; csm_bnb_order_kernel +
// csm_bnb_cand_kernel<CB>: step (3) of all pairs of a list as a launch of its own (the split form: lists of 6,144 to
// 65,536 pairs -- the first part's workgroups all take the same time, the candidates' vary 100-fold and the heaviest
// pairs are shared by several workgroups); csm_bnb_rot_kernel<CB>: rotations handed over by pairs with flat landscapes
// in small batches.  Exact sums of 16-bit grids run on the plane of high bytes (256 sum(hi) + 255 n bounds a pose's sum;
// only the poses that bound admits read 16-bit cells), which -- like the copy of the cells those reads use -- is stored
// in tiles of one cache line, because what a gather costs here is the number of distinct lines per load.  The two kernels
// that keep a rotation's runs by level-2 entry (candidates, hand-over) take their exact sums only over the 64-entry chunks
// of the origin list in which some entry's level-2 byte says a cell can be non-zero for the poses of the pass (chunk_mask).
//
// This file: candidate processing, the kernels, their launchers.  What they are built from lies in headers that only
// this file includes: nhip_bnb_wave.h (lane exchanges, wave reductions), nhip_bnb_origin.h (window origins),
// nhip_bnb_bounds.h (the three bounds), nhip_bnb_exact.h (the exact sums); nhip_bnb_params.h has the parameters and
// the layout of csm_bnb_kernel's LDS, which the host side shares.
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

// This file is compiled twice.  NHIP_BNB_INSTR = 0 (nhip_bnb.hip itself): the product kernels -- no statistics, no
// timestamps, no debug switches in the code -- and the host side.  NHIP_BNB_INSTR = 1 (nhip_bnb_instr.hip includes this
// file): the same kernels with the instrumentation compiled in, launched only when NHIP_BNB_INSTRUMENT=1 is set in
// the environment (tools/bnb_*.py, the tests that count evaluated blocks, bench.py's algorithm.stats).
#ifndef NHIP_BNB_INSTR
#define NHIP_BNB_INSTR 0
#endif
// (The compile-time measurement switches of rounds 2-4 -- lane exchanges through ds_bpermute, runs cut at 8 / 16 lanes,
//  unaligned row loads, highest-bound-first order, unmerged origin lists, per-lane nesting and double-precision forms of
//  the window origins, the row-major 8-bit plane, unaligned LDS reads, the v_fract near test, run lengths at the heads --
//  are out of the source: each lost its A/B, the numbers are in profiles/r03_matcher_experiments.txt and
//  profiles/r04_bounds_variants.txt, the code in the commits those files name.  What is left is what ships.)
#if NHIP_BNB_INSTR
#define csm_bnb_kernel csm_bnb_kernel_instr          // (their own names in profiles)
#define csm_bnb_rot_kernel csm_bnb_rot_kernel_instr
#define launchers_product launchers_instr
#define BNB_STATS(P) ((P).stats)
#define BNB_TIMELINE(P) ((P).timeline)
#else
#define BNB_STATS(P) (static_cast<unsigned long long *>(nullptr))
#define BNB_TIMELINE(P) (static_cast<unsigned long long *>(nullptr))
#endif

// (behind the macros above: the headers are compiled in both builds)
#include "nhip_bnb_params.h"
#include "nhip_bnb_wave.h"
#include "nhip_bnb_origin.h"
#include "nhip_bnb_bounds.h"
#include "nhip_bnb_exact.h"

namespace nhip {

namespace {

using namespace bnb;

constexpr int BNB_THREADS = 64 * BNB_WAVES;

// ---- one candidate block: refine through the sub-block bounds, or evaluate whole --------------------------
// `best` is the pair's running best key (LDS of the pair's workgroup, or keys[pair] in global memory for the
// rotations handed to the second kernel).  A sub-block is skipped only if its bound is below the best SUM found so far: it cannot hold
// the optimum nor a tie with it.  n[0] whole blocks evaluated, n[1] candidates refined, n[2] sub-blocks evaluated,
// n[3] poses of 16-bit grids read exactly; at the lattice's edge (blocks with fewer than 8 pose columns or rows): n[4] such
// blocks refined, n[5] sub-blocks evaluated that hold no pose (stays 0), n[6] such blocks evaluated whole (only ones with
// more than 4 pose columns and rows can be); n[7] passes that took two sub-blocks side by side at once (each adds 2 to
// n[2]), n[8] those of them that reach across a block boundary; the kernels that keep a run list: n[9] chunks of the cell
// list a pass of exact sums on the 8-bit plane would visit without the chunk masks (the list's chunks per pass), n[10]
// chunks visited; n[11], n[12] the same two for the poses of 16-bit grids read exactly.
constexpr int N_WORK = 13;
struct PairCtx {
  const uint8_t *grid;
  const float2 *pts;
  int32_t n_pts, cx, cy, pair;
};

// ---- which chunks of the cell list a pass of exact sums must visit
// An entry of the cell list adds nothing to any pose of a sub-block whose level-2 byte is 0 for it: that byte is the
// maximum (16-bit grids: ceil(max / 257)) over the 7 x 7 cells that hold every window the sub-block's poses read from any
// origin inside the entry's 4 x 4 level-2 entry.  The strip bounds load exactly those bytes, per RUN of the list (runs of
// consecutive entries with one level-2 entry), and leave per run the twelve-bit set of the strip's bytes that are not
// zero (`note`, nhip_bnb_bounds.h strip_sums); cache_origins left per run the chunks of the cell list its cells lie in
// (`span`: first chunk | reaches the next << 5).  A pass over the sub-blocks `fields` (bits 4 t + sy + 2 sx) visits the
// chunks of the runs that have one of those bytes set -- a superset of the chunks that hold a cell that is not zero -- so
// every sum is the full list's.  nrc <= 0 (no usable run list, or P.zero_chunks off): every chunk, `full`.
struct ChunkNotes {
  const uint16_t *note;  // the lane's word of run chunk 0
  const uint8_t *span;   // the lane's byte of run chunk 0
  int32_t nrc;           // chunks of the run list (wave-uniform)
  uint32_t full;         // (1 << chunks of the cell list) - 1
};
__device__ __forceinline__ uint32_t chunk_mask(const ChunkNotes &N, uint32_t fields) {
  if (N.nrc <= 0) return N.full;
  uint32_t acc = 0u;
#pragma unroll
  for (int j = 0; j < RUN_CHUNKS; j++) {
    // (both reads lie inside the wave's arrays whatever nrc is; past it the words are stale and not used)
    const uint32_t f = N.note[64 * j], s = N.span[64 * j];
    const uint32_t chunks = (1u + ((s >> 5) << 1)) << (s & 31u);
    acc |= (j < N.nrc && (f & fields) != 0u) ? chunks : 0u;
  }
  return wave_or(acc) & N.full;
}

template <int CB>
__device__ __forceinline__ void process_candidate(const BnbParams &P, const PairCtx &C, int32_t k, int32_t v, int lane,
                                                  unsigned long long *best, uint32_t (&n)[N_WORK]) {
  const int Y = v / NB, X = v - NB * Y;  // v: block index NB * Y + X
  const int32_t vx = block_extent(P.nx, X), vy = block_extent(P.ny, Y);
  const bool edge = vx < BNB_B || vy < BNB_B;
  float cf, sf;
  rotation_k(P, C.pair, k, &cf, &sf);
  if (P.levels >= 2) {
    const __amdgpu_buffer_rsrc_t p4 = uniform_rsrc(C.grid + P.grid_bytes + P.skip_bytes + P.pool_bytes, P.pool4_bytes);
    uint32_t sb[4];
    sub_bounds(P, p4, C.pts, C.n_pts, cf, sf, C.cx, C.cy, Y, X, lane, CB == 1 ? 1u : 257u, sb);
    n[1]++;
    n[4] += edge ? 1u : 0u;
    const uint32_t bsum = best_sum<false>(best);
    int alive = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) alive += (sub_valid(vy, vx, q >> 1, q & 1) && sb[q] != 0u && sb[q] >= bsum) ? 1 : 0;  // (as process_candidate_c)
    if (alive == 0) return;
    if (alive <= 2) {
      const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(C.grid, P.grid_bytes + P.skip_bytes);
#pragma unroll 1
      for (int q = 0; q < 4; q++) {
        const uint32_t b = q == 0 ? sb[0] : (q == 1 ? sb[1] : (q == 2 ? sb[2] : sb[3]));  // (no indexed array: scratch)
        if (!sub_valid(vy, vx, q >> 1, q & 1) || b == 0u || b < best_sum<false>(best)) continue;
        const unsigned long long key = eval_sub<CB>(P, rsrc, C.pts, C.n_pts, cf, sf, C.cx, C.cy, k, Y, X, q >> 1, q & 1, lane);
        wave_atomic_max(best, key, lane);
        n[2]++;
        n[5] += sub_valid(vy, vx, q >> 1, q & 1) ? 0u : 1u;
      }
      return;
    }
  }
  const unsigned long long key = eval_block<CB>(P, C.grid, C.pts, C.n_pts, cf, sf, C.cx, C.cy, k, Y, X, lane);
  wave_atomic_max(best, key, lane);
  n[0]++;
  n[6] += edge ? 1u : 0u;
}

// ... with the rotation's origins held by the wave and the block's four sub-block bounds at hand.  `rsrc` is the
// 8-bit plane the exact block sums are taken on (8-bit grids: the image; 16-bit grids: the plane of high bytes) and
// `pitch8` its pitch; `rsrc16` the 16-bit image (CB == 2).  ZC: the kernel keeps what chunk_mask needs (`CN`), and the
// exact sums walk the chunks it names.
template <int CB, bool GLOBAL, bool PAIR, bool ZC = false>
__device__ __forceinline__ void process_candidate_c(const BnbParams &P, __amdgpu_buffer_rsrc_t rsrc, uint32_t pitch8,  // (CB 2: tiles per row)
                                                    __amdgpu_buffer_rsrc_t rsrc16, const uint32_t *org, int32_t nch,
                                                    int32_t n_pts, int32_t k, int32_t Y, int32_t X,
                                                    uint32_t sb0, uint32_t sb1, uint32_t sb2, uint32_t sb3, int lane,
                                                    unsigned long long *best, uint32_t &bcopy, uint32_t (&n)[N_WORK],
                                                    int t, uint32_t &mk0, uint32_t &mk1,  // block t of its strip
                                                    const ChunkNotes &CN = ChunkNotes()) {
  const uint32_t bsum = best_sum_cached<GLOBAL>(best, bcopy);
  const int32_t vx = block_extent(P.nx, X), vy = block_extent(P.ny, Y);
  const bool edge = vx < BNB_B || vy < BNB_B;
  n[4] += edge ? 1u : 0u;
  // Only sub-blocks that hold a pose of the lattice count and are evaluated.  The others lie beyond the window's edge; a
  // landscape that rises towards it gives them the block's highest bounds, nothing they hold can raise the best, and so
  // nothing ever pruned them.  (Scalar: X and Y are.)  Sub-block q = 2 sy + sx.
  const bool ok0 = sub_valid(vy, vx, 0, 0), ok1 = sub_valid(vy, vx, 0, 1), ok2 = sub_valid(vy, vx, 1, 0), ok3 = sub_valid(vy, vx, 1, 1);
  const int alive = (ok0 && sb0 != 0u && sb0 >= bsum) + (ok1 && sb1 != 0u && sb1 >= bsum) + (ok2 && sb2 != 0u && sb2 >= bsum) +
                    (ok3 && sb3 != 0u && sb3 >= bsum);
  if (alive == 0) return;
  // a block with this many live sub-blocks is evaluated whole: one pass of 8 row loads per point instead of up to four
  // passes of 4, all 64 poses in one reduction (row-major planes: 2 beat 3, 7.70 -> 7.45 ms per 10,000 pairs; tiled planes:
  // loads are cheaper and 3 beats 2, 6.37 -> 6.22 ms).  A block at the lattice's edge with at most 4 pose columns or rows
  // (81 = 8 * 10 + 1) has at most two sub-blocks with a pose and never goes whole.
  constexpr int WHOLE_MIN = 3;
  if (alive >= WHOLE_MIN) {
    int dy, dx;
    // (ZC: a whole block's pass covers its four sub-blocks: the chunks of the runs with any of the block's four bytes set)
    const uint32_t visit = ZC ? chunk_mask(CN, 0xfu << (4 * t)) : 0u;
    const uint32_t total = ZC ? block_sums8_masked(rsrc, pitch8, (uint32_t)P.hi_copy_bytes, org, visit, Y, X, lane, &dy, &dx)
                              : block_sums8(rsrc, pitch8, (uint32_t)P.hi_copy_bytes, org, nch, Y, X, lane, &dy, &dx);
    const int32_t ix = BNB_B * X + dx, iy = BNB_B * Y + dy;
    if (ZC) {
      n[9] += (uint32_t)nch;
      n[10] += (uint32_t)__builtin_popcount(visit);
    }
    if (CB == 1) {
      const unsigned long long key = best_key(P, k, ix, iy, total, 32);
      wave_atomic_max(best, key, lane);  // (generic address: LDS or global)
      if (GLOBAL) bcopy = max(bcopy, (uint32_t)(key >> 32));
    } else {
      const uint32_t read = refine16<GLOBAL, ZC>(P, rsrc16, org, nch, n_pts, k, ix, iy, total, true, lane, best, bcopy, visit);
      n[3] += read;
      if (ZC) {
        n[11] += read * (uint32_t)nch;
        n[12] += read * (uint32_t)__builtin_popcount(visit);
      }
    }
    n[0]++;
    n[6] += __ballot(ix < P.nx && iy < P.ny) != ~0ull ? 1u : 0u;  // (from the poses themselves, not from the extents)
    return;
  }
  if (!PAIR) {  // one pass per sub-block, block by block
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
      const uint32_t b = q == 0 ? sb0 : (q == 1 ? sb1 : (q == 2 ? sb2 : sb3));
      if (!sub_valid(vy, vx, q >> 1, q & 1) || b == 0u || b < best_sum_cached<GLOBAL>(best, bcopy)) continue;
      int dy, dx;
      const uint32_t total = sub_sums8(rsrc, pitch8, (uint32_t)P.hi_copy_bytes, org, nch, Y, X, q >> 1, q & 1, lane, &dy, &dx);
      const int32_t ix = BNB_B * X + BNB_B4 * (q & 1) + dx, iy = BNB_B * Y + BNB_B4 * (q >> 1) + dy;
      if (CB == 1) {
        const unsigned long long key = best_key(P, k, ix, iy, total, 8);  // (lanes 16.. hold copies)
        wave_atomic_max(best, key, lane);
        if (GLOBAL) bcopy = max(bcopy, (uint32_t)(key >> 32));
      } else {
        n[3] += refine16<GLOBAL>(P, rsrc16, org, nch, n_pts, k, ix, iy, total, lane < 16, lane, best, bcopy);
      }
      n[2]++;
      n[5] += __ballot(ix < P.nx && iy < P.ny) == 0ull ? 1u : 0u;  // (from the poses themselves, not from sub_valid)
    }
    return;
  }
  // the live valid sub-blocks of a block that does not go whole: noted per sub-block row of the strip (bit 2 t + sx), taken
  // by strip_sub_blocks once the strip's blocks are through
  mk0 |= (uint32_t)((ok0 && sb0 != 0u && sb0 >= bsum) | ((ok1 && sb1 != 0u && sb1 >= bsum) << 1)) << (2 * t);
  mk1 |= (uint32_t)((ok2 && sb2 != 0u && sb2 >= bsum) | ((ok3 && sb3 != 0u && sb3 >= bsum) << 1)) << (2 * t);
}

// ... and the sub-blocks process_candidate_c noted: mk0 / mk1 over the strip's up to six sub-block columns c = 2 t + sx, for
// sy = 0 / 1; sb[4 t + 2 sy + sx] their bounds.  Each mask is walked from the left, every bound re-tested against the best
// right before its pass.  Two set neighbours whose bounds both still reach the best share ONE pass (pair_sums8: four row
// loads per chunk where two passes of sub_sums8 take eight) -- inside a block (c even) and, with PAIR_CROSS, across the
// boundary to the strip's next block (c odd); a sub-block without such a neighbour has its own pass.  Every pose evaluated is a
// pose of the lattice with its exact sum, every sub-block whose bound reaches the final best is still evaluated, and the
// keys are maxima: records and sums do not depend on the pairing.  P.pair_subs == 0: one pass per sub-block.
#ifndef NHIP_BNB_PAIR_CROSS
// (1: pairs across a block boundary too -- 30 % more pairs on the bench list, measured 0.01 - 0.03 ms faster than without,
//  which is inside the run-to-run spread: not shipped; profiles/r17_pair_passes.txt)
#define NHIP_BNB_PAIR_CROSS 0
#endif
constexpr bool PAIR_CROSS = NHIP_BNB_PAIR_CROSS != 0;
__device__ __forceinline__ uint32_t pick6(const uint32_t (&r)[6], int c) {  // (selects, not an indexed array: scratch)
  return c == 0 ? r[0] : (c == 1 ? r[1] : (c == 2 ? r[2] : (c == 3 ? r[3] : (c == 4 ? r[4] : r[5]))));
}
template <int CB, bool GLOBAL>
__device__ __forceinline__ void strip_sub_blocks(const BnbParams &P, __amdgpu_buffer_rsrc_t rsrc, uint32_t pitch8,
                                                 __amdgpu_buffer_rsrc_t rsrc16, const uint32_t *org, int32_t nch, int32_t n_pts,
                                                 int32_t k, int32_t Y, int32_t X0, const uint32_t (&sb)[12], uint32_t mk0,
                                                 uint32_t mk1, int lane, unsigned long long *best, uint32_t &bcopy,
                                                 uint32_t (&n)[N_WORK], const ChunkNotes &CN) {
#pragma unroll 1
  for (int sy = 0; sy < 2; sy++) {
    uint32_t mk = sy ? mk1 : mk0;
    if (mk == 0u) continue;
    uint32_t row[6];
#pragma unroll
    for (int c = 0; c < 6; c++) row[c] = sy ? sb[4 * (c >> 1) + 2 + (c & 1)] : sb[4 * (c >> 1) + (c & 1)];
#pragma unroll 1
    while (mk != 0u) {
      const int c = (int)__builtin_ctz(mk);
      mk &= mk - 1u;
      const uint32_t bsum = best_sum_cached<GLOBAL>(best, bcopy);
      if (pick6(row, c) < bsum) continue;  // the best has risen meanwhile
      const int32_t X = X0 + (c >> 1), sx = c & 1;
      const bool two = P.pair_subs != 0 && ((mk >> (c + 1)) & 1u) != 0u && (PAIR_CROSS || sx == 0) && pick6(row, c + 1) >= bsum;
      int dy, dx;
      uint32_t total;
      // the chunks to visit: those of the runs whose level-2 byte of the sub-block -- of either of a pair's two, which lie
      // two bits apart in the block's four -- is not zero (a pair across a block boundary, compiled out: every chunk)
      const uint32_t field = 1u << (4 * (c >> 1) + sy + 2 * sx);
      const uint32_t visit = two ? (sx == 0 ? chunk_mask(CN, field | (field << 2)) : CN.full) : chunk_mask(CN, field);
      n[9] += (uint32_t)nch;
      n[10] += (uint32_t)__builtin_popcount(visit);
      if (two) {
        mk &= ~(1u << (c + 1));
        total = pair_sums8_masked(rsrc, pitch8, (uint32_t)P.hi_copy_bytes, org, visit, Y, X, sy, sx, lane, &dy, &dx);
      } else {
        total = sub_sums8_masked(rsrc, pitch8, (uint32_t)P.hi_copy_bytes, org, visit, Y, X, sy, sx, lane, &dy, &dx);
      }
      const int32_t ix = BNB_B * X + BNB_B4 * sx + dx, iy = BNB_B * Y + BNB_B4 * sy + dy;
      if (CB == 1) {
        const unsigned long long key = best_key(P, k, ix, iy, total, 16);  // (lanes 32.. hold copies; a single's: lanes 16..)
        wave_atomic_max(best, key, lane);
        if (GLOBAL) bcopy = max(bcopy, (uint32_t)(key >> 32));
      } else {
        const uint32_t read = refine16<GLOBAL, true>(P, rsrc16, org, nch, n_pts, k, ix, iy, total, lane < (two ? 32 : 16), lane, best, bcopy, visit);
        n[3] += read;
        n[11] += read * (uint32_t)nch;
        n[12] += read * (uint32_t)__builtin_popcount(visit);
      }
      // (from the poses themselves, not from sub_valid: a pair's halves are the lanes with dx < 4 and dx >= 4)
      const bool pose = ix < P.nx && iy < P.ny;
      if (two) {
        n[2] += 2u;
        n[5] += (__ballot(pose && dx < BNB_B4) == 0ull ? 1u : 0u) + (__ballot(pose && dx >= BNB_B4) == 0ull ? 1u : 0u);
        n[7]++;
        n[8] += (uint32_t)sx;
      } else {
        n[2]++;
        n[5] += __ballot(pose) == 0ull ? 1u : 0u;
      }
    }
  }
}

// ---- shader-clock sums of a wave's rotation passes by part, and how many of the passes that asked for a run list took
// their strip bounds from it, or per cell because of the field check / the list's capacity (instrumented build)
struct PhaseClocks {
  long long org, strip, eval;
  uint32_t run_passes, cell_passes_field, cell_passes_full;
  // the seed passes among them (`done` set): all, those that began at a best sum of 0, those of them that left their strip
  // bounds out, and the seed blocks whose bounds were taken and held a 0 for a sub-block with a pose
  uint32_t seed_passes, seed_best0, seed_unbounded, seed_zero_sub;
};

// The instrumented build's flush into stats[] (indices: include/nautilus_hip_debug.h): work counts n[0..3] as
// process_candidate_c and rotation_pass count them, with the per-pair slot of `pair`, and / or a wave's phase clocks.
// `edge`: a wave's three counts at the lattice's edge and its two of pair passes, n + 4 (`chunks`: and its four of chunk
// visits behind them, the kernels that keep a run list).  Any may be null.  (The product build passes a null `stats`:
// dead code there.)
__device__ __forceinline__ void flush_stats(unsigned long long *stats, const uint32_t *n, int32_t pair, const PhaseClocks *clk,
                                            const uint32_t *edge = nullptr, bool chunks = false) {
  if (n) {
    if (n[0]) atomicAdd(&stats[0], (unsigned long long)n[0]);
    if (n[1]) atomicAdd(&stats[2], (unsigned long long)n[1]);
    if (n[2]) atomicAdd(&stats[3], (unsigned long long)n[2]);
    if (n[3]) atomicAdd(&stats[14], (unsigned long long)n[3]);  // poses of 16-bit grids evaluated exactly (refine16)
    if (pair < BNB_STATS_PAIRS) atomicAdd(&stats[BNB_STATS_HEAD + pair], 4ull * n[0] + n[2]);
  }
  if (edge && chunks) {  // a wave's n[9..12]: the chunk visits of its exact sums (behind the per-pair counts)
    unsigned long long *at = stats + BNB_STATS_HEAD + (size_t)BNB_STATS_PAIRS;
    for (int i = 0; i < BNB_STATS_CHUNKS; i++)
      if (edge[5 + i]) atomicAdd(&at[i], (unsigned long long)edge[5 + i]);
  }
  if (edge) {  // a wave's n[4..8]: the work at the lattice's edge, the pair passes
    if (edge[0]) atomicAdd(&stats[19], (unsigned long long)edge[0]);
    if (edge[1]) atomicAdd(&stats[20], (unsigned long long)edge[1]);
    if (edge[2]) atomicAdd(&stats[21], (unsigned long long)edge[2]);
    if (edge[3]) atomicAdd(&stats[22], (unsigned long long)edge[3]);
    if (edge[4]) atomicAdd(&stats[23], (unsigned long long)edge[4]);
  }
  if (clk) {
    atomicAdd(&stats[5], (unsigned long long)clk->org);
    atomicAdd(&stats[6], (unsigned long long)clk->strip);
    atomicAdd(&stats[7], (unsigned long long)clk->eval);
    if (clk->run_passes) atomicAdd(&stats[16], (unsigned long long)clk->run_passes);
    if (clk->cell_passes_field) atomicAdd(&stats[17], (unsigned long long)clk->cell_passes_field);
    if (clk->cell_passes_full) atomicAdd(&stats[18], (unsigned long long)clk->cell_passes_full);
  }
}

// ... and the seeds' own slots behind the chunk visits (nhip_bnb_stats_seeds): a wave's clocks by part as they stood when
// its seed pass was through, and the seed counts of `clk`
__device__ __forceinline__ void flush_seeds(unsigned long long *stats, const long long (&part)[3], const PhaseClocks &clk) {
  unsigned long long *at = stats + BNB_STATS_HEAD + (size_t)BNB_STATS_PAIRS + BNB_STATS_CHUNKS;
  const unsigned long long v[7] = {(unsigned long long)part[0], (unsigned long long)part[1], (unsigned long long)part[2],
                                   clk.seed_passes, clk.seed_best0, clk.seed_unbounded, clk.seed_zero_sub};
  for (int i = 0; i < 7; i++)
    if (v[i]) atomicAdd(&at[i], v[i]);
}

// ---- one rotation of one pair: its candidate blocks (masks m0 | m1 over block index b = NB * Y + X, bounds u0 / u1
// lane-wise) through sub-block bounds and exact sums, origins held in registers.  `done`: the workgroup's bound row
// of this rotation, where finished blocks are zeroed (seeds), or null.  PAIR: the sub-blocks of the strip's blocks that do
// not go whole are taken after its blocks, two side by side in one pass where both are alive (strip_sub_blocks); without
// it block by block, one pass each.  The candidates' kernels pair; csm_bnb_kernel -- the seeds, which take one block each,
// and the fused form's own rotations -- does not: the pair pass is 10 KB of code, and that kernel's by-rotation
// instantiations are at or past the 64 KB of the instruction cache as they are (profiles/r17_pair_passes_isa.txt).  RUNS: the wave has RUN_WAVE words at `runs` for
// the rotation's runs by level-2 entry, and the strip bounds walk those (unless P.l2_runs is off, or cache_origins
// reports that this rotation's runs do not fit the list or its 16-bit fields: then, as without RUNS, per cell).
template <int CB, bool GLOBAL, bool PAIR, bool RUNS = false>
__device__ __forceinline__ void rotation_pass(const BnbParams &P, const PairCtx &C, int32_t k, uint32_t u0, uint32_t u1,
                                              unsigned long long m0, unsigned long long m1, int lane,
                                              unsigned long long *best, uint32_t *done, uint32_t *org,
                                              uint32_t (&n_work)[N_WORK], PhaseClocks &clk, uint32_t *runs = nullptr,
                                              uint16_t *note = nullptr, uint8_t *span = nullptr) {
  long long t_mark = 0;
  float cf, sf;
  rotation_k(P, C.pair, k, &cf, &sf);
  // A seed pass (`done` set: one block, the wave's highest bound) that begins while the pair's best sum is still 0 -- no
  // score gate, no other wave's seed landed yet -- leaves the strip bounds out.  Against a sum of 0 they prune nothing: every
  // sub-block with a pose and a bound that is not 0 is alive, an interior block has four and goes whole.  All they could tell
  // is that a sub-block's windows hold only empty cells, which the highest-bound block of a rotation rarely has, and such
  // a sub-block's poses sum to 0 and yield keys that never beat the floor key.  With every bound at 0xffffffff, as without
  // level 2, process_candidate_c takes every sub-block that holds a pose (sub_valid: an edge block with at most two still
  // never goes whole): a superset of the poses the bounds admit, each with its exact sum, and keys are maxima -- records
  // and sums are the same.  The sum is read once, here (wave-uniform; one LDS round trip per pass, awaited where it is read).
  // P.seed_bounds (NHIP_BNB_SEED_BOUNDS=1): the bounds are taken whatever the sum.  profiles/r19_seeds.txt
  const bool seed_best0 = done != nullptr && best_sum<GLOBAL>(best) == 0u;
  const bool unbounded = seed_best0 && P.seed_bounds == 0;
  if (BNB_STATS(P)) t_mark = clock64();
  int32_t nrc = RUNS_NONE;
  const int32_t nch = cache_origins<RUNS>(P, C.pts, C.n_pts, cf, sf, C.cx, C.cy, lane, org, true, runs, RUNS && P.l2_runs != 0, &nrc, span);
  // (RUNS: the chunks of the cell list the exact sums visit come from the run list's notes, which the strip bounds write --
  //  without a usable run list, or without strip bounds, P.levels == 1: all)
  const ChunkNotes CN = {note + lane, span + lane, RUNS && P.zero_chunks != 0 && P.levels >= 2 ? nrc : 0, (1u << nch) - 1u};
  if (BNB_STATS(P)) clk.org += clock64() - t_mark;
  if (RUNS && BNB_STATS(P)) {
    clk.run_passes += nrc > 0 ? 1u : 0u;
    clk.cell_passes_field += nrc == RUNS_FIELD ? 1u : 0u;
    clk.cell_passes_full += nrc == RUNS_FULL ? 1u : 0u;
  }
  if (BNB_STATS(P) && done) {
    clk.seed_passes++;
    clk.seed_best0 += seed_best0 ? 1u : 0u;
    clk.seed_unbounded += unbounded && P.levels >= 2 ? 1u : 0u;
  }
  // (stored image + skip map: every offset an evaluation can form lies inside; see nhip_layout.hip make_layout)
  // (8-bit grids: the image, on which the exact sums run; 16-bit grids: the tiled copy of the image, for pose_sum16)
  const __amdgpu_buffer_rsrc_t rsrc16 = CB == 1 ? uniform_rsrc(C.grid, P.grid_bytes + P.skip_bytes)
                                                : uniform_rsrc(C.grid + P.hi_offset + 2 * P.hi_copy_bytes, P.t16_bytes);
  // the 8-bit plane of the exact block sums, tiled, two copies: the cells of 8-bit grids, the high bytes of 16-bit ones;
  // pitch8 = its tiles per tile row
  const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(C.grid + P.hi_offset, 2 * P.hi_copy_bytes);
  const uint32_t pitch8 = (uint32_t)P.hi_tpr;
  const __amdgpu_buffer_rsrc_t p4 = uniform_rsrc(C.grid + P.grid_bytes + P.skip_bytes + P.pool_bytes, P.pool4_bytes);
  // candidates in block order b = NB * Y + X; neighbours in X (up to three) share one pass over the table
  while ((m0 | m1) != 0ull) {
    const int b0 = m0 ? (int)__builtin_ctzll(m0) : 64 + (int)__builtin_ctzll(m1);
    const int Y = b0 / NB, X0 = b0 - NB * Y;
    int len = 1;
    while (len < 3 && X0 + len < NB) {
      const int b = b0 + len;
      if (!(((b < 64 ? m0 >> b : m1 >> (b - 64)) & 1ull))) break;
      len++;
    }
    uint32_t sb[12];
    uint32_t bcopy = GLOBAL ? best_sum<true>(best) : 0u;  // (one look per strip at a best in global memory)
    if (P.levels >= 2 && !unbounded) {
      if (BNB_STATS(P)) t_mark = clock64();
      if (RUNS && nrc > 0) strip_bounds_c<RunList<RUN_CHUNKS>, RUNS>(P, p4, runs + lane, nrc, Y, X0, len, CB == 1 ? 1u : 257u, sb, note + lane);
      else strip_bounds_c<CellList>(P, p4, org, nch, Y, X0, len, CB == 1 ? 1u : 257u, sb);
      if (BNB_STATS(P)) clk.strip += clock64() - t_mark;
      n_work[1] += (uint32_t)len;
      if (BNB_STATS(P) && done) {  // (a seed's strip is its one block)
        const int32_t vx = block_extent(P.nx, X0), vy = block_extent(P.ny, Y);
        clk.seed_zero_sub += ((sub_valid(vy, vx, 0, 0) && sb[0] == 0u) || (sub_valid(vy, vx, 0, 1) && sb[1] == 0u) ||
                              (sub_valid(vy, vx, 1, 0) && sb[2] == 0u) || (sub_valid(vy, vx, 1, 1) && sb[3] == 0u)) ? 1u : 0u;
      }
    } else {
      if (P.levels >= 2) n_work[1] += (uint32_t)len;  // (a seed block without its bounds still counts as a candidate refined)
#pragma unroll
      for (int q = 0; q < 12; q++) sb[q] = 0xffffffffu;
    }
    uint32_t mk0 = 0u, mk1 = 0u;  // the live sub-blocks of the strip's blocks that do not go whole, per sy
#pragma unroll 1
    for (int t = 0; t < len; t++) {
      const int b = b0 + t;
      if (b < 64) m0 &= ~(1ull << b);
      else m1 &= ~(1ull << (b - 64));
      const uint32_t ub = (uint32_t)__builtin_amdgcn_readlane((int)(b < 64 ? u0 : u1), b & 63);
      if (ub < best_sum_cached<GLOBAL>(best, bcopy)) continue;  // the best has risen meanwhile
      // (selects, not an indexed array: that would live in scratch)
      const uint32_t s0 = t == 0 ? sb[0] : (t == 1 ? sb[4] : sb[8]), s1 = t == 0 ? sb[1] : (t == 1 ? sb[5] : sb[9]);
      const uint32_t s2 = t == 0 ? sb[2] : (t == 1 ? sb[6] : sb[10]), s3 = t == 0 ? sb[3] : (t == 1 ? sb[7] : sb[11]);
      if (BNB_STATS(P)) t_mark = clock64();
      process_candidate_c<CB, GLOBAL, PAIR, RUNS>(P, rsrc, pitch8, rsrc16, org, nch, C.n_pts, k, Y, X0 + t, s0, s1, s2, s3, lane, best,
                                            bcopy, n_work, t, mk0, mk1, CN);
      if (BNB_STATS(P)) clk.eval += clock64() - t_mark;
      if (done && wave_leader(lane)) done[b] = 0u;
    }
    if (PAIR && (mk0 | mk1) != 0u) {
      if (BNB_STATS(P)) t_mark = clock64();
      strip_sub_blocks<CB, GLOBAL>(P, rsrc, pitch8, rsrc16, org, nch, C.n_pts, k, Y, X0, sb, mk0, mk1, lane, best, bcopy, n_work, CN);
      if (BNB_STATS(P)) clk.eval += clock64() - t_mark;
    }
  }
}

// ---- hand-over entries
__device__ __forceinline__ void read_entry(const RotEntry *ent, int32_t *pair, int32_t *k, unsigned long long *m0,
                                           unsigned long long *m1) {
  const unsigned long long w0 = ent->w[0], w1 = ent->w[1], w2 = ent->w[2], w3 = ent->w[3];
  *pair = (int32_t)(w0 >> 24);
  *k = (int32_t)(w0 & 0xffffffull);
  *m0 = w1 | (w2 << 41);          // blocks 0..63
  *m1 = (w2 >> 23) | (w3 << 18);  // blocks 64..120
}

__device__ __forceinline__ void pair_context(const BnbParams &P, int32_t pair, PairCtx *C) {
  const int32_t src = P.pair_src[pair], slot = P.pair_slot[pair];
  const int32_t beg = P.offsets[src];
  C->grid = P.grids + (size_t)slot * P.slot_bytes;
  C->pts = P.xy + beg;
  C->n_pts = P.offsets[src + 1] - beg;
  C->cx = P.pair_origin ? P.pair_origin[2 * pair] : 0;
  C->cy = P.pair_origin ? P.pair_origin[2 * pair + 1] : 0;
  C->pair = pair;
}

// BY_ROT: the pairs whose scan fits the register-held origins (n_pts <= 64 * OC), rotation by rotation; the other
// instantiation takes the longer scans -- or, with P.general_all (NHIP_BNB_QUEUE=1), every pair.
// Both are launched; a workgroup whose pair belongs to the other one returns at once.
// SPLIT (by-rotation form only): the workgroup ends after the seeds and leaves its state in P.ps_* for
// csm_bnb_cand_kernel.
// (the dynamic LDS: nhip_bnb_params.h has its layout, and lds_bytes() its size)
template <int CB, bool POOL_LDS, bool BY_ROT, bool SPLIT = false>
__global__ __launch_bounds__(SPLIT ? 64 * SPLIT_WAVES : BNB_THREADS, SPLIT ? SPLIT_WAVES / 2 : 4) void csm_bnb_kernel(BnbParams P) {
  constexpr int WAVES = SPLIT ? SPLIT_WAVES : BNB_WAVES, THREADS = 64 * WAVES;
  constexpr int QSPACE = lds_qspace(SPLIT);
  extern __shared__ __align__(16) uint8_t smem[];
  // first region: the pooled table (POOL_LDS) while the bounds are computed, then the waves' window origins
  uint8_t *s_pool = smem;
  uint32_t *s_org = reinterpret_cast<uint32_t *>(smem);
  uint32_t *s_U = reinterpret_cast<uint32_t *>(smem + P.lds_first);  // n_theta * 128
  unsigned long long *s_queue = reinterpret_cast<unsigned long long *>(s_U + (size_t)P.n_theta * 128);  // QSPACE
  LdsTail *s_tail = reinterpret_cast<LdsTail *>(s_queue + QSPACE);
  unsigned long long *s_best = &s_tail->best, *s_slow = &s_tail->slow;
  uint32_t *s_cnt = s_tail->cnt, *s_qn = s_cnt + LDS_QN, *s_qhead = s_cnt + LDS_QHEAD, *s_top = &s_tail->top;
  // phase 1 only: per wave a ring of LIST_ENTRIES run-length entries, in the queue's space
  uint32_t *s_list = reinterpret_cast<uint32_t *>(s_queue);
  static_assert(BNB_WAVES * LIST_ENTRIES * 4 <= QCAP * 4, "the run lists fit the first half of the queue");
  // by-rotation kernel: per rotation its highest bound (<< 32 | k), and the rotations in descending order of it,
  // behind the run lists (n_theta <= MAX_ROT): the second half of the queue's space
  unsigned long long *s_kmax = s_queue + (SPLIT ? WAVES * LIST_ENTRIES / 2 : QCAP / 2);
  uint32_t *s_order = reinterpret_cast<uint32_t *>(s_kmax + MAX_ROT);
  static_assert(SPLIT_WAVES * LIST_ENTRIES * 4 + MAX_ROT * 12 <= QSPACE_SPLIT * 8 && MAX_ROT * 12 <= QCAP * 4, "lists, maxima and order fit");

  // block -> pair: the pairs of one target are consecutive; keep them on one XCD (blocks b and b + 8 share one)
  const uint32_t bid = blockIdx.x;
  const int32_t pair = (int32_t)((bid & 7u) * (uint32_t)P.pairs_per_xcd + (bid >> 3));
  if ((int32_t)(bid >> 3) >= P.pairs_per_xcd || pair >= P.n_pairs) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  int32_t src = P.pair_src[pair], slot = P.pair_slot[pair];
  // (ids from device memory: a pair whose scan or slot lies outside the caller's counts is an empty scan -- it scores
  //  nothing, like a scan without points -- and is reported through the device's status words; both instantiations see it)
  const bool ids_ok = pair_ids_ok(P.ids, src, slot, pair + P.pair_base, threadIdx.x == 0);
  if (!ids_ok) src = slot = 0;
  const int32_t beg = ids_ok ? P.offsets[src] : 0, n_pts = ids_ok ? P.offsets[src + 1] - beg : 0;
  const float2 *pts = P.xy + beg;
  const uint8_t *grid = P.grids + (size_t)slot * P.slot_bytes;
  const int32_t cx = P.pair_origin ? P.pair_origin[2 * pair] : 0;
  const int32_t cy = P.pair_origin ? P.pair_origin[2 * pair + 1] : 0;
  const bool centre_ok = (abs(cx) + P.hx <= P.max_shift) && (abs(cy) + P.hy <= P.max_shift);
  if (BY_ROT != (n_pts <= 64 * OCL && (uint32_t)P.rows < ORG_LIMIT && !P.general_all)) return;  // the other instantiation's pair

  // pose 0 with sum 0 is a lower bound of the optimum (sums are >= 0; if all are 0, pose 0 is the answer): key0.  With a
  // score gate the best starts at the pair's floor key instead -- every pose below the floor is one the caller rejects --
  // and the kernels that take the pair over from keys[pair] prune against it alike (nhip_csm_shared.h; floor 0: key0)
  const int32_t gfloor = gate_floor(P.gate, n_pts);
  const unsigned long long fkey = gate_floor_key(gfloor);
  // (work counters: the instrumented build only.  Round 3 kept them in the general instantiation of the product build
  //  because it hung without them -- see wave_leader() for the cause, which was in the source, not in the counters.)
  unsigned long long *const stats_g = NHIP_BNB_INSTR ? P.stats : nullptr;
  const long long t_start = BNB_STATS(P) ? clock64() : 0;
  if (BNB_TIMELINE(P) && threadIdx.x == 0 && pair < BNB_STATS_PAIRS) BNB_TIMELINE(P)[4 * pair] = wall_clock64();
  if (threadIdx.x == 0) {
    *s_slow = 0ull;
    *s_best = fkey;
    s_cnt[0] = s_cnt[3] = s_cnt[4] = s_cnt[5] = 0u;
    s_top[0] = 0u;
    *s_qn = 0u;
    *s_qhead = 0u;
  }
  if (!centre_ok || n_pts <= 0) {  // (a centre the stored border cannot cover scores nothing)
    if (threadIdx.x == 0) P.keys[pair] = fkey;
    return;
  }
  // the terms of (cos, sin) of all of this wave's rotations, lane-wise: their loads fly under the staging below
  const RotationTerms terms = rotation_terms_of_wave<WAVES>(P, pair, wave, lane);
  if (POOL_LDS) {  // the target's pooled table -> LDS
    const uint4 *gp = reinterpret_cast<const uint4 *>(grid + P.grid_bytes + P.skip_bytes);
    uint4 *sp = reinterpret_cast<uint4 *>(s_pool);
    // (four loads per thread and round: 35 KB are 4.4 rounds of 512 threads, and a round trip each was 10 % of the pair.
    //  As compiled each load is sunk into the guard of its write and awaited there; holding all four in flight through an
    //  opaque copy before the first write was measured and bought nothing -- the other workgroup of the CU computes
    //  meanwhile -- profiles/r15_bounds_round_trips.txt.)
    const int32_t n16 = (int32_t)(P.pool_bytes / 16);
    for (int32_t i = threadIdx.x; i < n16; i += 4 * THREADS) {
      uint4 v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = gp[min(i + j * THREADS, n16 - 1)];
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (i + j * THREADS < n16) sp[i + j * THREADS] = v[j];
    }
  }
  const __amdgpu_buffer_rsrc_t prs = uniform_rsrc(grid + P.grid_bytes + P.skip_bytes, P.pool_bytes);
  float cfs, sfs;  // lane i: the wave's i-th rotation
  rotation_of(terms, &cfs, &sfs);
  __syncthreads();

  // (1) bounds of every block of every rotation this wave owns; the wave's own best bound
  const uint32_t scale = CB == 1 ? 1u : 257u;
  unsigned long long wbest = 0ull;  // (U << 32) | (k << 8 | slot)
  PointSlots slots;  // chunks 0 and 1 of the scan: primed here, loaded again by every rotation's last turn
  prime_slots(pts, wave < P.n_theta ? n_pts : 0, lane, slots);  // (a wave without a rotation loads nothing)
  int32_t mine = 0;  // the wave's rotations so far: the lane that holds the next one's (cos, sin)
  for (int32_t k = wave; k < P.n_theta; k += WAVES, mine++) {
    const float cf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cfs), mine));
    const float sf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sfs), mine));
    uint32_t umax = 0u;
    uint32_t tot[2];
    coarse_rotation<POOL_LDS>(P, s_pool, prs, pts, n_pts, slots, cf, sf, cx, cy, lane, s_list + wave * LIST_ENTRIES, tot);
    if (lane < 128 - NB * NB) s_U[k * 128 + NB * NB + lane] = 0u;  // (the row's unused tail)
#pragma unroll
    for (int i = 0; i < 2; i++) {
      // the bounds go to LDS in block order: entry b = NB * Y + X, so that neighbours in X are neighbours in b
      int Y, X;
      if (!slot_block(lane + 64 * i, &Y, &X)) continue;
      const uint32_t u = (Y < P.nby && X < P.nbx) ? tot[i] * scale : 0u;
      const int b = NB * Y + X;
      s_U[k * 128 + b] = u;
      umax = u > umax ? u : umax;
      const unsigned long long cand = ((unsigned long long)u << 32) | (uint32_t)((k << 8) | b);
      wbest = cand > wbest ? cand : wbest;
    }
    if (BY_ROT) {
      umax = wave_max(umax);  // (no LDS round trips)
      if (wave_leader(lane)) s_kmax[k] = ((unsigned long long)umax << 32) | (uint32_t)k;
    }
  }
  wbest = wave_max_u64(wbest);
  if (gfloor > 0) {  // (score gate; uniform over the workgroup)
    // no bound of the pair reaches the floor: no pose can be kept, the pair is settled -- no seeds, nothing handed over,
    // no candidates left for the split form's second kernel (its counts stay the zeros the host wrote)
    if (wave_leader(lane)) atomicMax(s_top, (uint32_t)(wbest >> 32));
    __syncthreads();
    if (*s_top < (uint32_t)gfloor) {
      if (threadIdx.x == 0) {
        P.keys[pair] = fkey;
        if (stats_g) {
          atomicAdd(&stats_g[1], (unsigned long long)(P.n_theta * P.nbx * P.nby));
          atomicAdd(&stats_g[15], 1ull);  // pairs settled after their bounds
        }
      }
      return;
    }
    // a wave's seed below the floor cannot raise the best: skipped
    if ((uint32_t)(wbest >> 32) < (uint32_t)gfloor) wbest = 0ull;
  }
  // (2) seed: the wave's highest-bound block, evaluated exactly
  uint32_t n_work[N_WORK] = {};
  PairCtx C;
  C.grid = grid;
  C.pts = pts;
  C.n_pts = n_pts;
  C.cx = cx;
  C.cy = cy;
  C.pair = pair;
  // Scans of up to 64 * OCL points: a wave owns a rotation at a time and keeps its window origins in LDS.
  // Longer scans take the general path below.
  if (BY_ROT) {
    // (the pooled table's space becomes the origins' once every wave is done with its bounds)
    // Seeds: every wave evaluates its highest-bound block.  (Fewer seeds -- only the waves with the highest bounds -- were
    // measured: 6 -> 8.1 ms, 4 -> 8.3, 1 -> 9.3 against 8.0 per 10,000 pairs; profiles/r03_matcher_experiments.txt.)
    __syncthreads();
    uint32_t *org = s_org + wave * ORG_WAVE + lane;
    // (NHIP_BNB_STATS=1: shader-clock sums -- wave time in phase 3 by part, and the workgroup's wall time)
    PhaseClocks clk = {0, 0, 0, 0u, 0u, 0u};
    long long clk_seed[3] = {0, 0, 0};  // (the wave's clocks by part when its seed was through: instrumented build)
    long long t_busy = 0, t_wall = 0;
    const long long t_phase1 = BNB_STATS(P) ? clock64() : 0;
    if (BNB_TIMELINE(P) && threadIdx.x == 0 && pair < BNB_STATS_PAIRS) BNB_TIMELINE(P)[4 * pair + 1] = wall_clock64();
    const uint32_t xcd = bid & 7u;
    bool handed_over = false;
    // One loop, one copy of the candidate code (it is large; three inlined copies did not fit the instruction
    // cache and halved the speed of everything).  A wave's work items, in this order:
    //  SEED  the wave's own highest-bound block, alone: the seeds give `best` a good lower bound before anything is
    //        pruned against it; then the workgroup orders its rotations by their highest bound and counts the
    //        candidates the seeds have left;
    //  OWN   rotations of the pair handed out one at a time, best first: every block of the rotation whose bound
    //        reaches the best sum found so far goes through its sub-block bounds and, where those hold, exact sums.
    //        A pair with a flat landscape (>= heavy_min candidates; see launch_csm_bnb) works only its first
    //        keep_ranks rotations here and hands the others -- the rotation and the mask of its candidate blocks --
    //        to the list of this XCD for the second kernel.
    enum { SEED, OWN };
    int state = SEED;
    bool heavy = false;  // (the pair hands its rotations over)
    for (;;) {
      bool have = false;
      int32_t k = 0;
      uint32_t u0 = 0u, u1 = 0u;
      unsigned long long m0 = 0ull, m1 = 0ull;
      uint32_t *done = nullptr;
      if (state == SEED) {
        if ((uint32_t)(wbest >> 32) != 0u) {
          const int32_t v = (int32_t)(wbest & 0xffu);
          const uint32_t ub = (uint32_t)(wbest >> 32);
          k = (int32_t)((uint32_t)wbest >> 8);
          u0 = v == lane ? ub : 0u;
          u1 = v == lane + 64 ? ub : 0u;
          m0 = v < 64 ? 1ull << v : 0ull;
          m1 = v < 64 ? 0ull : 1ull << (v - 64);
          done = s_U + k * 128;
          have = true;
        }
      } else if (state == OWN) {
        const int32_t rank = (int32_t)wave_fetch_add(s_qhead, 1u, lane);
        if (rank >= P.n_theta) break;
        k = (int32_t)s_order[rank];
        u0 = s_U[k * 128 + lane];
        u1 = s_U[k * 128 + 64 + lane];
        const uint32_t bsum = best_sum<false>(s_best);
        m0 = __ballot(u0 != 0u && u0 >= bsum);
        m1 = __ballot(u1 != 0u && u1 >= bsum && lane + 64 < NB * NB);
        if ((m0 | m1) == 0ull) continue;
        if (heavy && (uint32_t)rank >= P.keep_ranks) {
          // (a pair's rotations go round the eight lists, starting at its home XCD's: pairs with flat landscapes are
          //  consecutive pairs -- one XCD's list held them all and the other seven XCDs' waves found theirs empty)
          const uint32_t lx = (xcd + (uint32_t)rank) & 7u;
          const uint32_t e = wave_fetch_add(P.rot_count + 8 * lx, 1u, lane);
          if (e < P.rot_cap) {
            if (lane < 4) {
              const unsigned long long M41 = (1ull << 41) - 1ull;
              const unsigned long long word = lane == 0   ? ((unsigned long long)(uint32_t)pair << 24) | (uint32_t)k
                                              : lane == 1 ? (m0 & M41)
                                              : lane == 2 ? ((m0 >> 41) | (m1 << 23)) & M41
                                                          : (m1 >> 18);
              P.rot_list[(size_t)lx * P.rot_cap + e].w[lane] = word;
            }
            handed_over = true;
            continue;
          }  // (list full: the rotation stays here)
        }
        have = true;
      }
      if (have) rotation_pass<CB, false, false>(P, C, k, u0, u1, m0, m1, lane, s_best, done, org, n_work, clk);
      if (state == SEED) {
        __syncthreads();
        if (BNB_TIMELINE(P) && threadIdx.x == 0 && pair < BNB_STATS_PAIRS) BNB_TIMELINE(P)[4 * pair + 2] = wall_clock64();
        if (BNB_STATS(P)) {
          t_busy = clock64();
          t_wall = wall_clock64();
          clk_seed[0] = clk.org;
          clk_seed[1] = clk.strip;
          clk_seed[2] = clk.eval;
        }
        // best first: the rotations in descending order of their highest bound (rank by counting: n_theta^2 compares)
        for (int32_t kk = threadIdx.x; kk < P.n_theta; kk += THREADS) {
          const unsigned long long mine = s_kmax[kk];
          int32_t rank = 0;
          for (int32_t j = 0; j < P.n_theta; j++) rank += s_kmax[j] > mine ? 1 : 0;
          s_order[rank] = (uint32_t)kk;
        }
        // ... and how many candidates the seeds have left: a flat landscape leaves thousands (the median pair: ~30)
        if (P.rot_list || SPLIT) {
          const uint32_t bsum = best_sum<false>(s_best);
          uint32_t mine = 0u;
          for (int32_t kk = wave; kk < P.n_theta; kk += WAVES) {
            const uint32_t c0 = s_U[kk * 128 + lane], c1 = s_U[kk * 128 + 64 + lane];
            mine += (uint32_t)__builtin_popcountll(__ballot(c0 != 0u && c0 >= bsum)) +
                    (uint32_t)__builtin_popcountll(__ballot(c1 != 0u && c1 >= bsum && lane + 64 < NB * NB));
          }
          if (wave_leader(lane)) atomicAdd(s_qn, mine);
        }
        __syncthreads();
        if (SPLIT) {
          // the state for csm_bnb_cand_kernel: the rows of the rotations that still hold a candidate, best first
          const uint32_t bsum = best_sum<false>(s_best);
          uint32_t *rows = P.ps_rows + (size_t)pair * (size_t)P.n_theta * 128u;
          uint32_t live = 0u;
          for (int32_t r = wave; r < P.n_theta; r += WAVES) {
            const uint32_t kk = s_order[r];
            const uint32_t kmax = (uint32_t)(s_kmax[kk] >> 32);
            if (kmax == 0u || kmax < bsum) break;  // (descending: no later rank holds one either)
            live = (uint32_t)r + 1u;
            const uint32_t w1 = lane == 62 ? kmax : (lane == 63 ? kk : s_U[kk * 128 + 64 + lane]);
            rows[(size_t)r * 128u + lane] = s_U[kk * 128 + lane];
            rows[(size_t)r * 128u + 64 + lane] = w1;
          }
          if (live && wave_leader(lane)) atomicMax(s_qhead, live);  // (the hand-out counter is not used in this form)
          __syncthreads();
          if (threadIdx.x == 0) {
            P.ps_count[pair] = *s_qn;
            P.ps_live[pair] = *s_qhead;
            P.ps_next[pair] = 0u;
          }
          break;
        }
        heavy = P.rot_list && *s_qn >= P.heavy_min;
        state = OWN;
      }
    }
    if (BNB_STATS(P) && lane == 0) {
      const long long now = clock64();
      atomicAdd(&BNB_STATS(P)[4], (unsigned long long)(now - t_busy));       // wave time in phase 3 (until out of work)
      atomicAdd(&BNB_STATS(P)[11], (unsigned long long)(wall_clock64() - t_wall));  // the same in 100 MHz ticks
      flush_stats(BNB_STATS(P), nullptr, pair, &clk);  // (the counts: through s_cnt, below)
      flush_seeds(BNB_STATS(P), clk_seed, clk);
      atomicMax(s_slow, (unsigned long long)(now - t_busy));  // slowest wave
      if (wave == 0) {
        atomicAdd(&BNB_STATS(P)[9], (unsigned long long)(t_busy - t_phase1));  // seeds (wave 0's view)
        atomicAdd(&BNB_STATS(P)[10], (unsigned long long)(t_phase1 - t_start)); // bounds
        if (handed_over) atomicAdd(&BNB_STATS(P)[12], 1ull);
      }
    }
  } else {
  if ((uint32_t)(wbest >> 32) != 0u) {
      const int32_t k = (int32_t)((uint32_t)wbest >> 8), v = (int32_t)(wbest & 0xffu);
      const int Y = v / NB, X = v - NB * Y;
      float cf, sf;
      rotation_k(P, pair, k, &cf, &sf);
      const unsigned long long key = eval_block<CB>(P, grid, pts, n_pts, cf, sf, cx, cy, k, Y, X, lane);
      if (wave_leader(lane)) {
        atomicMax(s_best, key);
        s_U[k * 128 + v] = 0u;  // done
      }
      n_work[0]++;
    }
    __syncthreads();
    // (3) every block whose bound reaches the best sum found so far.  The survivors cluster in a few rotations,
    // i.e. in a few waves: they go through one queue per workgroup that all eight waves drain.
    for (int32_t k = wave; k < P.n_theta; k += BNB_WAVES) {
  #pragma unroll
      for (int i = 0; i < 2; i++) {
        const uint32_t u = s_U[k * 128 + lane + 64 * i];
        const uint32_t bsum = (uint32_t)(*(volatile unsigned long long *)s_best >> 32);
        bool cand = u != 0u && u >= bsum;
        const unsigned long long m = __ballot(cand);
        if (m == 0ull) continue;
        const uint32_t base = wave_fetch_add(s_qn, (uint32_t)__builtin_popcountll(m), lane);
        const uint32_t pos = base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        const unsigned long long entry = ((unsigned long long)u << 32) | (uint32_t)((k << 8) | (lane + 64 * i));
        if (cand && pos < (uint32_t)QCAP) s_queue[pos] = entry;
        unsigned long long over = __ballot(cand && pos >= (uint32_t)QCAP);  // queue full: this wave takes them itself
        while (over) {
          const int j = (int)__builtin_ctzll(over);
          over &= over - 1ull;
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)entry, j);
          const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(entry >> 32), j);
          if (hi >= best_sum<false>(s_best))  // (the best may have risen meanwhile)
            process_candidate<CB>(P, C, (int32_t)(lo >> 8), (int32_t)(lo & 0xffu), lane, s_best, n_work);
        }
      }
    }
    __syncthreads();
    {
      const uint32_t qn = min(*s_qn, (uint32_t)QCAP);
      for (;;) {
        const uint32_t i = wave_fetch_add(s_qhead, 1u, lane);
        if (i >= qn) break;
        const unsigned long long entry = s_queue[i];
        if ((uint32_t)(entry >> 32) >= best_sum<false>(s_best))
          process_candidate<CB>(P, C, (int32_t)((uint32_t)entry >> 8), (int32_t)(entry & 0xffu), lane, s_best, n_work);
      }
    }
}
  if (stats_g && lane == 0) {
    atomicAdd(&s_cnt[0], n_work[0]);
    atomicAdd(&s_cnt[3], n_work[1]);
    atomicAdd(&s_cnt[4], n_work[2]);
    atomicAdd(&s_cnt[5], n_work[3]);
    flush_stats(stats_g, nullptr, pair, nullptr, n_work + 4);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    P.keys[pair] = *s_best;  // (a pair that handed rotations over: the second kernel raises it from here)
    if (BNB_TIMELINE(P) && pair < BNB_STATS_PAIRS) {
      uint32_t hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      uint32_t xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      // 44 bits of time (100 MHz: two days), then the CU the workgroup ran on: HW_ID[15:8] = cu, sh, se; XCC id
      BNB_TIMELINE(P)[4 * pair + 3] = (wall_clock64() & 0xfffffffffffull) | ((unsigned long long)((hw >> 8) & 0xffu) << 44) |
                                      ((unsigned long long)(xcc & 0xfu) << 52);
    }
    if (BNB_STATS(P) && BY_ROT) atomicAdd(&BNB_STATS(P)[8], *s_slow);  // sum over pairs of the slowest wave's phase 3
    if (stats_g) {
      const uint32_t n_all[4] = {s_cnt[0], s_cnt[3], s_cnt[4], s_cnt[5]};  // (the workgroup's)
      flush_stats(stats_g, n_all, pair, nullptr);
      atomicAdd(&stats_g[1], (unsigned long long)(P.n_theta * P.nbx * P.nby));
    }
  }
}

// Second kernel: the rotations of the pairs with many candidates, one wave per (pair, rotation), every wave of the
// chip.  The pair's running best is keys[pair] (left by its workgroup after the seeds, raised by every wave that
// works on the pair); a block is skipped when that has passed its bound.
// (16-bit grids: compiled for five waves per SIMD like the candidates' kernel below -- the 96 registers it had before the
//  pair pass, which it otherwise passes by two; the instrumented build keeps its own 105)
template <int CB>
__global__ __launch_bounds__(256, CB == 2 && !NHIP_BNB_INSTR ? 5 : 4) void csm_bnb_rot_kernel(BnbParams P) {
  const int lane = threadIdx.x & 63;
  // workgroup b works on the list of XCD b & 7 (blocks b and b + 8 share an XCD)
  const uint32_t xcd = blockIdx.x & 7u;
  const uint32_t filled = P.rot_count[8 * xcd];
  const uint32_t count = filled < P.rot_cap ? filled : P.rot_cap;
  const RotEntry *list = P.rot_list + (size_t)xcd * P.rot_cap;
  __shared__ uint32_t s_org2[4 * ORG_WAVE];
  __shared__ uint32_t s_run2[4 * RUN_WAVE];
  __shared__ uint16_t s_note2[4 * RUN_WAVE];  // (per run: the strip's level-2 bytes that are not zero, the cell chunks)
  __shared__ uint8_t s_span2[4 * RUN_WAVE];
  uint32_t *org = s_org2 + (threadIdx.x >> 6) * ORG_WAVE + lane;
  uint32_t *runs = s_run2 + (threadIdx.x >> 6) * RUN_WAVE;
  uint16_t *note = s_note2 + (threadIdx.x >> 6) * RUN_WAVE;
  uint8_t *span = s_span2 + (threadIdx.x >> 6) * RUN_WAVE;
  PhaseClocks clk = {0, 0, 0, 0u, 0u, 0u};
  const long long t0 = BNB_STATS(P) ? clock64() : 0;
  for (;;) {
    const uint32_t i = wave_fetch_add(P.rot_count + 8 * xcd + 1, 1u, lane);
    if (i >= count) break;
    int32_t pair, k;
    unsigned long long m0, m1;
    read_entry(list + i, &pair, &k, &m0, &m1);
    PairCtx C;
    pair_context(P, pair, &C);
    uint32_t n[N_WORK] = {};
    // (no block bounds here: 0xffffffff lets every candidate through to its sub-block bounds, which are checked
    //  against the best as it stands in keys[pair])
    rotation_pass<CB, true, true, true>(P, C, k, 0xffffffffu, 0xffffffffu, m0, m1, lane, &P.keys[pair], nullptr, org, n, clk, runs, note, span);
    if (BNB_STATS(P) && lane == 0) flush_stats(BNB_STATS(P), n, pair, nullptr, n + 4, true);
  }
  if (BNB_STATS(P) && lane == 0) {
    atomicAdd(&BNB_STATS(P)[13], (unsigned long long)(clock64() - t0));  // wave time in the second kernel
    flush_stats(BNB_STATS(P), nullptr, 0, &clk);
  }
}

// ---- the split form's second and third launch ----------------------------------------------------------------
// The candidates' launch: per XCD (the pairs of a target stay where its grid is L2-resident) the list of its workgroups'
// pairs, IN PAIR ORDER -- the workgroups of a target's pairs then run together and share its lines in the XCD's L2.  The
// pairs with the most candidates left get one more workgroup per P.split_min of them, up to P.split_max (they share the
// pair's rotations through ps_next and its best through keys[pair]), granted by candidate count from the heaviest down
// while the XCD's list has room for a whole bucket's.  (Ordering the list by that count -- longest first -- was measured
// on the 10,000-pair workload and lost: 8.02 ms against 7.78 in target order; the kernel is bound by its memory pipeline,
// the shared heavy pairs leave no tail to hide, and the order scatters a target's pairs in time, L2 misses 4 % -> 30 %;
// shared pairs first: 7.9 ms.  profiles/r03_matcher_experiments.txt, commit 5048845 holds the code.)
// One workgroup per XCD segment.
constexpr int SORT_THREADS = 1024;
constexpr int SORT_BUCKETS = 16 * 21;
__device__ __forceinline__ int cand_bucket(uint32_t c) {  // sixteenths of an octave of the count; heaviest = bucket 0
  if (c == 0u) return SORT_BUCKETS - 1;
  const int e = 31 - __builtin_clz(c);                  // floor(log2 c)
  const int f = e >= 4 ? (int)((c >> (e - 4)) & 15u) : (int)((c << (4 - e)) & 15u);
  const int b = 16 * e + f;                              // ascending in c
  return b >= SORT_BUCKETS - 1 ? 0 : SORT_BUCKETS - 2 - b;
}
__device__ __forceinline__ uint32_t cand_shares(const BnbParams &P, uint32_t c) {
  const uint32_t w = 1u + c / P.split_min;
  return w < P.split_max ? w : P.split_max;
}

__global__ __launch_bounds__(SORT_THREADS) void csm_bnb_order_kernel(BnbParams P) {
  __shared__ uint32_t s_extra[SORT_BUCKETS];
  __shared__ uint32_t s_wave[SORT_THREADS / 64];
  __shared__ uint32_t s_base, s_idle;
  __shared__ int s_grant;
  const int32_t xcd = blockIdx.x;
  const int32_t lo = xcd * P.pairs_per_xcd, hi = min(lo + P.pairs_per_xcd, P.n_pairs);
  int32_t *work = P.ps_work + (size_t)xcd * P.ps_work_stride;
  for (int i = threadIdx.x; i < SORT_BUCKETS; i += SORT_THREADS) s_extra[i] = 0u;
  for (int i = threadIdx.x; i < P.ps_work_stride; i += SORT_THREADS) work[i] = -1;
  if (threadIdx.x == 0) s_base = s_idle = 0u;
  __syncthreads();
  // additional workgroups are granted by candidate count, from the heaviest pairs down, while the list has room for a
  // whole bucket's
  for (int32_t p = lo + (int32_t)threadIdx.x; p < hi; p += SORT_THREADS) {
    const uint32_t c = P.ps_count[p];
    atomicAdd(&s_extra[cand_bucket(c)], cand_shares(P, c) - 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t room = (uint32_t)P.ps_work_stride - (uint32_t)(hi > lo ? hi - lo : 0);
    int grant = 0;
    while (grant < SORT_BUCKETS && s_extra[grant] <= room) room -= s_extra[grant++];
    s_grant = grant;
  }
  __syncthreads();
  // the pairs with candidates, in pair order EXACTLY (a prefix sum, not atomics whose order scrambles windows of 1024 pairs)
  // -- in two passes when P.front_min is set: first the pairs with at least that many candidates left (a few per cent of
  // the list, a third of its work: a workgroup of theirs runs for 0.3 - 2 ms, and one that the in-order dispatch starts in
  // the launch's last half millisecond IS the launch's tail), then the others, whose workgroups take 0.03 - 0.2 ms
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int pass = P.front_min ? 0 : 1; pass < 2; pass++)
  for (int32_t p0 = lo; p0 < hi; p0 += SORT_THREADS) {
    const int32_t p = p0 + (int32_t)threadIdx.x;
    const uint32_t c = p < hi ? P.ps_count[p] : 0u;
    const bool mine = P.front_min == 0u || ((c >= P.front_min) == (pass == 0));
    const uint32_t w = (c != 0u && mine) ? (cand_bucket(c) < s_grant ? cand_shares(P, c) : 1u) : 0u;
    if (p < hi && mine) P.ps_nw[p] = c != 0u ? w : 1u;
    uint32_t v = w;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)v, off, 64);
      if (lane >= off) v += u;
    }
    if (lane == 63) s_wave[wv] = v;
    __syncthreads();
    uint32_t before = s_base;
    for (int q = 0; q < wv; q++) before += s_wave[q];
    const uint32_t at = before + v - w;
    for (uint32_t j = 0; j < w; j++) work[at + j] = p;
    __syncthreads();
    if (threadIdx.x == SORT_THREADS - 1) s_base = before + v;
    __syncthreads();
  }
  // (behind them the pairs with no candidate left: their workgroups return at once; any order)
  const uint32_t tail0 = s_base;
  for (int32_t p = lo + (int32_t)threadIdx.x; p < hi; p += SORT_THREADS)
    if (P.ps_count[p] == 0u) work[tail0 + atomicAdd(&s_idle, 1u)] = p;
}

// The work lists, spread form (the default): every pair ONCE in its home XCD's list, in pair order (the pairs of a target
// run together where its tables are L2-resident), and IN FRONT of those the additional workgroups of the pairs with many
// candidates left -- one more per P.split_min of them, up to P.split_max per pair -- dealt round-robin over ALL EIGHT
// lists.  Round 3 kept a pair's additional workgroups in its home XCD's list, behind a budget per XCD: the pairs with
// flat landscapes are consecutive pairs (the sources far from one target), so one XCD held them all, granted the
// heaviest bucket its shares and left the next bucket with ONE workgroup per pair -- on 3,000 pairs the candidates'
// launch ran 3.6 ms of which the last 2 ms were ten such pairs on one eighth of the chip (profiles/r04_small_lists.txt).
// The additional workgroups come first in the launch so that a heavy pair's work starts with the launch, not after it.
constexpr int ORDER_THREADS = 256;
__global__ __launch_bounds__(ORDER_THREADS) void csm_bnb_order_spread_kernel(BnbParams P) {
  const int32_t p = (int32_t)(blockIdx.x * ORDER_THREADS + threadIdx.x);
  if (p >= P.n_pairs) return;
  const int32_t extra_slots = P.ps_work_stride - P.pairs_per_xcd;  // per list
  const int32_t home = p / P.pairs_per_xcd;
  P.ps_work[(size_t)home * P.ps_work_stride + extra_slots + (p - home * P.pairs_per_xcd)] = p;
  const uint32_t want = cand_shares(P, P.ps_count[p]) - 1u;
  uint32_t got = 0u;
  if (want) {
    const uint32_t t0 = atomicAdd(P.ps_ticket, want);
    for (uint32_t j = 0; j < want; j++) {
      const uint32_t e = t0 + j;
      if ((int32_t)(e >> 3) >= extra_slots) break;  // (the lists are full: the pair works with what it got)
      // (a pair's additional workgroups start on the XCD after its home's and go round from there)
      P.ps_work[(size_t)((e + (uint32_t)home + 1u) & 7u) * P.ps_work_stride + (e >> 3)] = p;
      got++;
    }
  }
  P.ps_nw[p] = 1u + got;
}

// The candidates: the OWN loop of csm_bnb_kernel on the state its split form left.  Four waves per workgroup, each takes
// the pair's live rotations one at a time, best first.  A pair with one workgroup keeps its hand-out counter and its
// best in LDS; a shared pair uses ps_next[pair] and keys[pair] -- the code is the same, through generic pointers, with
// the look-once-per-strip discipline of a best that may live in global memory.
constexpr int CAND_WAVES = 4;  // waves per workgroup of the candidates' kernel
constexpr int CAND_THREADS = 64 * CAND_WAVES;
// waves per SIMD the kernel is compiled for (register budget 512 / that): 4 for 8-bit grids, 5 for 16-bit grids -- with
// their planes tiled the working set fits five (6.78 -> 6.43 ms; 4 / 6: profiles/r04_bounds_variants.txt)
template <int CB>
__global__ __launch_bounds__(CAND_THREADS, CB == 2 ? 5 : 4) void csm_bnb_cand_kernel(BnbParams P) {
  __shared__ uint32_t s_org2[CAND_WAVES * ORG_WAVE];
  __shared__ uint32_t s_run2[CAND_WAVES * RUN_WAVE];  // (25.6 KB with the origins ...
  __shared__ uint16_t s_note2[CAND_WAVES * RUN_WAVE];  //  ... and 6 KB of notes per run for the chunk masks: 31.0 KB; five
  __shared__ uint8_t s_span2[CAND_WAVES * RUN_WAVE];   //  workgroups per CU have 32 KB each)
  static_assert(CAND_WAVES * (ORG_WAVE * 4 + RUN_WAVE * 4 + RUN_NOTE_BYTES) + 16 <= 32 * 1024, "five workgroups per CU");
  __shared__ unsigned long long s_best2;
  __shared__ uint32_t s_next2;
  const int lane = threadIdx.x & 63;
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  if ((int32_t)slot >= P.ps_work_stride) return;
  const int32_t pair = P.ps_work[(size_t)xcd * P.ps_work_stride + slot];
  if (pair < 0) return;
  const uint32_t live = P.ps_live[pair];
  if (live == 0u) return;  // (nothing left after the seeds, or a pair of the general kernel)
  const bool shared = P.ps_nw[pair] > 1u;
  // (NHIP_BNB_TIMELINE=1, instrumented build: first start and last end over the pair's workgroups, 100 MHz ticks; the
  //  pair's index here is its index in the ROUND -- tools look at lists of one round)
  if (BNB_TIMELINE(P) && threadIdx.x == 0 && pair < BNB_STATS_PAIRS)
    atomicMin(&BNB_TIMELINE(P)[4 * (size_t)BNB_STATS_PAIRS + 2 + pair], wall_clock64());
  if (threadIdx.x == 0) {
    s_best2 = P.keys[pair];
    s_next2 = 0u;
  }
  __syncthreads();
  unsigned long long *best = shared ? &P.keys[pair] : &s_best2;
  uint32_t *next = shared ? &P.ps_next[pair] : &s_next2;
  const uint32_t *rows = P.ps_rows + (size_t)pair * (size_t)P.n_theta * 128u;
  uint32_t *org = s_org2 + (threadIdx.x >> 6) * ORG_WAVE + lane;
  uint32_t *runs = s_run2 + (threadIdx.x >> 6) * RUN_WAVE;
  uint16_t *note = s_note2 + (threadIdx.x >> 6) * RUN_WAVE;
  uint8_t *span = s_span2 + (threadIdx.x >> 6) * RUN_WAVE;
  PairCtx C;
  pair_context(P, pair, &C);
  uint32_t n_work[N_WORK] = {};
  PhaseClocks clk = {0, 0, 0, 0u, 0u, 0u};
  const long long t0 = BNB_STATS(P) ? clock64() : 0;
  for (;;) {
    const uint32_t rank = wave_fetch_add(next, 1u, lane);
    if (rank >= live) break;
    const uint32_t u0 = rows[(size_t)rank * 128u + lane], u1 = rows[(size_t)rank * 128u + 64 + lane];
    const uint32_t kmax = (uint32_t)__builtin_amdgcn_readlane((int)u1, 62);
    const int32_t k = __builtin_amdgcn_readlane((int)u1, 63);
    const uint32_t bsum = best_sum<true>(best);
    if (kmax < bsum) break;  // (best first: the later ranks hold nothing either)
    const unsigned long long m0 = __ballot(u0 != 0u && u0 >= bsum);
    const unsigned long long m1 = __ballot(u1 != 0u && u1 >= bsum && lane + 64 < NB * NB);
    if ((m0 | m1) == 0ull) continue;
    rotation_pass<CB, true, true, true>(P, C, k, u0, u1, m0, m1, lane, best, nullptr, org, n_work, clk, runs, note, span);
  }
  if (BNB_STATS(P) && lane == 0) {
    atomicAdd(&BNB_STATS(P)[13], (unsigned long long)(clock64() - t0));
    flush_stats(BNB_STATS(P), n_work, pair, &clk, n_work + 4, true);
  }
  if (BNB_TIMELINE(P) && lane == 0 && pair < BNB_STATS_PAIRS)
    atomicMax(&BNB_TIMELINE(P)[5 * (size_t)BNB_STATS_PAIRS + 2 + pair], wall_clock64());
  if (!shared) {
    __syncthreads();
    if (threadIdx.x == 0) P.keys[pair] = s_best2;
  }
}

}  // namespace

// ---- the kernel launches of one batch (compiled in both builds)
namespace bnb {

namespace {
// hipFuncSetAttribute once per instantiation and LDS size reached (not per launch)
template <int CB, bool PL, bool BR, bool SP = false>
int launch_main(const BnbParams &P, const BnbPlan &plan, hipStream_t s) {
  // (the split form's first kernel: its own workgroup size, and its own size of the queue's space)
  constexpr int THREADS = SP ? 64 * SPLIT_WAVES : BNB_THREADS;
  const size_t lds = lds_bytes((size_t)plan.lds_first, P.n_theta, SP);
  const int64_t blocks = (int64_t)P.pairs_per_xcd * 8;
  // (the attribute belongs to the function object of the CURRENT device: one high-water mark per device, so that a host
  //  with one thread per device raises it on each of them)
  constexpr int MAX_DEV = 64;
  static std::atomic<size_t> lds_set[MAX_DEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) dev = -1;
  if (dev < 0 || lds > lds_set[dev].load(std::memory_order_relaxed)) {
    NHIP_TRY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(csm_bnb_kernel<CB, PL, BR, SP>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (dev >= 0) lds_set[dev].store(lds, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL((csm_bnb_kernel<CB, PL, BR, SP>), dim3((uint32_t)blocks), dim3(THREADS), lds, s, P);
  return NHIP_OK;
}

// The split form's first part on one batch: bounds + seeds of the by-rotation pairs, the general kernel for the scans
// that form does not take, the order of the candidates' launch ...
template <int CB, bool PL>
int launch_split_a(const BnbParams &P, const BnbPlan &plan, hipStream_t s) {
  int rc = launch_main<CB, PL, true, true>(P, plan, s);
  if (rc) return rc;
  // (the general instantiation only has work when some scan does not fit the by-rotation form: a caller that knows its
  //  scan lengths says so -- NHIP_SEARCH_SHORT_SCANS -- and saves the launch of n_pairs workgroups that return at once)
  if (!P.short_scans && (rc = launch_main<CB, PL, false>(P, plan, s))) return rc;
  if (P.ps_ticket)
    hipLaunchKernelGGL(csm_bnb_order_spread_kernel, dim3((uint32_t)((P.n_pairs + ORDER_THREADS - 1) / ORDER_THREADS)), dim3(ORDER_THREADS), 0, s, P);
  else
    hipLaunchKernelGGL(csm_bnb_order_kernel, dim3(8), dim3(SORT_THREADS), 0, s, P);
  return NHIP_OK;
}

template <int CB, bool PL>
int launch_both(const BnbParams &P, const BnbPlan &plan, hipStream_t s) {
  // both instantiations are launched; a workgroup whose pair belongs to the other one returns at once
  if (!P.general_all) {
    int rc = launch_main<CB, PL, true>(P, plan, s);
    if (rc) return rc;
    if (P.short_scans) return NHIP_OK;
  }
  return launch_main<CB, PL, false>(P, plan, s);
}

// The one choice of a plan's template instantiation: f(cell bytes, pooled table in LDS) as integral constants.
template <class F>
int with_instantiation(const BnbPlan &plan, F f) {
  using CB1 = std::integral_constant<int, 1>;
  using CB2 = std::integral_constant<int, 2>;
  if (plan.cb == 1) return plan.pool_lds ? f(CB1{}, std::true_type{}) : f(CB1{}, std::false_type{});
  return plan.pool_lds ? f(CB2{}, std::true_type{}) : f(CB2{}, std::false_type{});
}

int launch_fused(const BnbParams &P, const BnbPlan &plan, hipStream_t s) {
  return with_instantiation(plan, [&](auto cb, auto pl) {
    const int rc = launch_both<decltype(cb)::value, decltype(pl)::value>(P, plan, s);
    if (rc) return rc;
    if (plan.second) {
      const uint32_t rot_blocks = 256 * 4;  // four workgroups of four waves per CU; the waves take entries off the lists
      hipLaunchKernelGGL(csm_bnb_rot_kernel<decltype(cb)::value>, dim3(rot_blocks), dim3(256), 0, s, P);
    }
    return NHIP_OK;
  });
}

int launch_split_bounds(const BnbParams &P, const BnbPlan &plan, hipStream_t s) {
  return with_instantiation(plan, [&](auto cb, auto pl) { return launch_split_a<decltype(cb)::value, decltype(pl)::value>(P, plan, s); });
}

// the split form's candidates (on any stream ordered behind the first part of the same batch)
int launch_split_cands(const BnbParams &P, const BnbPlan &plan, hipStream_t s) {
  return with_instantiation(plan, [&](auto cb, auto) {
    hipLaunchKernelGGL(csm_bnb_cand_kernel<decltype(cb)::value>, dim3((uint32_t)(8 * P.ps_work_stride)), dim3(CAND_THREADS), 0, s, P);
    return NHIP_OK;
  });
}
}  // namespace

BnbLaunchers launchers_product() { return {launch_fused, launch_split_bounds, launch_split_cands}; }

}  // namespace bnb


}  // namespace nhip
