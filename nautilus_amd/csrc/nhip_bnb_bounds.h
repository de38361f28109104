// nhip_bnb_bounds.h -- the three upper bounds of the branch-and-bound matcher's kernels (nhip_bnb.hip).
//
// Owns: coarse_rotation -- the bounds of all 11 x 11 blocks of one rotation from the pooled table, gathered per RUN of
// points that share a pooled entry (the run lists: LIST_ENTRIES words of LDS per wave) -- with PointSlots / prime_slots, its
// point prefetch's registers, which the caller keeps from rotation to rotation, and slot_block, the layout its totals come
// out in; sub_bounds -- the four 4 x 4 sub-block bounds of one block, from the points; strip_bounds_c -- the
// same for a strip of up to three blocks, from the origins a wave holds (CellList) or their runs by level-2 entry (RunList),
// which can also note per run which of the strip's bytes are not zero (NOTE: what the exact sums' chunk masks are made of).
// Assumes: the pooled tables behind the stored image as the table build leaves them (nhip_grid_blur.hip,
// nhip_grid_tables.hip: zero rows below the pooled image, a pitch that is a multiple of 16, offsets below
// 1 << RUN_SHIFT), 16-bit packed fields (LANE_WEIGHT, 18 chunks of 64 points).  Every bound is at least the largest sum of the poses it covers; nothing here reads the stored cells.
// Included by nhip_bnb.hip only.
#pragma once
#include <type_traits>

#include "nhip_bnb_origin.h"

namespace nhip {
namespace {

// ---- bounds of one rotation ------------------------------------------------------------------------------
// Returns this lane's two totals of the 128-slot layout: slot v = lane + 64 * i (i = 0, 1) holds packed register
// r = 32 i + 16 b5 + 8 b4 + 4 b3 + 2 b1 + b0, field b2 (b = bits of the lane) -- see slot_block().
// POOL_LDS: the pooled table is staged in LDS (`pool`); otherwise it is read from the grid slot in global memory
// through the buffer descriptor `prs` (tables of large grids, e.g. the 6000 x 6000 grid of the two-level drop-in).
//
// Consecutive beams hit the same wall: on a 1081-beam scan 5 to 10 consecutive points share a pooled entry
// (8 x 8 cells = 40 cm), and every one of them would gather the same 11 x 11 bytes.  So the points are first
// run-length compressed: a lane whose pooled offset differs from its predecessor's (or that starts a 64-point chunk)
// is the head of a run and writes (offset, run length <= 64) to the wave's list in LDS; the gather then works on
// list entries, 64 at a time, and adds every byte `length` times (one multiply-add in place of the add): ~165
// entries for 1081 points, three passes.  (Runs cut at every 8th lane, the first form: 265 entries, five passes.)
// Field widths: the accumulators and the first two reduction steps (over 4 lanes) hold 16-bit fields, so a lane may
// gather a total run length of at most LANE_WEIGHT = 64 between two reductions (4 lanes * 64 * 255 = 65,280); the
// wave reduces early when a pass would take some lane past that, otherwise once per rotation.
constexpr uint32_t LANE_WEIGHT = 64u;

// The two slots of coarse_rotation's point prefetch (see there).  A wave primes them once, before its first rotation; every
// rotation leaves them holding -- or awaiting -- chunks 0 and 1 again, which are the next rotation's first.
struct PointSlots {
  float2 q0, q1;
};
__device__ __forceinline__ void prime_slots(const float2 *pts, int32_t n_pts, int lane, PointSlots &S) {
  S.q0 = S.q1 = make_float2(0.f, 0.f);
  if (n_pts > 0) {  // (an empty scan loads nothing)
    const int32_t last = n_pts - 1;
    S.q0 = pts[min(lane, last)];
    __builtin_amdgcn_sched_barrier(0);
    S.q1 = pts[min(64 + lane, last)];
  }
}

template <bool POOL_LDS>
__device__ __forceinline__ void coarse_rotation(const BnbParams &P, const uint8_t *pool, __amdgpu_buffer_rsrc_t prs,
                                                const float2 *pts, int32_t n_pts, PointSlots &S, float cf, float sf,
                                                int32_t cx, int32_t cy, int lane, uint32_t *list, uint32_t (&tot)[2]) {
  const int32_t DP = P.pool_pitch;
  const uint32_t zero_a = (uint32_t)(((P.rows + BNB_B - 1) / BNB_B) * DP);  // NB + 1 rows of zeros below the pooled image
  tot[0] = tot[1] = 0u;
  uint32_t E[NB][3], O[NB][3];  // per block row Y: 12 byte sums = dwords 0..2, even (b0 | b2 << 16) and odd (b1 | b3 << 16)
#pragma unroll
  for (int y = 0; y < NB; y++)
#pragma unroll
    for (int d = 0; d < 3; d++) E[y][d] = O[y][d] = 0u;
  uint32_t head = 0u, tail = 0u;  // ring positions (wave-uniform)
  uint32_t reduced = 0u;          // `head` at the last reduction: passes were gathered since iff head != reduced (scalar)
  uint32_t weight = 0u;           // this lane's run lengths gathered since the last reduction

  // 64 list entries: every lane gathers the 11 x 12 bytes of its entry, weighted by the run length.  The bytes of dword d
  // of the window (byte offset s = a & 3 into the aligned words) come out of the pair (w[d + 1], w[d]) by one v_perm_b32
  // per field: selector bytes s, s + 2 give the even bytes b0 | b2 << 16, s + 1, s + 3 the odd ones b1 | b3 << 16, and
  // 0x0c a zero byte.  Both fields come out clean: the reduction takes them as they are.
  auto gather = [&](uint32_t a, uint32_t cnt) {
    const uint32_t se = __umul24(a & 3u, 0x10001u) + 0x0c020c00u, so = se + 0x00010001u;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(pool + (a & ~3u));
    auto add_row = [&](int y, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
      E[y][0] += __umul24(__builtin_amdgcn_perm(w1, w0, se), cnt); O[y][0] += __umul24(__builtin_amdgcn_perm(w1, w0, so), cnt);
      E[y][1] += __umul24(__builtin_amdgcn_perm(w2, w1, se), cnt); O[y][1] += __umul24(__builtin_amdgcn_perm(w2, w1, so), cnt);
      E[y][2] += __umul24(__builtin_amdgcn_perm(w3, w2, se), cnt); O[y][2] = mad24(__builtin_amdgcn_perm(w3, w2, so), cnt, O[y][2]);
    };
    auto load_row = [&](int y, uint32_t &w0, uint32_t &w1, uint32_t &w2, uint32_t &w3) {
      if (POOL_LDS) {
        const uint32_t *row = q + (y * DP) / 4;  // DP is a multiple of 16
        w0 = row[0]; w1 = row[1]; w2 = row[2]; w3 = row[3];
      } else {
        const u32x4 r4 = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)((a & ~3u) + (uint32_t)(y * DP)), 0, 0);
        w0 = r4.x; w1 = r4.y; w2 = r4.z; w3 = r4.w;
      }
    };
    // One row ahead: row y + 1's four dwords are in flight while row y is added, so that the wait before a row's adds
    // leaves the next row's reads outstanding -- an LDS round trip per row, eleven per pass, was fully exposed (the
    // scheduler issued a row's reads only after the adds of the row before; the global pool's buffer loads each behind a
    // full wait: profiles/r15_bounds_round_trips_isa.txt).  Four more registers; every by-rotation instantiation stays
    // below 124.  The barriers keep the order the source has; the reads of the last row are awaited alone.
    uint32_t n0, n1, n2, n3;
    load_row(0, n0, n1, n2, n3);
#pragma unroll
    for (int y = 0; y < NB; y++) {
      const uint32_t w0 = n0, w1 = n1, w2 = n2, w3 = n3;
      if (y + 1 < NB) load_row(y + 1, n0, n1, n2, n3);
      __builtin_amdgcn_sched_barrier(0);
      add_row(y, w0, w1, w2, w3);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // the transposing reduction of the 128 packed sums (see the layout above); clears the accumulators
  auto reduce = [&]() {
    // 64 packed registers: R[6 y + d] (y < 10): d < 3 = E[y][d] (X = 4 d, 4 d + 2), d >= 3 = O[y][d - 3] (X = 4 (d - 3) + 1, + 3);
    // the hi field of O[y][2] is X = 11 (unused): rows 0..2 carry X = 5, 7, 9 of block row 10 there.
    // R[60..62] = E[10][0..2], R[63] = O[10][0].
    uint32_t R[64];
#pragma unroll
    for (int y = 0; y < 10; y++)
#pragma unroll
      for (int d = 0; d < 3; d++) {
        R[6 * y + d] = E[y][d];
        R[6 * y + 3 + d] = O[y][d];
      }
    R[5] = (O[0][2] & 0xffffu) | (O[10][1] << 16);          // (10, 5)
    R[11] = (O[1][2] & 0xffffu) | (O[10][1] & 0xffff0000u);  // (10, 7)
    R[17] = (O[2][2] & 0xffffu) | (O[10][2] << 16);          // (10, 9)
    R[60] = E[10][0];
    R[61] = E[10][1];
    R[62] = E[10][2];
    R[63] = O[10][0];
    rs_step<64, 1>(R, lane & 1);
    rs_step<32, 2>(R, lane & 2);
    uint32_t V[32];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      V[2 * i] = R[i] & 0xffffu;
      V[2 * i + 1] = R[i] >> 16;
    }
    rs_step<32, 4>(V, lane & 4);
    rs_step<16, 8>(V, lane & 8);
    rs_step<8, 16>(V, lane & 16);
    rs_step<4, 32>(V, lane & 32);
    tot[0] += V[0];
    tot[1] += V[1];
#pragma unroll
    for (int y = 0; y < NB; y++)
#pragma unroll
      for (int d = 0; d < 3; d++) E[y][d] = O[y][d] = 0u;
  };

  // One chunk's pooled offsets `a` (point c + lane; lanes past the scan's end carry the zero rows) into the run list,
  // then the gather passes that have become due.  more == false: no chunk, the list is drained and reduced.
  auto feed = [&](uint32_t a, int32_t c, bool more) {
    if (more) {
      const bool live = c + lane < n_pts;
      // runs of equal offsets inside the chunk: the predecessor's offset by a DPP shift across the wave, no LDS round
      // trip; the chunk's first lane is a head anyway
      const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)a, (int)a, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
      const bool is_head = (lane & 63) == 0 || a != prev;
      // (the lane masks straight from the compares: a ballot of the bools goes through a 0 / 1 register and back)
      const unsigned long long H = __builtin_amdgcn_uicmp(a, prev, 33 /* ne */) | 1ull;
      // (the entry carries its first point's index modulo 128; the gather subtracts it from the next entry's -- one LDS
      //  read per 64 entries instead of two 64-bit shifts, a compare and two bit searches per 64 points.  The last run
      //  ends at the sentinel entry written after the last chunk.)
      uint32_t cnt = (uint32_t)(c + lane) & 127u;
      cnt += 1u;  // (stored as cnt - 1 below)
      const int32_t n_live = n_pts - c;  // (lanes past the scan's end emit nothing)
      const unsigned long long He = H & (n_live >= 64 ? ~0ull : (1ull << n_live) - 1ull);
      if (is_head && live) {
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(He >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)He, 0u));
        list[(tail + before) & (LIST_ENTRIES - 1)] = a | ((cnt - 1u) << RUN_SHIFT);
      }
      tail += (uint32_t)__builtin_popcountll(He);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (!more) {
      // the sentinel: where the last run ends.  (At most 64 entries are pending here -- the last chunk's turn drained
      // the list below 65 -- so the slot is free.)
      if (lane == 0) list[tail & (LIST_ENTRIES - 1)] = ((uint32_t)n_pts & 127u) << RUN_SHIFT;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    // gather passes: whenever 64 entries are pending (and the one after them, which ends the 64th's run),
    // and to the last entry once the scan is through; then one more turn for the rotation's (only, as a rule)
    // reduction -- one copy of that code
    for (;;) {
      const uint32_t avail = tail - head;
      if (avail < 65u && more) break;
      const bool last = avail == 0u;  // (!more)
      // (lanes past the list gather the zero rows with length 0)
      const bool mine = (uint32_t)lane < avail;
      const uint32_t entry = mine ? list[(head + (uint32_t)lane) & (LIST_ENTRIES - 1)] : zero_a;
      const uint32_t ea = entry & ((1u << RUN_SHIFT) - 1u);
      const uint32_t next = mine ? list[(head + (uint32_t)lane + 1u) & (LIST_ENTRIES - 1)] : 0u;
      const uint32_t cnt = mine ? ((next >> RUN_SHIFT) - (entry >> RUN_SHIFT)) & 127u : 0u;
      // (also before a pass that could overflow some lane's fields)
      // (the lane mask straight from the compare; `last` tested on a scalar register the compiler knows nothing about:
      //  as the bool above, which also ends the loop, it is inverted here through a 0 / 1 vector register)
      uint32_t left = avail;
      asm("" : "+s"(left));
      if (head != reduced && (left == 0u || __builtin_amdgcn_uicmp(weight + cnt, LANE_WEIGHT, 34 /* ugt */) != 0ull)) {
        reduce();
        reduced = head;
        weight = 0u;
      }
      if (last) break;
      gather(ea, cnt);
      weight += cnt;
      head += avail < 64u ? avail : 64u;
      __builtin_amdgcn_wave_barrier();
    }
  };

  // (Tried: the window origins of TWO chunks per turn in one basic block, so that the scheduler interleaves the two
  //  chains -- bounds + seeds 3.18 -> 3.23 ms, profiles/r04_bounds_variants.txt: the chains' latency is hidden already.)
  // The points of the next PD = 2 chunks are in flight while one chunk is worked: with two workgroups per CU gathering
  // from their grids, a point load takes ~1,300 clocks, more than a chunk's work.  Each slot is a register pair of its
  // own (q0, q1) and a turn of the loop works both, so that the wait before a slot's points are used is vmcnt(1): it
  // admits the other slot's load, issued one chunk later.  What keeps that depth in the compiled loop
  // (profiles/r14_point_prefetch_isa.txt; each of these, left out, brings back a full wait):
  //  - the chunk's points leave the slot through an opaque copy, and the slot's next chunk is loaded straight into it
  //    (a ring qn[d] = qn[d + 1] is loaded into a temporary and copied at the back-edge, behind vmcnt(0));
  //  - the load is unconditional, its index clamped to the scan's last point (a guarded load is a select on the loaded
  //    registers); lanes past the scan's end are dropped by `live` as before;
  //  - both slots load on every turn and only the second BODY is predicated (a break between the bodies leaves a path
  //    into the header on which the first slot's load is the youngest);
  //  - the priming loads (prime_slots) are issued first slot first.
  // Nothing else of the loop uses the vector-memory counter out of order: the gather's loads (global form) are awaited
  // inside their pass, and the run list is LDS.
  auto offsets = [&](float2 pt, int32_t c) {  // pooled offsets of chunk c from its points
    uint32_t a = zero_a;
    if (c + lane < n_pts) {
      int32_t prow, pcol;
      window_origin<true>(pt, cf, sf, P, cx, cy, &prow, &pcol);
      // (both factors are below 2^12: rows and pitch of the pooled image; the padding keeps prow positive)
      a = __umul24((uint32_t)prow >> 3, (uint32_t)DP) + ((uint32_t)pcol >> 3);
    }
    return a;
  };
  // The slots outlive the rotation (S, primed by the caller before the wave's first): the last turn, whose loads would lie
  // past the scan's end, loads chunks 0 and 1 again -- the same points for every rotation, with the priming loads' clamp
  // for scans shorter than 128 points -- so the next rotation's first chunks arrive behind this one's drain turn and
  // reduction, and the drain turn awaits no load.  (Before: the drain turn waited for two clamped loads nobody used, and
  // every rotation began with two priming loads and nothing to hide them behind.)
  constexpr int PD = 2;
  if (n_pts > 0) {  // (an empty scan loads nothing)
    const int32_t last = n_pts - 1;
    for (int32_t c = 0; c < n_pts; c += 64 * PD) {
      const int32_t cn = c + 64 * PD < n_pts ? c + 64 * PD : 0;  // (wave-uniform)
      {
        float2 pt = S.q0;
        asm volatile("" : "+v"(pt.x), "+v"(pt.y));
        S.q0 = pts[min(cn + lane, last)];
        feed(offsets(pt, c), c, true);
      }
      {
        float2 pt = S.q1;
        asm volatile("" : "+v"(pt.x), "+v"(pt.y));
        S.q1 = pts[min(cn + 64 + lane, last)];
        if (c + 64 < n_pts) feed(offsets(pt, c + 64), c + 64, true);
      }
    }
  }
  feed(zero_a, 0, false);  // (one more turn after the last chunk drains the list)
}

// (Tried, commit 9e18995: LANES = (list entry, block row) -- a lane holds 12 byte sums instead of 11 x 12, no transposing
//  reduction, 100 / 80 / 64 registers at 8 / 12 / 16 waves per workgroup.  Same records; bounds + seeds 3.16 -> 4.01 / 3.58 /
//  3.7 ms: decoding an entry per (entry, row) instead of per entry doubles the vector instructions per row, which eats what
//  the missing reduction saves, and six waves per SIMD do not make up for it.  profiles/r04_bounds_variants.txt.)
// (block row Y, block column X) of slot v of the 128-slot layout; false for the unused slots.
__device__ __forceinline__ bool slot_block(int v, int *Y, int *X) {
  const int lane = v & 63, i = v >> 6;
  const int r = 32 * i + 16 * ((lane >> 5) & 1) + 8 * ((lane >> 4) & 1) + 4 * ((lane >> 3) & 1) + 2 * ((lane >> 1) & 1) + (lane & 1);
  const int f = (lane >> 2) & 1;
  if (r >= 60) {
    *Y = 10;
    *X = r == 63 ? 1 + 2 * f : 4 * (r - 60) + 2 * f;
    return true;
  }
  const int y = r / 6, d = r % 6;
  if (d == 5 && f == 1) {  // the relocated values of block row 10
    *Y = 10;
    *X = 5 + 2 * y;
    return y < 3;
  }
  *Y = y;
  *X = d < 3 ? 4 * d + 2 * f : 4 * (d - 3) + 1 + 2 * f;
  return true;
}

// ---- second level: bounds of the four 4 x 4 sub-blocks of block (Y, X) ------------------------------------
// Sub-block (sy, sx) of a point with window origin (r, c) reads stored rows [r + 8Y + 4sy, + 4) and columns
// [c + 8X + 4sx, + 4): inside the 7 x 7 cells of P4[(r >> 2) + 2Y + sy][(c >> 2) + 2X + sx].  The table holds the
// byte pair {P4[i][j], P4[i + 1][j]} at (i, 2j): the four entries of a block are four consecutive bytes, ONE 8-byte
// load per point from a 4-byte-aligned offset -- against eight 12-byte loads for the block's exact sums.
// Returns the bounds (already scaled to the cell width) of sub-block q = 2 sy + sx in out[q], the same in every lane.
__device__ __forceinline__ void sub_bounds(const BnbParams &P, __amdgpu_buffer_rsrc_t p4, const float2 *pts, int32_t n_pts,
                                           float cf, float sf, int32_t cx, int32_t cy, int32_t Y, int32_t X, int lane,
                                           uint32_t scale, uint32_t (&out)[4]) {
  const int32_t DP = P.pool4_pitch;
  uint32_t A[4] = {0u, 0u, 0u, 0u};  // 32-bit sums, one per sub-block
  constexpr int U = 4;               // chunks whose loads are in flight together
  for (int32_t c = 0; c < n_pts; c += 64 * U) {
    uint32_t a[U];
    u32x2 w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int32_t idx = c + 64 * u + lane;
      a[u] = 0u;  // (no point: the table's first bytes lie in the zero border)
      if (idx < n_pts) {
        int32_t prow, pcol;
        window_origin(pts[idx], cf, sf, P, cx, cy, &prow, &pcol);
        a[u] = (uint32_t)(((prow >> 2) + 2 * Y) * DP + 2 * ((pcol >> 2) + 2 * X));
      }
      w[u] = __builtin_amdgcn_raw_buffer_load_b64(p4, (int)(a[u] & ~3u), 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t n = idx_guard(c + 64 * u + lane < n_pts, __builtin_amdgcn_alignbit(w[u].y, w[u].x, (a[u] & 2u) * 8u));
      A[0] += n & 0xffu;          // (sy 0, sx 0)
      A[2] += (n >> 8) & 0xffu;   // (sy 1, sx 0)
      A[1] += (n >> 16) & 0xffu;  // (sy 0, sx 1)
      A[3] += n >> 24;            // (sy 1, sx 1)
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int q = 0; q < 4; q++) A[q] += shfl_xor_u32(A[q], m);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) out[q] = A[q] * scale;
}

// Sub-block bounds of a strip of up to three blocks (Y, X0), (Y, X0 + 1), (Y, X0 + 2): their twelve table bytes are
// consecutive, ONE 16-byte load per list entry.  out[4 t + q]: block X0 + t, sub-block q = 2 sy + sx.
// `len` blocks are wanted (wave-uniform): their 4 len bytes start at a 2-byte-aligned offset, so 8 / 12 / 16 bytes are
// loaded -- the vector-memory address unit's time goes with the dwords a lane loads, and the candidates are bound by it.
// The list is the wave's origins merged by stored cell (CellList) or, where the wave keeps one, their runs by level-2
// entry (RunList): the address is a function of that entry alone, every member of a run reads the same bytes, and the
// sums are integers -- the twelve bounds come out the same from either list, from ~5 chunks of loads instead of ~12.
struct CellList {
  static constexpr int ROUNDS = 2, H = OC / ROUNDS;  // H: chunks whose loads are in flight together; a round past the list is skipped
  static __device__ __forceinline__ uint32_t entry(const uint32_t *list, int c) { return origin_of(list, c); }
  static __device__ __forceinline__ uint32_t offset(uint32_t o, uint32_t DP) { return (org_row(o) >> 2) * DP + 2u * (org_col(o) >> 2); }
  static __device__ __forceinline__ uint32_t count(uint32_t o) { return org_cnt(o); }
};
// (one round of H = 4, 5, 6 or 8 chunks, chosen by the list's length -- what the kernel pays for is load instructions, and 95 %
//  of a 1081-beam scan's rotations have 4 to 6 chunks of runs.  Past its end the run list reads as entries of no points in
//  the zero border.)
template <int CHUNKS>
struct RunList {
  static constexpr int ROUNDS = 1, H = CHUNKS;
  static __device__ __forceinline__ uint32_t entry(const uint32_t *list, int c) { return list[64 * c]; }
  static __device__ __forceinline__ uint32_t offset(uint32_t e, uint32_t DP) { return run_row2(e) * DP + 2u * run_col2(e); }
  static __device__ __forceinline__ uint32_t count(uint32_t e) { return run_cnt(e); }
};

// The bytes of a dword that are not zero, as bits 0 .. 3 (SWAR: bit 7 of every byte says so; one multiply gathers the four)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t n) {
  const uint32_t t = ((((n & 0x7f7f7f7fu) + 0x7f7f7f7fu) | n) & 0x80808080u) >> 7;
  return (t * 0x01020408u) >> 24;  // (bit 8 i -> bit 24 + i; no two products meet, so nothing carries)
}

// The packed sums of a strip over the list (`list`: the lane's word of chunk 0; nch: the list's chunks, wave-uniform) ...
// NOTE (run lists): every lane also leaves, per run, which of the strip's twelve level-2 bytes are not zero, in `note`
// (the lane's 16-bit word of chunk 0; bit 4 t + sy + 2 sx, the bytes' own order; a lane without a run: 0) -- the exact sums
// leave out the chunks of the cell list that hold only runs whose bytes are zero for the sub-blocks they take.
template <class LIST, bool NOTE = false>
__device__ __forceinline__ void strip_sums(const BnbParams &P, __amdgpu_buffer_rsrc_t p4, const uint32_t *list, int32_t nch,
                                           int32_t Y, int32_t X0, int len, uint32_t (&E)[3], uint32_t (&O)[3],
                                           uint16_t *note = nullptr) {
  const uint32_t DP = (uint32_t)P.pool4_pitch;
  const uint32_t off = (uint32_t)(2 * Y) * DP + (uint32_t)(4 * X0);
  constexpr int ROUNDS = LIST::ROUNDS, H = LIST::H;
#pragma unroll
  for (int h = 0; h < ROUNDS; h++) {
    if (H * h >= nch) continue;
    u32x4 w[H];
    uint32_t sh[H], cn[H];
    uint32_t aa[H];
#pragma unroll
    for (int j = 0; j < H; j++) {
      const uint32_t o = LIST::entry(list, H * h + j);
      // (lanes without a point: origin (0, 0), whose entries lie in the zero border)
      const uint32_t a = LIST::offset(o, DP) + off;
      sh[j] = (a & 2u) * 8u;
      aa[j] = a & ~3u;
      cn[j] = LIST::count(o);
    }
    if (len == 1) {
#pragma unroll
      for (int j = 0; j < H; j++) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(p4, (int)aa[j], 0, 0);
        w[j].x = v.x; w[j].y = v.y; w[j].z = 0u; w[j].w = 0u;
      }
    } else if (len == 2) {
#pragma unroll
      for (int j = 0; j < H; j++) {
        const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(p4, (int)aa[j], 0, 0);
        w[j].x = v.x; w[j].y = v.y; w[j].z = v.z; w[j].w = 0u;
      }
    } else {
#pragma unroll
      for (int j = 0; j < H; j++) w[j] = __builtin_amdgcn_raw_buffer_load_b128(p4, (int)aa[j], 0, 0);
    }
#pragma unroll
    for (int j = 0; j < H; j++) {
      const uint32_t n0 = __builtin_amdgcn_alignbit(w[j].y, w[j].x, sh[j]);
      const uint32_t n1 = __builtin_amdgcn_alignbit(w[j].z, w[j].y, sh[j]);
      const uint32_t n2 = __builtin_amdgcn_alignbit(w[j].w, w[j].z, sh[j]);
      // bytes of n_t: (sy 0, sx 0), (sy 1, sx 0), (sy 0, sx 1), (sy 1, sx 1) of block X0 + t
      E[0] += __umul24(n0 & M8, cn[j]); O[0] += __umul24((n0 >> 8) & M8, cn[j]);
      E[1] += __umul24(n1 & M8, cn[j]); O[1] += __umul24((n1 >> 8) & M8, cn[j]);
      E[2] += __umul24(n2 & M8, cn[j]); O[2] += __umul24((n2 >> 8) & M8, cn[j]);
      if (NOTE) {
        const uint32_t f = nonzero_bytes(n0) | (nonzero_bytes(n1) << 4) | (nonzero_bytes(n2) << 8);
        note[64 * (H * h + j)] = (uint16_t)(cn[j] != 0u ? f : 0u);
      }
    }
  }
}

// ... and the twelve bounds from them
template <class LIST, bool NOTE = false>
__device__ __forceinline__ void strip_bounds_c(const BnbParams &P, __amdgpu_buffer_rsrc_t p4, const uint32_t *list,
                                               int32_t nch, int32_t Y, int32_t X0, int len, uint32_t scale,
                                               uint32_t (&out)[12], uint16_t *note = nullptr) {
  uint32_t E[3] = {0u, 0u, 0u}, O[3] = {0u, 0u, 0u};  // 16-bit fields: at most 257 points per group of 8 lanes (cache_origins)
  if (std::is_same<LIST, CellList>::value) {
    strip_sums<CellList>(P, p4, list, nch, Y, X0, len, E, O);
  } else {
    static_assert(RUN_CHUNKS == 8, "the rounds below cover the run list");
    if (nch <= 4) strip_sums<RunList<4>, NOTE>(P, p4, list, nch, Y, X0, len, E, O, note);
    else if (nch == 5) strip_sums<RunList<5>, NOTE>(P, p4, list, nch, Y, X0, len, E, O, note);
    else if (nch == 6) strip_sums<RunList<6>, NOTE>(P, p4, list, nch, Y, X0, len, E, O, note);
    else strip_sums<RunList<8>, NOTE>(P, p4, list, nch, Y, X0, len, E, O, note);
  }
  // sums over the wave without LDS: the packed fields over groups of 8 lanes (quad permutations, then the mirror image
  // of the half row holds the other quad's sum), unpacked, over the row of 16 (its mirror image), then down the rows
  // (row_bcast:15 / :31 -- lane 63 ends with the total) and into a scalar register
#pragma unroll
  for (int t = 0; t < 3; t++) {
    E[t] = sum8(E[t]);
    O[t] = sum8(O[t]);
  }
#pragma unroll
  for (int t = 0; t < 3; t++) {
    out[4 * t + 0] = E[t] & 0xffffu;  // (0, 0)
    out[4 * t + 1] = E[t] >> 16;      // (0, 1)
    out[4 * t + 2] = O[t] & 0xffffu;  // (1, 0)
    out[4 * t + 3] = O[t] >> 16;      // (1, 1)
  }
#pragma unroll
  for (int q = 0; q < 12; q++) out[q] = wave_total_of8(out[q]) * scale;
}

}  // namespace
}  // namespace nhip
