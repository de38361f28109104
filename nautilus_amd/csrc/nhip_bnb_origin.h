// nhip_bnb_origin.h -- window origins of the branch-and-bound matcher's kernels (nhip_bnb.hip): where in the stored grid
// a point's lookup window starts under one rotation, and how a wave keeps a whole rotation's origins.
//
// Owns: window_origin (the spec's cell from single-precision arithmetic, with its double-precision rare path; LEAN: the
// form of the bounds phase, exact to the pooled entry), the rotation's (cos, sin) (rotation_k = rotation_terms + rotation_of;
// rotation_terms_of_wave: all of a wave's rotations at once, one per lane), patch_origin, the packed
// per-wave list of a rotation's origins in LDS (cache_origins, origin_of, org_row / org_col / org_cnt), the shorter list
// of their runs by level-2 entry (run_row2 / run_col2 / run_cnt; per run the chunks of the cell list its cells lie in,
// run_span), and the wave-uniform buffer descriptor every gather
// here reads through (uniform_rsrc, the u32xN load types, idx_guard).
// Assumes: BnbParams as launch_csm_bnb fills it (nhip_bnb_host.hip); a wave's list has ORG_WAVE words of LDS of its
// own, its run list RUN_WAVE; rows and columns of a stored grid below ORG_LIMIT for the packed form.  Included by
// nhip_bnb.hip only.
#pragma once
#include "nhip_bnb_params.h"
#include "nhip_bnb_wave.h"

namespace nhip {
namespace {

using namespace bnb;

// Window origins from single-precision arithmetic.  The spec's cell is floor(double(v) / res) (cimg_debug.h:31-37: float
// promoted to double, double division).  m = RN(v * RN_f32(1 / res)) differs from the true quotient q by at most
// |q| * 2^-23 (one rounding of the reciprocal, one of the product), and the spec's RN_double(q) by 2^-53 |q| more: the
// floors can differ only if m lies within that distance of an integer.  Lanes within |m| * 2^-22 of one (twice the bound;
// about one coordinate in 2,000 on the 1200-cell grid) take the double-precision path, so the result is the spec's,
// always.  From |m| >= 2^22 on (no fraction bits left to test) the cell is far outside any grid (sides <= 16384) on
// either path and the clamp decides; v_cvt_i32_f32 saturates.
// Window origin (stored-grid row, column of the top-left lookup cell) of point q under rotation (cf, sf): the
// same arithmetic as window_cell of nhip_csm.hip (spec: DESIGN.md section 3, items 1 and 3).
// LEAN (the bounds phase): see below; the candidates' kernels keep round 3's form -- the lean one costs the candidates'
// kernel of 16-bit grids, at its 96 registers, seven spilled dwords and 0.07 ms.
template <bool LEAN = false>
__device__ __forceinline__ void window_origin(float2 q, float cf, float sf, const BnbParams &P, int32_t cx, int32_t cy,
                                              int32_t *prow, int32_t *pcol) {
  const float xr = __fsub_rn(__fmul_rn(cf, q.x), __fmul_rn(sf, q.y));
  const float yr = __fadd_rn(__fmul_rn(sf, q.x), __fmul_rn(cf, q.y));
  const int32_t half = P.S / 2;
  const bool finite __attribute__((unused)) = (fabsf(xr) < 1e9f) && (fabsf(yr) < 1e9f);
  int32_t ix, iy;
  // the floors of both quotients with ONE test for the rare path, taken by the wave only if some lane needs it
  // (about one chunk in 16): the straight-line code has no nested exec masks.  A lane is "near" when either quotient
  // lies within |m| * 2^-22 of an integer -- which includes every |m| >= 2^22 (no fraction bits left), whose floors
  // the double-precision path then takes like any other.
  const float mx = __fmul_rn(xr, P.inv_res_f), my = __fmul_rn(yr, P.inv_res_f);
  const float fx = floorf(mx), fy = floorf(my);
  if (LEAN) {
    // The same test written so that it also holds for what is not a number: !(min(r, 1 - r) > tol) is true for NaN (an
    // infinite quotient: inf - inf), and every |v| >= 1e9 has |m| >= 2^22 at any cell size below 238 m, i.e. r == 0.  So
    // the points the spec calls non-finite all take the rare path, which gives them the floor that clamps to the window
    // position of a point that scores nothing (column -hx - 1, row -hy - 1: the lower clamp bounds), and the straight-line
    // code needs neither the two magnitude compares nor the selects -- one constant per coordinate after the clamp.
    const float rx = __fsub_rn(mx, fx), ry = __fsub_rn(my, fy);  // exact
    const float dx = fminf(rx, __fsub_rn(1.0f, rx)), dy = fminf(ry, __fsub_rn(1.0f, ry));
    const float tx = __fmul_rn(fabsf(mx), 0x1p-22f), ty = __fmul_rn(fabsf(my), 0x1p-22f);
    // (the lane mask straight from the compares, "unordered or <=": a ballot of the bool goes through a 0 / 1 register)
    const unsigned long long slow = __builtin_amdgcn_fcmpf(dx, tx, 13 /* ule */) | __builtin_amdgcn_fcmpf(dy, ty, 13 /* ule */);
    ix = (int32_t)fx;
    iy = (int32_t)fy;
    const int32_t kx = half + cx - P.hx + P.pad, ky = half + cy - P.hy + P.pad;  // (added after the clamp, below)
    if (slow != 0ull) {
      // Second stage, off the straight path.  The bounds phase uses only pcol >> 3 and prow >> 3 (the pooled entry), not
      // the cell.  For a near coordinate with |m| < 2^22 the quotient and m lie within |m| * 2^-23 < 1 / 2 of each other,
      // so the only integer that can separate them is n = rint(m): the spec's floor and the float floor are both n - 1 or
      // n.  The clamp c() is monotone with steps of 0 or 1: c(n - 1) and c(n) are equal, or they are n - 1 and n
      // themselves -- it creates no crossing that the unclamped values do not have -- and (n - 1 + K) >> 3 differs from
      // (n + K) >> 3 only where n + K is a multiple of 8 (K: the constant added after the clamp).  So a near coordinate
      // needs the double-precision floor only in that bucket, one time in eight; everywhere else the lane keeps
      // (int)floorf(m): its cell may be off by one, its pooled entry is not.  A coordinate that is not near has the
      // spec's floor already.  What stays: quotients that are not numbers and |m| >= 2^22 (which includes every point the
      // spec calls non-finite, see above) -- "!(|m| < 2^22)" holds for both.
      // (bitwise: straight-line code on lane masks, no short-circuit branches)
      const bool near_x = !(dx > tx), near_y = !(dy > ty);
      const bool big = (int)!(fabsf(mx) < 0x1p22f) | (int)!(fabsf(my) < 0x1p22f);
      const int32_t nx = (int32_t)rintf(mx), ny = (int32_t)rintf(my);  // (saturating; `big` covers what does not fit)
      const bool stay = (int)big | ((int)near_x & (int)(((nx + kx) & 7) == 0)) | ((int)near_y & (int)(((ny + ky) & 7) == 0));
      if (__builtin_amdgcn_ballot_w64(stay) != 0ull) {
        if (stay) {
          // (the magnitude test on the promoted values -- 1e9 is a float -- so that it stays on this path)
          const double xd = (double)xr, yd = (double)yr;
          const bool fin = (fabs(xd) < 1e9) && (fabs(yd) < 1e9);
          ix = (int32_t)fmin(fmax(floor_quotient(xd, P.res, P.inv_res), -2147483000.0), 2147483000.0);
          iy = (int32_t)fmin(fmax(floor_quotient(yd, P.res, P.inv_res), -2147483000.0), 2147483000.0);
          if (!fin) ix = iy = -2147483000;
        }
      }
    }
    const int32_t lo_x = -P.hx - 1 - half - cx, lo_y = -P.hy - 1 - half - cy;
    ix = min(max(ix, lo_x), P.S + P.hx - half - cx);
    iy = min(max(iy, lo_y), P.S + P.hy - half - cy);
    *pcol = ix + kx;
    *prow = iy + ky;
    return;
  }
  const float rx = __fsub_rn(mx, fx), ry = __fsub_rn(my, fy);  // exact
  const bool near = fminf(rx, __fsub_rn(1.0f, rx)) <= __fmul_rn(fabsf(mx), 0x1p-22f) ||
                    fminf(ry, __fsub_rn(1.0f, ry)) <= __fmul_rn(fabsf(my), 0x1p-22f);
  ix = (int32_t)fx;
  iy = (int32_t)fy;
  if (__builtin_amdgcn_ballot_w64(near && finite) != 0ull) {
    if (near && finite) {
      ix = (int32_t)fmin(fmax(floor_quotient((double)xr, P.res, P.inv_res), -2147483000.0), 2147483000.0);
      iy = (int32_t)fmin(fmax(floor_quotient((double)yr, P.res, P.inv_res), -2147483000.0), 2147483000.0);
    }
  }
  ix = min(max(ix, -P.hx - 1 - half - cx), P.S + P.hx - half - cx);
  iy = min(max(iy, -P.hy - 1 - half - cy), P.S + P.hy - half - cy);
  // col = clamp(S / 2 + floor(xr / res) + cx, -hx - 1, S + hx), as window_cell of nhip_csm.hip -- with the clamp
  // applied to the quotient's floor, so that everything stays in 32-bit arithmetic; non-finite points score nothing
  const int32_t col = finite ? half + ix + cx : -P.hx - 1, row = finite ? half + iy + cy : -P.hy - 1;
  *pcol = col - P.hx + P.pad;
  *prow = row - P.hy + P.pad;
}

// Rows of the stored grid are read through a buffer descriptor of the pair's grid slot: 12 bytes at a 4-byte-aligned
// offset in ONE instruction (buffer_load_dwordx3; hipcc splits the same read through a flat pointer into two
// overlapping 8-byte loads).  Every load instruction costs the L1 one tag lookup per lane and line, and the block
// evaluation is bound by exactly that.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Buffer descriptor of a wave-uniform range.  The inputs pass through readfirstlane so that hipcc can PROVE the
// descriptor uniform and keeps it in SGPRs: a descriptor it parks in VGPRs costs a serialising "waterfall" loop of
// ~10 instructions around every single buffer load.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void *base, int64_t bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
  const int n = __builtin_amdgcn_readfirstlane((int)(bytes < 0x7fffffffll ? bytes : 0x7fffffffll));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
}

__device__ __forceinline__ uint32_t idx_guard(bool live, uint32_t v) { return live ? v : 0u; }

// R(theta0) * R(delta_k), composed in double with individually rounded ops (as csm_correlate_kernel): the four terms
// from memory, and (cos, sin) from them.
struct RotationTerms {
  double c0, s0, cd, sd;
};
__device__ __forceinline__ RotationTerms rotation_terms(const BnbParams &P, int32_t pair, int32_t k) {
  RotationTerms T;
  T.c0 = P.rot0_cs[2 * pair];
  T.s0 = P.rot0_cs[2 * pair + 1];
  const int32_t kd = k + (P.pair_kbase ? P.pair_kbase[pair] : 0);  // (the pair's rotation k is entry kbase + k of the table)
  T.cd = P.delta_cs[2 * kd];
  T.sd = P.delta_cs[2 * kd + 1];
  return T;
}
__device__ __forceinline__ void rotation_of(const RotationTerms &T, float *cf, float *sf) {
  *cf = __double2float_rn(__dsub_rn(__dmul_rn(T.c0, T.cd), __dmul_rn(T.s0, T.sd)));
  *sf = __double2float_rn(__dadd_rn(__dmul_rn(T.s0, T.cd), __dmul_rn(T.c0, T.sd)));
}
__device__ __forceinline__ void rotation_k(const BnbParams &P, int32_t pair, int32_t k, float *cf, float *sf) {
  rotation_of(rotation_terms(P, pair, k), cf, sf);
}

// The rotations of one wave of the bounds loop (csm_bnb_kernel: k = wave, wave + WAVES, ...), all at once: lane i returns
// the terms of the wave's i-th rotation, k = wave + WAVES * i; the caller composes them (rotation_of) and its loop takes
// (cos, sin) out of the two registers by v_readlane.  rotation_k at the head of every rotation was three dependent round trips with nothing to hide behind
// (rot0_cs[pair], pair_kbase[pair], delta_cs[kd]; profiles/r15_bounds_round_trips_isa.txt); here they are paid once per
// wave, in parallel over its rotations, and the caller puts the staging of the pooled table between the loads (this
// function) and rotation_of.  The lanes past the wave's last rotation read that rotation's entry again: no address is
// formed that the loop would not read itself, under a pair_kbase too.  A wave without a rotation (wave >= n_theta) loads
// nothing.  The values are rotation_k's, bit for bit: the same two functions compute them.
template <int WAVES>
__device__ __forceinline__ RotationTerms rotation_terms_of_wave(const BnbParams &P, int32_t pair, int32_t wave, int lane) {
  static_assert(MAX_ROT <= 64 * WAVES, "a wave's rotations fit its lanes");
  RotationTerms T = {1.0, 0.0, 1.0, 0.0};
  if (wave < P.n_theta) {
    const int32_t mine = (P.n_theta - 1 - wave) / WAVES + 1;  // (>= 1)
    T = rotation_terms(P, pair, wave + WAVES * min(lane, mine - 1));
  }
  return T;
}

// Byte offset (into the grid slot) of the aligned dword that holds the first cell of a point's 8 x 8 patch of block
// (Y, X), and the bit shift of that cell inside it (8-bit cells).  Lanes without a point read the zero border
// (row 0 of the stored image).
__device__ __forceinline__ void patch_origin(const BnbParams &P, bool live, float2 q, float cf, float sf, int32_t cx,
                                             int32_t cy, int32_t Y, int32_t X, uint32_t *g, uint32_t *sh) {
  *g = 0u;
  *sh = 0u;
  if (live) {
    int32_t prow, pcol;
    window_origin(q, cf, sf, P, cx, cy, &prow, &pcol);
    const int32_t col = pcol + BNB_B * X;
    *g = (uint32_t)((prow + BNB_B * Y) * P.pitch + (col & ~3));
    *sh = (uint32_t)(col & 3) * 8u;
  }
}

// ==== the same three passes with the window origins of one rotation kept by the wave ========================
// All candidates of rotation k share the 1081 window origins; computing them (a point load, two double-precision
// floor quotients) per candidate made every pass a chain of dependent latencies.  A wave that owns rotation k keeps
// them packed (row << 16 | column; both < 65536) in LDS -- OCL chunks of 64, scans of up to 64 * OCL points, in the
// space of the pooled table, which the workgroup no longer needs once its bounds are done -- and a pass becomes:
// all loads of six to nine chunks issued back to back, then the adds.  (Held in 18 registers they were spilled:
// the register allocator kept the array in scratch memory and the kernel wrote 7 GB of it per launch.)  Lanes
// without a point hold origin (0, 0): every patch of theirs lies in the zero border (8 * NB + 7 < pad) and pooled
// entries there are zero.

// Entry format: row << 19 | column << 6 | (points - 1): consecutive beams that fall into the SAME stored cell (a third
// of a 1081-beam scan's) have the same window origin and read the same bytes in every bound and every exact sum of
// the rotation; they are kept as one entry with their number, and every sum adds the entry's bytes that many times.
// 749 entries instead of 1081 points on the bench workload: 12 chunks of loads instead of 17 in everything that
// follows.  Rows and columns < 8192 (grids up to 8000 cells + border; larger ones take the general kernel).
constexpr int ORG_COL_SHIFT = 6, ORG_ROW_SHIFT = 19;
__device__ __forceinline__ uint32_t org_row(uint32_t o) { return o >> ORG_ROW_SHIFT; }
__device__ __forceinline__ uint32_t org_col(uint32_t o) { return (o >> ORG_COL_SHIFT) & (ORG_LIMIT - 1u); }
__device__ __forceinline__ uint32_t org_cnt(uint32_t o) { return (o & 63u) + 1u; }

// (entry of chunk c for this lane; `org` points at the lane's word of chunk 0.  Past the list: row 0, column 0, whose
//  cells lie in the zero border)
__device__ __forceinline__ uint32_t origin_of(const uint32_t *org, int c) { return c < OCL ? org[64 * c] : 0u; }

// ---- the second list: runs of origins by level-2 entry
// The strip bounds (nhip_bnb_bounds.h) read the level-2 table at an address that depends only on the origin's 4 x 4 entry
// (row >> 2, column >> 2), and consecutive beams run along walls: of a 1081-beam scan's ~750 cells ~300 start a new
// entry.  A wave that has LDS for it (`runs`: RUN_WAVE words) writes, beside the list above, one word per RUN -- a live
// lane whose entry differs from its predecessor's, or that starts a 64-point chunk (so a run has at most 64 points;
// A, B, A stays three runs) -- as the origin's word with the bits below the entry cleared and the run's points in the
// cleared count field: (row >> 2) << 21 | (column >> 2) << 8 | points (1 .. 64; 0: no entry, adds nothing).
constexpr uint32_t RUN_KEY_MASK = (~0u << (ORG_ROW_SHIFT + 2)) | (((ORG_LIMIT >> 2) - 1u) << (ORG_COL_SHIFT + 2));
__device__ __forceinline__ uint32_t run_row2(uint32_t e) { return e >> (ORG_ROW_SHIFT + 2); }
__device__ __forceinline__ uint32_t run_col2(uint32_t e) { return (e >> (ORG_COL_SHIFT + 2)) & ((ORG_LIMIT >> 2) - 1u); }
__device__ __forceinline__ uint32_t run_cnt(uint32_t e) { return e & 127u; }
// What cache_origins says of the run list: the number of its 64-entry chunks (>= 1: the strip bounds may walk it), or why
// there is none -- not asked for; some aligned group of 8 lanes would hold more than 257 points (the same limit of the
// 16-bit fields as the cell list's, checked on its own: runs concentrate the counts), which includes every rotation whose
// cell list had to be rebuilt unmerged; more than RUN_WAVE runs.  Such a rotation takes the strip bounds per cell.
enum : int32_t { RUNS_NONE = 0, RUNS_FIELD = -1, RUNS_FULL = -2 };

// Returns the number of 64-entry chunks of the list (wave-uniform).  The packed sums of the bounds and exact sums hold
// 16-bit fields that are added over 8 lanes before they are unpacked: the points of every aligned group of 8 lanes,
// over all chunks, must not exceed 257 (257 * 255 = 65,535).  One point per entry keeps that by construction (<= 18
// chunks); with merged entries the wave checks it and, if a group would pass the limit (hundreds of beams in a few
// cells), builds the list again with one point per entry.
// `merged`: measured on 10,000 pairs with row-major planes 7.45 -> 7.38 ms for 16-bit grids and 6.81 -> 6.93 ms for
// 8-bit ones (the multiply-adds that replace the adds cost what the loads saved); with the tiled planes both widths
// merge (8-bit: 6.31 -> 6.25 ms).
// RUNS (with `runs`, the wave's RUN_WAVE words, and want_runs, wave-uniform): the run list is written in the same sweep
// and *run_chunks says what became of it (above); run_span (RUN_WAVE bytes of the wave's, or null): per run written, the
// chunk of the cell list that holds its first cell | 32 if its last cell lies in the next (nhip_bnb.hip chunk_mask).
// RING: the form of the loop over the scan's chunks, see there -- the ring of the candidates' kernels (the callers with
// RUNS) or the slots of the seeds.
template <bool RUNS = false, bool RING = RUNS>
__device__ __forceinline__ int32_t cache_origins(const BnbParams &P, const float2 *pts, int32_t n_pts, float cf, float sf,
                                                 int32_t cx, int32_t cy, int lane, uint32_t *org, bool merged,
                                                 uint32_t *runs = nullptr, bool want_runs = false,
                                                 int32_t *run_chunks = nullptr, uint8_t *run_span = nullptr) {
  uint32_t *base = org - lane;  // the wave's list
  const bool with_runs = RUNS && want_runs;
  if (RUNS) *run_chunks = RUNS_NONE;
  for (int merge = merged ? 1 : 0; merge >= 0; merge--) {
    // (the seeds, !RING.)  The points of the next D chunks are in flight while one chunk's origins are computed.  Each of
    // the D slots is a register pair of its own and a turn of the loop works all D (the turn is rolled: the origin
    // arithmetic holds a division on its rare path), so that the wait before a slot's points are used is vmcnt(D - 1): it
    // admits the D - 1 loads issued after it.  The form is coarse_rotation's (nhip_bnb_bounds.h, which says what loses the
    // depth again): the points leave the slot through an opaque copy and the slot's next chunk is loaded straight into
    // it, unconditionally, from an offset clamped to the scan's last point; every slot loads on every turn and only the
    // bodies after the first are predicated; the priming loads are issued in slot order.  D = 3, 4 and 6 measured the
    // same (bounds + seeds 2.71 -> 2.66 ms, profiles/r14_point_prefetch.txt); three take the fewest registers.
    constexpr int D = 3;
    uint32_t tail = 0u;  // entries written (wave-uniform)
    uint32_t rtail = 0u;  // runs found (wave-uniform; those past RUN_WAVE are not written)
    // the entries of chunk c (64 * c < n_pts) from its points
    auto chunk = [&](float2 pt, int c) {
      const int32_t idx = 64 * c + lane;
      const bool live = idx < n_pts;
      uint32_t o = 0u;
      if (live) {
        int32_t prow, pcol;
        window_origin(pt, cf, sf, P, cx, cy, &prow, &pcol);
        o = ((uint32_t)prow << ORG_ROW_SHIFT) | ((uint32_t)pcol << ORG_COL_SHIFT);
      }
      // runs of equal origins inside the chunk: the predecessor's by a DPP shift across the wave
      const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)o, (int)o, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
      const bool head = live && (lane == 0 || o != prev || merge == 0);
      const unsigned long long H = __ballot(head), L = __ballot(live);
      // run length = distance to the next head, or to the end of the chunk's live lanes
      const unsigned long long rest = ((H | ~L) >> lane) >> 1;  // (a dead lane ends the run as a head would)
      const uint32_t cnt = rest ? (uint32_t)__builtin_ctzll(rest) + 1u : (uint32_t)(64 - lane);
      if (head) {
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(H >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)H, 0u));
        base[tail + before] = o | (cnt - 1u);
      }
      tail += (uint32_t)__builtin_popcountll(H);
      if (RUNS && with_runs && merge) {
        // (a run's head is a cell's head too: the same predecessor, compared above the entry's low bits)
        const bool head2 = live && (lane == 0 || ((o ^ prev) & RUN_KEY_MASK) != 0u);
        const unsigned long long H2 = __ballot(head2);
        const unsigned long long rest2 = ((H2 | ~L) >> lane) >> 1;
        const uint32_t cnt2 = rest2 ? (uint32_t)__builtin_ctzll(rest2) + 1u : (uint32_t)(64 - lane);
        const uint32_t at = rtail + __builtin_amdgcn_mbcnt_hi((uint32_t)(H2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)H2, 0u));
        if (head2 && at < (uint32_t)RUN_WAVE) runs[at] = (o & RUN_KEY_MASK) | cnt2;
        if (run_span) {
          // The chunks of the cell list the run's cells lie in.  A run's head is a cell's head too: its first cell is entry
          // first = (entries before this chunk's) + (heads below the lane), its cells are the heads among its cnt2 lanes --
          // at most 64, so they end in the first cell's chunk or the next.
          const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(H >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)H, 0u));
          const uint32_t first = tail - (uint32_t)__builtin_popcountll(H) + below;
          const uint32_t end = (uint32_t)lane + cnt2;  // (<= 64)
          const unsigned long long upto = end >= 64u ? H : H & ((1ull << end) - 1ull);
          const uint32_t last = first + (uint32_t)__builtin_popcountll(upto) - below - 1u;
          if (head2 && at < (uint32_t)RUN_WAVE) run_span[at] = (uint8_t)((first >> 6) | ((last >> 6) != (first >> 6) ? 32u : 0u));
        }
        rtail += (uint32_t)__builtin_popcountll(H2);
      }
    };
    const int32_t n_in = min(n_pts, 64 * OCL);  // (the list holds OCL chunks; the callers send no longer scan here)
    if (RING) {
      // The candidates' kernels: a ring of R chunks that rotates so that its indices stay static.  Its compiled loop
      // awaits, at the back-edge, the load the turn has just issued -- and the slots below, which do not, were worth
      // 0.03 ms of these kernels' 2.48, inside the spread of their runs (profiles/r14_point_prefetch.txt: the waits
      // move into the exact sums, whose loads the address unit serialises anyway).  So they keep the parent's code.
      constexpr int R = 6;
      float px[R], py[R];
#pragma unroll
      for (int d = 0; d < R; d++) {
        const float2 q = 64 * d + lane < n_pts ? pts[64 * d + lane] : make_float2(0.f, 0.f);
        px[d] = q.x;
        py[d] = q.y;
      }
#pragma unroll 1
      for (int c = 0; c < OCL; c++) {
        const int32_t idx = 64 * c + lane;
        if (64 * c >= n_pts) break;
        const float2 pt = make_float2(px[0], py[0]);
        const float2 qn = idx + 64 * R < n_pts ? pts[idx + 64 * R] : make_float2(0.f, 0.f);
#pragma unroll
        for (int d = 0; d < R - 1; d++) {
          px[d] = px[d + 1];
          py[d] = py[d + 1];
        }
        px[R - 1] = qn.x;
        py[R - 1] = qn.y;
        chunk(pt, c);
      }
    } else if (n_in > 0) {  // (an empty scan loads nothing)
      // (a 32-bit byte offset from the wave-uniform pointer, at most 8 * 64 * OCL: one address register per load)
      const uint32_t last = 8u * (uint32_t)(n_in - 1);
      auto point_at = [&](int32_t i) {
        return *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(pts) + min(8u * (uint32_t)i, last));
      };
      float2 q[D];
#pragma unroll
      for (int d = 0; d < D; d++) {
        // (the offset opaque: these addresses are the same for every rotation, and kept across the caller's loop over
        //  its rotations they cost the kernel of 16-bit grids, at its 96 registers, spilled dwords)
        int32_t i = 64 * d + lane;
        asm volatile("" : "+v"(i));
        q[d] = point_at(i);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll 1
      for (int c = 0; 64 * c < n_in; c += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
          float2 pt = q[d];
          asm volatile("" : "+v"(pt.x), "+v"(pt.y));
          q[d] = point_at(64 * (c + d + D) + lane);
          if (d == 0 || 64 * (c + d) < n_in) chunk(pt, c + d);
        }
      }
    }
    const int32_t nch = (int32_t)((tail + 63u) >> 6);
    // (the rest of the list reads as row 0, column 0: the sums below unroll over groups of chunks and may read past nch)
    for (uint32_t e = tail + (uint32_t)lane; e < (uint32_t)ORG_WAVE; e += 64u) base[e] = 0u;
    // (... and the rest of the run list as entries of no points)
    if (RUNS && with_runs && merge)
      for (uint32_t e = rtail + (uint32_t)lane; e < (uint32_t)RUN_WAVE; e += 64u) runs[e] = 0u;
    // (the wave reads only its own words back: LDS operations of one wave are performed in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (merge == 0) {
      if (RUNS && with_runs) *run_chunks = RUNS_FIELD;
      return nch;
    }
    // the points of this lane's entries, summed over the aligned group of 8 lanes
    uint32_t w = 0u;
    for (int c = 0; c < nch; c++) {
      const uint32_t e = org[64 * c];
      w += 64u * (uint32_t)c + (uint32_t)lane < tail ? org_cnt(e) : 0u;
    }
    w = sum8(w);
    if (__ballot(w > 257u) == 0ull) {
      if (RUNS && with_runs) {
        // the same check of the run list, whose fields hold whole runs
        const int32_t nrc = (int32_t)((rtail + 63u) >> 6);
        uint32_t w2 = 0u;
        if (rtail <= (uint32_t)RUN_WAVE)
          for (int c = 0; c < nrc; c++) w2 += run_cnt(runs[64 * c + lane]);
        w2 = sum8(w2);
        *run_chunks = rtail > (uint32_t)RUN_WAVE ? RUNS_FULL : (__ballot(w2 > 257u) != 0ull ? RUNS_FIELD : nrc);
      }
      return nch;
    }
    __builtin_amdgcn_wave_barrier();
  }
  return 0;  // (not reached)
}

}  // namespace
}  // namespace nhip
