// nhip_bnb_params.h -- kernel parameters of the branch-and-bound matcher, shared by its two translation units:
// nhip_bnb.hip (the product kernels) and nhip_bnb_instr.hip (the same kernels with their instrumentation compiled in).
#pragma once
#include "nhip_common.h"
#include "nhip_csm_shared.h"  // (ScoreGate)

namespace nhip {
namespace bnb {

// ---- sizes the kernels (nhip_bnb.hip) and their host side (nhip_bnb_host.hip) share
constexpr int BNB_WAVES = 8;          // waves per workgroup of csm_bnb_kernel
constexpr int NB = BNB_MAX_NB;        // blocks per axis held in registers (11: nx, ny <= 88)
constexpr int MAX_ROT = 340;          // rotations per search: QCAP * 4 bytes hold their 12 bytes of ordering data
constexpr int QCAP = 1024;            // candidate queue entries per workgroup (overflow is evaluated by the wave that found it)
// Waves per workgroup of the split form's first kernel (bounds + seeds).  What bounds that kernel is the latency of a
// wave's own instruction chain more than issue slots: with ONE workgroup per CU (two waves per SIMD) it takes 1.63x the
// time of two.  Five waves per SIMD would need workgroups of ten waves at 96 registers; built and twice as slow -- ten
// waves spread 3 + 3 + 2 + 2 over the SIMDs, a second workgroup's would make six on two of them, which 96 registers do
// not allow, so ONE workgroup was resident per CU.  Twelve waves need 80 registers, a third workgroup of eight also 53 KB
// of LDS (profiles/r04_bounds_variants.txt).
constexpr int SPLIT_WAVES = 8;
constexpr int LIST_ENTRIES = 128;     // ring of pending run-list entries per wave (a chunk appends <= 64, 64 are consumed at a time)
constexpr int RUN_SHIFT = 25;         // run-list entry = pooled offset | (index of the run's first point mod 128) << RUN_SHIFT
constexpr int OC = 18;                // 64-entry chunks the by-rotation passes are unrolled for
constexpr int OCL = 17;               // chunks of window origins a wave holds: 1088 points (a 1081-beam scan)
constexpr int ORG_WAVE = OCL * 64;    // words of LDS per wave
constexpr int ORG_LDS = BNB_WAVES * ORG_WAVE * 4;  // bytes per workgroup (34,816: the 1200 x 1200 grid's pooled table is 35,712)
constexpr uint32_t ORG_LIMIT = 1u << 13;           // rows / columns of a stored grid the packed origins hold
// The second list of the kernels that work candidates rotation by rotation (csm_bnb_cand_kernel, csm_bnb_rot_kernel): runs of
// consecutive origins inside one 4 x 4 level-2 entry, which is all the strip bounds read (nhip_bnb_origin.h has the format).
constexpr int RUN_CHUNKS = 8;                      // 64-entry chunks of runs a wave holds: 512 runs (a 1081-beam scan: ~300)
constexpr int RUN_WAVE = RUN_CHUNKS * 64;          // words of LDS per wave
// Beside the run list those kernels keep, per run, the strip's level-2 bytes that are not zero (a 16-bit word: bit 4 t + sy +
// 2 sx for sub-block (sy, sx) of the strip's block t, written by the strip bounds) and the chunks of the cell list the run's
// cells lie in (a byte: first chunk | reaches the next << 5, written with the run list): what the exact sums need to leave
// out the chunks of the cell list that hold only empty windows (nhip_bnb.hip chunk_mask).  3 bytes per run.
constexpr int RUN_NOTE_BYTES = RUN_WAVE * 3;

// ---- the dynamic LDS of csm_bnb_kernel, in this order (the kernel carves it, bnb_plan and launch_main size it):
//   first region   the pooled table while the bounds are computed (if staged), then the waves' window origins
//   bounds         n_theta rows of 128 words
//   queue's space  words of 8 bytes: QCAP entries of the candidate queue -- or, in the split form, which has no queue,
//                  QSPACE_SPLIT words for the run lists of its SPLIT_WAVES waves and the rotations' maxima and order
//                  (the fused form keeps those in the queue's two halves)
//   LdsTail        in LDS_TAIL_BYTES
constexpr int QSPACE_SPLIT = (SPLIT_WAVES * LIST_ENTRIES * 4 + MAX_ROT * 12 + 15) / 16 * 2;
constexpr int lds_qspace(bool split) { return split ? QSPACE_SPLIT : QCAP; }
// bnb_fits() checks the fused form's size only: it holds for the split form because that form's is no larger
static_assert(QSPACE_SPLIT <= QCAP, "the split form's LDS must not exceed the fused form's, which bnb_fits() checks");
struct LdsTail {
  unsigned long long best;  // the pair's running best key
  uint32_t cnt[6];          // [0], [3..5]: work counters (instrumented build); [LDS_QN]: candidates counted / queued;
                            // [LDS_QHEAD]: next queue entry or rank to hand out
  unsigned long long slow;  // (stats: the slowest wave's time in the candidate phase)
  uint32_t top;             // (score gate: the workgroup's highest bound)
};
constexpr int LDS_QN = 1, LDS_QHEAD = 2, LDS_TAIL_BYTES = 64;
static_assert(sizeof(LdsTail) <= LDS_TAIL_BYTES, "the tail fits its 64 bytes");
// bytes of dynamic LDS of a launch whose first region has `first` bytes (a multiple of 16)
constexpr size_t lds_bytes(size_t first, int32_t n_theta, bool split) {
  return first + (size_t)n_theta * 128 * 4 + (size_t)lds_qspace(split) * 8 + LDS_TAIL_BYTES;
}

constexpr int BNB_STATS_PAIRS = 1 << 20;           // per-pair counters kept by NHIP_BNB_STATS=1
constexpr int BNB_STATS_HEAD = 24;    // totals: 4 counts, shader-clock sums of the by-rotation kernel, the strip paths (see nhip_bnb_stats_levels)
constexpr int BNB_STATS_CHUNKS = 4;   // behind the per-pair counts: chunk visits of the exact sums (see nhip_bnb_stats_chunks)
constexpr int BNB_STATS_SEEDS = 8;    // behind those: the seeds' clocks by part and their counts (see nhip_bnb_stats_seeds)

// One rotation of a pair with many candidates, handed to the second kernel: (pair, rotation) and the mask of its
// 121 candidate blocks.
struct RotEntry {
  unsigned long long w[4];  // w[0]: pair << 24 | rotation; w[1..3]: candidate blocks 0..40, 41..81, 82..120
};

struct BnbParams {
  const float2 *xy;
  const int32_t *offsets;
  const uint8_t *grids;
  const int32_t *pair_src;
  const int32_t *pair_slot;
  IdBounds ids;  // counts the pairs' scan ids and grid slots are checked against (nhip_common.h)
  const double *rot0_cs;
  const double *delta_cs;
  const int32_t *pair_origin;
  const int32_t *pair_kbase;  // optional: entry of delta_cs that is pair i's rotation 0 (a search's rotations dealt over
                              // several "pairs" = workgroups: nhip_csm_get_transformation's fine level); null = 0
  unsigned long long *keys;
  unsigned long long *timeline;  // optional (NHIP_BNB_TIMELINE=1): per pair 4 x 100 MHz ticks: start, bounds, seeds, end
  unsigned long long *stats;  // optional: [0] blocks evaluated whole, [1] blocks in all, [2] candidates refined,
                              //   [3] 4 x 4 sub-blocks evaluated; then one count of candidates per pair
  RotEntry *rot_list;          // optional lists of (pair, rotation) work items in the caller's workspace, one per XCD so
  uint32_t *rot_count;        //   that a pair's rotations are worked where its grid is L2-resident; per XCD 32 bytes of
  uint32_t rot_cap;           //   counters {filled, next}; entries per list
  uint32_t heavy_min;         // candidates (after the seeds) from which a PAIR hands its rotations over ...
  uint32_t keep_ranks;        // ... except its first keep_ranks rotations in best-first order (one per wave)
  // Split form (large batches): the workgroup of a pair ends after bounds and seeds and leaves its state -- per live
  // rotation, best first, the 128-word row of block bounds (word 126: the rotation's highest bound, word 127: the
  // rotation) -- in the caller's workspace; the candidates are worked by a second launch, heaviest pairs first.
  uint32_t *ps_rows;    // [pair][rank][128]; null = the fused form
  uint32_t *ps_count;   // [pair] candidate blocks the seeds have left
  uint32_t *ps_live;    // [pair] rotations with at least one of them
  uint32_t *ps_next;    // [pair] next rank to hand out (pairs worked by several workgroups)
  uint32_t *ps_nw;      // [pair] workgroups of the second launch that share the pair
  int32_t *ps_work;     // [8][ps_work_stride] pair of each workgroup of the second launch (-1: none), per XCD
  uint32_t *ps_ticket;  // spread form: counter of additional workgroups dealt over the eight lists (null: round 3's lists)
  int32_t ps_work_stride;
  uint32_t split_min;   // candidates per additional workgroup of a pair
  uint32_t split_max;   // workgroups per pair at most
  uint32_t front_min;   // candidates from which a pair's workgroups go to the FRONT of its XCD's list (0: pair order throughout)
  int32_t pair_base;    // index of this launch's pair 0 in the caller's arrays (rounds of the split form): what a bad id is reported at
  int32_t n_pairs, n_theta, nx, ny, hx, hy, nbx, nby;
  int32_t S, pad, pitch, rows, max_shift;
  int32_t pool_pitch, pool_rows, pairs_per_xcd;
  int32_t pool4_pitch;
  int32_t lds_first;    // bytes of the kernel's first LDS region: max(pooled table if staged, origins)
  int32_t general_all;  // the general instantiation takes every pair (NHIP_BNB_QUEUE=1)
  int32_t short_scans;  // the caller vouches that every scan fits the by-rotation form (NHIP_SEARCH_SHORT_SCANS)
  int32_t levels;  // 2: candidates are refined through the 4 x 4 sub-block bounds; 1: evaluated whole (NHIP_BNB_LEVELS)
  int64_t grid_bytes, skip_bytes, slot_bytes, pool_bytes, pool4_bytes;
  int64_t hi_offset, hi_bytes;  // 16-bit grids: the plane of high bytes inside a slot
  int32_t hi_pitch;
  int32_t hi_tpr;          // tiles per tile row and bytes of one copy of the tiled plane (nhip_common.h hi_tiled)
  int64_t hi_copy_bytes;
  int64_t t16_bytes;       // the tiled copy of the 16-bit image behind the two copies (nhip_common.h t16_tiled)
  int32_t t16_tpr;
  double res, inv_res;
  float inv_res_f;  // RN_f32(1 / res): the single-precision path of the window origins
  ScoreGate gate;   // the caller's min_score (nhip_csm_match_gated): a pair's best starts at its floor key (nhip_csm_shared.h)
  int32_t l2_runs;  // strip bounds from the list of level-2 runs where a kernel keeps one (0: NHIP_BNB_L2_RUNS=0, per cell everywhere)
  int32_t pair_subs;  // two live sub-blocks side by side on a strip's sub-block row share one pass (0: NHIP_BNB_PAIR_SUBS=0, one pass each)
  int32_t zero_chunks;  // exact sums leave out the cell-list chunks whose windows hold only empty cells (0: NHIP_BNB_ZERO_CHUNKS=0, every chunk)
  int32_t seed_bounds;  // a seed pass takes its block's sub-block bounds even while the pair's best sum is 0 (1: NHIP_BNB_SEED_BOUNDS=1; 0: it does not)
};

// The kernel launches of one batch in each build: launchers_product() (nhip_bnb.hip), launchers_instr()
// (nhip_bnb_instr.hip: the build that honours P.stats / P.timeline).  split_a: the split form's bounds + seeds + the
// ordering of the pairs by candidates left; split_b: its candidates (on any stream ordered behind split_a).
using BnbLaunch = int (*)(const BnbParams &P, const BnbPlan &plan, hipStream_t s);
struct BnbLaunchers { BnbLaunch fused, split_a, split_b; };
BnbLaunchers launchers_product();
BnbLaunchers launchers_instr();

}  // namespace bnb
}  // namespace nhip
