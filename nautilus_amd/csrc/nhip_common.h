// nhip_common.h -- shared internals of libnautilus_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nautilus_hip_debug.h"  // (the contract, nautilus_hip.h, and the timer ids)

namespace nhip {

// ---- error plumbing (thread-local message, int codes across the ABI) ----
void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define NHIP_TRY_HIP(expr)                                            \
  do {                                                                \
    hipError_t _e = (expr);                                           \
    if (_e != hipSuccess) return ::nhip::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)

#define NHIP_REQUIRE(cond, ...)          \
  do {                                   \
    if (!(cond)) {                       \
      ::nhip::set_error(__VA_ARGS__);    \
      return NHIP_ERR_ARG;               \
    }                                    \
  } while (0)

int require_device();

// Environment switches that select a form of the matcher (tests and measurements: every form returns the same records)
// are honoured only by a process that had NHIP_TUNABLES=1 in its environment when the library first asked (looked up
// once, std::call_once).  Such a process reads them at every launch, so a test can change form between calls; any other
// process -- a shipped host -- never reads any of them: tunable() is a null pointer there and every policy is its default.
const char *tunable(const char *name);

// ---- ids that live in device memory ----
// The "_dev" entry points read scan ids, grid slots, block and pose indices from DEVICE arrays the host cannot look at
// without a round trip.  Every kernel checks such an id against the count its caller passed before it forms an address
// from it: an id outside [0, count) is treated as an empty scan / a pair that scores nothing / a row that is skipped, and
// is reported through the current device's status words, which nhip_dev_status() turns into NHIP_ERR_ARG after the
// stream has drained.  A stale id costs the caller an error code, never the process (an out-of-bounds read in a kernel
// is an HSA abort of the whole process; it happened once, in a test: DESIGN.md section 5, "Ids in device memory").
struct IdBounds {          // (plain data: it travels inside the kernels' parameter blocks)
  int32_t n_scans;         // scans behind d_offsets (n_scans + 1 entries)
  int32_t n_slots;         // grids behind d_grids
  uint32_t *status;        // the device's status words, or null (ids are still checked, nothing is reported)
};
constexpr uint32_t BAD_TARGET_ID = 1u, BAD_PAIR_SRC = 2u, BAD_PAIR_SLOT = 4u, BAD_BLOCK_ID = 8u, BAD_POSE_ID = 16u,
                   BAD_SCAN_ID = 32u, BAD_FEATURE_IDX = 64u, BAD_FEATURE_COUNT = 128u, BAD_SCAN_OFFSETS = 256u,
                   BAD_MEMBER_ID = 512u, BAD_SUBMAP_CAPACITY = 1024u, BAD_CONTRIB_ID = 2048u, BAD_BLOCK_COLUMN = 4096u,
                   BAD_SYSTEM_ID = 8192u, BAD_MAP_SCAN_OFFSETS = 16384u, BAD_FREESPACE_PAIR = 32768u, BAD_PLACE_ID = 65536u,
                   BAD_CONSISTENCY_DEGREE = 131072u, BAD_CONSISTENCY_MEMBER = 262144u, BAD_MAPWIN_CELLS = 524288u,
                   BAD_MAPWIN_POINTS = 1048576u, BAD_RANGESIG = 2097152u, BAD_REFINE_ID = 4194304u;
constexpr int DEV_STATUS_WORDS = 4;  // {OR of the kinds seen, kind / value / index of the first report}
uint32_t *dev_status();              // of the current device (allocated on the device's first use; null if that failed)
#ifdef __HIPCC__
__device__ __forceinline__ void flag_bad_id(uint32_t *status, uint32_t kind, int32_t value, int32_t index) {
  if (!status) return;
  if (atomicOr(status, kind) != 0u) return;  // (the first report keeps the details)
  status[1] = kind;
  status[2] = (uint32_t)value;
  status[3] = (uint32_t)index;
}
__device__ __forceinline__ bool id_in(int32_t id, int32_t n) { return (uint32_t)id < (uint32_t)n; }
// ---- the float norm of the distance gates ----
// Vector2f::norm() as Eigen evaluates it on baseline x86-64, and as the oracles restate it: two rounded products, one
// rounded add, a CORRECTLY ROUNDED root.  The correspondence search (nhip_corr.hip), the loop-closure pair gate
// (nhip_lc.hip) and the scan features (nhip_feat.hip) compare this value with a threshold and promise the reference's
// decision bit for bit, so the root must round as std::sqrt does: a root one ulp off flips the decision for the d2
// values next to the threshold (tests/threshold_edges.py designs them; tests/test_round_ops_gpu.py holds this helper to
// numpy's float32 chain over every binade).  float_norm_root takes the d2 a caller already holds.  sqrtf, not the
// intrinsic whose name promises round-to-nearest: on gfx950 that one compiles to the bare hardware root, which is off
// by one ulp for a share of its inputs (measured: DESIGN.md section 5, K5); sqrtf adds the correction step.
__device__ __forceinline__ float float_norm_root(float d2) { return sqrtf(d2); }
__device__ __forceinline__ float float_norm(float dx, float dy) {
  return float_norm_root(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
}
// a pair's source scan and grid slot; false: the pair scores nothing (and is reported)
__device__ __forceinline__ bool pair_ids_ok(const IdBounds &B, int32_t src, int32_t slot, int32_t pair, bool report) {
  const bool s_ok = id_in(src, B.n_scans), g_ok = id_in(slot, B.n_slots);
  if (s_ok && g_ok) return true;
  if (report) flag_bad_id(B.status, s_ok ? BAD_PAIR_SLOT : BAD_PAIR_SRC, s_ok ? slot : src, pair);
  return false;
}
#endif

// ---- grid layout (host) ----
constexpr int32_t GRID_MAX_SIDE = 16384;  // cells per axis make_layout admits (the table build sizes its tile bitmap by it: nhip_grid.h)
struct GridLayout {
  int32_t S, pad, pitch, R;
  int32_t cb;      // bytes per cell: 1 or 2
  int32_t levels;  // quantisation steps: 255 or 65535
  int64_t K;  // tap sum
  int64_t plain_bytes; // pitch * rows: a grid in plain row-major form (the downloads' form)
  bool has_image;      // false with NHIP_GRID_NO_IMAGE: no row-major image (and no skip map) in the slot
  int64_t grid_bytes;  // the stored image: plain_bytes, or 0 without one
  int64_t skip_bytes;  // skip_pitch(pitch) * rows rounded up to 16: the skip map that follows the image
  int64_t pool_bytes;  // pool_rows * pool_pitch: the max-pooled table (branch-and-bound bounds) after the skip map
  int64_t pool4_bytes; // pool4_rows * pool4_pitch: the stride-4 pooled table (second bound level) after the first
  int64_t hi_bytes;    // 16-bit cells: stored bytes of the plane of high bytes after the second pooled table (two tiled
                       // copies: hi_tiled() below); else 0
  int32_t hi_pitch;    // bytes per row of the plane in its plain (downloaded) form: the 8-bit pitch of the same grid
  int32_t hi_tpr;      // tiles per tile row of a copy
  int64_t hi_copy_bytes;  // bytes of one copy
  int64_t t16_bytes;   // 16-bit cells: after the two copies, the 16-bit image once more, tiled 8 rows x 8 cells (t16_tiled())
  int32_t t16_tpr;     // its tiles per tile row
  int64_t hits_bytes;  // after the matcher's planes: the HIT RASTER, one bit per cell (rows S + 2 * HIT_PAD, hits_pitch bytes each):
  int32_t hits_pitch;  // what the table was blurred from.  The exact-score pass (NHIP_SEARCH_EXACT_SCORE) recomputes the
                       // integer blur sums of the 1081 cells the winning pose reads from it, and their logarithms in double
  int64_t slot_bytes;  // the sum of the parts above: stride between grids
  // Byte offset of each part inside a slot, in the order above (make_layout pads pool4_bytes and hits_bytes so that the
  // tiled planes and every slot start on a 128-byte line); the image is at 0
  int64_t skip_offset;   // the skip map (= grid_bytes)
  int64_t pool_offset;   // the max-pooled table
  int64_t pool4_offset;  // the stride-4 pooled table
  int64_t hi_offset;     // the matcher's tiled planes (hi_bytes): first the two copies of the 8-bit plane
  int64_t t16_offset;    // the tiled copy of the 16-bit image inside them: hi_offset + 2 * hi_copy_bytes
  int64_t hits_offset;   // the hit raster
  int32_t pool_pitch, pool_rows;
  int32_t pool4_pitch, pool4_rows;
  double Lf, step;
};
// The plane of high bytes is stored in tiles of 8 rows x 16 bytes = one 128-byte cache line, so that the points of a
// chunk -- neighbours along a wall whatever its direction -- read their rows from a dozen lines instead of forty
// (in a row-major plane every row of every point is a line of its own).  A row read of the matcher is 8 or 12 bytes
// from a 4-byte-aligned column and must not cross a tile: there are TWO copies, the second with its tiles shifted by
// 8 columns, and a read takes the copy in which it starts in a tile's first half.
// Byte offset of (row, col) in copy cp (0 / 1):
constexpr uint32_t HI_TILE_BYTES = 128u;
__host__ __device__ __forceinline__ uint32_t hi_tiled(uint32_t row, uint32_t col, uint32_t cp, uint32_t tpr, uint32_t copy_bytes) {
  const uint32_t c = col + 8u * cp;
  return cp * copy_bytes + ((row >> 3) * tpr + (c >> 4)) * HI_TILE_BYTES + (row & 7u) * 16u + (c & 15u);
}

// The matcher's exact 16-bit pose sums read ONE cell per point: from a copy of the 16-bit image tiled 8 rows x 8 cells
// (128 bytes), for the same reason.  Byte offset of cell (row, col):
__host__ __device__ __forceinline__ uint32_t t16_tiled(uint32_t row, uint32_t col, uint32_t tpr) {
  return ((row >> 3) * tpr + (col >> 3)) * HI_TILE_BYTES + (row & 7u) * 16u + (col & 7u) * 2u;
}

// The hit raster's zero border, in cells, on every side: >= the largest blur radius (16), and a multiple of 32 so that the
// 64 x 64 tiles of the build start on dword boundaries of the bit rows.  Bit (row, col) of the raster is bit
// (col + HIT_PAD) & 31 of dword (col + HIT_PAD) >> 5 of bit row row + HIT_PAD.
constexpr int HIT_PAD = 32;

// Branch and bound works on 8 x 8 blocks of translations; a pooled entry covers the 15 x 15 stored cells an 8 x 8
// block can reach from any window origin with the same (row >> 3, col >> 3).
constexpr int BNB_B = 8;
constexpr int BNB_POOL = 2 * BNB_B - 1;
constexpr int BNB_MAX_NB = 11;  // blocks per axis the kernel's register layout holds: nx, ny <= 88
// Second level: the four 4 x 4 sub-blocks of a block, bounded from a table pooled over 7 x 7 cells at stride 4.
constexpr int BNB_B4 = 4;
constexpr int BNB_POOL4 = 2 * BNB_B4 - 1;
// Geometry the skip map shares with the correlation kernel: a wave of csm_correlate_kernel owns
// CSM_WAVE_ROWS plane rows and reads CSM_ROW_DW aligned dwords of each (nhip_csm_strip.h).
constexpr int CSM_WAVE_ROWS = 21;
constexpr int CSM_ROW_DW = 21;  // per cell byte: a 16-bit-cell strip spans 2 * CSM_ROW_DW dwords
#ifdef __HIPCC__
// floor(RN(v / res)) without the division on the common path.  m = RN(v * RN(1 / res)) differs
// from the correctly rounded quotient by less than |m| * 2^-51, so the two floors can differ only
// if m lies within that distance of an integer; those lanes (one point in ~10^12) take the division.
__device__ __forceinline__ double floor_quotient(double v, double res, double inv_res) {
  const double m = __dmul_rn(v, inv_res);
  double f = floor(m);
  const double frac = __dsub_rn(m, f);  // exact
  const double tol = __dmul_rn(fabs(m), 0x1p-50);
  if (frac <= tol || __dsub_rn(1.0, frac) <= tol) f = floor(__ddiv_rn(v, res));
  return f;
}
#endif

// grid-build workspace: 256-byte header, [16-bit cells: the 65536-entry quantiser threshold table,] then per
// target one occupancy byte per 64x64 tile, one 4-byte list slot per tile and GRID_WS_MASK_WORDS words of LINE MASKS per
// list slot: which 128-byte lines of the matcher's tiled planes the blur wrote inside the tile (the next rebuild clears
// those and no others -- two thirds of a listed tile's lines hold nothing)
constexpr int64_t GRID_WS_HEADER = 256;
constexpr int64_t GRID_WS_THR16 = 65536 * 4;
constexpr int GRID_WS_MASK_WORDS = 5;  // 32 lines of the first copy of the 8-bit plane, 40 of the shifted copy, 64 of the 16-bit copy
inline int64_t grid_ws_per_target(int32_t S) {
  const int64_t tiles = (S + 63) / 64;
  return (5 + 4 * GRID_WS_MASK_WORDS) * tiles * tiles;
}
// bytes per skip-map row: one bit per aligned dword column, whole 8-byte words
__host__ __device__ constexpr int32_t skip_pitch(int32_t pitch) { return ((pitch / 4 + 63) / 64) * 8; }
int make_layout(const nhip_grid_spec_t *spec, GridLayout *L);

// Device-side constant tables of one grid spec (taps + quantiser thresholds), cached.
struct GridTables {
  int32_t taps[129];
  uint32_t thr[256];               // 8-bit cells
  const uint32_t *thr16 = nullptr;  // 16-bit cells: 65536 entries, owned by a process-wide cache
};
int make_tables(const nhip_grid_spec_t *spec, const GridLayout &L, GridTables *T);

// ---- in-stream timing ----
void timer_begin(int id, hipStream_t s);
void timer_end(int id, hipStream_t s);

// ---- kernel launchers (defined in the .hip files) ----
// the table build (nhip_grid.hip; its kernels: nhip_grid_blur.hip, nhip_grid_tables.hip, nhip_grid_clear.hip)
int launch_grid_build(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids,
                      int32_t n_targets, const nhip_grid_spec_t *spec, const GridLayout &L,
                      uint8_t *d_grids, void *d_ws, int64_t ws_bytes, hipStream_t s, bool incremental = false);

// Which kernel matches a list: decided by csm_plan (nhip_csm_plan.hip) and nowhere else; launch_csm_match dispatches on it.
// For MATCH_BNB, the form of the branch-and-bound run is decided by bnb_plan (nhip_bnb_host.hip) and nowhere else.
enum MatchForm : int32_t {
  MATCH_BNB,       // the branch-and-bound matcher (nhip_bnb.hip)
  MATCH_POSES,     // every add in the kernel whose lanes are poses (nhip_csm_small.hip): one plane, or tiles of rows
  MATCH_STRIPS8,   // every add in the strip kernels, 8-bit cells (nhip_csm.hip)
  MATCH_STRIPS16,  // every add in the strip kernels, 16-bit cells (nhip_csm16.hip): the one form that reads skip maps
};
struct MatchPlan {
  MatchForm form = MATCH_BNB;
  int32_t tile_rows = 0, n_tiles = 0;  // MATCH_POSES: rows of the plane per workgroup, workgroups per rotation
  // Set only by the chained GetTransformation, for its levels through the kernel whose lanes are poses: the kernel before
  // zeroed the keys (no memset), the kernel after decodes them (no finalize) -- dropin_bridge_kernel for the coarse level,
  // csm_exact_score_kernel for the fine one.
  bool keys_zeroed = false, keys_undecoded = false;
};
// the plan of a search of n_pairs pairs on these grids (the test hooks NHIP_CSM_EXHAUSTIVE / NHIP_CSM_SMALL are read here)
MatchPlan csm_plan(const GridLayout &L, const nhip_search_t *search, int32_t n_pairs);

// A branch-and-bound run's form and policies, decided by bnb_plan (nhip_bnb_host.hip; only it reads the NHIP_BNB_* hooks).
// Forms (ids as nhip_csm_last_launch reports them): one kernel per pair (+ the hand-over kernel when `second`), the split
// form in one round, in several rounds on the caller's stream, in rounds with the candidates on the helper stream.
enum BnbForm : int32_t { BNB_FUSED, BNB_SPLIT_ONE, BNB_SPLIT_ROUNDS, BNB_SPLIT_OVERLAP };
struct BnbPlan {
  BnbForm form;
  int32_t n_pairs, cb, levels;
  bool second, general_all, short_scans, pool_lds, instrumented, stats, timeline;
  bool l2_runs;      // strip bounds over runs of level-2 entries in the kernels that keep that list (NHIP_BNB_L2_RUNS=0: per cell)
  bool pair_subs;    // two live side-by-side sub-blocks of a strip in one pass of exact sums (NHIP_BNB_PAIR_SUBS=0: one pass each)
  bool zero_chunks;  // exact sums skip the cell-list chunks whose level-2 bytes are all zero (NHIP_BNB_ZERO_CHUNKS=0: every chunk)
  bool seed_bounds;  // seed passes take their sub-block bounds whatever the pair's best sum (NHIP_BNB_SEED_BOUNDS=1; default: only once it is not 0)
  bool sized_split;  // the size rule (bnb_workspace_bytes) gives this list room for the split form
  uint32_t rot_cap, heavy_min, keep_ranks, split_min, split_max;  // split_max 0: by the round's length
  int64_t batch, slots, slot_bytes, rounds;  // pairs per round (0: fused), rounds' state the workspace holds, bytes of one
  int64_t lds_first;  // bytes of the main kernel's first LDS region (bnb::lds_bytes gives a launch's total from it)
};
BnbPlan bnb_plan(const GridLayout &L, const nhip_search_t *search, int32_t n_pairs, int64_t workspace_bytes);

// One search of a list of pairs, as every launcher of the matcher takes it (the entry points of the C ABI fill one, by
// field name).  The plan is not part of it: the caller decides it, and the chained GetTransformation edits it per level.
struct MatchJob {
  const float *xy = nullptr;         // the points of all scans, (x, y) each
  const int32_t *offsets = nullptr;  // index of each scan's first point (ids.n_scans + 1 entries)
  IdBounds ids = {0, 0, nullptr};
  const uint8_t *grids = nullptr;
  const nhip_grid_spec_t *spec = nullptr;
  const GridLayout *L = nullptr;
  // per pair: source scan, grid slot, (cos, sin) theta0, optional (x, y) cell offset of the search centre, optional entry
  // of delta_cs that is the pair's rotation 0 (the branch-and-bound matcher's: BnbParams::pair_kbase)
  const int32_t *pair_src = nullptr, *pair_slot = nullptr;
  const double *rot0_cs = nullptr;
  const double *delta_cs = nullptr;  // (cos, sin) of the search's rotations
  const int32_t *pair_origin = nullptr, *pair_kbase = nullptr;
  int32_t n_pairs = 0;
  const nhip_search_t *search = nullptr;
  double min_score = -INFINITY;  // the score gate (-INFINITY: off)
  uint64_t *keys = nullptr;
  nhip_match_t *out = nullptr;
  int32_t *sums = nullptr;  // may be null
  hipStream_t stream = nullptr;
  void *workspace = nullptr;  // the branch-and-bound matcher's (bnb_workspace_bytes)
  int64_t workspace_bytes = 0;
};

int launch_csm_match(const MatchJob &job, const MatchPlan &plan);

// branch-and-bound matcher (nhip_bnb.hip); the lattice is one bnb_fits takes (csm_plan chose it)
int launch_csm_bnb(const MatchJob &job);
int64_t bnb_workspace_bytes(int32_t n_pairs);
int64_t bnb_workspace_bytes_lists(int32_t n_pairs);
void bnb_last_launch(int32_t out[8]);
bool bnb_fits(const GridLayout &L, const nhip_search_t *search);
int bnb_stats_read(unsigned long long out[24]);
int bnb_stats_chunks_read(unsigned long long out[4]);
int bnb_stats_seeds_read(unsigned long long out[8]);
int bnb_timeline_read(unsigned long long *out, int32_t n);
int bnb_timeline_cand_read(unsigned long long *out, int32_t n);
int bnb_stats_per_pair(unsigned long long *out, int32_t n);
// decodes the keys into records and sums and applies the score gate (min_score -INFINITY: off); with NHIP_SEARCH_EXACT_SCORE
// in search->flags only the floor on the sums, the exact-score pass gates the scores
void launch_csm_finalize(const MatchJob &job);

// the score volume of ONE pair (scan src against grid slot, search centre (origin_x, origin_y)) from the strip kernels;
// of the job it reads the scans, the grids, rot0_cs (one entry), delta_cs, the search and the stream
int launch_csm_scores(const MatchJob &job, int32_t src, int32_t slot, int32_t origin_x, int32_t origin_y, int32_t *d_volume);

// NHIP_SEARCH_EXACT_SCORE: replaces the records' scores by the winners' scores on the unquantised table and gates them
// (nhip_csm_score.hip); called by launch_csm_match
int launch_csm_exact_score(const MatchJob &job, const MatchPlan &plan);
// every add for lattices of few translations (nx * ny <= 256), both cell widths (nhip_csm_small.hip); tiling from the plan
bool csm_small_plane_fits(const nhip_search_t *search);
bool csm_small_tiled_fits(const nhip_search_t *search, int32_t n_pairs, int32_t *tile_rows, int32_t *n_tiles);
int launch_csm_small_match(const MatchJob &job, const MatchPlan &plan);
// skip maps of n finished 16-bit grids (the handle API's late build; occupancy unknown: every map tile is computed)
int launch_skipmap_build(uint8_t *d_grids, int32_t n_grids, const GridLayout &L, hipStream_t s);

int launch_resid_lidar(int kind, const float *d_corr, const int32_t *d_corr_block, int64_t n_corr,
                       const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                       const double *d_poses, int32_t n_poses, double *d_block_consts,
                       double *d_res, double *d_jsrc, double *d_jtgt, hipStream_t s, double *d_jtgt_theta = nullptr,
                       int32_t block_base = 0, double *d_q = nullptr);

int launch_resid_normal_eq(int kind, const float *d_corr, const int32_t *d_block_offsets,
                           const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                           const double *d_poses, int32_t n_poses, double *d_block_consts, double *d_out,
                           hipStream_t s);

int launch_corr_search(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                       const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                       const float *d_pose_aff, float thr, float min_cos, bool gate, const int64_t *d_cap_offsets,
                       float *d_corr_padded, int32_t *d_counts, hipStream_t s);

int launch_corr_compact(const float *d_corr_padded, const int64_t *d_cap_offsets,
                        const int32_t *d_counts, int32_t n_blocks, int32_t *d_block_offsets,
                        float *d_corr, int32_t *d_corr_block, hipStream_t s);

int launch_lc_scatter_scores(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, double *d_scores, hipStream_t s);
int launch_lc_chi_square(const double *d_poses, int32_t n_poses, const int32_t *d_src, const int32_t *d_tgt, const float *d_cov,
                         int32_t n, double max_score, double *d_scores, uint8_t *d_flags, hipStream_t s);
int launch_lc_pair_gate(const double *d_poses, int32_t n_poses, const int32_t *d_cand, int32_t n, double max_range,
                        int32_t min_sep, uint8_t *d_flags, hipStream_t s);

// the float norm of the distance gates on n inputs (nhip_lc.hip; the instrument nhip_round_norm_dev)
int launch_round_norm(const float *d_dx, const float *d_dy, int64_t n, int32_t root_only, float *d_out, hipStream_t s);

// scan features (nhip_feat.hip); the spec has passed feature_spec_check (nhip_host_features.hip)
int launch_feat_extract(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_feature_spec_t &spec,
                        int32_t *d_planar_idx, int32_t *d_planar_count, int32_t *d_edge_idx, int32_t *d_edge_count,
                        double *d_scores, hipStream_t s);
int launch_feat_pack(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_idx,
                     const int32_t *d_count, int32_t cap, float *d_xy_out, float *d_normals_out, int32_t *d_offsets_out,
                     hipStream_t s);

// submap clouds (nhip_submap.hip): the offsets kernel, then the gather; stores nothing past out_capacity points
int launch_submap_gather(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_member_scan,
                         const float *d_member_affine, const int32_t *d_member_offsets, int32_t n_targets, float *d_out_xy,
                         int64_t out_capacity, int32_t *d_out_offsets, hipStream_t s);

// scan normals (nhip_normals.hip); the spec has passed normals_spec_check (nhip_host_normals.hip), which also gives the
// sample limit's second term
int launch_normals_estimate(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_normals_spec_t &spec,
                            int32_t sample_limit, float *d_normals, int32_t *d_info, hipStream_t s);

// map vectorisation (nhip_vectorize.hip, K13); the spec has passed vectorize_spec_check (nhip_host_vectorize.hip)
struct VecState {     // the first bytes of the workspace: what the round kernels keep between launches
  int32_t stats[8];   // {M, segments, rounds, flag, cells emitted, cells retired, n_rho, 0}: the caller's stats, as they grow
  int32_t end;        // set once the call has ended: every kernel of a round returns at once; the ONE word the host reads between batches
  int32_t peak_t, peak_b, peak_votes;
  int32_t action;     // of the round's runs kernel: VEC_RETIRE / VEC_COMMIT
  int32_t n_band;     // entries of the band list
};
enum { VEC_RETIRE = 1, VEC_COMMIT = 2 };
struct VecLayout {    // byte offsets inside the workspace (256-byte aligned); the first four planes are the caller's to read
  int64_t state, counts, cells, votes, live, row_off, tables, partial, bits, run_of_bin, run_lo, run_hi, run_slot, band_list, bytes;
  int32_t n_rho, n_along, bit_words, max_runs;
};
void vec_layout(const nhip_vectorize_spec_t &spec, int32_t max_cells, VecLayout *L);
struct VecParams {    // plain data: travels in the kernels' parameter blocks
  int32_t width, height, cell_x0, cell_y0, n_theta, n_rho, n_along, min_hits, min_votes, band_q, gap1, min_length, max_segments,
      max_cells, max_rounds, n_scans;
  double res, inv_res;
  VecState *st;
  int32_t *counts, *cells, *votes, *row_off, *run_of_bin, *run_lo, *run_hi, *run_slot, *band_list;
  const int32_t *C, *S;
  uint8_t *live;
  unsigned long long *partial;
  uint32_t *bits;
  long long *records;
  uint32_t *status;
};
// clears the state and the counts, then raster, cell list and the votes of every cell
int launch_vec_front(const VecParams &P, const float *d_xy, const int32_t *d_offsets, const float *d_affines, hipStream_t s);
// enqueues `n` rounds; each returns at once when the call has ended
int launch_vec_rounds(const VecParams &P, int32_t n, hipStream_t s);

// occupancy grid (nhip_occupancy.hip, K14); the spec has passed occupancy_spec_check (nhip_host_occupancy.hip)
struct OccParams {    // plain data: travels in the kernels' parameter blocks
  int32_t width, height, cell_x0, cell_y0, max_ray_cells, min_obs, occ_permille, free_permille, n_scans;
  double res, inv_res;
  int32_t *hits, *misses;
  int8_t *grid;
  long long *stats;   // 8 words: {scans traced, scans dropped, beams traced, beams long, points dropped, occupied, free, unknown}
  uint32_t *status;
};
// clears the stats (and, with `clear`, both planes), then the trace of every scan and the classification of the window
int launch_occupancy(const OccParams &P, bool clear, const float *d_xy, const int32_t *d_offsets, const float *d_affines,
                     hipStream_t s);

// transient returns (nhip_transient.hip, K19); the spec has passed transient_spec_check (nhip_host_transient.hip)
struct TransientParams {  // plain data: travels in the kernels' parameter blocks
  int32_t width, height, cell_x0, cell_y0, support_radius, min_through, transient_permille, n_scans, n_points;
  double res, inv_res;
  const int32_t *hits, *misses;  // read as they are, never written
  uint8_t *labels;               // n_points
  float2 *out_xy;                // n_points
  int32_t *out_offsets;          // n_scans + 1
  int32_t *out_index;            // n_points
  long long *stats;   // 8 words: {points static, transient, unobserved, invalid, scans processed, scans whose offsets are not
                      // a scan, scans that had points and kept none, 0}
  uint32_t *status;
};
// clears the stats and sets every label to 3, then classify, offsets and pack
int launch_transient(const TransientParams &P, const float *d_xy, const int32_t *d_offsets, const float *d_affines, hipStream_t s);

// map windows (nhip_mapwin.hip, K20); the spec has passed mapwin_spec_check (nhip_host_mapwin.hip)
struct MapwinParams {  // plain data: travels in the kernels' parameter blocks
  int32_t width, height, cell_x0, cell_y0, side, occ_min;
  double res;
  long long *stats;   // 8 words: {occupied cells, queries, points stored, empty windows, largest window, cells overflow, points
                      // overflow, 0}: the cells call writes words 0 and 5 and clears the rest, the gather writes 1 - 4 and 6
  uint32_t *status;
};
// row count, scan (with the capacity decision) and row pack: row_ptr[height + 1], cols[<= max_cells]
int launch_mapwin_cells(const MapwinParams &P, const int8_t *d_grid, int32_t max_cells, int32_t *d_row_ptr, int32_t *d_cols,
                        hipStream_t s);
// window count into d_counts (n_queries int32 of the workspace), scan (with the capacity decision) and window pack
int launch_mapwin_gather(const MapwinParams &P, const int32_t *d_row_ptr, const int32_t *d_cols, const int32_t *d_origins,
                         int32_t n_queries, float *d_out_xy, int64_t out_capacity, int32_t *d_out_offsets, int32_t *d_counts,
                         hipStream_t s);

// range signatures (nhip_rangesig.hip, K21); the spec has passed rangesig_spec_check (nhip_host_rangesig.hip)
constexpr int32_t RANGESIG_MAX_ANCHORS = 1 << 20;
constexpr int32_t RANGESIG_MAX_NODES_PER_AXIS = 16384;  // lattice rows: the anchors' row counts take 64 KB of the workspace
constexpr int RANGESIG_QT = 8;                          // query rows a workgroup of the cost kernel takes with one load of its anchors
struct RangesigParams {  // plain data: travels in the kernels' parameter blocks
  int32_t width, height, occ_min, free_max, stride, rays_per_sector, top_k, min_sep, min_sectors, flags;
  long long *stats;   // 8 words: {lattice nodes, anchors, anchors that did not fit, rays ended on a wall, in unknown, outside or at n,
                      // queries without a record, records}: the anchors call writes 0 - 2 and clears the rest, the map call 3 - 5,
                      // the match 6 and 7
  uint32_t *status;
};
struct RangesigScanTables {  // plain data: travels in the scan kernel's parameter block (nhip_rangesig_tables / nhip_place_tables fill the same values)
  float edge2[256];   // [0] = 0, [1..254] the squared edges, [255] unused
  float dir[64];      // 32 x {cos, sin}
};
// fill with -1, row count, scan (with the capacity decision and the stats) and row pack; d_row_counts: the workspace, nj + 1 int32
int launch_rangesig_anchors(const RangesigParams &P, const int8_t *d_grid, int32_t max_anchors, int32_t *d_anchors,
                            int32_t *d_row_counts, hipStream_t s);
int launch_rangesig_map(const RangesigParams &P, const int8_t *d_grid, const int32_t *d_rays, const int32_t *d_anchors,
                        int32_t n_anchors, uint8_t *d_sig, hipStream_t s);
int launch_rangesig_scans(const RangesigScanTables &T, const float *d_xy, const int32_t *d_offsets, int32_t n_scans, uint8_t *d_sig,
                          hipStream_t s);
// clears stats 6 and 7, then cost and selection kernels per chunk of `chunk_rows` query rows (d_keys holds that many rows of `pitch`)
int launch_rangesig_match(const RangesigParams &P, const uint8_t *d_qsig, int32_t n_queries, const uint8_t *d_asig,
                          const int32_t *d_anchors, int32_t n_anchors, int32_t *d_records, uint32_t *d_keys, int32_t pitch,
                          int32_t chunk_rows, hipStream_t s);

// free-space check of match records (nhip_freespace.hip, K15); the specs have passed the checks of nhip_host_freespace.hip
struct FsParams {     // plain data: travels in the kernels' parameter blocks (the trace reads the first group, the check both)
  const float2 *xy;
  const int32_t *offsets;
  const uint8_t *grids;      // the slots: a slot's hit raster is at hits_offset
  uint8_t *free_planes;      // hits_bytes per slot, the raster's layout
  int32_t S, hits_pitch;
  int64_t slot_bytes, hits_offset, hits_bytes;
  double res, inv_res;
  IdBounds ids;
  const int32_t *target_ids;  // trace: the scan behind each slot
  int32_t n_targets;
  const int32_t *pair_src, *pair_slot, *pair_origin;  // check: as the matcher's (pair_origin may be null)
  const double *rot0_cs, *delta_cs;
  const nhip_match_t *matches;
  int32_t *counts;            // 8 per pair
  int32_t n_pairs, pairs_per_xcd, n_theta, nx, ny, hx, hy, hit_radius, end_margin;
};
int launch_fs_trace(const FsParams &P, hipStream_t s);
int launch_fs_check(const FsParams &P, hipStream_t s);

// match refinement (nhip_refine.hip, K22); the spec has passed refine_spec_check (nhip_host_refine.hip)
struct RefineParams {  // plain data: travels in the kernel's parameter block
  const float2 *xy, *normals;
  const int32_t *offsets, *pair_src, *pair_tgt;
  const double *pose0;   // 4 per pair
  nhip_refined_t *out;
  double *trace;         // NHIP_REFINE_TRACE_DOUBLES per pair, or null
  int32_t n_scans, n_pairs;
  uint32_t *status;
  nhip_refine_spec_t spec;
};
int launch_refine_icp(const RefineParams &P, hipStream_t s);

// place descriptors (nhip_place.hip, K16); the spec has passed place_spec_check (nhip_host_place.hip)
constexpr int PLACE_MAX_RINGS = 32;        // of a descriptor
constexpr int PLACE_MATCH_MAX_RINGS = 15;  // of a match: dist <= 64 R must stay below 1023 for the 16-bit key
constexpr int PLACE_QT = 16;               // query rows a workgroup of the distance kernel takes with one load of its candidates
struct PlaceTables {  // plain data: travels in the describe kernel's parameter block (nhip_place_tables fills the same values)
  int32_t n_rings;
  float edge2[PLACE_MAX_RINGS + 1];
  float dir[64];      // 32 x {cos, sin}
};
struct PlaceMatch {   // plain data: travels in the kernels' parameter blocks
  const unsigned long long *desc;  // n_scans x n_rings
  const int32_t *bits;             // n_scans
  const int32_t *ids;              // n_ids, ascending
  uint16_t *keys;                  // the workspace: chunk rows x pitch
  int32_t *records;                // n_ids x top_k x 4
  long long *stats;                // 8 words
  uint32_t *status;
  int32_t n_scans, n_ids, pitch, n_rings, top_k, min_separation, max_permille, flags;
};
int launch_place_describe(const PlaceTables &T, const float *d_xy, const int32_t *d_offsets, int32_t n_scans, uint64_t *d_desc,
                          int32_t *d_bits, hipStream_t s);
// clears the stats, then distance and top-K kernels per chunk of `chunk_rows` query rows (the workspace holds that many)
int launch_place_match(const PlaceMatch &P, int32_t chunk_rows, hipStream_t s);

// place sequences (nhip_place_seq.hip, K16b); the specs have passed place_seq_spec_check (nhip_host_place.hip)
struct PlaceSeq {     // plain data: travels in the kernels' parameter blocks
  const unsigned long long *desc;  // n_scans x n_rings
  const int32_t *bits;             // n_scans
  const int32_t *ids;              // n_ids, ascending
  uint16_t *plane;                 // the workspace's first part: single distances by scan id, (chunk scans + halo) x pitch_s
  uint16_t *keys;                  // its second part: seq per (query scan of the chunk, candidate entry), chunk scans x pitch
  int32_t *records;                // n_ids x top_k x 8
  long long *stats;                // 8 words
  uint32_t *status;
  int32_t n_scans, n_ids, pitch_s, pitch, n_rings, top_k, min_separation, max_permille, flags, half_window, step;
};
// clears the stats, then plane, window and top-K kernels per chunk of `chunk_scans` >= 1 query scans (the workspace holds
// that many rows of keys and that many plus 2 half_window step rows of the plane, or all scans' rows of both)
int launch_place_seq_match(const PlaceSeq &P, int32_t chunk_scans, hipStream_t s);

// loop-closure consistency (nhip_consistency.hip, K17); the spec has passed consistency_spec_check (nhip_host_consistency.hip)
constexpr int32_t CONSISTENCY_MAX_RECORDS = 65536;  // W = ceil(M / 64) <= 1024 words: the live set fits the score kernel's LDS
struct ConsistencyState {  // the first bytes of the workspace: what the step kernels keep between launches
  unsigned long long key;  // the step's best (score << 32 | ~u), by 64-bit atomicMax; 0 between steps
  int32_t steps;           // members appended so far
  int32_t done;            // set once the set has ended: every kernel returns at once; the ONE word the host reads between batches
};
struct ConsistencyTol {    // the spec's tolerances: plain data in the adjacency kernel's parameter block
  double t0, t_rate, t_max, r0, r_rate, r_max;
};
struct ConsistencySet {    // plain data: travels in the set kernels' parameter blocks
  const unsigned long long *adj;  // M rows of W words
  const int32_t *deg;             // M
  unsigned long long *C;          // W words of the workspace: the live set
  ConsistencyState *st;
  int32_t *members, *n_members;
  long long *stats;               // 8 words
  uint32_t *status;
  int32_t M, W, max_steps;        // (max_steps: already min(spec.max_steps, M))
};
// clears the degrees, then the whole matrix and the degrees, then stats = {M, edges, largest degree, 0 ...}
int launch_consistency_adjacency(const double *d_records, int32_t M, const ConsistencyTol &T, unsigned long long *d_adj, int32_t *d_deg,
                                 long long *d_stats, hipStream_t s);
// the members cleared to -1, the live set to all M records, the stats' first three words from the degrees
int launch_consistency_begin(const ConsistencySet &P, hipStream_t s);
// enqueues `n` steps (score + commit); each returns at once when the set has ended
int launch_consistency_steps(const ConsistencySet &P, int32_t n, hipStream_t s);

int launch_resid_point_to_line(const float *d_segments, const float *d_points,
                               const int32_t *d_point_block, int64_t n_points,
                               const int32_t *d_block_pose, const int32_t *d_block_line,
                               int32_t n_blocks, const double *d_poses, int32_t n_poses, const double *d_line_poses,
                               int32_t n_line_poses, double *d_res, double *d_jpose, double *d_jline, hipStream_t s);

// point-to-line blocks reduced to their normal equations (nhip_resid.hip): 28 doubles per block, blocks contiguous in d_points
int launch_resid_point_to_line_normal_eq(const float *d_segments, const float *d_points, const int32_t *d_block_offsets,
                                         const int32_t *d_block_pose, const int32_t *d_block_line, int32_t n_blocks,
                                         const double *d_poses, int32_t n_poses, const double *d_line_poses, int32_t n_line_poses,
                                         double *d_out, hipStream_t s);

// HITL point selection (nhip_hitl.hip); the spec has passed hitl_spec_check (nhip_host_solver.hip)
int launch_hitl_select(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const float *d_pose_f32,
                       const nhip_hitl_spec_t &spec, uint8_t *d_class, int32_t *d_counts, int32_t *d_scan_block,
                       int32_t *d_scan_offset, int32_t *d_totals, hipStream_t s);
int launch_hitl_pack(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_class, const int32_t *d_counts,
                     const int32_t *d_scan_block, const int32_t *d_scan_offset, const int32_t *d_totals, int32_t n_blocks,
                     int32_t n_points, float *d_points, int32_t *d_block_offsets, int32_t *d_block_pose, hipStream_t s);

int launch_resid_odometry(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                          const int32_t *d_pose_j, int32_t n_factors, double tw, double rw,
                          const double *d_poses, int32_t n_poses, double *d_res, double *d_ji, double *d_jj,
                          hipStream_t s);

// odometry factors reduced to their normal equations (nhip_resid.hip): 28 doubles per factor over [pose_i | pose_j]
int launch_resid_odometry_normal_eq(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                                    const int32_t *d_pose_j, int32_t n_factors, double tw, double rw,
                                    const double *d_poses, int32_t n_poses, double *d_out, hipStream_t s);

// the same under a robust loss (nhip_loss.hip): rows of the reweighted factors with rho(s) in slot 27, and unless d_weights
// is null {s, rho, rho', sqrt(rho')} per factor; the spec has passed loss_spec_check (nhip_layout.hip), which needs no HIP
int loss_spec_check(const nhip_loss_spec_t *loss, const char *who);
int launch_resid_odometry_robust_normal_eq(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                                           const int32_t *d_pose_j, int32_t n_factors, double tw, double rw, int32_t kind,
                                           double scale, const double *d_poses, int32_t n_poses, double *d_out,
                                           double *d_weights, hipStream_t s);

// relative-pose factors (nhip_relpose.hip, K23): r, J_i, J_j and -- unless null -- the 8 parts and the flags per factor; and
// their rows under a loss.  The arguments have passed relpose_args_check (nhip_layout.hip), which needs no HIP
int relpose_args_check(const void *z, const void *info, const void *pose_i, const void *pose_j, int32_t n_factors,
                       const void *poses, int32_t n_poses, const void *out, const char *who);
int launch_resid_relpose(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                         int32_t n_factors, const double *d_poses, int32_t n_poses, double *d_residuals, double *d_jac_i,
                         double *d_jac_j, double *d_parts, int32_t *d_flags, hipStream_t s);
int launch_resid_relpose_normal_eq(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                                   int32_t n_factors, int32_t kind, double scale, const double *d_poses, int32_t n_poses,
                                   double *d_out, double *d_weights, int32_t *d_flags, hipStream_t s);

// the block-sparse linear system of the pose graph (nhip_linsolve.hip, K11): assembly from 28-double rows, and the
// block-Jacobi preconditioned CG; the arguments have passed the checks of nhip_host_linsolve.hip
struct PcgStats {  // what the PCG kernels keep in the workspace's first bytes; the host reads it between batches and at the end
  int32_t done_a, done_b;  // set by the direction kernel / the update kernel once the solve has ended
  int32_t iterations, flag;
  double relres, bb;
};
int launch_bsr_assemble(const double *d_rows, int32_t n_rows, const int32_t *d_row_ptr, const int32_t *d_col,
                        const int32_t *d_contrib_ptr, const int32_t *d_contrib, int32_t nb, int32_t nnzb, int32_t n_contrib,
                        double *d_values, double *d_grad, double *d_cost, hipStream_t s);
int64_t bsr_pcg_workspace_bytes(int32_t nb, int32_t nnzb);
// enqueues the start of a solve (kernels of iteration `first` .. `last` - 1; first == 0: the set-up in front of them;
// final: the closing check behind them).  The state in the workspace's first bytes is a PcgStats.
int launch_bsr_pcg(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const double *d_grad,
                   const uint8_t *d_fixed, int32_t nb, int32_t nnzb, double lambda, double diag_floor, double tol,
                   int32_t first, int32_t last, bool final, double *d_x, void *d_ws, hipStream_t s);
// columns of the inverse: S systems (H + ridge I) x = e_j on one matrix, each with a block of its own held constant
// (nhip_linsolve_columns.hip, K12); launch_bsr_pcg_columns enqueues like launch_bsr_pcg; bsr_pcg_columns_read waits for the
// stream and brings down the number of systems still running and, where `iters` is given, every system's end words
int64_t bsr_pcg_columns_workspace_bytes(int32_t nb, int32_t nnzb, int32_t n_systems);
int launch_bsr_pcg_columns(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const uint8_t *d_fixed,
                           int32_t nb, int32_t nnzb, const int32_t *d_gauge, const int32_t *d_rhs_index, int32_t n_systems,
                           double ridge, double tol, int32_t first, int32_t last, bool final, double *d_x, void *d_ws,
                           hipStream_t s);
int bsr_pcg_columns_read(const void *d_ws, int32_t nb, int32_t n_systems, int32_t *n_active, int32_t *iters, int32_t *flag,
                         double *relres, hipStream_t s);

}  // namespace nhip
