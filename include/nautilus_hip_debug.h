/*
 * nautilus_hip_debug.h -- the INSTRUMENTS of libnautilus_hip: what its tests, its benchmark and its measuring tools read
 * back from a run.  Same library, same conventions as nautilus_hip.h (included below); nothing a nautilus host needs to
 * call is declared here, and nothing here changes what the calls of nautilus_hip.h compute.
 */
#ifndef NAUTILUS_HIP_DEBUG_H_
#define NAUTILUS_HIP_DEBUG_H_

#include "nautilus_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ where the host's time went */
/* Wall-clock seconds of the calling thread's last handle-API call (nhip_scans_upload, nhip_grids_build, nhip_csm_match and
 * the _free calls), by what the host waited for: out[0] hipMalloc, [1] zero-fill + host-to-device copies, [2] from the first
 * kernel launch to the end of the call (nhip_grids_build: the launches alone), [3] waiting for the kernels, [4] device-to-host
 * copies, [5] hipFree, [6] the whole call (nhip_csm_match), [7] unused.  Diagnostic: bench.py prints it per run of its
 * host-buffer leg, so that a slow call says where it was slow. */
int nhip_host_phases(double out[8]);

/* ------------------------------------------------------------------ what the matcher did */
/* The form the calling thread's last branch-and-bound match took (diagnostic; every form returns the same records):
 * out[0] = 0 one kernel per pair from start to end (+ the hand-over kernel when out[5]), 1 split form in one round,
 * 2 split form in several rounds on the caller's stream, 3 split form in rounds with the candidates on the library's
 * helper stream of the current device; out[1] pairs per round; out[2] rounds' state the workspace holds; out[3] rounds;
 * out[4] 1 when NHIP_SEARCH_SHORT_SCANS was honoured; out[5] hand-over kernel launched; out[6] bit 0: instrumented build,
 * bit 1: the kernels that keep a list of level-2 runs take their strip bounds from it (clear: NHIP_BNB_L2_RUNS=0),
 * bit 2: the candidates' kernels take two live sub-blocks side by side in one pass (clear: NHIP_BNB_PAIR_SUBS=0),
 * bit 3: their exact sums leave out the chunks of the cell list whose windows hold only empty cells (clear:
 * NHIP_BNB_ZERO_CHUNKS=0; what that saves is counted by nhip_bnb_stats_chunks, declared at the end of nautilus_hip.h),
 * bit 4: a seed takes its block's sub-block bounds even while the pair's best sum is 0 (set: NHIP_BNB_SEED_BOUNDS=1; clear,
 * the default: such a seed evaluates its block without them; nhip_bnb_stats_seeds, also at the end of nautilus_hip.h);
 * out[7] n_pairs. */
int nhip_csm_last_launch(int32_t out[8]);
/* What the calling thread's last nhip_csm_get_transformation did: {the coarse optimum's score, the form the fine level ran in
 * (0: the branch-and-bound matcher, 1: every add by the strip kernels -- a fine plane too large for the tiles of rows, 2: every
 * add by the kernel whose lanes are poses -- the default), 1 if the two levels were chained on the device (a cached target),
 * the coarse optimum's rotation index}.  (Measurement / tests.) */
int nhip_csm_get_transformation_info(double out[4]);

/* With NHIP_BNB_STATS=1 in the environment the branch-and-bound matcher counts its work: blocks of 8 x 8
 * translations whose sums it evaluated exactly (four 4 x 4 sub-blocks count as one block), and blocks in all, since
 * the last call (synchronises; resets). */
int nhip_bnb_stats(uint64_t *evaluated, uint64_t *total);
/* ... by level: out[0..3] = {blocks evaluated whole, blocks in all, candidate blocks refined through their four
 * sub-block bounds, 4 x 4 sub-blocks evaluated exactly}; out[4..10] = shader-clock sums of the matcher's kernel:
 * wave time in the candidate phase, of which window origins / sub-block bounds / exact sums, the slowest wave of
 * each pair, seed phase and bound phase (per workgroup); out[11..13] further clocks, out[14] = poses of 16-bit grids whose exact
 * sums were read from the 16-bit image (the rest was settled on the plane of high bytes); out[15] = pairs a score gate
 * settled right after their bounds (nhip_csm_match_gated); out[16..18] = rotation passes of the kernels that keep a list
 * of level-2 runs (the split form's candidates, the hand-over kernel; not the seeds) that took their strip bounds from
 * it, that took them per stored cell because some group of 8 lanes would have held more than 257 points, and that did
 * because the rotation had more runs than the list holds -- all three stay 0 under NHIP_BNB_L2_RUNS=0; out[19..21]
 * = the work at the lattice's edge, in blocks with fewer than 8 pose columns or rows (a lattice side that is no multiple
 * of 8 has one such block column or row): such blocks refined through their sub-block bounds, 4 x 4 sub-blocks evaluated
 * that hold no pose of the lattice, such blocks evaluated whole -- the matcher skips the former, so out[20] stays 0,
 * and only an edge block with more than 4 pose columns and rows, which has a pose in all four sub-blocks, can be the
 * latter: out[21] stays 0 on a lattice whose sides are 8 m + 0 .. 4 (the seed of a scan too long for the by-rotation
 * form is a whole block wherever it lies, and is not counted); out[22] = passes of exact sums that took TWO 4 x 4
 * sub-blocks side by side on a strip's sub-block row at once (the split form's candidates and the hand-over kernel; each
 * adds 2 to out[3], which keeps its meaning), out[23] = those of them whose window reaches across a block boundary -- both
 * stay 0 under NHIP_BNB_PAIR_SUBS=0 and in the kernel that works a pair from start to end (synchronises; resets) */
int nhip_bnb_stats_levels(uint64_t out[24]);
/* ... and per pair of the last launch (4 x 4 sub-blocks evaluated exactly, a whole block counting four), before
 * nhip_bnb_stats resets the totals */
int nhip_bnb_stats_per_pair(uint64_t *evaluated, int32_t n_pairs);
/* With NHIP_BNB_TIMELINE=1: per pair of the last launch four 100 MHz timestamps of its workgroup -- start, bounds
 * done, seeds done, end (the top 16 bits of the last one hold the hardware id of the CU it ran on); after the
 * n_pairs records two more values: first start and last end of the second kernel.  ticks: 4*n_pairs + 2 values */
int nhip_bnb_timeline(uint64_t *ticks, int32_t n_pairs);
/* ... and of the candidates' launch of the split form: ticks[i] = first start, ticks[n_pairs + i] = last end over the
 * workgroups that worked pair i of the last round (~0 / 0: none did).  ticks: 2*n_pairs values */
int nhip_bnb_timeline_candidates(uint64_t *ticks, int32_t n_pairs);

/* ------------------------------------------------------------------ the grid handle's other planes */
/* 1 when this handle's tables were built by an incremental REBUILD: nhip_grids_free hands the table buffer and its build
 * workspace back to the device buffer pool together, contents known; while nobody else has taken either, the next
 * nhip_grids_build of the same spec and target count takes the pair and clears what the previous build wrote (as
 * nhip_grid_rebuild_dev does, the workspace's tag checked on the device) instead of zero-filling every slot.  Same
 * tables, bit for bit.  0: a fresh allocation or a buffer of unknown contents, zero-filled (diagnostic). */
int nhip_grids_was_rebuilt(const nhip_grids_t *grids);
/* copy the plane of high bytes of grid `slot` (16-bit cells) to host in plain row-major form: rows x hi_pitch bytes.
 * On the device the plane is stored as two copies tiled 8 rows x 16 bytes (layout.hi_bytes bytes in all; the second
 * copy's tiles are shifted by 8 columns); `_copy` selects the copy that is read back (0 / 1: both hold the same bytes). */
int nhip_grids_download_hi_plane(const nhip_grids_t *grids, int32_t slot, uint8_t *out);
int nhip_grids_download_hi_plane_copy(const nhip_grids_t *grids, int32_t slot, int32_t copy, uint8_t *out);
/* 16-bit cells: the matcher's copy of the 16-bit image (tiled 8 rows x 8 cells on the device; it follows the two copies
 * of the plane of high bytes inside layout.hi_bytes) in the plain form of nhip_grids_download: layout.grid_bytes bytes */
int nhip_grids_download_tiled16(const nhip_grids_t *grids, int32_t slot, uint8_t *out);
/* copy the skip map of grid `slot` to host: layout.skip_bytes bytes (rows x 8*ceil(pitch/256) bytes, then padding) */
int nhip_grids_download_skip_map(const nhip_grids_t *grids, int32_t slot, uint8_t *out);
/* copy the max-pooled table of grid `slot` to host: layout.pool_bytes bytes (pool_rows x pool_pitch) */
int nhip_grids_download_pool(const nhip_grids_t *grids, int32_t slot, uint8_t *out);
/* the same for the second-level table: layout.pool4_bytes bytes (pool4_rows x pool4_pitch) */
int nhip_grids_download_pool4(const nhip_grids_t *grids, int32_t slot, uint8_t *out);
/* the hit raster of grid `slot`: layout.hits_bytes bytes (bit rows of hits_pitch bytes; see nhip_grid_layout_t.hits_bytes) */
int nhip_grids_download_hits(const nhip_grids_t *grids, int32_t slot, uint8_t *out);

/* ------------------------------------------------------------------ the float norm of the distance gates
 * The correspondence search, the loop-closure pair gate and the scan features decide by comparing ONE device function with
 * a threshold: norm(dx, dy) = sqrt(fl(fl(dx * dx) + fl(dy * dy))), every operation rounded to nearest on its own.  This runs
 * exactly that function on n device inputs on the caller's stream: d_out[i] = norm(d_dx[i], d_dy[i]), or with root_only
 * != 0 its last step alone, d_out[i] = sqrt(d_dx[i]) (d_dy is not read and may be null).  (Tests: the output must equal a
 * correctly rounded float chain as bit patterns.) */
int nhip_round_norm_dev(const float *d_dx, const float *d_dy, int64_t n, int32_t root_only, float *d_out, void *stream);

/* ------------------------------------------------------------------ in-stream kernel timing
 * When enabled, the dominant kernels are bracketed by hipEvents on their own stream.
 * ids: 0 = csm match (bounds, candidates, exact sums), 1 = grid build (everything nhip_grid_build_dev enqueues),
 *      2 = resid_lidar, 3 = corr_search, 4 = resid_normal_eq, 5 = the clearing part of a grid build (inside 1). */
#define NHIP_TIMER_CSM 0
#define NHIP_TIMER_GRID 1
#define NHIP_TIMER_RESID 2
#define NHIP_TIMER_CORR 3
#define NHIP_TIMER_NORMEQ 4
#define NHIP_TIMER_GRID_CLEAR 5
#define NHIP_TIMER_CSM_BOUNDS 6 /* split form of the matcher: bounds + seeds (csm_bnb_kernel<., ., true, true>) ... */
#define NHIP_TIMER_CSM_CAND 7   /* ... and the candidates (csm_bnb_cand_kernel); both inside NHIP_TIMER_CSM */
#define NHIP_TIMER_EXACT_SCORE 8 /* the pass of NHIP_SEARCH_EXACT_SCORE (after, not inside, NHIP_TIMER_CSM) */
#define NHIP_TIMER_VEC_RASTER 9  /* map vectorisation: clears, raster, cell list ... */
#define NHIP_TIMER_VEC_VOTES 10  /* ... the votes of every cell ... */
#define NHIP_TIMER_VEC_ROUNDS 11 /* ... and the rounds, one interval per batch of check_every rounds */
#define NHIP_TIMER_OCC_TRACE 12    /* occupancy grid: the clears and the ray trace of every scan ... */
#define NHIP_TIMER_OCC_CLASSIFY 13 /* ... and the classification of the window */
#define NHIP_TIMER_COUNT 14
int nhip_timing_enable(int on);
int nhip_timing_reset(void);
/* synchronises the recorded events; total_ms / launches since the last reset */
int nhip_timing_get(int id, double *total_ms, int32_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* NAUTILUS_HIP_DEBUG_H_ */
