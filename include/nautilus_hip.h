/*
 * nautilus_hip.h -- C ABI of the MI355X (gfx950) implementation of nautilus's loop-closure
 * correlative scan matcher and batched Ceres-residual evaluation.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ / torch types.  Each entry
 * point cites the reference interface it replaces (paths relative to the nautilus tree):
 *
 *   CorrelativeScanMatcher(30, 2, 0.3, 0.01)              src/optimization/solver.cc:56,633
 *   CorrelativeScanMatcher::GetTransformation(...)        src/optimization/solver.cc:634-638
 *   lookup-table geometry (side, cell index, rasterise)   src/visualization/cimg_debug.h:20-64
 *   LIDARNormalResidual / LIDARPointResidual functors     src/optimization/slam_residuals.h:64-177
 *   PointToLineResidual functor                           src/optimization/slam_residuals.h:179-216
 *   OdometryResidual functor                              src/optimization/slam_residuals.h:17-61
 *   ceres::CostFunction::Evaluate(parameters, residuals, jacobians) contract (Ceres 1.14):
 *       row-major num_residuals x 3 Jacobian per parameter block, NULL = not requested
 *   double pose[3] = (x, y, theta) parameter block        src/util/slam_types.h:159-178
 *
 * Conventions: every function returns 0 on success and a negative NHIP_ERR_* code on
 * failure (never aborts, never throws across the ABI); nhip_last_error() returns a
 * thread-local message.  "_dev" entry points take DEVICE pointers owned by the caller and
 * only enqueue work on `stream` (a hipStream_t passed as void*; NULL = default stream):
 * they allocate nothing and do not synchronise, so they can be captured in a hipGraph -- on a device that was named to
 * nhip_init (the current one) or nhip_set_device beforehand: those calls allocate the device's 16 status bytes (below).
 * A "_dev" call on a device the library never heard of allocates them itself, once (one hipMalloc + one synchronising
 * memset): do not let that be the first thing inside a stream capture.
 * Ids in device memory: the scan ids, grid slots, block ids and pose indices that a "_dev" entry point reads from DEVICE
 * arrays cannot be validated by the host without a round trip, so the KERNELS check each of them against the count
 * passed beside its array (n_scans, n_grids, n_blocks, n_poses ...).  An id outside [0, count) is never dereferenced: the
 * entry is treated as empty (a target without points, a pair that scores nothing, a correspondence that is skipped) and
 * recorded in the device's status words; nhip_dev_status(stream) -- call it where the host synchronises anyway --
 * returns NHIP_ERR_ARG with the offending id in nhip_last_error().  (The reference aborts on such input with a glog
 * CHECK, src/optimization/slam_residuals.h:99-101,109; a stale id here costs an error code, not the process.)
 * Handle entry points take HOST pointers, own their device memory and synchronise.
 * There is no CPU fallback anywhere: without a gfx950 device compute calls fail with
 * NHIP_ERR_NODEV.
 * The instruments -- counters, timers, launch reports, downloads of the matcher's private planes -- are declared in
 * nautilus_hip_debug.h, not here (one exception, at the end of this file: nhip_bnb_stats_chunks).
 */
#ifndef NAUTILUS_HIP_H_
#define NAUTILUS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NHIP_OK 0
#define NHIP_ERR_ARG (-1)    /* bad argument / shape mismatch (glog CHECK_* in the reference) */
#define NHIP_ERR_NODEV (-2)  /* no HIP device visible */
#define NHIP_ERR_HIP (-3)    /* a HIP runtime call failed */
#define NHIP_ERR_ALLOC (-4)  /* device or host allocation failed */
#define NHIP_ERR_STATE (-5)  /* handle used in the wrong state */

/* ------------------------------------------------------------------ general */
int nhip_init(int *n_devices);
int nhip_set_device(int device);
const char *nhip_last_error(void);
const char *nhip_version(void);
/* Synchronises `stream` (NULL = the default stream) and reports whether a kernel since the last call met an id in device
 * memory that was out of range (see "Ids in device memory" above): NHIP_OK, or NHIP_ERR_ARG with the message in
 * nhip_last_error().  info (may be NULL): {OR of the kinds seen, kind, value, index of the first one reported}; kinds:
 * 1 target scan id of a grid build, 2 source scan id of a pair, 4 grid slot of a pair, 8 block id of a correspondence,
 * 16 pose index of a block, 32 scan id of a correspondence-search block, 64 feature index and 128 feature count of
 * nhip_features_pack_dev, 256 scan offset of nhip_normals_estimate_dev, 512 member scan id and 1024 merged point count beyond
 * the capacity of nhip_submaps_gather_dev, 2048 contributor id of nhip_bsr_assemble_dev, 4096 block column of
 * nhip_bsr_assemble_dev / nhip_bsr_pcg_dev / nhip_bsr_pcg_columns_dev, 8192 gauge or right-hand-side index of
 * nhip_bsr_pcg_columns_dev, 16384 scan offset of nhip_vectorize_dev /
 * nhip_occupancy_dev / nhip_place_describe_dev / nhip_transient_filter_dev, 32768 source scan, grid slot or record index of a pair of
 * nhip_freespace_check_dev, 65536 scan id of the list of nhip_place_match_dev / nhip_place_seq_match_dev, 131072 degree and 262144
 * member index of nhip_consistency_set_dev, 524288 occupied cells beyond max_cells of nhip_mapwin_cells_dev (value: the cells
 * needed; index = height) or a row_ptr entry that is not a row in nhip_mapwin_gather_dev (index = the map row), 1048576 window
 * points beyond out_capacity of nhip_mapwin_gather_dev (value: the points needed, at most 2^31 - 1; index = n_queries), 2097152
 * anchors beyond max_anchors of nhip_rangesig_anchors_dev (value: the anchors found; index = max_anchors) or an entry of the ray
 * table that is not a ray in nhip_rangesig_map_dev (value: its n; index = the ray), 4194304 source or target scan id of a pair
 * of nhip_refine_icp_dev (index = the pair).
 * Clears the record
 * (in the order of `stream`).
 * ONE record per DEVICE, shared by every stream and host thread that uses the library on it: a host with several streams
 * on one device learns THAT an id was bad and which, not on which stream; a call that finds a record consumes it -- reports
 * of kernels still running on OTHER streams at that moment can be reported by this call or wiped by its clear.  Clients
 * that need their errors apart must check on their own device or serialise launch + nhip_dev_status.  The index reported is
 * the entry's position in the CALLER's array (also for lists the matcher works in rounds). */
int nhip_dev_status(void *stream, int32_t info[4]);

/* ------------------------------------------------------------------ likelihood grids
 * Replaces the lookup table CorrelativeScanMatcher builds from the target point cloud.
 * Geometry follows cimg_debug.h:20-37; the likelihood model (integer separable Gaussian
 * blur of the hit raster, floor, natural log, 8- or 16-bit quantisation) is the build-defined
 * spec of DESIGN.md section 3. */
typedef struct nhip_grid_spec {
  double range;       /* scanner range [m]: ctor arg 1 (solver.cc:633); side = floor(2*range/res) */
  double res;         /* cell size [m] */
  double sigma;       /* blur sigma in cells */
  double floor_p;     /* likelihood floor before the log (1e-10) */
  int32_t max_shift;  /* largest |cell shift| a search on these grids may use */
  int32_t cell_bits;  /* width of a quantised log-likelihood cell: 16 (or 0: the default) or 8.  16-bit cells
                         (65535 steps of 3.5e-4 nat) keep reported scores within 1e-5 relative of an unquantised
                         double table (cimg_debug.h:19 holds the reference's table as CImg<double>); 8-bit cells
                         (255 steps of 0.09 nat, scores within 1e-3) are the explicit opt-in for callers that only
                         gate on a threshold */
  int32_t flags;      /* 0, NHIP_GRID_SKIP_MAP or NHIP_GRID_NO_IMAGE */
  int32_t reserved;   /* 0 */
} nhip_grid_spec_t;
/* NHIP_GRID_SKIP_MAP: the slots of 16-bit grids carry a skip map too (8-bit grids always do).  Only the kernel that
 * performs every add reads it (NHIP_SEARCH_EXHAUSTIVE, lattices beyond the branch-and-bound matcher's envelope);
 * without it that kernel adds every window strip, zero or not -- same records, ~1.5x the time.  The flag describes
 * the buffer: pass the same spec to the build and to the match.  The handle API builds missing maps itself the first
 * time an exhaustive search needs them. */
#define NHIP_GRID_SKIP_MAP 1
/* NHIP_GRID_NO_IMAGE: the slots carry no row-major image (layout.grid_bytes = 0, layout.skip_bytes = 0): 8.4 MB per
 * 1200 x 1200 grid of 16-bit cells instead of 12.3, a third less to clear per rebuild, a quarter less for the build to
 * store.  The branch-and-bound matcher on scans of at most NHIP_SHORT_SCAN_POINTS points -- the product path: every
 * 1081-beam workload -- reads only the pooled tables, its tiled planes and (NHIP_SEARCH_EXACT_SCORE) the hit raster; the
 * pooled tables are then built from the tiled copy of the cells.  What needs the image is refused on such grids with
 * NHIP_ERR_ARG: the kernels that perform every add (NHIP_SEARCH_EXHAUSTIVE, lattices beyond the matcher's envelope, score
 * volumes), lists that hold a longer scan (the caller must set NHIP_SEARCH_SHORT_SCANS; the handle API sets it itself),
 * nhip_grids_download.  Not combinable with NHIP_GRID_SKIP_MAP.  The flag describes the buffer: pass the same spec to
 * the build and to the match. */
#define NHIP_GRID_NO_IMAGE 2

typedef struct nhip_grid_layout {
  int32_t side;        /* S: cells per side (cimg_debug.h:21-22) */
  int32_t pad;         /* zero border on every side: 2*max_shift + 16, multiple of 4 */
  int32_t pitch;       /* bytes per stored row = (S + 2*pad) * cell_bytes rounded up to a multiple of 16 */
  int32_t rows;        /* stored rows = S + 2*pad; cell (row, col) is at byte (row+pad)*pitch + (col+pad)*cell_bytes */
  int32_t blur_radius; /* R = ceil(3*sigma) */
  int32_t cell_bytes;  /* 1 or 2 */
  int64_t tap_sum;     /* K = sum of the integer blur taps */
  int64_t grid_bytes;  /* pitch*rows: bytes of one stored grid's row-major image (0 with NHIP_GRID_NO_IMAGE) */
  double score_floor;  /* Lf = ln(floor_p): value of cell 0 */
  double score_step;   /* log-likelihood per quantisation step = -Lf/255 (8-bit cells) or -Lf/65535 (16-bit) */
  int64_t skip_bytes;  /* bytes of the skip map stored right after each image: one bit per stored row
                          r and aligned dword column c (bit c&7 of byte c>>3, 8*ceil(pitch/256) bytes per
                          row) = "stored rows [r, r+21) x dwords [c, c+21*cell_bytes) hold a non-zero cell",
                          so the correlation kernel can leave out window strips that only add zeros (same
                          sums, bit for bit).  Built for 8-bit cells always, for 16-bit cells when the spec carries
                          NHIP_GRID_SKIP_MAP (the branch-and-bound matcher never reads it); zero otherwise */
  int64_t slot_bytes;  /* grid_bytes + skip_bytes + pool_bytes + pool4_bytes + hi_bytes + hits_bytes: grid t of a buffer
                          starts at byte t*slot_bytes */
  int64_t pool_bytes;  /* bytes of the max-pooled table stored after the skip map (branch-and-bound bounds):
                          pool_rows x pool_pitch bytes, entry (i, j) = max of stored cells [8i, 8i+15) x [8j, 8j+15)
                          (16-bit cells: ceil(max / 257)), so that the sum of pooled entries bounds every score of
                          an 8 x 8 block of translations from above */
  int32_t pool_pitch;
  int32_t pool_rows;
  int64_t pool4_bytes; /* the second-level table, stored after the first: pool4_rows x pool4_pitch bytes.  With
                          P4[i][j] = max of stored cells [4i, 4i+7) x [4j, 4j+7) (16-bit cells: ceil(max / 257)), the
                          bounds of the 4 x 4 sub-blocks of a block of translations, byte (i, 2j) holds P4[i][j] and
                          byte (i, 2j+1) holds P4[i+1][j]: one read returns both sub-block rows */
  int32_t pool4_pitch;
  int32_t pool4_rows;
  int64_t hi_bytes;    /* after the second table, the matcher's 8-BIT PLANE: the cells' HIGH BYTES (cell >> 8; 8-bit cells: the cells),
                          hi_bytes bytes: two copies tiled 8 rows x 16 bytes, the second shifted by 8 columns (nhip_common.h
                          hi_tiled(); nhip_grids_download_hi_plane returns it as rows x hi_pitch), then (16-bit cells) the image once
                          more, tiled 8 rows x 8 cells (nhip_grids_download_tiled16).  The branch-and-bound matcher
                          takes its exact block sums on this plane at the cost of 8-bit cells -- 256*sum(high bytes) +
                          255*points bounds a pose's 16-bit sum from above -- and reads 16-bit cells for the few poses
                          whose bound still reaches the best sum: same records, bit for bit */
  int32_t hi_pitch;
  int32_t hits_pitch;  /* bytes per bit row of the hit raster (below) */
  int64_t hits_bytes;  /* after the matcher's planes, the HIT RASTER the table was blurred from: one bit per cell, rows
                          side + 64 (a zero border of 32 cells on every side), hits_pitch bytes each; bit (row, col) is bit
                          (col + 32) & 31 of dword (col + 32) >> 5 of bit row row + 32.  NHIP_SEARCH_EXACT_SCORE reads it */
} nhip_grid_layout_t;

/* Pure host helpers (work without a GPU). */
int nhip_grid_layout(const nhip_grid_spec_t *spec, nhip_grid_layout_t *out);
/* bytes the caller must allocate for n grids (n*slot_bytes + 256 B read slack) */
int64_t nhip_grids_bytes(const nhip_grid_spec_t *spec, int64_t n_grids);
/* workspace for nhip_grid_build_dev processing `chunk` targets at a time: per target one occupancy byte, one list slot and
 * 20 bytes of line masks per 64 x 64 tile (what nhip_grid_rebuild_dev clears is read from there), + the 16-bit quantiser's table */
int64_t nhip_grid_workspace_bytes(const nhip_grid_spec_t *spec, int32_t chunk);
/* integer blur taps (2R+1 values) and the quantiser threshold table: 256 entries for 8-bit cells,
 * 65536 for 16-bit cells (thresholds[k] = smallest integer blur sum whose quantised value is >= k) */
int nhip_grid_tables(const nhip_grid_spec_t *spec, int32_t *taps, uint32_t *thresholds);

/* ------------------------------------------------------------------ search lattice
 * BASELINE config #2: n_theta = 61, theta_step = 1 deg, nx = ny = 81 (one cell = 5 cm).
 * Translations are integer cell shifts ix-(nx-1)/2, iy-(ny-1)/2; rotation k is
 * theta0 + (k-(n_theta-1)/2)*theta_step with theta0 = AngleMod(rot_a - rot_b)
 * (math_util.h:81-89), i.e. the odometry estimate of "A to B in B's frame"
 * (solver.cc:631-638). */
typedef struct nhip_search {
  int32_t n_theta;
  int32_t nx;
  int32_t ny;
  int32_t flags;     /* 0, or an OR of NHIP_SEARCH_* */
  double theta_step; /* radians */
} nhip_search_t;
/* The matcher's result is that of the exhaustive (theta, x, y) search, always.  By default it gets there by
 * branch and bound: upper bounds of every 8 x 8 block of translations from a max-pooled copy of the table, bounds
 * of the 4 x 4 sub-blocks of the blocks that reach the best sum found from a second one, then exact sums only for
 * the sub-blocks whose bound still reaches it (indices, sums and scores are identical to the exhaustive kernel's,
 * bit for bit: tests compare the two).  NHIP_SEARCH_EXHAUSTIVE (or, in a process started with NHIP_TUNABLES=1, the environment variable NHIP_CSM_EXHAUSTIVE=1)
 * forces the kernel that performs every add (csm_correlate_kernel for 8-bit, csm_correlate16_kernel for 16-bit cells;
 * also taken for lattices of more than 88 x 88 translations, or more rotations than fit the LDS beside the bounds:
 * ~230 -- e.g. GetTransformation with a rotation restriction of pi).
 * Scan length: sums are reported as int32, so with 16-bit cells a scan may hold at most 32,768 points (8-bit:
 * 8,421,504); the handle API checks it, callers of the _dev entry points must. */
#define NHIP_SEARCH_EXHAUSTIVE 1
/* NHIP_SEARCH_DENSE (with the kernel that performs every add): add every window strip, the all-zero ones the skip map
 * would leave out too -- literally every add of the exhaustive definition; same records, ~1.5x the time. */
#define NHIP_SEARCH_DENSE 2
/* NHIP_SEARCH_SHORT_SCANS: the caller vouches that every source scan of the list has at most NHIP_SHORT_SCAN_POINTS
 * points (a 1081-beam scan does).  The branch-and-bound matcher serves longer scans with a second instantiation of its
 * kernel, launched beside the first over all pairs (its workgroups return at once when their pair is not theirs); with
 * this flag it is not launched.  A PROMISE: pairs whose scan is longer are then not matched at all (their records are
 * whatever d_keys held).  The handle API (nhip_csm_match) knows the lengths and sets the flag itself. */
#define NHIP_SEARCH_SHORT_SCANS 4
#define NHIP_SHORT_SCAN_POINTS 1088
/* NHIP_SEARCH_EXACT_SCORE: the record's `score` is the winning pose's mean log-likelihood on the UNQUANTISED table -- what a
 * table of doubles (the reference's CImg<double>, cimg_debug.h:19) gives at that pose -- instead of Lf + step * sum / N on the
 * quantised cells.  Indices and integer sums are unchanged (the search itself runs on the quantised table); one more kernel
 * recomputes, for the one pose that won, the exact integer blur sum of each cell a point reads from the slot's hit raster
 * and its logarithm in double (~0.05 ms per 10,000 pairs).  Without the flag a reported score is within half a
 * quantisation step of that value per cell -- measured up to 2.3e-5 relative on 1,300 pairs with 16-bit cells, 8.5e-4 with
 * 8-bit cells; with it, within double rounding (the record's float: 6e-8). */
#define NHIP_SEARCH_EXACT_SCORE 8
/* NHIP_SEARCH_LATENCY (with NHIP_SEARCH_EXHAUSTIVE): the list is a FEW pairs and what counts is how soon the call returns, not
 * lookups per second.  Every add is then performed by the kernel whose lanes are poses (csm_small_plane_kernel), a plane of
 * more than 256 translations in tiles of whole rows, one workgroup per (pair, rotation, tile) -- as long as that is at most
 * 2,048 workgroups (otherwise the flag is ignored and the strip kernels take the list).  GetTransformation's fine level
 * (21 x 61 x 61 on a 6000 x 6000 table) takes ~45 us this way whatever the clouds.  Same records as every other form. */
#define NHIP_SEARCH_LATENCY 16

/* One result per candidate pair: 16 bytes, the record that is all-gathered across GPUs. */
typedef struct nhip_match {
  int32_t itheta;
  int32_t ix;
  int32_t iy;
  float score; /* mean log-likelihood (<= 0), cf. csm_score_threshold = -5 (default_config.lua:85) */
} nhip_match_t;

/* Device memory of the handle API.  Handles own their device buffers; a buffer a handle lets go of (nhip_*_free, the
 * workspace and scratch of nhip_csm_match, ...) is KEPT for the next allocation of the same device that it fits (at most
 * twice the size asked for) instead of going back to the driver: hipFree is a device-wide synchronisation whose cost is not
 * the library's to bound (measured: 0.2 - 8 ms per call on a quiet device, 0.33 s per call for seconds after another client
 * of the process released 130 GB).  A buffer is filed under the device it was ALLOCATED on, whatever
 * device is current when its handle is freed.  At most max_bytes are kept PER DEVICE (default 4 GB: the workspace of a
 * 10,000-pair match, the tables of a few hundred targets; least recently released out first; 0 = nothing is kept, every
 * release is a hipFree); a host that cycles larger tables through build / free raises it (bench.py's host-buffer leg: 32
 * GB).  What the pool holds is invisible to other allocators in the process (torch's caching allocator): call
 * nhip_device_pool_release() -- everything back to the driver now -- before handing the device's memory to them; _stats
 * reports what is held (all devices).  A failed allocation releases the device's pool and tries again.  On an error path a
 * handle call waits for the device before its buffers return to the pool.
 * The "_dev" entry points never allocate and are not concerned. */
int nhip_device_pool_configure(int64_t max_bytes);
int nhip_device_pool_release(void);
int nhip_device_pool_stats(int64_t *entries, int64_t *bytes);

/* Host helpers: (cos, sin) of theta0 per pair and of the lattice offsets, in double. */
int nhip_csm_rot0(const double *rot_a, const double *rot_b, int32_t n, double *cs_out /* 2n */);
int nhip_csm_delta_table(const nhip_search_t *search, double *cs_out /* 2*n_theta */);
/* Host helper: (tx, ty, theta) of a match, as consumed at solver.cc:640-644. */
int nhip_match_to_transform(const nhip_match_t *m, const nhip_grid_spec_t *spec,
                            const nhip_search_t *search, double theta0, int32_t origin_x,
                            int32_t origin_y, float *tx, float *ty, float *theta);
double nhip_score_from_sum(const nhip_grid_spec_t *spec, int64_t sum, int32_t n_points);
/* Host helper: the FLOOR of the score gate (nhip_csm_match_gated) for a scan of n_points points,
 *   floor = max(0, floor(n_points * ((min_score - Lf) / step - 1)))   (Lf = ln floor_p, step = -Lf / 255 or / 65535),
 * one whole quantisation step per point below the sum min_score implies.  Every pose whose sum is below it scores below
 * min_score, quantised or exact (NHIP_SEARCH_EXACT_SCORE): a gated search prunes against it from the start.  The kernels
 * evaluate the same expression.  min_score NaN or n_points < 0: NHIP_ERR_ARG; -INFINITY: 0. */
int nhip_csm_gate_floor(const nhip_grid_spec_t *spec, double min_score, int32_t n_points, int32_t *floor_sum);

/* ------------------------------------------------------------------ device-pointer API */
/* K1: build likelihood grids for n_targets scans (scan ids in d_target_ids) into
 * d_grids (nhip_grids_bytes(spec, n_targets) bytes): slot t = position in d_target_ids, at byte
 * t * slot_bytes, holds the stored image (grid_bytes) followed by its skip map (skip_bytes) and the two
 * max-pooled tables (pool_bytes, pool4_bytes).
 * d_xy: float2 points of all scans, d_offsets: n_scans+1 prefix offsets (in points).
 * d_target_ids live in device memory: the kernels check every id against n_scans; one outside [0, n_scans) gives an
 * all-floor grid (a target without points) and an error from nhip_dev_status().  The offsets themselves are the
 * caller's: they must be non-decreasing and end inside d_xy. */
int nhip_grid_build_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids,
                        int32_t n_targets, const nhip_grid_spec_t *spec, uint8_t *d_grids,
                        void *d_workspace, int64_t workspace_bytes, void *stream);

/* The same build INTO A BUFFER THE PREVIOUS BUILD FILLED: instead of zero-filling n_targets * slot_bytes (gigabytes at
 * 1000 targets) it clears the ~20 % of 64 x 64 tiles the previous build wrote -- their list is still in the workspace
 * -- and the small derived tables.  Contract: same d_workspace as the build that last wrote d_grids, and d_grids
 * untouched since.  The workspace header carries a tag of (d_grids, n_targets, geometry) that the clearing kernel checks
 * on the device: a header that does not vouch for this buffer (fresh or recycled workspace memory, another buffer,
 * another spec) makes the call clear everything, i.e. behave as nhip_grid_build_dev.  Same results, bit for bit. */
int nhip_grid_rebuild_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids,
                          int32_t n_targets, const nhip_grid_spec_t *spec, uint8_t *d_grids,
                          void *d_workspace, int64_t workspace_bytes, void *stream);

/* K10: SUBMAPS -- the target cloud of a table built from several neighbouring scans instead of one (DESIGN.md section 3,
 * "Submaps").  Target t has the members member_scan[member_offsets[t] .. member_offsets[t + 1]); member m has four floats
 * (c, s, tx, ty) at member_affine + 4m, its frame in the target's anchor frame.  A member point (x, y) becomes
 *   x' = ((c x) + ((-s) y)) + tx,   y' = ((s x) + (c y)) + ty
 * in float, every operation rounded on its own; the merged cloud of a target is its members' points in member order, then
 * point order.  Nothing is dropped or deduplicated, non-finite points stay non-finite, points outside the grid are left to
 * the table build.
 *
 * nhip_submap_member_affines: pure host (works without a GPU).  Member m's affine from the poses (x, y, theta: 3 doubles
 * each) of its anchor anchor_of_member[m] and of its scan member_scan[m], both indices into `poses`: the entries of
 * inverse(A(anchor)) * A(member) in double, A as PoseArrayToAffine (slam_util.h:20-28) and the inverse the rigid one,
 *   c = ca cm + sa sm,  s = ca sm - sa cm,  tx = ca dx + sa dy,  ty = ca dy - sa dx   (dx, dy = member - anchor translation),
 * each rounded to float.  An index outside [0, n_poses) is NHIP_ERR_ARG and nothing is written. */
int nhip_submap_member_affines(const double *poses, int32_t n_poses, const int32_t *anchor_of_member, const int32_t *member_scan,
                               int32_t n_members, float *out /* 4 per member */);
/* The merged clouds of n_targets submaps, on the caller's buffers and stream; never allocates.  Outputs: d_out_offsets
 * (n_targets + 1 prefix offsets, in points) and d_out_xy (the packed cloud, room for out_capacity points): exactly what
 * nhip_grid_build_dev / nhip_grid_rebuild_dev take as (d_xy, d_offsets, n_scans = n_targets) with target ids 0 .. n_targets - 1.
 * d_member_offsets (n_targets + 1, non-decreasing, the caller's like d_offsets) and d_member_scan live in device memory: a
 * member id outside [0, n_scans) is an EMPTY member -- never dereferenced -- and nhip_dev_status() reports it (kind 512).
 * If the merged clouds hold more than out_capacity points (or more than 2^31 - 1) NOTHING is stored in d_out_xy, every entry
 * of d_out_offsets is 0 (every target empty) and nhip_dev_status() reports it (kind 1024, value: the points needed). */
int nhip_submaps_gather_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_member_scan,
                            const float *d_member_affine, const int32_t *d_member_offsets, int32_t n_targets, float *d_out_xy,
                            int64_t out_capacity, int32_t *d_out_offsets, void *stream);

/* K2+K3: exhaustive (theta, x, y) correlation + argmax for n_pairs candidate pairs.
 * Pair i matches scan d_pair_src[i] (of the n_scans behind d_offsets) against grid slot d_pair_slot[i] (of the n_grids in
 * d_grids).  Both arrays live in device memory: a pair whose scan or slot is out of range scores nothing (record: pose 0,
 * sum 0, the floor score) and makes nhip_dev_status() return an error.
 * d_rot0_cs: 2 doubles (cos, sin theta0) per pair; d_delta_cs: 2 doubles per lattice rotation.
 * d_pair_origin: NULL, or 2 int32 per pair = (x, y) cell offset of the search centre (used by
 * the fine level of a coarse-to-fine search); |origin| + half-width must be <= max_shift.
 * d_keys: n_pairs uint64 scratch; d_out: n_pairs records; d_sums: n_pairs int32 or NULL.
 * d_workspace: NULL, or nhip_csm_workspace_bytes(n_pairs) bytes of scratch for the branch-and-bound matcher.  Lists of
 * fewer than 192 pairs use it for hand-over lists: a pair whose landscape is flat (hundreds of candidate blocks after
 * bounds and seeds; in lists of <= 64 pairs, e.g. a single GetTransformation call, every pair) hands all but its first
 * 8 rotations to a second kernel that works them with every wave of the chip instead of keeping its one workgroup busy
 * for milliseconds.  Lists of 192 pairs and more run as two kernels -- bounds + seeds, whose workgroups all take the
 * same time, then the candidates of all pairs, the heaviest pairs shared by several workgroups -- with each pair's rows
 * of bounds parked in the workspace in between (nhip_csm_workspace_bytes asks for 32 KB per pair there, for at most
 * 262,144 pairs: 328 MB at 10,000 pairs; 10,000 pairs: 8.2 -> 6.3 ms, 3,000 pairs: 4.1 -> 2.6 ms).  Lists of more than
 * 131,072 pairs go through in rounds of that many, the candidates of a round on an internal stream of the current
 * device (ordered before and after `stream` by events) beside the next round's bounds.  A workspace that is NULL or too
 * small takes the one-kernel form.  Same records in every form. */
int nhip_csm_match_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                       int32_t n_grids, const nhip_grid_spec_t *spec, const int32_t *d_pair_src,
                       const int32_t *d_pair_slot, const double *d_rot0_cs,
                       const double *d_delta_cs, const int32_t *d_pair_origin, int32_t n_pairs,
                       const nhip_search_t *search, uint64_t *d_keys, nhip_match_t *d_out,
                       int32_t *d_sums, void *d_workspace, int64_t workspace_bytes, void *stream);
/* The same match with a SCORE GATE: the caller's csm_score_threshold (default_config.lua:84-85, "above -5 => success").
 * Let rec / sum be what nhip_csm_match_dev returns for the same arguments.  The gated call returns
 *   - rec and sum unchanged when (double)rec.score >= min_score;
 *   - otherwise the REJECTED record {itheta = ix = iy = -1, score = -INFINITY} and sum -1.
 * This holds in every form the matcher runs in (branch and bound fused or split, with or without the hand-over kernel; the
 * strip kernels; NHIP_SEARCH_LATENCY), with or without NHIP_SEARCH_EXACT_SCORE and d_pair_origin.  A pair whose ids are out
 * of range still makes nhip_dev_status() report the error; its record (floor score) is gated like any other.
 * min_score = -INFINITY: the gate is off -- records, sums and nhip_csm_last_launch byte-identical to nhip_csm_match_dev's,
 * which is this call with -INFINITY.  min_score NaN: NHIP_ERR_ARG, nothing is written.  The gate never changes which form
 * runs.  What it saves: branch and bound starts each pair's best at the floor (nhip_csm_gate_floor), so blocks whose bound
 * is below it are pruned at once, and a pair whose highest bound is below it is settled right after its bounds. */
int nhip_csm_match_gated_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                             int32_t n_grids, const nhip_grid_spec_t *spec, const int32_t *d_pair_src,
                             const int32_t *d_pair_slot, const double *d_rot0_cs,
                             const double *d_delta_cs, const int32_t *d_pair_origin, int32_t n_pairs,
                             const nhip_search_t *search, uint64_t *d_keys, nhip_match_t *d_out,
                             int32_t *d_sums, void *d_workspace, int64_t workspace_bytes, void *stream, double min_score);
int64_t nhip_csm_workspace_bytes(int32_t n_pairs);

/* Full score volume of ONE pair (tests / debugging): sums[(k*nx + ix)*ny + iy]. */
int nhip_csm_scores_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                        int32_t n_grids, const nhip_grid_spec_t *spec, int32_t src, int32_t slot,
                        const double *d_rot0_cs, const double *d_delta_cs, int32_t origin_x,
                        int32_t origin_y, const nhip_search_t *search, int32_t *d_sums,
                        void *stream);

/* K4: batched LIDAR residual + Jacobian evaluation.
 * kind: NHIP_LIDAR_NORMAL (slam_residuals.h:65-89) or NHIP_LIDAR_POINT (:124-145).
 * d_corr: 8 floats per correspondence (source point, target point, source normal, target
 * normal -- the four vectors of PointCorrespondences, data_structures.h:62-66).
 * d_corr_block: block id of every correspondence; block b reads poses d_block_src[b]
 * ("source_pose", parameter block 0) and d_block_tgt[b] ("target_pose", block 1) from
 * d_poses[n_poses][3].  d_block_consts: n_blocks*8 doubles scratch.
 * Outputs: d_residuals 2 doubles / correspondence; d_jac_src, d_jac_tgt 6 doubles /
 * correspondence (rows 2i, 2i+1 of the row-major (2N x 3) Jacobian); either may be NULL. */
#define NHIP_LIDAR_NORMAL 0
#define NHIP_LIDAR_POINT 1
int nhip_resid_lidar_dev(int kind, const float *d_corr, const int32_t *d_corr_block,
                         int64_t n_corr, const int32_t *d_block_src, const int32_t *d_block_tgt,
                         int32_t n_blocks, const double *d_poses, int32_t n_poses,
                         double *d_block_consts, double *d_residuals, double *d_jac_src,
                         double *d_jac_tgt, void *stream);

/* On-device normal equations of the LIDAR blocks: instead of
 * shipping 96 B of Jacobian per correspondence to the host, each block is reduced to what a
 * Gauss-Newton / Levenberg-Marquardt step needs.  With J = [J_src | J_tgt] (2N x 6) and r (2N):
 *   d_out[28*b +  0..20] = upper triangle of J^T J, row-major (i <= j)
 *   d_out[28*b + 21..26] = J^T r
 *   d_out[28*b + 27]     = r^T r
 * Same functors, same closed-form Jacobians as nhip_resid_lidar_dev; d_block_offsets has
 * n_blocks+1 entries (rows of d_corr per block). */
int nhip_resid_lidar_normal_eq_dev(int kind, const float *d_corr, const int32_t *d_block_offsets,
                                   const int32_t *d_block_src, const int32_t *d_block_tgt,
                                   int32_t n_blocks, const double *d_poses, int32_t n_poses,
                                   double *d_block_consts, double *d_out, void *stream);

/* PointToLineResidual (slam_residuals.h:180-200): block b has line segment d_segments[4b..]
 * (x0 y0 x1 y1, LineSegment<float>), points d_points[2i..] with block id d_point_block[i],
 * parameter blocks pose = d_poses[d_block_pose[b]] and line_pose = d_line_poses[d_block_line[b]].
 * Outputs: 1 residual / point, 3 doubles / point per Jacobian (may be NULL). */
int nhip_resid_point_to_line_dev(const float *d_segments, const float *d_points,
                                 const int32_t *d_point_block, int64_t n_points,
                                 const int32_t *d_block_pose, const int32_t *d_block_line,
                                 int32_t n_blocks, const double *d_poses, int32_t n_poses,
                                 const double *d_line_poses, int32_t n_line_poses, double *d_residuals,
                                 double *d_jac_pose, double *d_jac_line, void *stream);

/* The normal equations of PointToLineResidual blocks, the point-to-line counterpart of nhip_resid_lidar_normal_eq_dev: block b
 * holds the points d_points[2 * d_block_offsets[b] .. 2 * d_block_offsets[b + 1]) (blocks are contiguous: the packed layout
 * of nhip_hitl_pack_dev; d_block_offsets has n_blocks + 1 entries), its segment, pose and line pose as above.  With one
 * residual per point and J = [d r / d pose | d r / d line_pose] (n x 6), the same functor and Jet rules as
 * nhip_resid_point_to_line_dev:
 *   d_out[28*b +  0..20] = upper triangle of J^T J, row-major (i <= j)
 *   d_out[28*b + 21..26] = J^T r
 *   d_out[28*b + 27]     = r^T r
 * An empty block gives 28 zeros.  A block whose pose or line-pose index is out of range gives 28 zeros and makes
 * nhip_dev_status() report it (kind 16, the index, the block).  A point whose Jet is NaN (a zero-length segment under the
 * point) makes the sums it enters NaN, as on the host.  The same input gives the same bits. */
int nhip_resid_point_to_line_normal_eq_dev(const float *d_segments, const float *d_points, const int32_t *d_block_offsets,
                                           const int32_t *d_block_pose, const int32_t *d_block_line, int32_t n_blocks,
                                           const double *d_poses, int32_t n_poses, const double *d_line_poses,
                                           int32_t n_line_poses, double *d_out, void *stream);

/* OdometryResidual (slam_residuals.h:18-40): factor f has T_odom d_t_odom[2f..] (Vector2f),
 * R_odom d_r_odom[f] (float), poses d_pose_i[f], d_pose_j[f].  3 residuals, 3x3 Jacobians. */
int nhip_resid_odometry_dev(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                            const int32_t *d_pose_j, int32_t n_factors, double translation_weight,
                            double rotation_weight, const double *d_poses, int32_t n_poses, double *d_residuals,
                            double *d_jac_i, double *d_jac_j, void *stream);

/* The same factors reduced to their normal equations, 28 doubles per factor in the layout of the other *_normal_eq_dev
 * calls, over the six parameters [pose_i | pose_j] (J = [J_i | J_j], 3 x 6):
 *   d_out[28*f + 0..20]  = upper triangle of J^T J, row-major     d_out[28*f + 21..26] = J^T r     d_out[28*f + 27] = r^T r
 * Every sum runs over the three residual rows, products rounded, added in row order 0, 1, 2 (no contraction): bit-equal to
 * the same sums formed on the host from nhip_resid_odometry_dev's J and r.  A factor whose pose index is out of range gives
 * 28 zeros and makes nhip_dev_status() report it (kind 16).  n_factors == 0 launches nothing. */
int nhip_resid_odometry_normal_eq_dev(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                                      const int32_t *d_pose_j, int32_t n_factors, double translation_weight,
                                      double rotation_weight, const double *d_poses, int32_t n_poses, double *d_out,
                                      void *stream);

/* The same factors under a ROBUST LOSS ("Robust loss"; kernel nhip_loss.hip).  With r and J as above,
 * s = r0 r0 + r1 r1 + r2 r2 (products rounded, added in that order; the plain call's slot 27), a the scale in units of the
 * weighted residual and b = a a (one rounded product):
 *   kind          rho(s)                                   rho'(s)
 *   NONE    (0)   s                                        1
 *   HUBER   (1)   s <= b: s;  else 2 a sqrt(s) - b         s <= b: 1;  else a / sqrt(s)
 *   SOFT_L1 (2)   2 b (sqrt(1 + s/b) - 1)                  1 / sqrt(1 + s/b)
 *   CAUCHY  (3)   b log1p(s/b)                             1 / (1 + s/b)
 * (Ceres' HuberLoss, SoftLOneLoss, CauchyLoss; the operation order is nhip_loss.hip's header and nautilus_amd/loss.py).
 * All have rho'' <= 0, for which Ceres' Corrector scales by w = sqrt(rho') and nothing else: r~ = w r, J~ = w J, every entry
 * one rounded product.  The row:
 *   d_out[28*f + 0..20] = upper triangle of J~^T J~     d_out[28*f + 21..26] = J~^T r~     d_out[28*f + 27] = rho(s)
 * with the sums in the plain call's order, so that half the sum of the slots 27 is Ceres' robust cost.  d_weights, unless
 * NULL, receives {s, rho, rho', sqrt(rho')} per factor.  NONE gives the plain call's row bit for bit.  A factor whose pose
 * index is out of range gives 28 + 4 zeros and is reported (kind 16); n_factors == 0 launches nothing.
 * NHIP_ERR_ARG before anything is launched, with or without a device: a kind outside 0..3, flags != 0, with a kind other
 * than NONE a scale that is not finite or is <= 0, a negative size, a null pointer other than d_weights. */
#define NHIP_LOSS_NONE 0
#define NHIP_LOSS_HUBER 1
#define NHIP_LOSS_SOFT_L1 2
#define NHIP_LOSS_CAUCHY 3
typedef struct nhip_loss_spec {
  int32_t kind;  /* NHIP_LOSS_* */
  int32_t flags; /* 0 */
  double scale;  /* a; unused by NONE */
} nhip_loss_spec_t;
int nhip_resid_odometry_robust_normal_eq_dev(const float *d_t_odom, const float *d_r_odom, const int32_t *d_pose_i,
                                             const int32_t *d_pose_j, int32_t n_factors, double translation_weight,
                                             double rotation_weight, const nhip_loss_spec_t *loss, const double *d_poses,
                                             int32_t n_poses, double *d_out, double *d_weights, void *stream);

/* ------------------------------------------------------------------ K23: relative-pose factors
 * A factor that measures one pose IN THE FRAME OF ANOTHER, with the measurement's own information (DESIGN.md section 3,
 * "Relative-pose factors"; kernel nhip_relpose.hip).  Factor f couples a = d_pose_i[f] (a loop closure's target scan) and
 * b = d_pose_j[f] (its source): d_z[4f ..] = (z_x, z_y, c_z, s_z), pose b in a's frame with the heading as cosine and sine --
 * a refined record's (tx, ty, c, s); d_info[6f ..] = L00 L01 L02 L11 L12 L22, the information over (x, y, theta) --
 * nhip_refined_t.info's layout.  All in double, every product and sum rounded on its own, sums in the order written:
 *   d   = R(theta_a)^T (t_b - t_a):  d_x = c_a D_x + s_a D_y,  d_y = (-s_a) D_x + c_a D_y
 *   e   = (d_x - z_x, d_y - z_y, atan2(s_e, c_e)),  c_r = c_a c_b + s_a s_b,  s_r = c_a s_b - s_a c_b,
 *         c_e = c_r c_z + s_r s_z,  s_e = s_r c_z - c_r s_z
 *   E   = d e / d [a | b]: (-c_a, -s_a, d_y, c_a, s_a, 0), (s_a, -c_a, -d_x, -s_a, c_a, 0), (0, 0, -1, 0, 0, 1)
 *   W   upper triangular with W^T W = Lambda, from the square-root-free Cholesky of K22's solve: D0 = L00, l10 = L01 / D0,
 *       l20 = L02 / D0, D1 = L11 - l10 L01, u = L12 - l20 L01, l21 = u / D1, D2 = (L22 - l20 L02) - l21 u, q_k = sqrt(D_k):
 *       W00 = q0, W01 = q0 l10, W02 = q0 l20, W11 = q1, W12 = q1 l21, W22 = q2
 *   r_k = sum_{m >= k} W_km e_m,  J_kp = sum_{m >= k} W_km E_mp  (ascending m, every term formed)
 * nhip_resid_relpose_dev writes r (3 per factor) and, unless NULL, J_i and J_j (3 x 3 row-major each: the halves of J),
 * d_parts (8 per factor: c_a, s_a, c_b, s_b, e_x, e_y, e_theta, 0) and d_flags (one int32 per factor).  A flagged factor is
 * all zeros:  NHIP_RELPOSE_BAD_INFO an entry of Lambda is not finite or a pivot D_k is not > 0;  NHIP_RELPOSE_BAD_MEASUREMENT
 * an entry of z is not finite;  NHIP_RELPOSE_SAME_POSE pose_i == pose_j (a row of the block-sparse system couples two
 * different blocks).  A pose id outside [0, n_poses) is never dereferenced: zeros, and nhip_dev_status() reports it (kind 16).
 *
 * nhip_resid_relpose_normal_eq_dev writes the factors' 28-double rows under a loss (NULL: NONE), exactly as
 * nhip_resid_odometry_robust_normal_eq_dev forms them from its r and J: s = r0 r0 + r1 r1 + r2 r2 -- here a squared
 * Mahalanobis distance, so the loss' scale is in standard deviations --, w = sqrt(rho'(s)), r~ = w r, J~ = w J, the upper
 * triangle of J~^T J~, J~^T r~, and rho(s) in slot 27; d_weights, unless NULL, {s, rho, rho', w} per factor; d_flags, unless
 * NULL, the flags.  One kernel, nothing allocated; n_factors == 0 launches nothing.  The same input gives the same bits.
 * NHIP_ERR_ARG before anything is launched, with or without a device: a bad loss spec, a negative size, a null pointer other
 * than those named optional above.
 *
 * nhip_relpose_information (pure host) makes the information of n refined records: Lambda = H (1 / sigma_m^2) -- one rounded
 * reciprocal of one rounded product, six products -- for a record that carries a refined pose (no flag but
 * NHIP_REFINE_NOT_CONVERGED); diag(wt wt, wt wt, wr wr) for any other, which kept its lattice pose.  from_icp[k], unless NULL,
 * is 1 for the former.  refined may be NULL: every record gets the diagonal.  A negative n, a null info, a sigma_m that is not
 * finite or is <= 0, a wt or wr that is not finite: NHIP_ERR_ARG.  (Declared behind nhip_refined_t, below.) */
/* CAUCHY under these rows: rho = b log1p_pinned(s / b), log1p for x >= 0 written out in IEEE operations (fdlibm's s_log1p.c, error
 * below 1 ulp), so that the device, this library's host compilation and nautilus_amd/loss.py's numpy form return the same doubles;
 * nhip_resid_odometry_robust_normal_eq_dev keeps the device library's log1p.  nhip_loss_log1p_pinned (pure host) evaluates it
 * on n doubles. */
int nhip_loss_log1p_pinned(const double *x, int64_t n, double *out);
#define NHIP_RELPOSE_BAD_INFO 1
#define NHIP_RELPOSE_BAD_MEASUREMENT 2
#define NHIP_RELPOSE_SAME_POSE 4
int nhip_resid_relpose_dev(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                           int32_t n_factors, const double *d_poses, int32_t n_poses, double *d_residuals, double *d_jac_i,
                           double *d_jac_j, double *d_parts, int32_t *d_flags, void *stream);
int nhip_resid_relpose_normal_eq_dev(const double *d_z, const double *d_info, const int32_t *d_pose_i, const int32_t *d_pose_j,
                                     int32_t n_factors, const nhip_loss_spec_t *loss, const double *d_poses, int32_t n_poses,
                                     double *d_out, double *d_weights, int32_t *d_flags, void *stream);

/* ------------------------------------------------------------------ K11: the pose graph's linear system on the device
 * The Gauss-Newton system of a pose graph as a block-sparse matrix of 3 x 3 blocks in fp64 (DESIGN.md section 3,
 * "Block-sparse system").  n_blocks unknown blocks of 3; the sources are 28-double rows (every *_normal_eq_dev call writes
 * them): row r couples two DIFFERENT unknown blocks u[r], v[r], its 6 x 6 ordered [u | v].  The structure is the caller's,
 * built once per graph (nautilus_amd/linsolve.py builds it): d_row_ptr[n_blocks + 1] and d_col[nnzb] (block columns,
 * ascending within a block row, the diagonal block always present, the full symmetric pattern), d_contrib_ptr[nnzb + 1] and
 * d_contrib[n_contrib]: the contributors of every stored block, ascending, as 4 * r + q -- quadrant q of row r's 6 x 6:
 * 0 (u,u), 1 (u,v), 2 (v,u) = quadrant 1 transposed, 3 (v,v).  d_row_ptr and d_contrib_ptr are the caller's like every
 * offsets array (non-decreasing, from 0 to nnzb / n_contrib); d_col and d_contrib are checked by the kernels.
 *
 * nhip_bsr_assemble_dev: d_values[9 * nnzb] (every block row-major), d_grad[3 * n_blocks] (block b: the sum over the
 * contributors of b's diagonal block of row[21..23] for q = 0 and row[24..26] for q = 3) and d_cost[0] = 1/2 the sum of
 * rows[r][27].  ONE pinned summation order for all three: partial l, l = 0 .. 63, adds terms l, l + 64, l + 128, ... one by
 * one starting from +0.0; then partial[l] += partial[l + s] for s = 32, 16, ..., 1; the sum is partial[0].  No atomics: the
 * same input gives the same bits.  A contributor id outside [0, 4 * n_rows) (kind 2048) or a block column outside
 * [0, n_blocks) (kind 4096) is never dereferenced: the block is zero and nhip_dev_status() reports it.  n_rows == 0 gives
 * zeros. */
int nhip_bsr_assemble_dev(const double *d_rows, int32_t n_rows, const int32_t *d_row_ptr, const int32_t *d_col,
                          const int32_t *d_contrib_ptr, const int32_t *d_contrib, int32_t n_blocks, int32_t nnzb,
                          int32_t n_contrib, double *d_values, double *d_grad, double *d_cost, void *stream);

/* What a solve reports (host memory). */
typedef struct {
  int32_t iterations;        /* CG iterations completed */
  int32_t flag;              /* 0 converged, 1 max_iters reached, 2 breakdown */
  double relative_residual;  /* the recursive residual's ||r|| / ||b|| at the end (0 for b = 0) */
} nhip_pcg_stats_t;

/* Solves (H + lambda * diag(diag(H) + diag_floor)) x = -g over the blocks with d_fixed[b] == 0 by preconditioned CG in
 * fp64; rows and columns of fixed blocks are skipped and x is exactly 0 there.  The preconditioner is the inverse of every
 * damped 3 x 3 diagonal block, formed once per solve.  It stops when the recursive residual satisfies
 * ||r||_2 <= tol * ||b||_2 (flag 0), after max_iters iterations (flag 1), or at a breakdown -- p^T A p <= 0 or a
 * non-finite scalar (flag 2; x is the last iterate before it).  b = 0: 0 iterations, x = 0.
 * Two launches per iteration, no grid-wide barrier inside a kernel, no floating-point atomics: the same input gives the same
 * bits.  This is the one call of the library that reads device memory between its launches: once per `check_every`
 * iterations it waits for the stream and reads the end words (launches queued behind the end are no-ops, so x and *stats
 * do not depend on check_every), and once more for *stats -- it returns with the stream drained, and it cannot be captured
 * into a graph.  d_workspace: nhip_bsr_pcg_workspace_bytes(n_blocks, nnzb) bytes, 16-byte aligned.  A block column outside
 * [0, n_blocks) is skipped and reported (kind 4096). */
int64_t nhip_bsr_pcg_workspace_bytes(int32_t n_blocks, int32_t nnzb);
int nhip_bsr_pcg_dev(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const double *d_grad,
                     const uint8_t *d_fixed, int32_t n_blocks, int32_t nnzb, double lambda, double diag_floor, double tol,
                     int32_t max_iters, int32_t check_every, double *d_x, void *d_workspace, int64_t workspace_bytes,
                     nhip_pcg_stats_t *stats, void *stream);

/* K12: columns of the inverse -- n_systems systems on ONE matrix.  System s solves (H + ridge * I) x = e_j, j = d_rhs_index[s]
 * a scalar index in [0, 3 * n_blocks), over the FREE blocks of s: every block with d_fixed[b] == 0 except block d_gauge[s]
 * (-1: none).  ridge >= 0 is added to every diagonal entry; there is no lambda term.  Each system runs nhip_bsr_pcg_dev's
 * algorithm on its own -- x = 0 at the start, the preconditioner the inverse of every ridged diagonal block (zero for a block
 * that is not free), the same end tests and flags, a breakdown before x is touched -- with its own scalars, end words, count
 * and residual; systems end at different iterations and a system that has ended is never written again.  j in a block that
 * is not free: x = 0, 0 iterations, flag 0, residual 0.
 * d_x: 3 * n_blocks * n_systems doubles, SYSTEM-MINOR -- element e of system s at d_x[e * n_systems + s]; exactly 0 on the
 * blocks that are not free.  stats: n_systems entries in host memory.
 * Two launches per iteration serve every system (a stored block is read once per 64 systems).  No floating-point atomics;
 * every dot product is summed in an order that depends on n_blocks alone: the bits of a system's x, its count, flag and
 * residual are the same in every run and do NOT depend on n_systems, on the system's place in the batch or on the other
 * systems of the batch -- a caller may split a list into chunks freely.  Like nhip_bsr_pcg_dev the call reads device memory
 * between its launches (one word per `check_every` iterations: the number of systems still running; x and stats do not depend
 * on check_every), returns with the stream drained and cannot be captured into a graph.
 * A d_gauge[s] outside [-1, n_blocks) or a d_rhs_index[s] outside [0, 3 * n_blocks) is never used as an index: that system is
 * x = 0, 0 iterations, flag 2, and nhip_dev_status() reports it (kind 8192, index = s).  A block column outside [0, n_blocks)
 * is skipped and reported (kind 4096).  Rows of any length are taken by one lane per system: a free block row of L stored
 * blocks costs its wave L dependent steps.  d_workspace: nhip_bsr_pcg_columns_workspace_bytes(...) bytes, 16-byte aligned.
 * 3 * n_blocks * n_systems must not exceed 2^31 - 1.  n_systems == 0 or n_blocks == 0: NHIP_OK, nothing launched. */
int64_t nhip_bsr_pcg_columns_workspace_bytes(int32_t n_blocks, int32_t nnzb, int32_t n_systems);
int nhip_bsr_pcg_columns_dev(const int32_t *d_row_ptr, const int32_t *d_col, const double *d_values, const uint8_t *d_fixed,
                             int32_t n_blocks, int32_t nnzb, const int32_t *d_gauge, const int32_t *d_rhs_index,
                             int32_t n_systems, double ridge, double tol, int32_t max_iters, int32_t check_every, double *d_x,
                             void *d_workspace, int64_t workspace_bytes, nhip_pcg_stats_t *stats, void *stream);

/* K5: correspondence search, the step that feeds K4 (Solver::GetPointToPointMatching,
 * src/optimization/solver.cc:132-172; KDTree::FindNearestPoint, src/util/kdtree.cc:253-305).
 * Block b pairs source scan d_block_src[b] with target scan d_block_tgt[b]: every source point is
 * moved into the target frame by inverse(T_target) * T_source (float affines of the poses, see
 * nhip_pose_affines), matched with its nearest target point and kept if the distance is below
 * outlier_threshold (default_config.lua:66).  d_normals: one float2 per point of d_xy (the
 * reference reads normals from its trees, solver.cc:67-78).  Rows (8 floats: source point, target
 * point, source normal, target normal) are written in source order at
 * d_corr_padded + 8*d_cap_offsets[b] (capacity = source points of block b); d_counts[b] rows are
 * valid.  nhip_corr_compact_dev packs them into the contiguous layout nhip_resid_lidar_dev takes
 * (d_block_offsets: n_blocks+1, d_corr: 8 floats/row, d_corr_block: block id per row). */
int nhip_pose_affines(const double *poses, int32_t n, float *out /* 4n: cos sin x y */);
int nhip_corr_search_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                         const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                         const float *d_pose_aff, float outlier_threshold,
                         const int64_t *d_cap_offsets, float *d_corr_padded, int32_t *d_counts,
                         void *stream);
/* The same search with the normal gate of Solver::GetPointToNormalMatching /
 * FindClosestPointWithSimilarNormal (solver.cc:177-260; defined but not called at this commit): among
 * the target points within outlier_threshold, the nearest whose normal satisfies
 * |n_target . n_source| > min_abs_cosine (NormalsSimilar, math_util.h:46-49; the reference passes
 * cos(20 deg)); n_source is the source point's normal in the SOURCE frame, as in the reference.
 * Exactly equal distances go to the lowest target index (the reference's std::sort leaves that open). */
int nhip_corr_search_normals_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                                 const int32_t *d_block_src, const int32_t *d_block_tgt, int32_t n_blocks,
                                 const float *d_pose_aff, float outlier_threshold, float min_abs_cosine,
                                 const int64_t *d_cap_offsets, float *d_corr_padded, int32_t *d_counts,
                                 void *stream);
int nhip_corr_compact_dev(const float *d_corr_padded, const int64_t *d_cap_offsets,
                          const int32_t *d_counts, int32_t n_blocks, int32_t *d_block_offsets,
                          float *d_corr, int32_t *d_corr_block, void *stream);

/* Loop-closure candidate gating, the step before the matcher.
 * nhip_lc_scatter_scores*: LCCandidateFilter's ComputeScatterMatrixScore (lc_candidate_filter.cc:22-51) for every
 * scan: float mean and scatter matrix summed in point order (the reference's float sums, bit for bit), min / max
 * eigenvalue (closed form in double); one double per scan, NaN for an empty scan.
 * nhip_lc_pair_gate*: for n candidate nodes (indices into poses[n_poses][3]), flags[i*n + j] = 1 iff candidates i and
 * j are different nodes more than min_separation apart in index whose translations (as Vector2f) are closer than
 * max_range -- a geometric stand-in for LCMatcher's per-pair ceres::Covariance test (lc_matcher.cc:28-74).
 * nhip_lc_chi_square_gate*: LCMatcher's own test given the covariance blocks -- for pair i, d = Vector2f(pose of
 * pair_tgt[i]) - Vector2f(pose of pair_src[i]), scores[i] = d^T cov_i^-1 d evaluated in float as ChiSquareScore does
 * (lc_matcher.cc:50-57; cov[i] = the Matrix2f of GetCovarianceMatrix, :28-46, row major m00 m01 m10 m11), widened to
 * double; flags[i] = 1 iff pair_src[i] != pair_tgt[i] and scores[i] < max_score (GetPossibleMatches, :59-74, which
 * passes 5000.0).  A singular block gives inf / NaN scores as the reference's inverse() does, and flag 0 for NaN.
 * d_cov must be 16-byte aligned.  The covariance solve itself (ceres::Covariance) stays with the host's solver. */
int nhip_lc_scatter_scores_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, double *d_scores,
                               void *stream);
int nhip_lc_pair_gate_dev(const double *d_poses, int32_t n_poses, const int32_t *d_candidates, int32_t n_candidates,
                          double max_range, int32_t min_separation, uint8_t *d_flags, void *stream);
int nhip_lc_chi_square_gate_dev(const double *d_poses, int32_t n_poses, const int32_t *d_pair_src, const int32_t *d_pair_tgt,
                                const float *d_cov, int32_t n_pairs, double max_score, double *d_scores,
                                uint8_t *d_flags, void *stream);

/* Scan features: the planar and the edge points Solver::SolveSLAM's FEATURE mode builds its residual blocks from
 * (solver.cc:297-318) -- FeatureExtractor(pointcloud, 0.008, 2.0, 10, 10, 20, 10) of every scan at once
 * (src/util/slam_types.h:66-69, src/input/feature_extracter.{h,cc}; the spec, quirks included: DESIGN.md section 3,
 * "Scan features").  Per point a smoothness score from its index neighbours (min / max eigenvalue of their float scatter
 * matrix, closed form in double as nhip_lc_scatter_scores; NaN = the point has no score); the planar points are the
 * greedy walk over ascending (score, index) that accepts what is not above `threshold` and not closer than
 * `distance_threshold` to an accepted point, up to max_planar; the edge points the same walk over descending (score, index),
 * not below `threshold`, up to max_edge.  Accepted ranges: neighbors_per_side 1..NHIP_FEATURE_MAX, min_neighbors
 * 1..2 * neighbors_per_side - 1, max_planar and max_edge 1..NHIP_FEATURE_MAX, threshold finite, the two distances finite
 * and >= 0; anything else is NHIP_ERR_ARG before anything is launched. */
#define NHIP_FEATURE_MAX 64
typedef struct nhip_feature_spec {
  double threshold;             /* planar: score <= threshold; edge: score >= threshold (0.008) */
  double distance_threshold;    /* accepted points of one set are at least this far apart [m] (2.0) */
  double max_neighbor_distance; /* a LEFT neighbour further away than this is dropped (feature_extracter.h:28: 0.8) */
  int32_t neighbors_per_side;   /* P: left neighbours i - P .. i - 1 (none for i < P), right i + 1 .. i + P - 1 (10) */
  int32_t min_neighbors;        /* fewer neighbours: the point has no score (10) */
  int32_t max_planar;           /* (20) */
  int32_t max_edge;             /* (10) */
} nhip_feature_spec_t;
/* the reference's values, as listed above; pure host */
int nhip_feature_spec_default(nhip_feature_spec_t *out);
/* d_xy, d_offsets: the scans as everywhere (d_offsets: n_scans + 1 entries).  Outputs, per scan s, scan-local indices IN
 * ACCEPTANCE ORDER (the order of planar_points / edge_points, hence of the rows of the residual blocks), -1 padded:
 * d_planar_idx[s][max_planar], d_planar_count[s], d_edge_idx[s][max_edge], d_edge_count[s]; d_scores (may be NULL): one
 * double per point of d_xy, NaN where a point has no score.  Scans of any length, empty ones included. */
int nhip_features_extract_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_feature_spec_t *spec,
                              int32_t *d_planar_idx, int32_t *d_planar_count, int32_t *d_edge_idx, int32_t *d_edge_count,
                              double *d_scores, void *stream);
/* Gathers the points d_idx[s][0 .. d_count[s]) (rows of `cap` entries, 1 <= cap <= NHIP_FEATURE_MAX) of every scan, and
 * their normals if d_normals is not NULL (then d_normals_out must not be either: a feature point keeps its own normal, as
 * GetPointNormal's lookup gives it, solver.cc:67-77, 164-166), into packed clouds: d_xy_out / d_normals_out (room for
 * n_scans * cap points) and d_offsets_out[n_scans + 1] -- the layout nhip_corr_search_dev takes.  d_idx and d_count are
 * checked by the kernels ("Ids in device memory" above): a count outside [0, cap] makes its scan contribute nothing, an
 * index outside its scan is left out, and nhip_dev_status() reports either. */
int nhip_features_pack_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                           const int32_t *d_idx, const int32_t *d_count, int32_t cap, float *d_xy_out,
                           float *d_normals_out, int32_t *d_offsets_out, void *stream);

/* Scan normals: NormalComputation::GetNormals (src/input/normal_computation.{h,cc}) of every scan at once -- the one input
 * of the correspondence search, the normal residual and the feature clouds that a real bag does not bring.  The randomised
 * Hough estimate of the reference, stated deterministically (the spec, and every departure from the reference: DESIGN.md
 * section 3, "Scan normals").  Per point i (scan-local index) of a scan:
 *   neighbours  the points j of the same scan, i included, in scan order, with sqrtf(dx * dx + dy * dy) < (float)r (float
 *               operations rounded one by one, strict); r = neighborhood_size, and while there are fewer than two and fewer
 *               than max_growth_steps growths were made, r += neighborhood_step_size (double) and the list is rebuilt.  Still
 *               fewer than two: the normal is (0, 0).  A non-finite point has no neighbours and is nobody's.
 *   samples     limit = min(m (m - 1), (size_t)(1 / (2.0 * mean_distance * mean_distance))) ordered pairs (a, b) of neighbour
 *               ranks, m the neighbour count; redrawn while a == b or the pair was taken.  The generator is counter based and
 *               keyed on (seed, i) alone: h(x) = lowbias32 (x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b,
 *               x ^= x >> 16), s0 = h(seed ^ h(i)), draw k = h(s0 + k), k = 0, 1, ... (a, then b, two per attempt), rank =
 *               ((uint64_t)draw * m) >> 32.  A scan's normals do not depend on where it sits in a batch.
 *   vote        n = (-dy, dx) / sqrtf(dx * dx + dy * dy) of p_b - p_a in float, negated if n.y < 0 or (n.y == 0 and n.x < 0);
 *               angle = acos(clamp((double)n.x, -1, 1)); bin = floor(angle / (2 pi / bin_number) + 0.5).  A pair of zero (or
 *               not finite) length casts no vote but counts as a sample.  The two leading bins follow
 *               CircularHoughAccumulator::AddVote.
 *   stop        after a vote, if votes(most) / B - votes(second) / B >= 2.0 * sqrt(1.0 / B), B = bin_number, the quotients
 *               INTEGER divisions (BinMean); otherwise the sample is counted, up to limit.
 *   result      a = (sum of the winning bin's angles in vote order) / votes(most) in double; ((float)cos(a), (float)sin(a));
 *               no vote at all: (0, 0).
 * Accepted ranges: the three lengths finite and > 0, bin_number 2..NHIP_NORMALS_MAX_BINS, the sample limit's second term
 * 1..NHIP_NORMALS_MAX_SAMPLES, max_growth_steps 0..1024, n_scans >= 0; anything else is NHIP_ERR_ARG before anything is
 * launched, with or without a device. */
#define NHIP_NORMALS_MAX_BINS 64
#define NHIP_NORMALS_MAX_SAMPLES 128
typedef struct nhip_normals_spec {
  double neighborhood_size;      /* starting radius [m] (nc_neighborhood_size, 0.15) */
  double neighborhood_step_size; /* radius growth per step [m] (nc_neighborhood_step_size, 0.1) */
  double mean_distance;          /* sets the sample limit (nc_mean_distance, 0.1: 49 samples) */
  int32_t bin_number;            /* Hough bins around the circle (nc_bin_number, 32) */
  int32_t max_growth_steps;      /* cap on the radius growth (32) */
  uint32_t seed;                 /* of the generator (1) */
  int32_t flags;                 /* 0 */
} nhip_normals_spec_t;
/* config/default_config.lua's nc_* values, as listed above; pure host */
int nhip_normals_spec_default(nhip_normals_spec_t *out);
/* d_xy, d_offsets: the scans as everywhere (d_offsets: n_scans + 1 entries); scans of any length, empty ones included.
 * d_normals: 2 floats per point of d_xy.  d_info (may be NULL): 4 int32 per point -- {neighbour count, growth steps made,
 * winning bin (-1: none), votes in it | samples counted << 16}.  The offsets are read by the kernels: a scan whose first
 * offset is negative or whose end lies before its start is treated as empty -- nothing is written for it -- and
 * nhip_dev_status() reports it (kind 256).  Scans of at most NHIP_SHORT_SCAN_POINTS points and specs whose sample limit is
 * at most 64 take the fast form; everything else a slow one with the same results. */
int nhip_normals_estimate_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_normals_spec_t *spec,
                              float *d_normals, int32_t *d_info, void *stream);

/* K13: MAP VECTORISATION -- Solver::Vectorize (solver.cc:581-624): every scan at its pose, merged, reduced to wall segments
 * x1 y1 x2 y2 ("Map vectorisation"; tests/vectorize_reference.py restates it in numpy).  Build-defined:
 * an exhaustive, deterministic Hough transform over the occupied cells of a world raster with greedy peak extraction; all
 * integer after the point transform.
 *   points   scan i's affine (c, s, tx, ty) = ((float)cos, (float)sin, (float)x, (float)y) of its pose (nhip_map_pose_affines);
 *            x' = ((c x) + ((-s) y)) + tx, y' = ((s x) + (c y)) + ty in float, every operation rounded on its own.
 *   raster   cell (floor((double)x' / res) - cell_x0, floor((double)y' / res) - cell_y0); a point that is not finite, whose
 *            floor is not below 2^63 in magnitude or whose cell is outside width x height is dropped; counts[height][width].
 *   cells    those with counts >= min_hits, row-major (cy, then cx), as (cx, cy) int32 pairs: M cells, all live.
 *   tables   C[t] = lrint(2^14 cos(pi t / n_theta)), S[t] = lrint(2^14 sin(pi t / n_theta)) (nhip_vectorize_tables);
 *            rho_q = cx C[t] + cy S[t] + (width << 14), bin b = rho_q >> 14, n_rho = 2 width + height + 1 bins;
 *            a_q = cy C[t] - cx S[t] + (width << 14), along-line bin a = a_q >> 14 (the floor: a_q is negative for some
 *            cells where C[t] < 0), -height <= a < width + height.
 *   votes    votes[t][b]: the live cells in that bin.
 *   a round  1. the peak: the largest votes, ties to the smallest t n_rho + b.  Below min_votes: the call ends, flag 0.
 *               Otherwise, if max_rounds rounds were made already: the call ends, flag 1.
 *            2. the band: live cells with |rho_q - ((b << 14) + (1 << 13))| <= lrint(band 2^14); the set of their bins a.
 *            3. runs: maximal ascending sequences of set bins whose neighbours differ by at most max_gap + 1; KEPT iff
 *               a_hi - a_lo + 1 >= min_length; taken in ascending a.
 *            4. no run kept: every band cell is retired (dies, its n_theta votes are subtracted, no record).  Kept runs that
 *               do not fit into what is left of max_segments: nothing is committed, the call ends, flag 2.  Otherwise every
 *               band cell inside a kept run dies, its votes are subtracted and it adds 1, cx, cy, cx^2, cx cy, cy^2 to its
 *               run's record; band cells outside the kept runs stay live.  `rounds` counts the rounds that retired or committed.
 *   record   10 int64: {t, b, a_lo, a_hi, n, sum x, sum y, sum xx, sum xy, sum yy}.
 *   stats    8 int32: {M, segments, rounds, flag, cells emitted, cells retired, n_rho, 0}.  More than max_cells cells: flag 3,
 *            M is the count needed, nothing is vectorised and nothing is written past the buffers.
 *   lines    nhip_vectorize_endpoints (pure host, double): m = (sum x / n, sum y / n); cxx = sum xx - sum x mx, cxy = sum xy -
 *            sum x my, cyy = sum yy - sum y my; phi = 0.5 atan2(2 cxy, cxx - cyy), d = (cos phi, sin phi).  The ends are the
 *            points (rho c - alpha s, rho s + alpha c) of the Hough line, c = C[t] / 2^14, s = S[t] / 2^14, rho = ((b << 14)
 *            + 2^13 - (width << 14)) / 2^14, alpha = a - width for a = a_lo and a = a_hi + 1, each projected onto the line
 *            through m along d: q = m + ((p - m) . d) d; metres ((cell_x0 + q.x) + 0.5) res, ((cell_y0 + q.y) + 0.5) res, rounded to
 *            float.  Every operation rounded on its own.
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): res finite and > 0;
 * width, height 1..16384; min_hits 1..2^30; n_theta 2..1024; min_votes >= 1; band finite, 0.5..65536 (cells); max_gap >= 0;
 * min_length >= 1; max_segments >= 0; max_cells >= 0; max_rounds >= 0; check_every >= 1. */
typedef struct nhip_vectorize_spec {
  double res;           /* metres per cell (0.05) */
  double band;          /* half width of a line's band, in cells (1.5) */
  int32_t cell_x0;      /* the window's first cell, in world cells (the caller's: hostside.map_window) */
  int32_t cell_y0;
  int32_t width;        /* cells */
  int32_t height;
  int32_t min_hits;     /* points that make a cell occupied (2) */
  int32_t n_theta;      /* rows of the accumulator: directions over half a turn (360) */
  int32_t min_votes;    /* the smallest peak that still makes a round (20) */
  int32_t max_gap;      /* empty along-line bins a run may bridge (4) */
  int32_t min_length;   /* along-line bins a kept run spans (10) */
  int32_t max_segments; /* capacity of the records (4096) */
  int32_t flags;        /* 0 */
  int32_t reserved;     /* 0 */
} nhip_vectorize_spec_t;
/* byte offsets of the planes a caller may read out of a workspace it owns (all 256-byte aligned, in this order), and its size */
typedef struct nhip_vectorize_layout {
  int64_t counts_offset; /* int32 [height][width] */
  int64_t cells_offset;  /* int32 (cx, cy) pairs, max_cells of them */
  int64_t votes_offset;  /* int32 [n_theta][n_rho]: after the call, the votes of the cells still live */
  int64_t live_offset;   /* one byte per cell: 1 live, 0 dead */
  int64_t bytes;         /* = nhip_vectorize_workspace_bytes */
  int32_t n_rho;         /* 2 width + height + 1 */
  int32_t n_along;       /* width + 2 height + 1: along-line bins, bin a at index a + height */
} nhip_vectorize_layout_t;
/* the defaults of the table above; the window (cell_x0, cell_y0, width, height) is 0 and is the caller's to set; pure host */
int nhip_vectorize_spec_default(nhip_vectorize_spec_t *out);
/* C[n_theta], S[n_theta]; pure host */
int nhip_vectorize_tables(const nhip_vectorize_spec_t *spec, int32_t *c_table, int32_t *s_table);
/* 4 floats per pose (x, y, theta: 3 doubles): ((float)cos theta, (float)sin theta, (float)x, (float)y), the cast of
 * TransformPointcloud (slam_util.h:55-63); pure host */
int nhip_map_pose_affines(const double *poses, int32_t n_poses, float *out);
/* bytes of the workspace for up to max_cells cells (-1: a bad spec, message in nhip_last_error); pure host */
int64_t nhip_vectorize_workspace_bytes(const nhip_vectorize_spec_t *spec, int32_t max_cells);
int nhip_vectorize_workspace_layout(const nhip_vectorize_spec_t *spec, int32_t max_cells, nhip_vectorize_layout_t *out);
/* The whole step on the caller's buffers and stream; never allocates.  d_affines: 4 floats per scan.  d_records: room for
 * max_segments records (may be NULL if that is 0); d_stats: 8 int32.  The host looks at the device once per check_every
 * rounds (one word) and once at the end: the call returns with the stream drained, and records, stats and planes do not
 * depend on check_every.  The offsets are read by the kernels: a scan whose first offset is negative or whose end lies
 * before its start is treated as empty and nhip_dev_status() reports it (kind 16384). */
int nhip_vectorize_dev(const float *d_xy, const int32_t *d_offsets, const float *d_affines, int32_t n_scans,
                       const nhip_vectorize_spec_t *spec, int32_t max_cells, int32_t max_rounds, int32_t check_every,
                       int64_t *d_records, int32_t *d_stats, void *d_workspace, int64_t workspace_bytes, void *stream);
/* records (n x 10 int64) -> lines (n x 4 floats: x1 y1 x2 y2, what WriteMapLines takes); pure host */
int nhip_vectorize_endpoints(const nhip_vectorize_spec_t *spec, const int64_t *records, int32_t n, float *lines);

/* K14: OCCUPANCY GRID -- the occupied / free / unknown raster of every scan at its pose, free space ray-traced from the
 * sensor to every return ("Occupancy grid"; tests/occupancy_reference.py restates it in numpy).
 * Build-defined and deterministic; all integer after the cells.
 *   points   as K13's: scan i's affine (nhip_map_pose_affines), x' = ((c x) + ((-s) y)) + tx, y' likewise, in float.  The
 *            ray origin of scan i is (tx, ty).
 *   cells    floor((double)v / res) of the origin and of every end point.  A scan whose origin is not finite or has a floor
 *            of magnitude >= 2^62 is DROPPED; a point that is not finite or has such a floor is DROPPED.  d = end - origin
 *            per axis (in double, from the two floors); |dx| or |dy| > max_ray_cells: the beam is LONG and adds nothing.
 *   ray      n = max(|dx|, |dy|); the free cells of a beam are origin + (rdiv(k dx, n), rdiv(k dy, n)) for k = 0 .. n - 1,
 *            rdiv(a, n) = floor((2 a + n) / (2 n)) (a floor division: nearest, halves up, on both signs).  n = 0: none.
 *   a scan   H = the end cells of its kept beams; F = the free cells of its kept beams minus H.  hits[cy][cx] counts the
 *            scans with the cell in H, misses[cy][cx] those with it in F: one observation per scan and cell, inside the
 *            window (cell_x0, cell_y0, width, height) -- rays that start or end outside it still mark what they cross.
 *   grid     int8 [height][width], ROS OccupancyGrid values; obs = hits + misses (int64): obs < min_obs: -1; else
 *            1000 hits >= occ_permille obs: 100; else 1000 hits <= free_permille obs: 0; else -1.
 *   planes   without NHIP_OCC_ACCUMULATE the call clears hits and misses first (in-stream); with it the call adds onto what
 *            they hold.  The grid is classified from the planes as they stand after the call.
 *   stats    8 int64: {scans traced, scans dropped (or offsets that are not a scan), beams traced, beams long, points dropped}
 *            of this call (the points of a dropped scan are counted nowhere), {cells occupied, free, unknown} of the grid.
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): res finite and > 0;
 * width, height 1..16384; max_ray_cells 1..4096; min_obs 1..2^30; occ_permille 1..1000; free_permille 0..occ_permille - 1;
 * flags 0 or NHIP_OCC_ACCUMULATE; reserved 0; n_scans >= 0. */
#define NHIP_OCC_ACCUMULATE 1
typedef struct nhip_occupancy_spec {
  double res;            /* metres per cell (0.05) */
  int32_t cell_x0;       /* the window's first cell, in world cells (the caller's: hostside.map_window) */
  int32_t cell_y0;
  int32_t width;         /* cells */
  int32_t height;
  int32_t max_ray_cells; /* the longest beam traced, in cells per axis (640: 30 m and the discretisation) */
  int32_t min_obs;       /* observations that make a cell known (1) */
  int32_t occ_permille;  /* hits per 1000 observations from which a cell is occupied (650: map_server's 0.65) */
  int32_t free_permille; /* ... up to which it is free (196: map_server's 0.196) */
  int32_t flags;         /* 0, or NHIP_OCC_ACCUMULATE */
  int32_t reserved;      /* 0 */
} nhip_occupancy_spec_t;
/* the defaults of the table above; the window is 0 and is the caller's to set; pure host */
int nhip_occupancy_spec_default(nhip_occupancy_spec_t *out);
/* The whole step on the caller's buffers and stream; never allocates, needs no workspace, enqueues and returns without
 * waiting.  d_affines: 4 floats per scan.  d_hits, d_misses: int32 [height][width], 16-byte aligned; d_grid: int8
 * [height][width], 4-byte aligned; d_stats: 8 int64.  n_scans = 0 is a call: the planes cleared (without the flag), the grid
 * classified.  The offsets are read by the kernels: a scan whose first offset is negative or whose end lies before its start
 * is treated as empty, counted as dropped, and nhip_dev_status() reports it (kind 16384). */
int nhip_occupancy_dev(const float *d_xy, const int32_t *d_offsets, const float *d_affines, int32_t n_scans,
                       const nhip_occupancy_spec_t *spec, int32_t *d_hits, int32_t *d_misses, int8_t *d_grid, int64_t *d_stats,
                       void *stream);

/* K19: TRANSIENT RETURNS -- every return of every scan classified by the two planes of the occupancy grid under it, and the
 * returns that are not transient packed into clouds of the layout every other entry point takes (DESIGN.md section 3,
 * "Transient returns"; tests/transient_reference.py and hostside.transient_filter restate it in numpy).  A wall cell is hit
 * by many scans and seen through by few; a cell where someone stood for one scan is hit once and seen through by every later
 * scan.  Build-defined and deterministic; all integer after the cells; the planes are read as they are and never written.
 *   cell     as K14's end cells: scan i's affine (nhip_map_pose_affines) in float, floor((double)v / res) per axis.
 *   label 3  INVALID: the point or its world point is not finite, or a floor has magnitude >= 2^62.  No scan is dropped as a
 *            whole: an affine that is not finite makes every point of its scan invalid.  A point of the cloud that belongs to
 *            no scan (or to one whose offsets are not a scan) keeps this label too.
 *   label 2  UNOBSERVED: the cell lies outside the window (cell_x0, cell_y0, width, height); the test is made in int64.
 *   counts   S = the sum of hits over the cells of the (2 support_radius + 1)^2 neighbourhood that lie inside the window;
 *            m = misses at the point's own cell; both int64.
 *   label 1  TRANSIENT: m >= min_through and 1000 S <= transient_permille (S + m); equality on either side counts.
 *   label 0  STATIC: everything else.
 *   kept     labels 0 and 2, in the layout of the input: out_offsets (n_scans + 1), out_xy (the kept points in the scan frame,
 *            bit copies, in their order inside each scan, scans in order), out_index (the index of each kept point in the
 *            input cloud, so that normals or intensities can be gathered alongside).
 *   stats    8 int64: {points static, transient, unobserved, invalid, scans processed, scans whose offsets are not a scan,
 *            scans that had points and kept none, 0}.
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): res finite and > 0;
 * width, height 1..16384; support_radius 0..4; min_through 1..2^30; transient_permille 0..1000; flags 0; reserved 0;
 * n_scans >= 0; n_points >= 0. */
typedef struct nhip_transient_spec {
  double res;                 /* metres per cell (0.05): the occupancy spec's */
  int32_t cell_x0;            /* the window of the planes: the occupancy spec's */
  int32_t cell_y0;
  int32_t width;
  int32_t height;
  int32_t support_radius;     /* hits are summed over (2 r + 1)^2 cells (1): a grazing beam ends one cell along its wall */
  int32_t min_through;        /* scans that must have seen through the cell (2) */
  int32_t transient_permille; /* hits per 1000 observations up to which the return is transient (500) */
  int32_t flags;              /* 0 */
  int32_t reserved;           /* 0 */
} nhip_transient_spec_t;
/* the defaults of the table above; the window is 0 and is the caller's to set; pure host */
int nhip_transient_spec_default(nhip_transient_spec_t *out);
/* The whole step on the caller's buffers and stream; never allocates, needs no workspace, enqueues and returns without
 * waiting -- in-stream after nhip_occupancy_dev it reads the planes that call wrote, with no synchronisation between.
 * n_points: the capacity of the clouds, input and output alike (d_xy, d_out_xy: 2 floats per point, 8-byte aligned;
 * d_labels: a byte per point; d_out_index: an int32 per point).  d_affines: 4 floats per scan.  d_hits, d_misses: int32
 * [height][width].  d_out_offsets: n_scans + 1 int32.  d_stats: 8 int64.  n_scans = 0 is a call: out_offsets[0] = 0, the
 * stats zero, every label 3.  The offsets are read by the kernels: a scan whose first offset is negative, whose end lies
 * before its start or whose end lies beyond n_points is treated as empty, counted in the stats, and nhip_dev_status() reports
 * the first such scan in scan order (kind 16384, the offset at fault and its index in d_offsets); the other scans are not
 * affected.  Scans are expected not to overlap in the cloud; if they do, the kept points are cut at n_points, the capacity of
 * the outputs, and a shared point carries the label of whichever scan wrote last. */
int nhip_transient_filter_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, int32_t n_points, const float *d_affines,
                              const nhip_transient_spec_t *spec, const int32_t *d_hits, const int32_t *d_misses, uint8_t *d_labels,
                              float *d_out_xy, int32_t *d_out_offsets, int32_t *d_out_index, int64_t *d_stats, void *stream);

/* K20: MAP WINDOWS -- the target clouds of scans that are localised in a finished occupancy grid: for every query the crop of
 * the grid's occupied cells around the world cell of its prior pose, as a cloud of the layout every other entry point takes, so
 * that nhip_grid_build_dev builds the query's table from it and nhip_csm_match_dev matches the scan against it (DESIGN.md
 * section 3, "Map windows"; tests/localize_reference.py and hostside.map_cells / map_windows restate it).  Build-defined and
 * deterministic: no atomics on any output, the same input gives the same bits.
 *   occupied a cell of the int8 grid [height][width] whose value >= occ_min, a signed compare (-1, unknown, never is).
 *   cells    row_ptr[height + 1] and cols[n_occ], int32: the local x indices of the occupied cells of map row y are
 *            cols[row_ptr[y] .. row_ptr[y + 1]), ascending.  More occupied cells than max_cells: nothing is packed, EVERY
 *            entry of row_ptr is 0 (a gather over the result sees an empty map) and nhip_dev_status() reports it (kind 524288,
 *            value: the cells needed).
 *   origin   of a query: the world cell of its prior, (floor(x / res), floor(y / res)) in double (nhip_mapwin_origins); its
 *            theta0 is the prior's heading.
 *   window   the target frame is the WORLD frame moved to the lower-left corner of the origin cell (ox, oy); it is not
 *            rotated and nothing is resampled.  World cell (wx, wy) belongs to the window iff kx = wx - ox and ky = wy - oy
 *            both lie in [-side/2, side - side/2 - 1] (tested in int64); its point is x = (float)(((double)kx + 0.5) * res),
 *            y likewise: one double multiply, one rounding to float.  The table build's side/2 + floor((double)v / res)
 *            returns the cell side/2 + k for it.  A window's points are in row order (y ascending, then x ascending), windows
 *            in query order: out_xy, out_offsets[n_queries + 1].  A window that misses the map is an empty scan.
 *   capacity more window points than out_capacity (or than 2^31 - 1): nothing is stored, every entry of out_offsets is 0 and
 *            nhip_dev_status() reports it (kind 1048576, value: the points needed).
 *   stats    8 int64: {occupied cells of the map (also when they were not packed), queries, points stored, empty windows,
 *            largest window, 1 if the cells did not fit, 1 if the points did not fit, 0}.  nhip_mapwin_cells_dev writes words 0
 *            and 5 and clears the others; nhip_mapwin_gather_dev writes words 1 - 4 and 6 and leaves the others as they are: one
 *            block given to both calls in turn holds the whole record.
 *   pose     from a record of the matcher with pair_origin 0 (host, double): x = (ox + ix - (nx - 1) / 2) res, y likewise,
 *            theta = angle_mod(theta0 + (itheta - (n_theta - 1) / 2) theta_step); a rejected record gives NaN
 *            (nautilus_amd/localize.py: compose).
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): res finite and > 0;
 * width, height 1..16384; side 2..8192; occ_min 1..100; flags 0; reserved 0; max_cells >= 0; n_queries >= 0;
 * out_capacity >= 0. */
typedef struct nhip_mapwin_spec {
  double res;        /* metres per cell: the occupancy spec's, and the grid spec's of the tables */
  int32_t cell_x0;   /* the map's window: the occupancy spec's */
  int32_t cell_y0;
  int32_t width;
  int32_t height;
  int32_t side;      /* the target table's side in cells: nhip_grid_layout(spec).side */
  int32_t occ_min;   /* a cell is occupied iff its value >= occ_min (100) */
  int32_t flags;     /* 0 */
  int32_t reserved;  /* 0 */
} nhip_mapwin_spec_t;
/* the defaults of the table above; the map's window and side are 0 and are the caller's to set; pure host */
int nhip_mapwin_spec_default(nhip_mapwin_spec_t *out);
/* origins (2 int32 per query: ox, oy) and theta0 (a double per query, may be NULL) of n priors (3 doubles each: x, y, heading);
 * pure host.  A pose that is not finite or whose floor has magnitude >= 2^30 is NHIP_ERR_ARG, the message names its index. */
int nhip_mapwin_origins(const double *poses, int32_t n, double res, int32_t *origins, double *theta0);
/* bytes of the gather's workspace for n_queries queries (the per-window counts; > 0 for every n_queries >= 0, else 0); pure host */
int64_t nhip_mapwin_workspace_bytes(int32_t n_queries);
/* The occupied cells of the grid, on the caller's buffers and stream; never allocates, enqueues and returns without waiting.
 * d_grid: int8 [height][width], any alignment; d_row_ptr: height + 1 int32; d_cols: max_cells int32 (may be NULL with
 * max_cells 0); d_stats: 8 int64, 8-byte aligned. */
int nhip_mapwin_cells_dev(const int8_t *d_grid, const nhip_mapwin_spec_t *spec, int32_t max_cells, int32_t *d_row_ptr,
                          int32_t *d_cols, int64_t *d_stats, void *stream);
/* The windows of n_queries origins (d_origins: 2 int32 each, any values) from the cells nhip_mapwin_cells_dev wrote (d_cols
 * holds d_row_ptr[height] entries), on the caller's buffers and stream; never allocates, enqueues and returns without waiting.
 * d_out_xy: out_capacity points of 2 floats, 8-byte aligned (may be NULL with out_capacity 0); d_out_offsets: n_queries + 1
 * int32; d_stats: 8 int64, 8-byte aligned; d_workspace: nhip_mapwin_workspace_bytes(n_queries) bytes, 4-byte aligned.  A window
 * costs `side` row lookups and its own output: the map is not read per query.  The entries of d_row_ptr are checked before
 * they become addresses: a row whose range is not inside [0, d_row_ptr[height]] is an empty row and nhip_dev_status() reports
 * it (kind 524288); the entries of d_cols are only compared and converted, never addresses.  n_queries = 0 is a call:
 * out_offsets[0] = 0. */
int nhip_mapwin_gather_dev(const int32_t *d_row_ptr, const int32_t *d_cols, const nhip_mapwin_spec_t *spec, const int32_t *d_origins,
                           int32_t n_queries, float *d_out_xy, int64_t out_capacity, int32_t *d_out_offsets, int64_t *d_stats,
                           void *d_workspace, int64_t workspace_bytes, void *stream);

/* K21: RANGE SIGNATURES -- global localisation: priors for scans that have NO prior, from the finished occupancy grid alone
 * ("Range signatures"; tests/rangesig_reference.py and hostside.range_signatures / scan_signatures /
 * signature_candidates restate it).  Every free lattice cell of the map (an anchor) gets 64 bytes, the quantised distance to
 * the nearest wall in each of 64 sectors, ray-cast in the grid; every scan the same 64 bytes from its returns; a scan is placed
 * at an anchor under the best of the 64 rotations by the sum of absolute differences of the bytes.  Integer after the float
 * comparisons of a scan's points; no output depends on an order: the same input gives the same bits.
 *   lattice  node (i, j) is the local cell (i stride + stride/2, j stride + stride/2), if that lies in the window; it is an
 *            ANCHOR iff the cell's value is in [0, free_max].  The anchor list holds the anchors in row-major order (j, then
 *            i), int32[4] = {cx, cy, i, j} each.  Of more anchors than max_anchors the first max_anchors are written;
 *            nhip_dev_status() reports it (kind 2097152, value: the anchors found, index = max_anchors).  Entries of the list
 *            behind the anchors found are four -1; an entry whose cell is not in the window is no anchor to the later calls:
 *            its signature is 64 x 255 and it is in no record.
 *   rays     nhip_rangesig_tables: ray t = 0 .. 64 m - 1 of an anchor points at phi = (t + 1/2) (2 pi / 64) / m and ends
 *            (dx, dy) = (lrint(L cos phi), lrint(L sin phi)) cells away, n = max(|dx|, |dy|); step k = 1 .. n is the cell
 *            anchor + (rdiv(k dx, n), rdiv(k dy, n)), rdiv(a, n) = floor((2 a + n) / (2 n)): the occupancy grid's ray.  The ray
 *            ends at the first step whose cell is outside the window (255), unknown (value < 0: 255) or a wall (value >=
 *            occ_min: min(254, (k scale) >> 16), scale = lrint(2^16 sqrt(dx dx + dy dy) res / (n unit))); no end by n: 255.
 *            With NHIP_RANGESIG_UNKNOWN_STOPS in flags an unknown cell gives its range as a wall does: in a map ray-traced
 *            from scans the cells in front of a wall that were hit in some scans and seen through in others are unknown.
 *            Byte j of the signature is the least value of rays j m .. j m + m - 1.
 *   scan     a point (x, y) falls in the sector of "place descriptors" (the same float operations); r2 = fl(fl(x x) + fl(y
 *            y)), dropped unless finite; its byte is #{k in 1..254 : r2 >= edge2[k]}, edge2[k] = e e (one float multiply), e
 *            = (float)((double)unit k).  Byte j is the least byte of the points in sector j, 255 without one.  Offsets that
 *            are not a scan give 64 x 255 and are reported (kind 16384).
 *   cost     cost(q, a, s) = sum over the sectors j with Q[j] != 255 of |Q[j] - A[(j + s) mod 64]|; cost(q, a) the least
 *            over s = 0 .. 63, shift the smallest such s; key = cost 64 + shift.  The heading of the proposal is
 *            angle_mod(shift 2 pi / 64).
 *   records  per query top_k records int32[4] = {index into the anchor list, shift, cost, valid}, valid = #{j : Q[j] != 255}:
 *            the anchors in ascending (key, index) order, one accepted iff no accepted one lies within min_sep lattice steps
 *            (Chebyshev distance on (i, j)); unfilled records four -1; a query with valid < min_sectors has none.
 *   stats    8 int64: {lattice nodes, anchors found, anchors that did not fit, rays that ended on a wall, in unknown, outside or
 *            at n, queries without a record, records written}.  nhip_rangesig_anchors_dev writes words 0 - 2 and clears the
 *            rest, nhip_rangesig_map_dev writes 3 - 5, nhip_rangesig_match_dev 6 and 7: one block given to the calls in turn
 *            holds the whole record.
 *   prior    (host, double) x = (cell_x0 + cx + 0.5) res, y likewise, heading as above (nautilus_amd/rangesig.py: priors).
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): res finite and > 0;
 * width, height 1..16384; occ_min 1..127; free_max 0..occ_min - 1; stride 1..1024; max_ray_cells 1..4096; rays_per_sector 1,
 * 2, 4 or 8; unit finite and > 0, with n scale < 2^31 for every ray; top_k 1..16; min_sep 0..64; min_sectors 1..64; flags 0 or
 * NHIP_RANGESIG_UNKNOWN_STOPS; reserved 0; max_anchors, n_anchors 0..2^20; n_queries, n_scans >= 0. */
typedef struct nhip_rangesig_spec {
  double res;               /* metres per cell: the map's */
  double unit;              /* metres per step of a signature byte (0.125) */
  int32_t cell_x0;          /* the map's window: the occupancy spec's */
  int32_t cell_y0;
  int32_t width;
  int32_t height;
  int32_t occ_min;          /* a cell >= occ_min stops a ray (100) */
  int32_t free_max;         /* a cell in [0, free_max] may hold an anchor (0) */
  int32_t stride;           /* cells between lattice nodes (10) */
  int32_t max_ray_cells;    /* L: a ray's length in cells (600) */
  int32_t rays_per_sector;  /* m (4) */
  int32_t top_k;            /* records per query (5) */
  int32_t min_sep;          /* lattice steps between two records of a query, exclusive (2) */
  int32_t min_sectors;      /* sectors with a return a query needs (8) */
  int32_t flags;            /* 0 or NHIP_RANGESIG_UNKNOWN_STOPS */
  int32_t reserved;         /* 0 */
} nhip_rangesig_spec_t;
#define NHIP_RANGESIG_SECTORS 64
#define NHIP_RANGESIG_UNKNOWN_STOPS 1 /* flags: an unknown cell ends a ray with its range, as a wall does, not with 255 */
#define NHIP_RANGESIG_WORKSPACE_MAX (64ll << 20) /* what nhip_rangesig_workspace_bytes asks for at most, one key row excepted */
/* the defaults of the table above; the map's window is 0 and is the caller's to set; pure host */
int nhip_rangesig_spec_default(nhip_rangesig_spec_t *out);
/* rays: 64 m x int32[4] = {dx, dy, n, scale}; edge2: 255 floats, edge2[0] = 0; either may be NULL; pure host.  The `dir` table
 * of the sectors is nhip_place_tables'. */
int nhip_rangesig_tables(const nhip_rangesig_spec_t *spec, int32_t *rays, float *edge2);
/* bytes of the workspace nhip_rangesig_anchors_dev and nhip_rangesig_match_dev take for a list of n_anchors entries and
 * n_queries queries: a row of 4-byte keys per query (rows of ceil(n_anchors / 64) 64 keys) if those fit
 * NHIP_RANGESIG_WORKSPACE_MAX, else as many rows as do, at least one; never less than the 65,792 bytes of the anchors' row counts.  -1 on a
 * bad argument; pure host */
int64_t nhip_rangesig_workspace_bytes(const nhip_rangesig_spec_t *spec, int32_t n_anchors, int32_t n_queries);
/* The anchor list of a grid, on the caller's buffers and stream; never allocates, enqueues and returns without waiting.
 * d_grid: int8 [height][width], any alignment; d_anchors: max_anchors x int32[4], 16-byte aligned (may be NULL with
 * max_anchors 0); d_stats: 8 int64, 8-byte aligned; d_workspace: nhip_rangesig_workspace_bytes(spec, 0, 0) bytes or more, 4-byte
 * aligned. */
int nhip_rangesig_anchors_dev(const int8_t *d_grid, const nhip_rangesig_spec_t *spec, int32_t max_anchors, int32_t *d_anchors,
                              int64_t *d_stats, void *d_workspace, int64_t workspace_bytes, void *stream);
/* The map signatures of the n_anchors entries of d_anchors: d_sig[n_anchors][64] bytes, 4-byte aligned.  d_rays: the table of
 * nhip_rangesig_tables in device memory (64 m x int32[4]); its entries and the anchors' cells are checked before a cell index
 * becomes an address: an entry with n outside 1..4096, |dx| or |dy| above n, or n scale >= 2^31 is a ray that ends at n at
 * once, reported with kind 2097152 (index = the ray).  Same rules as above. */
int nhip_rangesig_map_dev(const int8_t *d_grid, const nhip_rangesig_spec_t *spec, const int32_t *d_rays, const int32_t *d_anchors,
                          int32_t n_anchors, uint8_t *d_sig, int64_t *d_stats, void *stream);
/* The scan signatures of n_scans packed scans: d_sig[n_scans][64] bytes, 4-byte aligned.  Same rules as above. */
int nhip_rangesig_scans_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_rangesig_spec_t *spec,
                            uint8_t *d_sig, void *stream);
/* The records of n_queries query signatures against n_anchors map signatures (both plain bytes, [.][64], 4-byte aligned, any
 * values) and their anchor list: d_records[n_queries][top_k][4] int32.  The query rows are taken in chunks of what the
 * workspace holds (at least one row of ceil(n_anchors / 64) 64 keys of 4 bytes, 4-byte aligned); the records are the same for
 * any chunking.  Same rules as above. */
int nhip_rangesig_match_dev(const uint8_t *d_query_sig, int32_t n_queries, const uint8_t *d_map_sig, const int32_t *d_anchors,
                            int32_t n_anchors, const nhip_rangesig_spec_t *spec, int32_t *d_records, int64_t *d_stats,
                            void *d_workspace, int64_t workspace_bytes, void *stream);

/* K15: FREE-SPACE CHECK of match records ("Free-space check"; tests/freespace_reference.py restates it
 * in numpy).  A record's score says how much of the source landed on the target's blurred hits; the check says where the rest
 * landed.  Build-defined and deterministic; all integer after the cells; no matcher kernel is involved.
 *   free plane  one per slot, in the layout of the slot's hit raster (hits_pitch, side + 64 rows, zero border of 32 cells,
 *               hits_bytes per slot), in a buffer of its own.  The sensor's cell is (S/2, S/2); a target point's end cell is
 *               S/2 + floor((double)v / res) per axis; a non-finite or out-of-grid point gives no ray.  For an end cell d away,
 *               n = max(|dx|, |dy|), the free cells are (S/2, S/2) + (rdiv(k dx, n), rdiv(k dy, n)), k = 0 .. n - 1, rdiv the
 *               occupancy grid's.  F = the union over all beams minus the slot's hit raster.
 *   source cell the matcher's: R(theta_k) = R(theta0) R(delta_k) from the nhip_csm_rot0 / nhip_csm_delta_table values, the point
 *               rotated in float with individually rounded products; cell = S/2 + floor((double)v' / res) + shift, shift =
 *               pair_origin + (ix - (nx - 1) / 2, iy - (ny - 1) / 2).
 *   class       of each source point, the first that applies: DROPPED (non-finite after rotation), OUTSIDE (the shifted cell is
 *               out of the grid, or |dx| or |dy| of the unshifted cell offset exceeds 4096), HIT (a target hit within Chebyshev
 *               distance hit_radius of the cell), FREE (the cell's bit in F), UNKNOWN.
 *   through     of every point of class HIT, FREE or UNKNOWN: its beam runs from the source sensor's cell o = (S/2, S/2) + shift
 *               to the point's cell, d the unshifted offset; it counts if for some k = 0 .. n - 1 - end_margin the cell
 *               o + (rdiv(k dx, n), rdiv(k dy, n)) lies inside the grid and is a target hit (undilated).
 *   record      int32[8] per pair: {n_points, dropped, outside, hit, free, unknown, through, 0}; a rejected match record
 *               (itheta < 0) gives eight -1.
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): hit_radius 0..16,
 * end_margin 0..64, flags 0, reserved 0; a grid spec whose side / 2 exceeds 4096 is refused. */
typedef struct nhip_freespace_spec {
  int32_t hit_radius; /* Chebyshev radius of the dilated hit test, in cells (2) */
  int32_t end_margin; /* steps before a beam's end that `through` does not look at (3) */
  int32_t flags;      /* 0 */
  int32_t reserved;   /* 0 */
} nhip_freespace_spec_t;
/* the defaults; pure host */
int nhip_freespace_spec_default(nhip_freespace_spec_t *out);
/* bytes of the free planes of n_slots slots of these grids (hits_bytes each), or -1 for a spec the check refuses; pure host */
int64_t nhip_freespace_planes_bytes(const nhip_grid_spec_t *grid_spec, int64_t n_slots);
/* The free planes of the n_targets slots of d_grids (built from the same scans and target ids by nhip_grid_build_dev), into
 * d_free (16-byte aligned; every byte of it is written: it needs no clearing).  Never allocates, enqueues and returns without
 * waiting.  A target id outside [0, n_scans) is an empty scan and nhip_dev_status() reports it (kind 1). */
int nhip_freespace_trace_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids,
                             int32_t n_targets, const nhip_grid_spec_t *grid_spec, const uint8_t *d_grids, uint8_t *d_free,
                             void *stream);
/* The records of n_pairs pairs: the pair arguments of nhip_csm_match_dev, the planes nhip_freespace_trace_dev made of the
 * same d_grids, the match records (device memory, as the matcher left them) and d_counts (8 int32 per pair).  pair_origin is
 * any int32 pair (not held to max_shift: a shift beyond the grid puts every point OUTSIDE).  A pair whose source, slot or
 * record indices are out of range is never dereferenced: its record is eight zeros and nhip_dev_status() reports it (kind
 * 32768, index = the pair); the other pairs are unaffected. */
int nhip_freespace_check_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_grids,
                             int32_t n_grids, const nhip_grid_spec_t *grid_spec, const int32_t *d_pair_src,
                             const int32_t *d_pair_slot, const double *d_rot0_cs, const double *d_delta_cs,
                             const int32_t *d_pair_origin, int32_t n_pairs, const nhip_search_t *search, const uint8_t *d_free,
                             const nhip_match_t *d_matches, const nhip_freespace_spec_t *fs_spec, int32_t *d_counts,
                             void *stream);

/* K16: PLACE DESCRIPTORS -- loop-closure candidates by appearance, from no pose at all ("Place
 * descriptors"; tests/place_reference.py restates it in numpy).  The reference asks a learned embedding behind a service
 * (lc_match_threshold, solver.cc:58-60); the network is not in its tree, so the descriptor is build-defined: R rings x 64
 * sectors of the scan frame, one bit per bin that holds a return.  Two float comparisons per point, integers after them.
 *   tables      e_k = (float)((double)range_max k / R), edge2[k] = e_k e_k (one float multiply), k = 0 .. R;
 *               dir[j] = ((float)cos(2 pi j / 64), (float)sin(2 pi j / 64)), j = 0 .. 31, cos and sin in double.
 *   bit         of a point (x, y), every operation a float operation rounded on its own: r2 = (x x) + (y y); the point is
 *               dropped unless r2 is finite and r2 < edge2[R]; ring = #{k in 1 .. R-1: r2 >= edge2[k]}; neg = y < 0 or (y == 0
 *               and x < 0); (u, v) = neg ? (-x, -y) : (x, y); sector = #{j in 1 .. 31: (dir[j].x v) - (dir[j].y u) >= 0} +
 *               (neg ? 32 : 0); bit `sector` of word `ring` is set.
 *   descriptor  uint64 D[R] per scan, bits = the sum of the words' popcounts.
 *   distance    dist(i, j, s) = sum_r popcount(D_i[r] XOR rotl64(D_j[r], s)); dist(i, j) = min_s, shift = the smallest
 *               minimising s.  The heading of scan i relative to scan j is theta0 = AngleMod(-shift 2 pi / 64).
 *   list        ids: n_ids scan ids, strictly ascending.  Entry b (scan j) is admissible for query a (scan i) iff |i - j| >
 *               min_separation, j < i under NHIP_PLACE_PAST_ONLY, bits_i > 0 and bits_j > 0, and
 *               1000 dist <= max_permille (bits_i + bits_j).
 *   records     per query top_k x int32[4] = {j, shift, dist, bits_j}: the admissible candidates in ascending (dist, j)
 *               order; unfilled records are four -1.
 *   stats       8 int64: {n_ids, admissible pairs before the permille gate, after it, records written, queries without a
 *               record, scans of the list with bits == 0, 0, 0}.
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): n_rings 1..32 to
 * describe and 1..15 to match (a pair's result is a 16-bit key dist * 64 + shift, 0xFFFF for none: dist <= 64 R must stay
 * below 1023); range_max finite and > 0; top_k 1..32; min_separation >= 0; max_permille 0..1000; flags 0 or
 * NHIP_PLACE_PAST_ONLY; n_ids 0..2^20. */
#define NHIP_PLACE_PAST_ONLY 1
#define NHIP_PLACE_WORKSPACE_MAX (64ll << 20) /* what nhip_place_workspace_bytes asks for at most: longer lists go in chunks */
typedef struct nhip_place_spec {
  int32_t n_rings;        /* R (10) */
  float range_max;        /* the outer edge of the last ring, metres (30) */
  int32_t top_k;          /* K records per query (5) */
  int32_t min_separation; /* scans between the two of a pair (20) */
  int32_t max_permille;   /* the gate: dist per 1000 of bits_i + bits_j (1000: no gate) */
  int32_t flags;          /* 0, or NHIP_PLACE_PAST_ONLY */
} nhip_place_spec_t;
/* the defaults of the table above; pure host */
int nhip_place_spec_default(nhip_place_spec_t *out);
/* edge2: n_rings + 1 floats; dir: 32 x 2 floats; pure host */
int nhip_place_tables(const nhip_place_spec_t *spec, float *edge2, float *dir);
/* bytes of the key workspace of a list of n_ids: 2 bytes per (query row, candidate), rows of n_ids rounded up to 64
 * candidates, all rows if that stays within NHIP_PLACE_WORKSPACE_MAX, else as many multiples of 16 rows as do (at least 16);
 * -1: a bad spec or n_ids, message in nhip_last_error; pure host */
int64_t nhip_place_workspace_bytes(const nhip_place_spec_t *spec, int32_t n_ids);
/* The descriptors of all scans: d_desc n_scans x n_rings uint64, d_bits n_scans int32.  Never allocates, enqueues and
 * returns without waiting.  A scan whose first offset is negative or whose end lies before its start is treated as empty and
 * nhip_dev_status() reports it (kind 16384). */
int nhip_place_describe_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_place_spec_t *spec,
                            uint64_t *d_desc, int32_t *d_bits, void *stream);
/* The records of the list d_ids (ascending: the caller's promise) among the descriptors nhip_place_describe_dev made with
 * the same n_rings: d_records n_ids x top_k x 4 int32, d_stats 8 int64.  The workspace (2-byte aligned) may be smaller than
 * nhip_place_workspace_bytes says, down to 16 rows: the query rows are then taken in more chunks, with the same result.  An id
 * outside [0, n_scans) is never dereferenced: it is a scan without bits, in no record and with none of its own, and
 * nhip_dev_status() reports it (kind 65536, index = its position in the list). */
int nhip_place_match_dev(const uint64_t *d_desc, const int32_t *d_bits, int32_t n_scans, const int32_t *d_ids, int32_t n_ids,
                         const nhip_place_spec_t *spec, int32_t *d_records, int64_t *d_stats, void *d_workspace,
                         int64_t workspace_bytes, void *stream);

/* K16b: PLACE SEQUENCES -- the appearance match of K16 taken over a window of frames around both scans of a pair (DESIGN.md
 * section 3, "Place sequences"; tests/place_seq_reference.py restates it in numpy).  The reference votes over a window of frames
 * around a keyframe (lc_match_window_size = 5, default_config.lua:138-139); the code that used it is not in its tree, so the
 * window is build-defined: the diagonal sum of SeqSLAM over the single-scan distances.  Descriptors, bits, dist, shift and
 * theta0 are K16's.  A frame is a SCAN ID in [0, n_scans), not a position in the list.
 *   pair        entry b (scan j) is admissible for query a (scan i) iff |i - j| > min_separation, j < i under
 *               NHIP_PLACE_PAST_ONLY, bits_i > 0 and bits_j > 0 (K16's rule without the permille gate).
 *   frames      for direction sigma in {+1, -1} and offset d in -W .. W: a = i + d step, b = j + sigma d step.  Offset d counts
 *               for sigma iff 0 <= a < n_scans, 0 <= b < n_scans, bits_a > 0 and bits_b > 0 (d = 0 always counts).
 *   sums        sum_sigma = the sum of dist(a, b), norm_sigma = the sum of bits_a + bits_b, frames_sigma = the count, over the
 *               offsets that count.
 *   score       score_sigma = (sum_sigma (2W + 1)) div frames_sigma: a window cut short is scaled to a full one (<= 16,320).
 *   direction   0 (sigma = +1, the same way round) if score_+ <= score_-, else 1 (sigma = -1, the place revisited the other
 *               way round); seq, sum, norm and frames are those of the chosen direction.
 *   gate        1000 sum <= max_permille norm: K16's permille gate, taken on the window.
 *   records     per query top_k x int32[8] = {j, shift, dist, bits_j, seq, sum, frames, direction}: shift and dist of the centre
 *               frames (i, j); the admissible, gated candidates in ascending (seq, j); unfilled records are eight -1.
 *   stats       8 int64, laid out as K16's, with slot 6 = gated pairs whose direction is 1 and slot 7 = gated pairs with
 *               frames < 2W + 1.
 * At W = 0, fields 0..3 of every record and stats 0..5 are nhip_place_match_dev's, seq = sum = dist, frames = 1, direction = 0.
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): those of a K16 match
 * (n_rings 1..15), half_window 0..8, step 1..16, min_separation >= 2 half_window step (the two windows of a pair then never
 * touch); n_scans >= 0; n_ids 0..2^20. */
typedef struct nhip_place_seq_spec {
  int32_t half_window; /* W: the window is 2W + 1 frames (2: the reference's window of 5) */
  int32_t step;        /* scans between two frames of a window (1) */
} nhip_place_seq_spec_t;
/* the defaults of the table above; pure host */
int nhip_place_seq_spec_default(nhip_place_seq_spec_t *out);
/* bytes of the workspace: per query scan a row of the plane of single distances (2 bytes per scan, n_scans rounded up to 64) and
 * a row of window keys (2 bytes per entry, n_ids rounded up to 64).  All scans at once if that stays within
 * NHIP_PLACE_WORKSPACE_MAX; else as many query scans per chunk as fit beside the chunk's halo of 2 half_window step plane rows,
 * at least 16.  -1: a bad spec, n_scans or n_ids, message in nhip_last_error; pure host */
int64_t nhip_place_seq_workspace_bytes(const nhip_place_spec_t *spec, const nhip_place_seq_spec_t *seq, int32_t n_scans, int32_t n_ids);
/* The records of the list d_ids (ascending: the caller's promise) among the descriptors of ALL n_scans scans -- the window
 * frames need not be entries of the list: d_records n_ids x top_k x 8 int32, d_stats 8 int64.  The workspace (2-byte aligned)
 * may be smaller than nhip_place_seq_workspace_bytes says, down to 16 query scans and their halo: the query scans are then
 * taken in more chunks, with the same result.  Never allocates, enqueues and returns without waiting.  An id outside
 * [0, n_scans) is never dereferenced and is reported as by nhip_place_match_dev (kind 65536); a window frame outside the scans
 * is absent and no error. */
int nhip_place_seq_match_dev(const uint64_t *d_desc, const int32_t *d_bits, int32_t n_scans, const int32_t *d_ids, int32_t n_ids,
                             const nhip_place_spec_t *spec, const nhip_place_seq_spec_t *seq, int32_t *d_records, int64_t *d_stats,
                             void *d_workspace, int64_t workspace_bytes, void *stream);

/* K17: LOOP-CLOSURE CONSISTENCY -- the records of loop closure judged against each other ("Loop-closure
 * consistency"; tests/consistency_reference.py restates it in numpy).  The reference leaves wrong closures to a human (HITL
 * curation); this is pairwise consistency maximisation (Mangelson et al., ICRA 2018), build-defined: two records are consistent
 * if the cycle they form with the odometry between their ends closes up to the drift that odometry can have gathered, and a
 * large set of mutually consistent records is grown greedily.
 *   records     M x 8 doubles {cw, sw, xw, yw, px, py, la, lb}, prepared on the host (nautilus_amd/consistency.py, prepare):
 *               W_m = X_tgt o Z_m o X_src^-1 as cosine, sine and translation, the position of tgt, the arc lengths of src and
 *               tgt along the trajectory.  No kernel calls a transcendental.
 *   pair test   for m != n, lo = min(m, n), hi = max(m, n) (symmetric by construction); every operation an fp64 operation
 *               rounded on its own, in this order (a b: product; negation and the factor 2 are exact):
 *                 ihx = -((c_hi x_hi) + (s_hi y_hi))        ihy = (s_hi x_hi) - (c_hi y_hi)
 *                 cq  = (c_lo c_hi) + (s_lo s_hi)           sq  = (s_lo c_hi) - (c_lo s_hi)
 *                 qx  = ((c_lo ihx) - (s_lo ihy)) + x_lo    qy  = ((s_lo ihx) + (c_lo ihy)) + y_lo
 *                 ex  = (((cq px_lo) - (sq py_lo)) + qx) - px_lo
 *                 ey  = (((sq px_lo) + (cq py_lo)) + qy) - py_lo
 *                 e2  = (ex ex) + (ey ey)                   chord = 2 - (2 cq)
 *                 len = |la_lo - la_hi| + |lb_lo - lb_hi|
 *                 tt  = min(t0 + (t_rate len), t_max)       tr  = min(r0 + (r_rate len), r_max)
 *               with min(a, b) = b < a ? b : a (a NaN sum stays); consistent iff e2 <= (tt tt) and chord <= (tr tr): a NaN
 *               anywhere fails a comparison.  The diagonal is 0.
 *   matrix      M rows of W = ceil(M / 64) uint64 words, bit n of row m in bit n % 64 of word n / 64, zero beyond M;
 *               deg[m] = popcount(row m).
 *   set         C = all records; each step: u = the member of C with the largest score, the smaller index among equals --
 *               the score is deg[u] in the first step and popcount(A[u] & C) after it --, u is appended, C &= A[u]; until C is
 *               empty or max_steps members are appended.  M = 0: the empty set; a matrix without edges: record 0 alone.
 *   stats       8 int64: {M, edges, the largest degree, steps taken (= members), 1 if the step cap ended the set with C not
 *               empty, 0, 0, 0}; nhip_consistency_adjacency_dev writes the first three and zeros.
 * Accepted ranges (anything else is NHIP_ERR_ARG before anything is launched, with or without a device): every tolerance finite
 * and >= 0, t_max >= t0, r_max >= r0, max_steps >= 1, flags 0, M 0..65536. */
#define NHIP_CONSISTENCY_STATE_BYTES 8448 /* the set's own part of the workspace: 256 bytes of state, then 1024 words of C */
typedef struct nhip_consistency_spec {
  double t0;         /* translation tolerance of a cycle without odometry, metres (0.8) */
  double t_rate;     /* ... gained per metre of odometry the cycle spans (0.1) */
  double t_max;      /* ... and its cap (16) */
  double r0;         /* rotation tolerance, as a chord ~ radians (0.1) */
  double r_rate;     /* ... per metre (0.005) */
  double r_max;      /* ... cap (0.5) */
  int32_t max_steps; /* members appended at most (65536: no cap) */
  int32_t flags;     /* 0 */
} nhip_consistency_spec_t;
/* the defaults of the table above; pure host */
int nhip_consistency_spec_default(nhip_consistency_spec_t *out);
/* bytes of the ONE buffer a caller needs for M records: the set's state and live set in the first
 * NHIP_CONSISTENCY_STATE_BYTES, then room for the matrix (8 M W bytes, from that offset) and the degrees (4 M bytes, behind the
 * matrix), rounded up to 256.  -1: M outside 0..65536, message in nhip_last_error; pure host */
int64_t nhip_consistency_workspace_bytes(int32_t M);
/* The matrix and the degrees of M prepared records (d_records: M x 8 doubles): d_adj M x W uint64, d_deg M int32, d_stats 8
 * int64.  Never allocates, enqueues and returns without waiting. */
int nhip_consistency_adjacency_dev(const double *d_records, int32_t M, const nhip_consistency_spec_t *spec, uint64_t *d_adj,
                                   int32_t *d_deg, int64_t *d_stats, void *stream);
/* The consistent set of a matrix: d_members M int32 in pick order (-1 behind them), d_n_members one int32, d_stats 8 int64.
 * d_workspace (256-byte aligned) is the buffer of nhip_consistency_workspace_bytes(M) -- a smaller one is NHIP_ERR_ARG; d_adj
 * and d_deg normally lie inside it, at the offsets given there.  Steps are enqueued check_every at a time (0: the default,
 * 8) and the call reads one word between two batches: it WAITS for the stream, and check_every changes no result.  A degree
 * outside [0, M) counts as 0 and nhip_dev_status() reports it (kind 131072, index = the record); a member index outside
 * [0, M) -- only a workspace overwritten during the call can produce one -- ends the set and is reported (kind 262144).  Bits
 * of the matrix beyond M and on the diagonal are never followed. */
int nhip_consistency_set_dev(const uint64_t *d_adj, const int32_t *d_deg, int32_t M, const nhip_consistency_spec_t *spec,
                             int32_t check_every, int32_t *d_members, int32_t *d_n_members, int64_t *d_stats, void *d_workspace,
                             int64_t workspace_bytes, void *stream);

/* HITL point selection: GetRelevantPosesForHITL (solver.cc:479-513) for every scan at once.  A point p of scan s goes to
 * the world as w = (c px - s py + tx, s px + c py + ty) with (c, s, tx, ty) = d_pose_f32[4s ..], the entries of
 * PoseArrayToAffine(pose).cast<float>() (nhip_pose_affines forms them), every operation a float operation rounded on its
 * own; DistanceToLineSegment<float> (slam_util.h:92-110) against line a, and for a point not on a against line b; a point
 * is ON a line iff (double)distance <= line_width -- the reference's comparison of a float with CONFIG_DOUBLE
 * hitl_line_width, under which a distance of exactly float(0.05) is NOT on the line.  A non-finite point is on no line.
 * A scan with at least point_threshold points on a is an a-node and contributes its a-points only; otherwise one with at
 * least point_threshold points on b is a b-node and contributes its b-points only.  Blocks: all a-nodes in node order, then
 * all b-nodes in node order; points inside a block in scan order.
 * A non-finite or negative line_width, a point_threshold below 1 or a negative n_scans is NHIP_ERR_ARG before anything is
 * launched (with or without a device).  Scans of any length, empty ones included. */
typedef struct nhip_hitl_spec {
  float line_a[4];         /* x0 y0 x1 y1, LineSegment<float> (LineSegmentsFromHitlMsg, solver.cc:467-478) */
  float line_b[4];
  double line_width;       /* hitl_line_width (0.05) */
  int32_t point_threshold; /* hitl_pose_point_threshold (10) */
  int32_t reserved;        /* 0 */
} nhip_hitl_spec_t;
/* both lines zero, line_width 0.05, point_threshold 10; pure host */
int nhip_hitl_spec_default(nhip_hitl_spec_t *out);
/* Classifies and counts.  Outputs: d_class, one byte per point of d_xy (0: on neither line, 1: on a, 2: on b); d_counts[2s],
 * d_counts[2s + 1]: the points of scan s on a and on b; d_scan_block[s]: the block of scan s (-1: it joins neither line);
 * d_scan_offset[s]: the index of its first point in the packed array; d_totals = {n_a, n_b, n_points}: the a-nodes, the
 * b-nodes and the points of all blocks (zeros for n_scans == 0 or when nothing is selected). */
int nhip_hitl_select_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const float *d_pose_f32,
                         const nhip_hitl_spec_t *spec, uint8_t *d_class, int32_t *d_counts, int32_t *d_scan_block,
                         int32_t *d_scan_offset, int32_t *d_totals, void *stream);
/* Packs what nhip_hitl_select_dev selected into buffers the caller sized from the totals it downloaded: n_blocks = n_a + n_b,
 * n_points; d_points (2 floats per point, scan frame), d_block_offsets[n_blocks + 1], d_block_pose[n_blocks] (the node of
 * every block) -- the layout nhip_resid_point_to_line_normal_eq_dev takes.  Sizes that are not the totals behind d_totals
 * write nothing and make nhip_dev_status() report it (kind 8). */
int nhip_hitl_pack_dev(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const uint8_t *d_class,
                       const int32_t *d_counts, const int32_t *d_scan_block, const int32_t *d_scan_offset,
                       const int32_t *d_totals, int32_t n_blocks, int32_t n_points, float *d_points,
                       int32_t *d_block_offsets, int32_t *d_block_pose, void *stream);

/* ------------------------------------------------------------------ K22: match refinement (point-to-line ICP from the lattice pose)
 * A match record is a pose of the search lattice: one cell and one rotation step.  The refinement takes every pair of a
 * list from its lattice pose to the sub-cell pose at which the source scan's points lie on the target SCAN's lines: a few
 * Gauss-Newton updates on point-to-line residuals, one workgroup per pair, one launch for the list.  The rule -- every
 * operation, the order of every sum -- is DESIGN.md section 3, "Match refinement"; tests/refine_reference.py restates it in
 * numpy and the device equals it bit for bit.  A pose is (c, s, tx, ty) in double: q = R p + t takes a source point into
 * the target's frame (nhip_match_to_transform's convention). */
#define NHIP_REFINE_THRESHOLDS 16      /* slots of the spec's threshold table = the largest max_iterations */
#define NHIP_REFINE_TARGET_MAX 2048    /* points of a target scan the kernel stages */
#define NHIP_REFINE_TRACE_DOUBLES 64   /* per pair: (c, s, tx, ty) after update k at 4k ..; zeros behind the last update */
#define NHIP_REFINE_SKIPPED 1u         /* pose0 not finite (a rejected record): NaNs returned */
#define NHIP_REFINE_TARGET_TOO_LONG 2u /* the target has more than NHIP_REFINE_TARGET_MAX points: pose0 returned */
#define NHIP_REFINE_FEW 4u             /* an evaluation kept fewer than min_corr correspondences: pose0 returned */
#define NHIP_REFINE_SINGULAR 8u        /* a pivot <= 0 or lambda_min(H[0:2, 0:2]) / n_corr < min_spread: pose0 returned */
#define NHIP_REFINE_RUNAWAY 16u        /* an update left the start by more than max_shift_m / max_turn_sin: pose0 returned */
#define NHIP_REFINE_NOT_CONVERGED 32u  /* max_iterations updates without meeting the tolerances: the refined pose; informational */
typedef struct nhip_refine_spec {
  double thr0;          /* correspondence threshold of update 0 [m] (outlier_threshold, 0.25); the bucket grid's cells */
  double shrink;        /* factor per update (0.5), in (0, 1] */
  double thr_min;       /* floor of the thresholds (0.05), in (0, thr0] */
  double step_tol_m;    /* stop when sqrt(dx^2 + dy^2) < step_tol_m and |dtheta| < step_tol_rad (1e-5 both) */
  double step_tol_rad;
  double min_spread;    /* 0.02 */
  double max_shift_m;   /* 0.5 */
  double max_turn_sin;  /* sin(5 deg), filled by the host */
  float thr[NHIP_REFINE_THRESHOLDS]; /* thr[k] = (float)max(thr_min, thr0 * shrink^k), the power by repeated products in
                           double; update k reads thr[k], the final evaluation thr[max_iterations - 1].  The kernel reads THIS
                           table; a caller that edits thr0, shrink or thr_min fills it again (0 < thr[k] <= thr[0] = (float)thr0) */
  int32_t max_iterations; /* 8; 1 .. NHIP_REFINE_THRESHOLDS */
  int32_t min_corr;       /* 30; >= 3 */
  int32_t flags;          /* 0 */
  int32_t reserved;       /* 0 */
} nhip_refine_spec_t;
typedef struct nhip_refined {
  double c, s, tx, ty;  /* the pose returned (see the flags) */
  double info[6];       /* the final evaluation's H = sum J^T J over (x, y, theta): H00 H01 H02 H11 H12 H22 */
  double cost;          /* its sum of squared residuals [m^2] */
  int32_t n_corr;       /* its correspondences */
  int32_t iterations;   /* updates performed */
  uint32_t flags;       /* OR of NHIP_REFINE_* */
  uint32_t pad;         /* 0 */
} nhip_refined_t;
/* the defaults above, the table filled; pure host */
int nhip_refine_spec_default(nhip_refine_spec_t *out);
/* Pure host: the start poses of n records, 4 doubles each: theta = theta0 + (itheta - (n_theta - 1) / 2) theta_step,
 * t = (origin + i - (n - 1) / 2) res as nhip_match_to_transform forms them but in double; c = cos(theta), s = sin(theta)
 * from libm.  A rejected record (itheta < 0) gives four NaNs.  pair_origin (2 per pair) may be NULL: zeros. */
int nhip_refine_start_poses(const nhip_match_t *records, const double *theta0, const int32_t *pair_origin, int32_t n_pairs,
                            const nhip_grid_spec_t *grid_spec, const nhip_search_t *search, double *pose0);
/* The refinement of n_pairs pairs on device arrays: d_xy / d_normals (2 floats per point, the scan's frame), d_offsets
 * (n_scans + 1), d_pair_src / d_pair_tgt (scan ids), d_pose0 (4 doubles per pair) in; d_out (n_pairs records) and, unless
 * NULL, d_trace (NHIP_REFINE_TRACE_DOUBLES per pair) out.  Enqueues one kernel; allocates nothing.  A scan id outside
 * [0, n_scans) is never dereferenced: the pair matches nothing (NHIP_REFINE_FEW, pose0) and nhip_dev_status() reports it
 * (kind 4194304, index = the pair).  d_offsets itself must be valid, as for every "_dev" entry point: ascending, its last entry
 * at most the points behind d_xy and d_normals; the kernel checks the ids, not the offsets.  A spec outside its ranges is
 * NHIP_ERR_ARG with or without a device. */
int nhip_refine_icp_dev(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans,
                        const int32_t *d_pair_src, const int32_t *d_pair_tgt, const double *d_pose0, int32_t n_pairs,
                        const nhip_refine_spec_t *spec, nhip_refined_t *d_out, double *d_trace, void *stream);
/* The same on host arrays (n_points = offsets[n_scans] points): stages them, runs the kernel on the null stream, waits.
 * Scan ids are checked on the host (NHIP_ERR_ARG).  trace may be NULL. */
int nhip_refine_icp(const float *xy, const float *normals, const int32_t *offsets, int32_t n_scans, const int32_t *pair_src,
                    const int32_t *pair_tgt, const double *pose0, int32_t n_pairs, const nhip_refine_spec_t *spec,
                    nhip_refined_t *out, double *trace);
/* Pure host: (tx, ty, theta = atan2(s, c)) of a refined record. */
int nhip_refined_to_transform(const nhip_refined_t *r, double *tx, double *ty, double *theta);
/* Pure host: the information of relative-pose factors made from refined records (K23, above). */
int nhip_relpose_information(const nhip_refined_t *refined, int32_t n, double sigma_m, double wt, double wr, double *info,
                             uint8_t *from_icp);

/* ------------------------------------------------------------------ handle API (host pointers) */
typedef struct nhip_scans nhip_scans_t;
typedef struct nhip_grids nhip_grids_t;
typedef struct nhip_resid_batch nhip_resid_batch_t;

/* std::vector<Eigen::Vector2f> point clouds of n_scans scans, concatenated. */
int nhip_scans_upload(const float *xy, const int32_t *offsets, int32_t n_scans, nhip_scans_t **out);
int nhip_scans_free(nhip_scans_t *scans);

int nhip_grids_build(const nhip_scans_t *scans, const int32_t *target_ids, int32_t n_targets,
                     const nhip_grid_spec_t *spec, nhip_grids_t **out);
/* Tables of n_targets SUBMAPS of the uploaded scans (see nhip_submaps_gather_dev): slot t is the table of target t's merged
 * cloud, gathered on the device.  member_scan, member_affine (4 floats per member) and member_offsets (n_targets + 1) are
 * HOST arrays; a member id outside the scans or offsets that are not a prefix from 0 are NHIP_ERR_ARG.  The grids work with
 * nhip_csm_match, nhip_csm_match_gated, nhip_csm_scores and the downloads exactly as those of nhip_grids_build do. */
int nhip_grids_build_submaps(const nhip_scans_t *scans, const int32_t *member_scan, const float *member_affine,
                             const int32_t *member_offsets, int32_t n_targets, const nhip_grid_spec_t *spec,
                             nhip_grids_t **out);
int nhip_grids_free(nhip_grids_t *grids);
/* copy stored (padded) grid `slot` to host: layout.grid_bytes bytes (uint8 or uint16 cells) */
int nhip_grids_download(const nhip_grids_t *grids, int32_t slot, uint8_t *out);

/* Batched GetTransformation: theta0[i] = AngleMod(rot_a - rot_b) of pair i;
 * pair_origin: NULL or 2 int32 per pair (search centre in cells). */
int nhip_csm_match(const nhip_scans_t *scans, const nhip_grids_t *grids, const int32_t *pair_src,
                   const int32_t *pair_slot, const double *theta0, const int32_t *pair_origin,
                   int32_t n_pairs, const nhip_search_t *search, nhip_match_t *out,
                   int32_t *out_sums);
/* ... with the score gate of nhip_csm_match_gated_dev (same contract): a record whose score is below min_score comes back
 * as {-1, -1, -1, -INFINITY} with sum -1; -INFINITY is nhip_csm_match; NaN is NHIP_ERR_ARG and nothing is written. */
int nhip_csm_match_gated(const nhip_scans_t *scans, const nhip_grids_t *grids, const int32_t *pair_src,
                         const int32_t *pair_slot, const double *theta0, const int32_t *pair_origin,
                         int32_t n_pairs, const nhip_search_t *search, nhip_match_t *out,
                         int32_t *out_sums, double min_score);
int nhip_csm_scores(const nhip_scans_t *scans, const nhip_grids_t *grids, int32_t src, int32_t slot,
                    double theta0, int32_t origin_x, int32_t origin_y, const nhip_search_t *search,
                    int32_t *out_sums);

/* Host-pointer forms of the candidate gating. */
int nhip_lc_scatter_scores(const nhip_scans_t *scans, double *scores /* n_scans */);
int nhip_lc_pair_gate(const double *poses, int32_t n_poses, const int32_t *candidates, int32_t n_candidates,
                      double max_range, int32_t min_separation, uint8_t *flags /* n_candidates^2 */);
int nhip_lc_chi_square_gate(const double *poses, int32_t n_poses, const int32_t *pair_src, const int32_t *pair_tgt,
                            const float *cov /* n_pairs x 4 */, int32_t n_pairs, double max_score,
                            double *scores /* n_pairs */, uint8_t *flags /* n_pairs */);

/* nhip_features_extract_dev on uploaded scans; host outputs of the same shapes (scores: n_points doubles, may be NULL). */
int nhip_features_extract(const nhip_scans_t *scans, const nhip_feature_spec_t *spec, int32_t *planar_idx,
                          int32_t *planar_count, int32_t *edge_idx, int32_t *edge_count, double *scores);

/* nhip_normals_estimate_dev on uploaded scans; host outputs (normals: 2 floats per point; info: 4 int32 per point, may be
 * NULL). */
int nhip_normals_estimate(const nhip_scans_t *scans, const nhip_normals_spec_t *spec, float *normals, int32_t *info);

/* nhip_vectorize_dev on uploaded scans, with host poses (3 doubles per scan) and host outputs (records: room for
 * max_segments x 10 int64; stats: 8 int32); allocates and frees its workspace. */
int nhip_vectorize(const nhip_scans_t *scans, const double *poses, const nhip_vectorize_spec_t *spec, int32_t max_cells,
                   int32_t max_rounds, int32_t check_every, int64_t *records, int32_t *stats);

/* nhip_occupancy_dev on uploaded scans, with host poses (3 doubles per scan) and host outputs (hits, misses: width x height
 * int32; grid: width x height int8; stats: 8 int64); allocates and frees its device buffers.  With NHIP_OCC_ACCUMULATE hits
 * and misses are also inputs: they are uploaded first. */
int nhip_occupancy(const nhip_scans_t *scans, const double *poses, const nhip_occupancy_spec_t *spec, int32_t *hits,
                   int32_t *misses, int8_t *grid, int64_t *stats);

/* nhip_transient_filter_dev on uploaded scans (n_points: the points the handle holds), with host poses (3 doubles per scan),
 * host planes (hits, misses: width x height int32, uploaded, not modified) and host outputs (labels: a byte per point;
 * out_xy: 2 floats per point; out_offsets: n_scans + 1 int32; out_index: an int32 per point; stats: 8 int64); allocates and
 * frees its device buffers.  Only the first out_offsets[n_scans] entries of out_xy and out_index are written. */
int nhip_transient_filter(const nhip_scans_t *scans, const double *poses, const nhip_transient_spec_t *spec, const int32_t *hits,
                          const int32_t *misses, uint8_t *labels, float *out_xy, int32_t *out_offsets, int32_t *out_index,
                          int64_t *stats);

/* nhip_mapwin_cells_dev + nhip_mapwin_gather_dev on host memory: grid (width x height int8), origins (2 int32 per query) and the
 * outputs out_xy (room for `capacity` points of 2 floats; may be NULL with capacity 0), out_offsets (n_queries + 1 int32) and
 * stats (8 int64).  The cell list is sized from the grid, so only the points can fail to fit: the call then returns NHIP_OK
 * with every offset 0 and stats[6] = 1, and nhip_dev_status() reports it.  Only the first out_offsets[n_queries] points of
 * out_xy are written.  Allocates and frees its device buffers. */
int nhip_map_windows(const int8_t *grid, const nhip_mapwin_spec_t *spec, const int32_t *origins, int32_t n_queries, float *out_xy,
                     int64_t capacity, int32_t *out_offsets, int64_t *stats);

/* The four range-signature calls on host memory: grid (width x height int8), the packed scans xy (2 floats per point) and
 * offsets (n_scans + 1 int32, ascending from 0: anything else is NHIP_ERR_ARG before a launch), and the outputs records
 * (n_scans x top_k x 4 int32), anchors (room for max_anchors x 4 int32; may be NULL with max_anchors 0), n_anchors (one int32:
 * the entries written), stats (8 int64) and, unless NULL, map_sig (max_anchors x 64 bytes) and scan_sig (n_scans x 64 bytes).
 * More anchors than max_anchors: the first max_anchors are matched, stats[2] says how many were left out and
 * nhip_dev_status() reports it.  Allocates and frees its device buffers; the key workspace is nhip_rangesig_workspace_bytes. */
int nhip_rangesig_candidates(const int8_t *grid, const nhip_rangesig_spec_t *spec, const float *xy, const int32_t *offsets,
                             int32_t n_scans, int32_t max_anchors, int32_t *records, int32_t *anchors, int32_t *n_anchors,
                             int64_t *stats, uint8_t *map_sig, uint8_t *scan_sig);

/* nhip_freespace_check_dev on handles: the pair arguments of nhip_csm_match, the records it returned (host memory) and
 * counts (8 int32 per pair, host memory).  `scans` must be the scans `grids` was built from: the first call on a grids handle
 * traces its free planes from them (nhip_freespace_trace_dev) and keeps the planes with the handle; later calls only check.
 * Ids out of range are NHIP_ERR_ARG before anything is launched.  A handle built by nhip_grids_build_submaps is refused with
 * NHIP_ERR_STATE: a submap's free space needs one ray origin per member. */
int nhip_csm_freespace(const nhip_scans_t *scans, const nhip_grids_t *grids, const int32_t *pair_src, const int32_t *pair_slot,
                       const double *theta0, const int32_t *pair_origin, int32_t n_pairs, const nhip_search_t *search,
                       const nhip_match_t *matches, const nhip_freespace_spec_t *fs_spec, int32_t *counts);

/* nhip_place_describe_dev + nhip_place_match_dev on uploaded scans: ids (host, n_ids, strictly ascending and inside the
 * scans: anything else is NHIP_ERR_ARG before anything is launched), records (n_ids x top_k x 4 int32) and stats (8 int64)
 * in host memory; desc (n_scans x n_rings uint64) and bits (n_scans int32) may be NULL.  Allocates and frees its device
 * buffers; the key workspace is nhip_place_workspace_bytes. */
int nhip_place_candidates(const nhip_scans_t *scans, const int32_t *ids, int32_t n_ids, const nhip_place_spec_t *spec,
                          int32_t *records, int64_t *stats, uint64_t *desc, int32_t *bits);

/* nhip_place_describe_dev + nhip_place_seq_match_dev on uploaded scans: ids as for nhip_place_candidates, records (n_ids x
 * top_k x 8 int32) and stats (8 int64) in host memory.  Every scan a window reaches must be among the uploaded ones with its
 * points, or it is a frame without bits.  Allocates and frees its device buffers; the workspace is
 * nhip_place_seq_workspace_bytes. */
int nhip_place_seq_candidates(const nhip_scans_t *scans, const int32_t *ids, int32_t n_ids, const nhip_place_spec_t *spec,
                              const nhip_place_seq_spec_t *seq, int32_t *records, int64_t *stats);

/* nhip_consistency_adjacency_dev + nhip_consistency_set_dev on host memory: records (M x 8 doubles), members (M int32, -1 behind
 * the set), n_members (one int32) and stats (8 int64).  Allocates and frees its device buffers; steps in batches of 8. */
int nhip_consistency(const double *records, int32_t M, const nhip_consistency_spec_t *spec, int32_t *members, int32_t *n_members,
                     int64_t *stats);

/* The reference-shaped single-pair call: CorrelativeScanMatcher(scanner_range, trans_range, low_res, high_res)
 * .GetTransformation(pc_a, pc_b, rot_a, rot_b, rot_restriction) -> (score, ((tx, ty), theta))
 * (solver.cc:56, 633-644; the class lives in the absent third_party/csm).  Build-defined search:
 * exhaustive on the low_res grid over +-trans_range and +-rot_restriction in 1 degree steps, then exhaustive on the
 * high_res grid over +-low_res around the coarse optimum in 0.1 degree steps; the returned score is the fine optimum's
 * mean log-likelihood on the unquantised table (NHIP_SEARCH_EXACT_SCORE).  This is the ONE implementation of that
 * search: the C++ drop-in (adapters/CorrelativeScanMatcher.h) and the Python mirror (nautilus_amd/csm.py) both call it;
 * oracle/csm_oracle.c restates it independently for the tests.  Host pointers.  pc_a / pc_b: n x 2 floats
 * (std::vector<Eigen::Vector2f>).  The two tables built from pc_b stay in a cache of the last targets (keyed by the cloud's
 * bytes and the parameters, per device; least recently used out first under a byte cap, 3 GB by default -- one target of
 * the (30, 2, 0.3, 0.01) matcher is ~0.3 GB): SolveAutoLC -> GetRelativeTransform (solver.cc:630-649, 676-700) matches many
 * sources against one target in a row, and only the first of those calls pays the build.  Thread-safe. */
typedef struct nhip_csm_params {
  double scanner_range; /* ctor arg 1 (30) */
  double trans_range;   /* ctor arg 2 (2) */
  double low_res;       /* ctor arg 3 (0.3) */
  double high_res;      /* ctor arg 4 (0.01) */
  double sigma;         /* blur sigma in cells (2.0) */
  double floor_p;       /* likelihood floor (1e-10) */
  int32_t cell_bits;    /* 16 or 8 (0 = 16, as in nhip_grid_spec_t: scores within 1e-5 of an unquantised table) */
  int32_t reserved;
} nhip_csm_params_t;
/* The cache of nhip_csm_get_transformation: its byte cap (0 = keep nothing; entries beyond the new cap are freed), all
 * entries freed, and counters {entries, bytes held, hits, misses since the process started} (any pointer may be NULL). */
int nhip_csm_cache_configure(int64_t max_bytes);
int nhip_csm_cache_clear(void);
int nhip_csm_cache_stats(int64_t *entries, int64_t *bytes, int64_t *hits, int64_t *misses);
int nhip_csm_get_transformation(const nhip_csm_params_t *params, const float *pc_a, int32_t n_a, const float *pc_b,
                                int32_t n_b, double rot_a, double rot_b, double rot_restriction, double *score,
                                float *tx, float *ty, float *theta);

/* Residual batch: all LIDAR residual blocks of one ceres::Problem build (immutable after
 * creation, like the functors' copied vectors, slam_residuals.h:117-120). */
int nhip_resid_batch_create(int kind, const float *corr, const int32_t *block_offsets,
                            const int32_t *block_src, const int32_t *block_tgt, int32_t n_blocks,
                            int32_t n_poses, nhip_resid_batch_t **out);
/* poses: n_poses*3 doubles.  residuals: 2*n_corr; jac_src / jac_tgt: 6*n_corr or NULL. */
int nhip_resid_batch_eval(nhip_resid_batch_t *batch, const double *poses, double *residuals,
                          double *jac_src, double *jac_tgt);
/* The same evaluation with the target Jacobian in compact form: jac_tgt_theta holds 2 doubles per correspondence,
 * the theta column of its two rows.  The x and y columns of J_tgt are exactly the negated x and y columns of J_src
 * (dq/dt_t = -dq/dt_s), so a consumer rebuilds row i as (-J_src[i][0], -J_src[i][1], jac_tgt_theta[i]) while it
 * copies its slice: 80 instead of 112 bytes per correspondence cross PCIe. */
int nhip_resid_batch_eval_compact(nhip_resid_batch_t *batch, const double *poses, double *residuals,
                                  double *jac_src, double *jac_tgt_theta);
/* The same evaluation in its SMALLEST form over PCIe: per correspondence the residual pair and q = S2T p_s (the source point
 * in the target's frame, slam_residuals.h:78), per block the 8 constants {S2T's linear part l00 l01 l10 l11, its
 * translation tx ty, and i00 i01 of inverse(A(target_pose))'s linear part (i10 = -i01, i11 = i00)}.  Every Jacobian entry
 * ceres::AutoDiffCostFunction derives for these functors (slam_residuals.h:104-115, 160-171) is a closed form of q, those
 * constants and the correspondence's own points / normals, which the host holds: a consumer rebuilds the
 * rows of its block while it copies its slice -- nhip_resid_jacobians_from_q does exactly that, on the host, for `n` rows
 * of ONE block (corr: its n x 8 floats; q: its n x 2 doubles; block_consts: its 8 doubles; jac_src / jac_tgt: 6 n doubles
 * or NULL).  32 instead of 80 (compact) / 112 (full) bytes per correspondence cross PCIe; the Jacobians are
 * nhip_resid_batch_eval's bit for bit (u = L p_s is formed from the source point as the kernel forms it). */
int nhip_resid_batch_eval_q(nhip_resid_batch_t *batch, const double *poses, double *residuals, double *q, double *block_consts);
int nhip_resid_jacobians_from_q(int kind, const float *corr, const double *q, const double *block_consts, int64_t n,
                                double *jac_src, double *jac_tgt);
/* ONE block of the batch at explicitly given parameter blocks (source_pose[3], target_pose[3]): what a
 * ceres::CostFunction::Evaluate() called outside the batched evaluation point needs (Problem::Evaluate,
 * Covariance::Compute, a rejected trial step).  residuals: 2 n_b doubles; jac_src / jac_tgt: n_b x 2 rows of 3
 * doubles, either may be NULL. */
int nhip_resid_batch_eval_block(nhip_resid_batch_t *batch, int32_t block, const double *source_pose,
                                const double *target_pose, double *residuals, double *jac_src, double *jac_tgt);
int nhip_resid_batch_free(nhip_resid_batch_t *batch);

/* Page-locked host memory for buffers that cross PCIe every evaluation (device-to-host copies into pinned memory
 * run at the link rate; into pageable memory at about half of it). */
int nhip_host_alloc(size_t bytes, void **out);
int nhip_host_free(void *p);

/* Host-pointer forms of the two small functor families (OdometryResidual, slam_residuals.h:18-40:
 * one block per consecutive pose pair, solver.cc:370-387; PointToLineResidual, :180-200: HITL blocks,
 * solver.cc:515-532).  Same argument meaning as the *_dev entry points; poses / line_poses are
 * n x 3 doubles; outputs may be NULL where the *_dev form allows it.  They allocate, copy, launch
 * and synchronise per call (the inputs are a few KB). */
int nhip_resid_odometry(const float *t_odom, const float *r_odom, const int32_t *pose_i,
                        const int32_t *pose_j, int32_t n_factors, double translation_weight,
                        double rotation_weight, const double *poses, int32_t n_poses,
                        double *residuals, double *jac_i, double *jac_j);
/* nhip_resid_relpose_dev on host arrays (poses: n_poses x 3 doubles): pose ids are checked on the host (NHIP_ERR_ARG);
 * jac_i, jac_j, parts and flags may be NULL. */
int nhip_resid_relpose(const double *z, const double *info, const int32_t *pose_i, const int32_t *pose_j, int32_t n_factors,
                       const double *poses, int32_t n_poses, double *residuals, double *jac_i, double *jac_j, double *parts,
                       int32_t *flags);
int nhip_resid_point_to_line(const float *segments, const float *points, const int32_t *point_block,
                             int64_t n_points, const int32_t *block_pose, const int32_t *block_line,
                             int32_t n_blocks, const double *poses, int32_t n_poses,
                             const double *line_poses, int32_t n_line_poses, double *residuals,
                             double *jac_pose, double *jac_line);

/* ------------------------------------------------------------------ multi-GPU
 * The one collective of the path: every GPU matched its own shard of the candidate pairs
 * (pairs are independent; shard by target so a grid is built on exactly one GPU) and the
 * 16-byte records are all-gathered.  `comm` is the RCCL communicator (ncclComm_t, one rank
 * per GPU, created by the host with ncclCommInitRank) passed as void* so this header needs
 * no RCCL include; every rank contributes n_local records (pad the shards to equal length)
 * and receives world_size * n_local records ordered by rank.  librccl is bound on first use
 * (dlopen: the copy already loaded in the process if there is one), so single-GPU hosts
 * never need it.  A Python host does the same with torch.distributed (nautilus_amd/sharding.py). */
int nhip_allgather_matches(void *comm, const nhip_match_t *d_local, int32_t n_local,
                           nhip_match_t *d_all, void *stream);

/* ------------------------------------------------------------------ one instrument declared here
 * (the set of nautilus_hip_debug.h is closed -- tests/test_abi.py lists it name by name; read this one as part of it, after
 * nhip_bnb_stats_levels there.)  With NHIP_BNB_STATS=1, in the instrumented build: the chunk visits of the exact sums in the
 * kernels that keep a list of level-2 runs (the split form's candidates, the hand-over kernel; not the seeds), since the
 * last call -- a visit is one 64-entry chunk of a rotation's cell list taken by one pass.  out[0] = visits of the passes
 * on the 8-bit plane (a sub-block, two side by side, a whole block) if every pass took every chunk of the list, out[1] =
 * visits made: the passes leave out the chunks in which no entry has a level-2 byte that is not zero for a sub-block of
 * the pass, i.e. whose windows hold only empty cells; out[2], out[3] = the same two for the single poses of 16-bit grids
 * read from the 16-bit image.  out[1] == out[0] and out[3] == out[2] under NHIP_BNB_ZERO_CHUNKS=0 (synchronises; resets). */
int nhip_bnb_stats_chunks(uint64_t out[4]);
/* ... and, for the same reason here: the SEEDS of the kernel that takes a pair's bounds (every wave's highest-bound block,
 * evaluated exactly before anything is pruned), since the last call.  out[0..2] = shader-clock sums of the seed passes'
 * wave time by part: window origins, sub-block bounds, exact sums (in the split form nhip_bnb_stats_levels' out[5..7] add
 * the candidates' kernel's to these); out[3] = seed passes; out[4] = those that began while the pair's best sum was still 0
 * (no score gate, no other wave's seed landed yet); out[5] = those of out[4] that left their sub-block bounds out -- all of
 * them unless NHIP_BNB_SEED_BOUNDS=1 or a search without sub-block bounds; out[6] = seed blocks whose sub-block bounds were
 * taken and of which a sub-block that holds a pose had bound 0 -- what a pass without bounds evaluates in vain; out[7]
 * unused (synchronises; resets). */
int nhip_bnb_stats_seeds(uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* NAUTILUS_HIP_H_ */
