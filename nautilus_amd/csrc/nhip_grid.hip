// nhip_grid.hip -- K1, the likelihood-table build: the host driver (nhip_grid.h: what is built, the kernels' units).  A call goes
// in passes of as many targets as the workspace holds; per pass: clear (memset, or on a rebuild grid_clear_kernel) ->
// grid_occupancy_list_kernel -> grid_blur_kernel<CB> -> (grid_skipmap_kernel<CB>) -> grid_pool4_tiles_kernel<CB> -> level 1
// (grid_pool8_tiles_kernel or grid_pool8_from_pool4_kernel)
#include "nhip_grid.h"

namespace nhip {
int launch_grid_build(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_target_ids, int32_t n_targets,
                      const nhip_grid_spec_t *spec, const GridLayout &L, uint8_t *d_grids, void *d_ws, int64_t ws_bytes, hipStream_t s,
                      bool incremental) {
  NHIP_REQUIRE(L.R <= MAX_R, "grid_build: blur radius %d > %d (sigma too large)", L.R, MAX_R);
  NHIP_REQUIRE(L.K * L.K < (1ll << 32), "grid_build: tap sum overflows 32-bit accumulation");
  NHIP_REQUIRE(L.pitch % 4 == 0, "grid_build: pitch must be a multiple of 4");
  const GridGeom G = grid_geom(L, spec);
  const int64_t tiles2 = (int64_t)G.tiles * G.tiles;
  // workspace: 256-byte header (list counter, tag) | [16-bit cells: threshold table] | of a pass: tile occupancy bytes | tile list | line masks
  const int64_t per = grid_ws_per_target(L.S);
  const int64_t fixed = GRID_WS_HEADER + (L.cb == 2 ? GRID_WS_THR16 : 0);
  const int64_t chunk = (ws_bytes - fixed - 4) / per;
  NHIP_REQUIRE(chunk >= 1, "grid_build: workspace %lld B < one target (%lld B)", (long long)ws_bytes, (long long)(per + fixed + 4));
  GridTables T;
  int rc = make_tables(spec, L, &T);
  if (rc) return rc;
  GridKernelTables kt;
  memset(&kt, 0, sizeof(kt));
  for (int i = 0; i <= 2 * L.R; i++) kt.taps[i] = T.taps[i];
  for (int i = 0; i < 256; i++) kt.thr[i] = T.thr[i];
  uint8_t *const base = static_cast<uint8_t *>(d_ws);
  uint32_t *d_thr16 = nullptr;
  if (L.cb == 2) {
    // fit of the guess through two entries at the top of the table, where the integer thresholds are large and their
    // rounding does not matter (through thr16[16384] = 9 the guess was 75 steps off); a hint only: the table decides
    const double t1 = (double)T.thr16[57344], t2 = (double)T.thr16[65535];
    if (t1 >= 1.0 && t2 > t1) {
      const double a = (65535.0 - 57344.0) / (log(t2) - log(t1));
      kt.q16_a = (float)a;
      kt.q16_b = (float)(57344.0 - a * log(t1));
    }
    // the table travels with the launch (the caller owns the workspace; nothing is allocated here)
    d_thr16 = reinterpret_cast<uint32_t *>(base + GRID_WS_HEADER);
    NHIP_TRY_HIP(hipMemcpyAsync(d_thr16, T.thr16, GRID_WS_THR16, hipMemcpyHostToDevice, s));
  }
  // The skip map serves the every-add kernels; 16-bit grids -- the branch-and-bound matcher's -- carry one only when the spec asks.
  const bool with_map = L.has_image && (L.cb == 1 || (spec->flags & NHIP_GRID_SKIP_MAP));
  // second-level table from the listed tiles, or (NHIP_GRID_POOL=bands: measurement) by the band kernel, which walks the image
  const char *pk = tunable("NHIP_GRID_POOL");
  const bool bands = pk && pk[0] == 'b' && L.has_image;
  // one pass over all targets leaves a complete tile list behind: only then can the next build be incremental
  const bool one_pass = chunk >= n_targets;
  const bool rebuild = incremental && one_pass;
  const uint64_t tag = grid_tag(d_grids, n_targets, L, spec->flags);
  GridPass P = {G, reinterpret_cast<const float2 *>(d_xy), d_offsets, d_target_ids, n_scans, dev_status()};  // (each pass sets its own)
  P.count = reinterpret_cast<int32_t *>(base);
  P.occ = base + fixed;
  P.s = s;
  timer_begin(NHIP_TIMER_GRID, s);
  for (int64_t t0 = 0; t0 < n_targets; t0 += chunk) {
    P.g = d_grids + (size_t)t0 * L.slot_bytes;
    P.t0 = (int32_t)t0;
    P.n = (int32_t)((n_targets - t0 < chunk) ? (n_targets - t0) : chunk);
    P.list = reinterpret_cast<int32_t *>(P.occ + (((size_t)P.n * tiles2 + 3) & ~(size_t)3));
    // line masks behind the list, for geometries whose tiles start on line boundaries of the tiled planes
    P.masks = L.pad % 16 == 0 ? reinterpret_cast<uint32_t *>(P.list + (size_t)P.n * tiles2) : nullptr;
    P.blocks = (int32_t)(P.n * tiles2 < 8192 ? P.n * tiles2 : 8192);  // persistent over the list
    timer_begin(NHIP_TIMER_GRID_CLEAR, s);
    if (rebuild) launch_clear(P, tag, with_map);
    else NHIP_TRY_HIP(hipMemsetAsync(P.g, 0, (size_t)P.n * L.slot_bytes, s));
    // counter (and tag: the buffer is in flux until this build is through)
    NHIP_TRY_HIP(hipMemsetAsync(base, 0, GRID_WS_HEADER, s));
    timer_end(NHIP_TIMER_GRID_CLEAR, s);
    launch_list_and_blur(P, kt, d_thr16);
    if (with_map) launch_skipmap(G, P.occ, P.g, P.n, s);
    if (bands) launch_pool4_bands(P);
    else launch_pool4_tiles(P);
    // level 1 from level 2: the whole table on first builds (the memset covers it anyway, but the handle API's late builds have
    // no list), after the band kernel and for grids with a map, whose clear zeroes every derived table; else the listed tiles' entries
    launch_pool8(P, bands || with_map || !rebuild);
    if (one_pass) launch_tag(P, tag);
  }
  timer_end(NHIP_TIMER_GRID, s);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_skipmap_build(uint8_t *d_grids, int32_t n_grids, const GridLayout &L, hipStream_t s) {
  launch_skipmap(grid_geom(L, nullptr), nullptr, d_grids, n_grids, s);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}
}  // namespace nhip
