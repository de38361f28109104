// nhip_grid.h -- K1, the likelihood-table build: what its units share.  The build replaces the lookup table that
// CorrelativeScanMatcher rasterises from the target cloud (call site src/optimization/solver.cc:633-638; geometry
// src/visualization/cimg_debug.h:20-64).  Spec: hit raster -> exact integer separable Gaussian blur
// -> floor, natural log, 8- or 16-bit quantisation (by an integer threshold table, so the grid is bit-identical to the
// CPU formulation).  Stored with a zero border of `pad` cells so the correlation kernel never bounds-checks.  HBM-bound byte
// work: per target the slot is zero-filled (on a rebuild: the tiles of the build before are cleared) and the ~20 % of 64x64
// tiles within blur reach of a hit are computed; no intermediate raster.  Units: nhip_grid_blur.hip (tile list; per listed
// tile the cells, tiled planes, hit raster, level 2), nhip_grid_tables.hip (of a whole slot: skip map, band form of level 2,
// level 1 from level 2), nhip_grid_clear.hip (the incremental rebuild), nhip_grid.hip (the host driver).
#pragma once
#include "nhip_common.h"

namespace nhip {
constexpr int TILE = 64, MAX_R = 16, TH_MAX = TILE + 2 * MAX_R;  // tile side, largest blur radius, a tile's neighbourhood (96)
struct GridKernelTables {
  int32_t taps[2 * MAX_R + 1];
  uint32_t thr[256];
  float q16_a, q16_b;  // 16-bit cells: q ~ q16_a * ln(sum) + q16_b, the first guess of the table search
};
// ---- the geometry block: what the kernels read of a GridLayout, by value --------------------------------
// The matcher's tiled planes inside a slot (nhip_common.h, hi_tiled / t16_tiled): two copies of the 8-bit plane, then the
// 16-bit image tiled 8 rows x 8 cells.  g = the slot's first byte.
struct GridTiledPlanes {
  int64_t offset, copy_bytes;  // of the first copy in the slot; bytes of one copy of the 8-bit plane
  int32_t hi_tpr, t16_tpr;     // tiles per tile row
  template <class Byte> __device__ __forceinline__ Byte *hi(Byte *g, uint32_t row, uint32_t col, uint32_t cp) const {
    return g + offset + hi_tiled(row, col, cp, (uint32_t)hi_tpr, (uint32_t)copy_bytes);
  }
  template <class Byte> __device__ __forceinline__ Byte *t16(Byte *g, uint32_t row, uint32_t col) const {
    return g + offset + 2 * copy_bytes + t16_tiled(row, col, (uint32_t)t16_tpr);
  }
};
struct GridGeom {
  double res, inv_res;  // metres per cell and its rounded reciprocal (0 without a spec: for kernels that read cells, not points)
  int64_t slot_bytes, skip_offset, pool_offset, pool4_offset, hits_offset, hits_bytes;  // (the image is at 0)
  GridTiledPlanes tiled;
  int32_t S, pad, pitch, rows, tiles;  // raster side, border, bytes per image row, stored rows S + 2 pad, tiles per axis
  int32_t R, cb, has_image;            // blur radius, bytes per cell, 0 with NHIP_GRID_NO_IMAGE
  int32_t pool_pitch, pool4_pitch, hits_pitch, mpitch;  // (mpitch: dwords per image row, pitch / 4)
};
inline GridGeom grid_geom(const GridLayout &L, const nhip_grid_spec_t *spec) {
  GridGeom G;
  G.res = spec ? spec->res : 0.0, G.inv_res = spec ? 1.0 / spec->res : 0.0;
  G.slot_bytes = L.slot_bytes, G.skip_offset = L.skip_offset, G.pool_offset = L.pool_offset, G.pool4_offset = L.pool4_offset;
  G.hits_offset = L.hits_offset, G.hits_bytes = L.hits_bytes, G.hits_pitch = L.hits_pitch;
  G.tiled.offset = L.hi_offset, G.tiled.copy_bytes = L.hi_copy_bytes, G.tiled.hi_tpr = L.hi_tpr, G.tiled.t16_tpr = L.t16_tpr;
  G.S = L.S, G.pad = L.pad, G.pitch = L.pitch, G.mpitch = L.pitch / 4, G.rows = L.S + 2 * L.pad, G.tiles = (L.S + TILE - 1) / TILE;
  G.R = L.R, G.cb = L.cb, G.has_image = L.has_image ? 1 : 0, G.pool_pitch = L.pool_pitch, G.pool4_pitch = L.pool4_pitch;
  return G;
}
// ---- one pass of a build: targets [t0, t0 + n) of the call, their slots, their part of the workspace ----
struct GridPass {
  GridGeom G;
  const float2 *xy;  // the call's scans and target ids (device memory); status: the device's status words, for ids out of range
  const int32_t *offsets, *target_ids;
  int32_t n_scans;
  uint32_t *status;
  uint8_t *g;        // slot of target t0
  int32_t t0, n;
  int32_t *count;    // the workspace's header: [0] list counter, [2..3] tag
  uint8_t *occ;      // one byte per (target, tile)
  int32_t *list;     // occupied (target, tile) pairs: entry = target * tiles^2 + tile
  uint32_t *masks;   // GRID_WS_MASK_WORDS per list entry, or null (geometries whose tiles do not start on line boundaries)
  int32_t blocks;    // workgroups of the kernels that are persistent over the list
  hipStream_t s;
};
// nhip_grid_blur.hip: tile list, then the listed tiles' cells; level 2 of the pooled tables from the listed tiles
void launch_list_and_blur(const GridPass &P, const GridKernelTables &tab, const uint32_t *thr16);
void launch_pool4_tiles(const GridPass &P);
// nhip_grid_tables.hip: skip maps (occ null: every map tile); level 2 by the band kernel; level 1, whole or the listed tiles' entries
void launch_skipmap(const GridGeom &G, const uint8_t *occ, uint8_t *g, int32_t n, hipStream_t s);
void launch_pool4_bands(const GridPass &P);
void launch_pool8(const GridPass &P, bool whole);
// nhip_grid_clear.hip
uint64_t grid_tag(const void *d_grids, int64_t n_targets, const GridLayout &L, int32_t flags);
void launch_clear(const GridPass &P, uint64_t tag, bool with_map);
void launch_tag(const GridPass &P, uint64_t tag);
// Cell-width dispatch: the instance of a kernel template <int CB> for cells of cb bytes.
#define NHIP_BY_CELL_BYTES(kernel, cb) ((cb) == 1 ? kernel<1> : kernel<2>)
// gridDim.z is limited to 65,535: the targets of a pass go to kernels whose z is the target in slices, launch(z0, nz).
template <class Launch> inline void for_z_slices(int32_t n, Launch launch) {
  constexpr int32_t MAX_Z = 65535;
  for (int32_t z0 = 0; z0 < n; z0 += MAX_Z) launch(z0, n - z0 < MAX_Z ? n - z0 : MAX_Z);
}
// ---- tiles ------------------------------------------------------------------------------------------------
// tiles^2 bits of a target in LDS words (grid_occupancy_list_kernel): sized for the largest side make_layout admits
constexpr int OCC_WORDS_MAX = 2048, GRID_MAX_TILES = (GRID_MAX_SIDE + TILE - 1) / TILE;
static_assert(GRID_MAX_TILES * GRID_MAX_TILES <= 32 * OCC_WORDS_MAX, "the occupancy bitmap holds every tile of the largest side");
// The image is non-zero only inside listed tiles, so only level-2 entries whose 7 x 7 window meets a listed tile can be
// non-zero: per tile and axis the P4_NE entries that start between 4 cells before it and its last cell, over P4_REG cells.
constexpr int P4_NE = TILE / BNB_B4 + 1, P4_REG = BNB_B4 * (P4_NE - 1) + 2 * BNB_B4 - 1;  // 17 entries, 71 cells per axis
// ---- line masks ------------------------------------------------------------------------------------------
// Per list entry GRID_WS_MASK_WORDS words: which 128-byte lines of the three tiled planes the blur wrote inside the tile
// (geometries whose tiles start on line boundaries).  A tile has TILE / 8 rows of eight; per row of eight lr the first copy of
// the 8-bit plane has 4 lines (16-byte columns k), the copy shifted by 8 columns 5 (half, three whole, half), the 16-bit copy 8
// (8-cell columns).  Line (lr, k) of a plane is bit lr * COLS + k of the plane's bits, and every plane starts on a word.  Written
// by the tail of grid_blur_kernel, read by grid_clear_kernel.
enum LinePlane : int { LINES_HI0 = 0, LINES_HI1 = 1, LINES_T16 = 2 };
template <int P> struct Lines {
  static constexpr uint32_t COLS = P == LINES_HI0 ? TILE / 16 : (P == LINES_HI1 ? TILE / 16 + 1 : TILE / 8);  // lines per row of eight
  static constexpr uint32_t COUNT = (TILE / 8) * COLS, WORDS = (COUNT + 31u) / 32u;                            // 32 / 40 / 64 lines
  static constexpr uint32_t FIRST = Lines<P - 1>::FIRST + Lines<P - 1>::COUNT;  // the plane's first line among all of a tile's
  static constexpr uint32_t WORD0 = Lines<P - 1>::WORD0 + Lines<P - 1>::WORDS;  // the plane's first mask word
};
template <> struct Lines<-1> { static constexpr uint32_t COUNT = 0, WORDS = 0, FIRST = 0, WORD0 = 0; };
constexpr uint32_t LINE_COUNT_ALL = Lines<LINES_T16>::FIRST + Lines<LINES_T16>::COUNT;  // one thread per line: 136
static_assert(Lines<LINES_T16>::WORD0 + Lines<LINES_T16>::WORDS <= (uint32_t)GRID_WS_MASK_WORDS, "the line masks of a tile fit their words");
static_assert(Lines<LINES_HI0>::WORDS == 1 && Lines<LINES_HI1>::WORDS == 2 && Lines<LINES_T16>::WORDS == 2, "both sides index a plane's words so");

// Cell of a point (cimg_debug.h:31-37: side/2 + floor(x / resolution), float promoted to double);
// false for non-finite points and cells outside the grid (dropped, cimg_debug.h:48-50).
__device__ __forceinline__ bool hit_cell(float2 q, int32_t S, double res, double inv_res, int32_t *c, int32_t *r) {
  if (!(fabsf(q.x) < 1e9f) || !(fabsf(q.y) < 1e9f)) return false;
  const double fc = floor_quotient((double)q.x, res, inv_res), fr = floor_quotient((double)q.y, res, inv_res);
  const double half = (double)(S / 2);
  if (!(fc >= -half && fc < (double)S - half && fr >= -half && fr < (double)S - half)) return false;
  *c = S / 2 + (int32_t)fc;
  *r = S / 2 + (int32_t)fr;
  return true;
}
// The points of target scan `scan` (an id read from device memory): an id outside [0, n_scans) is an EMPTY scan -- its
// grid comes out all floor -- and is reported through the device's status words (nhip_dev_status), never dereferenced.
__device__ __forceinline__ void target_points(const int32_t *__restrict__ offsets, int32_t n_scans, int32_t scan, int32_t index,
                                              uint32_t *status, bool report, int32_t *beg, int32_t *end) {
  *beg = *end = 0;
  if (id_in(scan, n_scans)) {
    *beg = offsets[scan];
    *end = offsets[scan + 1];
  } else if (report) {
    flag_bad_id(status, BAD_TARGET_ID, scan, index);
  }
}
// A list entry: the target's index in the pass, and the tile's first raster row and column (formed where they are used)
struct ListedTile {
  int32_t t, tile, tiles;
  __device__ __forceinline__ int32_t r0() const { return (tile / tiles) * TILE; }
  __device__ __forceinline__ int32_t c0() const { return (tile % tiles) * TILE; }
};
__device__ __forceinline__ ListedTile listed_tile(int32_t entry, int32_t tiles) {
  return ListedTile{entry / (tiles * tiles), entry % (tiles * tiles), tiles};
}
// First level-2 entry (row or column) the tile that starts at raster cell c0 can reach: four cells before the tile
// (pad is a multiple of 4 and >= 16: never negative); P4_NE entries from there.
__device__ __forceinline__ int32_t p4_first(int32_t c0, int32_t pad) { return (c0 + pad) / BNB_B4 - 1; }
// ... and the level-1 entries that read one of them (level-2 rows p0 .. p0 + 16 feed level-1 rows (p0 - 1) >> 1 .. (p0 + 16) >> 1: ten)
__device__ __forceinline__ void p8_range(int32_t p0, int32_t *lo, int32_t *n) {
  *lo = (p0 - 1) >> 1;
  *n = ((p0 + P4_NE - 1) >> 1) - *lo + 1;
}
// whether the masks mk of a list entry name line b = lr * COLS + k of plane P
template <int P> __device__ __forceinline__ bool line_written(const uint32_t (&mk)[GRID_WS_MASK_WORDS], uint32_t b) {
  const uint32_t w = Lines<P>::WORDS == 1 ? mk[Lines<P>::WORD0] : (b < 32u ? mk[Lines<P>::WORD0] : mk[Lines<P>::WORD0 + 1]);
  return (w >> (Lines<P>::WORDS == 1 ? b : b & 31u)) & 1u;
}
// max of the two half-words of a and b
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  const us2 r = __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
  return __builtin_bit_cast(uint32_t, r);
}

}  // namespace nhip
