// nhip_grid_clear.hip -- K1 table build: the incremental rebuild.  A build leaves in the workspace the list of (target slot,
// 64 x 64 tile) entries it wrote and, in the header, a tag of the buffer it wrote them to.  nhip_grid_rebuild_dev clears exactly
// those tiles (image, and the plane of high bytes of 16-bit grids) instead of zero-filling gigabytes: ~20 % of a dense scan's
// tiles hold anything.  The tag is checked ON THE DEVICE (no host round trip): a header that does not describe this very buffer
// -- fresh or recycled workspace memory, another buffer, another geometry -- makes the same kernel clear everything instead.
#include "nhip_grid.h"

namespace nhip {
namespace {
constexpr uint64_t GRID_TAG_SEED = 0x9e3779b97f4a7c15ull;
// W = bytes per store the tiles' row starts allow ((pad * cell bytes) mod 16; tile columns are multiples of 64 cells)
template <int W> __device__ __forceinline__ void zero_store(uint8_t *p) {
  if (W == 16) *reinterpret_cast<uint4 *>(p) = make_uint4(0, 0, 0, 0);
  else if (W == 8) *reinterpret_cast<uint2 *>(p) = make_uint2(0, 0);
  else *reinterpret_cast<uint32_t *>(p) = 0u;
}
// rows [r0, r0 + 64) x bytes [col_byte, col_byte + row_bytes) of a plane of pitch `pitch`, clipped to the raster's rows
template <int W>
__device__ __forceinline__ void zero_tile(uint8_t *plane, int32_t pitch, int32_t r0, int32_t pad, int32_t S, int32_t col_byte,
                                          int32_t row_bytes) {
  const int per_row = row_bytes / W;
  for (int i = threadIdx.x; i < TILE * per_row; i += 256) {
    const int r = i / per_row, d = i % per_row;
    if (r0 + r < S) zero_store<W>(plane + (size_t)(r0 + r + pad) * pitch + col_byte + W * d);
  }
}

// header: the workspace's (its tag must equal `expect`, its counter is the list's length).  table_offset, table_bytes:
// the derived tables cleared whole in every slot (table_bytes 0: none); p4_pitch > 0: both pooled tables tile by tile.
// masks: null, or per list entry the lines of the tiled planes the previous build wrote inside the tile (grid_blur_kernel)
template <int W>
__global__ __launch_bounds__(256) void grid_clear_kernel(
    const int32_t *__restrict__ header, uint64_t expect, const int32_t *__restrict__ list, uint8_t *__restrict__ grids,
    int32_t n_targets, int32_t S, int32_t tiles, int32_t pad, int32_t pitch, int32_t cb, int64_t slot_bytes, int64_t table_offset,
    int64_t table_bytes, GridTiledPlanes tiled, int64_t p4_offset, int32_t p4_pitch, int64_t p8_offset, int32_t p8_pitch,
    int64_t hits_offset, int64_t hits_bytes, int32_t has_image, const uint32_t *__restrict__ masks) {
  const uint64_t tag = *reinterpret_cast<const uint64_t *>(header + 2);
  if (tag != expect) {  // unknown contents: everything goes (16-byte stores, grid-stride)
    uint4 *p = reinterpret_cast<uint4 *>(grids);
    const int64_t n16 = (int64_t)n_targets * slot_bytes / 16;  // (slot_bytes is a multiple of 16)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
    return;
  }
  // (1) the tiles the previous build wrote: 64 rows x 64 cells of the image and, for 16-bit cells, of the plane of high
  // bytes (a tile's last columns may lie in the raster's zero border: clearing them again is harmless)
  const int32_t n_entries = header[0];
  for (int32_t e = blockIdx.x; e < n_entries; e += gridDim.x) {
    const ListedTile T = listed_tile(list[e], tiles);
    const int32_t r0 = T.r0(), c0 = T.c0();
    uint8_t *g = grids + (size_t)T.t * slot_bytes;
    if (has_image) zero_tile<W>(g, pitch, r0, pad, S, (c0 + pad) * cb, TILE * cb);
    if (p4_pitch > 0) {
      // the second-level entries this tile's cells can have reached (grid_pool4_tiles_kernel: P4_NE x P4_NE entries from p4_first,
      // each also the second byte of the pair one row up): 18 rows x 17 byte pairs.  Entries elsewhere are zero already -- the image
      // is non-zero only inside listed tiles -- so the table as a whole (286 KB per slot at 1200 x 1200) is not rewritten.
      const int32_t pi0 = p4_first(r0, pad), pj0 = p4_first(c0, pad);
      for (int i = threadIdx.x; i < (P4_NE + 1) * P4_NE; i += 256) {
        const int32_t pi = pi0 - 1 + i / P4_NE, pj = pj0 + i % P4_NE;
        if (pi >= 0) *reinterpret_cast<uint16_t *>(g + p4_offset + (size_t)pi * p4_pitch + 2 * pj) = 0;
      }
      // ... and the first-level entries grid_pool8_tiles_kernel wrote for it
      int32_t i0, ni, j0, nj;
      p8_range(pi0, &i0, &ni);
      p8_range(pj0, &j0, &nj);
      for (int i = threadIdx.x; i < ni * nj; i += 256) g[p8_offset + (size_t)(i0 + i / nj) * p8_pitch + j0 + i % nj] = 0;
    }
    {
      // the tile's 64 x 64 cells in the matcher's tiled planes, 16 bytes (one tile row) a store where the tiles allow: pad and c0
      // are multiples of 16 columns here (W == 16), so per row the first copy of the high bytes takes four whole tile rows, the
      // shifted copy half a tile row + three whole + half, the 16-bit copy eight whole ones
      const uint32_t cc = (uint32_t)(c0 + pad);
      if (((c0 + pad) & 15) == 0) {
        using L0 = Lines<LINES_HI0>; using L1 = Lines<LINES_HI1>; using L2 = Lines<LINES_T16>;
        // 16-byte pieces per row: [0, D1) of the first copy, [D1, D2) of the shifted copy, then of the 16-bit copy
        constexpr int D1 = L0::COLS, D2 = L0::COLS + L1::COLS;
        const int per = cb == 2 ? D2 + (int)L2::COLS : D2;  // (8-bit cells: no tiled 16-bit copy)
        // the lines the previous build wrote (all of them without masks): the line masks of nhip_grid.h
        uint32_t mk[GRID_WS_MASK_WORDS];
#pragma unroll
        for (int k = 0; k < GRID_WS_MASK_WORDS; k++) mk[k] = masks ? masks[(size_t)e * GRID_WS_MASK_WORDS + k] : 0xffffffffu;
        for (int i = threadIdx.x; i < TILE * per; i += 256) {
          // (eight consecutive threads take the eight rows of one tile = the eight 16-byte pieces of one 128-byte line:
          //  row-by-row order sent every line to memory as eight partial writes)
          const int r = 8 * (i / (8 * per)) + (i & 7), d = (i >> 3) % per;
          if (r0 + r >= S) continue;
          const uint32_t row = (uint32_t)(r0 + r + pad), lr = (uint32_t)r >> 3;
          if (d < D1) {
            if (!line_written<LINES_HI0>(mk, lr * L0::COLS + (uint32_t)d)) continue;
            *reinterpret_cast<uint4 *>(tiled.hi(g, row, cc + 16u * (uint32_t)d, 0u)) = make_uint4(0, 0, 0, 0);
          } else if (d < D2) {
            const int k = d - D1;  // columns cc + 16 k - 8 ... of the plain plane = a tile row of the shifted copy
            if (!line_written<LINES_HI1>(mk, lr * L1::COLS + (uint32_t)k)) continue;
            uint8_t *q = tiled.hi(g, row, cc + 16u * (uint32_t)k, 1u) - 8;
            if (k == 0) *reinterpret_cast<uint2 *>(q + 8) = make_uint2(0, 0);
            else if (k == (int)L1::COLS - 1) *reinterpret_cast<uint2 *>(q) = make_uint2(0, 0);
            else *reinterpret_cast<uint4 *>(q) = make_uint4(0, 0, 0, 0);
          } else {
            if (!line_written<LINES_T16>(mk, lr * L2::COLS + (uint32_t)(d - D2))) continue;
            *reinterpret_cast<uint4 *>(tiled.t16(g, row, cc + 8u * (uint32_t)(d - D2))) = make_uint4(0, 0, 0, 0);
          }
        }
      } else {  // (odd geometries: a dword / four cells at a time)
        for (int i = threadIdx.x; i < TILE * (TILE / 4) * 3; i += 256) {
          const int k = i % 3, d = (i / 3) % (TILE / 4), r = (i / 3) / (TILE / 4);
          if (r0 + r >= S) continue;
          const uint32_t row = (uint32_t)(r0 + r + pad), col = cc + 4u * (uint32_t)d;
          if (k < 2) *reinterpret_cast<uint32_t *>(tiled.hi(g, row, col, (uint32_t)k)) = 0u;
          else if (cb == 2) *reinterpret_cast<uint2 *>(tiled.t16(g, row, col)) = make_uint2(0u, 0u);
        }
      }
    }
  }
  // (2) the derived tables of every slot (skip map, both pooled tables: between the image and the plane of high bytes)
  const int64_t per_slot = table_bytes / 16;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_slot * n_targets; i += (int64_t)gridDim.x * 256)
    *reinterpret_cast<uint4 *>(grids + (i / per_slot) * slot_bytes + table_offset + 16 * (i % per_slot)) = make_uint4(0, 0, 0, 0);
  // (3) the hit rasters, whole: 200 KB per slot in 16-byte stores.  (Tile by tile -- two dwords per row and tile, every
  // row another 128-byte line -- the same bits cost 0.10 ms per 1000 targets as partial line writes; this way 0.04.)
  const int64_t hits16 = hits_bytes / 16;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hits16 * n_targets; i += (int64_t)gridDim.x * 256)
    *reinterpret_cast<uint4 *>(grids + (i / hits16) * slot_bytes + hits_offset + 16 * (i % hits16)) = make_uint4(0, 0, 0, 0);
}

__global__ void grid_tag_kernel(int32_t *header, uint64_t tag) { *reinterpret_cast<uint64_t *>(header + 2) = tag; }
}  // namespace
uint64_t grid_tag(const void *d_grids, int64_t n_targets, const GridLayout &L, int32_t flags) {
  uint64_t h = GRID_TAG_SEED;
  const uint64_t v[6] = {(uint64_t)(uintptr_t)d_grids, (uint64_t)n_targets, (uint64_t)L.slot_bytes, (uint64_t)L.S,
                         (uint64_t)L.cb, (uint64_t)flags};
  for (uint64_t x : v) {
    h ^= x + GRID_TAG_SEED + (h << 6) + (h >> 2);
    h *= 0xff51afd7ed558ccdull;
  }
  return h | 1ull;  // (never 0: a zeroed header is never valid)
}

// The tiles the previous build wrote (or everything, if the header does not vouch for this buffer), then the derived
// tables between the image and the plane of high bytes: with a skip map, the map and the two pooled tables, whole, in
// every slot; without one only the pooled tables, tile by tile (nothing reads the map's space).
void launch_clear(const GridPass &P, uint64_t tag, bool with_map) {
  const GridGeom &G = P.G;
  const int64_t table_offset = with_map ? G.skip_offset : G.pool4_offset;
  const int64_t table_bytes = with_map ? G.tiled.offset - G.skip_offset : 0;
  const int w = (G.pad * G.cb) % 16 == 0 ? 16 : ((G.pad * G.cb) % 8 == 0 ? 8 : 4);
  const auto kernel = w == 16 ? grid_clear_kernel<16> : (w == 8 ? grid_clear_kernel<8> : grid_clear_kernel<4>);
  hipLaunchKernelGGL(kernel, dim3(4096), dim3(256), 0, P.s, P.count, tag, P.list, P.g, P.n, G.S, G.tiles, G.pad, G.pitch, G.cb,
                     G.slot_bytes, table_offset, table_bytes, G.tiled, G.pool4_offset, with_map ? 0 : G.pool4_pitch, G.pool_offset,
                     G.pool_pitch, G.hits_offset, G.hits_bytes, G.has_image, P.masks);
}

void launch_tag(const GridPass &P, uint64_t tag) { hipLaunchKernelGGL(grid_tag_kernel, dim3(1), dim3(1), 0, P.s, P.count, tag); }
}  // namespace nhip
