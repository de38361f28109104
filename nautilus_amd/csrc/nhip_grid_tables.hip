// nhip_grid_tables.hip -- K1 table build: what is derived from a slot's cells -- the skip map of the every-add kernels and
// the two max-pooled tables of the branch-and-bound matcher.
#include "nhip_grid.h"

namespace nhip {
namespace {
// ---- skip map ---------------------------------------------------------------------------
// A likelihood grid is zero except within the blur radius of a wall.  A wave of csm_correlate_kernel adds, per point, the
// CSM_WAVE_ROWS x CSM_ROW_DW-dword strip of the grid that starts at (window row, window column & ~3); on the 1081-beam scans
// ~45 % of those strips hold nothing but zeros.  The map stores one BIT per stored row r and aligned dword column c: "rows
// [r, r + 21) x dwords [c, c + 21) contain a non-zero cell" (bit c & 7 of byte c >> 3 of map row r, SKIP_PITCH(pitch) bytes
// per row), so the kernel can leave those strips out -- the sums are unchanged, bit for bit -- for one byte load per point.
// One block per 64-row x 64-dword map tile; tiles whose footprint touches no occupied blur tile stay on the memset's zeros.
constexpr int MT = 64, SK_ROWS = MT + CSM_WAVE_ROWS - 1;  // map tile side; grid rows feeding one map tile (84)
static_assert(2 * CSM_ROW_DW - 1 <= 64 && MT == 64, "row mask is built from two 64-lane ballots");

// CB = bytes per cell: a strip row spans ROW_DW = CB * CSM_ROW_DW aligned dwords (21 / 42; csm_correlate16_kernel starts its
// strips at 8-byte-aligned columns and looks up the even dword).  z = target index within the launch (t_base + blockIdx.z:
// for_z_slices).
template <int CB>
__global__ __launch_bounds__(256) void grid_skipmap_kernel(const uint8_t *__restrict__ occ, uint8_t *__restrict__ grids, GridGeom G,
                                                           int32_t t_base) {
  constexpr int ROW_DW = CB * CSM_ROW_DW, CPD = 4 / CB;  // (CPD: cells per dword)
  __shared__ unsigned long long sH[SK_ROWS];  // per grid row: bit c = a non-zero dword in [c0 + c, c0 + c + ROW_DW)
  const int32_t S = G.S, tiles = G.tiles, pad = G.pad, pitch = G.pitch, rows = G.rows;
  const int32_t t = t_base + blockIdx.z, tid = threadIdx.x;
  const int32_t r0 = blockIdx.y * MT, c0 = blockIdx.x * MT;  // first map row / dword column
  // footprint in raster coordinates -> blur tiles that could have written into it
  const int32_t fr0 = r0 - pad, fr1 = r0 + SK_ROWS - 1 - pad;
  const int32_t fc0 = CPD * c0 - pad, fc1 = CPD * (c0 + MT + ROW_DW - 1) - 1 - pad;
  int any = occ ? 0 : 1;  // (no occupancy bytes: the late build of the handle API computes every tile)
  if (occ && fr1 >= 0 && fr0 < S && fc1 >= 0 && fc0 < S) {
    const int32_t ty0 = max(fr0, 0) / TILE, ty1 = min(fr1, S - 1) / TILE;
    const int32_t tx0 = max(fc0, 0) / TILE, tx1 = min(fc1, S - 1) / TILE;
    const int32_t ntx = tx1 - tx0 + 1, nt = (ty1 - ty0 + 1) * ntx;
    for (int32_t i = tid; i < nt; i += 256)
      any |= occ[((size_t)t * tiles + ty0 + i / ntx) * tiles + tx0 + i % ntx];
  }
  if (!__syncthreads_or(any)) return;
  uint8_t *g = grids + (size_t)t * G.slot_bytes;
  uint8_t *M = g + G.skip_offset;
  const int32_t mpitch = G.mpitch;
  const int wave = tid >> 6, lane = tid & 63;
  // horizontal: (64 + ROW_DW - 1)-bit non-zero mask of a row (two ballots), then OR over windows of ROW_DW bits
  constexpr int UNR = 4;
  for (int32_t rb = wave * UNR; rb < SK_ROWS; rb += 4 * UNR) {
    uint32_t v0[UNR], v1[UNR];
#pragma unroll
    for (int u = 0; u < UNR; u++) {
      const int32_t r = r0 + rb + u;
      v0[u] = v1[u] = 0;
      if (rb + u < SK_ROWS && r < rows) {
        const uint32_t *row = reinterpret_cast<const uint32_t *>(g + (size_t)r * pitch);
        if (c0 + lane < mpitch) v0[u] = row[c0 + lane];
        if (lane < ROW_DW - 1 && c0 + 64 + lane < mpitch) v1[u] = row[c0 + 64 + lane];
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; u++) {
      const unsigned long long b0 = __ballot(v0[u] != 0u), b1 = __ballot(v1[u] != 0u);
      unsigned __int128 m = ((unsigned __int128)b1 << 64) | b0;
      m |= m >> 1;
      m |= m >> 2;
      m |= m >> 4;                                             // windows of 8
      unsigned __int128 mw = m | (m >> 8) | (m >> 13);         // [c, c+16) U [c+13, c+21): windows of 21
      if (CB == 2) mw |= mw >> 21;                             // windows of 42
      if (lane == 0 && rb + u < SK_ROWS) sH[rb + u] = (unsigned long long)mw;
    }
  }
  __syncthreads();
  // vertical: map row r = OR of the 21 row masks from r on; 64 bits = 8 map bytes
  if (tid < MT && r0 + tid < rows) {
    unsigned long long v = 0;
    for (int j = 0; j < CSM_WAVE_ROWS; j++) v |= sH[tid + j];
    *reinterpret_cast<unsigned long long *>(M + (size_t)(r0 + tid) * skip_pitch(pitch) + c0 / 8) = v;
  }
}
// ---- max-pooled tables (bounds of the branch-and-bound matcher, nhip_bnb.hip) --------------------------
// Level 1: pool[i][j] = max of the stored cells [8i, 8i + 15) x [8j, 8j + 15) (clipped to the image), one byte: the largest
// value an 8 x 8 block of translations can read for a point whose window origin has (row >> 3, col >> 3) = (i - Y, j - X).
// Level 2: [4i, 4i + 7) x [4j, 4j + 7), the same for a 4 x 4 sub-block, stored as byte pairs {P4[i][j], P4[i + 1][j]} (the two
// sub-block rows of a block in one read).  16-bit cells are scaled to a byte by ceil(max / 257), so 257 * pool >= max.  Level 2
// comes from the cells (grid_pool4_tiles_kernel, beside the blur whose list and tiled planes it reads), level 1 from level 2.
// Level 2 in BANDS (NHIP_GRID_POOL=bands: measurement; the product path is grid_pool4_tiles_kernel).  One block per (band of 8
// pooled rows, segment of 512 stored dwords, target): every thread walks the band's 8 * 4 + 3 stored rows down its dword columns
// keeping eight running maxima (a stored row feeds at most two pooled rows), the column maxima go to LDS and a 7-cell horizontal
// max finishes the entries.  Columns whose 64 x 64 blur tiles are all unoccupied hold only zeros and are not read (~80 % of a
// scan's image).
constexpr int POOL_BAND = 8, POOL_SEG_DW = 512, POOL_HALO_DW = 4;  // pooled rows per block, stored dwords per column segment, halo >= 7 cells * 2 bytes / 4

template <int CB>
__global__ __launch_bounds__(256) void grid_pool_kernel(const uint8_t *__restrict__ occ, uint8_t *__restrict__ grids, int32_t S,
                                                        int32_t tiles, int32_t pad, int32_t rows, int32_t pitch, int64_t table_offset,
                                                        int64_t slot_bytes, int32_t pool_pitch, int32_t t_base) {
  constexpr int ST = BNB_B4;
  constexpr int WIN = 2 * ST - 1;                    // cells a pooled entry spans per axis
  constexpr int ROWS_IN = POOL_BAND * ST + ST - 1;   // stored rows a band of pooled rows reads
  // column maxima per pooled row: 8-bit cells as two half-word planes (even bytes, odd bytes), 16-bit cells as is
  __shared__ uint32_t sM[POOL_BAND][CB == 1 ? 2 : 1][POOL_SEG_DW + POOL_HALO_DW];
  constexpr int CPD = 4 / CB;  // cells per dword
  const int32_t t = t_base + blockIdx.z, band = blockIdx.x, seg = blockIdx.y, tid = threadIdx.x;
  const uint8_t *g = grids + (size_t)t * slot_bytes;
  uint8_t *pool = grids + (size_t)t * slot_bytes + table_offset;
  const int32_t ndw = pitch / 4;
  const int32_t dw0 = seg * POOL_SEG_DW, dw1 = min(dw0 + POOL_SEG_DW + POOL_HALO_DW, ndw);
  const int32_t r0 = band * POOL_BAND * ST;
  // blur tiles the band's rows can touch
  const int32_t ty0 = max(r0 - pad, 0) / TILE, ty1 = min(r0 + ROWS_IN - 1 - pad, S - 1) / TILE;
  const bool rows_in = r0 + ROWS_IN - 1 - pad >= 0 && r0 - pad < S;
  int any = 0;
  for (int32_t c = dw0 + tid; c < dw1; c += 256) {
    uint32_t me[POOL_BAND], mo[POOL_BAND];
#pragma unroll
    for (int i = 0; i < POOL_BAND; i++) me[i] = mo[i] = 0u;
    const int32_t rc = c * CPD - pad;  // raster column of the dword's first cell (a dword never straddles tiles)
    bool live = rows_in && rc >= 0 && rc < S;
    if (live) {
      int o = 0;
      for (int32_t ty = ty0; ty <= ty1; ty++) o |= occ[((size_t)t * tiles + ty) * tiles + rc / TILE];
      live = o != 0;
    }
    if (live) {
#pragma unroll
      for (int rr = 0; rr < ROWS_IN; rr++) {
        // (rows past the image re-read its last row: zero border)
        const uint32_t w = reinterpret_cast<const uint32_t *>(g + (size_t)min(r0 + rr, rows - 1) * pitch)[c];
        const uint32_t we = CB == 1 ? (w & 0x00ff00ffu) : w, wo = CB == 1 ? ((w >> 8) & 0x00ff00ffu) : 0u;
        // pooled rows i with ST i <= rr < ST i + WIN
#pragma unroll
        for (int i = 0; i < POOL_BAND; i++) {
          if (ST * i <= rr && rr < ST * i + WIN) {
            me[i] = pk_max_u16(me[i], we);
            if (CB == 1) mo[i] = pk_max_u16(mo[i], wo);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < POOL_BAND; i++) {
      sM[i][0][c - dw0] = me[i];
      if (CB == 1) sM[i][1][c - dw0] = mo[i];
      any |= (me[i] | mo[i]) != 0u;
    }
  }
  if (!__syncthreads_or(any)) return;  // the memset's zeros stand
  const int32_t cells = rows;          // stored columns = stored rows (square image)
  const int32_t nj = (cells + ST - 1) / ST;
  constexpr int JSEG = POOL_SEG_DW * CPD / ST;  // pooled entries per segment
  const int32_t j0 = seg * JSEG;
  for (int32_t e = tid; e < POOL_BAND * JSEG; e += 256) {
    const int32_t i = e / JSEG, j = j0 + e % JSEG;
    if (j >= nj || band * POOL_BAND + i >= (rows + ST - 1) / ST) continue;
    uint32_t m = 0;
    const int32_t c1 = min(j * ST + WIN, cells);
    for (int32_t c = j * ST; c < c1; c++) {
      const int32_t d = c / CPD - dw0;
      uint32_t v;
      if (CB == 1) v = (sM[i][c & 1][d] >> (8 * (c & 2))) & 0xffu;  // byte c&3 of the dword: plane c&1, half-word (c>>1)&1
      else v = (sM[i][0][d] >> (16 * (c & 1))) & 0xffffu;
      m = max(m, v);
    }
    if (m) {
      const uint8_t v = (uint8_t)(CB == 1 ? m : (m + 256u) / 257u);
      const int32_t pi = band * POOL_BAND + i;
      // pairs: (i, 2j) = P4[i][j], (i, 2j + 1) = P4[i + 1][j]
      pool[(size_t)pi * pool_pitch + 2 * j] = v;
      if (pi > 0) pool[(size_t)(pi - 1) * pool_pitch + 2 * j + 1] = v;
    }
  }
}

// Level 1 from level 2: the window [8i, 8i + 15) x [8j, 8j + 15) of a level-1 entry is exactly the union of the nine level-2
// windows [4a, 4a + 7) x [4b, 4b + 7), a = 2i .. 2i + 2, b = 2j .. 2j + 2, and a maximum of maxima is the maximum (ceil(. / 257)
// is monotone, so the scaled bytes of 16-bit cells commute with it too): the 36 KB table is derived from the 286 KB one instead
// of from a second pass over the image (0.37 -> 0.03 ms per 1000 targets).
__global__ __launch_bounds__(256) void grid_pool8_from_pool4_kernel(uint8_t *__restrict__ grids, GridGeom G, int32_t t_base) {
  // one thread per four entries (i, 4q .. 4q + 3): five dwords of each of three level-2 rows in, one dword out
  const int32_t t = t_base + blockIdx.z, i = 4 * blockIdx.y + (threadIdx.x >> 6), q = blockIdx.x * 64 + (threadIdx.x & 63);
  const int32_t n8 = (G.rows + BNB_B - 1) / BNB_B;  // pooled rows = pooled columns (square image)
  if (i >= n8 || 4 * q >= n8) return;
  uint8_t *g = grids + (size_t)t * G.slot_bytes;
  const uint8_t *p4 = g + G.pool4_offset;
  uint32_t m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int da = 0; da < 3; da++) {
    // byte (a, 2 b) = P4[a][b]: for entry j, b = 2j, 2j + 1, 2j + 2 are bytes 4j, 4j + 2, 4j + 4 of row a
    const uint32_t *row = reinterpret_cast<const uint32_t *>(p4 + (size_t)(2 * i + da) * G.pool4_pitch) + 4 * q;
    uint32_t w[5];
#pragma unroll
    for (int d = 0; d < 5; d++) w[d] = row[d];
#pragma unroll
    for (int k = 0; k < 4; k++) m[k] = max(m[k], max(max(w[k] & 0xffu, (w[k] >> 16) & 0xffu), w[k + 1] & 0xffu));
  }
  // (entries past the table's n8 columns come out 0: their level-2 bytes are)
  *reinterpret_cast<uint32_t *>(g + G.pool_offset + (size_t)i * G.pool_pitch + 4 * q) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
}

// Level 1 from level 2 for the listed tiles only: the level-1 entries that read a level-2 entry a listed tile can have
// written (p8_range: ten per axis), each the full maximum of its nine level-2 entries, whoever wrote those.  Everything
// else in the table is zero (cleared the same way).
__global__ __launch_bounds__(128) void grid_pool8_tiles_kernel(const int32_t *__restrict__ count, const int32_t *__restrict__ list,
                                                               int32_t tiles, uint8_t *__restrict__ grids, int32_t pad, int32_t rows,
                                                               int64_t pool_offset, int64_t pool4_offset, int64_t slot_bytes,
                                                               int32_t pool_pitch, int32_t pool4_pitch) {
  const int32_t n_entries = *count;
  const int32_t n8 = (rows + BNB_B - 1) / BNB_B;
  for (int32_t e = blockIdx.x; e < n_entries; e += gridDim.x) {
    const ListedTile T = listed_tile(list[e], tiles);
    const int32_t pi0 = p4_first(T.r0(), pad), pj0 = p4_first(T.c0(), pad);
    int32_t i0, ni, j0, nj;
    p8_range(pi0, &i0, &ni);
    p8_range(pj0, &j0, &nj);
    uint8_t *g = grids + (size_t)T.t * slot_bytes;
    const uint8_t *p4 = g + pool4_offset;
    for (int32_t k = threadIdx.x; k < ni * nj; k += 128) {
      const int32_t i = i0 + k / nj, j = j0 + k % nj;
      if (i >= n8 || j >= n8) continue;
      uint32_t m = 0u;
#pragma unroll
      for (int da = 0; da < 3; da++) {
        const uint8_t *row = p4 + (size_t)(2 * i + da) * pool4_pitch + 4 * j;  // byte (a, 2 b) = P4[a][b]
        m = max(m, max(max((uint32_t)row[0], (uint32_t)row[2]), (uint32_t)row[4]));
      }
      g[pool_offset + (size_t)i * pool_pitch + j] = (uint8_t)m;
    }
  }
}
}  // namespace
void launch_skipmap(const GridGeom &G, const uint8_t *occ, uint8_t *g, int32_t n, hipStream_t s) {
  for_z_slices(n, [&](int32_t z0, int32_t nz) {
    hipLaunchKernelGGL(NHIP_BY_CELL_BYTES(grid_skipmap_kernel, G.cb), dim3((G.mpitch + MT - 1) / MT, (G.rows + MT - 1) / MT, nz),
                       dim3(256), 0, s, occ, g, G, z0);
  });
}

void launch_pool4_bands(const GridPass &P) {
  const GridGeom &G = P.G;
  const int32_t pooled_rows = (G.rows + BNB_B4 - 1) / BNB_B4;
  for_z_slices(P.n, [&](int32_t z0, int32_t nz) {
    hipLaunchKernelGGL(NHIP_BY_CELL_BYTES(grid_pool_kernel, G.cb),
                       dim3((pooled_rows + POOL_BAND - 1) / POOL_BAND, (G.mpitch + POOL_SEG_DW - 1) / POOL_SEG_DW, nz), dim3(256), 0,
                       P.s, P.occ, P.g, G.S, G.tiles, G.pad, G.rows, G.pitch, G.pool4_offset, G.slot_bytes, G.pool4_pitch, z0);
  });
}

void launch_pool8(const GridPass &P, bool whole) {
  const GridGeom &G = P.G;
  const int32_t n8 = (G.rows + BNB_B - 1) / BNB_B;
  if (!whole) hipLaunchKernelGGL(grid_pool8_tiles_kernel, dim3(P.blocks), dim3(128), 0, P.s, P.count, P.list, G.tiles, P.g, G.pad,
                                 G.rows, G.pool_offset, G.pool4_offset, G.slot_bytes, G.pool_pitch, G.pool4_pitch);
  else for_z_slices(P.n, [&](int32_t z0, int32_t nz) {
    hipLaunchKernelGGL(grid_pool8_from_pool4_kernel, dim3((n8 + 255) / 256, (n8 + 3) / 4, nz), dim3(256), 0, P.s, P.g, P.G, z0);
  });
}
}  // namespace nhip
