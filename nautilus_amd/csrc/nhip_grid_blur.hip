// nhip_grid_blur.hip -- K1 table build: the list of occupied tiles, and per listed tile the cells (image, the matcher's
// tiled planes), the hit raster and the line masks of the next rebuild's clear.
#include "nhip_grid.h"

namespace nhip {
namespace {
// One block per target scan: mark every 64x64 tile whose blur halo contains a hit, in an LDS bitmap; every occupancy byte of the
// target is written (no memset of the array), and the block appends its occupied tiles to the list with ONE atomic on the
// counter.  (There is no hit raster to start from: the blur kernel gathers a tile's hits straight from the point list.)  Entries
// of one target are consecutive and ascending; targets come in the order their blocks finish.
__global__ __launch_bounds__(256) void grid_occupancy_list_kernel(
    const float2 *__restrict__ xy, const int32_t *__restrict__ offsets, const int32_t *__restrict__ target_ids, int32_t t0,
    uint8_t *__restrict__ occ, GridGeom G, int32_t *__restrict__ count, int32_t *__restrict__ list, int32_t n_scans,
    uint32_t *__restrict__ status) {
  __shared__ uint32_t sBits[OCC_WORDS_MAX];  // (nhip_grid.h: holds the tiles of the largest side a layout can have)
  __shared__ int32_t sBase, sN;
  const int32_t S = G.S, tiles = G.tiles, R = G.R;
  const int32_t t = blockIdx.x, nt = tiles * tiles, nw = (nt + 31) / 32;
  int32_t beg, end;
  target_points(offsets, n_scans, target_ids[t0 + t], t0 + t, status, threadIdx.x == 0, &beg, &end);
  for (int i = threadIdx.x; i < nw; i += 256) sBits[i] = 0u;
  if (threadIdx.x == 0) sN = 0;
  __syncthreads();
  for (int32_t p = beg + threadIdx.x; p < end; p += 256) {
    int32_t c, r;
    if (!hit_cell(xy[p], S, G.res, G.inv_res, &c, &r)) continue;
    // tiles whose (tile + blur halo) contains this cell: at most 2 x 2 (R <= 16 < TILE)
    const int tx0 = max(c - R, 0) / TILE, tx1 = min(c + R, S - 1) / TILE;
    const int ty0 = max(r - R, 0) / TILE, ty1 = min(r + R, S - 1) / TILE;
    for (int ty = ty0; ty <= ty1; ty++)
      for (int tx = tx0; tx <= tx1; tx++) {
        const int k = ty * tiles + tx;
        atomicOr(&sBits[k >> 5], 1u << (k & 31));
      }
  }
  __syncthreads();
  // occupancy bytes (the skip map's and the band kernels' input), and this thread's words' share of the list
  uint8_t *o = occ + (size_t)t * nt;
  for (int i = threadIdx.x; i < nt; i += 256) o[i] = (uint8_t)((sBits[i >> 5] >> (i & 31)) & 1u);
  int32_t mine = 0;
  for (int w = threadIdx.x; w < nw; w += 256) mine += __builtin_popcount(sBits[w]);
  const int32_t at = mine ? atomicAdd(&sN, mine) : 0;  // (order inside the target's segment: by thread, then ascending)
  __syncthreads();
  if (threadIdx.x == 0) sBase = sN ? atomicAdd(count, sN) : 0;
  __syncthreads();
  int32_t k = sBase + at;
  for (int w = threadIdx.x; w < nw; w += 256) {
    uint32_t m = sBits[w];
    while (m) {
      const int b = __builtin_ctz(m);
      m &= m - 1u;
      list[k++] = t * nt + 32 * w + b;
    }
  }
}

// 64x64 output tile per list entry.  ~95 % of the tiles of a scan's grid see no hit within their blur halo, so the kernel runs as
// a persistent grid over the list of occupied (target, tile) pairs.  The hit raster is sparse (a few dozen hits per tile), so the
// separable blur is evaluated as a scatter: every hit of the tile's (64 + 2R)^2 neighbourhood adds taps[i] * taps[j] to the
// (2R+1)^2 outputs around it (LDS integer atomics -- the same integer sum as the two-pass form, in any order), ~170 adds per hit
// instead of 29 multiply-adds per OUTPUT; then the non-zero sums are quantised by search of the threshold table and stored as
// aligned dwords.  Grid memory is pre-zeroed.
constexpr int MAX_TILE_HITS = TH_MAX * TH_MAX, SEEN_WORDS = (MAX_TILE_HITS + 31) / 32;  // every cell of the neighbourhood a hit; a bit each
constexpr int GROUPS = TILE / 4;                       // groups of four columns per row of the tile
constexpr int TURNS = TILE * GROUPS / 256, GROUP = 2;  // a thread quantises one group per turn; turns go in groups of GROUP
static_assert(TURNS % GROUP == 0, "whole groups of turns");
// CB = bytes per cell.  8-bit cells: 256-entry threshold table passed by value (LDS copy); 16-bit cells: the 65536-entry table
// lives in the workspace (thr16, L2-resident).  masks: null, or GRID_WS_MASK_WORDS words per list entry -- the lines of the tiled
// planes this build writes inside the entry's tile (tiles that start on line boundaries: pad a multiple of 16), for the next clear
template <int CB>
__global__ __launch_bounds__(256) void grid_blur_kernel(
    const float2 *__restrict__ xy, const int32_t *__restrict__ offsets, const int32_t *__restrict__ target_ids, int32_t t0,
    const int32_t *__restrict__ count, const int32_t *__restrict__ list, int32_t tiles, uint8_t *__restrict__ grids, int32_t S,
    int32_t pad, int32_t pitch, int64_t slot_bytes, int32_t R, double res, double inv_res, GridKernelTables tab,
    const uint32_t *__restrict__ thr16, int64_t hi_offset, int32_t hi_tpr, int64_t hi_copy_bytes, int32_t t16_tpr, int32_t n_scans,
    int64_t hits_offset, int32_t hits_pitch, int32_t has_image, uint32_t *__restrict__ masks) {
  __shared__ uint32_t sMask[GRID_WS_MASK_WORDS];
  __shared__ unsigned long long sBal[2][TILE / 4];  // per four rows of the tile: lanes = (row & 3) * 16 + group of four columns
  __shared__ uint32_t sA[TILE][TILE + 1];
  __shared__ uint16_t sHits[MAX_TILE_HITS];
  __shared__ uint32_t sSeen[SEEN_WORDS];  // one bit per neighbourhood cell: a cell is a hit once
  __shared__ uint32_t sThr[256];
  __shared__ int32_t sTaps[2 * MAX_R + 1];
  __shared__ int32_t sNH;
  if (CB == 1) sThr[threadIdx.x] = tab.thr[threadIdx.x];
  if (threadIdx.x <= 2 * R) sTaps[threadIdx.x] = tab.taps[threadIdx.x];
  const int32_t n_entries = *count;
  const int TH = TILE + 2 * R, NT = 2 * R + 1;
  for (int32_t e = blockIdx.x; e < n_entries; e += gridDim.x) {
    const ListedTile T = listed_tile(list[e], tiles);
    const int32_t r0 = T.r0(), c0 = T.c0();
    uint8_t *g = grids + (size_t)T.t * slot_bytes;
    __syncthreads();  // the previous entry is done with the LDS arrays
    for (int i = threadIdx.x; i < TILE * (TILE + 1); i += 256) (&sA[0][0])[i] = 0u;
    for (int i = threadIdx.x; i < SEEN_WORDS; i += 256) sSeen[i] = 0u;
    if (threadIdx.x == 0) sNH = 0;
    if (threadIdx.x < GRID_WS_MASK_WORDS) {
      sMask[threadIdx.x] = 0u;
      if (masks) masks[(size_t)e * GRID_WS_MASK_WORDS + threadIdx.x] = 0u;  // (an entry without hits writes nothing)
    }
    if (threadIdx.x < 2 * (TILE / 4)) (&sBal[0][0])[threadIdx.x] = 0ull;
    __syncthreads();
    // ---- phase 1: the hits of the tile's neighbourhood (TH x TH cells from (r0 - R, c0 - R)) -> list of (row, column)
    // packed into 16 bits (TH <= 96): every point of the target scan whose cell falls inside, each cell once (sSeen)
    {
      // (a target whose id is out of range has no tiles on the list: the occupancy kernel reported it)
      int32_t beg, end;
      target_points(offsets, n_scans, target_ids[t0 + T.t], t0 + T.t, nullptr, false, &beg, &end);
      // (the neighbourhood in metres, a cell wider on every side: nineteen points in twenty lie outside it and are
      //  dropped by four single-precision compares instead of two double-precision quotients; the exact test follows)
      const float resf = (float)res;
      const float x_lo = (float)(c0 - R - S / 2 - 1) * resf, x_hi = (float)(c0 + TILE + R - S / 2 + 1) * resf;
      const float y_lo = (float)(r0 - R - S / 2 - 1) * resf, y_hi = (float)(r0 + TILE + R - S / 2 + 1) * resf;
      for (int32_t p = beg + threadIdx.x; p < end; p += 256) {
        int32_t c, r;
        const float2 q = xy[p];
        if (!(q.x >= x_lo && q.x < x_hi && q.y >= y_lo && q.y < y_hi)) continue;
        if (!hit_cell(q, S, res, inv_res, &c, &r)) continue;
        const int32_t rr = r - (r0 - R), cc = c - (c0 - R);
        if (rr < 0 || rr >= TH || cc < 0 || cc >= TH) continue;
        const uint32_t idx = (uint32_t)(rr * TH + cc), bit = 1u << (idx & 31u);
        if (!(atomicOr(&sSeen[idx >> 5], bit) & bit)) sHits[atomicAdd(&sNH, 1)] = (uint16_t)((rr << 8) | cc);
      }
    }
    __syncthreads();
    const int32_t nh = sNH;
    if (nh == 0) continue;
    // ---- phase 2: the tile's own hits into the slot's hit raster, what the exact-score pass reads (64 rows x 64 bits = two
    // dwords per row; pre-zeroed, a tile owns its dwords: tiles start at multiples of 64 cells and the raster's border is 32)
    if (threadIdx.x < 2 * TILE) {
      const int r = threadIdx.x >> 1, h = threadIdx.x & 1;
      if (r0 + r < S && c0 + 32 * h < S) {
        const uint32_t b0 = (uint32_t)((R + r) * TH + R + 32 * h);  // the row's first bit of this half in sSeen
        const uint32_t w0 = sSeen[b0 >> 5], w1 = sSeen[(b0 >> 5) + 1], sh = b0 & 31u;
        const uint32_t bits = sh ? (w0 >> sh) | (w1 << (32u - sh)) : w0;
        if (bits)
          *reinterpret_cast<uint32_t *>(g + hits_offset + (size_t)(r0 + r + HIT_PAD) * hits_pitch +
                                        4 * (size_t)(((c0 + HIT_PAD) >> 5) + h)) = bits;
      }
    }
    // ---- phase 3: the blur as a scatter, one work item per (hit, output row): up to 2R + 1 atomic adds
    for (int32_t wi = threadIdx.x; wi < nh * NT; wi += 256) {
      const int32_t hit = sHits[wi / NT], di = wi % NT;
      const int32_t ro = (hit >> 8) - di, cc = hit & 0xff;
      if (ro < 0 || ro >= TILE) continue;
      const uint32_t tr = (uint32_t)sTaps[di];
      for (int dj = 0; dj < NT; dj++) {
        const int32_t co = cc - dj;
        if (co >= 0 && co < TILE) atomicAdd(&sA[ro][co], tr * (uint32_t)sTaps[dj]);
      }
    }
    __syncthreads();
    // quantise; each thread produces 4 consecutive columns of one row per turn
#pragma unroll 1
    for (int turn0 = 0; turn0 < TURNS; turn0 += GROUP) {
      // Phase 4a, 16-bit cells.  The thresholds grow exponentially: a first guess from ln(a) is the answer except next to a
      // threshold, and the table settles it exactly.  The guesses of the eight cells of TWO turns first, then their table entries
      // (thr[g], thr[g + 1]), all in flight at once: two trips to the L2-resident table per thread and tile (round 4 made one per
      // turn; the cell-by-cell form before it two to four dependent ones per cell; all four turns at once need 171 registers).
      uint32_t avT[GROUP][4], gvT[GROUP][4];
      uint2 tvT[GROUP][4];
      if (CB == 2) {
#pragma unroll
        for (int u = 0; u < GROUP; u++) {
          const int i = threadIdx.x + 256 * (turn0 + u), r = i / GROUPS, c4 = (i % GROUPS) * 4;
#pragma unroll
          for (int b = 0; b < 4; b++) {
            avT[u][b] = r0 + r < S ? sA[r][c4 + b] : 0u;
            const float gf = tab.q16_a * __logf((float)(avT[u][b] ? avT[u][b] : 1u)) + tab.q16_b;
            gvT[u][b] = gf <= 0.f ? 0u : (gf >= 65534.f ? 65534u : (uint32_t)gf);
          }
        }
#pragma unroll
        for (int u = 0; u < GROUP; u++)
#pragma unroll
          for (int b = 0; b < 4; b++) {
            // (cells without a sum load nothing)
            tvT[u][b] = make_uint2(0u, 0u);
            if (avT[u][b]) tvT[u][b] = make_uint2(thr16[gvT[u][b]], thr16[gvT[u][b] + 1u]);
          }
      }
#pragma unroll
      for (int u = 0; u < GROUP; u++) {
        const int i = threadIdx.x + 256 * (turn0 + u);
        const int r = i / GROUPS, c4 = (i % GROUPS) * 4;
        if (r0 + r >= S) continue;
        uint32_t qv[4];
        uint32_t any = 0;
        if (CB == 2) {
          // Phase 4b: the guess stands unless the sum lies next to a threshold or the guess is poor
          uint32_t av[4], gv[4];  // (copies the compiler needs: without them it arranges the searches otherwise, + 172 instructions)
          uint2 tv[4];
#pragma unroll
          for (int b = 0; b < 4; b++) {
            av[b] = avT[u][b];
            gv[b] = gvT[u][b];
            tv[b] = tvT[u][b];
          }
#pragma unroll
          for (int b = 0; b < 4; b++) {
            const uint32_t a = av[b];
            uint32_t q = 0;
            if (a) {
              uint32_t gq = gv[b];
              if ((gq == 0u || tv[b].x <= a) && tv[b].y > a) {
                q = gq;
              } else {
                // a few steps either way, else the binary search
                int it = 0;
                while (gq < 65535u && it < 6 && thr16[gq + 1] <= a) {
                  gq++;
                  it++;
                }
                while (gq > 0u && it < 12 && thr16[gq] > a) {
                  gq--;
                  it++;
                }
                const bool settled = (gq == 0u || thr16[gq] <= a) && (gq == 65535u || thr16[gq + 1] > a);
                if (settled) {
                  q = gq;
                } else {
                  for (int step = 32768; step >= 1; step >>= 1) {
                    const uint32_t n = q + step;
                    if (n <= 65535 && thr16[n] <= a) q = n;
                  }
                }
              }
            }
            qv[b] = q;
            any |= q;
          }
        } else {
          // Phase 5, 8-bit cells: q = #{k in 1..levels : thr[k] <= a}; thr is non-decreasing
          for (int b = 0; b < 4; b++) {
            const uint32_t a = sA[r][c4 + b];
            uint32_t q = 0;
            if (a) {
              for (int step = 128; step >= 1; step >>= 1) {
                const uint32_t n = q + step;
                if (n <= 255 && sThr[n] <= a) q = n;
              }
            }
            qv[b] = q;
            any |= q;
          }
        }
        if (any == 0u) continue;  // the grid is pre-zeroed
        // Phase 6: stores.  The image: pad, c0, c4 are multiples of 4, a whole aligned dword / qword inside the raster
        uint8_t *dst = g + (size_t)(r0 + r + pad) * pitch + (size_t)(c0 + c4 + pad) * CB;
        if (!has_image) {  // (NHIP_GRID_NO_IMAGE: the cells live in the matcher's tiled copies only)
        } else if (c0 + c4 + 3 < S) {
          if (CB == 1) *reinterpret_cast<uint32_t *>(dst) = qv[0] | (qv[1] << 8) | (qv[2] << 16) | (qv[3] << 24);
          else *reinterpret_cast<uint2 *>(dst) = make_uint2(qv[0] | (qv[1] << 16), qv[2] | (qv[3] << 16));
        } else {
          for (int b = 0; b < 4; b++)
            if (c0 + c4 + b < S) {
              if (CB == 1) dst[b] = (uint8_t)qv[b];
              else reinterpret_cast<uint16_t *>(dst)[b] = (uint16_t)qv[b];
            }
        }
        if (masks) {
          // which of the wave's groups (four rows x 16 groups of four columns) store anything, and which store into the
          // 8-bit plane: two ballots, kept per (wave, turn) = per four rows; phase 7 reads them after the loop
          bool hi_any = false;
          for (int b = 0; b < 4; b++)
            if (c0 + c4 + b < S && (CB == 2 ? qv[b] >> 8 : qv[b])) hi_any = true;
          const unsigned long long act = __ballot(1), hib = __ballot(hi_any);  // (lanes still here: a non-zero group inside the raster)
          if ((int)(threadIdx.x & 63u) == __ffsll((long long)act) - 1) {
            sBal[0][r >> 2] = act;
            sBal[1][r >> 2] = hib;
          }
        }
        const uint32_t hr = (uint32_t)(r0 + r + pad), hc = (uint32_t)(c0 + c4 + pad);
        if (CB == 2) {  // the matcher's tiled copy of the 16-bit cells (a 4-aligned group of four lies in one tile row)
          uint8_t *td = g + hi_offset + 2 * hi_copy_bytes + t16_tiled(hr, hc, (uint32_t)t16_tpr);
          if (c0 + c4 + 3 < S) {
            *reinterpret_cast<uint2 *>(td) = make_uint2(qv[0] | (qv[1] << 16), qv[2] | (qv[3] << 16));
          } else {
            for (int b = 0; b < 4; b++)
              if (c0 + c4 + b < S) reinterpret_cast<uint16_t *>(td)[b] = (uint16_t)qv[b];
          }
        }
        {  // the matcher's 8-bit plane: the high bytes of 16-bit cells, the cells themselves of 8-bit ones (columns past
           // the raster stay zero, like the image's border)
          uint32_t h = 0u;
          for (int b = 0; b < 4; b++)
            if (c0 + c4 + b < S) h |= (CB == 2 ? qv[b] >> 8 : qv[b]) << (8 * b);
          if (h) {  // (both tiled copies: a 4-aligned group of four cells never straddles a tile of either)
            *reinterpret_cast<uint32_t *>(g + hi_offset + hi_tiled(hr, hc, 0u, (uint32_t)hi_tpr, (uint32_t)hi_copy_bytes)) = h;
            *reinterpret_cast<uint32_t *>(g + hi_offset + hi_tiled(hr, hc, 1u, (uint32_t)hi_tpr, (uint32_t)hi_copy_bytes)) = h;
          }
        }
      }
    }
    if (masks) {
      __syncthreads();
      // ---- phase 7: the entry's line masks (nhip_grid.h) from the rows' ballots (sBal[0]: groups that stored anything,
      // sBal[1]: into the 8-bit plane), one thread per line of the tile.  Line (lr, k) of the first copy covers groups 4k ..
      // 4k + 3 of its eight rows, of the copy shifted by 8 columns groups 4k - 2 .. 4k + 1, of the 16-bit copy groups 2k, 2k + 1.
      if (threadIdx.x < LINE_COUNT_ALL) {
        using L0 = Lines<LINES_HI0>; using L1 = Lines<LINES_HI1>; using L2 = Lines<LINES_T16>;
        const uint32_t line = threadIdx.x;
        uint32_t lr, word, bit;
        unsigned long long pat;  // the groups of one row; the ballot holds four rows, 16 lanes apart
        bool hi = true;
        if (line < L1::FIRST) {
          lr = line / L0::COLS;
          pat = 0xFull << (4u * (line % L0::COLS));
          word = L0::WORD0; bit = line;
        } else if (line < L2::FIRST) {
          const uint32_t b1 = line - L1::FIRST, k = b1 % L1::COLS;
          lr = b1 / L1::COLS;
          pat = k == 0u ? 0x3ull : (k == L1::COLS - 1u ? 0xC000ull : 0xFull << (4u * k - 2u));
          word = L1::WORD0 + (b1 >> 5); bit = b1 & 31u;
        } else {
          const uint32_t b2 = line - L2::FIRST;
          lr = b2 / L2::COLS;
          pat = 0x3ull << (2u * (b2 % L2::COLS));
          word = L2::WORD0 + (b2 >> 5); bit = b2 & 31u;
          hi = false;
        }
        pat |= pat << 16;
        pat |= pat << 32;
        const unsigned long long any = (sBal[hi ? 1 : 0][2u * lr] | sBal[hi ? 1 : 0][2u * lr + 1u]) & pat;
        if (any && (hi || CB == 2)) atomicOr(&sMask[word], 1u << bit);
      }
      __syncthreads();
      if (threadIdx.x < GRID_WS_MASK_WORDS) masks[(size_t)e * GRID_WS_MASK_WORDS + threadIdx.x] = sMask[threadIdx.x];
    }
  }
}

// Level 2 driven by the blur's TILE LIST (round 4): per listed tile the P4_NE x P4_NE entries it can reach (nhip_grid.h; the
// table is pre-zeroed; an entry two tiles share is written twice with the same byte).  One workgroup per list entry: the 71 x 71
// stored cells under those windows to LDS, 7-cell maxima down the columns, then along the rows.  The band kernel launches a block
// per (band, segment, target) -- 88,000 per 1000 targets, four fifths of which leave at once: 0.22 ms against 0.08 here.
template <int CB>
__global__ __launch_bounds__(256) void grid_pool4_tiles_kernel(
    const int32_t *__restrict__ count, const int32_t *__restrict__ list, int32_t tiles, uint8_t *__restrict__ grids, int32_t pad,
    int32_t rows, int32_t pitch, int64_t table_offset, int64_t slot_bytes, int32_t pool_pitch, int32_t has_image,
    int64_t hi_offset, int32_t hi_tpr, int64_t hi_copy_bytes, int32_t t16_tpr) {
  static_assert(BNB_B4 == 4, "windows of seven cells at stride four");
  // two cells per LDS word (16-bit cells as stored; 8-bit cells widened), 36 words per row of 71 (+ 1) cells
  constexpr int RW = (P4_REG + 1) / 2;
  __shared__ uint32_t sC[P4_REG][RW + 1];
  __shared__ uint32_t sV[P4_NE][RW + 1];
  const int32_t n_entries = *count, tid = threadIdx.x;
  const int32_t n4 = (rows + BNB_B4 - 1) / BNB_B4;  // pooled rows = pooled columns (square image)
  for (int32_t e = blockIdx.x; e < n_entries; e += gridDim.x) {
    const ListedTile T = listed_tile(list[e], tiles);
    // stored row / column of the region's first cell (pad is a multiple of 4 and >= 16: never negative, 4-aligned)
    const int32_t r0 = T.r0() + pad - BNB_B4, c0 = T.c0() + pad - BNB_B4;
    const uint8_t *g = grids + (size_t)T.t * slot_bytes;
    uint8_t *pool = grids + (size_t)T.t * slot_bytes + table_offset;
    __syncthreads();  // the previous entry is done with the LDS arrays
    for (int32_t i = tid; i < P4_REG * RW; i += 256) {
      const int32_t rr = i / RW, w = i - rr * RW;
      const int32_t sr = r0 + rr, sc = c0 + 2 * w;  // (even: the pitch covers whole pairs of cells)
      uint32_t v = 0u;                              // (windows are clipped to the image)
      if (sr < rows && sc < rows) {
        // (two cells at an even column: one dword of the image, or -- NHIP_GRID_NO_IMAGE -- of the matcher's tiled copy of
        //  the cells, where an even pair never straddles a tile row)
        if (CB == 2) {
          v = has_image ? *reinterpret_cast<const uint32_t *>(g + (size_t)sr * pitch + 2 * sc)
                          : *reinterpret_cast<const uint32_t *>(g + hi_offset + 2 * hi_copy_bytes + t16_tiled((uint32_t)sr, (uint32_t)sc, (uint32_t)t16_tpr));
        } else {
          const uint32_t h = has_image ? *reinterpret_cast<const uint16_t *>(g + (size_t)sr * pitch + sc)
                                         : *reinterpret_cast<const uint16_t *>(g + hi_offset + hi_tiled((uint32_t)sr, (uint32_t)sc, 0u, (uint32_t)hi_tpr, (uint32_t)hi_copy_bytes));
          v = (h & 0xffu) | ((h & 0xff00u) << 8);
        }
      }
      sC[rr][w] = v;
    }
    __syncthreads();
    for (int32_t i = tid; i < P4_NE * RW; i += 256) {
      const int32_t pi = i / RW, w = i - pi * RW;
      uint32_t m = 0u;
#pragma unroll
      for (int k = 0; k < 2 * BNB_B4 - 1; k++) m = pk_max_u16(m, sC[BNB_B4 * pi + k][w]);
      sV[pi][w] = m;
    }
    __syncthreads();
    for (int32_t i = tid; i < P4_NE * P4_NE; i += 256) {
      const int32_t a = i / P4_NE, b = i - a * P4_NE;
      // cells 4b .. 4b + 6: words 2b, 2b + 1, 2b + 2 whole and the low half of word 2b + 3
      const uint32_t m3 = pk_max_u16(pk_max_u16(sV[a][2 * b], sV[a][2 * b + 1]), sV[a][2 * b + 2]);
      uint32_t m = max(m3 & 0xffffu, m3 >> 16);
      m = max(m, sV[a][2 * b + 3] & 0xffffu);
      const int32_t pi = r0 / BNB_B4 + a, pj = c0 / BNB_B4 + b;  // (= p4_first(T.r0(), pad) + a: r0 is 4-aligned)
      if (m == 0u || pi >= n4 || pj >= n4) continue;
      const uint8_t v = (uint8_t)(CB == 1 ? m : (m + 256u) / 257u);
      // pairs: (i, 2j) = P4[i][j], (i, 2j + 1) = P4[i + 1][j]
      pool[(size_t)pi * pool_pitch + 2 * pj] = v;
      if (pi > 0) pool[(size_t)(pi - 1) * pool_pitch + 2 * pj + 1] = v;
    }
  }
}
}  // namespace
void launch_list_and_blur(const GridPass &P, const GridKernelTables &tab, const uint32_t *thr16) {
  const GridGeom &G = P.G;
  hipLaunchKernelGGL(grid_occupancy_list_kernel, dim3(P.n), dim3(256), 0, P.s, P.xy, P.offsets, P.target_ids, P.t0, P.occ, G, P.count,
                     P.list, P.n_scans, P.status);
  hipLaunchKernelGGL(NHIP_BY_CELL_BYTES(grid_blur_kernel, G.cb), dim3(P.blocks), dim3(256), 0, P.s, P.xy, P.offsets, P.target_ids, P.t0,
                     P.count, P.list, G.tiles, P.g, G.S, G.pad, G.pitch, G.slot_bytes, G.R, G.res, G.inv_res, tab, thr16, G.tiled.offset,
                     G.tiled.hi_tpr, G.tiled.copy_bytes, G.tiled.t16_tpr, P.n_scans, G.hits_offset, G.hits_pitch, G.has_image, P.masks);
}

void launch_pool4_tiles(const GridPass &P) {
  const GridGeom &G = P.G;
  hipLaunchKernelGGL(NHIP_BY_CELL_BYTES(grid_pool4_tiles_kernel, G.cb), dim3(P.blocks), dim3(256), 0, P.s, P.count, P.list, G.tiles, P.g,
                     G.pad, G.rows, G.pitch, G.pool4_offset, G.slot_bytes, G.pool4_pitch, G.has_image, G.tiled.offset, G.tiled.hi_tpr,
                     G.tiled.copy_bytes, G.tiled.t16_tpr);
}
}  // namespace nhip
