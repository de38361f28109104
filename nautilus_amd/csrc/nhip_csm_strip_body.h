// nhip_csm_strip_body.h -- the body of the strip kernels (nhip_csm_strip.h), INCLUDED INSIDE csm_correlate_kernel<VOLUME,
// DENSE> and csm_correlate16_kernel<VOLUME, DENSE>, after `using C = <the cell policy>;` and the kernel's static LDS
// array `C::Word s_tile[C::TILE_ROWS * LP_W]`; the kernel's parameter block is P.
// (As text and not as a function: called as a __forceinline__ function template the same statements compile to other
//  code -- the 8-bit score-volume kernels to 128 VGPRs and 28-32 bytes of scratch where they have 127 and none;
//  docs/history.md, appendix G.)
  using G = Strip<C>;
  constexpr int WG_WAVES = C::WG_WAVES, TILE_ROWS = C::TILE_ROWS, FILL_INFLIGHT = C::FILL_INFLIGHT;
  constexpr int LP = G::LP, COL_SPAN = G::COL_SPAN, ROW_CH = G::ROW_CH, FILL_ROWS = G::FILL_ROWS, STEP_ROWS = G::STEP_ROWS;

  // ---- block -> (pair, rotation, plane block); everything of a pair shares an XCD
  const int32_t npb = P.npbx * P.npby;
  const int32_t per_pair = P.n_theta * npb;
  int32_t pair, w;
  if (VOLUME) {
    pair = 0;
    w = blockIdx.x;
  } else {
    const uint32_t bid = blockIdx.x;
    const uint32_t xcd = bid & 7u, j = bid >> 3;
    pair = (int32_t)((j / per_pair) * 8u + xcd);
    w = (int32_t)(j % per_pair);
    if (pair >= P.n_pairs) return;
  }
  const int32_t k = w / npb;
  const int32_t pb = w % npb;
  const int32_t ox = (pb % P.npbx) * PB_NX, oy = (pb / P.npbx) * G::PB_NY;
  const int32_t nyb = min(P.ny - oy, G::PB_NY);  // plane rows of this block
  const int32_t row_span = TILE_ROWS - nyb;      // max (prow - tile_row0) of a covered point

  int32_t src = VOLUME ? P.single_src : P.pair_src[pair];
  int32_t slot = VOLUME ? P.single_slot : P.pair_slot[pair];
  // (ids from device memory: a pair whose scan or slot lies outside the caller's counts scores nothing and is reported)
  const bool ids_ok = VOLUME || pair_ids_ok(P.ids, src, slot, pair, threadIdx.x == 0 && w == 0);
  if (!ids_ok) src = slot = 0;
  const int32_t beg = ids_ok ? P.offsets[src] : 0, n_pts = ids_ok ? P.offsets[src + 1] - beg : 0;
  const uint8_t *grid = P.grids + (size_t)slot * P.slot_bytes;
  const uint8_t *skip_map = grid + P.grid_bytes;
  const int32_t mpitch = skip_pitch(P.pitch);
  // search centre in cells; a centre the stored border cannot cover scores nothing
  int32_t cx = VOLUME ? P.single_ox : (P.pair_origin ? P.pair_origin[2 * pair] : 0);
  int32_t cy = VOLUME ? P.single_oy : (P.pair_origin ? P.pair_origin[2 * pair + 1] : 0);
  const bool centre_ok = (abs(cx) + P.hx <= P.max_shift) && (abs(cy) + P.hy <= P.max_shift);

  float cf, sf;
  compose_rotation(P.rot0_cs, P.delta_cs, pair, k, cf, sf);

  // lane = 3 * (plane row) + segment; lane 63 idles
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lane_c = lane < 63 ? lane : 62;
  const int dy = wave * WAVE_ROWS + lane_c / SEGS, seg = lane_c % SEGS;
  const bool lane_live = lane < 63;
  const bool has_right = lane_live && seg < SEGS - 1;  // lane + 1 holds the next 28 cells of the same row
  // lanes past the plane block's rows re-read row 0 (their sums are never used)
  const int dyc = (dy < nyb) ? dy : 0;
  const uint32_t lane_off = (uint32_t)(dyc * LP + seg * SEG_COLS * C::CB);
  const auto tile = C::tile_base(s_tile);

  uint32_t acc[SEG_COLS];
#pragma unroll
  for (int i = 0; i < SEG_COLS; i++) acc[i] = 0;
  C::Acc A;
  C::clear(A);

  // current tile: stored-grid rows [t_row0, t_row0 + TILE_ROWS), byte columns [t_col0, t_col0 + LP)
  int32_t t_row0 = 0, t_col0 = 0;
  bool have_tile = false;

  // lane-chunks of 64 points.  Accumulators that unpack (C::UNPACKS) have a register set per alignment class, so what must
  // not overflow is the number of points ADDED PER CLASS since the last unpack (skipped points do not count): a chunk is
  // started only while no class has more than FLUSH_START_MAX, and an unconditional unpack follows every such run of
  // chunks.  The others take one chunk per pass of the outer loop and finish once, at the end.
  int32_t c64 = 0;
  while (c64 < n_pts && centre_ok) {
    int32_t added0 = 0, added1 = 0, added2 = 0, added3 = 0;  // per alignment class
    const int32_t c0 = c64;
    for (; C::UNPACKS ? c64 < n_pts && max(max(added0, added1), max(added2, added3)) <= C::FLUSH_START_MAX : c64 == c0; c64 += 64) {
      const int32_t n = min(n_pts - c64, 64);
      // one point per lane: rotated window cell, and whether this block's strip of its window
      // holds anything but zeros (skip map, nhip_grid_tables.hip)
      uint32_t vcell = 0u, vwork = 0u;  // vwork bit u: strip u of this plane block has work for the point
      if (lane < n) {
        vcell = window_cell(P.xy[beg + c64 + lane], cf, sf, P, ox, oy, cx, cy);
        // (the skip map has one bit per stored row and aligned dword: the dword the window's first aligned word starts at)
        const uint32_t sdw = ((vcell & 0xffffu) >> 2) * C::CB;
#pragma unroll
        for (int u = 0; u < WG_WAVES; u++) {
          if (u * WAVE_ROWS >= nyb) break;
          const uint32_t bit = DENSE ? 1u : (((uint32_t)skip_map[(size_t)((vcell >> 16) + u * WAVE_ROWS) * mpitch + (sdw >> 3)] >> (sdw & 7u)) & 1u);
          vwork |= bit << u;
        }
      }
      const int32_t vcol = (int32_t)(C::CB * (vcell & 0xffffu)), vrow = (int32_t)(vcell >> 16);  // (column in bytes)
      unsigned long long todo = __ballot(vwork != 0u);                 // points some wave of the workgroup needs
      const unsigned long long mine = __ballot((vwork >> wave) & 1u);  // points this wave adds
      if constexpr (C::UNPACKS) {
        // class of a point = (window start column) & 3: tile origins are multiples of 16, so it does
        // not depend on the tile the point will be read from
        const uint32_t vc = vcell & 3u;
        const unsigned long long k0 = __ballot(vc == 0u) & mine, k1 = __ballot(vc == 1u) & mine;
        const unsigned long long k2 = __ballot(vc == 2u) & mine;
        added0 += __builtin_popcountll(k0);
        added1 += __builtin_popcountll(k1);
        added2 += __builtin_popcountll(k2);
        added3 += __builtin_popcountll(mine) - __builtin_popcountll(k0 | k1 | k2);
      }
      while (todo) {
        const int32_t j = (int32_t)__builtin_ctzll(todo);
        // remaining points inside the staged tile; e = first remaining point that is not
        bool cov = have_tile && (uint32_t)(vcol - t_col0) <= (uint32_t)COL_SPAN &&
                   (uint32_t)(vrow - t_row0) <= (uint32_t)row_span;
        unsigned long long miss = ~__ballot(cov) & todo;
        int32_t e = miss ? (int32_t)__builtin_ctzll(miss) : 64;
        if (e == j) {
          // point j is outside: stage a new tile around it, biased along the sweep direction.
          // (This branch never touches the accumulators.)
          const int32_t ja = min(j + 16, n - 1);
          const int32_t cj = __builtin_amdgcn_readlane(vcol, j), rj = __builtin_amdgcn_readlane(vrow, j);
          const int32_t ca = __builtin_amdgcn_readlane(vcol, ja), ra = __builtin_amdgcn_readlane(vrow, ja);
          t_col0 = place(cj, ca, COL_SPAN - 15) & ~15;
          t_row0 = place(rj, ra, row_span);
          have_tile = true;
          const uint8_t *gsrc = grid + (size_t)t_row0 * P.pitch + t_col0;
          __syncthreads();  // orders the LDS reads of the old tile before the stores
          // Fill: the first FILL_ROWS * ROW_CH lanes of a wave move FILL_ROWS tile rows per step -- one 16-byte global load
          // per lane (t_col0 and the pitch are multiples of 16), FILL_INFLIGHT steps at a time -- then word-sized LDS stores
          // (the LDS pitch that makes the reads conflict-free is no multiple of 16: rows start on word boundaries).  Tile
          // rows past the stored grid re-read its last row; no covered window reaches them.
          if (lane < FILL_ROWS * ROW_CH) {
            // (recomputed here: staging is rare, VGPRs are not); wave w takes steps w, w + WG_WAVES, ...
            const int fr = lane / ROW_CH + FILL_ROWS * wave, fk = lane % ROW_CH;
            const int fill_w = fr * LP_W + G::CHUNK_W * fk;
            const uint8_t *lsrc = gsrc + 16 * fk;
            const int32_t last_row = P.rows - 1 - t_row0;
#pragma unroll
            for (int b = 0; b < TILE_ROWS / STEP_ROWS; b += FILL_INFLIGHT) {
              uint4 v[FILL_INFLIGHT];
#pragma unroll
              for (int u = 0; u < FILL_INFLIGHT; u++) {
                if (STEP_ROWS * (b + u) >= TILE_ROWS) continue;  // (compile time: the last batch may be short)
                const int32_t r = min(STEP_ROWS * (b + u) + fr, last_row);
                v[u] = *reinterpret_cast<const uint4 *>(lsrc + (uint32_t)(r * P.pitch));
              }
#pragma unroll
              for (int u = 0; u < FILL_INFLIGHT; u++)
                if (STEP_ROWS * (b + u) < TILE_ROWS) C::store_head(s_tile + STEP_ROWS * (b + u) * LP_W + fill_w, v[u]);
              if (fk < ROW_CH - 1) {
#pragma unroll
                for (int u = 0; u < FILL_INFLIGHT; u++) {
                  if (STEP_ROWS * (b + u) >= TILE_ROWS) continue;
                  C::store_tail(s_tile + STEP_ROWS * (b + u) * LP_W + fill_w, v[u]);
                }
              }
            }
          }
          __syncthreads();
          cov = (uint32_t)(vcol - t_col0) <= (uint32_t)COL_SPAN &&
                (uint32_t)(vrow - t_row0) <= (uint32_t)row_span;
          miss = ~__ballot(cov) & todo;
          e = miss ? (int32_t)__builtin_ctzll(miss) : 64;  // > j: the new tile covers point j
        }
        // remaining points before e are covered: LDS byte offset of each lane's window start,
        // then the grouped accumulation
        const uint32_t vorg = (uint32_t)(vrow - t_row0) * LP + (uint32_t)(vcol - t_col0);
        const unsigned long long seg_mask = todo & (e == 64 ? ~0ull : ((1ull << e) - 1ull));
        C::segment(A, tile, lane_off, vorg, seg_mask & mine);
        todo &= ~seg_mask;
      }
    }
    if constexpr (C::UNPACKS) C::finish(A, acc, has_right);
  }
  if constexpr (!C::UNPACKS) C::finish(A, acc, has_right);

  const int32_t iy = oy + dy;
  const bool row_ok = lane_live && dy < nyb;
  if (VOLUME) {
    if (row_ok) {
#pragma unroll
      for (int i = 0; i < SEG_COLS; i++) {
        const int32_t ix = ox + seg * SEG_COLS + i;
        if (seg * SEG_COLS + i < PB_NX && ix < P.nx)
          P.volume[((size_t)k * P.nx + ix) * P.ny + iy] = (int32_t)acc[i];
      }
    }
    return;
  }

  // ---- K3: the strip's best key
  unsigned long long best = 0ull;
  if (row_ok) {
#pragma unroll
    for (int i = 0; i < SEG_COLS; i++) {
      const int32_t ix = ox + seg * SEG_COLS + i;
      if (seg * SEG_COLS + i < PB_NX && ix < P.nx) {
        const unsigned long long key = pose_key(acc[i], (uint32_t)((k * P.nx + ix) * P.ny + iy));
        best = key > best ? key : best;
      }
    }
  }
  wave_max_to_key(best, lane, &P.keys[pair]);
