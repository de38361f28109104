// nhip_mapwin.hip -- K20: map windows.  A scan is localised in a finished occupancy grid by matching it against a table built
// from the grid's occupied cells around its prior pose; this unit makes those target clouds on the device: first the occupied
// cells of the map as a row-compressed list, then for every query the exact crop of that list around the world cell of its
// prior, as points of the layout every other entry point takes.  The spec is DESIGN.md section 3, "Map windows";
// tests/localize_reference.py restates it cell by cell, hostside.map_cells / map_windows in numpy.  Everything is integer up
// to the one double multiply and the one rounding to float that make a point, no output is written with an atomic, and every
// compaction keeps its order: the results are the reference's bit for bit, the same every run.
//
//   mapwin_row_count_kernel    a wave per map row: the bytes up to the first 16-byte boundary one per lane, the body as uint4
//                              loads (16 cells a lane), the tail one per lane; the popcount of the compare, reduced over the
//                              wave, goes to row_ptr[y].
//   mapwin_row_scan_kernel     one workgroup, 1024 rows per step (<= 16 steps): the exclusive scan of the counts in place,
//                              row_ptr[height] = their sum, and the capacity decision: more cells than max_cells and EVERY
//                              entry becomes 0, so that the pack stores nothing and a gather sees an empty map.
//   mapwin_row_pack_kernel     a wave per map row, a lane per cell, 64 cells per step: a lane's rank is the popcount of the
//                              ballot below it, so the x order is kept; a row ends as soon as its count is packed.
//   mapwin_window_count_kernel a workgroup per query, a lane per window row: the map row under it, the x range the window
//                              takes of it, two bisections of the row's cols; the sum goes to counts[q] (the workspace).
//   mapwin_window_scan_kernel  one workgroup, 1024 queries per step, any number of steps: int64 totals, the capacity decision
//                              (more points than out_capacity or than 2^31 - 1: every offset 0), int32 offsets, the stats.
//   mapwin_window_pack_kernel  a workgroup per query, MW_T window rows at a time: the rows' ranges once more, their scan into
//                              LDS, and every lane finds the row of each of its points by bisection of that table; the
//                              stores are float2 and contiguous across the whole window.
//
// No kernel reads the map per query: a window costs `side` row lookups and its own output.  Every entry of row_ptr is checked
// before it becomes an address (window_row); entries of cols and the origins are only compared and converted, in int64.
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int MW_T = 256;
constexpr int MW_WAVES = MW_T / 64;
constexpr int MW_SCAN_T = 1024;
constexpr int MW_MAX_QUERY_BLOCKS = 16384;  // workgroups along the queries; more queries than that: grid-stride

__device__ __forceinline__ int32_t occupied4(uint32_t v, int32_t occ_min) {  // of the four int8 cells of a dword
  int32_t n = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) n += (int32_t)(int8_t)(v >> (8 * k)) >= occ_min;
  return n;
}

__global__ __launch_bounds__(MW_T) void mapwin_row_count_kernel(MapwinParams P, const int8_t *__restrict__ grid,
                                                                int32_t *__restrict__ row_ptr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t y = (int32_t)blockIdx.x * MW_WAVES + wv;
  if (y >= P.height) return;  // (the whole wave)
  const int32_t w = P.width;
  const int8_t *row = grid + (size_t)y * (size_t)w;
  int32_t head = (int32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u);
  if (head > w) head = w;
  int32_t n = 0;
  if (lane < head) n += (int32_t)row[lane] >= P.occ_min;
  const int32_t chunks = (w - head) / 16;
  const uint4 *body = reinterpret_cast<const uint4 *>(row + head);  // (16-byte aligned; chunk c ends at head + 16 c + 16 <= w)
  for (int32_t c = lane; c < chunks; c += 64) {
    const uint4 v = body[c];
    n += occupied4(v.x, P.occ_min) + occupied4(v.y, P.occ_min) + occupied4(v.z, P.occ_min) + occupied4(v.w, P.occ_min);
  }
  const int32_t tail = head + 16 * chunks + lane;  // (fewer than 16 cells are left)
  if (tail < w) n += (int32_t)row[tail] >= P.occ_min;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
  if (lane == 0) row_ptr[y] = n;
}

// the inclusive scan of v over the MW_SCAN_T threads of the workgroup; *all: the sum.  Ends with a barrier: wave_sum is free again
__device__ __forceinline__ long long scan_1024(long long v, long long *wave_sum, long long *all) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  if (lane == 63) wave_sum[wv] = inc;
  __syncthreads();
  long long before = 0, sum = 0;
#pragma unroll
  for (int q = 0; q < MW_SCAN_T / 64; q++) {
    const long long s = wave_sum[q];
    if (q < wv) before += s;
    sum += s;
  }
  __syncthreads();
  *all = sum;
  return before + inc;
}

// One workgroup.  In: row_ptr[y] = the occupied cells of row y.  Out: row_ptr[y] = the index of its first, row_ptr[height] =
// their number -- or zeros throughout; stats[0], stats[5], the other words cleared.
__global__ __launch_bounds__(MW_SCAN_T) void mapwin_row_scan_kernel(MapwinParams P, int32_t max_cells, int32_t *__restrict__ row_ptr) {
  __shared__ long long wave_sum[MW_SCAN_T / 64];
  const int t = threadIdx.x;
  long long carry = 0;  // (uniform; <= 16384^2)
  for (int32_t base = 0; base < P.height; base += MW_SCAN_T) {
    const int32_t y = base + t;
    const long long v = y < P.height ? (long long)row_ptr[y] : 0;
    long long all;
    const long long inc = scan_1024(v, wave_sum, &all);
    if (y < P.height) row_ptr[y] = (int32_t)(carry + inc - v);
    carry += all;
  }
  const bool fits = carry <= (long long)max_cells;
  if (!fits)
    for (int32_t y = t; y < P.height; y += MW_SCAN_T) row_ptr[y] = 0;  // (row y was written by this thread)
  if (t == 0) {
    row_ptr[P.height] = fits ? (int32_t)carry : 0;
    for (int k = 0; k < 8; k++) P.stats[k] = 0;
    P.stats[0] = carry;
    P.stats[5] = fits ? 0 : 1;
    if (!fits) flag_bad_id(P.status, BAD_MAPWIN_CELLS, (int32_t)carry, P.height);
  }
}

__global__ __launch_bounds__(MW_T) void mapwin_row_pack_kernel(MapwinParams P, const int8_t *__restrict__ grid, int32_t max_cells,
                                                               const int32_t *__restrict__ row_ptr, int32_t *__restrict__ cols) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t y = (int32_t)blockIdx.x * MW_WAVES + wv;
  if (y >= P.height) return;  // (the whole wave)
  const int32_t b = row_ptr[y], e = row_ptr[y + 1];
  if (b < 0 || e <= b || e > max_cells) return;  // (an empty row; or the scan refused the map: every entry is 0)
  const int8_t *row = grid + (size_t)y * (size_t)P.width;
  int32_t at = b;  // where the step's first occupied cell goes (uniform)
  for (int32_t x0 = 0; x0 < P.width && at < e; x0 += 64) {
    const int32_t x = x0 + lane;
    const bool occ = x < P.width && (int32_t)row[x] >= P.occ_min;
    const unsigned long long m = __ballot(occ);
    const int32_t mine = at + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (occ && mine < e) cols[mine] = x;  // (mine < e <= max_cells)
    at += __builtin_popcountll(m);
  }
}

// The entries of cols that window row r of the query at origin (ox, oy) takes: *src is the index of the first, the return value
// their number.  A window row outside the map, or beside it, takes none.  row_ptr's two entries become addresses only if they
// are a range inside [0, n_cells].
__device__ __forceinline__ int32_t window_row(const MapwinParams &P, const int32_t *__restrict__ row_ptr,
                                              const int32_t *__restrict__ cols, int32_t n_cells, int32_t ox, int32_t oy, int32_t r,
                                              int32_t *src) {
  *src = 0;
  const long long half = (long long)(P.side / 2);
  const long long my = (long long)oy + ((long long)r - half) - (long long)P.cell_y0;  // the map row (|.| < 2^33)
  if (my < 0 || my >= (long long)P.height) return 0;
  long long lo = (long long)ox - half - (long long)P.cell_x0, hi = lo + (long long)P.side - 1;  // local x of the window's ends
  if (lo < 0) lo = 0;
  if (hi > (long long)P.width - 1) hi = (long long)P.width - 1;
  if (lo > hi) return 0;
  const int32_t b = row_ptr[my], e = row_ptr[my + 1];
  if (b < 0 || e < b || e > n_cells) {
    flag_bad_id(P.status, BAD_MAPWIN_CELLS, (b < 0 || b > n_cells) ? b : e, (int32_t)my);  // (the entry at fault)
    return 0;
  }
  int32_t a0 = b, a1 = e;  // the first entry >= lo
  while (a0 < a1) {
    const int32_t mid = a0 + (a1 - a0) / 2;
    if ((long long)cols[mid] < lo) a0 = mid + 1;
    else a1 = mid;
  }
  int32_t c0 = a0, c1 = e;  // the first entry > hi
  while (c0 < c1) {
    const int32_t mid = c0 + (c1 - c0) / 2;
    if ((long long)cols[mid] <= hi) c0 = mid + 1;
    else c1 = mid;
  }
  *src = a0;
  return c0 - a0;
}

__device__ __forceinline__ int32_t cells_held(const MapwinParams &P, const int32_t *__restrict__ row_ptr) {
  const int32_t n = row_ptr[P.height];
  return n > 0 ? n : 0;
}

__global__ __launch_bounds__(MW_T) void mapwin_window_count_kernel(MapwinParams P, const int32_t *__restrict__ row_ptr,
                                                                   const int32_t *__restrict__ cols,
                                                                   const int32_t *__restrict__ origins, int32_t n_queries,
                                                                   int32_t *__restrict__ counts) {
  __shared__ long long wave_n[MW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t n_cells = cells_held(P, row_ptr);
  for (long long qq = blockIdx.x; qq < n_queries; qq += gridDim.x) {
    const int32_t q = (int32_t)qq;
    const int32_t ox = origins[2 * (size_t)q], oy = origins[2 * (size_t)q + 1];
    long long n = 0;
    for (int32_t r = tid; r < P.side; r += MW_T) {
      int32_t src;
      n += window_row(P, row_ptr, cols, n_cells, ox, oy, r, &src);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if (lane == 0) wave_n[wv] = n;
    __syncthreads();
    if (tid == 0) {
      long long all = 0;
      for (int w = 0; w < MW_WAVES; w++) all += wave_n[w];
      counts[q] = (int32_t)all;  // (<= side^2 <= 2^26)
    }
    __syncthreads();  // (wave_n is rewritten by the workgroup's next query)
  }
}

// One workgroup.  out_offsets[q] = the index of window q's first point, out_offsets[n_queries] = their number -- or zeros
// throughout; stats[1..4] and stats[6].
__global__ __launch_bounds__(MW_SCAN_T) void mapwin_window_scan_kernel(MapwinParams P, const int32_t *__restrict__ counts,
                                                                       int32_t n_queries, int64_t out_capacity,
                                                                       int32_t *__restrict__ out_offsets) {
  __shared__ long long wave_sum[MW_SCAN_T / 64];
  __shared__ long long wave_empty[MW_SCAN_T / 64], wave_max[MW_SCAN_T / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  long long carry = 0;                // points of the steps before (uniform)
  long long n_empty = 0, largest = 0;  // of this thread
  for (long long base = 0; base < n_queries; base += MW_SCAN_T) {
    const long long q = base + t;
    long long v = 0;
    if (q < n_queries) {
      const int32_t c = counts[q];
      v = c > 0 ? (long long)c : 0;
      n_empty += v == 0;
      largest = v > largest ? v : largest;
    }
    long long all;
    const long long inc = scan_1024(v, wave_sum, &all);
    if (q < n_queries) out_offsets[q] = (int32_t)(carry + inc - v);  // (past the capacity: truncated here, zeroed below)
    carry += all;
  }
  const bool fits = carry <= (long long)out_capacity && carry <= 0x7fffffffll;
  if (!fits)
    for (long long q = t; q < n_queries; q += MW_SCAN_T) out_offsets[q] = 0;  // (query q was written by this thread)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_empty += __shfl_xor(n_empty, d, 64);
    const long long u = __shfl_xor(largest, d, 64);
    largest = u > largest ? u : largest;
  }
  if (lane == 0) wave_empty[wv] = n_empty, wave_max[wv] = largest;
  __syncthreads();
  if (t == 0) {
    long long e = 0, m = 0;
    for (int w = 0; w < MW_SCAN_T / 64; w++) {
      e += wave_empty[w];
      m = wave_max[w] > m ? wave_max[w] : m;
    }
    out_offsets[n_queries] = fits ? (int32_t)carry : 0;
    P.stats[1] = n_queries;
    P.stats[2] = fits ? carry : 0;
    P.stats[3] = e;
    P.stats[4] = m;
    P.stats[6] = fits ? 0 : 1;
    if (!fits) flag_bad_id(P.status, BAD_MAPWIN_POINTS, (int32_t)(carry > 0x7fffffffll ? 0x7fffffffll : carry), n_queries);
  }
}

__global__ __launch_bounds__(MW_T) void mapwin_window_pack_kernel(MapwinParams P, const int32_t *__restrict__ row_ptr,
                                                                  const int32_t *__restrict__ cols,
                                                                  const int32_t *__restrict__ origins, int32_t n_queries,
                                                                  float2 *__restrict__ out_xy, int64_t out_capacity,
                                                                  const int32_t *__restrict__ out_offsets) {
  __shared__ int32_t s_start[MW_T];  // index of the row's first point among the points of these MW_T rows
  __shared__ int32_t s_src[MW_T];    // index of its first cell in cols
  __shared__ int32_t s_wave[MW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t n_cells = cells_held(P, row_ptr);
  const long long half = (long long)(P.side / 2);
  for (long long qq = blockIdx.x; qq < n_queries; qq += gridDim.x) {
    const int32_t q = (int32_t)qq;
    const long long o = out_offsets[q], o_end = out_offsets[q + 1];
    if (o < 0 || o_end <= o || o_end > (long long)out_capacity) continue;  // (an empty window; or the scan refused: zeros.  Uniform)
    const int32_t ox = origins[2 * (size_t)q], oy = origins[2 * (size_t)q + 1];
    long long done = 0;  // points of this window stored by the rows before (uniform)
    for (int32_t r0 = 0; r0 < P.side; r0 += MW_T) {
      const int32_t r = r0 + tid;
      const int nb = P.side - r0 < MW_T ? P.side - r0 : MW_T;  // rows of this step
      int32_t len = 0, src = 0;
      if (r < P.side) len = window_row(P, row_ptr, cols, n_cells, ox, oy, r, &src);
      int32_t inc = len;  // inclusive scan over the workgroup: in the wave by shuffles, across the waves through LDS
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int32_t u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
      }
      if (lane == 63) s_wave[wv] = inc;
      __syncthreads();
      int32_t before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < MW_WAVES; w++) {
        const int32_t c = s_wave[w];
        if (w < wv) before += c;
        all += c;
      }
      s_start[tid] = before + inc - len;
      s_src[tid] = src;
      __syncthreads();
      for (int32_t i = tid; i < all; i += MW_T) {
        // the last row of the step that starts at or before point i (the first does, at 0): rows without points share their
        // start with the next one and are passed over
        int a = 0, b = nb;
        while (b - a > 1) {
          const int mid = (a + b) >> 1;
          if (s_start[mid] <= i) a = mid;
          else b = mid;
        }
        const int32_t c = cols[(size_t)s_src[a] + (size_t)(i - s_start[a])];  // (inside the row's range: window_row checked it)
        const long long kx = (long long)c + (long long)P.cell_x0 - (long long)ox, ky = (long long)(r0 + a) - half;
        const long long at = o + done + i;
        if (at < o_end)
          out_xy[at] = make_float2((float)__dmul_rn(__dadd_rn((double)kx, 0.5), P.res), (float)__dmul_rn(__dadd_rn((double)ky, 0.5), P.res));
      }
      done += all;
      __syncthreads();  // (the tables are rewritten by the next step)
    }
  }
}

}  // namespace

int launch_mapwin_cells(const MapwinParams &P, const int8_t *d_grid, int32_t max_cells, int32_t *d_row_ptr, int32_t *d_cols,
                        hipStream_t s) {
  const uint32_t blocks = (uint32_t)((P.height + MW_WAVES - 1) / MW_WAVES);
  hipLaunchKernelGGL(mapwin_row_count_kernel, dim3(blocks), dim3(MW_T), 0, s, P, d_grid, d_row_ptr);
  hipLaunchKernelGGL(mapwin_row_scan_kernel, dim3(1), dim3(MW_SCAN_T), 0, s, P, max_cells, d_row_ptr);
  if (max_cells > 0) hipLaunchKernelGGL(mapwin_row_pack_kernel, dim3(blocks), dim3(MW_T), 0, s, P, d_grid, max_cells, d_row_ptr, d_cols);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_mapwin_gather(const MapwinParams &P, const int32_t *d_row_ptr, const int32_t *d_cols, const int32_t *d_origins,
                         int32_t n_queries, float *d_out_xy, int64_t out_capacity, int32_t *d_out_offsets, int32_t *d_counts,
                         hipStream_t s) {
  const uint32_t blocks = (uint32_t)(n_queries < MW_MAX_QUERY_BLOCKS ? n_queries : MW_MAX_QUERY_BLOCKS);
  if (n_queries > 0)
    hipLaunchKernelGGL(mapwin_window_count_kernel, dim3(blocks), dim3(MW_T), 0, s, P, d_row_ptr, d_cols, d_origins, n_queries, d_counts);
  hipLaunchKernelGGL(mapwin_window_scan_kernel, dim3(1), dim3(MW_SCAN_T), 0, s, P, d_counts, n_queries, out_capacity, d_out_offsets);
  if (n_queries > 0 && out_capacity > 0)
    hipLaunchKernelGGL(mapwin_window_pack_kernel, dim3(blocks), dim3(MW_T), 0, s, P, d_row_ptr, d_cols, d_origins, n_queries,
                       reinterpret_cast<float2 *>(d_out_xy), out_capacity, d_out_offsets);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
