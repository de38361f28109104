// nhip_rangesig.hip -- K21: range signatures.  Global localisation in a finished occupancy grid: every free lattice cell of the
// map (an anchor) as 64 bytes, the quantised distance to the nearest wall in each of 64 sectors, ray-cast in the grid; every
// scan as the same 64 bytes from its returns; and the match of the two under the best of the 64 rotations by the sum of
// absolute differences of the bytes, the K best anchors per query with their neighbours suppressed.  The spec is DESIGN.md
// section 3, "Range signatures"; tests/rangesig_reference.py restates it ray by ray and step by step, hostside.range_signatures
// / scan_signatures / signature_candidates in numpy.  Integer after the float comparisons of a scan's points; minima and sums
// of integers know no order, and every compaction keeps its own: the results are the reference's bit for bit.
//
//   rs_fill_kernel        the anchor list set to -1 throughout (an entry behind the anchors found is no anchor).
//   rs_row_count_kernel   a wave per lattice row, a lane per node, 64 nodes a step: the free nodes of the row, reduced over the
//                         wave, go to row_counts[j] (the workspace).
//   rs_row_scan_kernel    one workgroup, 1024 rows per step (<= 16 steps): the exclusive scan in place, the stats, and the
//                         report when the anchors do not fit.
//   rs_row_pack_kernel    a wave per lattice row: a lane's rank is the popcount of the ballot below it, so the order of i is
//                         kept; a store is guarded by max_anchors.
//   rs_map_kernel         a lane per ray, the m rays of a sector in adjacent lanes, the 64 m rays of an anchor in adjacent
//                         lanes and waves: the walk of the occupancy grid's ray (nhip_ray.h, rdiv unchanged) to the first cell
//                         that is outside, unknown or a wall (under NHIP_RANGESIG_UNKNOWN_STOPS an unknown cell gives its range as
//                         a wall does); the sector's minimum by m - 1 shuffles, four sectors' bytes
//                         gathered into a dword by three more, one dword store per four sectors.  The ray table's entry and the
//                         anchor come from device memory: both are checked, and every cell index is tested against the window
//                         before it becomes an address.
//   rs_scan_kernel        a workgroup per scan (grid-stride), a lane per point: the byte by bisection of the edge table, the
//                         sector by the place descriptor's counts (the same single-rounded operations), the sector's minimum by
//                         LDS atomicMin; 16 dword stores per scan.
//   rs_cost_kernel        THE HOT PATH.  A lane is an anchor holding its 16 dwords for RANGESIG_QT queries in turn.  The query's
//                         bytes and its mask (0xff where the scan has a return) are wave-uniform; a rotation by s = 4 d + b
//                         sectors is a byte rotation by b of the query (four per query, on the scalar unit: what v_alignbyte_b32
//                         computes, kept in SGPRs) and a dword rotation by d, which is register renaming in the fully unrolled
//                         loop over d.  Per shift and
//                         dword: v_and_b32 of the anchor's dword with the rotated mask, v_sad_u8 against the rotated query
//                         (whose masked bytes are 0), accumulating.  The best key cost * 64 + shift by an unsigned minimum: the
//                         smallest shift wins a tie.  One uint32 key per (query, anchor) into the workspace.
//   rs_topk_kernel        a wave per query, as place_topk_kernel: K rounds of a wave-wide minimum over (key, anchor index)
//                         among the anchors that no accepted one suppresses (Chebyshev distance on the lattice indices, the
//                         accepted ones in registers) -- the greedy walk's result.
#include "nhip_common.h"
#include "nhip_ray.h"  // (rdiv: the ray's step, shared with K14 and K15)

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int RS_T = 256;
constexpr int RS_WAVES = RS_T / 64;
constexpr int RS_SCAN_T = 1024;
constexpr int RS_MAX_SCAN_BLOCKS = 4096;
constexpr int RS_MAX_K = 16;
constexpr uint32_t RS_KEY_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ int32_t nodes_along(int32_t cells, int32_t stride) {
  const int32_t h = stride / 2;
  return cells > h ? (cells - h - 1) / stride + 1 : 0;
}

__device__ __forceinline__ bool cell_in(const RangesigParams &P, int32_t x, int32_t y) {
  return (uint32_t)x < (uint32_t)P.width && (uint32_t)y < (uint32_t)P.height;
}

__global__ __launch_bounds__(RS_T) void rs_fill_kernel(int4 *__restrict__ anchors, int32_t max_anchors) {
  const long long i = (long long)blockIdx.x * RS_T + threadIdx.x;
  if (i < max_anchors) anchors[i] = make_int4(-1, -1, -1, -1);
}

__global__ __launch_bounds__(RS_T) void rs_row_count_kernel(RangesigParams P, const int8_t *__restrict__ grid,
                                                            int32_t *__restrict__ row_counts) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t ni = nodes_along(P.width, P.stride), nj = nodes_along(P.height, P.stride);
  const int32_t j = (int32_t)blockIdx.x * RS_WAVES + wv;
  if (j >= nj) return;  // (the whole wave)
  const int32_t h = P.stride / 2;
  const int8_t *row = grid + (size_t)(j * P.stride + h) * (size_t)P.width;  // (j stride + h < height: j < nj)
  int32_t n = 0;
  for (int32_t i = lane; i < ni; i += 64) {
    const int32_t v = (int32_t)row[i * P.stride + h];  // (i stride + h < width: i < ni)
    n += v >= 0 && v <= P.free_max;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
  if (lane == 0) row_counts[j] = n;
}

// One workgroup.  In: row_counts[j] = the anchors of lattice row j.  Out: row_counts[j] = the index of its first,
// row_counts[nj] = their number; stats[0..2], the other words cleared.
__global__ __launch_bounds__(RS_SCAN_T) void rs_row_scan_kernel(RangesigParams P, int32_t max_anchors, int32_t *__restrict__ row_counts) {
  __shared__ long long wave_sum[RS_SCAN_T / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int32_t ni = nodes_along(P.width, P.stride), nj = nodes_along(P.height, P.stride);
  long long carry = 0;  // (uniform; <= 16384^2)
  for (int32_t base = 0; base < nj; base += RS_SCAN_T) {
    const int32_t j = base + t;
    const long long v = j < nj ? (long long)row_counts[j] : 0;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long u = __shfl_up(inc, d, 64);
      if (lane >= d) inc += u;
    }
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < RS_SCAN_T / 64; q++) {
      const long long s = wave_sum[q];
      if (q < wv) before += s;
      all += s;
    }
    __syncthreads();  // (wave_sum is rewritten by the next step)
    const long long first = carry + before + inc - v;
    if (j < nj) row_counts[j] = (int32_t)(first < 0x7fffffffll ? first : 0x7fffffffll);
    carry += all;
  }
  if (t == 0) {
    row_counts[nj] = (int32_t)(carry < 0x7fffffffll ? carry : 0x7fffffffll);
    const long long left_out = carry > (long long)max_anchors ? carry - (long long)max_anchors : 0;
    for (int k = 0; k < 8; k++) P.stats[k] = 0;
    P.stats[0] = (long long)ni * (long long)nj;
    P.stats[1] = carry;
    P.stats[2] = left_out;
    if (left_out) flag_bad_id(P.status, BAD_RANGESIG, (int32_t)(carry < 0x7fffffffll ? carry : 0x7fffffffll), max_anchors);
  }
}

__global__ __launch_bounds__(RS_T) void rs_row_pack_kernel(RangesigParams P, const int8_t *__restrict__ grid, int32_t max_anchors,
                                                           const int32_t *__restrict__ row_counts, int4 *__restrict__ anchors) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t ni = nodes_along(P.width, P.stride), nj = nodes_along(P.height, P.stride);
  const int32_t j = (int32_t)blockIdx.x * RS_WAVES + wv;
  if (j >= nj) return;  // (the whole wave)
  const int32_t b = row_counts[j], e = row_counts[j + 1];
  if (b < 0 || e <= b || b >= max_anchors) return;  // (an empty row; or one wholly behind the capacity)
  const int32_t h = P.stride / 2, cy = j * P.stride + h;
  const int8_t *row = grid + (size_t)cy * (size_t)P.width;
  int32_t at = b;  // where the step's first anchor goes (uniform)
  for (int32_t i0 = 0; i0 < ni && at < e && at < max_anchors; i0 += 64) {
    const int32_t i = i0 + lane;
    bool is_free = false;
    if (i < ni) {
      const int32_t v = (int32_t)row[i * P.stride + h];
      is_free = v >= 0 && v <= P.free_max;
    }
    const unsigned long long m = __ballot(is_free);
    const int32_t mine = at + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (is_free && mine < max_anchors) anchors[mine] = make_int4(i * P.stride + h, cy, i, j);
    at += __builtin_popcountll(m);
  }
}

// a ray-table entry {dx, dy, n, scale} that the walk can take: n steps, no step beyond n cells, k scale below 2^31
__device__ __forceinline__ bool ray_ok(const int4 &r) {
  const int32_t ax = r.x < 0 ? -r.x : r.x, ay = r.y < 0 ? -r.y : r.y;
  return r.z >= 1 && r.z <= RAY_MAX_CELLS && r.x >= -RAY_MAX_CELLS && r.y >= -RAY_MAX_CELLS && ax <= r.z && ay <= r.z && r.w >= 0 &&
         (long long)r.z * (long long)r.w < 0x80000000ll;
}

__global__ __launch_bounds__(RS_T) void rs_map_kernel(RangesigParams P, const int8_t *__restrict__ grid, const int4 *__restrict__ rays,
                                                      const int4 *__restrict__ anchors, int32_t n_anchors, uint32_t *__restrict__ sig) {
  const int lane = threadIdx.x & 63;
  const int32_t m = P.rays_per_sector, per_anchor = 64 * m;  // (a power of two: 64 .. 512)
  const long long g = (long long)blockIdx.x * RS_T + threadIdx.x;
  const bool have = g < (long long)n_anchors * per_anchor;
  const int32_t a = have ? (int32_t)(g / per_anchor) : 0, t = (int32_t)(g % per_anchor);
  const int4 an = have ? anchors[a] : make_int4(-1, -1, -1, -1);
  const int4 r = have ? rays[t] : make_int4(0, 0, 0, 0);
  const bool an_ok = have && cell_in(P, an.x, an.y), r_ok = ray_ok(r);
  if (have && !r_ok && a == 0) flag_bad_id(P.status, BAD_RANGESIG, r.z, t);  // (once per entry)
  uint32_t val = 255u;
  int end = 2;  // 0: a wall, 1: unknown, 2: outside the window, or nothing by n
  if (an_ok && r_ok) {
    const int32_t n = r.z;
    const float inv_den = 1.0f / (float)(2 * n);
    for (int32_t k = 1; k <= n; k++) {
      const int32_t x = an.x + rdiv(k * r.x, n, inv_den), y = an.y + rdiv(k * r.y, n, inv_den);
      if (!cell_in(P, x, y)) break;
      const int32_t v = (int32_t)grid[(size_t)y * (size_t)P.width + (size_t)x];
      if (v < 0 || v >= P.occ_min) {
        end = v < 0 ? 1 : 0;
        if (v >= 0 || (P.flags & NHIP_RANGESIG_UNKNOWN_STOPS)) {
          const uint32_t q = ((uint32_t)k * (uint32_t)r.w) >> 16;  // (k scale < 2^31: ray_ok)
          val = q < 254u ? q : 254u;
        }
        break;
      }
    }
  }
  // the sector's minimum over its m adjacent lanes, then four sectors' bytes into the lane of the first
  for (int d = 1; d < m; d <<= 1) {
    const uint32_t o = __shfl_xor(val, d, 64);
    val = o < val ? o : val;
  }
  const uint32_t b1 = __shfl_down(val, m, 64), b2 = __shfl_down(val, 2 * m, 64), b3 = __shfl_down(val, 3 * m, 64);
  if (have && (t & (4 * m - 1)) == 0) sig[(size_t)a * 16 + (size_t)(t / (4 * m))] = val | (b1 << 8) | (b2 << 16) | (b3 << 24);
  const unsigned long long w0 = __ballot(an_ok && end == 0), w1 = __ballot(an_ok && end == 1), w2 = __ballot(an_ok && end == 2);
  if (lane == 0) {
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
    if (w0) atomicAdd(stats + 3, (unsigned long long)__popcll(w0));
    if (w1) atomicAdd(stats + 4, (unsigned long long)__popcll(w1));
    if (w2) atomicAdd(stats + 5, (unsigned long long)__popcll(w2));
  }
}

__global__ __launch_bounds__(RS_T) void rs_scan_kernel(RangesigScanTables T, const float2 *__restrict__ xy,
                                                       const int32_t *__restrict__ offsets, int32_t n_scans, uint32_t *__restrict__ sig,
                                                       uint32_t *status) {
  __shared__ float edge2[256];
  __shared__ float dir_x[32], dir_y[32];
  __shared__ uint32_t sect[64];
  const int tid = threadIdx.x;
  edge2[tid] = T.edge2[tid];
  if (tid < 32) dir_x[tid] = T.dir[2 * tid], dir_y[tid] = T.dir[2 * tid + 1];
  for (int32_t s = blockIdx.x; s < n_scans; s += gridDim.x) {
    if (tid < 64) sect[tid] = 255u;
    __syncthreads();
    int32_t beg = offsets[s], end = offsets[s + 1];
    if (!(beg >= 0 && end >= beg)) {  // (treated as empty: nothing is read)
      if (tid == 0) flag_bad_id(status, BAD_MAP_SCAN_OFFSETS, beg < 0 ? beg : end, beg < 0 ? s : s + 1);
      end = beg = 0;
    }
    for (long long i = (long long)beg + tid; i < end; i += RS_T) {
      const float2 p = xy[i];
      const float r2 = __fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y));
      if (!isfinite(r2)) continue;
      int lo = 1, hi = 255;  // the first k in 1 .. 254 with r2 < edge2[k], 255 without one: the edges ascend
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r2 >= edge2[mid]) lo = mid + 1;
        else hi = mid;
      }
      const bool neg = p.y < 0.0f || (p.y == 0.0f && p.x < 0.0f);
      const float u = neg ? -p.x : p.x, v = neg ? -p.y : p.y;
      int sector = neg ? 32 : 0;
#pragma unroll
      for (int j = 1; j < 32; j++) sector += __fsub_rn(__fmul_rn(dir_x[j], v), __fmul_rn(dir_y[j], u)) >= 0.0f;
      atomicMin(&sect[sector], (uint32_t)(lo - 1));
    }
    __syncthreads();
    if (tid < 16) sig[(size_t)s * 16 + tid] = sect[4 * tid] | (sect[4 * tid + 1] << 8) | (sect[4 * tid + 2] << 16) | (sect[4 * tid + 3] << 24);
    __syncthreads();  // (the sectors are reset for the next scan only after the reads)
  }
}

// Dword P of a 64-byte row rotated up by b = 0 .. 3 bytes: `hi` is dword P of the row, `lo` dword P - 1.  What v_alignbyte_b32
// computes for (hi, lo, 4 - b); written as a funnel shift of a 64-bit value so that wave-uniform operands stay in scalar
// registers (the vector instruction would put its result, and with it the rotated query, into 32 VGPRs).
__device__ __forceinline__ uint32_t rotate_in(uint32_t hi, uint32_t lo, uint32_t b) {
  return (uint32_t)(((((unsigned long long)hi << 32) | lo) << (8u * b)) >> 32);
}

// Query rows [row0, row0 + rows) against every anchor: keys[(a - row0) * pitch + b].  A query with fewer than min_sectors
// sectors has no keys: the selection does not read its row.
__global__ __launch_bounds__(RS_T) void rs_cost_kernel(RangesigParams P, const uint32_t *__restrict__ qsig, int32_t n_queries,
                                                       const uint32_t *__restrict__ asig, const int4 *__restrict__ anchors,
                                                       int32_t n_anchors, uint32_t *__restrict__ keys, int32_t pitch, int32_t row0,
                                                       int32_t rows) {
  const int32_t b = (int32_t)blockIdx.x * RS_T + (int32_t)threadIdx.x;
  const bool have = b < n_anchors;
  uint32_t A[16];
#pragma unroll
  for (int p = 0; p < 16; p++) A[p] = have ? asig[(size_t)b * 16 + p] : 0u;
  const int4 an = have ? anchors[b] : make_int4(-1, -1, -1, -1);
  const bool ok = have && cell_in(P, an.x, an.y);
  const int32_t a_end = min(row0 + min(rows, ((int32_t)blockIdx.y + 1) * RANGESIG_QT), n_queries);
  for (int32_t a = row0 + (int32_t)blockIdx.y * RANGESIG_QT; a < a_end; a++) {  // (uniform)
    uint32_t Q0[16], M0[16];
    int32_t valid = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
      const uint32_t q = __builtin_amdgcn_readfirstlane(qsig[(size_t)a * 16 + p]);
      const uint32_t t = ~q;                                                          // a byte is 0 iff the sector is 255
      const uint32_t hb = (((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;      // 0x80 in every byte that is not
      const uint32_t mask = (hb >> 7) * 0xffu;
      valid += __builtin_popcount(hb);
      Q0[p] = q & mask, M0[p] = mask;
    }
    if (valid < P.min_sectors) continue;
    uint32_t best = RS_KEY_NONE;
#pragma unroll 1
    for (uint32_t bb = 0; bb < 4; bb++) {
      uint32_t Qb[16], Mb[16];  // byte x of these is byte x - bb of the query's
#pragma unroll
      for (int p = 0; p < 16; p++) {
        Qb[p] = rotate_in(Q0[p], Q0[(p + 15) & 15], bb);
        Mb[p] = rotate_in(M0[p], M0[(p + 15) & 15], bb);
      }
#pragma unroll
      for (int d = 0; d < 16; d++) {
        uint32_t acc = 0;
#pragma unroll
        for (int p = 0; p < 16; p++) acc = __builtin_amdgcn_sad_u8(A[p] & Mb[(p - d) & 15], Qb[(p - d) & 15], acc);
        const uint32_t key = (acc << 6) | (4u * (uint32_t)d + bb);
        best = key < best ? key : best;
      }
    }
    if (have) keys[(size_t)(a - row0) * (size_t)pitch + (size_t)b] = ok ? best : RS_KEY_NONE;
  }
}

__global__ __launch_bounds__(RS_T) void rs_topk_kernel(RangesigParams P, const uint8_t *__restrict__ qsig, int32_t n_queries,
                                                       const int4 *__restrict__ anchors, int32_t n_anchors,
                                                       const uint32_t *__restrict__ keys, int32_t pitch, int32_t *__restrict__ records,
                                                       int32_t row0, int32_t rows) {
  const int lane = threadIdx.x & 63;
  const int32_t local = (int32_t)blockIdx.x * RS_WAVES + ((int32_t)threadIdx.x >> 6), a = row0 + local;  // (uniform per wave)
  if (local >= rows || a >= n_queries) return;
  const int32_t valid = (int32_t)__popcll(__ballot(qsig[(size_t)a * 64 + lane] != 255));
  const uint32_t *row = keys + (size_t)local * (size_t)pitch;
  int32_t *rec = records + (size_t)a * P.top_k * 4;
  constexpr unsigned long long NONE = ~0ull;
  int32_t acc_i[RS_MAX_K], acc_j[RS_MAX_K];  // the lattice indices of the accepted anchors (uniform; static indices only)
#pragma unroll
  for (int r = 0; r < RS_MAX_K; r++) acc_i[r] = acc_j[r] = 0;
  bool live = valid >= P.min_sectors;
  int32_t written = 0;
  for (int32_t k = 0; k < P.top_k; k++) {
    unsigned long long m = NONE;
    if (live)
      for (int32_t b = lane; b < n_anchors; b += 64) {
        const uint32_t key = row[b];
        if (key == RS_KEY_NONE) continue;
        const unsigned long long comp = ((unsigned long long)key << 32) | (uint32_t)b;
        if (comp >= m) continue;
        const int4 an = anchors[b];
        bool suppressed = false;
#pragma unroll
        for (int r = 0; r < RS_MAX_K; r++) {
          const long long di = (long long)an.z - acc_i[r], dj = (long long)an.w - acc_j[r];
          suppressed |= r < written && (di < 0 ? -di : di) <= P.min_sep && (dj < 0 ? -dj : dj) <= P.min_sep;
        }
        if (!suppressed) m = comp;
      }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(m, d, 64);
      m = o < m ? o : m;
    }
    int4 out = make_int4(-1, -1, -1, -1);
    if (m == NONE) {
      live = false;
    } else {
      const int32_t b = (int32_t)(uint32_t)m;  // (< n_anchors: it was a lane's index)
      const uint32_t key = (uint32_t)(m >> 32);
      const int4 an = anchors[b];
#pragma unroll
      for (int r = 0; r < RS_MAX_K; r++)
        if (r == written) acc_i[r] = an.z, acc_j[r] = an.w;
      out = make_int4(b, (int32_t)(key & 63u), (int32_t)(key >> 6), valid);
      written++;
    }
    if (lane < 4) rec[4 * k + lane] = lane == 0 ? out.x : lane == 1 ? out.y : lane == 2 ? out.z : out.w;
  }
  if (lane == 0) {
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
    if (written) atomicAdd(stats + 7, (unsigned long long)written);
    else atomicAdd(stats + 6, 1ull);
  }
}

int32_t host_nodes_along(int32_t cells, int32_t stride) {
  const int32_t h = stride / 2;
  return cells > h ? (cells - h - 1) / stride + 1 : 0;
}

}  // namespace

int launch_rangesig_anchors(const RangesigParams &P, const int8_t *d_grid, int32_t max_anchors, int32_t *d_anchors,
                            int32_t *d_row_counts, hipStream_t s) {
  const int32_t nj = host_nodes_along(P.height, P.stride);
  const uint32_t blocks = (uint32_t)((nj + RS_WAVES - 1) / RS_WAVES);
  int4 *anchors = reinterpret_cast<int4 *>(d_anchors);
  if (max_anchors > 0)
    hipLaunchKernelGGL(rs_fill_kernel, dim3((uint32_t)((max_anchors + RS_T - 1) / RS_T)), dim3(RS_T), 0, s, anchors, max_anchors);
  if (blocks) hipLaunchKernelGGL(rs_row_count_kernel, dim3(blocks), dim3(RS_T), 0, s, P, d_grid, d_row_counts);
  hipLaunchKernelGGL(rs_row_scan_kernel, dim3(1), dim3(RS_SCAN_T), 0, s, P, max_anchors, d_row_counts);
  if (blocks && max_anchors > 0)
    hipLaunchKernelGGL(rs_row_pack_kernel, dim3(blocks), dim3(RS_T), 0, s, P, d_grid, max_anchors, d_row_counts, anchors);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_rangesig_map(const RangesigParams &P, const int8_t *d_grid, const int32_t *d_rays, const int32_t *d_anchors,
                        int32_t n_anchors, uint8_t *d_sig, hipStream_t s) {
  NHIP_TRY_HIP(hipMemsetAsync(P.stats + 3, 0, 3 * sizeof(long long), s));
  const long long lanes = (long long)n_anchors * 64 * P.rays_per_sector;  // (<= 2^29)
  if (lanes > 0)
    hipLaunchKernelGGL(rs_map_kernel, dim3((uint32_t)((lanes + RS_T - 1) / RS_T)), dim3(RS_T), 0, s, P, d_grid,
                       reinterpret_cast<const int4 *>(d_rays), reinterpret_cast<const int4 *>(d_anchors), n_anchors,
                       reinterpret_cast<uint32_t *>(d_sig));
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_rangesig_scans(const RangesigScanTables &T, const float *d_xy, const int32_t *d_offsets, int32_t n_scans, uint8_t *d_sig,
                          hipStream_t s) {
  if (n_scans > 0)
    hipLaunchKernelGGL(rs_scan_kernel, dim3((uint32_t)(n_scans < RS_MAX_SCAN_BLOCKS ? n_scans : RS_MAX_SCAN_BLOCKS)), dim3(RS_T), 0, s, T,
                       reinterpret_cast<const float2 *>(d_xy), d_offsets, n_scans, reinterpret_cast<uint32_t *>(d_sig), dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_rangesig_match(const RangesigParams &P, const uint8_t *d_qsig, int32_t n_queries, const uint8_t *d_asig,
                          const int32_t *d_anchors, int32_t n_anchors, int32_t *d_records, uint32_t *d_keys, int32_t pitch,
                          int32_t chunk_rows, hipStream_t s) {
  NHIP_TRY_HIP(hipMemsetAsync(P.stats + 6, 0, 2 * sizeof(long long), s));
  const int4 *anchors = reinterpret_cast<const int4 *>(d_anchors);
  for (int32_t row0 = 0; row0 < n_queries; row0 += chunk_rows) {
    const int32_t rows = n_queries - row0 < chunk_rows ? n_queries - row0 : chunk_rows;
    if (n_anchors > 0) {
      const dim3 grid((uint32_t)((n_anchors + RS_T - 1) / RS_T), (uint32_t)((rows + RANGESIG_QT - 1) / RANGESIG_QT));
      hipLaunchKernelGGL(rs_cost_kernel, grid, dim3(RS_T), 0, s, P, reinterpret_cast<const uint32_t *>(d_qsig), n_queries,
                         reinterpret_cast<const uint32_t *>(d_asig), anchors, n_anchors, d_keys, pitch, row0, rows);
    }
    hipLaunchKernelGGL(rs_topk_kernel, dim3((uint32_t)((rows + RS_WAVES - 1) / RS_WAVES)), dim3(RS_T), 0, s, P, d_qsig, n_queries, anchors,
                       n_anchors, d_keys, pitch, d_records, row0, rows);
  }
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
