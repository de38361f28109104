// nhip_freespace.hip -- K15: the free-space check of match records.  A record says how much of the source landed on the
// target's blurred hits; this unit says where the rest landed: in space the target's beams crossed (a contradiction), where
// the target saw nothing (a partial overlap), and how many of the source's own beams run through a target hit.  The spec is
// DESIGN.md section 3, "Free-space check"; tests/freespace_reference.py restates it in numpy.  The ray is the occupancy
// grid's (nhip_ray.h), the cells are the matcher's; after the cells everything is integer, so the counts and planes are the
// reference's bit for bit.
//
//   fs_trace_kernel  a workgroup per (target, band): a band is FS_BITMAP_WORDS / words-per-row rows of the slot's hit raster,
//                    border included, ONE BIT PER CELL in LDS in the raster's own layout.  Waves take 64 beams at a time (a
//                    lane per point: the end cell), then every beam in turn, a lane per step k.  Free bits by LDS atomicOr; the
//                    band is written out with plain stores as bits & ~hits, so the plane needs no clearing and no atomics on
//                    global memory.
//   fs_check_kernel  a workgroup per pair, its waves 64 points at a time: a lane rotates its point as the matcher does, forms
//                    the cell and its class -- the dilated hit test reads 2 hit_radius + 1 row windows of the raster with
//                    64-bit loads --, then every kept beam in turn, a lane per step k, the steps in groups of up to four
//                    chunks of 64 whose raster reads are issued together, a ballot per group deciding `through`.  Eight
//                    counters reduced in the wave, summed over the waves in LDS, stored by eight lanes.
#include "nhip_common.h"
#include "nhip_ray.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int FS_T = 512;
constexpr int FS_WAVES = FS_T / 64;
constexpr int FS_BITMAP_WORDS = 15872;  // 62 KB of LDS: two workgroups a CU
constexpr int FS_CHECK_T = 256;
constexpr int FS_CHECK_WAVES = FS_CHECK_T / 64;
enum { FS_DROPPED = 0, FS_OUTSIDE = 1, FS_HIT = 2, FS_FREE = 3, FS_UNKNOWN = 4, FS_NONE = 5 };

__host__ __device__ constexpr int32_t fs_words_per_row(int32_t hits_pitch) { return hits_pitch >> 2; }
__host__ __device__ constexpr int32_t fs_band_rows(int32_t hits_pitch) { return FS_BITMAP_WORDS / fs_words_per_row(hits_pitch); }
// the widest raster the host admits: S / 2 <= RAY_MAX_CELLS
static_assert(FS_BITMAP_WORDS / ((2 * RAY_MAX_CELLS + 1 + 2 * HIT_PAD + 31) / 32) >= 1, "a row of the largest raster fits a band");

// the floor of a coordinate's cell offset (grid geometry, item 1); false: the point is not finite
__device__ __forceinline__ bool cell_floors(const FsParams &P, float x, float y, double *fx, double *fy) {
  if (!isfinite(x) || !isfinite(y)) return false;
  *fx = floor_quotient((double)x, P.res, P.inv_res);
  *fy = floor_quotient((double)y, P.res, P.inv_res);
  return true;
}

__global__ __launch_bounds__(FS_T) void fs_trace_kernel(FsParams P) {
  __shared__ uint32_t bits[FS_BITMAP_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t t = (int32_t)blockIdx.x, band = (int32_t)blockIdx.y;
  const int32_t wpr = fs_words_per_row(P.hits_pitch), band_rows = fs_band_rows(P.hits_pitch), rows_all = P.S + 2 * HIT_PAD;
  const int32_t row0 = band * band_rows;  // raster row of band row 0 (the launch has no band beyond the raster)
  const int32_t rows = rows_all - row0 < band_rows ? rows_all - row0 : band_rows;
  const int32_t half = P.S / 2;
  const int32_t rel0 = row0 - (half + HIT_PAD);  // band row 0 relative to the sensor's row
  const int32_t scan = P.target_ids[t];
  int32_t beg = 0, end = 0;
  if (id_in(scan, P.ids.n_scans)) {
    beg = P.offsets[scan];
    end = P.offsets[scan + 1];
    if (!(beg >= 0 && end >= beg)) beg = end = 0;
  } else if (band == 0 && tid == 0) {
    flag_bad_id(P.ids.status, BAD_TARGET_ID, scan, t);
  }
  for (int32_t j = tid; j < rows * wpr; j += FS_T) bits[j] = 0u;
  __syncthreads();

  for (long long base = (long long)beg + wv * 64; base < end; base += FS_WAVES * 64) {
    const long long i = base + lane;
    int32_t dx = 0, dy = 0;
    bool kept = false;
    if (i < end) {
      const float2 p = P.xy[i];
      double fx, fy;
      if (cell_floors(P, p.x, p.y, &fx, &fy)) {
        const double lo = -(double)half, hi = (double)(P.S - half);
        if (fx >= lo && fx < hi && fy >= lo && fy < hi) {
          dx = (int32_t)fx, dy = (int32_t)fy;  // (|d| <= S / 2 <= RAY_MAX_CELLS)
          kept = true;
        }
      }
    }
    unsigned long long todo = __ballot(kept);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int32_t bdx = __shfl(dx, b, 64), bdy = __shfl(dy, b, 64);
      const int32_t ax = bdx < 0 ? -bdx : bdx, ay = bdy < 0 ? -bdy : bdy, n = ax > ay ? ax : ay;
      if (n == 0) continue;
      // the steps whose row can lie in the band, two steps wide on both sides (as occ_trace_kernel narrows them); the test on
      // the row itself, below, decides
      int32_t k_lo = 0, k_hi = n;
      const int32_t ra = bdy < 0 ? -(rel0 + rows - 1) : rel0, rb = bdy < 0 ? -rel0 : rel0 + rows - 1;
      if (ay == 0) {
        if (ra > 0 || rb < 0) continue;
      } else {
        const int32_t lo = ((2 * ra - 1) * n) / (2 * ay) - 2, hi = ((2 * rb + 1) * n) / (2 * ay) + 3;
        k_lo = lo > 0 ? lo : 0;
        k_hi = hi < n ? hi : n;
      }
      const float inv_den = 1.0f / (float)(2 * n);
      const bool x_major = ax >= ay;
      const int32_t major = x_major ? (bdx < 0 ? -1 : 1) : (bdy < 0 ? -1 : 1), minor = x_major ? bdy : bdx;
      for (int32_t k = k_lo + lane; k < k_hi; k += 64) {
        const int32_t u = major * k, v = rdiv(k * minor, n, inv_den);  // (on the major axis rdiv(k d, n) is +-k exactly)
        const int32_t ry = (x_major ? v : u) - rel0, bx = (x_major ? u : v) + half + HIT_PAD;
        if ((uint32_t)ry >= (uint32_t)rows) continue;
        atomicOr(&bits[ry * wpr + (bx >> 5)], 1u << (bx & 31));  // (a free cell lies between the sensor and an end cell: in the grid)
      }
    }
  }
  __syncthreads();
  // ---- a cell that stops any beam is not free: the band minus the slot's hits, in whole words
  const uint32_t *hits = reinterpret_cast<const uint32_t *>(P.grids + (size_t)t * P.slot_bytes + P.hits_offset);
  uint32_t *out = reinterpret_cast<uint32_t *>(P.free_planes + (size_t)t * P.hits_bytes);
  const size_t first = (size_t)row0 * wpr;
  for (int32_t j = tid; j < rows * wpr; j += FS_T) out[first + j] = bits[j] & ~hits[first + j];
  if (row0 + rows == rows_all) {  // the words behind the last row (a window's second dword may fall there)
    const int32_t n_all = (int32_t)(P.hits_bytes >> 2);
    for (int32_t j = rows_all * wpr + tid; j < n_all; j += FS_T) out[j] = 0u;
  }
}

// a source beam under the matched pose: what its steps need (the same in every lane)
struct FsBeam {
  const uint32_t *hits32;  // the slot's hit raster
  long long ocx, ocy;      // the source sensor's cell
  int32_t S, wpr, n, k_end, major, minor;
  bool x_major;
  float inv_den;
};
// whether one of this lane's steps of chunks c0 .. c0 + NC - 1 is a target hit (steps k < k_end, cells inside the grid)
template <int NC>
__device__ __forceinline__ bool fs_steps(const FsBeam &B, int32_t c0, int lane) {
  uint32_t word[NC], bit[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) {
    const int32_t k = ((c0 + j) << 6) + lane;
    const bool on = k < B.k_end;
    const int32_t ks = on ? k : 0;
    const int32_t u = B.major * ks, v = rdiv_straight(ks * B.minor, B.n, B.inv_den);  // (on the major axis rdiv(k d, n) is +-k exactly)
    const long long col = B.ocx + (B.x_major ? u : v), row = B.ocy + (B.x_major ? v : u);
    const bool in = on && col >= 0 && col < B.S && row >= 0 && row < B.S;  // (ray cells outside the grid are skipped one by one)
    const uint32_t cb = (uint32_t)col + HIT_PAD;
    const uint32_t at = in ? (uint32_t)((int32_t)row + HIT_PAD) * (uint32_t)B.wpr + (cb >> 5) : 0u;
    word[j] = B.hits32[at];
    bit[j] = in ? (cb & 31u) | 32u : 0u;  // (bit 5: the step counts)
  }
  uint32_t found = 0u;
#pragma unroll
  for (int j = 0; j < NC; j++) found |= (word[j] >> (bit[j] & 31u)) & (bit[j] >> 5);
  return found != 0u;
}

__global__ __launch_bounds__(FS_CHECK_T) void fs_check_kernel(FsParams P) {
  __shared__ int32_t part[FS_CHECK_WAVES][8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // consecutive pairs (one target's, usually) on ONE XCD, as in csm_exact_score_kernel: its L2 fetches the target's rasters once
  const int32_t pair = (int32_t)(blockIdx.x & 7u) * P.pairs_per_xcd + (int32_t)(blockIdx.x >> 3);
  if (pair >= P.n_pairs) return;
  int32_t *out = P.counts + 8 * (size_t)pair;
  const nhip_match_t m = P.matches[pair];
  if (m.itheta < 0) {  // a rejected record
    if (tid < 8) out[tid] = -1;
    return;
  }
  const int32_t src = P.pair_src[pair], slot = P.pair_slot[pair];
  const bool src_ok = id_in(src, P.ids.n_scans), slot_ok = id_in(slot, P.ids.n_slots);
  const bool rec_ok = m.itheta < P.n_theta && id_in(m.ix, P.nx) && id_in(m.iy, P.ny);
  if (!(src_ok && slot_ok && rec_ok)) {  // never dereferenced: eight zeros, and the status word
    if (tid == 0) flag_bad_id(P.ids.status, BAD_FREESPACE_PAIR, !src_ok ? src : (!slot_ok ? slot : m.itheta), pair);
    if (tid < 8) out[tid] = 0;
    return;
  }
  int32_t beg = P.offsets[src], end = P.offsets[src + 1];
  if (!(beg >= 0 && end >= beg)) beg = end = 0;
  // rotation itheta: R(theta0) * R(delta_k), composed in double with individually rounded ops, as every matcher kernel
  const double c0 = P.rot0_cs[2 * (size_t)pair], s0 = P.rot0_cs[2 * (size_t)pair + 1];
  const double cd = P.delta_cs[2 * m.itheta], sd = P.delta_cs[2 * m.itheta + 1];
  const float cf = __double2float_rn(__dsub_rn(__dmul_rn(c0, cd), __dmul_rn(s0, sd)));
  const float sf = __double2float_rn(__dadd_rn(__dmul_rn(s0, cd), __dmul_rn(c0, sd)));
  // the shift of the matched pose, and the source sensor's cell under it (int64: an origin is any int32)
  const long long sx = (long long)(P.pair_origin ? P.pair_origin[2 * (size_t)pair] : 0) + m.ix - P.hx;
  const long long sy = (long long)(P.pair_origin ? P.pair_origin[2 * (size_t)pair + 1] : 0) + m.iy - P.hy;
  const long long half = P.S / 2, ocx = half + sx, ocy = half + sy;
  const int32_t wpr = P.hits_pitch >> 2, r = P.hit_radius;
  const uint8_t *hits = P.grids + (size_t)slot * P.slot_bytes + P.hits_offset;
  const uint32_t *hits32 = reinterpret_cast<const uint32_t *>(hits);
  const uint32_t *free32 = reinterpret_cast<const uint32_t *>(P.free_planes + (size_t)slot * P.hits_bytes);
  const unsigned long long mask = (1ull << (2 * r + 1)) - 1ull;  // (r <= 16: at most 33 bits, 31 + 33 <= 64)

  int32_t n_class[5] = {0, 0, 0, 0, 0}, n_points = 0, n_through = 0;  // (n_through: the wave's, the same in every lane)
  for (long long base = (long long)beg + wv * 64; base < end; base += FS_CHECK_WAVES * 64) {
    const long long i = base + lane;
    int kind = FS_NONE;
    int32_t dx = 0, dy = 0;
    if (i < end) {
      const float2 q = P.xy[i];
      const float xr = __fsub_rn(__fmul_rn(cf, q.x), __fmul_rn(sf, q.y));
      const float yr = __fadd_rn(__fmul_rn(sf, q.x), __fmul_rn(cf, q.y));
      double fx, fy;
      kind = FS_DROPPED;
      if (cell_floors(P, xr, yr, &fx, &fy)) {
        kind = FS_OUTSIDE;
        if (fabs(fx) <= (double)RAY_MAX_CELLS && fabs(fy) <= (double)RAY_MAX_CELLS) {
          dx = (int32_t)fx, dy = (int32_t)fy;
          const long long col = ocx + dx, row = ocy + dy;
          if (col >= 0 && col < P.S && row >= 0 && row < P.S) {
            // ---- any hit within Chebyshev distance r: the 2 r + 1 row windows, OR-ed (the border of 32 cells holds them)
            const uint32_t bit0 = (uint32_t)((int32_t)col - r + HIT_PAD), sh = bit0 & 31u;
            const uint8_t *w = hits + (size_t)((int32_t)row - r + HIT_PAD) * P.hits_pitch + 4 * (size_t)(bit0 >> 5);
            struct __attribute__((packed, aligned(4))) Win { uint32_t lo, hi; };
            unsigned long long any = 0ull;
            for (int32_t j = 0; j <= 2 * r; j++) {
              const Win win = *reinterpret_cast<const Win *>(w + (size_t)j * P.hits_pitch);
              any |= ((unsigned long long)win.hi << 32) | win.lo;
            }
            const uint32_t cb = (uint32_t)col + HIT_PAD;
            const uint32_t fbit = (free32[(size_t)((int32_t)row + HIT_PAD) * wpr + (cb >> 5)] >> (cb & 31u)) & 1u;
            kind = ((any >> sh) & mask) ? FS_HIT : (fbit ? FS_FREE : FS_UNKNOWN);
          }
        }
      }
      n_points++;
#pragma unroll
      for (int c = 0; c < 5; c++) n_class[c] += kind == c;  // (no indexed register array)
    }
    // ---- through: every kept beam in turn, a lane per step; the hit test here is undilated
    unsigned long long todo = __ballot(kind == FS_HIT || kind == FS_FREE || kind == FS_UNKNOWN);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int32_t bdx = __shfl(dx, b, 64), bdy = __shfl(dy, b, 64);
      const int32_t ax = bdx < 0 ? -bdx : bdx, ay = bdy < 0 ? -bdy : bdy, n = ax > ay ? ax : ay;
      const int32_t k_end = n - P.end_margin;  // steps 0 .. n - 1 - end_margin
      if (k_end <= 0) continue;
      const float inv_den = 1.0f / (float)(2 * n);
      const bool x_major = ax >= ay;
      const int32_t major = x_major ? (bdx < 0 ? -1 : 1) : (bdy < 0 ? -1 : 1), minor = x_major ? bdy : bdx;
      // 64 steps are a chunk; the chunks go in groups of up to four whose loads are issued together (straight-line code: a
      // step that is not examined, or whose cell is outside the grid, reads word 0 of the raster and masks it), one ballot a
      // group -- a ballot a chunk made every chunk a memory round trip of its own
      const FsBeam beam = {hits32, ocx, ocy, P.S, wpr, n, k_end, major, minor, x_major, inv_den};
      const int32_t chunks = (k_end + 63) >> 6;
      for (int32_t c0 = 0; c0 < chunks;) {
        const int32_t left = chunks - c0;
        bool found;
        if (left >= 3) {
          found = fs_steps<4>(beam, c0, lane);
          c0 += 4;
        } else if (left == 2) {
          found = fs_steps<2>(beam, c0, lane);
          c0 += 2;
        } else {
          found = fs_steps<1>(beam, c0, lane);
          c0 += 1;
        }
        if (__ballot(found)) {
          n_through++;
          break;
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_points += __shfl_xor(n_points, d, 64);
#pragma unroll
    for (int c = 0; c < 5; c++) n_class[c] += __shfl_xor(n_class[c], d, 64);
  }
  if (lane == 0) {
    part[wv][0] = n_points;
#pragma unroll
    for (int c = 0; c < 5; c++) part[wv][1 + c] = n_class[c];
    part[wv][6] = n_through;
    part[wv][7] = 0;
  }
  __syncthreads();
  if (tid < 8) {
    int32_t sum = 0;
#pragma unroll
    for (int w = 0; w < FS_CHECK_WAVES; w++) sum += part[w][tid];
    out[tid] = sum;
  }
}

}  // namespace

int launch_fs_trace(const FsParams &P, hipStream_t s) {
  if (P.n_targets <= 0) return NHIP_OK;
  const int32_t rows_all = P.S + 2 * HIT_PAD, band_rows = fs_band_rows(P.hits_pitch);
  const int32_t bands = (rows_all + band_rows - 1) / band_rows;
  hipLaunchKernelGGL(fs_trace_kernel, dim3((uint32_t)P.n_targets, (uint32_t)bands), dim3(FS_T), 0, s, P);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_fs_check(const FsParams &P0, hipStream_t s) {
  if (P0.n_pairs <= 0) return NHIP_OK;
  FsParams P = P0;
  P.pairs_per_xcd = (P.n_pairs + 7) / 8;
  hipLaunchKernelGGL(fs_check_kernel, dim3(8u * (uint32_t)P.pairs_per_xcd), dim3(FS_CHECK_T), 0, s, P);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
