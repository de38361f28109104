// nhip_occupancy.hip -- K14: the occupancy grid.  Every scan at its pose, free space ray-traced from the sensor's cell to the
// cell of every return, one observation per scan and cell, classified into ROS OccupancyGrid values.  The spec is DESIGN.md
// section 3, "Occupancy grid"; tests/occupancy_reference.py restates it in numpy.  After the cells everything is integer, so
// sums by atomics are order-free and the results are the reference's bit for bit.
//
//   occ_trace_kernel     a workgroup per (scan, band): a band is OCC_BITMAP_WORDS / words-per-row rows of the scan's
//                        (2 max_ray_cells + 1)^2 box, cut to the extent of the scan's end cells and to the rows the window
//                        holds (a room of 320 rows is ONE band of the default box's four), ONE BIT PER CELL in LDS.  Waves take
//                        64 beams at a time (a lane per point: transform, cells, kept / long / dropped), then every kept beam
//                        in turn, a lane per step k (closed form: any lane computes any step).  Free bits by LDS atomicOr; the
//                        end cells' bits cleared (H wins); the words swept row by row, a lane per cell, one no-return
//                        atomicAdd on `misses` per set bit -- consecutive lanes, consecutive cells of a row; the bitmap,
//                        cleared by the sweep, takes H and is swept into `hits`.  A scan costs its planes one atomic per
//                        DISTINCT cell, not one per ray step, and the cell under the sensor one, not a thousand.
//   occ_classify_kernel  one pass over the window: 16-byte loads of both planes, four cells of `grid` per store, the three
//                        cell counts reduced per workgroup, one atomic each.
#include "nhip_common.h"
#include "nhip_ray.h"  // (rdiv: the ray's step, shared with K15)

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int OCC_T = 512;
constexpr int OCC_WAVES = OCC_T / 64;
constexpr int OCC_BITMAP_WORDS = 15872;  // 62 KB of LDS: two workgroups a CU; a band is OCC_BITMAP_WORDS / words-per-row rows
constexpr int OCC_MAX_SCAN_BLOCKS = 1024;  // workgroups along the scans (times the bands); more scans than that: grid-stride
constexpr int CLS_T = 256;
constexpr int CLS_BLOCKS = 2048;
enum { BEAM_NONE = 0, BEAM_KEPT = 1, BEAM_LONG = 2, BEAM_DROPPED = 3 };
// TIMING ONLY, never shipped (make step-atomics; tools/occupancy_bench.py --step-atomics-lib): every ray step adds straight to
// `misses` with a global atomic.  That form counts steps, not scans -- its planes are not the spec's -- and exists to price
// the LDS bitmap against it.
#ifdef NHIP_OCC_STEP_ATOMICS
constexpr bool STEP_ATOMICS = true;
#else
constexpr bool STEP_ATOMICS = false;
#endif

__host__ __device__ constexpr int32_t occ_words_per_row(int32_t max_ray_cells) { return (2 * max_ray_cells + 1 + 31) >> 5; }
__host__ __device__ constexpr int32_t occ_band_rows(int32_t max_ray_cells) { return OCC_BITMAP_WORDS / occ_words_per_row(max_ray_cells); }
static_assert(occ_band_rows(4096) >= 1 && occ_words_per_row(4096) * occ_band_rows(4096) <= OCC_BITMAP_WORDS, "a row of the largest box fits");

struct ScanFrame {  // of one scan: its affine and its origin's floors
  float c, sn, tx, ty;
  double fox, foy;
};

// point i of the scan: kept (dx, dy: end cell minus origin cell), long or dropped
__device__ __forceinline__ int beam_of(const OccParams &P, const ScanFrame &F, const float2 p, int32_t *dx, int32_t *dy) {
  const float x = __fadd_rn(__fadd_rn(__fmul_rn(F.c, p.x), __fmul_rn(-F.sn, p.y)), F.tx);
  const float y = __fadd_rn(__fadd_rn(__fmul_rn(F.sn, p.x), __fmul_rn(F.c, p.y)), F.ty);
  if (!isfinite(x) || !isfinite(y)) return BEAM_DROPPED;
  const double fx = floor_quotient((double)x, P.res, P.inv_res), fy = floor_quotient((double)y, P.res, P.inv_res);
  if (!(fabs(fx) < 0x1p62) || !(fabs(fy) < 0x1p62)) return BEAM_DROPPED;
  const double ddx = __dsub_rn(fx, F.fox), ddy = __dsub_rn(fy, F.foy);
  if (fabs(ddx) > (double)P.max_ray_cells || fabs(ddy) > (double)P.max_ray_cells) return BEAM_LONG;
  *dx = (int32_t)ddx;
  *dy = (int32_t)ddy;
  return BEAM_KEPT;
}

struct Band {          // the part of a scan's box one workgroup holds: rows [rel0, rel0 + rows) relative to the origin's row
  int32_t rows, rel0;  // (0 rows: nothing of the box is in the window for this band)
  int32_t c_lo, c_hi;  // box columns [c_lo, c_hi) lie inside the window
  int32_t wpr;
  long long first;     // index in a plane of (band row 0, box column 0): may be negative, is not for a column in [c_lo, c_hi)
};

// every set bit of the band inside the window becomes one add on `plane`; the swept words are left zero
__device__ __forceinline__ void occ_sweep(uint32_t *bits, const Band &B, int32_t width, int32_t *plane) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t p_lo = B.c_lo >> 6, p_hi = (B.c_hi + 63) >> 6;
  for (int32_t r = wv; r < B.rows; r += OCC_WAVES) {
    uint32_t *row = bits + r * B.wpr;
    const long long at = B.first + (long long)r * width;
    for (int32_t p = p_lo; p < p_hi; p++) {
      const int32_t col = p * 64 + lane, w = col >> 5;
      const uint32_t word = w < B.wpr ? row[w] : 0u;
      if (((word >> (col & 31)) & 1u) && col >= B.c_lo && col < B.c_hi) atomicAdd(&plane[(size_t)(at + col)], 1);
      if ((lane & 31) == 0 && w < B.wpr) row[w] = 0u;  // (after the wave's read of it: one instruction stream)
    }
  }
}

__device__ __forceinline__ void occ_trace_scan(const OccParams &P, int32_t s, int32_t band, uint32_t *bits, int32_t *tally,
                                               const float2 *__restrict__ xy, const int32_t *__restrict__ offsets,
                                               const float *__restrict__ affines) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
  const int32_t beg = offsets[s], end = offsets[s + 1];
  if (!(beg >= 0 && end >= beg)) {  // (treated as empty: nothing is read)
    if (band == 0 && tid == 0) {
      flag_bad_id(P.status, BAD_MAP_SCAN_OFFSETS, beg < 0 ? beg : end, beg < 0 ? s : s + 1);
      atomicAdd(stats + 1, 1ull);
    }
    return;
  }
  ScanFrame F;
  F.c = affines[4 * (size_t)s], F.sn = affines[4 * (size_t)s + 1], F.tx = affines[4 * (size_t)s + 2], F.ty = affines[4 * (size_t)s + 3];
  F.fox = F.foy = 0.0;
  bool ok = isfinite(F.tx) && isfinite(F.ty);
  if (ok) {
    F.fox = floor_quotient((double)F.tx, P.res, P.inv_res), F.foy = floor_quotient((double)F.ty, P.res, P.inv_res);
    ok = fabs(F.fox) < 0x1p62 && fabs(F.foy) < 0x1p62;
  }
  if (!ok) {  // the scan is dropped
    if (band == 0 && tid == 0) atomicAdd(stats + 1, 1ull);
    return;
  }
  // Everything below is in int64 where the origin enters: |ox|, |oy| < 2^62 and the window's terms are int32, so no sum wraps
  // and every comparison is made on the true values.
  const long long ox = (long long)F.fox, oy = (long long)F.foy;
  const int32_t R = P.max_ray_cells, side = 2 * R + 1;
  // ---- the extent of the kept beams' end cells, the origin's (0, 0) included: a free cell lies between the origin and its
  // beam's end on both axes, so only that part of the box is banded, marked and swept (it changes no result)
  int32_t *ext = tally + 4;  // {min dx, max dx, min dy, max dy}
  if (tid < 8) tally[tid] = 0;
  __syncthreads();
  {
    int32_t lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0;
    for (long long i = (long long)beg + tid; i < end; i += OCC_T) {
      int32_t dx = 0, dy = 0;
      if (beam_of(P, F, xy[i], &dx, &dy) != BEAM_KEPT) continue;
      lo_x = dx < lo_x ? dx : lo_x, hi_x = dx > hi_x ? dx : hi_x;
      lo_y = dy < lo_y ? dy : lo_y, hi_y = dy > hi_y ? dy : hi_y;
    }
    atomicMin(&ext[0], lo_x);
    atomicMax(&ext[1], hi_x);
    atomicMin(&ext[2], lo_y);
    atomicMax(&ext[3], hi_y);
  }
  __syncthreads();
  const int32_t lo_x = ext[0], hi_x = ext[1], lo_y = ext[2], hi_y = ext[3];  // (-R <= lo <= 0 <= hi <= R)
  Band B;
  B.wpr = occ_words_per_row(R);
  const int32_t band_rows = occ_band_rows(R);
  const long long y_lo = oy + lo_y > (long long)P.cell_y0 ? oy + lo_y : (long long)P.cell_y0;
  const long long y_end = oy + hi_y + 1 < (long long)P.cell_y0 + P.height ? oy + hi_y + 1 : (long long)P.cell_y0 + P.height;
  const long long row0 = y_lo + (long long)band * band_rows;  // world row of band row 0
  const long long cxs = (ox - R) - (long long)P.cell_x0;      // window column of box column 0
  B.c_lo = cxs < 0 ? (int32_t)(-cxs < (long long)side ? -cxs : (long long)side) : 0;
  const long long room = (long long)P.width - cxs;
  B.c_hi = room <= 0 ? 0 : (int32_t)(room < (long long)side ? room : (long long)side);
  B.c_lo = B.c_lo > lo_x + R ? B.c_lo : lo_x + R;
  B.c_hi = B.c_hi < hi_x + R + 1 ? B.c_hi : hi_x + R + 1;
  B.rows = 0, B.rel0 = 0, B.first = 0;
  if (row0 < y_end && B.c_lo < B.c_hi) {
    B.rows = (int32_t)(y_end - row0 < (long long)band_rows ? y_end - row0 : (long long)band_rows);
    B.rel0 = (int32_t)(row0 - oy);  // in [lo_y, hi_y]
    B.first = (row0 - (long long)P.cell_y0) * P.width + cxs;
  }
  const bool active = B.rows > 0;
  if (!active && band != 0) return;  // (band 0 still counts the scan's beams)
  if (band == 0 && tid == 0) atomicAdd(stats + 0, 1ull);
  for (int32_t j = tid; j < B.rows * B.wpr; j += OCC_T) bits[j] = 0u;
  __syncthreads();

  // ---- F: the free cells of every kept beam
  int32_t n_kept = 0, n_long = 0, n_dropped = 0;
  for (long long base = (long long)beg + wv * 64; base < end; base += OCC_WAVES * 64) {
    const long long i = base + lane;
    int32_t dx = 0, dy = 0;
    const int kind = i < end ? beam_of(P, F, xy[i], &dx, &dy) : BEAM_NONE;
    n_kept += kind == BEAM_KEPT, n_long += kind == BEAM_LONG, n_dropped += kind == BEAM_DROPPED;
    if (!active) continue;
    unsigned long long todo = __ballot(kind == BEAM_KEPT);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int32_t bdx = __shfl(dx, b, 64), bdy = __shfl(dy, b, 64);
      const int32_t ax = bdx < 0 ? -bdx : bdx, ay = bdy < 0 ? -bdy : bdy, n = ax > ay ? ax : ay;
      if (n == 0) continue;
      // The steps whose row can lie in the band: row(k) is k bdy / n rounded, so row(k) in [ra, rb] needs
      // (2 ra - 1) n <= 2 k |bdy| < (2 rb + 1) n (mirrored for bdy < 0); taken two steps wide on both sides, which covers C's
      // truncation and the half that rounds up -- the test on the row itself, below, decides
      int32_t k_lo = 0, k_hi = n;
      const int32_t ra = bdy < 0 ? -(B.rel0 + B.rows - 1) : B.rel0, rb = bdy < 0 ? -B.rel0 : B.rel0 + B.rows - 1;
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
        const int32_t ry = (x_major ? v : u) - B.rel0, bx = (x_major ? u : v) + R;
        if ((uint32_t)ry >= (uint32_t)B.rows) continue;
        if (!STEP_ATOMICS)
          atomicOr(&bits[ry * B.wpr + (bx >> 5)], 1u << (bx & 31));  // (0 <= bx < side)
        else if (bx >= B.c_lo && bx < B.c_hi)
          atomicAdd(&P.misses[(size_t)(B.first + (long long)ry * P.width + bx)], 1);
      }
    }
  }
  if (band == 0) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      n_kept += __shfl_xor(n_kept, d, 64);
      n_long += __shfl_xor(n_long, d, 64);
      n_dropped += __shfl_xor(n_dropped, d, 64);
    }
    if (lane == 0) {
      atomicAdd(&tally[0], n_kept);
      atomicAdd(&tally[1], n_long);
      atomicAdd(&tally[2], n_dropped);
    }
  }
  __syncthreads();
  if (band == 0 && tid < 3 && tally[tid]) atomicAdd(stats + 2 + tid, (unsigned long long)tally[tid]);
  if (!active) return;

  // ---- H wins: the end cells' bits cleared, F swept into misses; then the bitmap takes H and is swept into hits
  for (int pass = STEP_ATOMICS ? 1 : 0; pass < 2; pass++) {
    for (long long i = (long long)beg + tid; i < end; i += OCC_T) {
      int32_t dx = 0, dy = 0;
      if (beam_of(P, F, xy[i], &dx, &dy) != BEAM_KEPT) continue;
      const int32_t ry = dy - B.rel0, bx = dx + R;
      if ((uint32_t)ry >= (uint32_t)B.rows) continue;
      uint32_t *w = &bits[ry * B.wpr + (bx >> 5)];
      if (pass == 0)
        atomicAnd(w, ~(1u << (bx & 31)));
      else
        atomicOr(w, 1u << (bx & 31));
    }
    __syncthreads();
    occ_sweep(bits, B, P.width, pass == 0 ? P.misses : P.hits);
    __syncthreads();
  }
}

__global__ __launch_bounds__(OCC_T) void occ_trace_kernel(OccParams P, const float2 *__restrict__ xy,
                                                          const int32_t *__restrict__ offsets,
                                                          const float *__restrict__ affines) {
  __shared__ uint32_t bits[OCC_BITMAP_WORDS];
  __shared__ int32_t tally[8];  // {beams kept, long, dropped, -, the extent's four}
  for (int32_t s = blockIdx.x; s < P.n_scans; s += gridDim.x) {
    occ_trace_scan(P, s, (int32_t)blockIdx.y, bits, tally, xy, offsets, affines);
    __syncthreads();  // (the returns above are the whole workgroup's)
  }
}

__device__ __forceinline__ int32_t occ_class(const OccParams &P, int32_t h, int32_t m, int32_t *n) {
  const long long obs = (long long)h + m;
  int32_t v = -1, k = 2;
  if (obs >= P.min_obs) {
    if (1000ll * h >= (long long)P.occ_permille * obs)
      v = 100, k = 0;
    else if (1000ll * h <= (long long)P.free_permille * obs)
      v = 0, k = 1;
  }
  n[k]++;
  return v;
}

__global__ __launch_bounds__(CLS_T) void occ_classify_kernel(OccParams P) {
  __shared__ int32_t total[3];
  const int tid = threadIdx.x;
  if (tid < 3) total[tid] = 0;
  __syncthreads();
  const int32_t cells = P.width * P.height, groups = cells >> 2;  // (<= 2^28 cells)
  int32_t n[3] = {0, 0, 0};
  const int4 *hits4 = reinterpret_cast<const int4 *>(P.hits), *misses4 = reinterpret_cast<const int4 *>(P.misses);
  uint32_t *grid4 = reinterpret_cast<uint32_t *>(P.grid);
  for (int32_t g = blockIdx.x * CLS_T + tid; g < groups; g += gridDim.x * CLS_T) {
    const int4 h = hits4[g], m = misses4[g];
    const uint32_t a = (uint32_t)occ_class(P, h.x, m.x, n) & 255u, b = (uint32_t)occ_class(P, h.y, m.y, n) & 255u,
                   c = (uint32_t)occ_class(P, h.z, m.z, n) & 255u, d = (uint32_t)occ_class(P, h.w, m.w, n) & 255u;
    grid4[g] = a | (b << 8) | (c << 16) | (d << 24);
  }
  if (blockIdx.x == 0 && tid < (cells & 3)) {  // the cells behind the last whole group
    const int32_t i = (groups << 2) + tid;
    P.grid[i] = (int8_t)occ_class(P, P.hits[i], P.misses[i], n);
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n[k] += __shfl_xor(n[k], d, 64);
    if ((tid & 63) == 0 && n[k]) atomicAdd(&total[k], n[k]);
  }
  __syncthreads();
  if (tid < 3 && total[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(P.stats) + 5 + tid, (unsigned long long)total[tid]);
}

}  // namespace

int launch_occupancy(const OccParams &P, bool clear, const float *d_xy, const int32_t *d_offsets, const float *d_affines,
                     hipStream_t s) {
  const size_t cells = (size_t)P.width * (size_t)P.height;
  timer_begin(NHIP_TIMER_OCC_TRACE, s);
  NHIP_TRY_HIP(hipMemsetAsync(P.stats, 0, 8 * sizeof(long long), s));
  if (clear) {
    NHIP_TRY_HIP(hipMemsetAsync(P.hits, 0, sizeof(int32_t) * cells, s));
    NHIP_TRY_HIP(hipMemsetAsync(P.misses, 0, sizeof(int32_t) * cells, s));
  }
  if (P.n_scans > 0) {
    const int32_t bands = (2 * P.max_ray_cells + 1 + occ_band_rows(P.max_ray_cells) - 1) / occ_band_rows(P.max_ray_cells);
    hipLaunchKernelGGL(occ_trace_kernel, dim3((uint32_t)(P.n_scans < OCC_MAX_SCAN_BLOCKS ? P.n_scans : OCC_MAX_SCAN_BLOCKS), (uint32_t)bands), dim3(OCC_T), 0, s,
                       P, reinterpret_cast<const float2 *>(d_xy), d_offsets, d_affines);
  }
  timer_end(NHIP_TIMER_OCC_TRACE, s);
  timer_begin(NHIP_TIMER_OCC_CLASSIFY, s);
  const size_t want = (cells / 4 + CLS_T - 1) / CLS_T;
  hipLaunchKernelGGL(occ_classify_kernel, dim3((uint32_t)(want < 1 ? 1 : want < CLS_BLOCKS ? want : CLS_BLOCKS)), dim3(CLS_T), 0, s, P);
  timer_end(NHIP_TIMER_OCC_CLASSIFY, s);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
