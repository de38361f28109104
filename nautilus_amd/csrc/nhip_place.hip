// nhip_place.hip -- K16: place descriptors.  Every scan as R rings x 64 sectors of one bit ("a return fell in this bin"),
// and the appearance match of a list of scans against itself: the Hamming distance of two descriptors under the best of the
// 64 rotations, the K nearest per query.  The spec is DESIGN.md section 3, "Place descriptors"; tests/place_reference.py
// restates it in numpy.  Two float comparisons per point, integers after them: OR and popcount know no order, so the
// results are the reference's bit for bit.
//
//   place_describe_kernel  a workgroup per scan (grid-stride), a lane per point: ring and sector by the spec's COUNTS against
//                          the tables (parameters, copied to LDS; no transcendental here), the bit by LDS atomicOr on the
//                          32-bit half of the ring's word; one store of the R words and of their popcount per scan.
//   place_dist_kernel<R>   a lane per candidate, its R words in VGPRs for PLACE_QT queries in turn; the query's words are
//                          wave-uniform (scalar registers), and it is the QUERY that is rotated -- popcount(rotr64(D_i, s)
//                          XOR D_j) = popcount(D_i XOR rotl64(D_j, s)) -- so the rotation is scalar work and the vector work is
//                          two XORs and two popcount-accumulates per ring and shift.  All 64 shifts in-lane, the best kept
//                          with a strict <: the smallest shift wins.  Both gates are applied here, where both scans' bit
//                          counts are in registers: a uint16 key dist * 64 + shift per (query, candidate), 0xFFFF for a
//                          candidate that is inadmissible or fails the permille gate (dist <= 64 R <= 960 < 1023: R <= 15).
//                          A wave none of whose candidates is admissible for a query -- half of them under PAST_ONLY -- skips it.
//   place_topk_kernel      a wave per query: K rounds of a wave-wide minimum over (dist, position in the list) -- the list
//                          ascends, so that is (dist, j) -- each round the smallest key above the last one taken.
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int DESC_T = 256;
constexpr int DESC_MAX_BLOCKS = 4096;
constexpr int DIST_T = 256;  // candidates per workgroup
constexpr uint32_t KEY_NONE = 0xFFFFu;

__global__ __launch_bounds__(DESC_T) void place_describe_kernel(PlaceTables T, const float2 *__restrict__ xy,
                                                                const int32_t *__restrict__ offsets, int32_t n_scans,
                                                                unsigned long long *__restrict__ desc, int32_t *__restrict__ bits,
                                                                uint32_t *status) {
  __shared__ float edge2[PLACE_MAX_RINGS + 1];
  __shared__ float dir_x[32], dir_y[32];
  __shared__ uint32_t words[2 * PLACE_MAX_RINGS];
  const int tid = threadIdx.x, R = T.n_rings;
  if (tid <= R) edge2[tid] = T.edge2[tid];
  if (tid < 32) dir_x[tid] = T.dir[2 * tid], dir_y[tid] = T.dir[2 * tid + 1];
  for (int32_t s = blockIdx.x; s < n_scans; s += gridDim.x) {
    if (tid < 2 * R) words[tid] = 0u;
    __syncthreads();
    int32_t beg = offsets[s], end = offsets[s + 1];
    if (!(beg >= 0 && end >= beg)) {  // (treated as empty: nothing is read)
      if (tid == 0) flag_bad_id(status, BAD_MAP_SCAN_OFFSETS, beg < 0 ? beg : end, beg < 0 ? s : s + 1);
      end = beg = 0;
    }
    const float outer = edge2[R];
    for (long long i = (long long)beg + tid; i < end; i += DESC_T) {
      const float2 p = xy[i];
      const float r2 = __fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y));
      if (!(isfinite(r2) && r2 < outer)) continue;
      int ring = 0;
      for (int k = 1; k < R; k++) ring += r2 >= edge2[k];
      const bool neg = p.y < 0.0f || (p.y == 0.0f && p.x < 0.0f);
      const float u = neg ? -p.x : p.x, v = neg ? -p.y : p.y;
      int sector = neg ? 32 : 0;
#pragma unroll
      for (int j = 1; j < 32; j++) sector += __fsub_rn(__fmul_rn(dir_x[j], v), __fmul_rn(dir_y[j], u)) >= 0.0f;
      atomicOr(&words[2 * ring + (sector >> 5)], 1u << (sector & 31));
    }
    __syncthreads();
    if (tid < R) desc[(size_t)s * R + tid] = (unsigned long long)words[2 * tid] | ((unsigned long long)words[2 * tid + 1] << 32);
    if (tid == 64) {  // (another wave than the one that stores the words)
      int32_t n = 0;
      for (int k = 0; k < 2 * R; k++) n += __popc(words[k]);
      bits[s] = n;
    }
    __syncthreads();  // (the words are cleared for the next scan only after both reads)
  }
}

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {  // the value of the first lane, in scalar registers
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

// Query rows [row0, row0 + rows) of the list against every candidate: keys[(a - row0) * pitch + b].
template <int R>
__global__ __launch_bounds__(DIST_T) void place_dist_kernel(PlaceMatch P, int32_t row0, int32_t rows) {
  const int32_t b = blockIdx.x * DIST_T + threadIdx.x;
  const bool have = b < P.n_ids;
  int32_t j = have ? P.ids[b] : -1;
  if (have && !id_in(j, P.n_scans)) {
    if (blockIdx.y == 0 && row0 == 0) flag_bad_id(P.status, BAD_PLACE_ID, j, b);  // (once per entry)
    j = -1;
  }
  unsigned long long c[R];
  const int32_t bits_j = j >= 0 ? P.bits[j] : 0;
#pragma unroll
  for (int r = 0; r < R; r++) c[r] = j >= 0 ? P.desc[(size_t)j * R + r] : 0ull;
  const bool past_only = P.flags & NHIP_PLACE_PAST_ONLY;
  unsigned long long n_before = 0, n_after = 0;  // (per wave: every lane holds the wave's count)
  const int32_t a_end = min(row0 + min(rows, ((int32_t)blockIdx.y + 1) * PLACE_QT), P.n_ids);
  for (int32_t a = row0 + (int32_t)blockIdx.y * PLACE_QT; a < a_end; a++) {
    int32_t i = P.ids[a];  // (uniform)
    if (!id_in(i, P.n_scans)) i = -1;
    const int32_t bits_i = i >= 0 ? P.bits[i] : 0;
    const long long sep = (long long)i - j;
    const bool adm = i >= 0 && j >= 0 && (sep < 0 ? -sep : sep) > P.min_separation && (!past_only || j < i) && bits_i > 0 && bits_j > 0;
    uint32_t key = KEY_NONE;
    const unsigned long long any = __ballot(adm);
    if (any) {
      n_before += (unsigned long long)__popcll(any);
      unsigned long long q[R];
#pragma unroll
      for (int r = 0; r < R; r++) q[r] = uniform64(P.desc[(size_t)i * R + r]);
      uint32_t best = 0xFFFFFFFFu, best_s = 0;
      for (uint32_t s = 0; s < 64; s++) {
        uint32_t d = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
          const unsigned long long rot = s ? (q[r] >> s) | (q[r] << (64 - s)) : q[r];
          d += (uint32_t)__popcll(rot ^ c[r]);
        }
        if (d < best) best = d, best_s = s;
      }
      const bool kept = adm && 1000ll * best <= (long long)P.max_permille * ((long long)bits_i + bits_j);
      if (kept) key = best * 64u + best_s;
      n_after += (unsigned long long)__popcll(__ballot(kept));
    }
    if (have) P.keys[(size_t)(a - row0) * P.pitch + b] = (uint16_t)key;
  }
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
    if (n_before) atomicAdd(stats + 1, n_before);
    if (n_after) atomicAdd(stats + 2, n_after);
  }
}

__global__ __launch_bounds__(256) void place_topk_kernel(PlaceMatch P, int32_t row0, int32_t rows) {
  const int lane = threadIdx.x & 63;
  const int32_t local = blockIdx.x * 4 + (threadIdx.x >> 6), a = row0 + local;  // (uniform per wave)
  if (local >= rows || a >= P.n_ids) return;
  unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
  const uint16_t *row = P.keys + (size_t)local * P.pitch;
  int32_t *rec = P.records + (size_t)a * P.top_k * 4;
  constexpr unsigned long long NONE = ~0ull;
  unsigned long long last = 0;  // (composites are (dist << 32 | b) + 1: 0 is below them all)
  int32_t written = 0;
  for (int32_t k = 0; k < P.top_k; k++) {
    unsigned long long m = NONE;
    if (last != NONE)
      for (int32_t b = lane; b < P.n_ids; b += 64) {
        const uint32_t key = row[b];
        if (key == KEY_NONE) continue;
        const unsigned long long comp = (((unsigned long long)(key >> 6) << 32) | (uint32_t)b) + 1ull;
        if (comp > last && comp < m) m = comp;
      }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(m, d, 64);
      m = o < m ? o : m;
    }
    last = m;
    if (lane < 4) {
      int32_t v = -1;
      if (m != NONE) {
        const int32_t b = (int32_t)(uint32_t)(m - 1ull);
        const uint32_t key = row[b];
        const int32_t j = P.ids[b];  // (in range: its key is not KEY_NONE)
        v = lane == 0 ? j : lane == 1 ? (int32_t)(key & 63u) : lane == 2 ? (int32_t)(key >> 6) : P.bits[j];
      }
      rec[4 * k + lane] = v;
    }
    written += m != NONE;
  }
  if (lane == 0) {
    const int32_t i = P.ids[a];
    if (a == 0) atomicAdd(stats + 0, (unsigned long long)P.n_ids);
    if (written) atomicAdd(stats + 3, (unsigned long long)written);
    if (!written) atomicAdd(stats + 4, 1ull);
    if (!id_in(i, P.n_scans) || P.bits[i] == 0) atomicAdd(stats + 5, 1ull);
  }
}

template <int R>
void launch_dist(const PlaceMatch &P, int32_t row0, int32_t rows, hipStream_t s) {
  const dim3 grid((uint32_t)((P.n_ids + DIST_T - 1) / DIST_T), (uint32_t)((rows + PLACE_QT - 1) / PLACE_QT));
  hipLaunchKernelGGL(place_dist_kernel<R>, grid, dim3(DIST_T), 0, s, P, row0, rows);
}

}  // namespace

int launch_place_describe(const PlaceTables &T, const float *d_xy, const int32_t *d_offsets, int32_t n_scans, uint64_t *d_desc,
                          int32_t *d_bits, hipStream_t s) {
  if (n_scans > 0)
    hipLaunchKernelGGL(place_describe_kernel, dim3((uint32_t)(n_scans < DESC_MAX_BLOCKS ? n_scans : DESC_MAX_BLOCKS)), dim3(DESC_T), 0, s, T,
                       reinterpret_cast<const float2 *>(d_xy), d_offsets, n_scans, reinterpret_cast<unsigned long long *>(d_desc), d_bits,
                       dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_place_match(const PlaceMatch &P, int32_t chunk_rows, hipStream_t s) {
  NHIP_TRY_HIP(hipMemsetAsync(P.stats, 0, 8 * sizeof(long long), s));
  for (int32_t row0 = 0; row0 < P.n_ids; row0 += chunk_rows) {
    const int32_t rows = P.n_ids - row0 < chunk_rows ? P.n_ids - row0 : chunk_rows;
    switch (P.n_rings) {
#define NHIP_PLACE_CASE(R) \
  case R: launch_dist<R>(P, row0, rows, s); break;
      NHIP_PLACE_CASE(1) NHIP_PLACE_CASE(2) NHIP_PLACE_CASE(3) NHIP_PLACE_CASE(4) NHIP_PLACE_CASE(5)
      NHIP_PLACE_CASE(6) NHIP_PLACE_CASE(7) NHIP_PLACE_CASE(8) NHIP_PLACE_CASE(9) NHIP_PLACE_CASE(10)
      NHIP_PLACE_CASE(11) NHIP_PLACE_CASE(12) NHIP_PLACE_CASE(13) NHIP_PLACE_CASE(14) NHIP_PLACE_CASE(15)
#undef NHIP_PLACE_CASE
      default: set_error("place_match: n_rings %d outside 1..%d", P.n_rings, PLACE_MATCH_MAX_RINGS); return NHIP_ERR_ARG;
    }
    hipLaunchKernelGGL(place_topk_kernel, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, s, P, row0, rows);
  }
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
