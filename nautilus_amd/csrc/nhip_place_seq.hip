// nhip_place_seq.hip -- K16b: place sequences.  The appearance match of K16 (nhip_place.hip) taken over a window of frames
// around both scans of a pair: the sum of the single-scan distances of the frames i + d step and j +- d step, d = -W .. W, in
// both directions of travel, the better direction kept, the permille gate taken on the window.  The spec is DESIGN.md section 3,
// "Place sequences"; tests/place_seq_reference.py restates it in numpy.  Integers only: the results are the reference's bit for
// bit.  Query SCANS go in chunks [s0, s0 + S) of the workspace; a list entry belongs to the chunk that holds its scan id.
//
//   place_seq_plane_kernel<R>  the single distances by scan id: rows [r0, r0 + rows) = the chunk's scans and their halo of
//                              W step scans on either side, clipped to the scans; columns all scans.  K16's arithmetic -- a lane
//                              per column, its R words in VGPRs, the row's words wave-uniform and rotated in scalar registers --
//                              without gates: a uint16 key dist * 64 + shift, 0xFFFF where either scan has no bits.  Every
//                              (row, column) is computed once per chunk, not once per window offset.
//   place_seq_window_kernel    a lane per candidate entry, the query entry uniform: 2 (2W + 1) two-byte reads of the plane --
//                              consecutive along a row for consecutive j -- both directions, the choice, the gate, and a uint16
//                              key seq (<= 16,320; 0xFFFF for none) per (query scan, candidate entry).  Stats from wave ballots.
//   place_seq_topk_kernel      a wave per query entry: K rounds of a wave-wide minimum over (seq, position in the list), as in
//                              K16; then lane k recomputes the window of winner k from the plane, still resident, and writes
//                              its eight fields.
#include "nhip_common.h"

namespace nhip {

namespace {

constexpr int DIST_T = 256;  // columns per workgroup of the plane kernel
constexpr int WIN_T = 256;   // candidate entries per workgroup of the window kernel
constexpr int WIN_QT = 32;   // query entries a workgroup of the window kernel looks at (n_ids <= 2^20: at most 32768 along y)
constexpr uint32_t KEY_NONE = 0xFFFFu;

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {  // the value of the first lane, in scalar registers
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

template <int R>
__global__ __launch_bounds__(DIST_T) void place_seq_plane_kernel(PlaceSeq P, int32_t r0, int32_t rows) {
  const int32_t j = blockIdx.x * DIST_T + threadIdx.x;
  const bool have = j < P.n_scans;
  unsigned long long c[R];
  const int32_t bits_j = have ? P.bits[j] : 0;
#pragma unroll
  for (int r = 0; r < R; r++) c[r] = have ? P.desc[(size_t)j * R + r] : 0ull;
  const int32_t t_end = min(rows, ((int32_t)blockIdx.y + 1) * PLACE_QT);
  for (int32_t t = (int32_t)blockIdx.y * PLACE_QT; t < t_end; t++) {
    const int32_t i = r0 + t;  // (uniform, inside the scans: the rows are clipped to them)
    uint32_t key = KEY_NONE;
    if (P.bits[i] > 0) {
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
      if (bits_j > 0) key = best * 64u + best_s;
    }
    if (have) P.plane[(size_t)t * P.pitch_s + j] = (uint16_t)key;
  }
}

// The window of the pair (scan i, scan j), both inside the scans and i inside the chunk whose plane starts at row r0: the sums
// of direction 0 (sigma = +1) and 1 (sigma = -1).  A frame outside the scans or without bits is absent (its key is KEY_NONE).
struct SeqWindow {
  int32_t sum[2], norm[2], frames[2];
};
__device__ __forceinline__ SeqWindow seq_window(const PlaceSeq &P, int32_t r0, int32_t i, int32_t j) {
  SeqWindow w = {{0, 0}, {0, 0}, {0, 0}};
  for (int32_t d = -P.half_window; d <= P.half_window; d++) {
    const long long a = (long long)i + d * P.step;
    if (a < 0 || a >= P.n_scans) continue;
    const int32_t bits_a = P.bits[a];
    if (bits_a <= 0) continue;
    const uint16_t *row = P.plane + (size_t)(a - r0) * P.pitch_s;
#pragma unroll
    for (int sg = 0; sg < 2; sg++) {
      const long long b = (long long)j + (sg ? -d : d) * P.step;
      if (b < 0 || b >= P.n_scans) continue;
      const uint32_t key = row[b];
      if (key == KEY_NONE) continue;
      w.sum[sg] += (int32_t)(key >> 6), w.norm[sg] += bits_a + P.bits[b], w.frames[sg]++;
    }
  }
  return w;
}
// score_sigma = (sum_sigma (2W + 1)) div frames_sigma; frames >= 1 for an admissible pair (d = 0 always counts)
__device__ __forceinline__ int32_t seq_score(const PlaceSeq &P, const SeqWindow &w, int sg) {
  return w.sum[sg] * (2 * P.half_window + 1) / w.frames[sg];
}
__device__ __forceinline__ int seq_direction(const PlaceSeq &P, const SeqWindow &w) { return seq_score(P, w, 0) <= seq_score(P, w, 1) ? 0 : 1; }

// The query entries whose scan lies in [s0, s0 + S) against every candidate entry: keys[(i - s0) * pitch + b].
__global__ __launch_bounds__(WIN_T) void place_seq_window_kernel(PlaceSeq P, int32_t s0, int32_t S, int32_t r0) {
  const int32_t b = blockIdx.x * WIN_T + threadIdx.x;
  const bool have = b < P.n_ids;
  int32_t j = have ? P.ids[b] : -1;
  if (!id_in(j, P.n_scans)) j = -1;  // (reported by the top-K kernel, where the entry is a query)
  const int32_t bits_j = j >= 0 ? P.bits[j] : 0;
  const bool past_only = P.flags & NHIP_PLACE_PAST_ONLY;
  unsigned long long n_before = 0, n_after = 0, n_reverse = 0, n_short = 0;  // (per wave: every lane holds the wave's count)
  const int32_t a_end = min(P.n_ids, ((int32_t)blockIdx.y + 1) * WIN_QT);
  for (int32_t a = (int32_t)blockIdx.y * WIN_QT; a < a_end; a++) {
    const int32_t i = P.ids[a];  // (uniform)
    if ((long long)i < s0 || (long long)i >= (long long)s0 + S) continue;  // (another chunk's query, or no scan at all)
    const int32_t bits_i = P.bits[i];
    const long long sep = (long long)i - j;
    const bool adm = j >= 0 && (sep < 0 ? -sep : sep) > P.min_separation && (!past_only || j < i) && bits_i > 0 && bits_j > 0;
    uint32_t key = KEY_NONE;
    const unsigned long long any = __ballot(adm);
    if (any) {
      n_before += (unsigned long long)__popcll(any);
      bool kept = false, reverse = false, cut = false;
      if (adm) {
        const SeqWindow w = seq_window(P, r0, i, j);
        const int dir = seq_direction(P, w);
        kept = 1000ll * w.sum[dir] <= (long long)P.max_permille * w.norm[dir];
        reverse = kept && dir == 1, cut = kept && w.frames[dir] < 2 * P.half_window + 1;
        if (kept) key = (uint32_t)seq_score(P, w, dir);
      }
      n_after += (unsigned long long)__popcll(__ballot(kept));
      n_reverse += (unsigned long long)__popcll(__ballot(reverse));
      n_short += (unsigned long long)__popcll(__ballot(cut));
    }
    if (have) P.keys[(size_t)(i - s0) * P.pitch + b] = (uint16_t)key;
  }
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
    if (n_before) atomicAdd(stats + 1, n_before);
    if (n_after) atomicAdd(stats + 2, n_after);
    if (n_reverse) atomicAdd(stats + 6, n_reverse);
    if (n_short) atomicAdd(stats + 7, n_short);
  }
}

__global__ __launch_bounds__(256) void place_seq_topk_kernel(PlaceSeq P, int32_t s0, int32_t S, int32_t r0) {
  const int lane = threadIdx.x & 63;
  const int32_t a = blockIdx.x * 4 + (threadIdx.x >> 6);  // (uniform per wave)
  if (a >= P.n_ids) return;
  unsigned long long *stats = reinterpret_cast<unsigned long long *>(P.stats);
  int32_t *rec = P.records + (size_t)a * P.top_k * 8;
  const int32_t i = P.ids[a];
  if (!id_in(i, P.n_scans)) {  // no scan: no record, reported; the first chunk answers for it
    if (s0 != 0) return;
    if (lane < P.top_k)
      for (int f = 0; f < 8; f++) rec[8 * lane + f] = -1;
    if (lane == 0) {
      flag_bad_id(P.status, BAD_PLACE_ID, i, a);
      if (a == 0) atomicAdd(stats + 0, (unsigned long long)P.n_ids);
      atomicAdd(stats + 4, 1ull);
      atomicAdd(stats + 5, 1ull);
    }
    return;
  }
  if (i < s0 || (long long)i >= (long long)s0 + S) return;
  const uint16_t *row = P.keys + (size_t)(i - s0) * P.pitch;
  constexpr unsigned long long NONE = ~0ull;
  unsigned long long last = 0, mine = NONE;  // (composites are (seq << 32 | b) + 1: 0 is below them all)
  int32_t written = 0;
  for (int32_t k = 0; k < P.top_k; k++) {
    unsigned long long m = NONE;
    if (last != NONE)
      for (int32_t b = lane; b < P.n_ids; b += 64) {
        const uint32_t key = row[b];
        if (key == KEY_NONE) continue;
        const unsigned long long comp = (((unsigned long long)key << 32) | (uint32_t)b) + 1ull;
        if (comp > last && comp < m) m = comp;
      }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(m, d, 64);
      m = o < m ? o : m;
    }
    last = m;
    if (lane == k) mine = m;
    written += m != NONE;
  }
  if (lane < P.top_k) {  // lane k writes record k
    int32_t v[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    if (mine != NONE) {
      const int32_t b = (int32_t)(uint32_t)(mine - 1ull);
      const int32_t j = P.ids[b];  // (inside the scans: its key is not KEY_NONE)
      const uint32_t centre = P.plane[(size_t)(i - r0) * P.pitch_s + j];
      const SeqWindow w = seq_window(P, r0, i, j);
      const int dir = seq_direction(P, w);
      v[0] = j, v[1] = (int32_t)(centre & 63u), v[2] = (int32_t)(centre >> 6), v[3] = P.bits[j];
      v[4] = seq_score(P, w, dir), v[5] = w.sum[dir], v[6] = w.frames[dir], v[7] = dir;
    }
#pragma unroll
    for (int f = 0; f < 8; f++) rec[8 * lane + f] = v[f];
  }
  if (lane == 0) {
    if (a == 0) atomicAdd(stats + 0, (unsigned long long)P.n_ids);
    if (written) atomicAdd(stats + 3, (unsigned long long)written);
    if (!written) atomicAdd(stats + 4, 1ull);
    if (P.bits[i] == 0) atomicAdd(stats + 5, 1ull);
  }
}

template <int R>
void launch_plane(const PlaceSeq &P, int32_t r0, int32_t rows, hipStream_t s) {
  const dim3 grid((uint32_t)((P.n_scans + DIST_T - 1) / DIST_T), (uint32_t)((rows + PLACE_QT - 1) / PLACE_QT));
  hipLaunchKernelGGL(place_seq_plane_kernel<R>, grid, dim3(DIST_T), 0, s, P, r0, rows);
}

}  // namespace

int launch_place_seq_match(const PlaceSeq &P, int32_t chunk_scans, hipStream_t s) {
  NHIP_TRY_HIP(hipMemsetAsync(P.stats, 0, 8 * sizeof(long long), s));
  if (P.n_ids <= 0) return NHIP_OK;
  const long long halo = (long long)P.half_window * P.step;
  int32_t s0 = 0;
  do {  // (once even without scans: every entry of the list is then reported by the first chunk)
    const int32_t S = P.n_scans - s0 < chunk_scans ? P.n_scans - s0 : chunk_scans;
    const int32_t r0 = (int32_t)(s0 - halo > 0 ? s0 - halo : 0);
    const int32_t r1 = (int32_t)((long long)s0 + S + halo < P.n_scans ? (long long)s0 + S + halo : P.n_scans);
    if (r1 > r0) {
      switch (P.n_rings) {
#define NHIP_PLACE_CASE(R) \
  case R: launch_plane<R>(P, r0, r1 - r0, s); break;
        NHIP_PLACE_CASE(1) NHIP_PLACE_CASE(2) NHIP_PLACE_CASE(3) NHIP_PLACE_CASE(4) NHIP_PLACE_CASE(5)
        NHIP_PLACE_CASE(6) NHIP_PLACE_CASE(7) NHIP_PLACE_CASE(8) NHIP_PLACE_CASE(9) NHIP_PLACE_CASE(10)
        NHIP_PLACE_CASE(11) NHIP_PLACE_CASE(12) NHIP_PLACE_CASE(13) NHIP_PLACE_CASE(14) NHIP_PLACE_CASE(15)
#undef NHIP_PLACE_CASE
        default: set_error("place_seq_match: n_rings %d outside 1..%d", P.n_rings, PLACE_MATCH_MAX_RINGS); return NHIP_ERR_ARG;
      }
      const dim3 grid((uint32_t)((P.n_ids + WIN_T - 1) / WIN_T), (uint32_t)((P.n_ids + WIN_QT - 1) / WIN_QT));
      hipLaunchKernelGGL(place_seq_window_kernel, grid, dim3(WIN_T), 0, s, P, s0, S, r0);
    }
    hipLaunchKernelGGL(place_seq_topk_kernel, dim3((uint32_t)((P.n_ids + 3) / 4)), dim3(256), 0, s, P, s0, S, r0);
    s0 += S;
  } while (s0 < P.n_scans);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
