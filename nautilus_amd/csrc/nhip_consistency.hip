// nhip_consistency.hip -- K17: loop-closure consistency.  The records of loop closure are judged against EACH OTHER: two records
// are consistent if the cycle they form with the odometry between their ends closes up to the drift that odometry can have
// gathered (pairwise consistency maximisation: Mangelson et al., ICRA 2018), and a large set of mutually consistent records is
// grown greedily.  The spec is DESIGN.md section 3, "Loop-closure consistency"; tests/consistency_reference.py restates it in
// numpy.  The pair test is fp64 + - x and comparisons, every operation rounded on its own in the spec's order (no
// transcendental: the host prepared the records); the set is integers, whose order-free operations give the reference's bits.
//
//   consistency_adjacency_kernel  place_dist_kernel's shape: a lane holds one COLUMN record, 8 doubles in VGPRs, a wave one
//                                 64-column word; it walks ADJ_ROWS rows whose 8 doubles are wave-uniform (scalar loads).  The
//                                 test orders a pair (lo, hi) by index, so the matrix is symmetric by construction; a wave
//                                 wholly on one side of the diagonal knows the order without a select.  One __ballot per (row,
//                                 word), one plain vector store of the word by lane 0, the word's popcount added to deg[row].
//   consistency_begin_kernel      one workgroup: the live set C = all M records, the step state cleared, the stats' first words.
//   consistency_score_kernel      a wave per row u of C (C staged in LDS: W <= 1024 words): popcount(A[u] & C) summed over the
//                                 wave, key = score << 32 | ~u by 64-bit atomicMax to one word of device memory: the largest
//                                 score, the smallest index among equals.  In the first step C is everything and the score is
//                                 the caller's deg[u].  Workgroups none of whose rows is in C leave before the staging.
//   consistency_commit_kernel     one workgroup: reads the key, appends u, C &= A[u], clears the key, counts the live bits and
//                                 sets `done` when C is empty or the step cap is reached.
// Two launches per step, as in the PCG; both return at once when `done` is set, so the host enqueues steps in batches and
// reads `done` between them.  No grid-wide synchronisation and no waiting on a device word anywhere.
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int ADJ_T = 256;      // 4 waves: 4 words of a row
constexpr int ADJ_ROWS = 32;    // rows a workgroup walks with one load of its columns
constexpr int SET_T = 256;
constexpr int SCORE_ROWS = 16;  // rows per workgroup of the score kernel, 4 per wave; 16 divides 64: they share ONE word of C

struct Rec {
  double cw, sw, xw, yw, px, py, la, lb;
};

__device__ __forceinline__ Rec load_rec(const double *__restrict__ p) { return Rec{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}; }

// the spec's pair test, a = the record of the smaller index; a NaN anywhere fails a comparison
__device__ __forceinline__ bool pair_consistent(const Rec &a, const Rec &b, const ConsistencyTol &T) {
  const double ihx = -__dadd_rn(__dmul_rn(b.cw, b.xw), __dmul_rn(b.sw, b.yw));  // W_hi^-1
  const double ihy = __dsub_rn(__dmul_rn(b.sw, b.xw), __dmul_rn(b.cw, b.yw));
  const double cq = __dadd_rn(__dmul_rn(a.cw, b.cw), __dmul_rn(a.sw, b.sw));    // Q = W_lo o W_hi^-1
  const double sq = __dsub_rn(__dmul_rn(a.sw, b.cw), __dmul_rn(a.cw, b.sw));
  const double qx = __dadd_rn(__dsub_rn(__dmul_rn(a.cw, ihx), __dmul_rn(a.sw, ihy)), a.xw);
  const double qy = __dadd_rn(__dadd_rn(__dmul_rn(a.sw, ihx), __dmul_rn(a.cw, ihy)), a.yw);
  const double ex = __dsub_rn(__dadd_rn(__dsub_rn(__dmul_rn(cq, a.px), __dmul_rn(sq, a.py)), qx), a.px);
  const double ey = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(sq, a.px), __dmul_rn(cq, a.py)), qy), a.py);
  const double e2 = __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey));
  const double chord = __dsub_rn(2.0, __dmul_rn(2.0, cq));
  const double len = __dadd_rn(fabs(__dsub_rn(a.la, b.la)), fabs(__dsub_rn(a.lb, b.lb)));
  double tt = __dadd_rn(T.t0, __dmul_rn(T.t_rate, len)), tr = __dadd_rn(T.r0, __dmul_rn(T.r_rate, len));
  tt = T.t_max < tt ? T.t_max : tt;  // (the spec's min: a NaN sum stays)
  tr = T.r_max < tr ? T.r_max : tr;
  return e2 <= __dmul_rn(tt, tt) && chord <= __dmul_rn(tr, tr);
}

__global__ __launch_bounds__(ADJ_T) void consistency_adjacency_kernel(const double *__restrict__ rec, int32_t M, int32_t W,
                                                                      ConsistencyTol T, unsigned long long *__restrict__ adj,
                                                                      int32_t *__restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int32_t w = __builtin_amdgcn_readfirstlane((int32_t)(blockIdx.x * (ADJ_T / 64) + (threadIdx.x >> 6)));
  if (w >= W) return;
  const int32_t col = w * 64 + lane;
  const bool have = col < M;  // (columns >= M vote 0)
  Rec c{0, 0, 0, 0, 0, 0, 0, 0};
  if (have) c = load_rec(rec + 8 * (size_t)col);
  const int32_t r0 = (int32_t)blockIdx.y * ADJ_ROWS, r1 = min(r0 + ADJ_ROWS, M);
  for (int32_t row = r0; row < r1; row++) {
    const Rec r = load_rec(rec + 8 * (size_t)row);  // (wave-uniform)
    bool ok;
    if (row < w * 64)
      ok = pair_consistent(r, c, T);
    else if (row >= w * 64 + 64)
      ok = pair_consistent(c, r, T);
    else  // the word that holds the diagonal
      ok = row != col && (row < col ? pair_consistent(r, c, T) : pair_consistent(c, r, T));
    const unsigned long long word = __ballot(ok && have);
    if (lane == 0) {
      adj[(size_t)row * W + w] = word;
      if (word) atomicAdd(deg + row, (int32_t)__popcll(word));
    }
  }
}

__device__ __forceinline__ long long block_sum(long long v, long long *part) {  // of SET_T threads; every thread gets the sum
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();  // (part may still be read from the call before)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

// a degree outside [0, M) is counted as 0 (and reported)
__device__ __forceinline__ int32_t checked_degree(const int32_t *deg, int32_t u, int32_t M, uint32_t *status) {
  const int32_t d = deg[u];
  if (id_in(d, M)) return d;
  flag_bad_id(status, BAD_CONSISTENCY_DEGREE, d, u);
  return 0;
}

// stats = {M, edges, largest degree, 0, 0, 0, 0, 0} from the degrees; one workgroup
__device__ __forceinline__ void degree_stats(const int32_t *deg, int32_t M, long long *stats, uint32_t *status, long long *part,
                                             int32_t *part_max) {
  long long sum = 0;
  int32_t mx = 0;
  for (int32_t u = threadIdx.x; u < M; u += SET_T) {
    const int32_t d = checked_degree(deg, u, M, status);
    sum += d, mx = d > mx ? d : mx;
  }
  sum = block_sum(sum, part);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int32_t o = __shfl_xor(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0) part_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < SET_T / 64; k++) mx = part_max[k] > mx ? part_max[k] : mx;
    stats[0] = M, stats[1] = sum / 2, stats[2] = mx;
    for (int k = 3; k < 8; k++) stats[k] = 0;
  }
}

__global__ __launch_bounds__(SET_T) void consistency_stats_kernel(const int32_t *deg, int32_t M, long long *stats, uint32_t *status) {
  __shared__ long long part[SET_T / 64];
  __shared__ int32_t part_max[SET_T / 64];
  degree_stats(deg, M, stats, status, part, part_max);
}

__global__ __launch_bounds__(SET_T) void consistency_begin_kernel(ConsistencySet P) {
  __shared__ long long part[SET_T / 64];
  __shared__ int32_t part_max[SET_T / 64];
  for (int32_t i = threadIdx.x; i < P.W; i += SET_T)
    P.C[i] = (i == P.W - 1 && (P.M & 63)) ? (1ull << (P.M & 63)) - 1ull : ~0ull;  // (nothing beyond M is ever live)
  degree_stats(P.deg, P.M, P.stats, P.status, part, part_max);
  if (threadIdx.x == 0) {
    P.st->key = 0ull, P.st->steps = 0, P.st->done = P.M == 0;
    *P.n_members = 0;
  }
}

__global__ __launch_bounds__(SET_T) void consistency_score_kernel(ConsistencySet P) {
  __shared__ unsigned long long c_lds[CONSISTENCY_MAX_RECORDS / 64];
  if (P.st->done) return;
  const int32_t u0 = (int32_t)blockIdx.x * SCORE_ROWS;  // (< M by the grid, so its word is one of the W)
  const unsigned long long mine = (P.C[u0 >> 6] >> (u0 & 63)) & ((1ull << SCORE_ROWS) - 1ull);
  if (!mine) return;  // (rows outside C leave at once: the same word for the whole workgroup)
  const bool first = P.st->steps == 0;
  if (!first) {
    for (int32_t i = threadIdx.x; i < P.W; i += SET_T) c_lds[i] = P.C[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < SCORE_ROWS / 4; k++) {
    const int32_t local = wave * (SCORE_ROWS / 4) + k, u = u0 + local;
    if (u >= P.M || !((mine >> local) & 1ull)) continue;  // (uniform per wave)
    uint32_t n = 0;
    if (first) {
      n = (uint32_t)checked_degree(P.deg, u, P.M, lane == 0 ? P.status : nullptr);
    } else {
      const unsigned long long *row = P.adj + (size_t)u * P.W;
      for (int32_t i = lane; i < P.W; i += 64) n += (uint32_t)__popcll(row[i] & c_lds[i]);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    }
    if (lane == 0) atomicMax(&P.st->key, ((unsigned long long)n << 32) | (unsigned long long)(~(uint32_t)u));
  }
}

__global__ __launch_bounds__(SET_T) void consistency_commit_kernel(ConsistencySet P) {
  __shared__ long long part[SET_T / 64];
  ConsistencyState *st = P.st;
  if (st->done) return;
  const unsigned long long key = st->key;
  const int32_t steps = st->steps;
  const int32_t u = (int32_t)(~(uint32_t)key);
  if (!id_in(u, P.M) || !id_in(steps, P.M)) {  // (no row voted, or the state was overwritten between two launches: the set ends)
    if (threadIdx.x == 0) {
      flag_bad_id(P.status, BAD_CONSISTENCY_MEMBER, u, steps);
      st->done = 1;
      *P.n_members = id_in(steps, P.M) ? steps : 0;
      P.stats[3] = *P.n_members, P.stats[4] = 0;
    }
    return;
  }
  const unsigned long long *row = P.adj + (size_t)u * P.W;
  long long live = 0;
  for (int32_t i = threadIdx.x; i < P.W; i += SET_T) {
    unsigned long long c = P.C[i] & row[i];
    if (i == (u >> 6)) c &= ~(1ull << (u & 63));  // (the diagonal is 0: a member never stays live, whatever the caller's matrix holds)
    P.C[i] = c;
    live += __popcll(c);
  }
  live = block_sum(live, part);  // (its barriers also order every thread's read of the key before the clear below)
  if (threadIdx.x == 0) {
    P.members[steps] = u;
    st->steps = steps + 1;
    st->key = 0ull;
    if (live == 0 || steps + 1 >= P.max_steps) {
      st->done = 1;
      *P.n_members = steps + 1;
      P.stats[3] = steps + 1, P.stats[4] = live != 0;
    }
  }
}

}  // namespace

int launch_consistency_adjacency(const double *d_records, int32_t M, const ConsistencyTol &T, unsigned long long *d_adj, int32_t *d_deg,
                                 long long *d_stats, hipStream_t s) {
  const int32_t W = (M + 63) / 64;
  if (M > 0) {
    NHIP_TRY_HIP(hipMemsetAsync(d_deg, 0, sizeof(int32_t) * (size_t)M, s));
    const dim3 grid((uint32_t)((W + ADJ_T / 64 - 1) / (ADJ_T / 64)), (uint32_t)((M + ADJ_ROWS - 1) / ADJ_ROWS));
    hipLaunchKernelGGL(consistency_adjacency_kernel, grid, dim3(ADJ_T), 0, s, d_records, M, W, T, d_adj, d_deg);
  }
  hipLaunchKernelGGL(consistency_stats_kernel, dim3(1), dim3(SET_T), 0, s, d_deg, M, d_stats, dev_status());
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_consistency_begin(const ConsistencySet &P, hipStream_t s) {
  if (P.M > 0) NHIP_TRY_HIP(hipMemsetAsync(P.members, 0xFF, sizeof(int32_t) * (size_t)P.M, s));
  hipLaunchKernelGGL(consistency_begin_kernel, dim3(1), dim3(SET_T), 0, s, P);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_consistency_steps(const ConsistencySet &P, int32_t n, hipStream_t s) {
  if (P.M <= 0) return NHIP_OK;
  const dim3 grid((uint32_t)((P.M + SCORE_ROWS - 1) / SCORE_ROWS));
  for (int32_t k = 0; k < n; k++) {
    hipLaunchKernelGGL(consistency_score_kernel, grid, dim3(SET_T), 0, s, P);
    hipLaunchKernelGGL(consistency_commit_kernel, dim3(1), dim3(SET_T), 0, s, P);
  }
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
