// nhip_csm_score.hip -- from the matcher's keys to its records: csm_finalize_kernel decodes a search's keys, computes the
// quantised score and applies the score gate; csm_exact_score_kernel (NHIP_SEARCH_EXACT_SCORE) replaces the score of the
// pose that won by its score on the unquantised table.
#include "nhip_csm_shared.h"

namespace nhip {

namespace {

using namespace csm;

__global__ void csm_finalize_kernel(const unsigned long long *__restrict__ keys,
                                    const int32_t *__restrict__ pair_src,
                                    const int32_t *__restrict__ offsets, int32_t n_scans, int32_t n_pairs,
                                    int32_t nx, int32_t ny, ScoreGate gate, bool score_later,
                                    nhip_match_t *__restrict__ out, int32_t *__restrict__ sums) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  const unsigned long long key = keys[i];
  const uint32_t sum = (uint32_t)(key >> 32);
  const int32_t src = pair_src[i];
  const int32_t n = id_in(src, n_scans) ? offsets[src + 1] - offsets[src] : 0;  // (an id out of range: the matcher reported it)
  nhip_match_t m;
  decode_key(key, nx, ny, m);
  double sc = gate.Lf;
  if (n > 0) sc = __dadd_rn(gate.Lf, __ddiv_rn(__dmul_rn(gate.step, (double)sum), (double)n));
  m.score = __double2float_rn(sc);
  // (score_later: NHIP_SEARCH_EXACT_SCORE replaces the score and gates it; here only the floor on the sum)
  const bool rejected = gate_rejects(gate, sum, n, score_later ? INFINITY : m.score);
  out[i] = rejected ? gate_rejected_record() : m;
  if (sums) sums[i] = rejected ? -1 : (int32_t)sum;
}

// ---- NHIP_SEARCH_EXACT_SCORE: the winning pose's score on the UNQUANTISED table -----------------------------------------
// The argmax is found on quantised cells (bit-exact against the oracle; on 1,300 pairs of the bench workload it is also the
// argmax of a double table every time).  The score reported with it, Lf + step * sum / N, carries the cells' rounding: up
// to 2.3e-5 relative at the best-matching pairs of that sample, where |score| is smallest -- outside the north star's
// 1e-5.  This pass recomputes the score of the ONE pose that won the way the reference's table type would give it
// (CImg<double>, cimg_debug.h:19): for each of the scan's points the exact integer blur sum V of the cell it reads --
// from the hit raster the table was blurred from (13 x 13 bits around the cell at sigma = 2) --, ln(max(V / K^2, floor))
// in double, the mean over the points in double: 1081 x 13 dword pairs of a 200 KB raster per pair.
struct ExactParams {
  const float2 *xy;
  const int32_t *offsets;
  const uint8_t *grids;
  const int32_t *pair_src, *pair_slot;
  const double *rot0_cs, *delta_cs;
  const int32_t *pair_origin;
  const int32_t *pair_kbase;  // optional: entry of delta_cs that is pair i's rotation 0 (nhip_bnb_params.h)
  nhip_match_t *out;
  const unsigned long long *keys;  // optional: the search's keys, decoded here (the record's indices, the sum) instead of by csm_finalize_kernel
  int32_t *sums;                   // where the integer sums go (may be null): all of them with keys, else -1 of a rejected record
  ScoreGate gate;                  // the caller's min_score: a pair that fails it gets the rejected record
  IdBounds ids;
  int32_t n_pairs, pairs_per_xcd, nx, ny, hx, hy, S, R, hits_pitch, max_shift;
  int64_t slot_bytes, hits_offset;
  double res, inv_res, K2, floor_p, Lf;
  int32_t taps[2 * 16 + 1];
};

// One 256-thread workgroup per pair; a thread takes the points tid, tid + 256, ... (five at most on a 1081-beam scan).  The
// first version ran one wave per pair with a rolled loop over the window's rows: 17 points x 13 dependent round trips per
// lane, 0.44 ms per 10,000 pairs of pure latency.  Here the 2 NR dword loads of a point's window are issued together
// (NR = 2 R + 1 rows, a compile-time constant for the blur radii in use; the generic instantiation loops).
constexpr int EX_THREADS = 256;  // (512 -- three rounds of loads per thread instead of five -- measured slower: 0.140 against 0.131 ms)
template <int NR>
__global__ __launch_bounds__(EX_THREADS) void csm_exact_score_kernel(ExactParams P) {
  __shared__ double s_part[EX_THREADS / 64];
  __shared__ uint32_t s_taps[2 * 16 + 1];  // (indexed by a set bit's position: from LDS, not from the kernel's argument block)
  // Row sums by table: a window row of up to 14 bits is two 7-bit halves, s_lut[h][bits] = sum of the taps of the set
  // bits of half h -- two LDS reads per row, where the loop over set bits ran as long as the wave's fullest lane needed
  // (the pass was 420 vector instructions per point, most of them that loop: 0.145 -> 0.131 ms per 10,000 pairs).
  __shared__ uint32_t s_lut[2][128];
  if (threadIdx.x <= 2 * 16) s_taps[threadIdx.x] = (uint32_t)P.taps[threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 256) {
    const int h = threadIdx.x >> 7, b = threadIdx.x & 127;
    uint32_t t = 0u;
#pragma unroll
    for (int i = 0; i < 7; i++)
      if ((b >> i) & 1) t += s_taps[7 * h + i];  // (entries past 2 R are zero)
    s_lut[h][b] = t;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // consecutive pairs (one target's, usually) on ONE XCD, as in the matcher's kernels: its L2 then fetches the target's hit
  // raster once -- with pair = blockIdx the eight XCDs each fetched it (536 MB of L2 misses per 10,000 pairs for 200 MB
  // of rasters: the pass was bound by them)
  const int32_t pair = (int32_t)(blockIdx.x & 7u) * P.pairs_per_xcd + (int32_t)(blockIdx.x >> 3);
  if (pair >= P.n_pairs) return;
  int32_t src = P.pair_src[pair], slot = P.pair_slot[pair];
  const bool ids_ok = pair_ids_ok(P.ids, src, slot, pair, false);  // (the matcher reported it)
  if (!ids_ok) src = slot = 0;
  const int32_t beg = ids_ok ? P.offsets[src] : 0, n_pts = ids_ok ? P.offsets[src + 1] - beg : 0;
  nhip_match_t m;
  if (P.keys) {  // (as csm_finalize_kernel decodes them; the quantised-formula score it would store is what this pass replaces)
    const unsigned long long key = P.keys[pair];
    const int32_t ny = P.ny, nx = P.nx;  // (read in this order: the kernel's code is then what it was with the decoding written out)
    decode_key(key, nx, ny, m);
    m.score = (float)P.Lf;
    if (gate_rejects(P.gate, (uint32_t)(key >> 32), n_pts, INFINITY)) m = gate_rejected_record();  // (below the floor)
    if (threadIdx.x == 0) {
      P.out[pair] = m;
      if (P.sums) P.sums[pair] = m.itheta < 0 ? -1 : (int32_t)(uint32_t)(key >> 32);
    }
  } else {
    m = P.out[pair];
  }
  if (m.itheta < 0) return;  // rejected by its sum already: no raster to read
  {
    // a search centre the stored border cannot cover "scores nothing" in every matcher kernel (sum 0, pose 0, score Lf):
    // the record keeps that score -- the real score at pose 0 would contradict the sum beside it
    const int32_t ox = P.pair_origin ? P.pair_origin[2 * pair] : 0, oy = P.pair_origin ? P.pair_origin[2 * pair + 1] : 0;
    if (abs(ox) + P.hx > P.max_shift || abs(oy) + P.hy > P.max_shift) {
      if (threadIdx.x == 0 && gate_rejects(P.gate, 0u, 0, (float)P.Lf)) {
        P.out[pair] = gate_rejected_record();
        if (P.sums) P.sums[pair] = -1;
      }
      return;
    }
  }
  const int32_t cx = (P.pair_origin ? P.pair_origin[2 * pair] : 0) + m.ix - P.hx;
  const int32_t cy = (P.pair_origin ? P.pair_origin[2 * pair + 1] : 0) + m.iy - P.hy;
  // rotation itheta: R(theta0) * R(delta_k), composed in double with individually rounded ops, as every matcher kernel
  // (csm::compose_rotation, written out: as a call the kernel compiles to other code -- docs/history.md, appendix G)
  const double c0 = P.rot0_cs[2 * pair], s0 = P.rot0_cs[2 * pair + 1];
  const int32_t kd = m.itheta + (P.pair_kbase ? P.pair_kbase[pair] : 0);
  const double cd = P.delta_cs[2 * kd], sd = P.delta_cs[2 * kd + 1];
  const float cf = __double2float_rn(__dsub_rn(__dmul_rn(c0, cd), __dmul_rn(s0, sd)));
  const float sf = __double2float_rn(__dadd_rn(__dmul_rn(s0, cd), __dmul_rn(c0, sd)));
  const uint8_t *hits = P.grids + (size_t)slot * P.slot_bytes + P.hits_offset;
  const int nr = NR > 0 ? NR : 2 * P.R + 1;
  const uint32_t mask = (1u << nr) - 1u;  // (R <= 15: at most 31 bits)
  double acc = 0.0;
  for (int32_t p = (int32_t)threadIdx.x; p < n_pts; p += EX_THREADS) {
    const float2 q = P.xy[beg + p];
    const float xr = __fsub_rn(__fmul_rn(cf, q.x), __fmul_rn(sf, q.y));
    const float yr = __fadd_rn(__fmul_rn(sf, q.x), __fmul_rn(cf, q.y));
    double L = P.Lf;  // non-finite points and lookups outside the grid contribute the floor
    if ((fabsf(xr) < 1e9f) && (fabsf(yr) < 1e9f)) {
      const double fc = floor_quotient((double)xr, P.res, P.inv_res) + (double)(P.S / 2 + cx);
      const double fr = floor_quotient((double)yr, P.res, P.inv_res) + (double)(P.S / 2 + cy);
      if (fc >= 0.0 && fc < (double)P.S && fr >= 0.0 && fr < (double)P.S) {
        const int32_t col = (int32_t)fc, row = (int32_t)fr;
        const uint32_t bit0 = (uint32_t)(col - P.R + HIT_PAD), sh = bit0 & 31u;  // first bit of the row windows
        const uint8_t *w = hits + (size_t)(row - P.R + HIT_PAD) * P.hits_pitch + 4 * (size_t)(bit0 >> 5);
        uint32_t V = 0u;
        if (NR > 0) {
          // (a row's 64-bit window in ONE load from its 4-byte-aligned address: the pass is bound by its load instructions)
          struct __attribute__((packed, aligned(4))) Win { uint32_t lo, hi; };
          Win win[NR > 0 ? NR : 1];
#pragma unroll
          for (int i = 0; i < NR; i++) win[i] = *reinterpret_cast<const Win *>(w + (size_t)i * P.hits_pitch);
#pragma unroll
          for (int i = 0; i < NR; i++) {
            uint32_t bits = (uint32_t)((((unsigned long long)win[i].hi << 32) | win[i].lo) >> sh) & mask;
            uint32_t rowsum = 0u;
            if (NR <= 14) {
              rowsum = s_lut[0][bits & 127u] + s_lut[1][bits >> 7];
            } else {
              while (bits) {
                rowsum += s_taps[__builtin_ctz(bits)];
                bits &= bits - 1u;
              }
            }
            V += s_taps[i] * rowsum;
          }
        } else {
          for (int i = 0; i < nr; i++) {
            const uint32_t lo = *reinterpret_cast<const uint32_t *>(w + (size_t)i * P.hits_pitch);
            const uint32_t hi = *reinterpret_cast<const uint32_t *>(w + (size_t)i * P.hits_pitch + 4);
            uint32_t bits = (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh) & mask;
            uint32_t rowsum = 0u;
            while (bits) {
              rowsum += s_taps[__builtin_ctz(bits)];
              bits &= bits - 1u;
            }
            V += s_taps[i] * rowsum;
          }
        }
        double v = __ddiv_rn((double)V, P.K2);
        if (v < P.floor_p) v = P.floor_p;
        L = log(v);
      }
    }
    acc += L;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = shfl_xor_u64(__double_as_longlong(acc), s);
    acc += __longlong_as_double((long long)o);
  }
  if (lane == 0) s_part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = s_part[0];
#pragma unroll
    for (int w = 1; w < EX_THREADS / 64; w++) tot += s_part[w];
    const float score = __double2float_rn(n_pts > 0 ? __ddiv_rn(tot, (double)n_pts) : P.Lf);
    if (gate_rejects(P.gate, 0u, 0, score)) {  // (the sum passed the floor; the exact score decides)
      P.out[pair] = gate_rejected_record();
      if (P.sums) P.sums[pair] = -1;
    } else {
      P.out[pair].score = score;
    }
  }
}

}  // namespace

int launch_csm_exact_score(const MatchJob &job, const MatchPlan &plan) {
  const nhip_grid_spec_t *spec = job.spec;
  const GridLayout &L = *job.L;
  const hipStream_t s = job.stream;
  NHIP_REQUIRE(L.R <= 15, "exact score: blur radius %d > 15", L.R);
  GridTables T;
  int rc = make_tables(spec, L, &T);
  if (rc) return rc;
  ExactParams P;
  fill_job_common(P, job);
  P.pair_kbase = job.pair_kbase;
  P.out = job.out;
  if (plan.keys_undecoded) P.keys = reinterpret_cast<const unsigned long long *>(job.keys);
  P.sums = job.sums;
  P.pairs_per_xcd = (job.n_pairs + 7) / 8;
  P.R = L.R;
  P.hits_pitch = L.hits_pitch;
  P.hits_offset = L.hits_offset;
  P.K2 = (double)L.K * (double)L.K;
  P.floor_p = spec->floor_p;
  P.Lf = L.Lf;
  P.gate = job_gate(job);
  for (int i = 0; i <= 2 * L.R; i++) P.taps[i] = T.taps[i];
  timer_begin(NHIP_TIMER_EXACT_SCORE, s);
  if (L.R == 6) hipLaunchKernelGGL(csm_exact_score_kernel<13>, dim3(8u * (uint32_t)P.pairs_per_xcd), dim3(EX_THREADS), 0, s, P);  // sigma = 2
  else if (L.R == 3) hipLaunchKernelGGL(csm_exact_score_kernel<7>, dim3(8u * (uint32_t)P.pairs_per_xcd), dim3(EX_THREADS), 0, s, P);  // sigma = 1
  else hipLaunchKernelGGL(csm_exact_score_kernel<0>, dim3(8u * (uint32_t)P.pairs_per_xcd), dim3(EX_THREADS), 0, s, P);
  timer_end(NHIP_TIMER_EXACT_SCORE, s);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

void launch_csm_finalize(const MatchJob &job) {
  hipLaunchKernelGGL(csm_finalize_kernel, dim3((job.n_pairs + 255) / 256), dim3(256), 0, job.stream,
                     reinterpret_cast<const unsigned long long *>(job.keys), job.pair_src, job.offsets, job.ids.n_scans, job.n_pairs,
                     job.search->nx, job.search->ny, job_gate(job), (job.search->flags & NHIP_SEARCH_EXACT_SCORE) != 0, job.out,
                     job.sums);
}

}  // namespace nhip
