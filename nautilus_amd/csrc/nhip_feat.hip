// nhip_feat.hip -- the planar and edge features of every scan: what Solver::SolveSLAM's FEATURE mode builds its residual
// blocks from (src/optimization/solver.cc:297-318; FeatureExtractor, src/input/feature_extracter.cc:15-165, constructed
// at src/util/slam_types.h:66-69).  The spec is DESIGN.md section 3, "Scan features".
//
//   feat_extract_kernel   one scan per workgroup, lanes are points.  Phase 1: the smoothness score of every point from its
//                         <= 2 P - 1 index neighbours (GetNeighborhood + ComputeSmoothnessScores), the arithmetic of
//                         lc_scatter_score_kernel (nhip_lc.hip) on the neighbourhood in the reference's order.  Phase 2: the
//                         two greedy walks over the sorted scores (GetPlanarPoints / GetEdgePoints) WITHOUT a sort: a walk
//                         accepts the extreme (score, index) key among the points that pass the threshold and lie outside
//                         the distance threshold of everything accepted so far -- so each acceptance is one workgroup
//                         argmin, and the walk's distance rejections are one suppression pass over the points.  The pass
//                         of round r and the argmin scan of round r + 1 are one loop; planar and edge run side by side: at
//                         most max(max_planar, max_edge) + 1 rounds of one barrier each.
//   feat_offsets_kernel   exclusive scan of the per-scan feature counts (after checking them, and every index, against
//   feat_pack_kernel      the scan they name) and the gather of the selected points' xy / normals into packed clouds:
//                         the arena layout nhip_corr_search_dev takes.
//
// A thread owns the points tid, tid + 256, ...: a point's score and suppression flags are read and written by its owner
// alone, only the accepted points' coordinates are shared.  Scans of up to FEAT_LDS_N points keep coordinates, scores and
// flags in LDS; a longer scan keeps nothing per point: its lanes read the cloud from global memory (L2), compute a
// point's score again in every round in which the point is still eligible, and derive its flags from the accepted
// points, which LDS holds (<= 64 per set).  Same functions, same rounding, any length.
#include "nhip_common.h"

namespace nhip {

namespace {

constexpr int FT = 256;            // threads of a workgroup
constexpr int FEAT_LDS_N = 2048;   // points of a scan that LDS holds (16 KB coordinates + 16 KB scores + 2 KB flags)
constexpr int FEAT_MAX_CAP = 64;   // the largest max_planar / max_edge (and neighbors_per_side: the left mask is 64 bits)

__device__ __forceinline__ double feat_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// (a - b).norm() as Eigen evaluates it for Vector2f: every float operation rounded on its own
__device__ __forceinline__ float norm2f(float2 a, float2 b) {
  return float_norm(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y));  // (nhip_common.h: the root is correctly rounded)
}

// The smoothness score of point i of a scan of n points, NaN for "no score" (too few neighbours, or 0 / 0).
// Neighbourhood order: the kept left neighbours ascending, the right neighbours ascending, the point itself.
template <class PT>
__device__ __forceinline__ double feat_score(PT pt, int32_t i, int32_t n, const nhip_feature_spec_t &S) {
  const int32_t P = S.neighbors_per_side;
  const float2 p = pt(i);
  uint64_t left = 0;  // bit k: neighbour i - P + k is kept
  int32_t cnt = 0;
  float mx = 0.f, my = 0.f;
  if (i >= P) {  // (the reference's start index i - P wraps for i < P: no left neighbours at all)
    for (int32_t k = 0; k < P; k++) {
      const float2 q = pt(i - P + k);
      if ((double)norm2f(p, q) <= S.max_neighbor_distance) {
        left |= 1ull << k;
        cnt++;
        mx = __fadd_rn(mx, q.x);
        my = __fadd_rn(my, q.y);
      }
    }
  }
  const int32_t rend = (n - i > P) ? i + P : n;  // min(n, i + P): P - 1 right neighbours, none of them distance-tested
  for (int32_t k = i + 1; k < rend; k++) {
    const float2 q = pt(k);
    mx = __fadd_rn(mx, q.x);
    my = __fadd_rn(my, q.y);
  }
  cnt += rend - i - 1;
  if (cnt < S.min_neighbors) return feat_nan();
  mx = __fadd_rn(mx, p.x);
  my = __fadd_rn(my, p.y);
  const float inv = (float)(1.0 / (double)(cnt + 1));
  mx = __fmul_rn(inv, mx);
  my = __fmul_rn(inv, my);
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
  auto add = [&](float2 q) {
    const float dx = __fsub_rn(q.x, mx), dy = __fsub_rn(q.y, my);
    a = __fadd_rn(a, __fmul_rn(dx, dx));
    b = __fadd_rn(b, __fmul_rn(dx, dy));
    c = __fadd_rn(c, __fmul_rn(dy, dx));
    d = __fadd_rn(d, __fmul_rn(dy, dy));
  };
  if (left)
    for (int32_t k = 0; k < P; k++)
      if ((left >> k) & 1ull) add(pt(i - P + k));
  for (int32_t k = i + 1; k < rend; k++) add(pt(k));
  add(p);
  // eigenvalues of [[a, b], [c, d]] in closed form in double, as lc_scatter_score_kernel (nhip_lc.hip)
  const double A = a, B = b, Cc = c, D = d;
  const double half_tr = __dmul_rn(0.5, __dadd_rn(A, D)), half_df = __dmul_rn(0.5, __dsub_rn(A, D));
  const double disc = __dadd_rn(__dmul_rn(half_df, half_df), __dmul_rn(B, Cc));
  const double root = __dsqrt_rn(disc < 0.0 ? 0.0 : disc);
  const double e1 = __dadd_rn(half_tr, root), e2 = __dsub_rn(half_tr, root);
  const double lo = e1 < e2 ? e1 : e2, hi = e1 < e2 ? e2 : e1;
  const double score = __ddiv_rn(lo, hi);
  return score != score ? feat_nan() : score;
}

// (score, index) keys, compared AS DOUBLES (scores can be slightly negative, and -0.0 ties with 0.0); index < 0: no key.
// Planar: the smallest key is the best; edge: the largest.
template <bool EDGE>
__device__ __forceinline__ bool key_better(double sa, int32_t ia, double sb, int32_t ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  return EDGE ? (sa > sb || (sa == sb && ia > ib)) : (sa < sb || (sa == sb && ia < ib));
}

template <bool EDGE>
__device__ __forceinline__ void wave_best(double &s, int32_t &i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double so = __shfl_xor(s, off, 64);
    const int32_t io = __shfl_xor(i, off, 64);
    if (key_better<EDGE>(so, io, s, i)) {
      s = so;
      i = io;
    }
  }
}

struct FeatShared {
  float2 xy[FEAT_LDS_N];
  double score[FEAT_LDS_N];
  uint8_t flag[FEAT_LDS_N];          // bit 0: out of the planar walk (accepted, or within the distance of one), bit 1: edge
  double red_s[2][2][FT / 64];       // [round parity][planar / edge][wave]
  int32_t red_i[2][2][FT / 64];
  int32_t idx[2][FEAT_MAX_CAP];      // the accepted indices, in acceptance order
  float2 acc[2][FEAT_MAX_CAP];       // their coordinates (read by the long-scan path only)
};

// One scan.  IN_LDS: n <= FEAT_LDS_N and sh.xy / sh.score / sh.flag hold it.  Returns the two counts (uniform).
template <bool IN_LDS>
__device__ __forceinline__ void feat_scan(const float2 *__restrict__ gxy, int32_t n, const nhip_feature_spec_t &S, FeatShared &sh,
                                          double *__restrict__ g_scores, int32_t &cnt_p, int32_t &cnt_e) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto pt = [&](int32_t i) -> float2 { return IN_LDS ? sh.xy[i] : gxy[i]; };
  // ---- phase 1
  if (IN_LDS) {
    for (int32_t i = tid; i < n; i += FT) sh.xy[i] = gxy[i];
    __syncthreads();
    for (int32_t i = tid; i < n; i += FT) {
      const double sc = feat_score(pt, i, n, S);
      sh.score[i] = sc;
      sh.flag[i] = 0;
      if (g_scores) g_scores[i] = sc;
    }
  } else if (g_scores) {
    for (int32_t i = tid; i < n; i += FT) g_scores[i] = feat_score(pt, i, n, S);
  }
  // ---- phase 2
  const double thr = S.threshold, dthr = S.distance_threshold;
  cnt_p = cnt_e = 0;
  bool done_p = false, done_e = false;
  int32_t last_p = -1, last_e = -1;  // accepted in the round before: their suppression pass is part of this round's scan
  float2 wp = make_float2(0.f, 0.f), we = wp;
  for (int round = 0; !(done_p && done_e); round++) {
    double bs_p = 0.0, bs_e = 0.0;
    int32_t bi_p = -1, bi_e = -1;
    for (int32_t i = tid; i < n; i += FT) {
      const float2 p = pt(i);
      uint32_t f = 0;
      double sc;
      if (IN_LDS) {
        f = sh.flag[i];
        if (last_p >= 0 && (i == last_p || (double)norm2f(wp, p) < dthr)) f |= 1u;
        if (last_e >= 0 && (i == last_e || (double)norm2f(we, p) < dthr)) f |= 2u;
        sh.flag[i] = (uint8_t)f;
        sc = sh.score[i];
      } else {
        for (int32_t k = 0; k < cnt_p; k++)
          if (i == sh.idx[0][k] || (double)norm2f(sh.acc[0][k], p) < dthr) f |= 1u;
        for (int32_t k = 0; k < cnt_e; k++)
          if (i == sh.idx[1][k] || (double)norm2f(sh.acc[1][k], p) < dthr) f |= 2u;
        if (((f & 1u) || done_p) && ((f & 2u) || done_e)) continue;
        sc = feat_score(pt, i, n, S);
      }
      if (sc != sc) continue;  // no score
      if (!done_p && !(f & 1u) && !(sc > thr) && key_better<false>(sc, i, bs_p, bi_p)) {
        bs_p = sc;
        bi_p = i;
      }
      if (!done_e && !(f & 2u) && !(sc < thr) && key_better<true>(sc, i, bs_e, bi_e)) {
        bs_e = sc;
        bi_e = i;
      }
    }
    // the workgroup's best keys: shuffles inside a wave, one LDS row per wave across them.  Rows alternate by round: a
    // wave writes round r + 2's only after the barrier of round r + 1, which every wave passes after reading round r's
    wave_best<false>(bs_p, bi_p);
    wave_best<true>(bs_e, bi_e);
    const int par = round & 1;
    if (lane == 0) {
      sh.red_s[par][0][wv] = bs_p;
      sh.red_i[par][0][wv] = bi_p;
      sh.red_s[par][1][wv] = bs_e;
      sh.red_i[par][1][wv] = bi_e;
    }
    __syncthreads();
    bi_p = bi_e = -1;
#pragma unroll
    for (int w = 0; w < FT / 64; w++) {
      const double sp = sh.red_s[par][0][w], se = sh.red_s[par][1][w];
      const int32_t ip = sh.red_i[par][0][w], ie = sh.red_i[par][1][w];
      if (key_better<false>(sp, ip, bs_p, bi_p)) {
        bs_p = sp;
        bi_p = ip;
      }
      if (key_better<true>(se, ie, bs_e, bi_e)) {
        bs_e = se;
        bi_e = ie;
      }
    }
    last_p = last_e = -1;
    if (!done_p) {
      if (bi_p >= 0) {
        wp = pt(bi_p);
        if (tid == 0) {
          sh.idx[0][cnt_p] = bi_p;
          sh.acc[0][cnt_p] = wp;
        }
        last_p = bi_p;
        done_p = ++cnt_p >= S.max_planar;
      } else {
        done_p = true;  // nothing eligible is left (the first key past the threshold is not eligible either)
      }
    }
    if (!done_e) {
      if (bi_e >= 0) {
        we = pt(bi_e);
        if (tid == 0) {
          sh.idx[1][cnt_e] = bi_e;
          sh.acc[1][cnt_e] = we;
        }
        last_e = bi_e;
        done_e = ++cnt_e >= S.max_edge;
      } else {
        done_e = true;
      }
    }
    if (!IN_LDS) __syncthreads();  // (the next round reads sh.idx / sh.acc)
  }
}

__global__ __launch_bounds__(FT) void feat_extract_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ offsets,
                                                          const nhip_feature_spec_t S, int32_t *__restrict__ planar_idx,
                                                          int32_t *__restrict__ planar_count, int32_t *__restrict__ edge_idx,
                                                          int32_t *__restrict__ edge_count, double *__restrict__ scores) {
  __shared__ FeatShared sh;
  const int32_t s = blockIdx.x;
  const int32_t beg = offsets[s];
  int32_t n = offsets[s + 1] - beg;
  if (n < 0) n = 0;
  int32_t cnt_p, cnt_e;
  if (n <= FEAT_LDS_N)
    feat_scan<true>(xy + beg, n, S, sh, scores ? scores + beg : nullptr, cnt_p, cnt_e);
  else
    feat_scan<false>(xy + beg, n, S, sh, scores ? scores + beg : nullptr, cnt_p, cnt_e);
  __syncthreads();
  for (int32_t k = threadIdx.x; k < S.max_planar; k += FT) planar_idx[(size_t)s * S.max_planar + k] = k < cnt_p ? sh.idx[0][k] : -1;
  for (int32_t k = threadIdx.x; k < S.max_edge; k += FT) edge_idx[(size_t)s * S.max_edge + k] = k < cnt_e ? sh.idx[1][k] : -1;
  if (threadIdx.x == 0) {
    planar_count[s] = cnt_p;
    edge_count[s] = cnt_e;
  }
}

// ---- packing ------------------------------------------------------------------------------------------------------
// idx and count are device memory of any origin: a count outside [0, cap] makes its scan contribute nothing, an index
// outside its scan is left out; both are reported (once, here), neither becomes an address.
__device__ __forceinline__ int32_t report_index(int64_t i) { return (int32_t)(i < 0x7fffffff ? i : 0x7fffffff); }

// offsets_out = exclusive scan of the scans' numbers of valid features (one workgroup, 1024 scans per step)
__global__ __launch_bounds__(1024) void feat_offsets_kernel(const int32_t *__restrict__ offsets, int32_t n_scans,
                                                            const int32_t *__restrict__ idx, const int32_t *__restrict__ count,
                                                            int32_t cap, int32_t *__restrict__ offsets_out,
                                                            uint32_t *__restrict__ status) {
  __shared__ int32_t sc[1024];
  __shared__ int32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int32_t base = 0; base < n_scans; base += 1024) {
    const int32_t s = base + threadIdx.x;
    int32_t v = 0;
    if (s < n_scans) {
      const int32_t ns = offsets[s + 1] - offsets[s], c = count[s];
      if (c < 0 || c > cap) {
        flag_bad_id(status, BAD_FEATURE_COUNT, c, s);
      } else {
        for (int32_t k = 0; k < c; k++) {
          const int32_t id = idx[(size_t)s * cap + k];
          if (id_in(id, ns)) v++;
          else flag_bad_id(status, BAD_FEATURE_IDX, id, report_index((int64_t)s * cap + k));
        }
      }
    }
    sc[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int32_t u = threadIdx.x >= off ? sc[threadIdx.x - off] : 0;
      __syncthreads();
      sc[threadIdx.x] += u;
      __syncthreads();
    }
    if (s < n_scans) offsets_out[s] = carry + sc[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += sc[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets_out[n_scans] = carry;
}

// one wave per scan, one lane per slot of its idx row (cap <= 64); valid entries keep their order
__global__ __launch_bounds__(FT) void feat_pack_kernel(const float2 *__restrict__ xy, const float2 *__restrict__ normals,
                                                       const int32_t *__restrict__ offsets, int32_t n_scans,
                                                       const int32_t *__restrict__ idx, const int32_t *__restrict__ count,
                                                       int32_t cap, const int32_t *__restrict__ offsets_out,
                                                       float2 *__restrict__ xy_out, float2 *__restrict__ normals_out) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * (FT / 64) + (threadIdx.x >> 6);
  if (s >= n_scans) return;
  const int32_t beg = offsets[s], ns = offsets[s + 1] - beg;
  int32_t c = count[s];
  if (c < 0 || c > cap) c = 0;
  const int32_t id = lane < c ? idx[(size_t)s * cap + lane] : -1;
  const bool ok = lane < c && id_in(id, ns);
  const unsigned long long m = __ballot(ok);
  if (!ok) return;
  const size_t o = (size_t)offsets_out[s] + (size_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
  xy_out[o] = xy[(size_t)beg + id];
  if (normals) normals_out[o] = normals[(size_t)beg + id];
}

}  // namespace

int launch_feat_extract(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const nhip_feature_spec_t &spec,
                        int32_t *d_planar_idx, int32_t *d_planar_count, int32_t *d_edge_idx, int32_t *d_edge_count,
                        double *d_scores, hipStream_t s) {
  if (n_scans == 0) return NHIP_OK;
  static_assert(FEAT_MAX_CAP == NHIP_FEATURE_MAX, "the kernel's arrays and the contract's limit");
  hipLaunchKernelGGL(feat_extract_kernel, dim3((uint32_t)n_scans), dim3(FT), 0, s, reinterpret_cast<const float2 *>(d_xy), d_offsets,
                     spec, d_planar_idx, d_planar_count, d_edge_idx, d_edge_count, d_scores);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

int launch_feat_pack(const float *d_xy, const float *d_normals, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_idx,
                     const int32_t *d_count, int32_t cap, float *d_xy_out, float *d_normals_out, int32_t *d_offsets_out,
                     hipStream_t s) {
  hipLaunchKernelGGL(feat_offsets_kernel, dim3(1), dim3(1024), 0, s, d_offsets, n_scans, d_idx, d_count, cap, d_offsets_out,
                     dev_status());
  if (n_scans > 0)
    hipLaunchKernelGGL(feat_pack_kernel, dim3((uint32_t)((n_scans + FT / 64 - 1) / (FT / 64))), dim3(FT), 0, s,
                       reinterpret_cast<const float2 *>(d_xy), reinterpret_cast<const float2 *>(d_normals), d_offsets, n_scans, d_idx,
                       d_count, cap, d_offsets_out, reinterpret_cast<float2 *>(d_xy_out), reinterpret_cast<float2 *>(d_normals_out));
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
