// nhip_submap.hip -- K10: the target cloud of a SUBMAP, made on the device in front of the table build.  A submap is an anchor
// scan plus members (scan id, float affine of the member's frame in the anchor's); its cloud is the members' transformed
// points, in member order then point order.  The spec is DESIGN.md section 3, "Submaps"; tests/submap_reference.py and
// hostside.submap_clouds restate it in numpy.
//
//   submap_offsets_kernel  one workgroup, 1024 targets per step, a lane per target: the merged length of every target (a
//                          member whose scan id is out of range counts 0 points and is reported), the exclusive scan that
//                          gives out_offsets[n_targets + 1].  A total beyond the caller's capacity (or beyond int32) is
//                          reported and EVERY entry of out_offsets becomes 0: the gather, which reads its extent from
//                          out_offsets[n_targets], then stores nothing, and a table build over the result finds empty
//                          targets instead of offsets past the buffer.
//   submap_gather_kernel   the streaming pass.  A workgroup owns chunks of SUB_CHUNK consecutive OUTPUT points (grid-stride),
//                          whatever targets and members they fall into: it finds the chunk's first target by bisection of
//                          out_offsets, loads that target's member list 256 members at a time -- lane m: id, length, source
//                          offset, affine -- into LDS with the members' output offsets from a workgroup scan, and every lane
//                          finds the member of each of its points by bisection of that table.  Loads are float2 runs of a
//                          member (contiguous in the scan), stores float2 and contiguous across the whole chunk.  A target
//                          of 11 dense members is a dozen chunks of equal work, a target of one short member a fraction
//                          of one: nothing serialises, no atomics.
//
// The point transform is  x' = ((c x) + ((-s) y)) + tx,  y' = ((s x) + (c y)) + ty  in float, every operation rounded on its
// own (build-defined): the intrinsics below keep that whatever the unit's contraction setting.  Non-finite points come out
// non-finite; nothing is dropped, clipped or deduplicated -- the table build drops what leaves the grid, as always.
#include "nhip_common.h"

#pragma clang fp contract(off)

namespace nhip {

namespace {

constexpr int SUB_T = 256;         // threads of a gather workgroup = members of a target held in LDS at a time
constexpr int SUB_CHUNK = 2048;    // output points of a chunk: 8 per lane
constexpr int SUB_MAX_GRID = 2048; // 256 CUs x 8 workgroups; the chunks beyond are taken grid-stride

// points of member m (0 for an id outside [0, n_scans): never dereferenced); *src: the index of its first point
__device__ __forceinline__ int32_t member_points(const int32_t *__restrict__ offsets, int32_t n_scans, int32_t id, int32_t *src) {
  *src = 0;
  if (!id_in(id, n_scans)) return 0;
  const int32_t b = offsets[id], e = offsets[id + 1];
  *src = b;
  return e > b ? e - b : 0;
}

__global__ __launch_bounds__(1024) void submap_offsets_kernel(const int32_t *__restrict__ offsets, int32_t n_scans,
                                                              const int32_t *__restrict__ member_scan,
                                                              const int32_t *__restrict__ member_offsets, int32_t n_targets,
                                                              int64_t out_capacity, int32_t *__restrict__ out_offsets,
                                                              uint32_t *__restrict__ status) {
  __shared__ long long sc[1024];
  __shared__ long long carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int32_t base = 0; base < n_targets; base += 1024) {
    const int32_t tg = base + t;
    long long len = 0;
    if (tg < n_targets) {
      const int32_t mb = member_offsets[tg], me = member_offsets[tg + 1];
      for (int32_t m = mb; m < me; m++) {
        const int32_t id = member_scan[m];
        int32_t src;
        len += member_points(offsets, n_scans, id, &src);
        if (!id_in(id, n_scans)) flag_bad_id(status, BAD_MEMBER_ID, id, m);
      }
    }
    sc[t] = len;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const long long u = t >= off ? sc[t - off] : 0;
      __syncthreads();
      sc[t] += u;
      __syncthreads();
    }
    // (entries past the capacity are written truncated here and zeroed below)
    if (tg < n_targets) out_offsets[tg] = (int32_t)(carry + sc[t] - len);
    __syncthreads();
    if (t == 0) carry += sc[1023];
    __syncthreads();
  }
  const long long total = carry;
  const bool fits = total <= (long long)out_capacity && total <= 0x7fffffffll;
  if (!fits)
    for (int32_t tg = t; tg < n_targets; tg += 1024) out_offsets[tg] = 0;  // (target tg was written by this thread)
  if (t == 0) {
    out_offsets[n_targets] = fits ? (int32_t)total : 0;
    if (!fits) flag_bad_id(status, BAD_SUBMAP_CAPACITY, (int32_t)(total > 0x7fffffffll ? 0x7fffffffll : total), n_targets);
  }
}

__global__ __launch_bounds__(SUB_T) void submap_gather_kernel(const float2 *__restrict__ xy, const int32_t *__restrict__ offsets,
                                                              int32_t n_scans, const int32_t *__restrict__ member_scan,
                                                              const float *__restrict__ member_affine,
                                                              const int32_t *__restrict__ member_offsets, int32_t n_targets,
                                                              float2 *__restrict__ out_xy, int64_t out_capacity,
                                                              const int32_t *__restrict__ out_offsets) {
  __shared__ int32_t s_start[SUB_T];  // output index of the member's first point
  __shared__ int32_t s_src[SUB_T];    // index of its first point in xy
  __shared__ float4 s_aff[SUB_T];     // c, s, tx, ty
  __shared__ int32_t s_wave[SUB_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t total = out_offsets[n_targets];
  if (total <= 0 || total > out_capacity) return;  // (nothing to do, or the offsets kernel refused: it wrote 0)
  for (int64_t pos = (int64_t)blockIdx.x * SUB_CHUNK; pos < total; pos += (int64_t)gridDim.x * SUB_CHUNK) {
    const int64_t end = pos + SUB_CHUNK < total ? pos + SUB_CHUNK : total;
    // the target of the chunk's first point: out_offsets[lo] <= pos < out_offsets[hi] (0 <= pos < total holds it at the ends)
    int32_t lo = 0, hi = n_targets;
    while (hi - lo > 1) {
      const int32_t mid = lo + (hi - lo) / 2;
      if (out_offsets[mid] <= pos) lo = mid;
      else hi = mid;
    }
    int64_t at = pos;  // the first point of the chunk not yet written (uniform)
    for (int32_t tg = lo; tg < n_targets && at < end; tg++) {
      const int64_t t_beg = out_offsets[tg], t_end = out_offsets[tg + 1];
      if (t_end <= at) continue;  // (an empty target)
      const int64_t t_stop = t_end < end ? t_end : end;
      const int32_t mb = member_offsets[tg], me = member_offsets[tg + 1];
      int64_t run = t_beg;  // output index of the first member of the batch
      for (int32_t base = mb; base < me && at < t_stop; base += SUB_T) {
        const int32_t m = base + tid;
        const int nb = me - base < SUB_T ? me - base : SUB_T;  // members of this batch
        int32_t len = 0, src = 0;
        float4 aff = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        if (m < me) {
          len = member_points(offsets, n_scans, member_scan[m], &src);
          const float *a4 = member_affine + 4 * (size_t)m;  // (four loads: the array need not be 16-byte aligned)
          aff = make_float4(a4[0], a4[1], a4[2], a4[3]);
        }
        // inclusive scan of the lengths over the workgroup: in the wave by shuffles, across the four waves through LDS
        int32_t inc = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int32_t u = __shfl_up(inc, d, 64);
          if (lane >= d) inc += u;
        }
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        int32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SUB_T / 64; w++) {
          const int32_t c = s_wave[w];
          if (w < wv) before += c;
          all += c;
        }
        s_start[tid] = (int32_t)(run + before + inc - len);
        s_src[tid] = src;
        s_aff[tid] = aff;
        __syncthreads();
        const int64_t b_end = run + all;
        if (b_end > at) {
          const int64_t stop = b_end < t_stop ? b_end : t_stop;
          for (int64_t i = at + tid; i < stop; i += SUB_T) {
            // the last member of the batch that starts at or before point i (the first does: run <= at): members without
            // points share their start with the next one and are passed over
            int a = 0, b = nb;
            while (b - a > 1) {
              const int mid = (a + b) >> 1;
              if (s_start[mid] <= i) a = mid;
              else b = mid;
            }
            const float4 T = s_aff[a];
            const float2 p = xy[(size_t)s_src[a] + (size_t)(i - s_start[a])];
            float2 q;
            q.x = __fadd_rn(__fadd_rn(__fmul_rn(T.x, p.x), __fmul_rn(-T.y, p.y)), T.z);
            q.y = __fadd_rn(__fadd_rn(__fmul_rn(T.y, p.x), __fmul_rn(T.x, p.y)), T.w);
            out_xy[i] = q;  // (i < stop <= total <= out_capacity)
          }
          at = stop;
        }
        run = b_end;
        __syncthreads();  // (the table is rewritten by the next batch)
      }
      // (out_offsets is this call's own sum of the same lengths: the members have covered the target up to t_stop.  Were
      //  the arrays changed under the kernel, points stay unwritten; the walk still ends)
      at = t_stop;
    }
  }
}

}  // namespace

int launch_submap_gather(const float *d_xy, const int32_t *d_offsets, int32_t n_scans, const int32_t *d_member_scan,
                         const float *d_member_affine, const int32_t *d_member_offsets, int32_t n_targets, float *d_out_xy,
                         int64_t out_capacity, int32_t *d_out_offsets, hipStream_t s) {
  hipLaunchKernelGGL(submap_offsets_kernel, dim3(1), dim3(1024), 0, s, d_offsets, n_scans, d_member_scan, d_member_offsets,
                     n_targets, out_capacity, d_out_offsets, dev_status());
  const int64_t cap = out_capacity < 0x7fffffffll ? out_capacity : 0x7fffffffll;
  const int64_t chunks = (cap + SUB_CHUNK - 1) / SUB_CHUNK;
  if (chunks > 0 && n_targets > 0)
    hipLaunchKernelGGL(submap_gather_kernel, dim3((uint32_t)(chunks < SUB_MAX_GRID ? chunks : SUB_MAX_GRID)), dim3(SUB_T), 0, s,
                       reinterpret_cast<const float2 *>(d_xy), d_offsets, n_scans, d_member_scan,
                       d_member_affine, d_member_offsets, n_targets,
                       reinterpret_cast<float2 *>(d_out_xy), out_capacity, d_out_offsets);
  NHIP_TRY_HIP(hipGetLastError());
  return NHIP_OK;
}

}  // namespace nhip
