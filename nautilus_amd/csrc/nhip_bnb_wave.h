// nhip_bnb_wave.h -- lane exchanges and wave-level reductions of the branch-and-bound matcher's kernels (nhip_bnb.hip).
//
// Owns: the xor shuffles, the one-lane-acts-for-the-wave idiom (wave_leader and the atomics built on it), the steps of
// the transposing reduction over packed sums (rs_pair / rs_step / add_xor), the 24-bit multiply-add, and the sums and
// maxima over 8 lanes and over the wave.  None of them goes through LDS: DPP inside a row of 16 lanes, permlane swaps
// across rows.
// Assumes: wave64 on gfx950 (v_permlane16_swap / v_permlane32_swap, DPP row_bcast), all 64 lanes active at every call.
// Knows nothing of BnbParams or of the search; included by nhip_bnb.hip only (both of its builds).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nhip {
namespace {

constexpr uint32_t M8 = 0x00ff00ffu;  // the even bytes of a register: two byte sums in 16-bit fields

__device__ __forceinline__ uint32_t shfl_xor_u32(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }

__device__ __forceinline__ unsigned long long shfl_xor_u64b(unsigned long long v, int m) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  lo = shfl_xor_u32(lo, m);
  hi = shfl_xor_u32(hi, m);
  return ((unsigned long long)hi << 32) | lo;
}

// ---- one lane acts for the wave ------------------------------------------------------------------------------
// `if (lane == 0) x = atomicAdd(...); x = readfirstlane(x);` at the head of a loop whose body ends in
// `if (lane == 0) atomicMax(...)` is two tests of ONE value, and hipcc threads the second into the first: lanes 1..63,
// for which both are false, get a loop of their own that bypasses both blocks, and lane 0 is parked until they leave
// it.  readfirstlane is a convergent operation: without lane 0 it returns lane 1's x = 0, the sub-wave takes entry 0
// again and again (lane 0's atomicMax, which would prune it, never runs) and the kernel does not return.  That was the
// hang of the general instantiation under NHIP_BNB_LEVELS=1 once its counters were compiled out (round 3; the
// counters' increments kept the two blocks apart): profiles/r04_general_kernel_hang_isa.txt shows the threaded loop.
// So the lane id of every such test passes through an empty asm: each test is then of a value the compiler knows
// nothing about, and no two of them can be related.
__device__ __forceinline__ bool wave_leader(int lane) {
  asm volatile("" : "+v"(lane));
  return lane == 0;
}
// atomicAdd by one lane, the old value in every lane (wave-uniform, in a scalar register)
__device__ __forceinline__ uint32_t wave_fetch_add(uint32_t *p, uint32_t v, int lane) {
  uint32_t r = 0u;
  if (wave_leader(lane)) r = atomicAdd(p, v);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
}
// atomicMax of a wave-uniform key by one lane (generic address: LDS or global)
__device__ __forceinline__ void wave_atomic_max(unsigned long long *p, unsigned long long key, int lane) {
  if (wave_leader(lane)) atomicMax(p, key);
}

// One step of a transposing reduction over the lanes: lanes pair up across MASK; of every two registers the
// lane keeps the one its own bit selects, adds the partner's copy of the same register, and gives the other away.
// N registers in, N / 2 out.  No step goes through LDS:
//   MASK 1, 2   partners inside a quad: DPP quad permutation fused into the add;
//   MASK 4, 8   partners inside a row of 16 lanes: two DPP adds with complementary BANK masks (a bank = 4 lanes) --
//               lanes whose bit is clear add register 2i of the lane MASK above (row_ror:16 - MASK), the others
//               register 2i + 1 of the lane MASK below (row_ror:MASK); no select instructions at all;
//   MASK 16, 32 partners in another row / the other half of the wave: v_permlane16_swap / v_permlane32_swap
//               exchange the odd rows (upper half) of register 2i with the even rows (lower half) of register
//               2i + 1, after which the two registers hold own and partner's copy lane by lane: one add.
template <int MASK>
__device__ __forceinline__ uint32_t shfl_xor_c(uint32_t v) {
  if (MASK == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);  // quad_perm [1, 0, 3, 2]
  if (MASK == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2, 3, 0, 1]
  return shfl_xor_u32(v, MASK);
}

template <int MASK>
__device__ __forceinline__ uint32_t rs_pair(uint32_t x, uint32_t y, bool bit) {
  if (MASK == 4) {
    uint32_t r;
    // (s_nop 1: a DPP operand written by the previous vector instruction needs two wait states)
    asm volatile("s_nop 1\n\tv_add_u32_dpp %0, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_u32_dpp %0, %2, %2 row_ror:4 row_mask:0xf bank_mask:0xa"
                 : "=&v"(r) : "v"(x), "v"(y));
    return r;
  }
  if (MASK == 8) {
    uint32_t r;
    asm volatile("s_nop 1\n\tv_add_u32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_u32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xc"
                 : "=&v"(r) : "v"(x), "v"(y));
    return r;
  }
  if (MASK == 16) {
    const auto sw = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    return sw[0] + sw[1];
  }
  if (MASK == 32) {
    const auto sw = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    return sw[0] + sw[1];
  }
  const uint32_t keep = bit ? y : x, send = bit ? x : y;
  return keep + shfl_xor_c<MASK>(send);
}

template <int N, int MASK, int CAP>
__device__ __forceinline__ void rs_step(uint32_t (&R)[CAP], bool bit) {
  static_assert(N <= CAP, "rs_step: more registers than the array holds");
#pragma unroll
  for (int i = 0; i < N / 2; i++) R[i] = rs_pair<MASK>(R[2 * i], R[2 * i + 1], bit);
}

// sum over the lane pairs MASK apart of one register (the tail of a reduction whose copies may coincide)
template <int MASK>
__device__ __forceinline__ uint32_t add_xor(uint32_t v) {
  if (MASK == 16) {
    const auto sw = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return sw[0] + sw[1];
  }
  if (MASK == 32) {
    const auto sw = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return sw[0] + sw[1];
  }
  return v + shfl_xor_u32(v, MASK);
}

// acc + a * b on 24-bit factors as ONE v_mad_u32_u24, whatever the compiler learns about the bits of the result that are
// used: where only part of a packed sum is read later (the fields O[y][2] of the gather below, whose high halves are
// unused or carry block row 10) hipcc narrows `acc += __umul24(a, b)` and then selects the quarter-rate v_mad_u64_u32.
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t acc) {
  uint32_t r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));
  return r;
}

// sum over each aligned group of 8 lanes, in all of them
__device__ __forceinline__ uint32_t sum8(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1, 0, 3, 2]
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
}
// sum over the wave of a value that is the same in each aligned group of 8 lanes, counted once per group (wave-uniform)
__device__ __forceinline__ uint32_t wave_total_of8(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror: the row's other half
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xF, 0xF, false);  // row_bcast:15: the row above's sum
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xF, 0xF, false);  // row_bcast:31: rows 0 + 1 into 2, 3
  // (lane 63 holds the total whatever the rows without a source lane received: its own two sources do have one)
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// sum and max over the 64 lanes, no LDS: DPP inside a row of 16, permlane swaps across rows
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1, 0, 3, 2]
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);  // row_ror:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
  v = add_xor<16>(v);
  return add_xor<32>(v);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false));
  const auto s16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = max(s16[0], s16[1]);
  const auto s32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return max(s32[0], s32[1]);
}
// the bitwise OR over the 64 lanes, by the same route (wave-uniform, in a scalar register)
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
  const auto s16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = s16[0] | s16[1];
  const auto s32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(s32[0] | s32[1]));
}
// the same over 64-bit keys (both halves take the same route; every lane ends with the wave's maximum)
template <int CTRL>
__device__ __forceinline__ unsigned long long max_dpp_u64(unsigned long long v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o > v ? o : v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  v = max_dpp_u64<0xB1>(v);
  v = max_dpp_u64<0x4E>(v);
  v = max_dpp_u64<0x124>(v);
  v = max_dpp_u64<0x128>(v);
  {
    const auto l = __builtin_amdgcn_permlane16_swap((uint32_t)v, (uint32_t)v, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap((uint32_t)(v >> 32), (uint32_t)(v >> 32), false, false);
    const unsigned long long a = ((unsigned long long)h[0] << 32) | l[0], b = ((unsigned long long)h[1] << 32) | l[1];
    v = a > b ? a : b;
  }
  const auto l = __builtin_amdgcn_permlane32_swap((uint32_t)v, (uint32_t)v, false, false);
  const auto h = __builtin_amdgcn_permlane32_swap((uint32_t)(v >> 32), (uint32_t)(v >> 32), false, false);
  const unsigned long long a = ((unsigned long long)h[0] << 32) | l[0], b = ((unsigned long long)h[1] << 32) | l[1];
  return a > b ? a : b;
}

}  // namespace
}  // namespace nhip
