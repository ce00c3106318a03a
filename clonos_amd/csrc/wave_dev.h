// wave_dev.h -- what the kernels of the typed-columns family (columns.hip, payload.hip,
// encode_columns.hip and, through pack_dev.h, the four pack files) share below the level of a
// format: the wave's primitives on 32- and 64-bit unsigned words, the workgroup's minimum, a tile's
// exclusive scan across its threads, and the one-workgroup scan of per-tile values that every
// "ONE workgroup" pass of the family is.
// Device code only, file-local in each unit that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clg {
namespace {

// ---- the wave: 64 lanes -------------------------------------------------------------------------

// x of lane ^ o, and of lane - o (a lane below o gets its own), in the word's width.
__device__ __forceinline__ uint32_t wave_xor(uint32_t x, int o) { return (uint32_t)__shfl_xor((int)x, o, 64); }
__device__ __forceinline__ uint64_t wave_xor(uint64_t x, int o) {
  return (uint64_t)__shfl_xor((unsigned long long)x, o, 64);
}
__device__ __forceinline__ uint32_t wave_up(uint32_t x, uint32_t o) { return (uint32_t)__shfl_up((int)x, o, 64); }
__device__ __forceinline__ uint64_t wave_up(uint64_t x, uint32_t o) {
  return (uint64_t)__shfl_up((unsigned long long)x, o, 64);
}

// Set bits of m below this lane.
__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

// The wave's sum and minimum, in every lane.  T: uint32_t or uint64_t.
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += wave_xor(x, o);
  return x;
}
template <class T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T y = wave_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}

// The wave's inclusive prefix sum; lane 63 holds the wave's total.
template <class T>
__device__ __forceinline__ T wave_incl(T x, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const T y = wave_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// ---- the workgroup ------------------------------------------------------------------------------

// The minimum of x over a workgroup of kThreads, in thread 0: the waves' minima through LDS.  All
// threads call it; one __syncthreads inside.
template <uint32_t kThreads, class T>
__device__ __forceinline__ T block_min(T x) {
  __shared__ T wb[kThreads / 64];
  x = wave_min(x);
  if ((threadIdx.x & 63) == 0) wb[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t j = 1; j < kThreads / 64; ++j) x = wb[j] < x ? wb[j] : x;
  }
  return x;
}

// The values before this thread's among kWaves * 64 threads numbered tid (a workgroup, or the part
// of one that works on a tile): the exclusive scan of the threads' x.  ws: kWaves words of LDS of
// those threads' own.  All of them call it; one __syncthreads inside.
template <uint32_t kWaves>
__device__ __forceinline__ uint64_t tile_excl(uint64_t x, uint32_t tid, uint64_t* ws) {
  const uint32_t lane = tid & 63, w = tid >> 6;
  const uint64_t inc = wave_incl(x, lane);
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  uint64_t before = 0;
#pragma unroll
  for (uint32_t k = 0; k < kWaves; ++k) before += k < w ? ws[k] : 0;
  return before + inc - x;
}

// The one-workgroup scan of per-tile values: kLanes independent columns of n_tiles values each
// become their exclusive prefixes, and the columns' totals are returned (in every thread).  A tile
// a thread and round, kThreads tiles a round, no look-back: each wave scans its values, the waves
// combine through LDS, and a 64-bit carry runs across the rounds.
//   load(t, c)   fills c[0 .. kLanes) with tile t's values (t < n_tiles; the thread's own tile)
//   store(t, b)  takes tile t's exclusive prefixes b[0 .. kLanes), 64 bits each
// The store of a tile follows its load in the same thread, so the two may name the same memory.
// T is the element inside a round: uint32_t where kThreads of the largest values cannot pass 2^32
// (the instance states that bound in a static_assert), uint64_t otherwise.  All kThreads threads
// call it; the barriers inside are uniform (n_tiles is).
template <uint32_t kLanes>
struct ScanTotals {
  uint64_t v[kLanes];
};
template <uint32_t kThreads, uint32_t kLanes, class T, class Load, class Store>
__device__ __forceinline__ ScanTotals<kLanes> tile_scan(uint32_t n_tiles, Load load, Store store) {
  constexpr uint32_t kW = kThreads / 64;
  static_assert(kThreads % 64 == 0 && kW <= 64, "one wave scans the waves' totals");
  __shared__ T ws[kW][kLanes];
  __shared__ T wtot[kLanes];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  ScanTotals<kLanes> carry;
#pragma unroll
  for (uint32_t k = 0; k < kLanes; ++k) carry.v[k] = 0;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kThreads) {
    const uint32_t t = t0 + tid;
    T c[kLanes], inc[kLanes];
#pragma unroll
    for (uint32_t k = 0; k < kLanes; ++k) c[k] = 0;
    if (t < n_tiles) load(t, c);  // (the last round is partial: the threads past it scan zeros)
#pragma unroll
    for (uint32_t k = 0; k < kLanes; ++k) {
      inc[k] = wave_incl(c[k], lane);
      if (lane == 63) ws[w][k] = inc[k];
    }
    __syncthreads();
    if (tid < 64) {  // the waves' totals -> their exclusive prefix, and the round's total
#pragma unroll
      for (uint32_t k = 0; k < kLanes; ++k) {
        const T x = lane < kW ? ws[lane][k] : T(0);
        const T s = wave_incl(x, lane);
        if (lane < kW) ws[lane][k] = s - x;
        if (lane == kW - 1) wtot[k] = s;
      }
    }
    __syncthreads();
    uint64_t before[kLanes];
#pragma unroll
    for (uint32_t k = 0; k < kLanes; ++k) {
      before[k] = carry.v[k] + ws[w][k] + (inc[k] - c[k]);
      carry.v[k] += wtot[k];
    }
    if (t < n_tiles) store(t, before);
    __syncthreads();  // (ws and wtot are written again in the next round)
  }
  return carry;
}

}  // namespace
}  // namespace clg
