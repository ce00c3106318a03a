// pack_dev.h -- what the pack kernels of pack.hip and pack_wide.hip share on the device: the
// workgroup's shape, the wave's signed minimum / maximum by DPP and the wave scans.  Device code
// only, file-local in each unit that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pack.h"

namespace clg {
namespace {

constexpr uint32_t kPackThreads = 256;
constexpr uint32_t kPackWaves = kPackThreads / 64;
constexpr uint32_t kPackPerThread = kPackBlock / kPackThreads;
constexpr uint32_t kPackTopThreads = 1024;
static_assert(kPackPerThread == 4, "four values a thread");
static_assert(kPackScanGroup == kPackThreads, "the group passes take a block a thread");

// v of the lane the DPP control names; a lane without a source keeps its own.
template <int kCtrl>
__device__ __forceinline__ int64_t pack_dpp(int64_t v) {
  const uint32_t lo = uint32_t(uint64_t(v)), hi = uint32_t(uint64_t(v) >> 32);
  const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp((int)lo, (int)lo, kCtrl, 0xF, 0xF, false);
  const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp((int)hi, (int)hi, kCtrl, 0xF, 0xF, false);
  return int64_t(uint64_t(a) | uint64_t(b) << 32);
}
__device__ __forceinline__ int64_t pack_lane63(int64_t v) {
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)uint32_t(uint64_t(v)), 63);
  const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)uint32_t(uint64_t(v) >> 32), 63);
  return int64_t(uint64_t(a) | uint64_t(b) << 32);
}
__device__ __forceinline__ int64_t pack_min(int64_t a, int64_t b) { return b < a ? b : a; }
__device__ __forceinline__ int64_t pack_max(int64_t a, int64_t b) { return b > a ? b : a; }
// The wave's signed minimum / maximum: quads, the rows of 16 (row_ror 4 and 8), then
// row_bcast 15 and 31; lane 63 holds the result.
#define CLG_PACK_WAVE_REDUCE(op, v)       \
  v = op(v, pack_dpp<0xB1>(v));           \
  v = op(v, pack_dpp<0x4E>(v));           \
  v = op(v, pack_dpp<0x124>(v));          \
  v = op(v, pack_dpp<0x128>(v));          \
  v = op(v, pack_dpp<0x142>(v));          \
  v = op(v, pack_dpp<0x143>(v));          \
  v = pack_lane63(v)

__device__ __forceinline__ uint32_t pack_wave_incl(uint32_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}
__device__ __forceinline__ uint64_t pack_wave_incl64(uint64_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}

}  // namespace
}  // namespace clg
