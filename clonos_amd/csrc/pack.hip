// pack.hip -- packed typed columns (pack.h): the five narrow columns bit-packed block by block
// where they lie, so that what crosses the link is the bits the values hold.
//
//  * k_pack_measure     pass 1: a workgroup per block of kPackBlock values, all five streams in
//                       one grid.  Four coalesced values a thread, the DELTA predecessor through
//                       LDS, the residuals' signed minimum and maximum by a DPP wave reduction and
//                       LDS across the four waves; writes ref, first, width, count and, in pos,
//                       the payload's size
//  * k_pack_scan_sums   pass 2a: a workgroup per group of kPackScanGroup blocks sums their sizes
//  * k_pack_scan_top    pass 2b: ONE workgroup scans the groups' sums (config 2's 125 K blocks are
//                       489 groups: one round) and writes the total to pinned memory, which the
//                       host checks against the capacities before anything is written to the caller
//  * k_pack_scan_apply  pass 2c: a workgroup per group scans its blocks' sizes and adds the
//                       group's base: pos becomes the payload's offset
//  * k_pack_write       pass 3: a workgroup per block reloads the values, forms p_i, assembles
//                       the payload in 8 KiB of LDS and stores it with one aligned 16-byte store
//                       a lane; the descriptor goes to the caller's array
//
// Kernel boundaries order the passes.  No global atomics, no spin waits, no word taken from
// another running workgroup, no scratch; LDS atomics only inside a workgroup.  The result is a
// pure function of the columns.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "pack.h"
#include "pack_dev.h"
#include "kernels.h"

namespace clg {

namespace {

// The stream that holds block blk: the last one whose base is at or below it (the bases do not
// decrease, and an empty stream shares its base with the next).
__device__ __forceinline__ uint32_t pack_stream_of(const PackIn& in, uint64_t blk) {
  return uint32_t(blk >= in.blk_base[1]) + uint32_t(blk >= in.blk_base[2]) + uint32_t(blk >= in.blk_base[3]) +
         uint32_t(blk >= in.blk_base[4]);
}
// The block's place in its stream.
struct PackAt {
  const void* col;
  uint64_t i0;  // the block's first value
  uint32_t m;   // its values
};
__device__ __forceinline__ PackAt pack_at(const void* col, uint64_t n, uint64_t base, uint64_t blk) {
  const uint64_t i0 = (blk - base) * kPackBlock;
  const uint64_t left = i0 < n ? n - i0 : 0;
  return PackAt{col, i0, uint32_t(left < kPackBlock ? left : kPackBlock)};
}
// The kernels' bodies are instantiated per stream (the element type and the scheme are then
// constants) and the argument arrays are only ever indexed by constants.
#define CLG_PACK_DISPATCH(in, blk, body, ...)                                                   \
  switch (pack_stream_of(in, blk)) {                                                            \
    case 0: body<0>(pack_at(in.col[0], in.n[0], in.blk_base[0], blk), __VA_ARGS__); break;      \
    case 1: body<1>(pack_at(in.col[1], in.n[1], in.blk_base[1], blk), __VA_ARGS__); break;      \
    case 2: body<2>(pack_at(in.col[2], in.n[2], in.blk_base[2], blk), __VA_ARGS__); break;      \
    case 3: body<3>(pack_at(in.col[3], in.n[3], in.blk_base[3], blk), __VA_ARGS__); break;      \
    default: body<4>(pack_at(in.col[4], in.n[4], in.blk_base[4], blk), __VA_ARGS__); break;     \
  }

template <uint32_t kC>
__device__ __forceinline__ void pack_measure_body(const PackAt at, clg_pack_block* __restrict__ desc, int64_t* s_x,
                                                  int64_t* s_lo, int64_t* s_hi) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  constexpr bool delta = kC == CLG_PACK_TIMESTAMP;
  int64_t x[kPackPerThread];
#pragma unroll
  for (uint32_t k = 0; k < kPackPerThread; ++k) {
    const uint32_t i = k * kPackThreads + tid;
    x[k] = i < at.m ? pack_load(kC, at.col, at.i0 + i) : 0;
  }
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  if (delta) {
#pragma unroll
    for (uint32_t k = 0; k < kPackPerThread; ++k) s_x[k * kPackThreads + tid] = x[k];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPackPerThread; ++k) {
      const uint32_t i = k * kPackThreads + tid;
      if (i >= 1 && i < at.m) {
        const int64_t r = int64_t(uint64_t(x[k]) - uint64_t(s_x[i - 1]));
        lo = pack_min(lo, r), hi = pack_max(hi, r);
      }
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kPackPerThread; ++k)
      if (k * kPackThreads + tid < at.m) lo = pack_min(lo, x[k]), hi = pack_max(hi, x[k]);
  }
  CLG_PACK_WAVE_REDUCE(pack_min, lo);
  CLG_PACK_WAVE_REDUCE(pack_max, hi);
  if (lane == 0) s_lo[w] = lo, s_hi[w] = hi;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (uint32_t j = 1; j < kPackWaves; ++j) lo = pack_min(lo, s_lo[j]), hi = pack_max(hi, s_hi[j]);
    const uint32_t k = pack_resid(kC, at.m);
    clg_pack_block d;
    d.ref = k ? lo : 0;
    d.first = delta && at.m ? x[0] : 0;  // (thread 0's first value is the block's)
    d.width = k ? pack_width(uint64_t(hi) - uint64_t(lo)) : 0;
    d.count = at.m;
    d.pos = pack_payload_bytes(k, d.width);  // the size; the scan turns it into the offset
    desc[blockIdx.x] = d;
  }
}

// s_w: 8 KiB, the block's values (the DELTA predecessors), then the payload's words.
template <uint32_t kC>
__device__ __forceinline__ void pack_write_body(const PackAt at, const clg_pack_block d, unsigned long long* s_w,
                                                uint8_t* __restrict__ bits, uint64_t lim_bits) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr bool delta = kC == CLG_PACK_TIMESTAMP;
  const uint32_t k = pack_resid(kC, at.m), width = d.width;
  const uint32_t bytes = pack_payload_bytes(k, width);
  if (!bytes) return;  // (uniform: a constant block, or a DELTA block of one value)
  const uint32_t n_words = bytes / 8;
  uint64_t p[kPackPerThread];
  uint32_t j[kPackPerThread];  // the residual's index; >= k: none
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t i = q * kPackThreads + tid;
    p[q] = i < at.m ? uint64_t(pack_load(kC, at.col, at.i0 + i)) : 0;
    j[q] = i < at.m ? i : kPackBlock;
  }
  if (delta) {
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) s_w[q * kPackThreads + tid] = p[q];
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) {
      const uint32_t i = q * kPackThreads + tid;
      if (i >= 1 && i < at.m) p[q] -= s_w[i - 1], j[q] = i - 1;
      else j[q] = kPackBlock;
    }
    __syncthreads();  // (s_w is written again below)
  }
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) p[q] -= uint64_t(d.ref);

  if (width == 64) {  // a word a value: no shifts
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q)
      if (j[q] < k) s_w[j[q]] = p[q];
    if (tid == 0 && (k & 1)) s_w[k] = 0;  // the padding word
  } else if (width == 1 && !delta) {  // a wave's 64 values are one word: a ballot
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) {
      const uint64_t m = __ballot(j[q] < k && (p[q] & 1));
      const uint32_t word = q * kPackWaves + wv;
      if (lane == 0 && word < n_words) s_w[word] = m;
    }
  } else {
    for (uint32_t i = tid; i < n_words; i += kPackThreads) s_w[i] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q)
      if (j[q] < k) {
        const uint32_t bit = j[q] * width, sh = bit & 63;
        atomicOr(&s_w[bit >> 6], (unsigned long long)(p[q] << sh));
        if (sh + width > 64) atomicOr(&s_w[(bit >> 6) + 1], (unsigned long long)(p[q] >> (64 - sh)));  // (sh > 0)
      }
  }
  __syncthreads();
  for (uint32_t i = tid; i < bytes / 16; i += kPackThreads) {
    const uint64_t a = d.pos + uint64_t(i) * 16;
    if (a + 16 <= lim_bits) {
      const unsigned long long lo = s_w[2 * i], hi = s_w[2 * i + 1];
      *reinterpret_cast<uint4*>(bits + a) = make_uint4(uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32));
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kPackThreads) void k_pack_measure(const PackIn in, clg_pack_block* __restrict__ desc) {
  __shared__ int64_t s_x[kPackBlock];  // the block's values: the DELTA predecessors
  __shared__ int64_t s_lo[kPackWaves], s_hi[kPackWaves];
  CLG_PACK_DISPATCH(in, blockIdx.x, pack_measure_body, desc, s_x, s_lo, s_hi)
}

__global__ __launch_bounds__(kPackThreads) void k_pack_scan_sums(const clg_pack_block* __restrict__ desc, uint32_t n_blocks,
                                                                uint64_t* __restrict__ gsum) {
  __shared__ uint32_t ws[kPackWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t b = uint64_t(blockIdx.x) * kPackScanGroup + tid;
  const uint32_t x = b < n_blocks ? uint32_t(desc[b].pos) : 0u;  // (at most 8 KiB a block)
  const uint32_t s = pack_wave_incl(x, lane);
  if (lane == 63) ws[w] = s;
  __syncthreads();
  if (tid == 0) {
    uint64_t t = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPackWaves; ++j) t += ws[j];
    gsum[blockIdx.x] = t;
  }
}

// The groups' sums -> their exclusive prefix, in place; the total -> *res.  One workgroup, a
// group a thread and round: no look-back.
__global__ __launch_bounds__(kPackTopThreads) void k_pack_scan_top(uint64_t* __restrict__ gsum, uint32_t n_groups,
                                                                  PackRes* __restrict__ res) {
  constexpr uint32_t kW = kPackTopThreads / 64;
  __shared__ uint64_t ws[kW];
  __shared__ uint64_t wtot;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint64_t carry = 0;
  for (uint32_t g0 = 0; g0 < n_groups; g0 += kPackTopThreads) {
    const uint32_t g = g0 + tid;
    const uint64_t x = g < n_groups ? gsum[g] : 0;
    const uint64_t inc = pack_wave_incl64(x, lane);
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    if (tid < 64) {
      const uint64_t y = lane < kW ? ws[lane] : 0;
      const uint64_t s = pack_wave_incl64(y, lane);
      if (lane < kW) ws[lane] = s - y;
      if (lane == kW - 1) wtot = s;
    }
    __syncthreads();
    if (g < n_groups) gsum[g] = carry + ws[w] + (inc - x);
    carry += wtot;
    __syncthreads();  // (ws is written again in the next round)
  }
  if (tid == 0) res->n_bits = carry;
}

__global__ __launch_bounds__(kPackThreads) void k_pack_scan_apply(clg_pack_block* __restrict__ desc, uint32_t n_blocks,
                                                                 const uint64_t* __restrict__ gsum) {
  __shared__ uint32_t ws[kPackWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t b = uint64_t(blockIdx.x) * kPackScanGroup + tid;
  const uint32_t x = b < n_blocks ? uint32_t(desc[b].pos) : 0u;
  const uint32_t inc = pack_wave_incl(x, lane);
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPackWaves; ++j) before += j < w ? ws[j] : 0u;
  if (b < n_blocks) desc[b].pos = gsum[blockIdx.x] + before + (inc - x);
}

__global__ __launch_bounds__(kPackThreads) void k_pack_write(const PackIn in, const clg_pack_block* __restrict__ desc,
                                                            clg_pack_block* __restrict__ out_desc,
                                                            uint8_t* __restrict__ bits, uint64_t lim_desc,
                                                            uint64_t lim_bits) {
  __shared__ unsigned long long s_w[kPackBlock];
  const clg_pack_block d = desc[blockIdx.x];  // (uniform)
  if (threadIdx.x == 0 && blockIdx.x < lim_desc) out_desc[blockIdx.x] = d;
  CLG_PACK_DISPATCH(in, blockIdx.x, pack_write_body, d, s_w, bits, lim_bits)
}

int launch_pack_measure_scan(const PackIn& in, uint32_t n_blocks, clg_pack_block* d_desc, uint64_t* d_gsum, PackRes* res,
                             void* stream) {
  if (n_blocks) hipLaunchKernelGGL(k_pack_measure, dim3(n_blocks), dim3(kPackThreads), 0, (hipStream_t)stream, in, d_desc);
  return launch_pack_scan(n_blocks, d_desc, d_gsum, res, stream);
}

int launch_pack_scan(uint32_t n_blocks, clg_pack_block* d_desc, uint64_t* d_gsum, PackRes* res, void* stream) {
  const uint32_t n_groups = (n_blocks + kPackScanGroup - 1) / kPackScanGroup;
  if (n_blocks)
    hipLaunchKernelGGL(k_pack_scan_sums, dim3(n_groups), dim3(kPackThreads), 0, (hipStream_t)stream, d_desc, n_blocks, d_gsum);
  hipLaunchKernelGGL(k_pack_scan_top, dim3(1), dim3(kPackTopThreads), 0, (hipStream_t)stream, d_gsum, n_groups, res);
  if (n_blocks)
    hipLaunchKernelGGL(k_pack_scan_apply, dim3(n_groups), dim3(kPackThreads), 0, (hipStream_t)stream, d_desc, n_blocks, d_gsum);
  return launch_status(hipGetLastError());
}

int launch_pack_write(const PackIn& in, uint32_t n_blocks, const clg_pack_block* d_desc, clg_pack_block* out_desc,
                      uint8_t* bits, uint64_t lim_desc, uint64_t lim_bits, void* stream) {
  if (n_blocks)
    hipLaunchKernelGGL(k_pack_write, dim3(n_blocks), dim3(kPackThreads), 0, (hipStream_t)stream, in, d_desc, out_desc, bits,
                       lim_desc, lim_bits);
  return launch_status(hipGetLastError());
}

}  // namespace clg
