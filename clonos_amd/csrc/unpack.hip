// unpack.hip -- packed typed columns as input (pack.h): the five narrow columns unpacked where the
// packed bytes lie, so that a packed batch that crossed the link narrow becomes plain columns in
// HBM without a host pass.
//
//  * k_unpack_check   pass 1: a wave per block, all five streams in one grid.  The block check
//                     (pack_block_in_ok) on the block's descriptor; then, only for a stream
//                     narrower than 64 bits whose [ref, ref + 2^width - 1] does not already lie
//                     inside the type, every value of the payload.  No address is formed from a
//                     descriptor that failed the block check.  A bad block raises the verdict word
//                     of its kind to ~index with one vector atomicMax (the host zeroes the words
//                     through the stream; a clean input issues no atomic at all)
//  * k_unpack_write   pass 2, queued by the host only after it has read a clean verdict: a
//                     workgroup per block stages the payload (at most 8 KiB) in LDS with aligned
//                     16-byte loads, each thread extracts four consecutive values, FOR adds ref,
//                     DELTA takes the inclusive prefix sum of first and the residuals (the
//                     thread's four, pack_dev.h's wave scan, the four waves through LDS), and
//                     stores them coalesced
//
// Kernel boundaries order the passes.  No spin waits, no word taken from another running
// workgroup, no scratch; LDS is private to a workgroup.  The output is a pure function of the
// packed bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "pack.h"
#include "pack_dev.h"
#include "kernels.h"

namespace clg {

namespace {

constexpr uint32_t kUnpackThreads = 256;
constexpr uint32_t kUnpackWaves = kUnpackThreads / 64;
constexpr uint32_t kUnpackPerThread = kPackBlock / kUnpackThreads;
static_assert(kUnpackPerThread == 4, "four consecutive values a thread");

// The stream that holds block blk (the bases do not decrease: the host's layout check).
__device__ __forceinline__ uint32_t unpack_stream_of(const UnpackIn& in, uint64_t blk) {
  return uint32_t(blk >= in.blk_base[1]) + uint32_t(blk >= in.blk_base[2]) + uint32_t(blk >= in.blk_base[3]) +
         uint32_t(blk >= in.blk_base[4]);
}

// Residual j's p from 64-bit words, 1 <= w <= 63: no shift by 64 (sh + w > 64 implies sh > 0), and
// the second word is read only when the value reaches into it, so never past the payload.
__device__ __forceinline__ uint64_t unpack_bits(const unsigned long long* words, uint32_t w, uint32_t j) {
  const uint32_t bit = j * w, sh = bit & 63;
  uint64_t v = words[bit >> 6] >> sh;
  if (sh + w > 64) v |= uint64_t(words[(bit >> 6) + 1]) << (64 - sh);
  return v & ((uint64_t(1) << w) - 1);
}

// Every value of a well-formed block of stream kC (narrower than 64 bits) inside its type?  The
// wave's lanes take the values 64 apart; the payload is read from global memory in place.
template <uint32_t kC>
__device__ __forceinline__ bool unpack_values_ok(const clg_pack_block& d, const uint8_t* __restrict__ bits, uint32_t lane) {
  const unsigned long long* words = reinterpret_cast<const unsigned long long*>(bits + d.pos);
  const uint32_t w = d.width;
  bool ok = true;
  for (uint32_t i = lane; i < d.count; i += 64) {
    const uint64_t p = w == 0 ? 0 : w == 64 ? uint64_t(words[i]) : unpack_bits(words, w, i);
    ok = ok && pack_value_ok(kC, int64_t(p + uint64_t(d.ref)));
  }
  return __ballot(!ok) == 0;
}

// Four consecutive values to dst[0 .. n) (n <= 4) in the stream's element type: one store of
// four elements where all four are there and the column allows it, else an element at a time.
template <uint32_t kC>
__device__ __forceinline__ void unpack_store4(void* col, uint64_t at, const uint64_t v[4], uint32_t n, bool wide) {
  if (kC == CLG_PACK_TIMESTAMP) {
    int64_t* dst = static_cast<int64_t*>(col) + at;
    if (n == 4 && wide) {
      reinterpret_cast<ulonglong2*>(dst)[0] = make_ulonglong2(v[0], v[1]);
      reinterpret_cast<ulonglong2*>(dst)[1] = make_ulonglong2(v[2], v[3]);
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
        if (q < n) dst[q] = int64_t(v[q]);
    }
  } else if (kC >= CLG_PACK_RNG) {
    int32_t* dst = static_cast<int32_t*>(col) + at;
    if (n == 4 && wide) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3]));
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
        if (q < n) dst[q] = int32_t(uint32_t(v[q]));
    }
  } else {
    uint8_t* dst = static_cast<uint8_t*>(col) + at;
    if (n == 4 && wide) {
      *reinterpret_cast<uint32_t*>(dst) = uint32_t(v[0] & 255) | uint32_t(v[1] & 255) << 8 | uint32_t(v[2] & 255) << 16 |
                                          uint32_t(v[3] & 255) << 24;
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
        if (q < n) dst[q] = uint8_t(v[q]);
    }
  }
}

// s_w: the payload's words (8 KiB and one spare pair); s_ws: the waves' sums.
template <uint32_t kC>
__device__ __forceinline__ void unpack_write_body(void* col, uint64_t i0, const clg_pack_block d,
                                                  const uint8_t* __restrict__ bits, unsigned long long* s_w,
                                                  unsigned long long* s_ws) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr bool delta = kC == CLG_PACK_TIMESTAMP;
  const uint32_t m = d.count, k = pack_resid(kC, m), width = d.width;
  const uint32_t n16 = pack_payload_bytes(k, width) / 16;
  // the payload into LDS: aligned 16-byte loads (bits is 16-byte aligned, pos a multiple of 16)
  const uint4* src = reinterpret_cast<const uint4*>(bits + d.pos);
  for (uint32_t i = tid; i < n16; i += kUnpackThreads) reinterpret_cast<uint4*>(s_w)[i] = src[i];
  if (n16) __syncthreads();  // (uniform)

  const uint32_t first_i = tid * kUnpackPerThread;
  uint64_t v[kUnpackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kUnpackPerThread; ++q) {
    const uint32_t i = first_i + q;
    // the residual's index: FOR i, DELTA i - 1 (value 0 is `first`)
    const bool has = delta ? (i >= 1 && i < m) : i < m;
    const uint32_t j = delta ? i - 1 : i;
    uint64_t p = 0;
    if (has) {
      if (width == 64) p = s_w[j];  // (the widths 0 and 64 are uniform cases: no shifts)
      else if (width) p = unpack_bits(s_w, width, j);
      p += uint64_t(d.ref);
    }
    v[q] = delta && i == 0 ? uint64_t(d.first) : p;
  }
  if (delta) {  // the inclusive prefix sum, modulo 2^64: the thread's four, the wave, the four waves
    v[1] += v[0], v[2] += v[1], v[3] += v[2];
    const uint64_t incl = pack_wave_incl64(v[3], lane);
    if (lane == 63) s_ws[wv] = incl;
    __syncthreads();
    uint64_t before = incl - v[3];
#pragma unroll
    for (uint32_t w2 = 0; w2 < kUnpackWaves; ++w2) before += w2 < wv ? uint64_t(s_ws[w2]) : 0;
#pragma unroll
    for (uint32_t q = 0; q < kUnpackPerThread; ++q) v[q] += before;
  }
  const uint32_t n = first_i < m ? (m - first_i < 4 ? m - first_i : 4) : 0;
  constexpr uint32_t kWide = kC == CLG_PACK_TIMESTAMP || kC >= CLG_PACK_RNG ? 16 : 4;
  const bool wide = (reinterpret_cast<uintptr_t>(col) & (kWide - 1)) == 0;  // (uniform; i0 keeps the alignment)
  if (n) unpack_store4<kC>(col, i0 + first_i, v, n, wide);
}

}  // namespace

__global__ __launch_bounds__(kUnpackThreads) void k_unpack_check(const UnpackIn in, uint32_t n_blocks,
                                                                UnpackVerdict* __restrict__ verdict) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = uint64_t(blockIdx.x) * kUnpackWaves + (threadIdx.x >> 6);  // (wave-uniform)
  if (blk >= n_blocks) return;
  const uint32_t c = unpack_stream_of(in, blk);
  const clg_pack_block d = in.desc[blk];
  bool block_ok = false, values_ok = true;
  switch (c) {  // wave-uniform: the stream is a constant in each body
    case 0:
      block_ok = pack_block_in_ok(d, pack_is_delta(0), blk - in.blk_base[0], in.n[0], in.n_bits);
      if (block_ok && !pack_range_inside(0, d.ref, d.width)) values_ok = unpack_values_ok<0>(d, in.bits, lane);
      break;
    case 1:
      block_ok = pack_block_in_ok(d, pack_is_delta(1), blk - in.blk_base[1], in.n[1], in.n_bits);
      if (block_ok && !pack_range_inside(1, d.ref, d.width)) values_ok = unpack_values_ok<1>(d, in.bits, lane);
      break;
    case 2: block_ok = pack_block_in_ok(d, pack_is_delta(2), blk - in.blk_base[2], in.n[2], in.n_bits); break;  // 64 bits: every value passes
    case 3:
      block_ok = pack_block_in_ok(d, pack_is_delta(3), blk - in.blk_base[3], in.n[3], in.n_bits);
      if (block_ok && !pack_range_inside(3, d.ref, d.width)) values_ok = unpack_values_ok<3>(d, in.bits, lane);
      break;
    default:
      block_ok = pack_block_in_ok(d, pack_is_delta(4), blk - in.blk_base[4], in.n[4], in.n_bits);
      if (block_ok && !pack_range_inside(4, d.ref, d.width)) values_ok = unpack_values_ok<4>(d, in.bits, lane);
      break;
  }
  if (lane == 0) {
    if (!block_ok) atomicMax(&verdict->bad_block, ~(unsigned long long)blk);
    else if (!values_ok) atomicMax(&verdict->bad_value, ~(unsigned long long)blk);
  }
}

__global__ __launch_bounds__(kUnpackThreads) void k_unpack_write(const UnpackIn in, const UnpackOut out) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_w[kPackBlock + 2];
  __shared__ unsigned long long s_ws[kUnpackWaves];
  const uint64_t blk = blockIdx.x;
  const clg_pack_block d = in.desc[blk];  // (uniform)
  switch (unpack_stream_of(in, blk)) {
#define CLG_UNPACK_CASE(c)                                                                             \
  if (pack_block_in_ok(d, pack_is_delta(c), blk - in.blk_base[c], in.n[c], in.n_bits))                                \
    unpack_write_body<c>(out.col[c], (blk - in.blk_base[c]) * kPackBlock, d, in.bits, s_w, s_ws);      \
  break
    case 0: CLG_UNPACK_CASE(0);
    case 1: CLG_UNPACK_CASE(1);
    case 2: CLG_UNPACK_CASE(2);
    case 3: CLG_UNPACK_CASE(3);
    default: CLG_UNPACK_CASE(4);
#undef CLG_UNPACK_CASE
  }
}

int launch_unpack_check(const UnpackIn& in, uint32_t n_blocks, UnpackVerdict* d_verdict, void* stream) {
  if (hipMemsetAsync(d_verdict, 0, sizeof(UnpackVerdict), (hipStream_t)stream) != hipSuccess)
    return launch_status(hipGetLastError());
  if (n_blocks)
    hipLaunchKernelGGL(k_unpack_check, dim3((n_blocks + kUnpackWaves - 1) / kUnpackWaves), dim3(kUnpackThreads), 0,
                       (hipStream_t)stream, in, n_blocks, d_verdict);
  return launch_status(hipGetLastError());
}

int launch_unpack_write(const UnpackIn& in, const UnpackOut& out, uint32_t n_blocks, void* stream) {
  if (n_blocks)
    hipLaunchKernelGGL(k_unpack_write, dim3(n_blocks), dim3(kUnpackThreads), 0, (hipStream_t)stream, in, out);
  return launch_status(hipGetLastError());
}

}  // namespace clg
