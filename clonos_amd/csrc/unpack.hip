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
//                     workgroup per block (pack_dev.h's decode, instantiated on the stream's
//                     element and scheme) stages the payload (at most 8 KiB) in LDS with aligned
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

constexpr uint32_t kUnpackThreads = kPackThreads;
constexpr uint32_t kUnpackWaves = kPackWaves;

// The stream that holds block blk (the bases do not decrease: the host's layout check).
__device__ __forceinline__ uint32_t unpack_stream_of(const UnpackIn& in, uint64_t blk) {
  return uint32_t(blk >= in.blk_base[1]) + uint32_t(blk >= in.blk_base[2]) + uint32_t(blk >= in.blk_base[3]) +
         uint32_t(blk >= in.blk_base[4]);
}

// Every value of a well-formed block of stream kC (FOR, narrower than 64 bits) inside its type?  The
// wave's lanes take the values 64 apart; the payload is read from global memory in place.
template <uint32_t kC>
__device__ __forceinline__ bool unpack_values_ok(const clg_pack_block& d, const uint8_t* __restrict__ bits, uint32_t lane) {
  static_assert(!pack_is_delta(kC), "the narrow DELTA stream holds 64-bit values: every one passes");
  const unsigned long long* words = reinterpret_cast<const unsigned long long*>(bits + d.pos);
  bool ok = true;
  for (uint32_t i = lane; i < d.count; i += 64)
    ok = ok && pack_value_ok(kC, int64_t(unpack_resid(words, d.width, i) + uint64_t(d.ref)));
  return __ballot(!ok) == 0;
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
    unpack_block_write<pack_stream_elem(c), pack_is_delta(c)>(out.col[c], (blk - in.blk_base[c]) * kPackBlock, d, \
                                                              in.bits, s_w, s_ws);                     \
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
