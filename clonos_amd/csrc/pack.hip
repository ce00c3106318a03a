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
// Measure and write are pack_dev.h's block codec, instantiated with kPackStream's (element,
// scheme) of each stream.  Kernel boundaries order the passes.  No global atomics, no spin waits, no word taken from
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
// pack_dev.h's bodies are instantiated per stream (the element and the scheme are kPackStream's
// constants) and the argument arrays are only ever indexed by constants.
#define CLG_PACK_CASE(c, in, blk, body, ...) \
  body<pack_stream_elem(c), pack_is_delta(c)>(pack_at(in.col[c], in.n[c], in.blk_base[c], blk), __VA_ARGS__); break;
#define CLG_PACK_DISPATCH(in, blk, body, ...)              \
  switch (pack_stream_of(in, blk)) {                       \
    case 0: CLG_PACK_CASE(0, in, blk, body, __VA_ARGS__)   \
    case 1: CLG_PACK_CASE(1, in, blk, body, __VA_ARGS__)   \
    case 2: CLG_PACK_CASE(2, in, blk, body, __VA_ARGS__)   \
    case 3: CLG_PACK_CASE(3, in, blk, body, __VA_ARGS__)   \
    default: CLG_PACK_CASE(4, in, blk, body, __VA_ARGS__)  \
  }

}  // namespace

__global__ __launch_bounds__(kPackThreads) void k_pack_measure(const PackIn in, clg_pack_block* __restrict__ desc) {
  __shared__ int64_t s_x[kPackBlock];  // the block's values: the DELTA predecessors
  __shared__ int64_t s_lo[kPackWaves], s_hi[kPackWaves];
  CLG_PACK_DISPATCH(in, blockIdx.x, pack_block_measure, desc + blockIdx.x, s_x, s_lo, s_hi)
}

__global__ __launch_bounds__(kPackThreads) void k_pack_scan_sums(const clg_pack_block* __restrict__ desc, uint32_t n_blocks,
                                                                uint64_t* __restrict__ gsum) {
  __shared__ uint32_t ws[kPackWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t b = uint64_t(blockIdx.x) * kPackScanGroup + tid;
  const uint32_t x = b < n_blocks ? uint32_t(desc[b].pos) : 0u;  // (at most 8 KiB a block)
  const uint32_t s = wave_incl(x, lane);
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
  const auto tot = tile_scan<kPackTopThreads, 1, uint64_t>(
      n_groups, [&](uint32_t g, uint64_t c[1]) { c[0] = gsum[g]; },
      [&](uint32_t g, const uint64_t before[1]) { gsum[g] = before[0]; });
  if (threadIdx.x == 0) res->n_bits = tot.v[0];
}

__global__ __launch_bounds__(kPackThreads) void k_pack_scan_apply(clg_pack_block* __restrict__ desc, uint32_t n_blocks,
                                                                 const uint64_t* __restrict__ gsum) {
  __shared__ uint32_t ws[kPackWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t b = uint64_t(blockIdx.x) * kPackScanGroup + tid;
  const uint32_t x = b < n_blocks ? uint32_t(desc[b].pos) : 0u;
  const uint32_t inc = wave_incl(x, lane);
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
  CLG_PACK_DISPATCH(in, blockIdx.x, pack_block_write, d, s_w, bits, lim_bits)
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
