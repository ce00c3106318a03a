// pack_wide.hip -- packed wide rows (pack_wide.h): the seven w_* arrays partitioned by record kind
// and bit-packed block by block, so that a stream holds one kind of number.
//
//  * k_wpack_kind     pass 1: a workgroup per tile of kWPackTile rows.  A thread loads w_idx,
//                     checks it against n_rec, loads the tag and writes the kind byte to engine
//                     scratch; the tile's four kind counts by ballot per wave and LDS across the
//                     waves.  A bad row (and only a bad row) issues one vector atomicMin
//  * k_wpack_scan     pass 2: ONE workgroup scans the tile counts into per-kind tile bases; the
//                     four totals and the bad-row word go to pinned memory, from which the host
//                     lays the 26 streams out (WPackTab) after one sync
//  * k_wpack_split    pass 3: a workgroup per tile; a row's rank is its tile's base for its kind
//                     plus its rank inside the tile (ballot and mbcnt in the wave, LDS across the
//                     waves and the four quarters); the six fields go to per-kind arrays
//  * k_wpack_measure  pass 4a: the block codec's measure (pack_dev.h) over the 26 streams; then
//                     pack.hip's three scan kernels, unchanged
//  * k_wpack_write    pass 4b: the block codec's write over the 26 streams
//
// Measure and write are instantiated on (element, scheme), as pack.hip instantiates them; a
// block's stream is found from the table's blk_base wave-uniformly.  Kernel boundaries order the passes.  No spin waits, no word
// taken from another running workgroup, no scratch; LDS atomics only inside a workgroup.  The
// result is a pure function of the rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "pack_wide.h"
#include "pack_wide_dev.h"
#include "kernels.h"

namespace clg {

namespace {

static_assert(sizeof(WPackTab::col) / sizeof(void*) == kWPackStreams, "WPackTab holds the format's streams");

__device__ __forceinline__ PackAt wpack_at(const WPackTab* __restrict__ tab, uint32_t s, uint64_t blk) {
  const uint64_t n = tab->n[s], i0 = (blk - tab->blk_base[s]) * kPackBlock;
  const uint64_t left = i0 < n ? n - i0 : 0;
  return PackAt{tab->col[s], i0, uint32_t(left < kPackBlock ? left : kPackBlock)};
}

}  // namespace

__global__ __launch_bounds__(kPackThreads) void k_wpack_kind(const WPackSrc src, uint8_t* __restrict__ kind_out,
                                                            uint32_t* __restrict__ cnt, unsigned long long* __restrict__ bad) {
  uint32_t kind[kPackPerThread];
  const uint64_t mine = wpack_row_kinds(src, blockIdx.x, kind_out, kind);
  if (mine != ~0ull) atomicMin(bad, (unsigned long long)mine);
  wpack_kind_counts(kind, cnt, blockIdx.x);
}

// The tile counts -> d_base, the rows of each kind before the tile; the totals and the bad-row
// word -> *res.  One workgroup: wave_dev.h's scan, the four kinds at once.
__global__ __launch_bounds__(kPackTopThreads) void k_wpack_scan(const uint32_t* __restrict__ cnt, uint32_t n_tiles,
                                                               uint64_t* __restrict__ base,
                                                               const unsigned long long* __restrict__ bad,
                                                               WPackRes* __restrict__ res) {
  const auto tot = wpack_kind_scan(cnt, n_tiles, base);
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) res->tot[t] = tot.v[t];
    res->bad_row = *bad;
  }
}

__global__ __launch_bounds__(kPackThreads) void k_wpack_split(const WPackSrc src, const uint8_t* __restrict__ kind_in,
                                                             const uint64_t* __restrict__ base,
                                                             const WPackTab* __restrict__ tab) {
  __shared__ WPackTileLds l;
  uint32_t kind[kPackPerThread];
  uint64_t r[kPackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint64_t k = uint64_t(blockIdx.x) * kWPackTile + q * kPackThreads + threadIdx.x;
    kind[q] = k < src.n_wide ? uint32_t(kind_in[k]) : kWPackKinds;
  }
  wpack_tile_rank(tab, base, blockIdx.x, kind, l, r);
  wpack_split_rows(src, blockIdx.x, kind, r, l);
}

__global__ __launch_bounds__(kPackThreads) void k_wpack_measure(const WPackTab* __restrict__ tab,
                                                               clg_pack_block* __restrict__ desc) {
  __shared__ int64_t s_x[kPackBlock];  // the block's values: the DELTA predecessors
  __shared__ int64_t s_lo[kPackWaves], s_hi[kPackWaves];
  const uint32_t s = wpack_stream_of(tab, blockIdx.x);
  const PackAt at = wpack_at(tab, s, blockIdx.x);
  CLG_WPACK_DISPATCH(s, pack_block_measure, at, desc + blockIdx.x, s_x, s_lo, s_hi)
}

__global__ __launch_bounds__(kPackThreads) void k_wpack_write(const WPackTab* __restrict__ tab,
                                                             const clg_pack_block* __restrict__ desc,
                                                             clg_pack_block* __restrict__ out_desc,
                                                             uint8_t* __restrict__ bits, uint64_t lim_desc,
                                                             uint64_t lim_bits) {
  __shared__ unsigned long long s_w[kPackBlock];
  const clg_pack_block d = desc[blockIdx.x];  // (uniform)
  if (threadIdx.x == 0 && blockIdx.x < lim_desc) out_desc[blockIdx.x] = d;
  const uint32_t s = wpack_stream_of(tab, blockIdx.x);
  const PackAt at = wpack_at(tab, s, blockIdx.x);
  CLG_WPACK_DISPATCH(s, pack_block_write, at, d, s_w, bits, lim_bits)
}

int launch_wpack_count_scan(const WPackSrc& src, uint32_t n_tiles, uint8_t* d_kind, uint32_t* d_cnt, uint64_t* d_base,
                            unsigned long long* d_bad, WPackRes* res, void* stream) {
  if (hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
    return launch_status(hipGetLastError());
  if (n_tiles)
    hipLaunchKernelGGL(k_wpack_kind, dim3(n_tiles), dim3(kPackThreads), 0, (hipStream_t)stream, src, d_kind, d_cnt, d_bad);
  hipLaunchKernelGGL(k_wpack_scan, dim3(1), dim3(kPackTopThreads), 0, (hipStream_t)stream, d_cnt, n_tiles, d_base, d_bad, res);
  return launch_status(hipGetLastError());
}

int launch_wpack_split_measure(const WPackSrc& src, uint32_t n_tiles, const uint8_t* d_kind, const uint64_t* d_base,
                               const WPackTab* d_tab, uint32_t n_blocks, clg_pack_block* d_desc, void* stream) {
  if (n_tiles)
    hipLaunchKernelGGL(k_wpack_split, dim3(n_tiles), dim3(kPackThreads), 0, (hipStream_t)stream, src, d_kind, d_base, d_tab);
  if (n_blocks) hipLaunchKernelGGL(k_wpack_measure, dim3(n_blocks), dim3(kPackThreads), 0, (hipStream_t)stream, d_tab, d_desc);
  return launch_status(hipGetLastError());
}

int launch_wpack_write(const WPackTab* d_tab, uint32_t n_blocks, const clg_pack_block* d_desc, clg_pack_block* out_desc,
                       uint8_t* bits, uint64_t lim_desc, uint64_t lim_bits, void* stream) {
  if (n_blocks)
    hipLaunchKernelGGL(k_wpack_write, dim3(n_blocks), dim3(kPackThreads), 0, (hipStream_t)stream, d_tab, d_desc, out_desc, bits,
                       lim_desc, lim_bits);
  return launch_status(hipGetLastError());
}

}  // namespace clg
