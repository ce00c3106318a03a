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
#include "pack_dev.h"
#include "kernels.h"

namespace clg {

namespace {

static_assert(kWPackTile == kPackThreads * kPackPerThread, "a tile is four rows a thread");
static_assert(sizeof(WPackTab::col) / sizeof(void*) == kWPackStreams, "WPackTab holds the format's streams");
constexpr uint32_t kWPackParts = kPackPerThread * kPackWaves;  // (quarter, wave) pieces of a tile, in row order

// Lanes below this one whose bit is set in m.
__device__ __forceinline__ uint32_t wpack_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

// The stream that holds block blk: the last one whose base is at or below it.
__device__ __forceinline__ uint32_t wpack_stream_of(const WPackTab* __restrict__ tab, uint64_t blk) {
  uint32_t s = 0;
#pragma unroll
  for (uint32_t c = 1; c < kWPackStreams; ++c) s += uint32_t(blk >= tab->blk_base[c]);
  return s;
}
__device__ __forceinline__ PackAt wpack_at(const WPackTab* __restrict__ tab, uint32_t s, uint64_t blk) {
  const uint64_t n = tab->n[s], i0 = (blk - tab->blk_base[s]) * kPackBlock;
  const uint64_t left = i0 < n ? n - i0 : 0;
  return PackAt{tab->col[s], i0, uint32_t(left < kPackBlock ? left : kPackBlock)};
}
#define CLG_WPACK_CASE(body, e, d, at, ...) \
  case (e) * 2 + (d): body<e, d != 0>(at, __VA_ARGS__); break;
#define CLG_WPACK_DISPATCH(s, body, at, ...)                                  \
  switch (wpack_stream_elem(s) * 2 + uint32_t(wpack_is_delta(s))) {           \
    CLG_WPACK_CASE(body, kElemU8, 0, at, __VA_ARGS__)                         \
    CLG_WPACK_CASE(body, kElemU8, 1, at, __VA_ARGS__)                         \
    CLG_WPACK_CASE(body, kElemU32, 0, at, __VA_ARGS__)                        \
    CLG_WPACK_CASE(body, kElemU32, 1, at, __VA_ARGS__)                        \
    CLG_WPACK_CASE(body, kElemI32, 0, at, __VA_ARGS__)                        \
    CLG_WPACK_CASE(body, kElemI32, 1, at, __VA_ARGS__)                        \
    CLG_WPACK_CASE(body, kElemI64, 0, at, __VA_ARGS__)                        \
    CLG_WPACK_CASE(body, kElemI64, 1, at, __VA_ARGS__)                        \
  }

}  // namespace

__global__ __launch_bounds__(kPackThreads) void k_wpack_kind(const WPackSrc src, uint8_t* __restrict__ kind_out,
                                                            uint32_t* __restrict__ cnt, unsigned long long* __restrict__ bad) {
  __shared__ uint32_t s_cnt[kPackWaves][kWPackKinds];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t c[kWPackKinds] = {};  // (the wave's counts: the same in every lane)
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint64_t k = uint64_t(blockIdx.x) * kWPackTile + q * kPackThreads + tid;
    uint32_t kind = kWPackKinds;
    if (k < src.n_wide) {
      kind = wpack_kind_of(src.tag, src.n_rec, src.w_idx[k]);
      if (kind >= kWPackKinds) atomicMin(bad, (unsigned long long)k);
      kind_out[k] = uint8_t(kind);  // (kWPackKinds: the split passes the row by; the host rejects the call)
    }
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) c[t] += uint32_t(__popcll(__ballot(kind == t)));
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) s_cnt[w][t] = c[t];
  }
  __syncthreads();
  if (tid < kWPackKinds) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPackWaves; ++j) s += s_cnt[j][tid];
    cnt[uint64_t(blockIdx.x) * kWPackKinds + tid] = s;
  }
}

// The tile counts -> d_base, the rows of each kind before the tile; the totals and the bad-row
// word -> *res.  One workgroup, a tile a thread and round: no look-back.
__global__ __launch_bounds__(kPackTopThreads) void k_wpack_scan(const uint32_t* __restrict__ cnt, uint32_t n_tiles,
                                                               uint64_t* __restrict__ base,
                                                               const unsigned long long* __restrict__ bad,
                                                               WPackRes* __restrict__ res) {
  __shared__ uint64_t ws[kPackTopThreads / 64];
  __shared__ uint64_t wtot;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  for (uint32_t t = 0; t < kWPackKinds; ++t) {
    uint64_t carry = 0;
    for (uint32_t g0 = 0; g0 < n_tiles; g0 += kPackTopThreads) {
      const uint32_t g = g0 + tid;
      const uint64_t before = pack_scan_round(g < n_tiles ? cnt[uint64_t(g) * kWPackKinds + t] : 0, lane, ws, &wtot);
      if (g < n_tiles) base[uint64_t(g) * kWPackKinds + t] = carry + before;
      carry += wtot;
      __syncthreads();  // (ws is written again in the next round)
    }
    if (tid == 0) res->tot[t] = carry;
  }
  if (tid == 0) res->bad_row = *bad;
}

__global__ __launch_bounds__(kPackThreads) void k_wpack_split(const WPackSrc src, const uint8_t* __restrict__ kind_in,
                                                             const uint64_t* __restrict__ base,
                                                             const WPackTab* __restrict__ tab) {
  __shared__ uint32_t s_pre[kWPackParts][kWPackKinds];  // a piece's counts, then the rows of the tile before it
  __shared__ uint64_t s_col[kWPackKinds * kWPackFields];
  __shared__ uint64_t s_n[kWPackKinds], s_base[kWPackKinds];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < kWPackKinds * kWPackFields) s_col[tid] = uint64_t(reinterpret_cast<uintptr_t>(tab->col[2 + tid]));
  if (tid < kWPackKinds) {
    s_n[tid] = tab->n[wpack_stream(tid, 0)];
    s_base[tid] = base[uint64_t(blockIdx.x) * kWPackKinds + tid];
  }
  uint32_t kind[kPackPerThread], below[kPackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint64_t k = uint64_t(blockIdx.x) * kWPackTile + q * kPackThreads + tid;
    kind[q] = k < src.n_wide ? uint32_t(kind_in[k]) : kWPackKinds;
    below[q] = 0;
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) {
      const uint64_t m = __ballot(kind[q] == t);
      if (kind[q] == t) below[q] = wpack_below(m);
      if (lane == 0) s_pre[q * kPackWaves + w][t] = uint32_t(__popcll(m));
    }
  }
  __syncthreads();
  if (tid < kWPackKinds) {
    uint32_t run = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWPackParts; ++j) {
      const uint32_t x = s_pre[j][tid];
      s_pre[j][tid] = run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t t = kind[q];
    if (t >= kWPackKinds) continue;
    const uint64_t k = uint64_t(blockIdx.x) * kWPackTile + q * kPackThreads + tid;
    const uint64_t r = s_base[t] + s_pre[q * kPackWaves + w][t] + below[q];
    if (r >= s_n[t]) continue;  // (never, while the kind bytes are what pass 1 counted)
    const uint64_t* col = &s_col[t * kWPackFields];
    reinterpret_cast<int32_t*>(uintptr_t(col[CLG_WPACK_RC]))[r] = src.w_rc[k];
    reinterpret_cast<int64_t*>(uintptr_t(col[CLG_WPACK_V1]))[r] = src.w_v1[k];
    reinterpret_cast<uint32_t*>(uintptr_t(col[CLG_WPACK_VAR_OFF]))[r] = src.w_var_off[k];
    reinterpret_cast<uint32_t*>(uintptr_t(col[CLG_WPACK_VAR_LEN]))[r] = src.w_var_len[k];
    reinterpret_cast<uint8_t*>(uintptr_t(col[CLG_WPACK_SUB]))[r] = src.w_sub[k];
    reinterpret_cast<int64_t*>(uintptr_t(col[CLG_WPACK_V0]))[r] = src.w_v0[k];
  }
}

__global__ __launch_bounds__(kPackThreads) void k_wpack_measure(const WPackTab* __restrict__ tab,
                                                               clg_pack_block* __restrict__ desc) {
  __shared__ int64_t s_x[kPackBlock];  // the block's values: the DELTA predecessors
  __shared__ int64_t s_lo[kPackWaves], s_hi[kPackWaves];
  const uint32_t s = wpack_stream_of(tab, blockIdx.x);
  const PackAt at = wpack_at(tab, s, blockIdx.x);
  CLG_WPACK_DISPATCH(s, pack_block_measure, at, desc, s_x, s_lo, s_hi)
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
