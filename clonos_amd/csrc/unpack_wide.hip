// unpack_wide.hip -- packed wide rows as input (pack_wide.h): the 26 streams checked and unpacked
// where the packed bytes lie and the rows put back in row order, so that a clg_packed_wide that
// crossed the link narrow becomes the seven w_* arrays (and the payload column's pos) in HBM
// without a host pass.  The mirror of pack_wide.hip's passes.
//
//  * k_wunpack_check  pass 1a: a wave per block, all 26 streams.  The block check on the block's
//                     descriptor; then every value, but only where the descriptor alone does not
//                     already hold them inside the type: a FOR block whose [ref, ref + 2^width - 1]
//                     lies inside it, a DELTA block that cannot decrease and whose largest possible
//                     last value lies inside it, and every 64-bit stream pass unread.  KIND's bound
//                     is 3.  A bad block raises its verdict word to ~index with one vector atomicMax
//  * k_wunpack_kind   pass 1b: a workgroup per KIND block, a tile of kWPackTile rows.  The block
//                     check again (no address is formed from a descriptor that failed), the
//                     kinds to a byte array in engine scratch, the tile's four counts by ballot
//                     per wave and LDS across the waves.  A value above 3 is counted nowhere
//  * k_wunpack_scan   pass 1c: ONE workgroup scans the tile counts into per-kind tile bases; the
//                     four totals go to pinned memory.  The host reads the verdict and the totals
//                     after one sync; nothing has been written outside engine scratch
//  * k_wunpack_write  pass 2: a workgroup per block of streams 1 .. 25, pack_dev.h's decode
//                     instantiated on (element, scheme): IDX to w_idx, the 24 field streams to
//                     per-kind arrays in engine scratch
//  * k_wunpack_merge  pass 3: a workgroup per tile; a row's rank is its tile's base for its kind
//                     plus its rank inside the tile (ballot and mbcnt in the wave, LDS across the
//                     waves and the four quarters, as k_wpack_split); the six fields are gathered
//                     from the kind's arrays at that rank, clamped below the kind's length, and
//                     stored in row order; the tile's sum of w_var_len; with the tags (the
//                     combined calls), the cross rule's word by one vector atomicMin a bad row
//  * k_wunpack_tscan, k_wunpack_pos   pass 4, only when pos is wanted: one workgroup scans the
//                     tile sums, then a workgroup per tile writes pos[k] and pos[n_wide]
//
// Kernel boundaries order the passes.  No spin waits, no word taken from another running
// workgroup, no scratch; LDS atomics: none.  The output is a pure function of the packed bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "pack_wide.h"
#include "pack_wide_dev.h"
#include "kernels.h"

namespace clg {

namespace {

static_assert(sizeof(WUnpackTab::col) / sizeof(void*) == kWPackStreams, "WUnpackTab holds the format's streams");

__device__ __forceinline__ bool wunpack_block_ok(const WUnpackTab* __restrict__ tab, uint32_t s, uint64_t blk,
                                                 const clg_pack_block& d) {
  return pack_block_in_ok(d, wpack_is_delta(s), blk - tab->blk_base[s], tab->n[s], tab->n_bits);
}
// Does the descriptor alone hold every value of a well-formed block inside [lo, hi] (both inside
// 33 bits)?  FOR: [ref, ref + 2^width - 1] inside it.  DELTA: first inside it, no residual below
// zero, and first plus count - 1 largest residuals at most hi (below 2^44: no overflow).
__device__ __forceinline__ bool wunpack_range_inside(const clg_pack_block& d, bool delta, int64_t lo, int64_t hi) {
  if (d.width > 32 || d.ref > hi) return false;
  const int64_t top = d.ref + int64_t((uint64_t(1) << d.width) - 1);
  if (!delta) return d.ref >= lo && top <= hi;
  return d.ref >= 0 && d.first >= lo && d.first <= hi && d.first + int64_t(d.count - 1) * top <= hi;
}

}  // namespace

__global__ __launch_bounds__(kPackThreads) void k_wunpack_check(const WUnpackTab* __restrict__ tab, uint32_t n_blocks,
                                                               WUnpackVerdict* __restrict__ verdict) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = uint64_t(blockIdx.x) * kPackWaves + (threadIdx.x >> 6);  // (wave-uniform)
  if (blk >= n_blocks) return;
  const uint32_t s = wpack_stream_of(tab, blk);
  const clg_pack_block d = tab->desc[blk];
  const bool delta = wpack_is_delta(s);
  const bool block_ok = wunpack_block_ok(tab, s, blk, d);
  bool values_ok = true;
  const uint32_t elem = wpack_stream_elem(s);
  if (block_ok && elem != kElemI64) {
    const int64_t lo = pack_elem_lo(elem), hi = s == CLG_WPACK_KIND ? int64_t(kWPackKinds - 1) : pack_elem_hi(elem);
    if (!wunpack_range_inside(d, delta, lo, hi))
      values_ok = delta ? unpack_values_in<true>(d, tab->bits, lane, lo, hi) : unpack_values_in<false>(d, tab->bits, lane, lo, hi);
  }
  if (lane == 0) {
    if (!block_ok) atomicMax(&verdict->bad_block, ~(unsigned long long)blk);
    else if (!values_ok) atomicMax(&verdict->bad_value, ~(unsigned long long)blk);
  }
}

__global__ __launch_bounds__(kPackThreads) void k_wunpack_kind(const WUnpackTab* __restrict__ tab, uint32_t* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_w[kPackBlock + 2];
  __shared__ unsigned long long s_ws[kPackWaves];
  const clg_pack_block d = tab->desc[blockIdx.x];  // (uniform; KIND's blocks are the first: blk_base[0] == 0)
  uint32_t kind[kPackPerThread] = {kWPackKinds, kWPackKinds, kWPackKinds, kWPackKinds};
  if (wunpack_block_ok(tab, CLG_WPACK_KIND, blockIdx.x, d)) {  // (uniform)
    uint64_t v[kPackPerThread];
    unpack_block_values<false>(d, tab->bits, s_w, s_ws, v);
    const uint32_t first_i = threadIdx.x * kPackPerThread, m = d.count;
    const uint32_t n = first_i < m ? (m - first_i < 4 ? m - first_i : 4) : 0;
    if (n) unpack_store4<kElemU8>(tab->col[CLG_WPACK_KIND], uint64_t(blockIdx.x) * kPackBlock + first_i, v, n, true);
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q)
      if (q < n && v[q] < kWPackKinds) kind[q] = uint32_t(v[q]);
  }
  wpack_kind_counts(kind, cnt, blockIdx.x);
}

// The tile counts -> base, the rows of each kind before the tile; the totals -> *res.  One
// workgroup: wave_dev.h's scan, the four kinds at once.
__global__ __launch_bounds__(kPackTopThreads) void k_wunpack_scan(const uint32_t* __restrict__ cnt, uint32_t n_tiles,
                                                                 uint64_t* __restrict__ base, WUnpackRes* __restrict__ res) {
  const auto tot = wpack_kind_scan(cnt, n_tiles, base);
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) res->tot[t] = tot.v[t];
  }
}

__global__ __launch_bounds__(kPackThreads) void k_wunpack_write(const WUnpackTab* __restrict__ tab, uint32_t first_blk) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_w[kPackBlock + 2];
  __shared__ unsigned long long s_ws[kPackWaves];
  const uint64_t blk = uint64_t(blockIdx.x) + first_blk;
  const uint32_t s = wpack_stream_of(tab, blk);  // (uniform)
  const clg_pack_block d = tab->desc[blk];
  if (!wunpack_block_ok(tab, s, blk, d)) return;  // (the input changed under the call: nothing is written)
  void* col = tab->col[s];
  const uint64_t i0 = (blk - tab->blk_base[s]) * kPackBlock;
  CLG_WPACK_DISPATCH(s, unpack_block_write, col, i0, d, tab->bits, s_w, s_ws)
}

__global__ __launch_bounds__(kPackThreads) void k_wunpack_merge(const WUnpackTab* __restrict__ tab,
                                                               const uint64_t* __restrict__ base, const WUnpackDst dst,
                                                               uint64_t n_wide, uint64_t* __restrict__ tsum,
                                                               WUnpackVerdict* __restrict__ verdict) {
  __shared__ WPackTileLds l;
  __shared__ uint64_t s_sum[kPackWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint8_t* __restrict__ kind_in = static_cast<const uint8_t*>(tab->col[CLG_WPACK_KIND]);
  uint32_t kind[kPackPerThread];
  uint64_t rank[kPackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint64_t k = uint64_t(blockIdx.x) * kWPackTile + q * kPackThreads + tid;
    kind[q] = k < n_wide ? uint32_t(kind_in[k]) : kWPackKinds;
  }
  wpack_tile_rank(tab, base, blockIdx.x, kind, l, rank);
  uint64_t len_sum = 0;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t t = kind[q];
    if (t >= kWPackKinds || l.n[t] == 0) continue;  // (the latter never, while the kind bytes are what pass 1 counted)
    const uint64_t k = uint64_t(blockIdx.x) * kWPackTile + q * kPackThreads + tid;
    const uint64_t r = rank[q] < l.n[t] ? rank[q] : l.n[t] - 1;  // (the clamp never, likewise: no load leaves the kind's array)
    const uint64_t* col = &l.col[t * kWPackFields];
    const uint32_t len = reinterpret_cast<const uint32_t*>(uintptr_t(col[CLG_WPACK_VAR_LEN]))[r];
    static_cast<int32_t*>(dst.col[CLG_WPACK_RC])[k] = reinterpret_cast<const int32_t*>(uintptr_t(col[CLG_WPACK_RC]))[r];
    static_cast<int64_t*>(dst.col[CLG_WPACK_V1])[k] = reinterpret_cast<const int64_t*>(uintptr_t(col[CLG_WPACK_V1]))[r];
    if (dst.col[CLG_WPACK_VAR_OFF])
      static_cast<uint32_t*>(dst.col[CLG_WPACK_VAR_OFF])[k] = reinterpret_cast<const uint32_t*>(uintptr_t(col[CLG_WPACK_VAR_OFF]))[r];
    static_cast<uint32_t*>(dst.col[CLG_WPACK_VAR_LEN])[k] = len;
    static_cast<uint8_t*>(dst.col[CLG_WPACK_SUB])[k] = reinterpret_cast<const uint8_t*>(uintptr_t(col[CLG_WPACK_SUB]))[r];
    static_cast<int64_t*>(dst.col[CLG_WPACK_V0])[k] = reinterpret_cast<const int64_t*>(uintptr_t(col[CLG_WPACK_V0]))[r];
    len_sum += len;
    if (dst.tag) {
      const uint32_t idx = static_cast<const uint32_t*>(tab->col[CLG_WPACK_IDX])[k];
      if (!wpack_cross_ok(dst.tag, dst.n_rec, idx, t)) atomicMin(&verdict->cross_row, (unsigned long long)k);
    }
  }
  const uint64_t incl = wave_incl(len_sum, lane);
  if (lane == 63) s_sum[w] = incl;
  __syncthreads();
  if (tid == 0) {
    uint64_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPackWaves; ++j) s += s_sum[j];
    tsum[blockIdx.x] = s;
  }
}

// The tile sums -> in place, the bytes before each tile.  One workgroup.
__global__ __launch_bounds__(kPackTopThreads) void k_wunpack_tscan(uint64_t* __restrict__ tsum, uint32_t n_tiles) {
  tile_scan<kPackTopThreads, 1, uint64_t>(
      n_tiles, [&](uint32_t g, uint64_t c[1]) { c[0] = tsum[g]; },
      [&](uint32_t g, const uint64_t before[1]) { tsum[g] = before[0]; });
}

// pos[k] for the tile's rows, four consecutive rows a thread, and pos[n_wide] behind the last row.
__global__ __launch_bounds__(kPackThreads) void k_wunpack_pos(const uint32_t* __restrict__ len, uint64_t n_wide,
                                                             const uint64_t* __restrict__ tbase, uint64_t* __restrict__ pos) {
  __shared__ uint64_t s_sum[kPackWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t k0 = uint64_t(blockIdx.x) * kWPackTile + tid * kPackPerThread;
  uint32_t x[kPackPerThread];
  uint64_t mine = 0;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    x[q] = k0 + q < n_wide ? len[k0 + q] : 0;
    mine += x[q];
  }
  const uint64_t incl = wave_incl(mine, lane);
  if (lane == 63) s_sum[w] = incl;
  __syncthreads();
  uint64_t run = tbase[blockIdx.x] + (incl - mine);
#pragma unroll
  for (uint32_t j = 0; j < kPackWaves; ++j) run += j < w ? s_sum[j] : 0;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint64_t k = k0 + q;
    if (k < n_wide) {
      pos[k] = run;
      run += x[q];
      if (k + 1 == n_wide) pos[n_wide] = run;
    }
  }
}

int launch_wunpack_check(const WUnpackTab* d_tab, uint32_t n_blocks, uint32_t n_tiles, uint32_t* d_cnt, uint64_t* d_base,
                         WUnpackVerdict* d_verdict, WUnpackRes* res, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_verdict, 0, offsetof(WUnpackVerdict, cross_row), st) != hipSuccess ||
      hipMemsetAsync(&d_verdict->cross_row, 0xFF, sizeof(unsigned long long), st) != hipSuccess)
    return launch_status(hipGetLastError());
  if (!n_blocks || !n_tiles) return CLG_OK;
  hipLaunchKernelGGL(k_wunpack_check, dim3((n_blocks + kPackWaves - 1) / kPackWaves), dim3(kPackThreads), 0, st, d_tab, n_blocks,
                     d_verdict);
  hipLaunchKernelGGL(k_wunpack_kind, dim3(n_tiles), dim3(kPackThreads), 0, st, d_tab, d_cnt);
  hipLaunchKernelGGL(k_wunpack_scan, dim3(1), dim3(kPackTopThreads), 0, st, d_cnt, n_tiles, d_base, res);
  return launch_status(hipGetLastError());
}

int launch_wunpack_write(const WUnpackTab* d_tab, uint32_t n_blocks, uint32_t n_kind_blocks, uint32_t n_tiles,
                         const uint64_t* d_base, const WUnpackDst& dst, uint64_t n_wide, uint64_t* d_tsum, uint64_t* pos,
                         WUnpackVerdict* d_verdict, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  if (!n_tiles || n_blocks <= n_kind_blocks) return CLG_OK;
  hipLaunchKernelGGL(k_wunpack_write, dim3(n_blocks - n_kind_blocks), dim3(kPackThreads), 0, st, d_tab, n_kind_blocks);
  hipLaunchKernelGGL(k_wunpack_merge, dim3(n_tiles), dim3(kPackThreads), 0, st, d_tab, d_base, dst, n_wide, d_tsum, d_verdict);
  if (pos) {
    hipLaunchKernelGGL(k_wunpack_tscan, dim3(1), dim3(kPackTopThreads), 0, st, d_tsum, n_tiles);
    hipLaunchKernelGGL(k_wunpack_pos, dim3(n_tiles), dim3(kPackThreads), 0, st,
                       static_cast<const uint32_t*>(dst.col[CLG_WPACK_VAR_LEN]), n_wide, d_tsum, pos);
  }
  return launch_status(hipGetLastError());
}

}  // namespace clg
