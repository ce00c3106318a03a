// pack_wide_dev.h -- what pack_wide.hip and unpack_wide.hip share on the device beyond pack_dev.h:
// a block's stream from the table, the (element, scheme) dispatch of the block codec's bodies, the
// tile's kind counts, and a row's rank among its kind.  The two files differ in where a row's kind
// comes from and in which way the six fields move; those parts stay in their kernels.
// Device code only, file-local in each unit that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pack_wide.h"
#include "pack_dev.h"
#include "kernels.h"

namespace clg {
namespace {

static_assert(kWPackTile == kPackThreads * kPackPerThread, "a tile is four rows a thread");
static_assert(kWPackTile == kPackBlock, "a tile of rows is a KIND block");
constexpr uint32_t kWPackParts = kPackPerThread * kPackWaves;  // (quarter, wave) pieces of a tile, in row order

// The stream that holds block blk: the last one whose base is at or below it (the bases do not
// decrease).  Tab: WPackTab or WUnpackTab.
template <class Tab>
__device__ __forceinline__ uint32_t wpack_stream_of(const Tab* __restrict__ tab, uint64_t blk) {
  uint32_t s = 0;
#pragma unroll
  for (uint32_t c = 1; c < kWPackStreams; ++c) s += uint32_t(blk >= tab->blk_base[c]);
  return s;
}

// body<element, scheme>(...) of stream s (uniform): pack_dev.h's measure, write or decode.
#define CLG_WPACK_CASE(body, e, d, ...) \
  case (e) * 2 + (d): body<e, d != 0>(__VA_ARGS__); break;
#define CLG_WPACK_DISPATCH(s, body, ...)                              \
  switch (wpack_stream_elem(s) * 2 + uint32_t(wpack_is_delta(s))) {   \
    CLG_WPACK_CASE(body, kElemU8, 0, __VA_ARGS__)                     \
    CLG_WPACK_CASE(body, kElemU8, 1, __VA_ARGS__)                     \
    CLG_WPACK_CASE(body, kElemU32, 0, __VA_ARGS__)                    \
    CLG_WPACK_CASE(body, kElemU32, 1, __VA_ARGS__)                    \
    CLG_WPACK_CASE(body, kElemI32, 0, __VA_ARGS__)                    \
    CLG_WPACK_CASE(body, kElemI32, 1, __VA_ARGS__)                    \
    CLG_WPACK_CASE(body, kElemI64, 0, __VA_ARGS__)                    \
    CLG_WPACK_CASE(body, kElemI64, 1, __VA_ARGS__)                    \
  }

// The kinds of the thread's four rows of `tile` (row q * kPackThreads + tid of the tile; a row past
// n_wide and a row without a kind: kWPackKinds), from w_idx against n_rec and the tag; a row's kind
// byte goes to kind_out (kWPackKinds: the split passes the row by, the call is rejected).  Returns
// the lowest of the thread's rows that have no kind, ~0 for none.
__device__ __forceinline__ uint64_t wpack_row_kinds(const WPackSrc& src, uint32_t tile, uint8_t* __restrict__ kind_out,
                                                    uint32_t kind[kPackPerThread]) {
  uint64_t bad = ~0ull;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint64_t k = uint64_t(tile) * kWPackTile + q * kPackThreads + threadIdx.x;
    kind[q] = kWPackKinds;
    if (k < src.n_wide) {
      kind[q] = wpack_kind_of(src.tag, src.n_rec, src.w_idx[k]);
      if (kind[q] >= kWPackKinds && k < bad) bad = k;
      kind_out[k] = uint8_t(kind[q]);
    }
  }
  return bad;
}

// The tile's four kind counts -> cnt[tile * 4 + kind] (global memory or LDS), from the kinds of the
// thread's four rows (kWPackKinds or above: counted nowhere): ballots per wave, LDS across the
// waves.  All kPackThreads threads call it; one __syncthreads inside, and a caller that counts tile
// after tile in one workgroup puts another between two calls.
__device__ __forceinline__ void wpack_kind_counts(const uint32_t kind[kPackPerThread], uint32_t* __restrict__ cnt,
                                                  uint32_t tile) {
  __shared__ uint32_t s_cnt[kPackWaves][kWPackKinds];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t c[kWPackKinds] = {};  // (the wave's counts: the same in every lane)
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q)
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) c[t] += uint32_t(__popcll(__ballot(kind[q] == t)));
  if (lane == 0) {
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) s_cnt[w][t] = c[t];
  }
  __syncthreads();
  if (tid < kWPackKinds) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPackWaves; ++j) s += s_cnt[j][tid];
    cnt[uint64_t(tile) * kWPackKinds + tid] = s;
  }
}

// The one-workgroup scan of the tile counts: base[tile * 4 + kind] = the rows of the kind before
// the tile; the four totals are returned.  cnt is 16-byte aligned (engine scratch).
__device__ __forceinline__ ScanTotals<kWPackKinds> wpack_kind_scan(const uint32_t* __restrict__ cnt, uint32_t n_tiles,
                                                                  uint64_t* __restrict__ base) {
  // (a round holds at most kPackTopThreads tiles of kWPackTile rows: its sums fit 32 bits)
  static_assert(uint64_t(kPackTopThreads) * kWPackTile <= UINT32_MAX, "a round's kind counts are summed in 32 bits");
  return tile_scan<kPackTopThreads, kWPackKinds, uint32_t>(
      n_tiles,
      [&](uint32_t g, uint32_t c[kWPackKinds]) {
        const uint4 v = *reinterpret_cast<const uint4*>(cnt + uint64_t(g) * kWPackKinds);
        c[0] = v.x, c[1] = v.y, c[2] = v.z, c[3] = v.w;
      },
      [&](uint32_t g, const uint64_t before[kWPackKinds]) {
#pragma unroll
        for (uint32_t t = 0; t < kWPackKinds; ++t) base[uint64_t(g) * kWPackKinds + t] = before[t];
      });
}

// A tile's LDS for wpack_tile_rank: what split and merge then read per row.
struct WPackTileLds {
  uint32_t pre[kWPackParts][kWPackKinds];    // a piece's counts, then the rows of the tile before it
  uint64_t col[kWPackKinds * kWPackFields];  // the per-kind field arrays (tab->col[2 ..])
  uint64_t n[kWPackKinds], base[kWPackKinds];
};

// r[q]: the rank of the thread's row q (row q * kPackThreads + tid of `tile`) among all rows of
// its kind: its tile's base for the kind plus its rank inside the tile (ballot and mbcnt in the
// wave, LDS across the (quarter, wave) pieces in row order).  A kind of kWPackKinds or above has
// no rank.  Also fills l.col and l.n from the table (global memory or LDS, as base is).  All
// kPackThreads threads call it; two __syncthreads inside, the second after l's last write; a
// caller that ranks tile after tile in one workgroup puts another between two calls.
template <class Tab>
__device__ __forceinline__ void wpack_tile_rank(const Tab* __restrict__ tab, const uint64_t* __restrict__ base, uint32_t tile,
                                                const uint32_t kind[kPackPerThread], WPackTileLds& l,
                                                uint64_t r[kPackPerThread]) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < kWPackKinds * kWPackFields) l.col[tid] = uint64_t(reinterpret_cast<uintptr_t>(tab->col[2 + tid]));
  if (tid < kWPackKinds) {
    l.n[tid] = tab->n[wpack_stream(tid, 0)];
    l.base[tid] = base[uint64_t(tile) * kWPackKinds + tid];
  }
  uint32_t below[kPackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    below[q] = 0;
#pragma unroll
    for (uint32_t t = 0; t < kWPackKinds; ++t) {
      const uint64_t m = __ballot(kind[q] == t);
      if (kind[q] == t) below[q] = lane_rank(m);
      if (lane == 0) l.pre[q * kPackWaves + w][t] = uint32_t(__popcll(m));
    }
  }
  __syncthreads();
  if (tid < kWPackKinds) {
    uint32_t run = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWPackParts; ++j) {
      const uint32_t x = l.pre[j][tid];
      l.pre[j][tid] = run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t t = kind[q];
    r[q] = t < kWPackKinds ? l.base[t] + l.pre[q * kPackWaves + w][t] + below[q] : 0;
  }
}

// The split of a tile, after wpack_tile_rank: the six fields of the thread's four rows to the
// per-kind arrays (l.col) at the rows' ranks; no store at or past a kind's length.
__device__ __forceinline__ void wpack_split_rows(const WPackSrc& src, uint32_t tile, const uint32_t kind[kPackPerThread],
                                                 const uint64_t r[kPackPerThread], const WPackTileLds& l) {
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t t = kind[q];
    if (t >= kWPackKinds || r[q] >= l.n[t]) continue;  // (the latter never, while the kind bytes are what pass 1 counted)
    const uint64_t k = uint64_t(tile) * kWPackTile + q * kPackThreads + threadIdx.x;
    const uint64_t* col = &l.col[t * kWPackFields];
    reinterpret_cast<int32_t*>(uintptr_t(col[CLG_WPACK_RC]))[r[q]] = src.w_rc[k];
    reinterpret_cast<int64_t*>(uintptr_t(col[CLG_WPACK_V1]))[r[q]] = src.w_v1[k];
    reinterpret_cast<uint32_t*>(uintptr_t(col[CLG_WPACK_VAR_OFF]))[r[q]] = src.w_var_off[k];
    reinterpret_cast<uint32_t*>(uintptr_t(col[CLG_WPACK_VAR_LEN]))[r[q]] = src.w_var_len[k];
    reinterpret_cast<uint8_t*>(uintptr_t(col[CLG_WPACK_SUB]))[r[q]] = src.w_sub[k];
    reinterpret_cast<int64_t*>(uintptr_t(col[CLG_WPACK_V0]))[r[q]] = src.w_v0[k];
  }
}

}  // namespace
}  // namespace clg
