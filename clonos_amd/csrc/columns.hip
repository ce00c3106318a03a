// columns.hip -- typed replay columns (columns.h): the stable partition of a decoded batch by
// determinant class, computed where the records already are.
//
//  * k_col_count     pass 1: a workgroup per tile of kColTile records reads the tags only (one
//                    16-byte load per thread) and writes the tile's count per class and its
//                    number of tags above 7
//  * k_col_scan      pass 2: ONE workgroup loops over all tiles' counts (config 2's 64 M records
//                    are 16 K tiles: 16 rounds, no look-back) and writes the exclusive per-class
//                    base of every tile; the totals and the first tile with a tag above 7 go to
//                    pinned memory, which the host reads before anything is written to the caller
//  * k_col_write     pass 3: a workgroup per tile reads the tags again and v0, ranks each record
//                    within its class (ballot and mbcnt in the wave, the waves' totals through
//                    LDS) and stores the narrowed value at tile base + rank
//  * k_col_span_base a wave per span boundary: the base of the tile that holds the boundary's
//                    record plus the class counts of the tags before it inside the tile
//  * k_col_wide_v0   a thread per side row: w_v0[k] = v0[w_idx[k]]
//  * k_col_find_bad  one wave: the lowest record of a tile whose tag is above 7
//
// No atomics, no spin waits and no word taken from another running workgroup: kernel boundaries
// order the passes, and the result is deterministic.
//
// In k_col_write a thread's 16 records are kColThreads apart (record k * 256 + thread), so a
// wave's tag and v0 loads are contiguous and, in every round, its lanes of one class store to
// adjacent addresses.  The order column is written with per-lane byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "columns.h"
#include "kernels.h"
#include "wave_dev.h"

namespace clg {

namespace {

constexpr uint32_t kColWaves = kColThreads / 64;
constexpr uint32_t kColChunks = kColPerThread * kColWaves;  // a tile's (round, wave) chunks, in record order
static_assert(kColChunks == 64, "the chunk counts are scanned by one wave");

// The class counts of records i0 .. i0 + 15 (those below n) in 8-bit fields, at most 16 each:
// field c < 5 counts class c, field 5 the tags above 7.
__device__ __forceinline__ uint64_t col_count16(const uint8_t* __restrict__ tag, uint64_t i0, uint64_t n) {
  uint64_t acc = 0;
  if (i0 + kColPerThread <= n && ((uintptr_t)(tag + i0) & 15) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(tag + i0);
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc += 1ull << (8u * col_class((q[j] >> (8 * b)) & 0xFFu));
  } else {  // the batch's last records, or a tag array that is not 16-byte aligned
    for (uint32_t j = 0; j < kColPerThread; ++j)
      if (i0 + j < n) acc += 1ull << (8u * col_class(tag[i0 + j]));
  }
  return acc;
}

}  // namespace

// counts[tile * kColCountWords + c]: records of class c (c < 5), tags above 7 (c == 5).
__global__ __launch_bounds__(kColThreads) void k_col_count(const uint8_t* __restrict__ tag, uint64_t n,
                                                          uint32_t* __restrict__ counts) {
  __shared__ uint32_t ws[kColWaves][6];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t i0 = uint64_t(blockIdx.x) * kColTile + uint64_t(tid) * kColPerThread;
  const uint64_t acc = col_count16(tag, i0, n);
#pragma unroll
  for (uint32_t c = 0; c < 6; ++c) {
    const uint32_t s = wave_sum(uint32_t(acc >> (8u * c)) & 0xFFu);
    if (lane == 0) ws[w][c] = s;
  }
  __syncthreads();
  if (tid < kColCountWords) {
    uint32_t s = 0;
    if (tid < 6)
      for (uint32_t k = 0; k < kColWaves; ++k) s += ws[k][tid];
    counts[size_t(blockIdx.x) * kColCountWords + tid] = s;
  }
}

__global__ __launch_bounds__(kColScanThreads) void k_col_scan(const uint32_t* __restrict__ counts, uint32_t n_tiles,
                                                             uint64_t* __restrict__ base, ColRes* __restrict__ res) {
  // (a round holds at most kColScanThreads * kColTile records: its sums fit 32 bits)
  static_assert(uint64_t(kColScanThreads) * kColTile <= UINT32_MAX, "a round's class counts are summed in 32 bits");
  uint32_t bad = ~0u;  // this thread's first tile with a tag above 7
  const auto tot = tile_scan<kColScanThreads, kColClasses, uint32_t>(
      n_tiles,
      [&](uint32_t t, uint32_t c[kColClasses]) {
        const uint4 lo = *reinterpret_cast<const uint4*>(counts + size_t(t) * kColCountWords);
        const uint2 hi = *reinterpret_cast<const uint2*>(counts + size_t(t) * kColCountWords + 4);
        c[0] = lo.x, c[1] = lo.y, c[2] = lo.z, c[3] = lo.w, c[4] = hi.x;
        if (hi.y && t < bad) bad = t;
      },
      [&](uint32_t t, const uint64_t before[kColClasses]) {
#pragma unroll
        for (uint32_t k = 0; k < kColClasses; ++k) base[size_t(t) * kColClasses + k] = before[k];
      });
  bad = block_min<kColScanThreads>(bad);
  if (threadIdx.x == 0) {
    for (uint32_t k = 0; k < kColClasses; ++k) res->total[k] = tot.v[k];
    res->bad_tile = bad == ~0u ? kColNoTile : uint64_t(bad);
  }
}

struct ColLimits {
  uint64_t n[4];  // the class totals the host checked against the capacities: no store at or past them
};

// One tile's write, by kColThreads threads (tid 0 .. 255, waves w 0 .. 3) that all call it: the
// records i0 .. i0 + kColTile (those below n) go to tb[class] + rank within the tile.  cnt is the
// calling threads' own LDS.  Two __syncthreads inside; cnt is read until the function returns.
__device__ __forceinline__ void col_write_tile(const uint8_t* __restrict__ tag, const int64_t* __restrict__ v0, uint64_t n,
                                               uint64_t i0, uint32_t tid, const uint64_t tb[4],
                                               uint32_t (*cnt)[4], const ColOut& out, const ColLimits& lim) {
  const uint32_t lane = tid & 63, w = tid >> 6;
  uint32_t cls[kColPerThread];
  int64_t v[kColPerThread];
#pragma unroll
  for (uint32_t k = 0; k < kColPerThread; ++k) {
    const uint64_t i = i0 + k * kColThreads + tid;
    cls[k] = i < n ? col_class(tag[i]) : kColBad;
  }
#pragma unroll
  for (uint32_t k = 0; k < kColPerThread; ++k) {
    const uint64_t i = i0 + k * kColThreads + tid;
    v[k] = cls[k] < kColWide ? v0[i] : 0;  // (wide records' v0 goes to w_v0)
  }
  // the chunks' counts, then their exclusive prefix in record order (round-major, then wave)
#pragma unroll
  for (uint32_t k = 0; k < kColPerThread; ++k) {
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      const uint64_t m = __ballot(cls[k] == c);
      if (lane == 0) cnt[k * kColWaves + w][c] = (uint32_t)__popcll(m);
    }
  }
  __syncthreads();
  if (tid < kColChunks) {
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      const uint32_t x = cnt[tid][c];
      cnt[tid][c] = wave_incl(x, lane) - x;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kColPerThread; ++k) {
    uint32_t rank = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      const uint64_t m = __ballot(cls[k] == c);
      if (cls[k] == c) rank = lane_rank(m);
    }
    const uint32_t c = cls[k];
    if (c < 4) {
      const uint64_t at = tb[c] + cnt[k * kColWaves + w][c] + rank;
      if (at < lim.n[c]) {
        if (c == kColOrder) out.order[at] = col_i8(v[k]);
        else if (c == kColTimestamp) out.timestamp[at] = v[k];
        else if (c == kColRng) out.rng[at] = col_i32(v[k]);
        else out.buffer_built[at] = col_i32(v[k]);
      }
    }
  }
}

__global__ __launch_bounds__(kColThreads) void k_col_write(const uint8_t* __restrict__ tag, const int64_t* __restrict__ v0,
                                                          uint64_t n, const uint64_t* __restrict__ base, ColOut out,
                                                          ColLimits lim) {
  __shared__ uint32_t cnt[kColChunks][4];
  uint64_t tb[4];
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c) tb[c] = base[size_t(blockIdx.x) * kColClasses + c];
  col_write_tile(tag, v0, n, uint64_t(blockIdx.x) * kColTile, threadIdx.x, tb, cnt, out, lim);
}

// span_base[s * 5 + c], s <= n_spans: the class-c records before record span_rec_base[s].
__global__ __launch_bounds__(256) void k_col_span_base(const uint8_t* __restrict__ tag, uint64_t n,
                                                      const uint64_t* __restrict__ base, const ColRes* __restrict__ res,
                                                      const uint64_t* __restrict__ span_rec_base, uint32_t n_spans,
                                                      uint64_t* __restrict__ span_base) {
  const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (s > n_spans) return;  // (wave-uniform)
  const uint64_t r = span_rec_base[s];
  uint64_t b[kColClasses];
  uint32_t c[kColClasses] = {0, 0, 0, 0, 0};
  if (r >= n) {  // the end of the batch: the totals
#pragma unroll
    for (uint32_t k = 0; k < kColClasses; ++k) b[k] = res->total[k];
  } else {
    const uint64_t tile = r / kColTile, t0 = tile * kColTile;
#pragma unroll
    for (uint32_t k = 0; k < kColClasses; ++k) b[k] = base[tile * kColClasses + k];
    for (uint64_t i = t0 + lane; i < r; i += 64) {
      const uint32_t k = col_class(tag[i]);
#pragma unroll
      for (uint32_t q = 0; q < kColClasses; ++q) c[q] += k == q;
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kColClasses; ++k) {
    const uint32_t t = wave_sum(c[k]);
    if (lane == k) span_base[uint64_t(s) * kColClasses + k] = b[k] + t;
  }
}

__global__ __launch_bounds__(256) void k_col_wide_v0(const uint32_t* __restrict__ w_idx, uint64_t n_wide,
                                                    const int64_t* __restrict__ v0, uint64_t n,
                                                    int64_t* __restrict__ w_v0) {
  const uint64_t k = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= n_wide) return;
  const uint32_t i = w_idx[k];
  w_v0[k] = i < n ? v0[i] : 0;
}

__global__ __launch_bounds__(64) void k_col_find_bad(const uint8_t* __restrict__ tag, uint64_t n, uint64_t tile,
                                                    ColRes* __restrict__ res) {
  const uint32_t lane = threadIdx.x;
  const uint64_t t0 = tile * kColTile, t1 = t0 + kColTile < n ? t0 + kColTile : n;
  uint64_t best = ~0ull;
  for (uint64_t i = t0 + lane; i < t1; i += 64)
    if (col_class(tag[i]) == kColBad && i < best) best = i;
  best = wave_min(best);
  if (lane == 0) {
    res->bad_index = best;
    res->bad_tag = best != ~0ull ? tag[best] : 0;
  }
}

// ---- small batches, one launch --------------------------------------------------------------
// ONE workgroup does everything above for a batch of at most kColSmallRecords records and
// kColSmallSpans spans.  Phase 1 reads the tags only (a round is four tiles, a 16-byte load per
// thread): per-tile class counts in LDS, their exclusive bases, the totals, the lowest record
// with a tag above 7, every span's base (the waves share the boundaries), and then the check the
// host does between the multi-kernel form's passes.  The result block goes to pinned memory.
// Phase 2 runs only when the check passed: the rounds' tiles through col_write_tile with the
// bases from LDS, then the tags, the side rows and w_v0.  __syncthreads only: no atomics, no
// flags, no waits.
namespace {

constexpr uint32_t kSmallWaves = kColScanThreads / 64;
constexpr uint32_t kSmallRoundTiles = kColScanThreads / kColThreads;
constexpr uint32_t kSmallMaxTiles = (kColSmallRecords + kColTile - 1) / kColTile;
static_assert(kSmallRoundTiles * 6 <= kColScanThreads, "a thread per (tile of the round, class)");

// Array i < n elements from src to dst by the whole workgroup (dst null: not written).
template <class T>
__device__ __forceinline__ void col_small_copy(T* __restrict__ dst, const T* __restrict__ src, uint64_t n, uint32_t tid) {
  if (!dst) return;
  for (uint64_t i = tid; i < n; i += kColScanThreads) dst[i] = src[i];
}

}  // namespace

__global__ __launch_bounds__(kColScanThreads) void k_col_small(const ColSmallIn in, const ColSmallOut out,
                                                              ColSmallRes* __restrict__ res,
                                                              uint64_t* __restrict__ span_base) {
  __shared__ uint32_t ws[kSmallWaves][6];
  __shared__ uint32_t tile[kSmallMaxTiles][6];  // a tile's counts, then (classes 0 .. 4) its exclusive bases
  __shared__ uint32_t tot[kColClasses];
  __shared__ uint64_t wbad[kSmallWaves];
  __shared__ uint32_t s_write;
  __shared__ ColLimits s_lim;  // (indexed by a record's class: in LDS by name, not as a promoted private array)
  __shared__ uint32_t cnt[kSmallRoundTiles][kColChunks][4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t n = in.n;
  const uint32_t n_tiles = uint32_t((n + kColTile - 1) / kColTile);  // (<= kSmallMaxTiles: the host's eligibility)

  // ---- phase 1: the tags
  uint64_t bad = ~0ull;  // this thread's lowest record with a tag above 7
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kSmallRoundTiles) {
    const uint64_t i0 = uint64_t(t0) * kColTile + uint64_t(tid) * kColPerThread;
    const uint64_t acc = col_count16(in.tag, i0, n);
    if ((acc >> 40) && bad == ~0ull)
      for (uint32_t j = 0; j < kColPerThread; ++j)
        if (i0 + j < n && col_class(in.tag[i0 + j]) == kColBad) {
          bad = i0 + j;
          break;
        }
#pragma unroll
    for (uint32_t c = 0; c < 6; ++c) {
      const uint32_t s = wave_sum(uint32_t(acc >> (8u * c)) & 0xFFu);
      if (lane == 0) ws[w][c] = s;
    }
    __syncthreads();
    if (tid < kSmallRoundTiles * 6) {
      const uint32_t q = tid / 6, c = tid % 6;
      uint32_t s = 0;
      for (uint32_t k = 0; k < kColWaves; ++k) s += ws[q * kColWaves + k][c];
      if (t0 + q < n_tiles) tile[t0 + q][c] = s;
    }
    __syncthreads();  // (ws is written again in the next round)
  }
  bad = wave_min(bad);
  if (lane == 0) wbad[w] = bad;
  if (tid < kColClasses) {  // (the tiles' counts were written before the loop's last barrier)
    uint32_t run = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
      const uint32_t x = tile[t][tid];
      tile[t][tid] = run;
      run += x;
    }
    tot[tid] = run;
  }
  __syncthreads();

  // every span's base: the base of the tile that holds the boundary's record plus the counts
  // before it inside the tile (k_col_span_base's rule), a wave per boundary
  if (span_base && in.span_rec_base && in.n_spans) {
    for (uint32_t s = w; s <= in.n_spans; s += kSmallWaves) {
      const uint64_t r = in.span_rec_base[s];
      uint32_t b[kColClasses], c[kColClasses] = {0, 0, 0, 0, 0};
      if (r >= n) {
#pragma unroll
        for (uint32_t k = 0; k < kColClasses; ++k) b[k] = tot[k];
      } else {
        const uint32_t t = uint32_t(r / kColTile);
#pragma unroll
        for (uint32_t k = 0; k < kColClasses; ++k) b[k] = tile[t][k];
        for (uint64_t i = uint64_t(t) * kColTile + lane; i < r; i += 64) {
          const uint32_t k = col_class(in.tag[i]);
#pragma unroll
          for (uint32_t q = 0; q < kColClasses; ++q) c[q] += k == q;
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < kColClasses; ++k) {
        const uint32_t x = wave_sum(c[k]);
        if (lane == k) span_base[uint64_t(s) * kColClasses + k] = uint64_t(b[k]) + x;
      }
    }
  }

  // the check, and the result block
  if (tid == 0) {
    for (uint32_t j = 1; j < kSmallWaves; ++j) bad = wbad[j] < bad ? wbad[j] : bad;
    uint64_t t64[kColClasses];
#pragma unroll
    for (uint32_t k = 0; k < kColClasses; ++k) res->total[k] = t64[k] = tot[k];
    uint32_t verdict = kColSmallWritten, short_cap = 0;
    if (bad != ~0ull) {
      verdict = kColSmallBadTag;
    } else if (t64[kColWide] != in.n_wide) {
      verdict = kColSmallWideCount;
    } else if (in.sizes_only) {
      verdict = kColSmallSizes;
    } else {
      const uint64_t need[6] = {n, t64[0], t64[1], t64[2], t64[3], t64[4]};
#pragma unroll
      for (int k = 5; k >= 0; --k)
        if (out.cap[k] < need[k]) verdict = kColSmallCapacity, short_cap = uint32_t(k);  // (ends at the first short one)
    }
    res->bad_index = bad;
    res->bad_tag = bad != ~0ull ? in.tag[bad] : 0;
    res->verdict = verdict;
    res->short_cap = short_cap;
    uint64_t off[13];
    col_pack_offsets(n, t64, off);
#pragma unroll
    for (int k = 0; k < 13; ++k) res->pack_off[k] = off[k];
    s_write = verdict == kColSmallWritten;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) s_lim.n[k] = t64[k];
  }
  __syncthreads();
  if (!s_write) return;  // no column written

  // ---- phase 2: the write
  uint64_t t64[kColClasses];
#pragma unroll
  for (uint32_t k = 0; k < kColClasses; ++k) t64[k] = tot[k];
  ColSmallOut o = out;
  if (out.pack) {
    uint64_t off[13];
    col_pack_offsets(n, t64, off);
    o.tag = out.pack + off[0];
    o.order = reinterpret_cast<int8_t*>(out.pack + off[1]);
    o.timestamp = reinterpret_cast<int64_t*>(out.pack + off[2]);
    o.rng = reinterpret_cast<int32_t*>(out.pack + off[3]);
    o.buffer_built = reinterpret_cast<int32_t*>(out.pack + off[4]);
    o.w_idx = reinterpret_cast<uint32_t*>(out.pack + off[5]);
    o.w_rc = reinterpret_cast<int32_t*>(out.pack + off[6]);
    o.w_v1 = reinterpret_cast<int64_t*>(out.pack + off[7]);
    o.w_var_off = reinterpret_cast<uint32_t*>(out.pack + off[8]);
    o.w_var_len = reinterpret_cast<uint32_t*>(out.pack + off[9]);
    o.w_sub = out.pack + off[10];
    o.w_v0 = reinterpret_cast<int64_t*>(out.pack + off[11]);
  }
  const ColOut co{o.order, o.timestamp, o.rng, o.buffer_built, o.w_v0};
  const uint32_t q = tid / kColThreads;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kSmallRoundTiles) {
    const uint32_t t = t0 + q;
    uint64_t tb[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) tb[c] = t < n_tiles ? tile[t][c] : 0;
    col_write_tile(in.tag, in.v0, n, uint64_t(t) * kColTile, tid % kColThreads, tb, cnt[q], co, s_lim);
    __syncthreads();  // (cnt is written again in the next round)
  }
  // the arrays that stay as they are, and the wide rows' v0
  const uint64_t nw = in.n_wide;
  if (o.tag) {
    if (((uintptr_t(o.tag) | uintptr_t(in.tag)) & 15) == 0) {
      const uint64_t n16 = n / 16;
      col_small_copy(reinterpret_cast<uint4*>(o.tag), reinterpret_cast<const uint4*>(in.tag), n16, tid);
      if (n16 * 16 + tid < n) o.tag[n16 * 16 + tid] = in.tag[n16 * 16 + tid];
    } else {
      col_small_copy(o.tag, in.tag, n, tid);
    }
  }
  col_small_copy(o.w_idx, in.w_idx, nw, tid);
  col_small_copy(o.w_rc, in.w_rc, nw, tid);
  col_small_copy(o.w_v1, in.w_v1, nw, tid);
  col_small_copy(o.w_var_off, in.w_var_off, nw, tid);
  col_small_copy(o.w_var_len, in.w_var_len, nw, tid);
  col_small_copy(o.w_sub, in.w_sub, nw, tid);
  if (o.w_v0)
    for (uint64_t k = tid; k < nw; k += kColScanThreads) {
      const uint32_t i = in.w_idx[k];
      o.w_v0[k] = i < n ? in.v0[i] : 0;
    }
}

int launch_col_small(const ColSmallIn& in, const ColSmallOut& out, ColSmallRes* res, uint64_t* span_base, void* stream) {
  hipLaunchKernelGGL(k_col_small, dim3(1), dim3(kColScanThreads), 0, (hipStream_t)stream, in, out, res, span_base);
  return launch_status(hipGetLastError());
}

int launch_col_count_scan(const ColIn& in, uint32_t n_tiles, uint32_t* d_counts, uint64_t* d_base, ColRes* res,
                          void* stream) {
  if (n_tiles)
    hipLaunchKernelGGL(k_col_count, dim3(n_tiles), dim3(kColThreads), 0, (hipStream_t)stream, in.tag, in.n, d_counts);
  hipLaunchKernelGGL(k_col_scan, dim3(1), dim3(kColScanThreads), 0, (hipStream_t)stream, d_counts, n_tiles, d_base, res);
  return launch_status(hipGetLastError());
}

int launch_col_find_bad(const ColIn& in, uint64_t tile, ColRes* res, void* stream) {
  hipLaunchKernelGGL(k_col_find_bad, dim3(1), dim3(64), 0, (hipStream_t)stream, in.tag, in.n, tile, res);
  return launch_status(hipGetLastError());
}

int launch_col_write(const ColIn& in, uint32_t n_tiles, const uint64_t* d_base, const ColRes* res, bool write,
                     const ColOut& out, const uint64_t* d_span_rec_base, uint32_t n_spans, uint64_t* span_base,
                     void* stream) {
  if (write && n_tiles) {
    ColLimits lim;
    for (int c = 0; c < 4; ++c) lim.n[c] = res->total[c];
    hipLaunchKernelGGL(k_col_write, dim3(n_tiles), dim3(kColThreads), 0, (hipStream_t)stream, in.tag, in.v0, in.n,
                       d_base, out, lim);
  }
  if (write && out.w_v0 && in.n_wide)
    hipLaunchKernelGGL(k_col_wide_v0, dim3((uint32_t)((in.n_wide + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       in.w_idx, in.n_wide, in.v0, in.n, out.w_v0);
  if (span_base && d_span_rec_base)
    hipLaunchKernelGGL(k_col_span_base, dim3((n_spans + 1 + 3) / 4), dim3(256), 0, (hipStream_t)stream, in.tag, in.n,
                       d_base, res, d_span_rec_base, n_spans, span_base);
  return launch_status(hipGetLastError());
}

}  // namespace clg
