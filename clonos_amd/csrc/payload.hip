// payload.hip -- the payload column (payload.h): the wide rows' payload bytes packed back to
// back in row order, gathered from wherever the spans lie (pool segments, a caller's device
// buffer, staged host input).
//
//  * k_pay_size   pass 1: a workgroup per tile of kPayTile rows loads the rows' offsets and
//                 lengths (a 16-byte load each per thread), finds each row's span (one search
//                 for the tile's ends, one per thread inside them, then steps), checks
//                 off + len <= span length and writes the tile's byte sum (u64) and its lowest
//                 bad row; a bad row counts as length 0 and none of its bytes is loaded
//  * k_pay_scan   pass 2: ONE workgroup loops over the tiles' sums (a carry between rounds, no
//                 look-back) and writes every tile's base; n_var and the lowest bad row go to
//                 pinned memory, which the host reads before anything is written to the caller
//  * k_pay_pos    pass 3: pos[k] = tile base + the scan inside the tile; pos[n_rows] = n_var
//  * k_pay_copy   pass 4: the tile's scan again (pos may lie across the link and is not read
//                 back), then a row of under kPayWaveRow bytes is copied by its own lane, byte
//                 by byte inside the row's range, and a longer row by one wave, a per-segment
//                 piece at a time, through copy_range<64>
//
// No atomics between workgroups, no spin waits and no word taken from another running
// workgroup: kernel boundaries order the passes, and the result is deterministic (the order in
// which a tile's long rows are handed to its waves is not, the bytes are).
//
// Source address: a span is either contiguous (PaySpan::base set) or a run of a log's physical
// bytes behind the call's segment table; the kernels branch on base.  A degenerate table would
// have to express a caller's buffer as pool segments, which it is not.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "copy_range.h"
#include "kernels.h"
#include "payload.h"
#include "wave_dev.h"

namespace clg {

namespace {

constexpr uint32_t kPayWaves = kPayThreads / 64;
static_assert(kPayPerThread == 4, "a thread's offsets and lengths are one 16-byte load each");
static_assert(kPayTile <= 65536, "a tile's long rows are listed as u16");

// Rows k0 .. k0 + 3 of a[] (n entries): zero at and past n.
__device__ __forceinline__ void pay_load4(const uint32_t* __restrict__ a, uint64_t k0, uint64_t n, uint32_t v[4]) {
  if (k0 + kPayPerThread <= n && ((uintptr_t)(a + k0) & 15) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(a + k0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {  // the last rows, or an array that is not 16-byte aligned
#pragma unroll
    for (uint32_t j = 0; j < kPayPerThread; ++j) v[j] = k0 + j < n ? a[k0 + j] : 0u;
  }
}

// The spans of the tile's first and last row (thread 0 -> rng[0], rng[1]); the caller syncs.
__device__ __forceinline__ void pay_tile_spans(const PayIn& in, uint64_t tile0, uint32_t* rng) {
  const uint64_t last = (tile0 + kPayTile < in.n_rows ? tile0 + kPayTile : in.n_rows) - 1;
  rng[0] = pay_span_of(in.row_base, 0, in.n_spans, tile0);
  rng[1] = pay_span_of(in.row_base, rng[0], in.n_spans, last);
}

// This thread's rows k0 .. k0 + 3: offsets, lengths (0 past n_rows) and spans.
struct PayRows {
  uint32_t off[kPayPerThread], len[kPayPerThread], span[kPayPerThread];
};
__device__ __forceinline__ void pay_rows(const PayIn& in, uint64_t k0, const uint32_t* rng, PayRows& r) {
  pay_load4(in.off, k0, in.n_rows, r.off);
  pay_load4(in.len, k0, in.n_rows, r.len);
#pragma unroll
  for (uint32_t j = 0; j < kPayPerThread; ++j) r.span[j] = 0;
  if (k0 >= in.n_rows) return;
  uint32_t s = pay_span_of(in.row_base, rng[0], rng[1] + 1, k0);
#pragma unroll
  for (uint32_t j = 0; j < kPayPerThread; ++j) {
    const uint64_t k = k0 + j;
    if (k < in.n_rows) {
      while (in.row_base[s + 1] <= k) ++s;  // (k < n_rows = row_base[n_spans]: ends at s < n_spans)
      r.span[j] = s;
    }
  }
}

// One lane copies a short row: loads and stores stay inside the row's own bytes, across a
// segment boundary too.
__device__ __forceinline__ void pay_copy_lane(const PayIn& in, const PaySpan& sp, uint32_t off, uint32_t len,
                                              uint8_t* __restrict__ dst) {
  if (sp.base) {
    const uint8_t* src = sp.base + off;
    for (uint32_t i = 0; i < len; ++i) dst[i] = src[i];
    return;
  }
  const uint32_t C = in.seg_bytes;
  uint64_t p = uint64_t(sp.phys) + off;
  uint32_t done = 0;
  while (done < len) {
    const uint32_t so = uint32_t(p % C), take = len - done < C - so ? len - done : C - so;
    const uint8_t* src = in.pool + size_t(in.segtab[sp.segtab_off + p / C]) * C + so;
    for (uint32_t i = 0; i < take; ++i) dst[done + i] = src[i];
    done += take;
    p += take;
  }
}

// One wave copies a long row, a per-segment piece at a time (arguments wave-uniform).
__device__ __forceinline__ void pay_copy_wave(const PayIn& in, const PaySpan& sp, uint32_t off, uint32_t len,
                                              uint8_t* dst, uint32_t lane) {
  if (sp.base) {
    copy_range<64>(sp.base + off, dst, len, lane);
    return;
  }
  const uint32_t C = in.seg_bytes;
  uint64_t p = uint64_t(sp.phys) + off;
  uint32_t done = 0;
  while (done < len) {
    const uint32_t so = uint32_t(p % C), take = len - done < C - so ? len - done : C - so;
    copy_range<64>(in.pool + size_t(in.segtab[sp.segtab_off + p / C]) * C + so, dst + done, take, lane);
    done += take;
    p += take;
  }
}

}  // namespace

__global__ __launch_bounds__(kPayThreads) void k_pay_size(const PayIn in, uint64_t* __restrict__ sum,
                                                         uint64_t* __restrict__ bad) {
  __shared__ uint32_t rng[2];
  __shared__ uint64_t ws[kPayWaves], wb[kPayWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t tile0 = uint64_t(blockIdx.x) * kPayTile, k0 = tile0 + uint64_t(tid) * kPayPerThread;
  if (tid == 0) pay_tile_spans(in, tile0, rng);
  __syncthreads();
  PayRows r;
  pay_rows(in, k0, rng, r);
  uint64_t acc = 0, b = kPayNoRow;
#pragma unroll
  for (uint32_t j = 0; j < kPayPerThread; ++j) {
    if (k0 + j >= in.n_rows) continue;
    if (pay_row_ok(r.off[j], r.len[j], in.spans[r.span[j]].len)) acc += r.len[j];
    else if (b == kPayNoRow) b = k0 + j;
  }
  acc = wave_sum(acc);
  b = wave_min(b);
  if (lane == 0) ws[w] = acc, wb[w] = b;
  __syncthreads();
  if (tid == 0) {
    for (uint32_t k = 1; k < kPayWaves; ++k) acc += ws[k], b = wb[k] < b ? wb[k] : b;
    sum[blockIdx.x] = acc;
    bad[blockIdx.x] = b;
  }
}

__global__ __launch_bounds__(kPayScanThreads) void k_pay_scan(const uint64_t* __restrict__ sum,
                                                             const uint64_t* __restrict__ bad, uint32_t n_tiles,
                                                             uint64_t* __restrict__ base, PayRes* __restrict__ res) {
  uint64_t b = kPayNoRow;  // this thread's lowest bad row
  const auto tot = tile_scan<kPayScanThreads, 1, uint64_t>(
      n_tiles,
      [&](uint32_t t, uint64_t c[1]) {
        c[0] = sum[t];
        const uint64_t x = bad[t];
        b = x < b ? x : b;
      },
      [&](uint32_t t, const uint64_t before[1]) { base[t] = before[0]; });
  b = block_min<kPayScanThreads>(b);
  if (threadIdx.x == 0) {
    res->n_var = tot.v[0];
    res->bad_row = b;
  }
}

__global__ __launch_bounds__(kPayThreads) void k_pay_pos(const PayIn in, const uint64_t* __restrict__ base,
                                                        uint64_t n_var, uint64_t* __restrict__ pos) {
  __shared__ uint64_t ws[kPayWaves];
  const uint32_t tid = threadIdx.x;
  const uint64_t k0 = uint64_t(blockIdx.x) * kPayTile + uint64_t(tid) * kPayPerThread;
  uint32_t len[kPayPerThread];
  pay_load4(in.len, k0, in.n_rows, len);
  uint64_t at = base[blockIdx.x] + tile_excl<kPayWaves>(uint64_t(len[0]) + len[1] + len[2] + len[3], tid, ws);
#pragma unroll
  for (uint32_t j = 0; j < kPayPerThread; ++j) {
    if (k0 + j < in.n_rows) pos[k0 + j] = at;
    at += len[j];
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) pos[in.n_rows] = n_var;
}

// A tile's LDS for pay_copy_tile.
struct PayTileLds {
  uint64_t s_pos[kPayTile];   // the long rows' destinations
  uint64_t ws[kPayWaves];
  uint32_t s_span[kPayTile];  // ... and spans
  uint32_t rng[2];
  uint32_t s_nlong;
  uint16_t s_long[kPayTile];  // the tile's long rows, in any order
};

// One tile's pos and copy, by kPayThreads threads (tid 0 .. 255) that all call it: the rows
// tile0 .. tile0 + kPayTile (those below n_rows), whose bytes start at `base`.  pos null: not
// written.  l is the calling threads' own LDS; three __syncthreads inside.
__device__ __forceinline__ void pay_copy_tile(const PayIn& in, uint64_t tile0, uint32_t tid, uint64_t base, uint64_t n_var,
                                              uint64_t* __restrict__ pos, uint8_t* __restrict__ var, PayTileLds& l) {
  const uint32_t lane = tid & 63, w = tid >> 6;
  const uint64_t k0 = tile0 + uint64_t(tid) * kPayPerThread;
  if (tid == 0) {
    if (tile0 < in.n_rows) pay_tile_spans(in, tile0, l.rng);
    l.s_nlong = 0;
  }
  __syncthreads();
  PayRows r;
  pay_rows(in, k0, l.rng, r);
  uint64_t at = base + tile_excl<kPayWaves>(uint64_t(r.len[0]) + r.len[1] + r.len[2] + r.len[3], tid, l.ws);
#pragma unroll
  for (uint32_t j = 0; j < kPayPerThread; ++j) {
    const uint32_t L = r.len[j];
    if (pos && k0 + j < in.n_rows) pos[k0 + j] = at;
    if (L && at + L <= n_var) {  // (n_var: the total that was checked against the capacity)
      if (L < kPayWaveRow) {
        pay_copy_lane(in, in.spans[r.span[j]], r.off[j], L, var + at);
      } else {
        const uint32_t q = tid * kPayPerThread + j, i = atomicAdd(&l.s_nlong, 1u);  // (LDS, this workgroup's own)
        l.s_long[i] = uint16_t(q);
        l.s_pos[q] = at;
        l.s_span[q] = r.span[j];
      }
    }
    at += L;
  }
  __syncthreads();
  const uint32_t n_long = l.s_nlong;
  for (uint32_t i = w; i < n_long; i += kPayWaves) {
    const uint32_t q = l.s_long[i];
    const uint64_t k = tile0 + q;
    pay_copy_wave(in, in.spans[l.s_span[q]], in.off[k], in.len[k], var + l.s_pos[q], lane);
  }
}

__global__ __launch_bounds__(kPayThreads) void k_pay_copy(const PayIn in, const uint64_t* __restrict__ base,
                                                         uint64_t n_var, uint8_t* __restrict__ var) {
  __shared__ PayTileLds l;
  pay_copy_tile(in, uint64_t(blockIdx.x) * kPayTile, threadIdx.x, base[blockIdx.x], n_var, nullptr, var, l);
}

// ---- small batches, one launch --------------------------------------------------------------
// ONE workgroup does size, scan, the check the host does between the multi-kernel form's
// passes, pos and the copy, for at most kPaySmallRows rows.  A round is four tiles, one per 256
// threads.  Phase 1: the rows' spans and ranges, the tiles' byte sums in LDS, n_var, the lowest
// bad row, the capacities; the result block goes to pinned memory.  Phase 2, only when the
// check passed: the tiles through pay_copy_tile with the bases from LDS.  No byte of a bad row is
// loaded (a bad row ends the kernel before any copy) and no store lands at or past n_var.
namespace {
constexpr uint32_t kPaySmallWaves = kPayScanThreads / 64;
constexpr uint32_t kPaySmallRoundTiles = kPayScanThreads / kPayThreads;
constexpr uint32_t kPaySmallMaxTiles = (kPaySmallRows + kPayTile - 1) / kPayTile;
}  // namespace

__global__ __launch_bounds__(kPayScanThreads) void k_pay_small(const PayIn in, uint64_t* __restrict__ pos,
                                                              uint8_t* __restrict__ var, uint64_t cap_pos, uint64_t cap_var,
                                                              uint32_t sizes_only, PaySmallRes* __restrict__ res) {
  __shared__ PayTileLds l[kPaySmallRoundTiles];
  __shared__ uint64_t ws[kPaySmallWaves], wb[kPaySmallWaves];
  __shared__ uint64_t tsum[kPaySmallMaxTiles];  // a tile's byte sum, then the bytes before it
  __shared__ uint64_t tbad[kPaySmallMaxTiles];
  __shared__ uint64_t s_nvar;
  __shared__ uint32_t s_write;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t q = tid / kPayThreads, ttid = tid % kPayThreads;
  const uint32_t n_tiles = uint32_t((in.n_rows + kPayTile - 1) / kPayTile);  // (<= kPaySmallMaxTiles: the host's eligibility)

  // ---- phase 1: sizes
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kPaySmallRoundTiles) {
    const uint64_t tile0 = uint64_t(t0 + q) * kPayTile, k0 = tile0 + uint64_t(ttid) * kPayPerThread;
    if (ttid == 0 && tile0 < in.n_rows) pay_tile_spans(in, tile0, l[q].rng);
    __syncthreads();
    PayRows r;
    pay_rows(in, k0, l[q].rng, r);
    uint64_t acc = 0, b = kPayNoRow;
#pragma unroll
    for (uint32_t j = 0; j < kPayPerThread; ++j) {
      if (k0 + j >= in.n_rows) continue;
      if (pay_row_ok(r.off[j], r.len[j], in.spans[r.span[j]].len)) acc += r.len[j];
      else if (b == kPayNoRow) b = k0 + j;
    }
    acc = wave_sum(acc);
    b = wave_min(b);
    if (lane == 0) ws[w] = acc, wb[w] = b;
    __syncthreads();
    if (ttid == 0 && t0 + q < n_tiles) {
      for (uint32_t k = 1; k < kPayWaves; ++k) acc += ws[w + k], b = wb[w + k] < b ? wb[w + k] : b;
      tsum[t0 + q] = acc;
      tbad[t0 + q] = b;
    }
    __syncthreads();  // (ws, wb and rng are written again in the next round)
  }
  if (tid == 0) {
    uint64_t run = 0, b = kPayNoRow;
    for (uint32_t t = 0; t < n_tiles; ++t) {
      const uint64_t x = tsum[t];
      tsum[t] = run;
      run += x;
      b = tbad[t] < b ? tbad[t] : b;
    }
    uint32_t verdict = kPaySmallWritten, short_cap = 0;
    if (b != kPayNoRow) verdict = kPaySmallBadRow;
    else if (sizes_only) verdict = kPaySmallSizes;
    else if (cap_pos < in.n_rows + 1) verdict = kPaySmallCapacity, short_cap = 0;
    else if (cap_var < run) verdict = kPaySmallCapacity, short_cap = 1;
    res->n_var = run;
    res->bad_row = b;
    res->verdict = verdict;
    res->short_cap = short_cap;
    s_nvar = run;
    s_write = verdict == kPaySmallWritten;
  }
  __syncthreads();
  if (!s_write) return;  // nothing written

  // ---- phase 2: pos and the copy
  const uint64_t n_var = s_nvar;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += kPaySmallRoundTiles) {
    const uint32_t t = t0 + q;
    pay_copy_tile(in, uint64_t(t) * kPayTile, ttid, t < n_tiles ? tsum[t] : n_var, n_var, pos, var, l[q]);
    __syncthreads();  // (l is written again in the next round)
  }
  if (tid == 0) pos[in.n_rows] = n_var;
}

int launch_pay_size_scan(const PayIn& in, uint32_t n_tiles, uint64_t* d_sum, uint64_t* d_bad, uint64_t* d_base,
                         PayRes* res, void* stream) {
  if (n_tiles) hipLaunchKernelGGL(k_pay_size, dim3(n_tiles), dim3(kPayThreads), 0, (hipStream_t)stream, in, d_sum, d_bad);
  hipLaunchKernelGGL(k_pay_scan, dim3(1), dim3(kPayScanThreads), 0, (hipStream_t)stream, d_sum, d_bad, n_tiles, d_base, res);
  return launch_status(hipGetLastError());
}

int launch_pay_small(const PayIn& in, uint64_t* pos, uint8_t* var, uint64_t cap_pos, uint64_t cap_var, bool sizes_only,
                     PaySmallRes* res, void* stream) {
  hipLaunchKernelGGL(k_pay_small, dim3(1), dim3(kPayScanThreads), 0, (hipStream_t)stream, in, pos, var, cap_pos, cap_var,
                     uint32_t(sizes_only), res);
  return launch_status(hipGetLastError());
}

int launch_pay_write(const PayIn& in, uint32_t n_tiles, const uint64_t* d_base, uint64_t n_var, uint64_t* pos,
                     uint8_t* var, void* stream) {
  if (!n_tiles) return CLG_OK;
  if (pos) hipLaunchKernelGGL(k_pay_pos, dim3(n_tiles), dim3(kPayThreads), 0, (hipStream_t)stream, in, d_base, n_var, pos);
  if (var && n_var)
    hipLaunchKernelGGL(k_pay_copy, dim3(n_tiles), dim3(kPayThreads), 0, (hipStream_t)stream, in, d_base, n_var, var);
  return launch_status(hipGetLastError());
}

}  // namespace clg
