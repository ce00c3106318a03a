// ppay.hip -- the packed payload column (ppay.h): rows front-coded against the lowest row of their
// length in their tile.  A workgroup of kPackThreads threads per tile of kPpayTile rows, four
// consecutive rows a thread, as the pack units and payload.hip have it.
//
//  pack    k_ppay_lcp    the lengths from pos and the lowest bad row; the tile's anchors; every
//                        row's lcp (a row under kPayWaveRow bytes by its lane, a longer one by a
//                        wave with a ballot of the first differing piece); the lcps to scratch,
//                        the tile's block measured, the tile's tail sum
//          k_ppay_scan   ONE workgroup: tail sums -> tail bases, block sizes -> pos in bits; the
//                        totals and the lowest bad row to pinned memory, where the host checks them
//          k_ppay_write  the block (pack_block_write), the rows' tail offsets by an in-tile scan,
//                        the tails copied, lane or wave by length
//  unpack  k_ppay_in     the block check, the lcps decoded, the pos rules, the anchors, the lcp
//                        rules, the tail sum, the tile's findings
//          k_ppay_in_scan  ONE workgroup: tail bases, the lowest finding of each kind, the totals
//          k_ppay_out    the tail offsets (the anchors' too), then prefix and tail to var + pos[k]
//
// The anchor step (ppay_anchors) is one function for both directions.  No atomics on global
// memory, no spin waits between workgroups: kernel boundaries order the passes and the bytes are
// the same on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "copy_range.h"
#include "diff.h"
#include "kernels.h"
#include "pack_dev.h"
#include "payload.h"
#include "ppay.h"

namespace clg {

namespace {

constexpr uint32_t kPpayEmpty = ~0u;  // a free slot's key; a row of this length has a slot of its own
static_assert(kPpayTile == kPackThreads * kPackPerThread, "four rows a thread");
static_assert(kPpayTile <= 65536, "a tile's rows are listed as u16");

// ---- the anchors -------------------------------------------------------------------------------
// The lowest row of each length among the tile's rows: an open-addressing table over the lengths.
// A row claims its length's slot with a compare-and-swap on the key (the first free slot from the
// hash on, or the one that already holds the length) and then takes the minimum on the slot's row.
// Which slot a length ends in depends on the order of arrival; the minimum under it does not.
struct PpayAnchorLds {
  uint32_t key[kPpaySlots];
  uint32_t row[kPpaySlots + 1];  // (the last: the length kPpayEmpty's)
};

// anchor[q] of this thread's rows 4 * tid + q, q < n_mine, from their lengths; tile-relative.  All
// kPackThreads threads call it; two __syncthreads inside, and the caller puts one before the table
// is used again.
__device__ __forceinline__ void ppay_anchors(const uint32_t len[kPackPerThread], uint32_t n_mine, PpayAnchorLds& l,
                                             uint32_t anchor[kPackPerThread]) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < kPpaySlots; i += kPackThreads) l.key[i] = kPpayEmpty, l.row[i] = kPpayEmpty;
  if (tid == 0) l.row[kPpaySlots] = kPpayEmpty;
  __syncthreads();
  uint32_t slot[kPackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    slot[q] = kPpaySlots;
    if (q >= n_mine) continue;
    if (len[q] != kPpayEmpty) {
      // (at most kPpayTile of kPpaySlots slots are ever taken: the probe ends)
      uint32_t h = ppay_hash(len[q]);
      for (;;) {
        const uint32_t prev = atomicCAS(&l.key[h], kPpayEmpty, len[q]);  // (LDS, this workgroup's own)
        if (prev == kPpayEmpty || prev == len[q]) break;
        h = (h + 1) & (kPpaySlots - 1);
      }
      slot[q] = h;
    }
    atomicMin(&l.row[slot[q]], tid * kPackPerThread + q);
  }
  __syncthreads();
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) anchor[q] = q < n_mine ? l.row[slot[q]] : tid * kPackPerThread + q;
}

// ---- rows --------------------------------------------------------------------------------------
// pos of this thread's rows k0 .. k0 + 3 and the end of the last: p[q] for q <= n_mine (the rows
// below n_rows), the rest equal to the last (rows of no bytes).  Returns n_mine.
__device__ __forceinline__ uint32_t ppay_pos5(const uint64_t* __restrict__ pos, uint64_t k0, uint64_t n_rows,
                                              uint64_t p[kPackPerThread + 1]) {
  const uint32_t n_mine = k0 < n_rows ? uint32_t(n_rows - k0 < kPackPerThread ? n_rows - k0 : kPackPerThread) : 0u;
  uint64_t last = 0;
#pragma unroll
  for (uint32_t q = 0; q <= kPackPerThread; ++q) {
    if (q <= n_mine && k0 < n_rows) last = pos[k0 + q];
    p[q] = last;
  }
  return n_mine;
}

// ---- the compare -------------------------------------------------------------------------------
// The first 16 bytes of the n >= 1 bytes at p; those at or past n are unspecified.  Neither row is
// aligned: only aligned 16-byte words that hold a byte of the range are loaded, so a load never
// leaves the pages the range lies on, and the bytes are realigned in registers.
__device__ __forceinline__ uint4 ppay_load16(const uint8_t* p, uint32_t n) {
  const uintptr_t a = (uintptr_t)p, q = a & ~(uintptr_t)15, end = a + n;
  const uint32_t m = uint32_t(a & 15);
  const uint4 lo = *reinterpret_cast<const uint4*>(q);
  uint4 hi = make_uint4(0, 0, 0, 0);
  if (m && q + 16 < end) hi = *reinterpret_cast<const uint4*>(q + 16);
  return m ? funnel16(lo, hi, m) : lo;
}
// The first of the leading min(16, n) bytes in which a and b differ; 16: none.
__device__ __forceinline__ uint32_t ppay_diff16(const uint8_t* a, const uint8_t* b, uint32_t n) {
  const uint4 x = ppay_load16(a, n), y = ppay_load16(b, n);
  const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
  uint32_t at = 16;
#pragma unroll
  for (int w = 3; w >= 0; --w) {
    const uint32_t left = n > 4u * w ? n - 4u * w : 0u;
    const uint32_t m = df_edge_mask(0, left < 4 ? left : 4u);
    const uint32_t d = df_first_diff(xs[w] & m, ys[w] & m);
    if (d < 4) at = 4u * w + d;
  }
  return at;
}
// lcp of two rows of n bytes, by one lane.
__device__ __forceinline__ uint32_t ppay_lcp_lane(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint64_t off = 0; off < n; off += 16) {
    const uint32_t d = ppay_diff16(a + off, b + off, uint32_t(n - off));
    if (d < 16) return uint32_t(off) + d;
  }
  return n;
}
// ... by a wave (arguments wave-uniform, the result too): 16 bytes a lane and round, a ballot of
// the lanes that found a difference, the lowest lane's offset.
__device__ __forceinline__ uint32_t ppay_lcp_wave(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t lane) {
  for (uint64_t base = 0; base < n; base += 1024) {
    const uint64_t off = base + uint64_t(lane) * 16;
    const uint32_t d = off < n ? ppay_diff16(a + off, b + off, uint32_t(n - off)) : 16u;
    const uint64_t found = __ballot(d < 16);
    if (found) {
      const uint32_t first = uint32_t(__builtin_ctzll(found));
      return uint32_t(base) + first * 16 + uint32_t(__shfl(int(d), int(first), 64));
    }
  }
  return n;
}

}  // namespace

// ---- the pack ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kPackThreads) void k_ppay_lcp(const uint8_t* __restrict__ var, const uint64_t* __restrict__ pos,
                                                           uint64_t n_rows, const PpayWork w) {
  __shared__ PpayAnchorLds al;
  __shared__ uint64_t s_pos[kPpayTile];   // the rows' starts
  __shared__ uint32_t s_len[kPpayTile];
  __shared__ uint32_t s_lcp[kPpayTile];
  __shared__ uint16_t s_anc[kPpayTile];
  __shared__ uint16_t s_long[kPpayTile];  // the rows a wave compares, in any order
  __shared__ int64_t s_lo[kPackWaves], s_hi[kPackWaves];
  __shared__ uint64_t s_sum[kPackWaves];
  __shared__ uint64_t s_bad;
  __shared__ uint32_t s_nlong;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t tile0 = uint64_t(blockIdx.x) * kPpayTile, k0 = tile0 + uint64_t(tid) * kPackPerThread;
  const uint32_t m = uint32_t(n_rows - tile0 < kPpayTile ? n_rows - tile0 : kPpayTile);
  const uint64_t n_var = pos[n_rows];  // no byte of var at or past it is read

  uint64_t p[kPackPerThread + 1];
  const uint32_t n_mine = ppay_pos5(pos, k0, n_rows, p);
  uint64_t b = kPpayNoRow;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q)
    if (q < n_mine && b == kPpayNoRow && ppay_row_bad(k0 + q, p[q], p[q + 1])) b = k0 + q;
  b = block_min<kPackThreads>(b);
  if (tid == 0) s_bad = b, s_nlong = 0;
  __syncthreads();
  const bool tile_bad = s_bad != kPpayNoRow;  // (uniform) then its lengths mean nothing: no byte of var is read

  uint32_t len[kPackPerThread], lcp[kPackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t r = tid * kPackPerThread + q;
    len[q] = tile_bad ? 0u : uint32_t(p[q + 1] - p[q]);
    lcp[q] = 0;
    s_pos[r] = p[q], s_len[r] = len[q], s_lcp[r] = 0;
  }
  if (!tile_bad) {
    uint32_t anchor[kPackPerThread];
    ppay_anchors(len, n_mine, al, anchor);  // (its barriers publish s_pos and s_len as well)
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) {
      const uint32_t r = tid * kPackPerThread + q;
      // (an anchor lies below its row in a tile without a bad row: its bytes end at or before p[q])
      if (q >= n_mine || anchor[q] == r || !len[q] || p[q + 1] > n_var) continue;
      if (len[q] < kPayWaveRow) {
        lcp[q] = ppay_lcp_lane(var + p[q], var + s_pos[anchor[q]], len[q]);
        s_lcp[r] = lcp[q];
      } else {
        const uint32_t i = atomicAdd(&s_nlong, 1u);  // (LDS, this workgroup's own)
        s_long[i] = uint16_t(r);
        s_anc[r] = uint16_t(anchor[q]);
      }
    }
    __syncthreads();
    const uint32_t n_long = s_nlong;
    for (uint32_t i = wv; i < n_long; i += kPackWaves) {
      const uint32_t r = s_long[i];
      const uint32_t c = ppay_lcp_wave(var + s_pos[r], var + s_pos[s_anc[r]], s_len[r], lane);
      if (lane == 0) s_lcp[r] = c;
    }
  }
  __syncthreads();
  uint64_t acc = 0;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q)
    if (q < n_mine) {
      const uint32_t c = s_lcp[tid * kPackPerThread + q];
      w.lcp[k0 + q] = c;
      acc += len[q] - c;
    }
  acc = wave_sum(acc);
  if (lane == 0) s_sum[wv] = acc;
  // the tile's block of the lcp stream, measured from LDS (pos: its payload's size)
  pack_block_measure<kElemU32, false>(PackAt{s_lcp, 0, m}, w.desc + blockIdx.x, nullptr, s_lo, s_hi);
  if (tid == 0) {  // (the measure's barrier is behind s_sum's writes)
    for (uint32_t k = 1; k < kPackWaves; ++k) acc += s_sum[k];
    w.tsum[blockIdx.x] = acc;
    w.bad[blockIdx.x] = s_bad;
  }
}

__global__ __launch_bounds__(kPackTopThreads) void k_ppay_scan(const PpayWork w, uint32_t n_tiles,
                                                               const uint64_t* __restrict__ pos, uint64_t n_rows,
                                                               PpayRes* __restrict__ res) {
  uint64_t b = kPpayNoRow;  // this thread's lowest bad row
  const auto tot = tile_scan<kPackTopThreads, 2, uint64_t>(
      n_tiles,
      [&](uint32_t t, uint64_t c[2]) {
        c[0] = w.tsum[t];
        c[1] = w.desc[t].pos;
        const uint64_t x = w.bad[t];
        b = x < b ? x : b;
      },
      [&](uint32_t t, const uint64_t before[2]) {
        w.tbase[t] = before[0];
        w.desc[t].pos = before[1];
      });
  b = block_min<kPackTopThreads>(b);
  if (threadIdx.x == 0) {
    res->n_tail = tot.v[0];
    res->n_bits = tot.v[1];
    res->n_var = pos[n_rows];
    res->bad_row = b;
    res->bad_block = res->bad_value = kPpayNoRow;
  }
}

__global__ __launch_bounds__(kPackThreads) void k_ppay_write(const uint8_t* __restrict__ var, const uint64_t* __restrict__ pos,
                                                             uint64_t n_rows, const PpayWork w, clg_pack_block* __restrict__ desc,
                                                             uint8_t* __restrict__ bits, uint8_t* __restrict__ tail,
                                                             uint64_t n_bits, uint64_t n_tail) {
  __shared__ unsigned long long s_w[kPackBlock];
  __shared__ uint64_t s_at[kPpayTile];    // the long tails' destinations
  __shared__ uint64_t s_ws[kPackWaves];
  __shared__ uint16_t s_long[kPpayTile];  // the tails a wave copies, in any order
  __shared__ uint32_t s_nlong;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t tile0 = uint64_t(blockIdx.x) * kPpayTile, k0 = tile0 + uint64_t(tid) * kPackPerThread;
  const uint32_t m = uint32_t(n_rows - tile0 < kPpayTile ? n_rows - tile0 : kPpayTile);
  if (tid == 0) s_nlong = 0;

  const clg_pack_block d = w.desc[blockIdx.x];
  if (tid == 0) desc[blockIdx.x] = d;
  pack_block_write<kElemU32, false>(PackAt{w.lcp, tile0, m}, d, s_w, bits, n_bits);
  __syncthreads();

  uint64_t p[kPackPerThread + 1];
  const uint32_t n_mine = ppay_pos5(pos, k0, n_rows, p);
  uint32_t lcp[kPackPerThread], left[kPackPerThread];
  uint64_t mine = 0;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t len = uint32_t(p[q + 1] - p[q]);
    lcp[q] = q < n_mine ? w.lcp[k0 + q] : 0u;
    left[q] = lcp[q] <= len ? len - lcp[q] : 0u;
    mine += left[q];
  }
  uint64_t at = w.tbase[blockIdx.x] + tile_excl<kPackWaves>(mine, tid, s_ws);
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t n = left[q];
    if (n && at + n <= n_tail) {  // (n_tail: the total that was checked against the capacity)
      if (n < kPayWaveRow) {
        const uint8_t* src = var + p[q] + lcp[q];
        uint8_t* dst = tail + at;
        for (uint32_t i = 0; i < n; ++i) dst[i] = src[i];
      } else {
        const uint32_t r = tid * kPackPerThread + q, i = atomicAdd(&s_nlong, 1u);  // (LDS, this workgroup's own)
        s_long[i] = uint16_t(r);
        s_at[r] = at;
      }
    }
    at += n;
  }
  __syncthreads();
  const uint32_t n_long = s_nlong;
  for (uint32_t i = wv; i < n_long; i += kPackWaves) {
    const uint32_t r = s_long[i];
    const uint64_t k = tile0 + r, from = pos[k];
    const uint32_t c = w.lcp[k], len = uint32_t(pos[k + 1] - from);
    copy_range<64>(var + from + c, tail + s_at[r], len - c, lane);
  }
}

// ---- the unpack --------------------------------------------------------------------------------

__global__ __launch_bounds__(kPackThreads) void k_ppay_in(const clg_pack_block* __restrict__ desc,
                                                          const uint8_t* __restrict__ bits, uint64_t n_bits,
                                                          const uint64_t* __restrict__ pos, uint64_t n_rows, const PpayWork w) {
  __shared__ PpayAnchorLds al;
  __shared__ unsigned long long s_w[kPackBlock + 2];
  __shared__ unsigned long long s_ws[kPackWaves];
  __shared__ uint64_t s_sum[kPackWaves];
  __shared__ clg_pack_block s_d;
  __shared__ uint32_t s_ok;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t tile0 = uint64_t(blockIdx.x) * kPpayTile, k0 = tile0 + uint64_t(tid) * kPackPerThread;
  if (tid == 0) {
    s_d = desc[blockIdx.x];
    s_ok = pack_block_in_ok(s_d, false, blockIdx.x, n_rows, n_bits) ? 1u : 0u;
  }
  __syncthreads();
  const bool block_ok = s_ok != 0;  // (uniform) no address is formed from a descriptor that failed
  uint64_t v[kPackPerThread] = {0, 0, 0, 0};
  if (block_ok) unpack_block_values<false>(s_d, bits, s_w, s_ws, v);

  uint64_t p[kPackPerThread + 1];
  const uint32_t n_mine = ppay_pos5(pos, k0, n_rows, p);
  uint32_t len[kPackPerThread], anchor[kPackPerThread];
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) len[q] = uint32_t(p[q + 1] - p[q]);
  // (the lengths of a tile with a bad row mean nothing; nothing is addressed by them here)
  ppay_anchors(len, n_mine, al, anchor);
  bool finding = false;
  uint64_t acc = 0;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    if (q >= n_mine) continue;
    const bool row_bad = ppay_row_bad(k0 + q, p[q], p[q + 1]) || v[q] > p[q + 1] - p[q] ||
                         (anchor[q] == tid * kPackPerThread + q && v[q] != 0);
    finding = finding || row_bad;
    if (!row_bad) acc += p[q + 1] - p[q] - v[q];
    w.lcp[k0 + q] = uint32_t(v[q]);
  }
  acc = wave_sum(acc);
  if (lane == 0) s_sum[wv] = acc;
  const uint32_t none = block_min<kPackThreads>(finding ? 0u : 1u);  // (its barrier is behind s_sum's writes)
  if (tid == 0) {
    for (uint32_t k = 1; k < kPackWaves; ++k) acc += s_sum[k];
    w.tsum[blockIdx.x] = acc;
    w.bad[2 * uint64_t(blockIdx.x)] = block_ok ? kPpayNoRow : uint64_t(blockIdx.x);
    w.bad[2 * uint64_t(blockIdx.x) + 1] = none ? kPpayNoRow : uint64_t(blockIdx.x);
  }
}

__global__ __launch_bounds__(kPackTopThreads) void k_ppay_in_scan(const PpayWork w, uint32_t n_tiles,
                                                                  const uint64_t* __restrict__ pos, uint64_t n_rows,
                                                                  PpayRes* __restrict__ res) {
  uint64_t bb = kPpayNoRow, bv = kPpayNoRow;  // this thread's lowest findings
  const auto tot = tile_scan<kPackTopThreads, 1, uint64_t>(
      n_tiles,
      [&](uint32_t t, uint64_t c[1]) {
        c[0] = w.tsum[t];
        const uint64_t x = w.bad[2 * uint64_t(t)], y = w.bad[2 * uint64_t(t) + 1];
        bb = x < bb ? x : bb;
        bv = y < bv ? y : bv;
      },
      [&](uint32_t t, const uint64_t before[1]) { w.tbase[t] = before[0]; });
  bb = block_min<kPackTopThreads>(bb);
  __syncthreads();  // (block_min's words are written again)
  bv = block_min<kPackTopThreads>(bv);
  if (threadIdx.x == 0) {
    res->n_tail = tot.v[0];
    res->n_bits = 0;
    res->n_var = pos[n_rows];
    res->bad_row = kPpayNoRow;
    res->bad_block = bb;
    res->bad_value = bv;
  }
}

__global__ __launch_bounds__(kPackThreads) void k_ppay_out(const uint8_t* __restrict__ tail, const uint64_t* __restrict__ pos,
                                                           uint64_t n_rows, const PpayWork w, uint8_t* __restrict__ var,
                                                           uint64_t n_tail, uint64_t n_var) {
  __shared__ PpayAnchorLds al;
  __shared__ uint64_t s_toff[kPpayTile];  // the rows' tail offsets: a row's own, and its anchor's
  __shared__ uint64_t s_ws[kPackWaves];
  __shared__ uint16_t s_anc[kPpayTile];
  __shared__ uint16_t s_long[kPpayTile];  // the rows a wave copies, in any order
  __shared__ uint32_t s_nlong;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t tile0 = uint64_t(blockIdx.x) * kPpayTile, k0 = tile0 + uint64_t(tid) * kPackPerThread;
  if (tid == 0) s_nlong = 0;

  uint64_t p[kPackPerThread + 1];
  const uint32_t n_mine = ppay_pos5(pos, k0, n_rows, p);
  uint32_t len[kPackPerThread], lcp[kPackPerThread], anchor[kPackPerThread];
  uint64_t mine = 0;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    len[q] = uint32_t(p[q + 1] - p[q]);
    lcp[q] = q < n_mine ? w.lcp[k0 + q] : 0u;
    if (lcp[q] > len[q]) lcp[q] = len[q];  // (the check passed: only an input that changed under the call)
    mine += len[q] - lcp[q];
  }
  uint64_t at = w.tbase[blockIdx.x] + tile_excl<kPackWaves>(mine, tid, s_ws);
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    s_toff[tid * kPackPerThread + q] = at;
    at += len[q] - lcp[q];
  }
  ppay_anchors(len, n_mine, al, anchor);  // (its barriers publish s_toff and s_nlong as well)
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t r = tid * kPackPerThread + q, L = len[q], c = lcp[q];
    if (q >= n_mine || !L) continue;
    const uint64_t own = s_toff[r], pre = s_toff[anchor[q]];
    // (n_tail and n_var: the totals that were checked; an anchor's tail is a whole row of L bytes)
    if (p[q] + L > n_var || own + (L - c) > n_tail || pre + c > n_tail) continue;
    if (L < kPayWaveRow) {
      uint8_t* dst = var + p[q];
      const uint8_t *s0 = tail + pre, *s1 = tail + own;
      for (uint32_t i = 0; i < c; ++i) dst[i] = s0[i];
      for (uint32_t i = 0; i < L - c; ++i) dst[c + i] = s1[i];
    } else {
      const uint32_t i = atomicAdd(&s_nlong, 1u);  // (LDS, this workgroup's own)
      s_long[i] = uint16_t(r);
      s_anc[r] = uint16_t(anchor[q]);
    }
  }
  __syncthreads();
  const uint32_t n_long = s_nlong;
  for (uint32_t i = wv; i < n_long; i += kPackWaves) {
    const uint32_t r = s_long[i];
    const uint64_t k = tile0 + r, to = pos[k];
    const uint32_t L = uint32_t(pos[k + 1] - to), c0 = w.lcp[k], c = c0 < L ? c0 : L;
    if (to + L > n_var || s_toff[r] + (L - c) > n_tail || s_toff[s_anc[r]] + c > n_tail) continue;
    copy_range<64>(tail + s_toff[s_anc[r]], var + to, c, lane);
    copy_range<64>(tail + s_toff[r], var + to + c, L - c, lane);
  }
}

// ---- launches ----------------------------------------------------------------------------------

int launch_ppay_lcp_scan(const uint8_t* var, const uint64_t* pos, uint64_t n_rows, uint32_t n_tiles, const PpayWork& w,
                         PpayRes* res, void* stream) {
  hipLaunchKernelGGL(k_ppay_lcp, dim3(n_tiles), dim3(kPackThreads), 0, (hipStream_t)stream, var, pos, n_rows, w);
  hipLaunchKernelGGL(k_ppay_scan, dim3(1), dim3(kPackTopThreads), 0, (hipStream_t)stream, w, n_tiles, pos, n_rows, res);
  return launch_status(hipGetLastError());
}

int launch_ppay_write(const uint8_t* var, const uint64_t* pos, uint64_t n_rows, uint32_t n_tiles, const PpayWork& w,
                      clg_pack_block* desc, uint8_t* bits, uint8_t* tail, uint64_t n_bits, uint64_t n_tail, void* stream) {
  hipLaunchKernelGGL(k_ppay_write, dim3(n_tiles), dim3(kPackThreads), 0, (hipStream_t)stream, var, pos, n_rows, w, desc, bits,
                     tail, n_bits, n_tail);
  return launch_status(hipGetLastError());
}

int launch_ppay_in_scan(const clg_pack_block* desc, const uint8_t* bits, uint64_t n_bits, const uint64_t* pos, uint64_t n_rows,
                        uint32_t n_tiles, const PpayWork& w, PpayRes* res, void* stream) {
  hipLaunchKernelGGL(k_ppay_in, dim3(n_tiles), dim3(kPackThreads), 0, (hipStream_t)stream, desc, bits, n_bits, pos, n_rows, w);
  hipLaunchKernelGGL(k_ppay_in_scan, dim3(1), dim3(kPackTopThreads), 0, (hipStream_t)stream, w, n_tiles, pos, n_rows, res);
  return launch_status(hipGetLastError());
}

int launch_ppay_out(const uint8_t* tail, const uint64_t* pos, uint64_t n_rows, uint32_t n_tiles, const PpayWork& w,
                    uint8_t* var, uint64_t n_tail, uint64_t n_var, void* stream) {
  hipLaunchKernelGGL(k_ppay_out, dim3(n_tiles), dim3(kPackThreads), 0, (hipStream_t)stream, tail, pos, n_rows, w, var, n_tail,
                     n_var);
  return launch_status(hipGetLastError());
}

}  // namespace clg
