// pack_dev.h -- what the kernels of pack.hip, pack_wide.hip, unpack.hip and unpack_wide.hip share
// on the device: the workgroup's shape, the wave's signed minimum / maximum by DPP, and the block
// codec's measure, write and decode, instantiated on (element, scheme).  The wave scans and the
// one-workgroup scan are wave_dev.h's.
// Device code only, file-local in each unit that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pack.h"
#include "wave_dev.h"

namespace clg {
namespace {

constexpr uint32_t kPackThreads = 256;
constexpr uint32_t kPackWaves = kPackThreads / 64;
constexpr uint32_t kPackPerThread = kPackBlock / kPackThreads;
constexpr uint32_t kPackTopThreads = 1024;
static_assert(kPackPerThread == 4, "four values a thread");
static_assert(kPackScanGroup == kPackThreads, "the group passes take a block a thread");

// v of the lane the DPP control names; a lane without a source keeps its own.
template <int kCtrl>
__device__ __forceinline__ int64_t pack_dpp(int64_t v) {
  const uint32_t lo = uint32_t(uint64_t(v)), hi = uint32_t(uint64_t(v) >> 32);
  const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp((int)lo, (int)lo, kCtrl, 0xF, 0xF, false);
  const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp((int)hi, (int)hi, kCtrl, 0xF, 0xF, false);
  return int64_t(uint64_t(a) | uint64_t(b) << 32);
}
__device__ __forceinline__ int64_t pack_lane63(int64_t v) {
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)uint32_t(uint64_t(v)), 63);
  const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)uint32_t(uint64_t(v) >> 32), 63);
  return int64_t(uint64_t(a) | uint64_t(b) << 32);
}
__device__ __forceinline__ int64_t pack_min(int64_t a, int64_t b) { return b < a ? b : a; }
__device__ __forceinline__ int64_t pack_max(int64_t a, int64_t b) { return b > a ? b : a; }
// The wave's signed minimum / maximum: quads, the rows of 16 (row_ror 4 and 8), then
// row_bcast 15 and 31; lane 63 holds the result.
#define CLG_PACK_WAVE_REDUCE(op, v)       \
  v = op(v, pack_dpp<0xB1>(v));           \
  v = op(v, pack_dpp<0x4E>(v));           \
  v = op(v, pack_dpp<0x124>(v));          \
  v = op(v, pack_dpp<0x128>(v));          \
  v = op(v, pack_dpp<0x142>(v));          \
  v = op(v, pack_dpp<0x143>(v));          \
  v = pack_lane63(v)

// ---- the block codec on the device: a workgroup of kPackThreads per block ----------------------

// A block's place, which each unit finds in its own way: its stream's array, the block's first
// value and how many it holds.
struct PackAt {
  const void* col;
  uint64_t i0;
  uint32_t m;
};
// Block blk of a stream of n values in col whose first block is `base`.
__device__ __forceinline__ PackAt pack_at(const void* col, uint64_t n, uint64_t base, uint64_t blk) {
  const uint64_t i0 = (blk - base) * kPackBlock;
  const uint64_t left = i0 < n ? n - i0 : 0;
  return PackAt{col, i0, uint32_t(left < kPackBlock ? left : kPackBlock)};
}
// The measure: four coalesced values a thread, the DELTA predecessor through LDS (s_x: kPackBlock
// words), the residuals' signed minimum and maximum by the wave reduction and LDS across the waves
// (s_lo, s_hi: a word a wave); thread 0 writes ref, first, width, count and, in pos, the payload's
// size to *slot (global memory or LDS).  The element and the scheme are constants in each instance.
// A caller that measures block after block in one workgroup puts a __syncthreads between two
// calls: thread 0 reads s_lo and s_hi last.
template <uint32_t kElem, bool kDelta>
__device__ __forceinline__ void pack_block_measure(const PackAt at, clg_pack_block* slot, int64_t* s_x, int64_t* s_lo,
                                                   int64_t* s_hi) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t x[kPackPerThread];
#pragma unroll
  for (uint32_t k = 0; k < kPackPerThread; ++k) {
    const uint32_t i = k * kPackThreads + tid;
    x[k] = i < at.m ? pack_load(kElem, at.col, at.i0 + i) : 0;
  }
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  if (kDelta) {
#pragma unroll
    for (uint32_t k = 0; k < kPackPerThread; ++k) s_x[k * kPackThreads + tid] = x[k];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPackPerThread; ++k) {
      const uint32_t i = k * kPackThreads + tid;
      if (i >= 1 && i < at.m) {
        const int64_t r = int64_t(uint64_t(x[k]) - uint64_t(s_x[i - 1]));
        lo = pack_min(lo, r), hi = pack_max(hi, r);
      }
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kPackPerThread; ++k)
      if (k * kPackThreads + tid < at.m) lo = pack_min(lo, x[k]), hi = pack_max(hi, x[k]);
  }
  CLG_PACK_WAVE_REDUCE(pack_min, lo);
  CLG_PACK_WAVE_REDUCE(pack_max, hi);
  if (lane == 0) s_lo[w] = lo, s_hi[w] = hi;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (uint32_t j = 1; j < kPackWaves; ++j) lo = pack_min(lo, s_lo[j]), hi = pack_max(hi, s_hi[j]);
    const uint32_t k = pack_residuals(kDelta, at.m);
    clg_pack_block d;
    d.ref = k ? lo : 0;
    d.first = kDelta && at.m ? x[0] : 0;  // (thread 0's first value is the block's)
    d.width = k ? pack_width(uint64_t(hi) - uint64_t(lo)) : 0;
    d.count = at.m;
    d.pos = pack_payload_bytes(k, d.width);  // the size; the scan turns it into the offset
    *slot = d;
  }
}

// The write: the values reloaded, p_i formed, the payload assembled in LDS and stored with one
// aligned 16-byte store a lane, below lim_bits.  s_w: 8 KiB, the block's values (the DELTA
// predecessors), then the payload's words.
template <uint32_t kElem, bool kDelta>
__device__ __forceinline__ void pack_block_write(const PackAt at, const clg_pack_block d, unsigned long long* s_w,
                                                 uint8_t* __restrict__ bits, uint64_t lim_bits) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t k = pack_residuals(kDelta, at.m), width = d.width;
  const uint32_t bytes = pack_payload_bytes(k, width);
  if (!bytes) return;  // (uniform: a constant block, or a DELTA block of one value)
  const uint32_t n_words = bytes / 8;
  uint64_t p[kPackPerThread];
  uint32_t j[kPackPerThread];  // the residual's index; >= k: none
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t i = q * kPackThreads + tid;
    p[q] = i < at.m ? uint64_t(pack_load(kElem, at.col, at.i0 + i)) : 0;
    j[q] = i < at.m ? i : kPackBlock;
  }
  if (kDelta) {
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) s_w[q * kPackThreads + tid] = p[q];
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) {
      const uint32_t i = q * kPackThreads + tid;
      if (i >= 1 && i < at.m) p[q] -= s_w[i - 1], j[q] = i - 1;
      else j[q] = kPackBlock;
    }
    __syncthreads();  // (s_w is written again below)
  }
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) p[q] -= uint64_t(d.ref);

  if (width == 64) {  // a word a value: no shifts
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q)
      if (j[q] < k) s_w[j[q]] = p[q];
    if (tid == 0 && (k & 1)) s_w[k] = 0;  // the padding word
  } else if (width == 1 && !kDelta) {  // a wave's 64 values are one word: a ballot
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) {
      const uint64_t m = __ballot(j[q] < k && (p[q] & 1));
      const uint32_t word = q * kPackWaves + wv;
      if (lane == 0 && word < n_words) s_w[word] = m;
    }
  } else {
    for (uint32_t i = tid; i < n_words; i += kPackThreads) s_w[i] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q)
      if (j[q] < k) {
        const uint32_t bit = j[q] * width, sh = bit & 63;
        atomicOr(&s_w[bit >> 6], (unsigned long long)(p[q] << sh));
        if (sh + width > 64) atomicOr(&s_w[(bit >> 6) + 1], (unsigned long long)(p[q] >> (64 - sh)));  // (sh > 0)
      }
  }
  __syncthreads();
  for (uint32_t i = tid; i < bytes / 16; i += kPackThreads) {
    const uint64_t a = d.pos + uint64_t(i) * 16;
    if (a + 16 <= lim_bits) {
      const unsigned long long lo = s_w[2 * i], hi = s_w[2 * i + 1];
      *reinterpret_cast<uint4*>(bits + a) = make_uint4(uint32_t(lo), uint32_t(lo >> 32), uint32_t(hi), uint32_t(hi >> 32));
    }
  }
}

// ---- the block codec's decode on the device ----------------------------------------------------

// Residual j's p from 64-bit words, 1 <= w <= 63: no shift by 64 (sh + w > 64 implies sh > 0), and
// the second word is read only when the value reaches into it, so never past the payload.
__device__ __forceinline__ uint64_t unpack_bits(const unsigned long long* words, uint32_t w, uint32_t j) {
  const uint32_t bit = j * w, sh = bit & 63;
  uint64_t v = words[bit >> 6] >> sh;
  if (sh + w > 64) v |= uint64_t(words[(bit >> 6) + 1]) << (64 - sh);
  return v & ((uint64_t(1) << w) - 1);
}
__device__ __forceinline__ uint64_t unpack_resid(const unsigned long long* words, uint32_t w, uint32_t j) {
  return w == 0 ? 0 : w == 64 ? uint64_t(words[j]) : unpack_bits(words, w, j);
}

// Every value of a well-formed block inside [lo, hi]?  A wave per block, the payload read from
// global memory in place.  FOR: the lanes take the values 64 apart.  DELTA: 64 consecutive values a
// round, the wave's inclusive scan of first and the residuals, the carry from lane 63.
template <bool kDelta>
__device__ __forceinline__ bool unpack_values_in(const clg_pack_block& d, const uint8_t* __restrict__ bits, uint32_t lane,
                                                 int64_t lo, int64_t hi) {
  const unsigned long long* words = reinterpret_cast<const unsigned long long*>(bits + d.pos);
  const uint32_t w = d.width;
  bool ok = true;
  if (!kDelta) {
    for (uint32_t i = lane; i < d.count; i += 64) {
      const int64_t x = int64_t(unpack_resid(words, w, i) + uint64_t(d.ref));
      ok = ok && x >= lo && x <= hi;
    }
  } else {
    uint64_t carry = 0;
    for (uint32_t i0 = 0; i0 < d.count; i0 += 64) {  // (wave-uniform)
      const uint32_t i = i0 + lane;
      uint64_t r = 0;
      if (i == 0) r = uint64_t(d.first);
      else if (i < d.count) r = unpack_resid(words, w, i - 1) + uint64_t(d.ref);
      const uint64_t x = carry + wave_incl(r, lane);
      ok = ok && (i >= d.count || (int64_t(x) >= lo && int64_t(x) <= hi));
      carry = uint64_t(pack_lane63(int64_t(x)));
    }
  }
  return __ballot(!ok) == 0;
}

// Four consecutive values to col[at .. at + n) (n <= 4) in the element's type: one store of four
// elements where all four are there and the column allows it (wide), else an element at a time.
template <uint32_t kElem>
__device__ __forceinline__ void unpack_store4(void* col, uint64_t at, const uint64_t v[4], uint32_t n, bool wide) {
  if (kElem == kElemI64) {
    int64_t* dst = static_cast<int64_t*>(col) + at;
    if (n == 4 && wide) {
      reinterpret_cast<ulonglong2*>(dst)[0] = make_ulonglong2(v[0], v[1]);
      reinterpret_cast<ulonglong2*>(dst)[1] = make_ulonglong2(v[2], v[3]);
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
        if (q < n) dst[q] = int64_t(v[q]);
    }
  } else if (kElem == kElemI32 || kElem == kElemU32) {
    uint32_t* dst = static_cast<uint32_t*>(col) + at;
    if (n == 4 && wide) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3]));
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
        if (q < n) dst[q] = uint32_t(v[q]);
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

// A well-formed block's values, four consecutive ones a thread (v[q] is value 4 * tid + q; those at
// or past count are not values): the payload (at most 8 KiB) staged in LDS with aligned 16-byte
// loads (bits is 16-byte aligned, pos a multiple of 16), FOR adds ref, DELTA takes the inclusive
// prefix sum of first and the residuals, modulo 2^64: the thread's four, the wave scan, the four
// waves through LDS.  s_w: the payload's words (8 KiB and one spare pair); s_ws: the waves' sums.
template <bool kDelta>
__device__ __forceinline__ void unpack_block_values(const clg_pack_block d, const uint8_t* __restrict__ bits,
                                                    unsigned long long* s_w, unsigned long long* s_ws,
                                                    uint64_t v[kPackPerThread]) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t m = d.count, k = pack_residuals(kDelta, m), width = d.width;
  const uint32_t n16 = pack_payload_bytes(k, width) / 16;
  const uint4* src = reinterpret_cast<const uint4*>(bits + d.pos);
  for (uint32_t i = tid; i < n16; i += kPackThreads) reinterpret_cast<uint4*>(s_w)[i] = src[i];
  if (n16) __syncthreads();  // (uniform)

  const uint32_t first_i = tid * kPackPerThread;
#pragma unroll
  for (uint32_t q = 0; q < kPackPerThread; ++q) {
    const uint32_t i = first_i + q;
    // the residual's index: FOR i, DELTA i - 1 (value 0 is `first`)
    const bool has = kDelta ? (i >= 1 && i < m) : i < m;
    const uint32_t j = kDelta ? i - 1 : i;
    uint64_t p = 0;
    if (has) {
      if (width == 64) p = s_w[j];  // (the widths 0 and 64 are uniform cases: no shifts)
      else if (width) p = unpack_bits(s_w, width, j);
      p += uint64_t(d.ref);
    }
    v[q] = kDelta && i == 0 ? uint64_t(d.first) : p;
  }
  if (kDelta) {
    v[1] += v[0], v[2] += v[1], v[3] += v[2];
    const uint64_t incl = wave_incl(v[3], lane);
    if (lane == 63) s_ws[wv] = incl;
    __syncthreads();
    uint64_t before = incl - v[3];
#pragma unroll
    for (uint32_t w2 = 0; w2 < kPackWaves; ++w2) before += w2 < wv ? uint64_t(s_ws[w2]) : 0;
#pragma unroll
    for (uint32_t q = 0; q < kPackPerThread; ++q) v[q] += before;
  }
}

// The write: the block's values stored coalesced to col[i0 .. i0 + count).
template <uint32_t kElem, bool kDelta>
__device__ __forceinline__ void unpack_block_write(void* col, uint64_t i0, const clg_pack_block d,
                                                   const uint8_t* __restrict__ bits, unsigned long long* s_w,
                                                   unsigned long long* s_ws) {
  uint64_t v[kPackPerThread];
  unpack_block_values<kDelta>(d, bits, s_w, s_ws, v);
  const uint32_t first_i = threadIdx.x * kPackPerThread, m = d.count;
  const uint32_t n = first_i < m ? (m - first_i < 4 ? m - first_i : 4) : 0;
  constexpr uint32_t kWide = kElem == kElemU8 || kElem == kElemI8 ? 4 : 16;
  const bool wide = (reinterpret_cast<uintptr_t>(col) & (kWide - 1)) == 0;  // (uniform; i0 keeps the alignment)
  if (n) unpack_store4<kElem>(col, i0 + first_i, v, n, wide);
}

}  // namespace
}  // namespace clg
