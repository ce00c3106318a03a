// digest.hip -- the log digest (digest.h) of many spans, computed where the bytes live.
//
//  * k_digest_pieces   pass 1: a wave per piece (a source pointer, the logical offset of its first
//                      byte in the packed order, a length that never crosses a segment; what
//                      k_expand_pieces produces from SegSpan runs) -> one partial per piece,
//                      already weighted by R^(words after the piece in its span)
//  * k_digest_runs     pass 2: a wave per run adds its pieces' partials (contiguous) mod p and
//                      writes {hash, len}
//
// No atomics, no spin waits and no word taken from another running workgroup: the kernel
// boundary orders the two passes, and the result is deterministic.
//
// Pass 1 reads aligned 16-byte words and only those that hold a byte of the piece (as the
// gather's copy_range does), so it never leaves the pages the piece lies on.  A lane's window is
// 32 physical bytes at a 16-byte-aligned address; the span's logical words sit at a constant
// byte shift s = (physical - logical) mod 4 inside it (segment boundaries are multiples of 4, so
// s is constant over a run), and the nine dwords of a window realign to eight logical words
// with v_alignbit.  Bytes outside the piece are masked to zero: a word straddling two segments
// is two masked words, one in each piece, with the same weight.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "digest.h"
#include "kernels.h"

namespace clg {

namespace {

constexpr uint32_t kWinWords = 8;                  // logical words per lane window (32 bytes)
constexpr uint32_t kIterWords = 64 * kWinWords;    // words a wave covers per iteration

__device__ __forceinline__ uint32_t dg_find_run(const SegSpan* spans, uint32_t n, uint32_t g) {
  uint32_t lo = 0, hi = n;  // last run with first <= g
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (spans[mid].first <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// The aligned dword at address x with the bytes outside [src, end) cleared.
__device__ __forceinline__ uint32_t mask_dword(uint32_t v, uintptr_t x, uintptr_t src, uintptr_t end) {
  const uint32_t lo = x < src ? (src - x < 4 ? (uint32_t)(src - x) : 4u) : 0u;
  const uint32_t hi = x + 4 <= end ? 4u : (end > x ? (uint32_t)(end - x) : 0u);
  if (lo >= hi) return 0u;
  const uint32_t below_hi = hi == 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1u;
  return v & below_hi & ~((1u << (8 * lo)) - 1u);  // lo < hi <= 4, so the shift is below 32
}

// Loads by address, from global memory (an integer cast to a plain pointer would be a flat load).
typedef uint32_t dg_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) dg_u32x4* g_u32x4_p;
typedef const __attribute__((address_space(1))) uint32_t* g_u32_p;
__device__ __forceinline__ uint4 load16(uintptr_t a) {
  const dg_u32x4 v = *(g_u32x4_p)a;
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint32_t load4(uintptr_t a) { return *(g_u32_p)a; }

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  return (uint64_t)__shfl_xor((unsigned long long)v, m, 64);
}

}  // namespace

__global__ __launch_bounds__(256) void k_digest_pieces(const GatherPiece* __restrict__ pieces, uint32_t n_pieces,
                                                       const SegSpan* __restrict__ runs, uint32_t n_runs,
                                                       const uint64_t* __restrict__ tab,
                                                       uint64_t* __restrict__ partial) {
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (g >= n_pieces) return;  // (wave-uniform)
  const GatherPiece pc = pieces[g];
  if (pc.len == 0) {
    if (lane == 0) partial[g] = 0;
    return;
  }
  const SegSpan r = runs[dg_find_run(runs, n_runs, g)];
  const uint32_t a = (uint32_t)(pc.dst - r.dst);  // the piece's first byte in its span
  const uint32_t m = (r.len + 3u) >> 2;           // the span's words
  const uint32_t k1 = (a + pc.len - 1u) >> 2;     // the piece's last logical word
  const uintptr_t src = (uintptr_t)pc.src, end = src + pc.len;
  const uintptr_t vbase = src - (a & 3u);         // where the piece's first logical word starts
  const uintptr_t q0 = vbase & ~(uintptr_t)15;
  const uint32_t s = (uint32_t)(vbase & 3u), s8 = 8u * s;
  // virtual word i sits at q0 + s + 4 i; those before the piece's first word mask to zero
  const uint32_t nw = (uint32_t)((end - q0 - s + 3u) >> 2);
  const uint32_t nwin = (nw + kWinWords - 1u) / kWinWords;
  const uint32_t rem = nw - kWinWords * (nwin - 1u);  // words of the last window, 1..8
  // between a lane's windows lie 64 windows' words; before the (shorter) last window, fewer
  const uint64_t r_iter = tab[kDigestTabIter];
  const uint64_t r_last = dg_mul(tab[kDigestTabWin + 63], tab[kDigestTabOne + rem]);

  uint64_t acc = 0;
  uint32_t jl = 0;
  for (uint32_t j = lane; j < nwin; j += 64u) {
    const uintptr_t q = q0 + 32u * (uintptr_t)j;
    uint32_t d[kWinWords + 1];
#pragma unroll
    for (uint32_t t = 0; t <= kWinWords; ++t) d[t] = 0;
    if (q + 16 > src && q < end) {
      const uint4 v = load16(q);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    if (q + 32 > src && q + 16 < end) {
      const uint4 v = load16(q + 16);
      d[4] = v.x; d[5] = v.y; d[6] = v.z; d[7] = v.w;
    }
    if (s && q + 36 > src && q + 32 < end) d[8] = load4(q + 32);
    if (q < src || q + 36 > end) {  // a window at the piece's edge
#pragma unroll
      for (uint32_t t = 0; t <= kWinWords; ++t) d[t] = mask_dword(d[t], q + 4u * t, src, end);
    }
    uint64_t h = 0;
    if (j + 1u < nwin) {
#pragma unroll
      for (uint32_t t = 0; t < kWinWords; ++t)
        h = dg_step_lazy(h, (uint32_t)((((uint64_t)d[t + 1] << 32) | d[t]) >> s8));
    } else {  // the last window: no step for a word past the piece
#pragma unroll
      for (uint32_t t = 0; t < kWinWords; ++t)
        if (t < rem) h = dg_step_lazy(h, (uint32_t)((((uint64_t)d[t + 1] << 32) | d[t]) >> s8));
    }
    h = dg_reduce(h);  // (the chain's steps leave h below 2^63, not below p)
    acc = dg_add(dg_mul(acc, j + 1u < nwin ? r_iter : r_last), h);
    jl = j;
  }
  // weight the lane by R^(words after its last window in the piece)
  if (lane < nwin && jl + 1u < nwin)
    acc = dg_mul(acc, dg_mul(tab[kDigestTabWin + (nwin - 2u - jl)], tab[kDigestTabOne + rem]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = dg_add(acc, shfl_xor64(acc, o));
  // R^(words after the piece in its span): lane j holds the ladder entry of exponent bit j
  const uint32_t e = m - 1u - k1;
  uint64_t f = (lane < (uint32_t)kDigestLadder && ((e >> lane) & 1u)) ? tab[lane] : 1u;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) f = dg_mul(f, shfl_xor64(f, o));
  if (lane == 0) partial[g] = dg_mul(acc, f);
}

__global__ __launch_bounds__(256) void k_digest_runs(const SegSpan* __restrict__ runs, uint32_t n_runs,
                                                     uint32_t n_pieces, const uint64_t* __restrict__ partial,
                                                     clg_digest* __restrict__ out) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (w >= n_runs) return;
  const SegSpan r = runs[w];
  const uint32_t p1 = w + 1u < n_runs ? runs[w + 1u].first : n_pieces;
  uint64_t acc = 0;
  for (uint32_t i = r.first + lane; i < p1; i += 64u) acc = dg_add(acc, partial[i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = dg_add(acc, shfl_xor64(acc, o));
  if (lane == 0) out[r.pad] = clg_digest{acc, r.len};
}

void digest_table(uint64_t* tab) {
  dg_ladder(tab);
  for (uint32_t q = 0; q < 64; ++q) tab[kDigestTabWin + q] = dg_pow(kWinWords * q);
  for (uint32_t k = 0; k <= kWinWords; ++k) tab[kDigestTabOne + k] = dg_pow(k);
  tab[kDigestTabIter] = dg_pow(kIterWords);
}

int launch_digest(const GatherPiece* d_pieces, uint32_t n_pieces, const SegSpan* d_runs, uint32_t n_runs,
                  const uint64_t* d_tab, uint64_t* d_partial, clg_digest* d_out, void* stream) {
  if (!n_pieces || !n_runs) return CLG_OK;
  hipLaunchKernelGGL(k_digest_pieces, dim3((n_pieces + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_pieces, n_pieces,
                     d_runs, n_runs, d_tab, d_partial);
  hipLaunchKernelGGL(k_digest_runs, dim3((n_runs + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_runs, n_runs, n_pieces,
                     d_partial, d_out);
  return launch_status(hipGetLastError());
}

}  // namespace clg
