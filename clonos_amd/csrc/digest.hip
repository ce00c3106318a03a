// digest.hip -- the log digest (digest.h) of many spans, computed where the bytes live.
//
//  * k_digest_pieces   pass 1: a wave per piece (a source pointer, the logical offset of its first
//                      byte in the packed order, a length that never crosses a segment; what
//                      k_expand_pieces produces from SegSpan runs) -> one partial per piece,
//                      already weighted by R^(words after the piece in its span)
//  * k_digest_runs     pass 2: a wave per run adds its pieces' partials (contiguous) mod p and
//                      writes {hash, len}
//
// Prefix digests (digest.h, "prefix digests": a range's digest at many cuts) run the same two
// passes over stretches -- a run per non-empty stretch between two cuts, digested in the range's
// word frame: kLead instantiations, where a run has a lead-in of (previous cut) mod 4 zero
// bytes and pass 2 writes the stretch's sum S to a scratch word -- and then
//  * k_digest_chain    pass 3: a wave per request evaluates D_j = D_{j-1} R^dm_j + S_j over its
//                      cuts, 64 cuts per round by a scan of (multiplier, addend) maps, and writes
//                      {D_j, min(cut, len)} per cut; k_digest_chain_short, a thread per request
//                      walking its cuts in turn, serves calls whose requests all have few cuts
//
// No atomics, no spin waits and no word taken from another running workgroup: the kernel
// boundaries order the passes, and the result is deterministic.
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

// kLead: the runs are stretches of prefix digests, run k with lead[k] zero bytes in front of it
// (the whole-log digest runs the instantiation without: no load, no add).
template <bool kLead>
__global__ __launch_bounds__(256) void k_digest_pieces(const GatherPiece* __restrict__ pieces, uint32_t n_pieces,
                                                       const SegSpan* __restrict__ runs, uint32_t n_runs,
                                                       const uint32_t* __restrict__ lead,
                                                       const uint64_t* __restrict__ tab,
                                                       uint64_t* __restrict__ partial) {
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (g >= n_pieces) return;  // (wave-uniform)
  const GatherPiece pc = pieces[g];
  if (pc.len == 0) {
    if (lane == 0) partial[g] = 0;
    return;
  }
  const uint32_t ri = dg_find_run(runs, n_runs, g);
  const SegSpan r = runs[ri];
  const uint32_t ld = kLead ? lead[ri] : 0u;
  const uint32_t a = (uint32_t)(pc.dst - r.dst) + ld;  // the piece's first byte in its span (its frame)
  const uint32_t m = (r.len + ld + 3u) >> 2;           // the span's (the frame's) words
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

// kSum: write the run's sum to sums[run index] (a stretch's S) instead of a row to out[run.pad]
template <bool kSum>
__global__ __launch_bounds__(256) void k_digest_runs(const SegSpan* __restrict__ runs, uint32_t n_runs,
                                                     uint32_t n_pieces, const uint64_t* __restrict__ partial,
                                                     clg_digest* __restrict__ out, uint64_t* __restrict__ sums) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (w >= n_runs) return;
  const SegSpan r = runs[w];
  const uint32_t p1 = w + 1u < n_runs ? runs[w + 1u].first : n_pieces;
  uint64_t acc = 0;
  for (uint32_t i = r.first + lane; i < p1; i += 64u) acc = dg_add(acc, partial[i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = dg_add(acc, shfl_xor64(acc, o));
  if (lane == 0) {
    if (kSum) sums[w] = acc;
    else out[r.pad] = clg_digest{acc, r.len};
  }
}

namespace {

__device__ __forceinline__ DgMap cut_map(const PrefixCut c, const uint64_t* __restrict__ tab,
                                         const uint64_t* __restrict__ sums) {
  return DgMap{dg_pow_lad(tab, c.dm), c.slot != kPrefixNoSlot ? sums[c.slot] : 0u};
}

}  // namespace

// Pass 3, a wave per request: lane t of a round takes cut t's map x -> x R^dm + S, an inclusive
// scan by shuffles composes the maps of the cuts up to it, and applying that to the carry (the
// digest before the round) gives D at the cut; lane 63's goes into the next round.
__global__ __launch_bounds__(256) void k_digest_chain(const uint64_t* __restrict__ first, uint32_t n_req,
                                                      const PrefixCut* __restrict__ cuts,
                                                      const uint64_t* __restrict__ tab,
                                                      const uint64_t* __restrict__ sums,
                                                      clg_digest* __restrict__ out) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (w >= n_req) return;  // (wave-uniform)
  const uint64_t k0 = first[w], k1 = first[w + 1u];
  uint64_t carry = 0;
  for (uint64_t base = k0; base < k1; base += 64u) {  // (wave-uniform trip count)
    const uint64_t k = base + lane;
    const bool live = k < k1;
    PrefixCut c{0u, 0u, kPrefixNoSlot, 0u};
    if (live) c = cuts[k];
    DgMap f = live ? cut_map(c, tab, sums) : DgMap{1u, 0u};
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const DgMap g{(uint64_t)__shfl_up((unsigned long long)f.mul, o, 64),
                    (uint64_t)__shfl_up((unsigned long long)f.add, o, 64)};
      if (lane >= (uint32_t)o) f = dg_then(g, f);
    }
    const uint64_t d = dg_apply(f, carry);
    if (live) out[k] = clg_digest{d, c.len};
    carry = (uint64_t)__shfl((unsigned long long)d, 63, 64);  // (dead lanes hold the identity: d passes through)
  }
}

// Pass 3 for a call whose requests all have few cuts (tens of thousands of logs with an epoch
// or two each): a thread per request walks its cuts in turn.
__global__ __launch_bounds__(256) void k_digest_chain_short(const uint64_t* __restrict__ first, uint32_t n_req,
                                                            const PrefixCut* __restrict__ cuts,
                                                            const uint64_t* __restrict__ tab,
                                                            const uint64_t* __restrict__ sums,
                                                            clg_digest* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_req) return;
  uint64_t d = 0;
  for (uint64_t k = first[i], k1 = first[i + 1u]; k < k1; ++k) {
    const PrefixCut c = cuts[k];
    d = dg_apply(cut_map(c, tab, sums), d);
    out[k] = clg_digest{d, c.len};
  }
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
  hipLaunchKernelGGL(k_digest_pieces<false>, dim3((n_pieces + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_pieces,
                     n_pieces, d_runs, n_runs, (const uint32_t*)nullptr, d_tab, d_partial);
  hipLaunchKernelGGL(k_digest_runs<false>, dim3((n_runs + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_runs, n_runs,
                     n_pieces, d_partial, d_out, (uint64_t*)nullptr);
  return launch_status(hipGetLastError());
}

int launch_digest_prefixes(const GatherPiece* d_pieces, uint32_t n_pieces, const SegSpan* d_runs, uint32_t n_runs,
                           const uint32_t* d_lead, const uint64_t* d_first, uint32_t n_req, const PrefixCut* d_cuts,
                           bool few_cuts, const uint64_t* d_tab, uint64_t* d_partial, uint64_t* d_sums,
                           clg_digest* d_out, void* stream) {
  if (!n_req) return CLG_OK;
  if (n_pieces && n_runs) {
    hipLaunchKernelGGL(k_digest_pieces<true>, dim3((n_pieces + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_pieces,
                       n_pieces, d_runs, n_runs, d_lead, d_tab, d_partial);
    hipLaunchKernelGGL(k_digest_runs<true>, dim3((n_runs + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_runs, n_runs,
                       n_pieces, d_partial, (clg_digest*)nullptr, d_sums);
  }
  if (few_cuts)
    hipLaunchKernelGGL(k_digest_chain_short, dim3((n_req + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_first,
                       n_req, d_cuts, d_tab, d_sums, d_out);
  else
    hipLaunchKernelGGL(k_digest_chain, dim3((n_req + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_first, n_req,
                       d_cuts, d_tab, d_sums, d_out);
  return launch_status(hipGetLastError());
}

}  // namespace clg
