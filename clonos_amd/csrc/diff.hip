// diff.hip -- the longest common prefix (diff.h) of many log ranges and their reference spans,
// computed where the bytes live.
//
//  * k_diff_pieces   pass 1: a wave per piece (a source pointer, the logical offset of its first
//                    byte in the packed order, a length that never crosses a segment; what
//                    k_expand_pieces produces from SegSpan runs), clipped to the common range
//                    min(len_log, len_ref) of its run -> one u32 per piece: the offset in the
//                    piece of its first byte that differs from the reference, or kDiffNone
//  * k_diff_runs     pass 2: a wave per run takes the minimum over its pieces (contiguous) of
//                    piece offset in range + value and writes {lcp, len_log, len_ref}
//
// No atomics, no spin waits and no word taken from another running workgroup: the kernel
// boundary orders the two passes, and the result is deterministic.  Nothing tells the pieces
// after a mismatching one to stop: a divergent log is the rare case, and equal inputs read
// everything anyway.
//
// Pass 1 walks the piece in 16-byte windows at aligned addresses on the log side (one dwordx4
// each).  The reference bytes of a window sit at a byte shift m = (reference - log) mod 16 that
// is constant over the piece: the two aligned 16-byte words that hold them are loaded and
// realigned in registers with v_alignbyte, as the gather's copy_range realigns its source.  On
// both sides only aligned words that hold a byte of the clipped piece are loaded, so no load
// leaves the pages the ranges lie on.  Bytes outside the clipped piece are masked out of the
// xor.  A wave takes kDiffUnroll * 64 windows per iteration (all loads issued before the first
// compare) and stops after an iteration in which any lane found a mismatch: iterations ascend,
// so the minimum over the lanes is the piece's first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/clonos_engine.h"
#include "diff.h"
#include "kernels.h"

namespace clg {

namespace {

constexpr int kDiffUnroll = 4;  // windows per lane and iteration: a wave covers 4 KiB

__device__ __forceinline__ uint32_t df_find_run(const SegSpan* spans, uint32_t n, uint32_t g) {
  uint32_t lo = 0, hi = n;  // last run with first <= g
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (spans[mid].first <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// Loads by address, from global memory (an integer cast to a plain pointer would be a flat load).
typedef uint32_t df_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) df_u32x4* df_g_u32x4_p;
__device__ __forceinline__ uint4 df_load16(uintptr_t a) {
  const df_u32x4 v = *(df_g_u32x4_p)a;
  return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint32_t df_fsh(uint32_t hi, uint32_t lo, uint32_t s) {
  return __builtin_amdgcn_alignbyte(hi, lo, s);  // s in 0..3; 0 gives lo
}
// 16 bytes starting m bytes into the 32-byte window lo:hi (m in 0..15, wave-uniform).
__device__ __forceinline__ uint4 df_funnel16(const uint4 lo, const uint4 hi, uint32_t m) {
  const uint32_t s = m & 3;
  switch (m >> 2) {
    case 0: return make_uint4(df_fsh(lo.y, lo.x, s), df_fsh(lo.z, lo.y, s), df_fsh(lo.w, lo.z, s), df_fsh(hi.x, lo.w, s));
    case 1: return make_uint4(df_fsh(lo.z, lo.y, s), df_fsh(lo.w, lo.z, s), df_fsh(hi.x, lo.w, s), df_fsh(hi.y, hi.x, s));
    case 2: return make_uint4(df_fsh(lo.w, lo.z, s), df_fsh(hi.x, lo.w, s), df_fsh(hi.y, hi.x, s), df_fsh(hi.z, hi.y, s));
    default: return make_uint4(df_fsh(hi.x, lo.w, s), df_fsh(hi.y, hi.x, s), df_fsh(hi.z, hi.y, s), df_fsh(hi.w, hi.z, s));
  }
}

// The mask of the aligned dword at address x that keeps its bytes inside [b, e).
__device__ __forceinline__ uint32_t df_mask_at(uintptr_t x, uintptr_t b, uintptr_t e) {
  const uint32_t lo = x < b ? (b - x < 4 ? (uint32_t)(b - x) : 4u) : 0u;
  const uint32_t hi = x + 4 <= e ? 4u : (e > x ? (uint32_t)(e - x) : 0u);
  return df_edge_mask(lo, hi);
}

}  // namespace

__global__ __launch_bounds__(256) void k_diff_pieces(const GatherPiece* __restrict__ pieces, uint32_t n_pieces,
                                                     const SegSpan* __restrict__ runs, uint32_t n_runs,
                                                     const DiffRef* __restrict__ refs, uint32_t* __restrict__ first) {
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (g >= n_pieces) return;  // (wave-uniform)
  const GatherPiece pc = pieces[g];
  const uint32_t ri = df_find_run(runs, n_runs, g);
  const SegSpan r = runs[ri];
  const DiffRef rf = refs[ri];
  const uint32_t a = (uint32_t)(pc.dst - r.dst);  // the piece's first byte in its range
  const uint32_t common = r.len < rf.len ? r.len : rf.len;
  if (pc.len == 0 || a >= common) {  // nothing of the piece inside the common range
    if (lane == 0) first[g] = kDiffNone;
    return;
  }
  const uint32_t cl = pc.len < common - a ? pc.len : common - a;  // the clipped piece
  const uintptr_t l0 = (uintptr_t)pc.src, l1 = l0 + cl;
  const uintptr_t a0 = l0 & ~(uintptr_t)15;
  const uintptr_t r0 = (uintptr_t)rf.ref + a, r1 = r0 + cl;
  const uintptr_t delta = r0 - l0;  // reference address = log address + delta
  const uint32_t m = __builtin_amdgcn_readfirstlane((uint32_t)(delta & 15));
  const uint32_t nch = (uint32_t)((((l1 + 15) & ~(uintptr_t)15) - a0) >> 4);

  uint32_t best = kDiffNone;
  for (uint32_t j0 = 0; j0 < nch; j0 += kDiffUnroll * 64u) {
    uint4 lg[kDiffUnroll], lo[kDiffUnroll], hi[kDiffUnroll];
#pragma unroll
    for (int k = 0; k < kDiffUnroll; ++k) {
      const uint32_t j = j0 + lane + 64u * (uint32_t)k;
      lg[k] = lo[k] = hi[k] = make_uint4(0, 0, 0, 0);
      if (j < nch) {  // (every window from a0 on holds a byte of [l0, l1))
        const uintptr_t c = a0 + 16u * (uintptr_t)j;
        lg[k] = df_load16(c);
        const uintptr_t sa = (c + delta) & ~(uintptr_t)15;
        if (sa + 16 > r0 && sa < r1) lo[k] = df_load16(sa);
        if (m && sa + 32 > r0 && sa + 16 < r1) hi[k] = df_load16(sa + 16);
      }
    }
#pragma unroll
    for (int k = 0; k < kDiffUnroll; ++k) {
      const uint32_t j = j0 + lane + 64u * (uint32_t)k;
      if (j < nch) {
        const uintptr_t c = a0 + 16u * (uintptr_t)j;
        const uint4 v = df_funnel16(lo[k], hi[k], m);
        uint32_t x[4] = {lg[k].x ^ v.x, lg[k].y ^ v.y, lg[k].z ^ v.z, lg[k].w ^ v.w};
        if (c < l0 || c + 16 > l1) {  // a window at the clipped piece's edge
#pragma unroll
          for (uint32_t t = 0; t < 4; ++t) x[t] &= df_mask_at(c + 4u * t, l0, l1);
        }
        if (x[0] | x[1] | x[2] | x[3]) {
          // (a byte before l0 is masked, so the first differing byte is at or after l0)
          const uint32_t t = x[0] ? 0u : x[1] ? 1u : x[2] ? 2u : 3u;
          const uint32_t at = (uint32_t)(c + 4u * t - l0) + df_first_diff(x[t], 0u);
          best = at < best ? at : best;  // k ascends, so a lane's first hit is its lowest
        }
      }
    }
    if (__ballot(best != kDiffNone)) break;  // iterations ascend: the piece's first is among these
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)best, o, 64);
    best = w < best ? w : best;
  }
  if (lane == 0) first[g] = best;
}

__global__ __launch_bounds__(256) void k_diff_runs(const SegSpan* __restrict__ runs, uint32_t n_runs, uint32_t n_pieces,
                                                   const GatherPiece* __restrict__ pieces,
                                                   const DiffRef* __restrict__ refs, const uint32_t* __restrict__ first,
                                                   clg_diff* __restrict__ out) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (w >= n_runs) return;
  const SegSpan r = runs[w];
  const DiffRef rf = refs[w];
  const uint32_t p1 = w + 1u < n_runs ? runs[w + 1u].first : n_pieces;
  uint64_t best = r.len < rf.len ? r.len : rf.len;  // no mismatch: the common range
  for (uint32_t i = r.first + lane; i < p1; i += 64u) {
    const uint32_t v = first[i];
    if (v != kDiffNone) {
      const uint64_t at = pieces[i].dst - r.dst + v;
      best = at < best ? at : best;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)best, o, 64);
    best = x < best ? x : best;
  }
  if (lane == 0) out[r.pad] = clg_diff{best, r.len, rf.len};
}

int launch_diff(const GatherPiece* d_pieces, uint32_t n_pieces, const SegSpan* d_runs, uint32_t n_runs,
                const DiffRef* d_refs, uint32_t* d_first, clg_diff* d_out, void* stream) {
  if (!n_pieces || !n_runs) return CLG_OK;
  hipLaunchKernelGGL(k_diff_pieces, dim3((n_pieces + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_pieces, n_pieces,
                     d_runs, n_runs, d_refs, d_first);
  hipLaunchKernelGGL(k_diff_runs, dim3((n_runs + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_runs, n_runs, n_pieces,
                     d_pieces, d_refs, d_first, d_out);
  return launch_status(hipGetLastError());
}

}  // namespace clg
