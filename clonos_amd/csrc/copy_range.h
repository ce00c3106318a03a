// copy_range.h -- the byte-range copy the gather, the scatter (kernels.hip) and the payload
// column (payload.hip) share: destination-aligned 16-byte chunks, the source realigned in
// registers with v_alignbyte (the shift is uniform per range).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clg {

__device__ __forceinline__ uint32_t fsh(uint32_t hi, uint32_t lo, uint32_t s) {
  return s ? __builtin_amdgcn_alignbyte(hi, lo, s) : lo;
}
// 16 bytes starting m bytes into the 32-byte window lo:hi (m in 1..15, uniform).
__device__ __forceinline__ uint4 funnel16(const uint4 lo, const uint4 hi, uint32_t m) {
  const uint32_t s = m & 3;
  switch (m >> 2) {
    case 0: return make_uint4(fsh(lo.y, lo.x, s), fsh(lo.z, lo.y, s), fsh(lo.w, lo.z, s), fsh(hi.x, lo.w, s));
    case 1: return make_uint4(fsh(lo.z, lo.y, s), fsh(lo.w, lo.z, s), fsh(hi.x, lo.w, s), fsh(hi.y, hi.x, s));
    case 2: return make_uint4(fsh(lo.w, lo.z, s), fsh(hi.x, lo.w, s), fsh(hi.y, hi.x, s), fsh(hi.z, hi.y, s));
    default: return make_uint4(fsh(hi.x, lo.w, s), fsh(hi.y, hi.x, s), fsh(hi.z, hi.y, s), fsh(hi.w, hi.z, s));
  }
}

// [src, src + len) -> [dst, dst + len) by NT threads (tid 0..NT-1).  Each thread takes up to
// kCopyK destination chunks (NT apart) and issues all their source loads before any store.
// Chunks that straddle the range's ends are written byte by byte from the same registers (no
// dependent loads).  A source load is issued only for an aligned 16-byte word that holds a
// byte of the range, so it never leaves the pages the range lies on (a caller's buffer ending
// at an unmapped page is safe).
constexpr int kCopyK = 4;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <uint32_t NT>
__device__ __forceinline__ void copy_range(const uint8_t* src, uint8_t* dst, uint32_t len, uint32_t tid) {
  if (len == 0) return;
  const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + len;
  const uintptr_t a0 = d0 & ~(uintptr_t)15;
  const uintptr_t sdelta = (uintptr_t)src - d0;  // src address = dst address + sdelta
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + len;
  const uint32_t m = (uint32_t)(sdelta & 15);
  const uint32_t nch = (uint32_t)((((d1 + 15) & ~(uintptr_t)15) - a0) >> 4);
  for (uint32_t j0 = 0; j0 < nch; j0 += kCopyK * NT) {
    uint4 lo[kCopyK], hi[kCopyK];
#pragma unroll
    for (int k = 0; k < kCopyK; ++k) {
      const uint32_t j = j0 + tid + NT * (uint32_t)k;
      lo[k] = hi[k] = make_uint4(0, 0, 0, 0);
      if (j < nch) {
        const uintptr_t sa = (a0 + 16u * (uintptr_t)j + sdelta) & ~(uintptr_t)15;
        if (sa + 16 > s0 && sa < s1) lo[k] = *reinterpret_cast<const uint4*>(sa);
        if (m && sa + 32 > s0 && sa + 16 < s1) hi[k] = *reinterpret_cast<const uint4*>(sa + 16);
      }
    }
#pragma unroll
    for (int k = 0; k < kCopyK; ++k) {
      const uint32_t j = j0 + tid + NT * (uint32_t)k;
      if (j < nch) {
        const uintptr_t c = a0 + 16u * (uintptr_t)j;
        const uint4 v = m ? funnel16(lo[k], hi[k], m) : lo[k];
        if (c >= d0 && c + 16 <= d1) {
          const u32x4 nv = {v.x, v.y, v.z, v.w};
          __builtin_nontemporal_store(nv, reinterpret_cast<u32x4*>(c));
        } else {  // range edge: the bytes inside [d0, d1)
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int x = 0; x < 16; ++x)
            if (c + x >= d0 && c + x < d1) *reinterpret_cast<uint8_t*>(c + x) = (uint8_t)(w[x >> 2] >> (8 * (x & 3)));
        }
      }
    }
  }
}

}  // namespace clg
