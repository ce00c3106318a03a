// diff.h -- what the log comparison's host and device sides share, written once.
//
// The longest common prefix (lcp) of two byte strings is the number of leading bytes they have
// in common.  Both sides find it a little-endian 32-bit word at a time: the first differing
// byte of a word pair is ctz(a ^ b) / 8, and a word at the edge of a range is cut by a mask on
// both sides before it is compared.
//
// Plain C++: compiles under hipcc (host and device) and under g++ without HIP
// (tests/diff_host.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLG_DF_HD __host__ __device__ __forceinline__
#else
#define CLG_DF_HD inline
#endif

namespace clg {

constexpr uint32_t kDiffNone = ~0u;  // no mismatch (a piece's result; never an offset in a piece)

// Index (0..3) of the first byte in memory order in which the little-endian words a and b
// differ; 4 when they are equal.
CLG_DF_HD uint32_t df_first_diff(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  return x ? uint32_t(__builtin_ctz(x)) >> 3 : 4u;
}

// The mask that keeps bytes [lo, hi) of a little-endian word, 0 <= lo, hi <= 4 (lo >= hi: none).
CLG_DF_HD uint32_t df_edge_mask(uint32_t lo, uint32_t hi) {
  if (lo >= hi) return 0u;
  const uint32_t below_hi = hi >= 4u ? 0xFFFFFFFFu : (1u << (8u * hi)) - 1u;
  return below_hi & ~((1u << (8u * lo)) - 1u);  // lo < hi <= 4, so the shift is below 32
}

// lcp of a[0, na) and b[0, nb): whole words, then the last 0..3 bytes as one masked word.
inline uint64_t df_lcp_bytes(const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb) {
  const uint64_t n = na < nb ? na : nb;
  uint64_t i = 0;
  for (; i + 4 <= n; i += 4) {
    uint32_t x, y;
    memcpy(&x, a + i, 4);
    memcpy(&y, b + i, 4);
    if (x != y) {
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
      x = __builtin_bswap32(x);
      y = __builtin_bswap32(y);
#endif
      return i + df_first_diff(x, y);
    }
  }
  if (i < n) {
    uint32_t x = 0, y = 0;
    for (uint32_t k = 0; i + k < n; ++k) {
      x |= uint32_t(a[i + k]) << (8 * k);
      y |= uint32_t(b[i + k]) << (8 * k);
    }
    const uint32_t m = df_edge_mask(0, uint32_t(n - i));
    const uint32_t d = df_first_diff(x & m, y & m);
    if (d < 4) return i + d;
  }
  return n;
}

}  // namespace clg
