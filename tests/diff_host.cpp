// Host build of clonos_amd/csrc/diff.h for tests/test_diff_host.py (plain g++, no HIP): a
// stand-alone program that checks the word compare, the edge masks and the host lcp
// (df_lcp_bytes, what clg_lcp_host returns) against a byte loop.  Exit status 0: all passed.
// It may be built with -fsanitize=address,undefined: every buffer is exactly as long as its
// string, so a read past an end is caught.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../clonos_amd/csrc/diff.h"

static int failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      if (failures++ < 20) {              \
        fprintf(stderr, "FAIL %s: ", #cond); \
        fprintf(stderr, __VA_ARGS__);     \
        fprintf(stderr, "\n");            \
      }                                   \
    }                                     \
  } while (0)

static uint64_t lcp_loop(const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb) {
  uint64_t i = 0;
  while (i < na && i < nb && a[i] == b[i]) ++i;
  return i;
}

static uint32_t le32(const uint8_t* p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

int main() {
  // word pairs differing in each of the four bytes, in one bit of it and in its high bit only
  const uint8_t base[4] = {0x12, 0x80, 0x00, 0xFE};
  EXPECT(clg::df_first_diff(le32(base), le32(base)) == 4, "equal words");
  EXPECT(clg::df_first_diff(0u, 0u) == 4 && clg::df_first_diff(~0u, ~0u) == 4, "equal words");
  for (uint32_t k = 0; k < 4; ++k) {
    for (uint32_t bit = 0; bit < 8; ++bit) {
      uint8_t o[4] = {base[0], base[1], base[2], base[3]};
      o[k] ^= uint8_t(1u << bit);
      EXPECT(clg::df_first_diff(le32(base), le32(o)) == k, "byte %u bit %u", k, bit);
      EXPECT(clg::df_first_diff(le32(o), le32(base)) == k, "byte %u bit %u (swapped)", k, bit);
      for (uint32_t k2 = k + 1; k2 < 4; ++k2) {  // a later byte differing too does not matter
        uint8_t o2[4] = {o[0], o[1], o[2], o[3]};
        o2[k2] ^= 0xFF;
        EXPECT(clg::df_first_diff(le32(base), le32(o2)) == k, "bytes %u and %u", k, k2);
      }
    }
  }
  EXPECT(clg::df_first_diff(0u, 0x80000000u) == 3, "the word's high bit only");
  EXPECT(clg::df_first_diff(0u, 0x00000080u) == 0, "the first byte's high bit only");

  // edge masks at every cut 0..4
  for (uint32_t lo = 0; lo <= 4; ++lo) {
    for (uint32_t hi = 0; hi <= 4; ++hi) {
      uint32_t want = 0;
      for (uint32_t k = lo; k < hi; ++k) want |= 0xFFu << (8 * k);
      EXPECT(clg::df_edge_mask(lo, hi) == want, "mask [%u, %u)", lo, hi);
    }
  }

  // the host lcp on pairs of every length 0..40 with the flip at every position
  uint32_t seed = 12345;
  for (uint32_t na = 0; na <= 40; ++na) {
    for (uint32_t nb = 0; nb <= 40; ++nb) {
      std::vector<uint8_t> a(na), b(nb);  // exactly as long as the strings
      for (uint32_t i = 0; i < na; ++i) a[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
      for (uint32_t i = 0; i < nb; ++i) b[i] = i < na ? a[i] : uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
      const uint32_t n = na < nb ? na : nb;
      EXPECT(clg::df_lcp_bytes(a.data(), na, b.data(), nb) == n, "equal prefix %u %u", na, nb);
      for (uint32_t d = 0; d < n; ++d) {
        for (uint8_t bit : {uint8_t(0x01), uint8_t(0x80)}) {
          b[d] ^= bit;
          const uint64_t got = clg::df_lcp_bytes(a.data(), na, b.data(), nb);
          EXPECT(got == d && got == lcp_loop(a.data(), na, b.data(), nb), "lengths %u %u flip at %u: %llu", na, nb, d,
                 (unsigned long long)got);
          if (d + 1 < nb) {  // a second flip behind the first
            b[nb - 1] ^= 0x40;
            EXPECT(clg::df_lcp_bytes(a.data(), na, b.data(), nb) == d, "lengths %u %u flips at %u and the end", na, nb, d);
            b[nb - 1] ^= 0x40;
          }
          b[d] ^= bit;
        }
      }
    }
  }
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("diff_host: ok\n");
  return 0;
}
