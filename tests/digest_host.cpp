// Host build of clonos_amd/csrc/digest.h for tests/test_digest_host.py (plain g++, no HIP):
// the power function the digest kernels' weights come from, behind a C ABI.
#include "../clonos_amd/csrc/digest.h"

extern "C" {
uint64_t dgh_pow(uint32_t e) { return clg::dg_pow(e); }
uint64_t dgh_pow_ladder(uint32_t e) {
  uint64_t lad[clg::kDigestLadder];
  clg::dg_ladder(lad);
  return clg::dg_pow_lad(lad, e);
}
uint64_t dgh_mul(uint64_t a, uint64_t b) { return clg::dg_mul(a, b); }
uint64_t dgh_step(uint64_t h, uint32_t w) { return clg::dg_step(h, w); }
uint64_t dgh_step_lazy(uint64_t h, uint32_t w) { return clg::dg_step_lazy(h, w); }
uint64_t dgh_reduce(uint64_t x) { return clg::dg_reduce(x); }
uint64_t dgh_bytes(const uint8_t* b, uint64_t n) { return clg::dg_bytes(b, n); }
}
