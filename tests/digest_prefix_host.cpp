// Host build of clonos_amd/csrc/digest.h for tests/test_digest_prefix_host.py (plain g++, no
// HIP), a program of its own: the one-pass prefix function dg_prefixes against dg_bytes of each
// prefix -- random spans with random cuts (duplicates and cuts past the end included), and cuts
// at every byte of a 300-byte span -- and the scan's map algebra against the plain recurrence.
// Prints "ok <rows checked>"; a mismatch is printed and ends it with status 1.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../clonos_amd/csrc/digest.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

uint64_t checked = 0;

bool check(const std::vector<uint8_t>& b, const std::vector<uint32_t>& cuts) {
  std::vector<uint64_t> hash(cuts.size() + 1), len(cuts.size() + 1);
  clg::dg_prefixes(b.data(), b.size(), cuts.data(), uint32_t(cuts.size()), hash.data(), len.data());
  for (size_t j = 0; j < cuts.size(); ++j) {
    const uint64_t c = std::min<uint64_t>(cuts[j], b.size());
    const uint64_t want = clg::dg_bytes(b.data(), c);
    if (hash[j] != want || len[j] != c) {
      printf("span of %zu bytes, cut %zu = %u: got {%llx, %llu}, want {%llx, %llu}\n", b.size(), j, cuts[j],
             (unsigned long long)hash[j], (unsigned long long)len[j], (unsigned long long)want, (unsigned long long)c);
      return false;
    }
    ++checked;
  }
  return true;
}

}  // namespace

int main() {
  for (int t = 0; t < 400; ++t) {
    std::vector<uint8_t> b(rnd() % 700);
    for (auto& x : b) x = uint8_t(rnd());
    std::vector<uint32_t> cuts(rnd() % 20);
    for (auto& c : cuts) c = uint32_t(rnd() % (b.size() + 9));
    if (t % 7 == 0 && !cuts.empty()) cuts.back() = 0xFFFFFFFFu;
    if (t % 5 == 0 && cuts.size() > 2) cuts[1] = cuts[0];
    std::sort(cuts.begin(), cuts.end());
    if (!check(b, cuts)) return 1;
  }
  {
    std::vector<uint8_t> b(300);
    for (auto& x : b) x = uint8_t(rnd());
    std::vector<uint32_t> cuts(b.size() + 1);
    for (size_t c = 0; c < cuts.size(); ++c) cuts[c] = uint32_t(c);
    if (!check(b, cuts)) return 1;
  }
  // composing the maps of consecutive cuts (what the chain kernel's scan does) gives the recurrence
  for (int t = 0; t < 200; ++t) {
    clg::DgMap f[5], all{1, 0};
    uint64_t x = rnd() % clg::kDigestP, step = x;
    for (auto& g : f) {
      g = clg::DgMap{clg::dg_pow(uint32_t(rnd() % 1000)), rnd() % clg::kDigestP};
      step = clg::dg_apply(g, step);
      all = clg::dg_then(all, g);
    }
    const clg::DgMap right = clg::dg_then(f[0], clg::dg_then(f[1], clg::dg_then(f[2], clg::dg_then(f[3], f[4]))));
    if (clg::dg_apply(all, x) != step || clg::dg_apply(right, x) != step) {
      printf("map composition %d\n", t);
      return 1;
    }
    ++checked;
  }
  printf("ok %llu\n", (unsigned long long)checked);
  return 0;
}
