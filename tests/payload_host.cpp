// Host build of clonos_amd/csrc/payload.h for tests/test_payload_host.py (plain g++, no HIP), a
// program of its own (so it also builds with -fsanitize=address,undefined and runs directly).
// For seeded spans and rows: pay_build_host (clg_gather_payloads_host's body) against a
// byte-by-byte loop -- empty spans, zero-length rows, a row ending on its span's last byte -- the
// sizes-only call, both capacity failures with the outputs untouched, and the lowest bad row with
// nothing written.  The byte buffer is exactly as long as the spans, so a load past a span's end
// in the last span is a heap overflow the sanitizer reports.
// Prints "ok <checks>"; a mismatch is printed and ends it with status 1.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../clonos_amd/csrc/payload.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

uint64_t checked = 0;
int g_case = 0;
#define REQUIRE(c)                                             \
  do {                                                         \
    if (!(c)) {                                                \
      printf("line %d: %s (case %d)\n", __LINE__, #c, g_case); \
      return false;                                            \
    }                                                          \
    ++checked;                                                 \
  } while (0)

constexpr uint64_t kGuard = 32;  // guard bytes either side of var, guard entries either side of pos

struct Case {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> span_off, span_len, row_base;
  std::vector<uint32_t> off, len;
};

// n_spans spans (about a quarter empty), rows per span 0..max_rows; every non-empty span with rows
// gets one row ending on its last byte; about a quarter of the rows have length 0.
Case make_case(uint32_t n_spans, uint32_t max_rows, uint32_t max_span) {
  Case c;
  c.row_base.push_back(0);
  uint64_t at = 0;
  for (uint32_t s = 0; s < n_spans; ++s) {
    const uint64_t L = rnd() % 4 == 0 ? 0 : 1 + rnd() % max_span;
    at += rnd() % 7;  // a gap between spans
    c.span_off.push_back(at);
    c.span_len.push_back(L);
    at += L;
    const uint32_t rows = uint32_t(rnd() % (max_rows + 1));
    for (uint32_t r = 0; r < rows; ++r) {
      uint32_t o, l;
      if (L == 0) {
        o = 0, l = 0;
      } else if (r == 0) {  // ends on the span's last byte
        l = uint32_t(1 + rnd() % L);
        o = uint32_t(L - l);
      } else if (rnd() % 4 == 0) {
        o = uint32_t(rnd() % (L + 1)), l = 0;  // (a zero-length row may sit at the span's end)
      } else {
        o = uint32_t(rnd() % L);
        l = uint32_t(rnd() % (L - o + 1));
      }
      c.off.push_back(o);
      c.len.push_back(l);
    }
    c.row_base.push_back(c.off.size());
  }
  c.bytes.resize(at);
  for (auto& b : c.bytes) b = uint8_t(rnd());
  return c;
}

struct Out {
  std::vector<uint8_t> var;
  std::vector<uint64_t> pos;
  clg_payloads p{};
  Out(uint64_t cap_var, uint64_t cap_pos) : var(cap_var + 2 * kGuard, 0xA5), pos(cap_pos + 2 * kGuard, 0xA5A5A5A5A5A5A5A5ull) {
    p.var = var.data() + kGuard;
    p.pos = pos.data() + kGuard;
    p.cap_var = cap_var;
    p.cap_pos = cap_pos;
    p.out_kind = CLG_MEM_HOST;
  }
  bool guards_ok() const {
    for (uint64_t i = 0; i < kGuard; ++i)
      if (var[i] != 0xA5 || var[kGuard + p.cap_var + i] != 0xA5 || pos[i] != 0xA5A5A5A5A5A5A5A5ull ||
          pos[kGuard + p.cap_pos + i] != 0xA5A5A5A5A5A5A5A5ull)
        return false;
    return true;
  }
  bool untouched() const {
    for (uint8_t b : var)
      if (b != 0xA5) return false;
    for (uint64_t w : pos)
      if (w != 0xA5A5A5A5A5A5A5A5ull) return false;
    return true;
  }
};

int build(const Case& c, clg_payloads* p) {
  return clg::pay_build_host(c.bytes.data(), c.span_off.data(), c.span_len.data(), uint32_t(c.span_len.size()),
                             c.off.data(), c.len.data(), c.row_base.data(), p);
}

bool check_case(const Case& c) {
  const uint32_t ns = uint32_t(c.span_len.size());
  const uint64_t n = c.off.size();
  // the byte-by-byte loop
  std::vector<uint8_t> want;
  std::vector<uint64_t> want_pos;
  for (uint32_t s = 0; s < ns; ++s)
    for (uint64_t k = c.row_base[s]; k < c.row_base[s + 1]; ++k) {
      want_pos.push_back(want.size());
      for (uint32_t i = 0; i < c.len[k]; ++i) want.push_back(c.bytes[c.span_off[s] + c.off[k] + i]);
    }
  want_pos.push_back(want.size());

  // sizes only
  clg_payloads sz{};
  REQUIRE(build(c, &sz) == CLG_OK);
  REQUIRE(sz.n_rows == n && sz.n_var == want.size() && sz.bad_row == clg::kPayNoRow);

  // exact capacities
  Out o(want.size(), n + 1);
  REQUIRE(build(c, &o.p) == CLG_OK);
  REQUIRE(o.guards_ok());
  REQUIRE(o.p.n_rows == n && o.p.n_var == want.size() && o.p.bad_row == clg::kPayNoRow);
  for (uint64_t k = 0; k <= n; ++k) REQUIRE(o.p.pos[k] == want_pos[k]);
  for (uint64_t i = 0; i < want.size(); ++i) REQUIRE(o.p.var[i] == want[i]);

  // one short in each array
  if (!want.empty()) {
    Out s(want.size() - 1, n + 1);
    REQUIRE(build(c, &s.p) == CLG_E_CAPACITY);
    REQUIRE(s.untouched() && s.p.n_rows == n && s.p.n_var == want.size());
  }
  {
    Out s(want.size(), n);
    REQUIRE(build(c, &s.p) == CLG_E_CAPACITY);
    REQUIRE(s.untouched() && s.p.n_rows == n && s.p.n_var == want.size());
  }

  // bad rows: one byte past the span's end, at two places; the lowest is reported
  if (n >= 2) {
    Case b = c;
    uint64_t k1 = rnd() % n, k2 = rnd() % n;
    if (k2 < k1) std::swap(k1, k2);
    uint64_t counted = want.size();
    for (int j = 0; j < (k1 == k2 ? 1 : 2); ++j) {
      const uint64_t k = j ? k2 : k1;
      uint32_t s = 0;
      while (b.row_base[s + 1] <= k) ++s;
      counted -= b.len[k];  // (a bad row counts as length 0)
      if (rnd() & 1) {
        b.off[k] = uint32_t(b.span_len[s]);  // one byte past the span's last
        b.len[k] = 1;
      } else {
        b.off[k] = 0xFFFFFFFFu;  // off + len wraps in 32 bits
        b.len[k] = 2;
      }
    }
    Out s(want.size() + 8, n + 1);
    REQUIRE(build(b, &s.p) == CLG_E_INVALID_ARG);
    REQUIRE(s.p.bad_row == k1 && s.p.n_rows == n && s.p.n_var == counted);
    REQUIRE(s.untouched());
  }
  return true;
}

bool fixed_cases() {
  // no spans, no rows: only pos[0]
  {
    Out o(0, 1);
    REQUIRE(clg::pay_build_host(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &o.p) == CLG_OK);
    REQUIRE(o.p.n_rows == 0 && o.p.n_var == 0 && o.p.pos[0] == 0 && o.guards_ok());
  }
  // only empty spans, rows of length 0
  {
    Case c;
    c.span_off = {0, 0, 0}, c.span_len = {0, 0, 0}, c.row_base = {0, 2, 2, 3};
    c.off = {0, 0, 0}, c.len = {0, 0, 0};
    if (!check_case(c)) return false;
    c.off[2] = 1;  // offset 1 of an empty span, length 0: past the end
    clg_payloads p{};
    REQUIRE(build(c, &p) == CLG_E_INVALID_ARG && p.bad_row == 2);
  }
  // row_base that decreases, or does not start at 0
  {
    Case c = make_case(3, 4, 50);
    Case d = c;
    d.row_base[0] = 1;
    clg_payloads p{};
    if (d.row_base[1] >= 1) REQUIRE(build(d, &p) == CLG_E_INVALID_ARG);
    d = c;
    d.row_base[2] = d.row_base[3] + 1;
    REQUIRE(build(d, &p) == CLG_E_INVALID_ARG);
  }
  return true;
}

}  // namespace

int main() {
  if (!fixed_cases()) return 1;
  for (g_case = 1; g_case <= 400; ++g_case) {
    const uint32_t ns = 1 + uint32_t(rnd() % 12), rows = uint32_t(rnd() % 40), span = 1 + uint32_t(rnd() % 600);
    if (!check_case(make_case(ns, rows, span))) return 1;
  }
  printf("ok %llu\n", (unsigned long long)checked);
  return 0;
}
