// pack_small_host.cpp -- what the one-launch pack (pack_small.hip) takes from pack.h and pack_wide.h
// on the host side, under plain g++: the staging bounds are never below what the CPU packers
// produce, and the in-header stream layout is the one the CPU packer lays out.  Stand-alone:
// prints "ok <checks>" and returns 0, or says what failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../clonos_amd/csrc/pack.h"
#include "../clonos_amd/csrc/pack_wide.h"

using namespace clg;

static long g_checks = 0;
#define REQUIRE(c, ...)                                    \
  do {                                                     \
    ++g_checks;                                            \
    if (!(c)) {                                            \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      exit(1);                                             \
    }                                                      \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

enum Pattern { kRandom, kEqual, kExtremes, kAlternate, kPatterns };
// Value i of a pattern, as 64 bits that every element truncates: random, all equal, INT64_MIN
// beside INT64_MAX (a narrow element: its own extremes), 0 beside all ones.
static uint64_t value(int pattern, uint64_t i) {
  switch (pattern) {
    case kRandom: return rnd();
    case kEqual: return 0x5A5A5A5A5A5A5A5Aull;
    case kExtremes: return i & 1 ? uint64_t(INT64_MAX) : uint64_t(INT64_MIN);
    default: return i & 1 ? ~0ull : 0ull;
  }
}
static const uint64_t kLens[] = {0, 1, 2, 1023, 1024, 1025, 2049};

static void narrow_case(const uint64_t n[kPackStreams], int pattern) {
  std::vector<uint8_t> tag(n[0] + 1);
  std::vector<int8_t> order(n[1] + 1);
  std::vector<int64_t> ts(n[2] + 1);
  std::vector<int32_t> rng(n[3] + 1), bb(n[4] + 1);
  for (uint64_t i = 0; i < n[0]; ++i) tag[i] = uint8_t(value(pattern, i));
  for (uint64_t i = 0; i < n[1]; ++i) order[i] = pattern == kExtremes ? (i & 1 ? 127 : -128) : int8_t(value(pattern, i));
  for (uint64_t i = 0; i < n[2]; ++i) ts[i] = int64_t(value(pattern, i));
  for (uint64_t i = 0; i < n[3]; ++i) rng[i] = pattern == kExtremes ? (i & 1 ? INT32_MAX : INT32_MIN) : int32_t(value(pattern, i));
  for (uint64_t i = 0; i < n[4]; ++i) bb[i] = int32_t(value(pattern, i + 1));
  clg_columns c{};
  c.tag = tag.data(), c.order = order.data(), c.timestamp = ts.data(), c.rng = rng.data(), c.buffer_built = bb.data();
  c.n_rec = n[0];
  for (int k = 0; k < 4; ++k) c.n_class[k] = n[k + 1];
  clg_packed p{};
  REQUIRE(pack_build_host(&c, &p) == CLG_OK, "sizes");
  const uint64_t bound = pack_bits_bound_narrow(n);
  REQUIRE(p.n_bits <= bound, "narrow pattern %d: %llu bytes, bound %llu", pattern, (unsigned long long)p.n_bits,
          (unsigned long long)bound);
  // ... and per stream, from the blocks the packer wrote
  std::vector<clg_pack_block> desc(p.blk_base[kPackStreams] + 1);
  std::vector<uint8_t> bits(p.n_bits + 16);
  p.desc = desc.data(), p.bits = bits.data(), p.cap_desc = desc.size(), p.cap_bits = bits.size();
  REQUIRE(pack_build_host(&c, &p) == CLG_OK, "write");
  for (uint32_t s = 0; s < kPackStreams; ++s) {
    uint64_t used = 0;
    for (uint64_t b = p.blk_base[s]; b < p.blk_base[s + 1]; ++b) {
      REQUIRE(desc[b].width <= pack_width_bound(pack_stream_elem(s), pack_is_delta(s)), "stream %u width %u", s, desc[b].width);
      used += pack_payload_bytes(pack_resid(s, desc[b].count), desc[b].width);
    }
    REQUIRE(used <= pack_bits_bound(pack_stream_elem(s), pack_is_delta(s), n[s]), "stream %u", s);
  }
}

// n rows whose kinds come from `mix` (0: all kinds in turn, 1..4: kind mix - 1 alone, 5: random).
static void wide_case(uint64_t n, int pattern, int mix) {
  const uint64_t nr = n + 3;
  std::vector<uint8_t> tag(nr), sub(n + 1);
  std::vector<uint32_t> idx(n + 1), off(n + 1), len(n + 1);
  std::vector<int32_t> rc(n + 1);
  std::vector<int64_t> v1(n + 1), v0(n + 1);
  uint64_t tot[kWPackKinds] = {};
  for (uint64_t k = 0; k < n; ++k) {
    const uint32_t kind = mix == 0 ? uint32_t(k % 4) : mix <= 4 ? uint32_t(mix - 1) : uint32_t(rnd() % 4);
    ++tot[kind];
    idx[k] = uint32_t(k + 1), tag[k + 1] = uint8_t(kWPackFirstTag + kind);
    off[k] = pattern == kExtremes || pattern == kAlternate ? (k & 1 ? 0xFFFFFFFFu : 0u) : uint32_t(value(pattern, k));
    len[k] = uint32_t(value(pattern, k + 1)), sub[k] = uint8_t(value(pattern, k));
    rc[k] = pattern == kExtremes ? (k & 1 ? INT32_MAX : INT32_MIN) : int32_t(value(pattern, k));
    v1[k] = int64_t(value(pattern, k)), v0[k] = int64_t(value(pattern, k + 1));
  }
  clg_columns c{};
  c.tag = tag.data(), c.n_rec = nr, c.n_class[4] = n;
  c.w_idx = idx.data(), c.w_rc = rc.data(), c.w_v1 = v1.data(), c.w_var_off = off.data(), c.w_var_len = len.data();
  c.w_sub = sub.data(), c.w_v0 = v0.data();
  clg_packed_wide p{};
  REQUIRE(wpack_build_host(&c, &p) == CLG_OK, "sizes");
  REQUIRE(p.n_bits <= wpack_bits_bound(n), "wide n %llu pattern %d mix %d: %llu bytes, bound %llu", (unsigned long long)n, pattern,
          mix, (unsigned long long)p.n_bits, (unsigned long long)wpack_bits_bound(n));
  REQUIRE(p.blk_base[kWPackStreams] <= wpack_blocks_bound(n), "wide n %llu: %llu blocks, bound %llu", (unsigned long long)n,
          (unsigned long long)p.blk_base[kWPackStreams], (unsigned long long)wpack_blocks_bound(n));
  // the in-header layout against the packer's, and against the rule spelled out
  uint64_t n_val[kWPackStreams], blk_base[kWPackStreams + 1];
  wpack_layout_streams(n, tot, n_val, blk_base);
  uint64_t at = 0;
  for (uint32_t s = 0; s < kWPackStreams; ++s) {
    const uint64_t want = s < 2 ? n : tot[(s - 2) / kWPackFields];
    REQUIRE(n_val[s] == p.n_val[s] && n_val[s] == want, "n_val[%u]", s);
    REQUIRE(blk_base[s] == p.blk_base[s] && blk_base[s] == at, "blk_base[%u]", s);
    at += (want + kPackBlock - 1) / kPackBlock;
  }
  REQUIRE(blk_base[kWPackStreams] == p.blk_base[kWPackStreams] && blk_base[kWPackStreams] == at, "blk_base's end");
  // the per-kind arrays' layout: the fields one behind the other, aligned, none overlapping
  for (uint32_t f = 0; f < kWPackFields; ++f) {
    REQUIRE(wpack_soa_field(f, n) % 16 == 0, "field %u", f);
    REQUIRE(wpack_soa_field(f + 1, n) - wpack_soa_field(f, n) >= n * pack_elem_bytes(kWPackField[f].elem), "field %u", f);
  }
  if (pattern == kAlternate && mix == 1 && n >= 3) {  // 0, 0xFFFFFFFF, 0, ...: a residual wider than its element
    std::vector<clg_pack_block> desc(p.blk_base[kWPackStreams]);
    std::vector<uint8_t> bits(p.n_bits + 16);
    p.desc = desc.data(), p.bits = bits.data(), p.cap_desc = desc.size(), p.cap_bits = bits.size();
    REQUIRE(wpack_build_host(&c, &p) == CLG_OK, "write");
    REQUIRE(desc[p.blk_base[wpack_stream(0, CLG_WPACK_VAR_OFF)]].width == 33, "VAR_OFF width %u",
            desc[p.blk_base[wpack_stream(0, CLG_WPACK_VAR_OFF)]].width);
  }
}

int main() {
  REQUIRE(pack_width_bound(kElemU32, true) == 33 && pack_width_bound(kElemI32, true) == 33, "33 bits");
  REQUIRE(pack_width_bound(kElemI64, true) == 64 && pack_width_bound(kElemU8, false) == 8, "element widths");
  REQUIRE(kWPackSmallBlocks == wpack_blocks_bound(kWPackSmallRows), "kWPackSmallBlocks");
  for (int pattern = 0; pattern < kPatterns; ++pattern) {
    for (uint64_t a : kLens)
      for (uint64_t b : kLens) {
        const uint64_t n[kPackStreams] = {a, b, a, b, a};
        narrow_case(n, pattern);
        const uint64_t m[kPackStreams] = {b, 0, b, a, 0};
        narrow_case(m, pattern);
      }
    for (uint64_t n : kLens)
      for (int mix = 0; mix <= 5; ++mix) wide_case(n, pattern, mix);
    wide_case(4 * 1024, pattern, 0);   // every kind exactly one block
    wide_case(4 * 1024 + 4, pattern, 0);  // every kind one value into its second block
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
