// Host build of clonos_amd/csrc/columns.h for tests/test_columns_host.py (plain g++, no HIP), a
// program of its own (so it also builds with -fsanitize=address,undefined and runs directly).
// For seeded tag and v0 arrays: the one-pass host function col_build_host against a naive
// per-class filter, the inverse (col_to_soa), the span bases, the sizes-only call,
// CLG_E_CAPACITY with the guard words either side of every column intact, and the lowest bad
// index for tags above 7.  Prints "ok <checks>"; a mismatch is printed and ends it with status 1.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../clonos_amd/csrc/columns.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

uint64_t checked = 0;
#define REQUIRE(c)                                       \
  do {                                                   \
    if (!(c)) {                                          \
      printf("line %d: %s (case %d)\n", __LINE__, #c, g_case); \
      return false;                                      \
    }                                                    \
    ++checked;                                           \
  } while (0)
int g_case = 0;

constexpr uint64_t kGuard = 4;  // guard elements either side of every column

// A column with guard elements either side, every guard byte 0xA5.
template <class T>
struct Guarded {
  std::vector<T> mem;
  uint64_t cap;
  explicit Guarded(uint64_t c) : mem(c + 2 * kGuard), cap(c) { memset(mem.data(), 0xA5, mem.size() * sizeof(T)); }
  T* data() { return mem.data() + kGuard; }
  bool guards_ok() const {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(mem.data());
    for (uint64_t i = 0; i < kGuard * sizeof(T); ++i)
      if (b[i] != 0xA5 || b[(kGuard + cap) * sizeof(T) + i] != 0xA5) return false;
    return true;
  }
  bool untouched() const {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(mem.data());
    for (uint64_t i = 0; i < mem.size() * sizeof(T); ++i)
      if (b[i] != 0xA5) return false;
    return true;
  }
};

struct Batch {
  std::vector<uint8_t> tag, w_sub;
  std::vector<int64_t> v0, w_v1;
  std::vector<uint32_t> w_idx, w_var_off, w_var_len;
  std::vector<int32_t> w_rc;
  std::vector<uint64_t> base;  // span_rec_base
  clg_decoded dec() {
    clg_decoded d{};
    d.tag = tag.data(), d.v0 = v0.data(), d.w_idx = w_idx.data(), d.w_rc = w_rc.data(), d.w_v1 = w_v1.data();
    d.w_var_off = w_var_off.data(), d.w_var_len = w_var_len.data(), d.w_sub = w_sub.data();
    d.n_rec = tag.size(), d.n_wide = w_idx.size();
    return d;
  }
  uint32_t n_spans() const { return uint32_t(base.size() - 1); }
};

// v0 as the decode leaves it: the field's own width, sign-extended.
int64_t value_for(uint8_t t) {
  const uint64_t r = rnd();
  switch (t) {
    case 0: return int8_t(r);
    case 2:
    case 7: return int32_t(r);
    default: return int64_t(r);
  }
}

Batch make(uint64_t n, uint32_t n_spans, int mode) {
  Batch b;
  for (uint64_t i = 0; i < n; ++i) {
    uint8_t t;
    switch (mode) {
      case 0: t = uint8_t(rnd() % 8); break;                       // every tag
      case 1: t = uint8_t(i & 1); break;                           // strict alternation
      case 2: t = uint8_t(i == 0 ? 0 : 1); break;                  // one Order, then Timestamps
      case 3: t = uint8_t(3 + rnd() % 4); break;                   // wide only
      default: t = uint8_t(mode - 4 < 3 ? mode - 4 : 7); break;    // all one narrow class (modes 4..7)
    }
    b.tag.push_back(t);
    b.v0.push_back(value_for(t));
    if (t >= 3 && t <= 6) {
      b.w_idx.push_back(uint32_t(i));
      b.w_rc.push_back(int32_t(rnd()));
      b.w_v1.push_back(int64_t(rnd()));
      b.w_var_off.push_back(uint32_t(rnd()));
      b.w_var_len.push_back(uint32_t(rnd() % 100));
      b.w_sub.push_back(uint8_t(rnd()));
    }
  }
  b.base.assign(n_spans + 1, 0);
  for (uint32_t s = 1; s < n_spans; ++s) b.base[s] = rnd() % (n + 1);  // (duplicates: empty spans)
  b.base[n_spans] = n;
  if (n_spans > 2 && rnd() % 2) b.base[1] = 0;          // an empty first span
  if (n_spans > 2 && rnd() % 2) b.base[n_spans - 1] = n;  // an empty last span
  std::sort(b.base.begin(), b.base.end());
  return b;
}

struct Cols {
  Guarded<uint8_t> tag, w_sub;
  Guarded<int8_t> order;
  Guarded<int64_t> timestamp, w_v1, w_v0;
  Guarded<int32_t> rng, buffer_built, w_rc;
  Guarded<uint32_t> w_idx, w_var_off, w_var_len;
  std::vector<uint64_t> span_base;
  Cols(uint64_t n, const uint64_t t[5], uint32_t n_spans)
      : tag(n), w_sub(t[4]), order(t[0]), timestamp(t[1]), w_v1(t[4]), w_v0(t[4]), rng(t[2]), buffer_built(t[3]),
        w_rc(t[4]), w_idx(t[4]), w_var_off(t[4]), w_var_len(t[4]), span_base((n_spans + 1) * 5, ~0ull) {}
  clg_columns c() {
    clg_columns o{};
    o.tag = tag.data(), o.order = order.data(), o.timestamp = timestamp.data(), o.rng = rng.data();
    o.buffer_built = buffer_built.data(), o.w_idx = w_idx.data(), o.w_rc = w_rc.data(), o.w_v1 = w_v1.data();
    o.w_var_off = w_var_off.data(), o.w_var_len = w_var_len.data(), o.w_sub = w_sub.data(), o.w_v0 = w_v0.data();
    o.span_base = span_base.data();
    o.cap_tag = tag.cap, o.cap_order = order.cap, o.cap_timestamp = timestamp.cap, o.cap_rng = rng.cap;
    o.cap_buffer_built = buffer_built.cap;
    o.cap_wide = std::min({w_idx.cap, w_rc.cap, w_v1.cap, w_var_off.cap, w_var_len.cap, w_sub.cap, w_v0.cap});
    return o;
  }
  bool guards_ok() const {
    return tag.guards_ok() && w_sub.guards_ok() && order.guards_ok() && timestamp.guards_ok() && w_v1.guards_ok() &&
           w_v0.guards_ok() && rng.guards_ok() && buffer_built.guards_ok() && w_rc.guards_ok() && w_idx.guards_ok() &&
           w_var_off.guards_ok() && w_var_len.guards_ok();
  }
  bool untouched() const {
    return tag.untouched() && w_sub.untouched() && order.untouched() && timestamp.untouched() && w_v1.untouched() &&
           w_v0.untouched() && rng.untouched() && buffer_built.untouched() && w_rc.untouched() && w_idx.untouched() &&
           w_var_off.untouched() && w_var_len.untouched();
  }
};

bool check(Batch& b) {
  const uint64_t n = b.tag.size();
  const uint32_t ns = b.n_spans();
  clg_decoded d = b.dec();

  // the naive reference: one filter per class, and the span bases by counting
  std::vector<int64_t> want[5];
  for (uint64_t i = 0; i < n; ++i) want[clg::col_class(b.tag[i])].push_back(b.v0[i]);
  uint64_t tot[5];
  for (int c = 0; c < 5; ++c) tot[c] = want[c].size();

  // sizes only
  std::vector<uint64_t> sb((ns + 1) * 5, ~0ull);
  clg_columns so{};
  so.span_base = sb.data();
  REQUIRE(clg::col_build_host(&d, b.base.data(), ns, &so) == CLG_OK);
  REQUIRE(so.n_rec == n);
  for (int c = 0; c < 5; ++c) REQUIRE(so.n_class[c] == tot[c]);
  for (uint32_t s = 0; s <= ns; ++s) {
    uint64_t cnt[5] = {0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < b.base[s]; ++i) ++cnt[clg::col_class(b.tag[i])];
    for (int c = 0; c < 5; ++c) REQUIRE(sb[s * 5 + c] == cnt[c]);
  }

  // exact capacities: every value, the guards, the inverse
  Cols cols(n, tot, ns);
  clg_columns o = cols.c();
  REQUIRE(clg::col_build_host(&d, b.base.data(), ns, &o) == CLG_OK);
  REQUIRE(cols.guards_ok());
  REQUIRE(cols.span_base == sb);
  for (uint64_t i = 0; i < n; ++i) REQUIRE(o.tag[i] == b.tag[i]);
  for (uint64_t k = 0; k < tot[0]; ++k) REQUIRE(o.order[k] == int8_t(want[0][k]) && int64_t(o.order[k]) == want[0][k]);
  for (uint64_t k = 0; k < tot[1]; ++k) REQUIRE(o.timestamp[k] == want[1][k]);
  for (uint64_t k = 0; k < tot[2]; ++k) REQUIRE(int64_t(o.rng[k]) == want[2][k]);
  for (uint64_t k = 0; k < tot[3]; ++k) REQUIRE(int64_t(o.buffer_built[k]) == want[3][k]);
  for (uint64_t k = 0; k < tot[4]; ++k) {
    REQUIRE(o.w_v0[k] == want[4][k] && o.w_idx[k] == b.w_idx[k] && o.w_rc[k] == b.w_rc[k] && o.w_v1[k] == b.w_v1[k]);
    REQUIRE(o.w_var_off[k] == b.w_var_off[k] && o.w_var_len[k] == b.w_var_len[k] && o.w_sub[k] == b.w_sub[k]);
  }
  std::vector<uint8_t> tag2(n);
  std::vector<int64_t> v2(n);
  REQUIRE(clg::col_to_soa(o, tag2.data(), v2.data()));
  REQUIRE(tag2 == b.tag && v2 == b.v0);

  // one element short in each column in turn: CLG_E_CAPACITY, the totals, nothing written
  for (int which = 0; which < 6; ++which) {
    const uint64_t full = which == 0 ? n : tot[which - 1];
    if (!full) continue;
    uint64_t t2[5] = {tot[0], tot[1], tot[2], tot[3], tot[4]};
    uint64_t n2 = n;
    if (which == 0) --n2; else --t2[which - 1];
    Cols sh(n2, t2, ns);
    clg_columns q = sh.c();
    REQUIRE(clg::col_build_host(&d, b.base.data(), ns, &q) == CLG_E_CAPACITY);
    REQUIRE(q.n_rec == n);
    for (int c = 0; c < 5; ++c) REQUIRE(q.n_class[c] == tot[c]);
    REQUIRE(sh.span_base == sb);
    REQUIRE(sh.untouched());
  }

  // a tag above 7 at two places: the lower index comes back, nothing is written
  if (n >= 2) {
    uint64_t i0 = rnd() % n, i1 = rnd() % n;
    if (i0 > i1) std::swap(i0, i1);
    const uint8_t k0 = b.tag[i0], k1 = b.tag[i1];
    b.tag[i0] = uint8_t(8 + rnd() % 248);
    b.tag[i1] = 9;
    const uint8_t bad = b.tag[i0];
    Cols e(n, tot, ns);
    clg_columns q = e.c();
    REQUIRE(clg::col_build_host(&d, b.base.data(), ns, &q) == CLG_E_INVALID_ARG);
    REQUIRE(q.err_status == CLG_E_INVALID_ARG && q.err_off == int64_t(i0) && q.err_tag == bad);
    uint32_t span = 0;  // the last span that starts at or before the record
    for (uint32_t s = 0; s < ns; ++s)
      if (b.base[s] <= i0) span = s;
    REQUIRE(q.err_span == span);
    REQUIRE(e.untouched());
    b.tag[i0] = k0;
    b.tag[i1] = k1;
  }
  return true;
}

}  // namespace

int main() {
  const uint64_t T = clg::kColTile;
  const uint64_t sizes[] = {0, 1, 2, 63, 64, 65, 300, T - 1, T, T + 1, 2 * T + 1};
  for (uint64_t n : sizes)
    for (int mode = 0; mode < 8; ++mode) {
      ++g_case;
      Batch b = make(n, uint32_t(n == 0 ? mode % 3 : 1 + rnd() % 9), mode);
      if (!check(b)) return 1;
    }
  {  // more than 64 one-record spans
    ++g_case;
    Batch b = make(200, 1, 0);
    b.base.clear();
    for (uint64_t i = 0; i <= 200; ++i) b.base.push_back(i);
    if (!check(b)) return 1;
  }
  {  // the class map and the narrowing
    for (uint32_t t = 0; t < 256; ++t) {
      const uint32_t want = t == 0 ? 0 : t == 1 ? 1 : t == 2 ? 2 : t == 7 ? 3 : t <= 6 ? 4 : 5;
      if (clg::col_class(t) != want) return printf("class of tag %u\n", t), 1;
      ++checked;
    }
    if (clg::col_i8(-128) != -128 || clg::col_i8(127) != 127 || clg::col_i32(INT32_MIN) != INT32_MIN ||
        clg::col_i32(-1) != -1)
      return printf("narrowing\n"), 1;
  }
  {  // side rows that do not match the wide tags; spans outside the batch
    ++g_case;
    Batch b = make(50, 2, 3);
    uint64_t tot[5] = {0, 0, 0, 0, 50};
    Cols c(50, tot, 2);
    clg_columns q = c.c();
    clg_decoded d = b.dec();
    d.n_wide = 49;
    if (clg::col_build_host(&d, b.base.data(), 2, &q) != CLG_E_INVALID_ARG) return printf("n_wide check\n"), 1;
    b.base[1] = 51;  // span_rec_base past n_rec
    if (clg::col_build_host(&d, b.base.data(), 2, &q) != CLG_E_INVALID_ARG) return printf("span check\n"), 1;
    checked += 2;
  }
  printf("ok %llu\n", (unsigned long long)checked);
  return 0;
}
