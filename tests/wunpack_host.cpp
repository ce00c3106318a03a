// Stand-alone check of what the calls that take both packed forms do on the CPU
// (clonos_amd/csrc/pack_wide.h: wpack_unpack_both_host and its parts, the cross rule, the offset of
// a wide finding's stream, the prefix sum) with encode_columns.h's host encode behind it: the
// unpacked arrays and pos against the rows they were packed from, the encode of the two packed
// forms against the encode of the plain columns, every check in its order (narrow layout, totals,
// wide layout, n_class[4], a narrow finding before a wide one, the wide findings with their
// offset, the cross rule in the first and in the last tile with the lowest row winning), and the
// encode's output untouched on every rejection.  Row counts 0, 1, 1023, 1024, 1025 and 2049.
// Built with g++ (no HIP), plainly and with -fsanitize=address,undefined; every array is allocated
// at its exact size so that a read or write past a stated length is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../clonos_amd/csrc/encode_columns.h"
#include "../clonos_amd/csrc/pack_wide.h"

namespace {

uint64_t g_checks = 0;
#define REQUIRE(x)                                                     \
  do {                                                                 \
    ++g_checks;                                                        \
    if (!(x)) {                                                        \
      fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

constexpr uint8_t kFill = 0xA5;

// Plain columns with their payload column: n_wide wide records, each behind `gap` narrow ones.
struct Plain {
  std::vector<uint8_t> tag, w_sub, var;
  std::vector<int8_t> order;
  std::vector<int64_t> timestamp, w_v1, w_v0;
  std::vector<int32_t> rng, buffer_built, w_rc;
  std::vector<uint32_t> w_idx, w_var_off, w_var_len;
  std::vector<uint64_t> pos;

  Plain(uint32_t n_wide, uint32_t gap, uint32_t seed) {
    std::mt19937_64 g(seed);
    int64_t clock = 1700000000000ll;
    uint32_t off = 0;
    for (uint32_t k = 0; k < n_wide; ++k) {
      for (uint32_t i = 0; i < gap; ++i) {
        static const uint8_t narrow[4] = {0, 1, 2, 7};
        const uint8_t t = narrow[g() % 4];
        tag.push_back(t);
        clock += int64_t(g() % 40);
        if (t == 0) order.push_back(int8_t(g() % 5));
        else if (t == 1) timestamp.push_back(clock);
        else if (t == 2) rng.push_back(int32_t(g()));
        else buffer_built.push_back(int32_t(g() % 4096));
      }
      const uint32_t kind = uint32_t(g() % 4);
      w_idx.push_back(uint32_t(tag.size()));
      tag.push_back(uint8_t(3 + kind));
      const uint32_t len = kind == 3 ? 0 : uint32_t(g() % 23);
      w_rc.push_back(int32_t(g() % 100000)), w_v1.push_back(kind ? clock : 0);
      w_var_off.push_back(off), w_var_len.push_back(len);
      w_sub.push_back(kind == 1 ? (g() % 2 ? 6 : 0) : kind == 2 ? (g() % 2 ? 0x80 : 0) : 0);
      w_v0.push_back(kind == 0 ? int64_t(len) : clock - 3);
      off += len + 9;
    }
    pos.resize(size_t(n_wide) + 1);
    clg::wpack_pos_host(w_var_len.data(), n_wide, pos.data());
    var.resize(size_t(pos[n_wide]));
    for (size_t i = 0; i < var.size(); ++i) var[i] = uint8_t(i * 7 + 1);
  }
  clg_columns cols() const {
    clg_columns c{};
    c.tag = const_cast<uint8_t*>(tag.data()), c.order = const_cast<int8_t*>(order.data());
    c.timestamp = const_cast<int64_t*>(timestamp.data()), c.rng = const_cast<int32_t*>(rng.data());
    c.buffer_built = const_cast<int32_t*>(buffer_built.data());
    c.w_idx = const_cast<uint32_t*>(w_idx.data()), c.w_rc = const_cast<int32_t*>(w_rc.data());
    c.w_v1 = const_cast<int64_t*>(w_v1.data()), c.w_var_off = const_cast<uint32_t*>(w_var_off.data());
    c.w_var_len = const_cast<uint32_t*>(w_var_len.data()), c.w_sub = const_cast<uint8_t*>(w_sub.data());
    c.w_v0 = const_cast<int64_t*>(w_v0.data());
    c.n_rec = tag.size();
    c.n_class[0] = order.size(), c.n_class[1] = timestamp.size(), c.n_class[2] = rng.size();
    c.n_class[3] = buffer_built.size(), c.n_class[4] = w_idx.size();
    return c;
  }
  // what the combined calls take beside the packed forms
  clg_columns_in rest() const {
    clg_columns_in r{};
    r.var = var.data(), r.n_var = var.size(), r.n_rec = tag.size();
    r.n_class[0] = order.size(), r.n_class[1] = timestamp.size(), r.n_class[2] = rng.size();
    r.n_class[3] = buffer_built.size(), r.n_class[4] = w_idx.size();
    r.in_kind = CLG_MEM_HOST;
    return r;
  }
  clg_columns_in full() const {
    clg_columns_in r = rest();
    r.tag = tag.data(), r.order = order.data(), r.timestamp = timestamp.data(), r.rng = rng.data();
    r.buffer_built = buffer_built.data(), r.w_rc = w_rc.data(), r.w_v1 = w_v1.data(), r.w_var_len = w_var_len.data();
    r.w_sub = w_sub.data(), r.w_v0 = w_v0.data(), r.w_idx = w_idx.data(), r.pos = pos.data();
    return r;
  }
};

// Both packed forms of plain columns, in exactly sized arrays.
struct Both {
  std::vector<clg_pack_block> ndesc, wdesc;
  std::vector<uint8_t> nbits, wbits;
  clg_packed narrow{};
  clg_packed_wide wide{};
  explicit Both(const clg_columns& c, bool with_wide = true) {
    REQUIRE(clg::pack_build_host(&c, &narrow) == CLG_OK);
    ndesc.resize(size_t(narrow.blk_base[clg::kPackStreams])), nbits.resize(size_t(narrow.n_bits));
    narrow.desc = ndesc.data(), narrow.bits = nbits.data(), narrow.cap_desc = ndesc.size(), narrow.cap_bits = nbits.size();
    REQUIRE(clg::pack_build_host(&c, &narrow) == CLG_OK);
    if (!with_wide) return;
    REQUIRE(clg::wpack_build_host(&c, &wide) == CLG_OK);
    wdesc.resize(size_t(wide.blk_base[clg::kWPackStreams])), wbits.resize(size_t(wide.n_bits));
    wide.desc = wdesc.data(), wide.bits = wbits.data(), wide.cap_desc = wdesc.size(), wide.cap_bits = wbits.size();
    REQUIRE(clg::wpack_build_host(&c, &wide) == CLG_OK);
  }
};

struct Enc {
  int st;
  std::vector<uint8_t> bytes;
  clg_encoded e{};
};
// The host encode of complete columns: sizes, then exactly sized bytes.
Enc encode_plain(const clg_columns_in& in) {
  Enc r;
  r.st = clg::ecol_build_host(&in, &r.e);
  if (r.st != CLG_OK) return r;
  r.bytes.resize(size_t(r.e.n_bytes));
  r.e.bytes = r.bytes.data(), r.e.cap = r.bytes.size();
  r.st = clg::ecol_build_host(&in, &r.e);
  return r;
}
// The combined call on the CPU, as clg_encode_columns_packed_wide_host composes it, into `cap`
// bytes of kFill.
struct EncBoth {
  int st;
  clg_unpack_bad bad;
  std::vector<uint8_t> bytes;
  clg_encoded e{};
};
EncBoth encode_both(const clg_packed& narrow, const clg_packed_wide& wide, const clg_columns_in& rest, size_t cap) {
  EncBoth r;
  r.bytes.assign(cap, kFill);
  r.e.bytes = r.bytes.data(), r.e.cap = cap;
  clg::ecol_reset_result(&r.e);
  clg::WPackBothHost h;
  clg_columns_in full;
  const char* what = "";
  r.st = clg::wpack_unpack_both_host(&narrow, &wide, &rest, &r.bad, &h, &full, &what);
  if (r.st == CLG_OK) r.st = clg::ecol_build_host(&full, &r.e, &what);
  return r;
}
bool untouched(const EncBoth& r) {
  for (uint8_t b : r.bytes)
    if (b != kFill) return false;
  return r.e.bad_what == CLG_ENC_BAD_NONE && r.e.n_bytes == 0;
}

void round_trips(uint32_t n_wide, uint32_t gap, uint32_t seed) {
  const Plain p(n_wide, gap, seed);
  const clg_columns c = p.cols();
  const Both b(c);
  const clg_columns_in rest = p.rest();
  // the arrays and pos
  clg::WPackBothHost h;
  clg_columns_in full;
  clg_unpack_bad bad;
  const char* what = "";
  REQUIRE(clg::wpack_unpack_both_host(&b.narrow, &b.wide, &rest, &bad, &h, &full, &what) == CLG_OK);
  REQUIRE(bad.what == CLG_UNPACK_BAD_NONE);
  for (uint64_t i = 0; i < c.n_rec; ++i) REQUIRE(full.tag[i] == p.tag[i]);
  for (uint32_t k = 0; k < n_wide; ++k) {
    REQUIRE(full.w_idx[k] == p.w_idx[k] && full.w_rc[k] == p.w_rc[k] && full.w_v1[k] == p.w_v1[k]);
    REQUIRE(full.w_var_len[k] == p.w_var_len[k] && full.w_sub[k] == p.w_sub[k] && full.w_v0[k] == p.w_v0[k]);
    REQUIRE(h.w_var_off[k] == p.w_var_off[k] && full.pos[k] == p.pos[k]);
  }
  REQUIRE(full.pos[n_wide] == p.pos[n_wide] && full.var == p.var.data() && full.n_var == p.var.size());
  // the bytes
  const Enc want = encode_plain(p.full());
  REQUIRE(want.st == CLG_OK);
  const EncBoth got = encode_both(b.narrow, b.wide, rest, want.bytes.size());
  REQUIRE(got.st == CLG_OK && got.e.n_bytes == want.e.n_bytes && got.bytes == want.bytes);
}

#define REJECTED(r, w, s, b) \
  REQUIRE((r).st == CLG_E_INVALID_ARG && (r).bad.what == (w) && (r).bad.stream == (s) && (r).bad.block == (b) && untouched(r))

void check_order() {
  const uint32_t n = 2500;
  const Plain p(n, 2, 77);
  const clg_columns c = p.cols();
  const clg_columns_in rest = p.rest();
  const size_t cap = 1 << 20;
  const uint32_t W = CLG_UNPACK_WIDE_STREAM;
  {  // rest must not carry what the packed forms give
    const Both b(c);
    clg_columns_in r = rest;
    r.w_rc = p.w_rc.data();
    EncBoth e = encode_both(b.narrow, b.wide, r, cap);
    REQUIRE(e.st == CLG_E_INVALID_ARG && e.bad.what == CLG_UNPACK_BAD_NONE && untouched(e));
    r = rest, r.pos = p.pos.data();
    e = encode_both(b.narrow, b.wide, r, cap);
    REQUIRE(e.st == CLG_E_INVALID_ARG && e.bad.what == CLG_UNPACK_BAD_NONE && untouched(e));
  }
  {  // both layouts broken: the narrow one is reported; then the totals; then the wide layout; then n_class[4]
    Both b(c);
    b.narrow.blk_base[3] += 1, b.wide.blk_base[7] += 1;
    REJECTED(encode_both(b.narrow, b.wide, rest, cap), CLG_UNPACK_BAD_LAYOUT, 2u, 0u);
    b.narrow.blk_base[3] -= 1;
    clg_columns_in r = rest;
    r.n_class[1] += 1;
    REJECTED(encode_both(b.narrow, b.wide, r, cap), CLG_UNPACK_BAD_LAYOUT, 2u, 0u);
    REJECTED(encode_both(b.narrow, b.wide, rest, cap), CLG_UNPACK_BAD_LAYOUT, W + 6, 0u);
    b.wide.blk_base[7] -= 1;
    b.wide.n_val[CLG_WPACK_IDX] -= 1;
    REJECTED(encode_both(b.narrow, b.wide, rest, cap), CLG_UNPACK_BAD_LAYOUT, W + 1, 0u);
    b.wide.n_val[CLG_WPACK_IDX] += 1;
    r = rest, r.n_class[4] -= 1;
    REJECTED(encode_both(b.narrow, b.wide, r, cap), CLG_UNPACK_BAD_LAYOUT, W, 0u);
  }
  {  // a narrow VALUE finding comes before a wide BLOCK finding; alone, the wide one carries the offset
    Both b(c);
    b.wdesc[1].width = 65;  // KIND's block 1
    b.ndesc[size_t(b.narrow.blk_base[CLG_PACK_RNG])].ref = int64_t(1) << 40;
    REJECTED(encode_both(b.narrow, b.wide, rest, cap), CLG_UNPACK_BAD_VALUE, uint32_t(CLG_PACK_RNG), 0u);
    b.ndesc[size_t(b.narrow.blk_base[CLG_PACK_RNG])].ref = 0;
    b.ndesc[size_t(b.narrow.blk_base[CLG_PACK_RNG])].width = 0;  // (any i32 values: the unpack is clean, the encode runs)
    REJECTED(encode_both(b.narrow, b.wide, rest, cap), CLG_UNPACK_BAD_BLOCK, W, 1u);
  }
  {  // the wide value findings: a KIND above 3, then the histogram, with the offset
    Both b(c);
    b.wdesc[1].ref += 3;
    REJECTED(encode_both(b.narrow, b.wide, rest, cap), CLG_UNPACK_BAD_VALUE, W, 1u);
    b.wdesc[1].ref -= 3;
    REQUIRE(b.wdesc[0].width == 2);
    b.wbits[size_t(b.wdesc[0].pos)] = uint8_t((b.wbits[size_t(b.wdesc[0].pos)] & 0xFC) | ((b.wbits[size_t(b.wdesc[0].pos)] + 1) & 3));
    REJECTED(encode_both(b.narrow, b.wide, rest, cap), CLG_UNPACK_BAD_VALUE, W, 0u);
  }
  // the cross rule: the wide rows packed from consistent columns, the narrow columns from tags in
  // which two wide records of different kinds are swapped
  const auto swapped = [&](uint32_t lo, uint32_t hi_limit, Plain* q) {
    for (uint32_t k = lo; k + 1 < hi_limit; ++k)
      if (q->tag[q->w_idx[k]] != q->tag[q->w_idx[k + 1]]) {
        std::swap(q->tag[q->w_idx[k]], q->tag[q->w_idx[k + 1]]);
        return k;
      }
    REQUIRE(false);
    return 0u;
  };
  {
    const Both good(c);
    Plain q = p;
    const uint32_t last = swapped(2048 + 100, n, &q);   // the last tile
    const Both bad_last(q.cols());
    REJECTED(encode_both(bad_last.narrow, good.wide, rest, cap), CLG_UNPACK_BAD_VALUE, W + CLG_WPACK_IDX, uint64_t(last / 1024));
    REQUIRE(last / 1024 == 2);
    const uint32_t first = swapped(17, 1024, &q);       // ... and the first: the lowest row wins
    const Both bad_both(q.cols());
    REJECTED(encode_both(bad_both.narrow, good.wide, rest, cap), CLG_UNPACK_BAD_VALUE, W + CLG_WPACK_IDX, 0u);
    (void)first;
    // a w_idx that names a narrow record, or none
    Both b(c);
    Plain z = p;
    z.tag[z.w_idx[5]] = 0;
    z.order.push_back(1);
    const Both narrow_tag(z.cols(), false);
    REJECTED(encode_both(narrow_tag.narrow, b.wide, z.rest(), cap), CLG_UNPACK_BAD_VALUE, W + CLG_WPACK_IDX, 0u);
  }
  {  // a tag of 8 at a narrow position after a clean unpack is the encode's finding
    Plain q = p;
    uint32_t at = 0;
    while (q.tag[at] != 2) ++at;
    const Both b(c);
    q.tag[at] = 8;  // (the columns and `rest`'s totals stay)
    const Both eight(q.cols());
    const EncBoth e = encode_both(eight.narrow, b.wide, rest, cap);
    REQUIRE(e.st == CLG_E_INVALID_ARG && e.bad.what == CLG_UNPACK_BAD_NONE && e.e.bad_what == CLG_ENC_BAD_TAG && e.e.bad_index == at);
  }
}

void pieces() {
  uint8_t tag[6] = {0, 3, 4, 5, 6, 7};
  for (uint32_t t = 0; t < 4; ++t) REQUIRE(clg::wpack_cross_ok(tag, 6, 1 + t, t) && !clg::wpack_cross_ok(tag, 6, 1 + t, (t + 1) % 4));
  REQUIRE(!clg::wpack_cross_ok(tag, 6, 0, 0) && !clg::wpack_cross_ok(tag, 6, 5, 3) && !clg::wpack_cross_ok(tag, 6, 6, 0));
  REQUIRE(!clg::wpack_cross_ok(tag, 2, 2, 1));  // at n_rec
  clg_unpack_bad bad;
  REQUIRE(clg::wpack_bad_cross(&bad, 2049) == CLG_E_INVALID_ARG);
  REQUIRE(bad.what == CLG_UNPACK_BAD_VALUE && bad.stream == 33 && bad.block == 2);
  REQUIRE(clg::wpack_bad_wide(&bad, CLG_UNPACK_BAD_BLOCK, 25, 7) == CLG_E_INVALID_ARG && bad.stream == 57 && bad.block == 7);
  const uint32_t len[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 5};
  uint64_t pos[4];
  clg::wpack_pos_host(len, 3, pos);
  REQUIRE(pos[0] == 0 && pos[1] == 0xFFFFFFFFull && pos[2] == 0x1FFFFFFFEull && pos[3] == 0x200000003ull);
  clg::wpack_pos_host(len, 0, pos);
  REQUIRE(pos[0] == 0);
}

}  // namespace

int main() {
  pieces();
  const uint32_t counts[] = {0, 1, 1023, 1024, 1025, 2049};
  for (uint32_t n : counts)
    for (uint32_t gap = 0; gap < 3; ++gap) round_trips(n, gap, 1000 * gap + n);
  check_order();
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
