// Stand-alone check of the CPU pack and unpack of the payload column (clonos_amd/csrc/ppay.h)
// against a naive reference kept here (anchors by a scan over the tile's earlier rows, lcps a byte
// at a time, the lcps' values read back through pack.h's decode): round trips over seeded columns
// with tile seams, empty rows and rows either side of 64 bytes, the two size bounds, a tile of one
// length, sizes only, the capacity failures over filled outputs, every rejection of the pack and
// every finding of the unpack in its order, and a non-maximal lcp.  Built with g++ (no HIP),
// plainly and with -fsanitize=address,undefined; every array is allocated at its exact size so
// that a read or write past a stated length is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../clonos_amd/csrc/ppay.h"

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

struct Column {
  std::vector<uint8_t> var;
  std::vector<uint64_t> pos{0};
  void add(const std::vector<uint8_t>& row) {
    var.insert(var.end(), row.begin(), row.end());
    pos.push_back(var.size());
  }
  uint64_t rows() const { return pos.size() - 1; }
};

struct Packed {
  std::vector<clg_pack_block> desc;
  std::vector<uint8_t> bits, tail;
  clg_packed_payloads p{};
  // the struct over the vectors at their exact sizes, results kept
  clg_packed_payloads* view() {
    p.desc = desc.data(), p.bits = bits.data(), p.tail = tail.data();
    p.cap_desc = desc.size(), p.cap_bits = bits.size(), p.cap_tail = tail.size();
    return &p;
  }
};

// The naive reference: lcp and anchor of every row.
void naive(const Column& c, std::vector<uint32_t>* lcp, std::vector<uint64_t>* anchor) {
  const uint64_t n = c.rows();
  lcp->assign(n, 0), anchor->assign(n, 0);
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t t0 = k / 1024 * 1024, len = c.pos[k + 1] - c.pos[k];
    uint64_t a = k;
    for (uint64_t j = t0; j < k; ++j)
      if (c.pos[j + 1] - c.pos[j] == len) {
        a = j;
        break;
      }
    (*anchor)[k] = a;
    uint32_t m = 0;
    if (a != k)
      while (m < len && c.var[c.pos[k] + m] == c.var[c.pos[a] + m]) ++m;
    (*lcp)[k] = m;
  }
}

Packed pack(const Column& c) {
  Packed out;
  REQUIRE(clg::ppay_build_host(c.var.data(), c.pos.data(), c.rows(), &out.p) == CLG_OK);  // sizes only
  REQUIRE(out.p.n_rows == c.rows() && out.p.n_var == c.var.size() && out.p.bad_row == clg::kPpayNoRow);
  // the two bounds
  REQUIRE(out.p.n_tail <= clg::ppay_tail_bound(out.p.n_var));
  REQUIRE(out.p.n_bits <= clg::ppay_bits_bound(out.p.n_rows));
  out.desc.resize(clg::ppay_blocks(c.rows())), out.bits.resize(out.p.n_bits), out.tail.resize(out.p.n_tail);
  const clg_packed_payloads sizes = out.p;
  if (!c.rows()) return out;
  std::vector<uint8_t> spare(1);  // an array without bytes still has an address
  clg_packed_payloads* v = out.view();
  if (!v->bits) v->bits = spare.data();
  if (!v->tail) v->tail = spare.data();
  REQUIRE(clg::ppay_build_host(c.var.data(), c.pos.data(), c.rows(), v) == CLG_OK);
  REQUIRE(v->n_bits == sizes.n_bits && v->n_tail == sizes.n_tail && v->n_var == sizes.n_var);
  out.view();
  return out;
}

std::vector<uint8_t> unpack(Packed& pk, const Column& c, int want = CLG_OK, uint32_t what = CLG_UNPACK_BAD_NONE,
                            uint64_t block = ~0ull) {
  std::vector<uint8_t> var(c.var.size() + 1, 0xA5);  // (one spare byte: a null var is the sizes-only call)
  clg_payloads out{};
  out.var = var.data(), out.cap_var = c.var.size();
  clg_unpack_bad bad{9, 9, 9};
  const int st = clg::ppay_unpack_host(pk.view(), c.pos.data(), &out, &bad);
  REQUIRE(st == want);
  REQUIRE(bad.what == what && bad.block == block);
  REQUIRE(bad.stream == (what == CLG_UNPACK_BAD_NONE ? 0u : uint32_t(CLG_PPAY_STREAM)));
  if (st != CLG_OK)
    for (uint8_t b : var) REQUIRE(b == 0xA5);  // nothing written
  else
    REQUIRE(out.n_rows == c.rows() && out.n_var == c.var.size());
  REQUIRE(var.back() == 0xA5);
  var.pop_back();
  return var;
}

void check(const Column& c) {
  Packed pk = pack(c);
  std::vector<uint32_t> lcp;
  std::vector<uint64_t> anchor;
  naive(c, &lcp, &anchor);
  // the lcps are the naive ones, the tails the bytes behind them, in row order
  uint64_t at = 0, pos_bits = 0;
  int64_t x[clg::kPpayTile];
  for (uint64_t t = 0; t < pk.desc.size(); ++t) {
    const clg_pack_block& d = pk.desc[t];
    REQUIRE(clg::pack_block_in_ok(d, false, t, c.rows(), pk.bits.size()));
    REQUIRE(d.pos == pos_bits && d.first == 0);
    pos_bits += clg::pack_payload_bytes(d.count, d.width);
    clg::pack_decode_block(d, false, pk.bits.data() + d.pos, x);
    for (uint32_t i = 0; i < d.count; ++i) {
      const uint64_t k = t * 1024 + i;
      REQUIRE(uint64_t(x[i]) == lcp[k]);
      for (uint64_t b = c.pos[k] + lcp[k]; b < c.pos[k + 1]; ++b) REQUIRE(pk.tail[at++] == c.var[b]);
    }
  }
  REQUIRE(pos_bits == pk.bits.size() && at == pk.tail.size());
  REQUIRE(unpack(pk, c) == c.var);
}

Column seeded(std::mt19937_64& rng, uint64_t n, const std::vector<uint32_t>& lens, uint32_t alphabet) {
  Column c;
  std::vector<std::vector<uint8_t>> seen;
  for (uint64_t k = 0; k < n; ++k) {
    const uint32_t L = lens[rng() % lens.size()];
    std::vector<uint8_t> row(L);
    for (auto& b : row) b = uint8_t(rng() % alphabet);
    for (const auto& s : seen)
      if (s.size() == L && rng() % 4) {
        const uint32_t keep = uint32_t(rng() % (L + 1));
        for (uint32_t i = 0; i < keep; ++i) row[i] = s[i];
        break;
      }
    if (seen.size() < 64) seen.push_back(row);
    c.add(row);
  }
  return c;
}

void rejections(std::mt19937_64& rng) {
  const Column c = seeded(rng, 2100, {0, 1, 5, 63, 64, 65, 130}, 3);
  Packed good = pack(c);

  // ---- the pack: bad rows, found before any byte of var is read (var is null here)
  {
    clg_packed_payloads p{};
    std::vector<uint64_t> pos = c.pos;
    pos[0] = 1;
    REQUIRE(clg::ppay_build_host(nullptr, pos.data(), c.rows(), &p) == CLG_E_INVALID_ARG && p.bad_row == 0);
    pos = c.pos;
    pos[1500] = pos[1499] - 1;  // decreases over row 1498 (or an earlier equal one)
    REQUIRE(clg::ppay_build_host(nullptr, pos.data(), c.rows(), &p) == CLG_E_INVALID_ARG);
    uint64_t first = 0;
    while (pos[first + 1] >= pos[first]) ++first;
    REQUIRE(p.bad_row == first && first <= 1499);
    const uint64_t huge[3] = {0, 5, 5 + (1ull << 32)};
    REQUIRE(clg::ppay_build_host(nullptr, huge, 2, &p) == CLG_E_INVALID_ARG && p.bad_row == 1);
    const uint64_t under[3] = {0, 5, 4 + (1ull << 32)};  // one byte under the limit: the rows pass, var is missed
    REQUIRE(clg::ppay_build_host(nullptr, under, 2, &p) == CLG_E_INVALID_ARG && p.bad_row == clg::kPpayNoRow);
    REQUIRE(clg::ppay_build_host(c.var.data(), nullptr, c.rows(), &p) == CLG_E_INVALID_ARG);
    REQUIRE(clg::ppay_build_host(c.var.data(), c.pos.data(), c.rows(), nullptr) == CLG_E_INVALID_ARG);
    REQUIRE(clg::ppay_build_host(nullptr, nullptr, 0, &p) == CLG_OK && p.n_rows == 0 && p.n_bits == 0 && p.n_tail == 0);
  }
  // ---- the pack: each capacity one below its total, results filled, outputs untouched
  for (int which = 0; which < 3; ++which) {
    std::vector<clg_pack_block> desc(good.desc.size() - (which == 0));
    std::vector<uint8_t> bits(good.bits.size() - (which == 1), 0xA5), tail(good.tail.size() - (which == 2), 0xA5);
    memset(desc.data(), 0xA5, desc.size() * sizeof(clg_pack_block));
    clg_packed_payloads p{};
    p.desc = desc.data(), p.bits = bits.data(), p.tail = tail.data();
    p.cap_desc = desc.size(), p.cap_bits = bits.size(), p.cap_tail = tail.size();
    REQUIRE(clg::ppay_build_host(c.var.data(), c.pos.data(), c.rows(), &p) == CLG_E_CAPACITY);
    REQUIRE(p.n_rows == c.rows() && p.n_var == c.var.size() && p.n_bits == good.bits.size() && p.n_tail == good.tail.size());
    for (uint8_t b : bits) REQUIRE(b == 0xA5);
    for (uint8_t b : tail) REQUIRE(b == 0xA5);
    for (size_t i = 0; i < desc.size() * sizeof(clg_pack_block); ++i) REQUIRE(reinterpret_cast<uint8_t*>(desc.data())[i] == 0xA5);
  }

  // ---- the unpack: sizes only, capacity
  {
    clg_payloads out{};
    clg_unpack_bad bad{};
    REQUIRE(clg::ppay_unpack_host(good.view(), c.pos.data(), &out, &bad) == CLG_OK);
    REQUIRE(out.n_rows == c.rows() && out.n_var == c.var.size() && bad.what == CLG_UNPACK_BAD_NONE && bad.block == ~0ull);
    std::vector<uint8_t> var(c.var.size() - 1, 0xA5);
    out.var = var.data(), out.cap_var = var.size();
    REQUIRE(clg::ppay_unpack_host(good.view(), c.pos.data(), &out, &bad) == CLG_E_CAPACITY && bad.what == CLG_UNPACK_BAD_NONE);
    for (uint8_t b : var) REQUIRE(b == 0xA5);
  }
  const uint32_t L = CLG_UNPACK_BAD_LAYOUT, B = CLG_UNPACK_BAD_BLOCK, V = CLG_UNPACK_BAD_VALUE, T = CLG_UNPACK_BAD_TOTAL;
  const int E = CLG_E_INVALID_ARG;
  // ---- layout
  {
    Packed p = good;
    p.view()->cap_desc -= 1;
    std::vector<uint8_t> var(c.var.size(), 0xA5);
    clg_payloads out{};
    out.var = var.data(), out.cap_var = var.size();
    clg_unpack_bad bad{};
    REQUIRE(clg::ppay_unpack_host(&p.p, c.pos.data(), &out, &bad) == E && bad.what == L && bad.stream == CLG_PPAY_STREAM && bad.block == 0);
    p.view()->cap_bits -= 1;
    REQUIRE(clg::ppay_unpack_host(&p.p, c.pos.data(), &out, &bad) == E && bad.what == L);
    p.view()->cap_tail -= 1;
    REQUIRE(clg::ppay_unpack_host(&p.p, c.pos.data(), &out, &bad) == E && bad.what == L);
    p.view()->tail = nullptr;
    REQUIRE(clg::ppay_unpack_host(&p.p, c.pos.data(), &out, &bad) == E && bad.what == L);
    p.view();
    REQUIRE(clg::ppay_unpack_host(&p.p, nullptr, &out, &bad) == E && bad.what == L);
    p.view()->n_rows += 1024;  // a block more than desc holds
    REQUIRE(clg::ppay_unpack_host(&p.p, c.pos.data(), &out, &bad) == E && bad.what == L);
    for (uint8_t b : var) REQUIRE(b == 0xA5);
  }
  // ---- block: the lowest; a block finding goes before a value finding in a lower tile
  {
    Packed p = good;
    p.desc[2].width = 65;
    p.desc[1].pos += 8;  // not a multiple of 16
    unpack(p, c, E, B, 1);
    p = good;
    p.desc[2].count = 1024;  // the last tile holds fewer
    p.desc[0].ref = 1;       // a value finding in tile 0 (an anchor's lcp)
    unpack(p, c, E, B, 2);
    p = good;
    p.desc[1].pos = p.bits.size();  // its payload passes n_bits
    REQUIRE(p.desc[1].width > 0);
    unpack(p, c, E, B, 1);
  }
  // ---- value: an lcp above its row's length; a non-zero lcp on an anchor; the pos rules
  {
    Packed p = good;
    p.desc[1].ref = 200;  // every row of tile 1 gets an lcp above 130
    unpack(p, c, E, V, 1);
    p = good;
    p.desc[0].ref = 1, p.desc[2].ref = 1;  // row 0 is an anchor
    unpack(p, c, E, V, 0);
    Column q = c;
    q.pos[0] = 1;
    unpack(good, q, E, V, 0);
    q = c;
    q.pos[1100] = q.pos[1101] + 1;  // row 1100 decreases
    unpack(good, q, E, V, 1);
    Column two;
    two.add({1, 2, 3});
    two.add({4});
    Packed pt = pack(two);
    two.pos[2] = 3 + (1ull << 32);
    pt.p.n_var = two.pos[2];
    std::vector<uint8_t> var(8, 0xA5);
    clg_payloads out{};
    out.var = var.data(), out.cap_var = ~0ull;
    clg_unpack_bad bad{};
    REQUIRE(clg::ppay_unpack_host(pt.view(), two.pos.data(), &out, &bad) == E && bad.what == V && bad.block == 0);
    for (uint8_t b : var) REQUIRE(b == 0xA5);
  }
  // ---- total: the tails' sum, and pos's end
  {
    Packed p = good;
    p.tail.push_back(0);
    p.p.n_tail = p.tail.size();
    unpack(p, c, E, T, 0);
    p = good;
    p.p.n_tail -= 1;
    unpack(p, c, E, T, 0);
    p = good;
    p.p.n_var -= 1;
    std::vector<uint8_t> var(c.var.size(), 0xA5);
    clg_payloads out{};
    out.var = var.data(), out.cap_var = var.size();
    clg_unpack_bad bad{};
    REQUIRE(clg::ppay_unpack_host(p.view(), c.pos.data(), &out, &bad) == E && bad.what == T && bad.block == 0);
    for (uint8_t b : var) REQUIRE(b == 0xA5);
  }
}

// A non-maximal lcp unpacks to the same column: row 1 keeps one byte less of its anchor.
void non_maximal() {
  Column c;
  c.add({7, 8, 9, 10});
  c.add({7, 8, 9, 11});
  c.add({7, 8, 0, 0});
  Packed p = pack(c);
  REQUIRE(p.tail.size() == 4 + 1 + 2);
  const int64_t x[3] = {0, 2, 2};  // (the maximal ones: 0, 3, 2)
  clg_pack_block d = clg::pack_measure_block(x, 3, false);
  d.pos = 0;
  p.desc[0] = d;
  p.bits.assign(clg::pack_payload_bytes(3, d.width), 0);
  clg::pack_write_block(x, d, false, p.bits.data());
  p.tail = {7, 8, 9, 10, 9, 11, 0, 0};
  p.p.n_bits = p.bits.size(), p.p.n_tail = p.tail.size();
  REQUIRE(unpack(p, c) == c.var);
}

}  // namespace

int main() {
  std::mt19937_64 rng(0x99A7);
  check(Column{});
  for (uint64_t n : {1ull, 2ull, 1023ull, 1024ull, 1025ull, 2049ull}) {
    check(seeded(rng, n, {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65}, 2));
    check(seeded(rng, n, {47}, 4));       // one length for a whole tile
    check(seeded(rng, n, {0}, 2));        // no bytes at all
    check(seeded(rng, n, {0, 300}, 2));   // empty rows between others
  }
  {  // m identical rows of L bytes leave L tail bytes; 1024 distinct lengths leave everything
    Column c;
    for (int i = 0; i < 1000; ++i) c.add(std::vector<uint8_t>(47, uint8_t(0x5A)));
    REQUIRE(pack(c).p.n_tail == 47);
    check(c);
    Column d;
    for (uint32_t i = 0; i < 1024; ++i) d.add(std::vector<uint8_t>(i, uint8_t(i)));
    const Packed pd = pack(d);
    REQUIRE(pd.p.n_tail == d.var.size() && pd.p.n_bits == 0);
    check(d);
  }
  {  // the first difference at every byte 0 .. 16 of rows of 17 bytes, and lcp == len
    Column c;
    std::vector<uint8_t> base(17);
    for (uint32_t i = 0; i < 17; ++i) base[i] = uint8_t(i + 1);
    c.add(base);
    for (uint32_t at = 0; at <= 17; ++at) {
      std::vector<uint8_t> row = base;
      if (at < 17) row[at] ^= 0x80;
      c.add(row);
    }
    check(c);
  }
  rejections(rng);
  non_maximal();
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
