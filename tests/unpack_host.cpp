// Stand-alone check of the whole-call unpack of packed typed columns on the CPU
// (clg::pack_unpack_all_host in clonos_amd/csrc/pack.h, the reference the device unpack is held
// to): the round trip of every width 0..64 on the DELTA stream and every width the type allows on
// the FOR streams, stream lengths 0, 1, 2, 1023, 1024, 1025 and 3073, INT64_MIN beside INT64_MAX,
// sizes only, capacities short by one, blocks out of payload order and sharing a payload, and
// every rejection with its (what, stream, block) -- over output arrays held between canaries that
// no rejection may change.  Built with g++ (no HIP), plainly and with
// -fsanitize=address,undefined; the packed arrays are allocated at their exact sizes so that a
// read past a stated length is an error the sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../clonos_amd/csrc/pack.h"

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
constexpr size_t kGuard = 64;  // bytes either side of every output array

struct Cols {
  std::vector<uint8_t> tag;
  std::vector<int8_t> order;
  std::vector<int64_t> timestamp;
  std::vector<int32_t> rng, buffer_built;
  clg_columns c() const {
    clg_columns x{};
    x.tag = const_cast<uint8_t*>(tag.data()), x.order = const_cast<int8_t*>(order.data());
    x.timestamp = const_cast<int64_t*>(timestamp.data()), x.rng = const_cast<int32_t*>(rng.data());
    x.buffer_built = const_cast<int32_t*>(buffer_built.data());
    x.n_rec = tag.size(), x.n_class[0] = order.size(), x.n_class[1] = timestamp.size();
    x.n_class[2] = rng.size(), x.n_class[3] = buffer_built.size();
    return x;
  }
  const void* data(uint32_t s) const {
    const void* const p[5] = {tag.data(), order.data(), timestamp.data(), rng.data(), buffer_built.data()};
    return p[s];
  }
  uint64_t n(uint32_t s) const {
    const uint64_t v[5] = {tag.size(), order.size(), timestamp.size(), rng.size(), buffer_built.size()};
    return v[s];
  }
};

// The packed form in exactly sized arrays.
struct Packed {
  std::vector<clg_pack_block> desc;
  std::vector<uint8_t> bits;
  clg_packed p{};
  explicit Packed(const Cols& cols) {
    const clg_columns in = cols.c();
    REQUIRE(clg::pack_build_host(&in, &p) == CLG_OK);
    desc.resize(p.blk_base[5]), bits.resize(p.n_bits);
    refresh();
    REQUIRE(clg::pack_build_host(&in, &p) == CLG_OK);
  }
  void refresh() {  // after desc or bits were resized
    p.desc = desc.empty() ? nullptr : desc.data(), p.bits = bits.empty() ? nullptr : bits.data();
    p.cap_desc = desc.size(), p.cap_bits = bits.size();
  }
};

// Output arrays between canaries, each its own allocation; spare: extra capacity (elements).
struct Out {
  std::vector<uint8_t> buf[5];
  clg_columns c{};
  Out(const uint64_t n[5], uint64_t spare = 0, int short_one = -1) {
    uint64_t cap[5];
    for (uint32_t s = 0; s < 5; ++s) {
      cap[s] = n[s] + spare - (int(s) == short_one ? 1 : 0);
      buf[s].assign(2 * kGuard + cap[s] * clg::pack_stream_bytes(s), kFill);
    }
    c.tag = buf[0].data() + kGuard, c.order = reinterpret_cast<int8_t*>(buf[1].data() + kGuard);
    c.timestamp = reinterpret_cast<int64_t*>(buf[2].data() + kGuard), c.rng = reinterpret_cast<int32_t*>(buf[3].data() + kGuard);
    c.buffer_built = reinterpret_cast<int32_t*>(buf[4].data() + kGuard);
    c.cap_tag = cap[0], c.cap_order = cap[1], c.cap_timestamp = cap[2], c.cap_rng = cap[3], c.cap_buffer_built = cap[4];
    c.n_class[4] = 77, c.err_status = -5, c.cap_wide = 9;  // fields the unpack leaves alone
  }
  bool untouched() const {
    for (const auto& b : buf)
      for (uint8_t x : b)
        if (x != kFill) return false;
    return c.n_class[4] == 77 && c.err_status == -5 && c.cap_wide == 9;
  }
  // the values are cols', and nothing outside [0, n) of any array was written
  bool holds(const Cols& cols) const {
    for (uint32_t s = 0; s < 5; ++s) {
      const size_t nb = cols.n(s) * clg::pack_stream_bytes(s);
      if (nb && memcmp(buf[s].data() + kGuard, cols.data(s), nb)) return false;
      for (size_t i = 0; i < buf[s].size(); ++i)
        if ((i < kGuard || i >= kGuard + nb) && buf[s][i] != kFill) return false;
    }
    return c.n_class[4] == 77 && c.err_status == -5;
  }
};

bool sizes_are(const clg_columns& c, const Cols& cols) {
  return c.n_rec == cols.n(0) && c.n_class[0] == cols.n(1) && c.n_class[1] == cols.n(2) && c.n_class[2] == cols.n(3) &&
         c.n_class[3] == cols.n(4);
}
bool bad_is(const clg_unpack_bad& b, uint32_t what, uint32_t stream, uint64_t block) {
  return b.what == what && b.stream == stream && b.block == block;
}

// The round trip, sizes only, spare capacity, and each capacity short by one.
void round_trip(const Cols& cols) {
  Packed pk(cols);
  const uint64_t n[5] = {cols.n(0), cols.n(1), cols.n(2), cols.n(3), cols.n(4)};
  clg_unpack_bad bad{9, 9, 9};
  {
    Out o(n);
    REQUIRE(clg::pack_unpack_all_host(&pk.p, &o.c, &bad) == CLG_OK);
    REQUIRE(bad_is(bad, CLG_UNPACK_BAD_NONE, 0, ~0ull) && sizes_are(o.c, cols) && o.holds(cols));
  }
  {
    Out o(n, 5);
    REQUIRE(clg::pack_unpack_all_host(&pk.p, &o.c, nullptr) == CLG_OK && o.holds(cols));
  }
  {
    clg_columns sizes{};
    REQUIRE(clg::pack_unpack_all_host(&pk.p, &sizes, &bad) == CLG_OK && sizes_are(sizes, cols));
  }
  for (int s = 0; s < 5; ++s)
    if (n[s]) {
      Out o(n, 0, s);
      REQUIRE(clg::pack_unpack_all_host(&pk.p, &o.c, &bad) == CLG_E_CAPACITY);
      REQUIRE(sizes_are(o.c, cols) && o.untouched() && bad.what == CLG_UNPACK_BAD_NONE);
    }
}

// n values whose residuals span exactly `width` bits from the signed minimum `lo`.
std::vector<uint64_t> residuals(std::mt19937_64& r, uint32_t width, size_t n, int64_t lo) {
  std::vector<uint64_t> v(n);
  const uint64_t span = width == 64 ? ~0ull : (1ull << width) - 1;
  for (uint64_t& x : v) x = uint64_t(lo) + (span == ~0ull ? r() : r() % (span + 1));
  if (n >= 2 && width) {
    const size_t a = r() % n, b = (a + 1 + r() % (n - 1)) % n;
    v[a] = uint64_t(lo), v[b] = uint64_t(lo) + span;
  }
  return v;
}

void widths() {
  std::mt19937_64 r(0xFACADE);
  const size_t lens[] = {3, 1023, 1024};
  for (uint32_t w = 0; w <= 64; ++w)
    for (size_t n : lens) {
      Cols c;
      const int64_t lo = w >= 63 ? INT64_MIN : int64_t(r() % (1ull << 62)) - int64_t(1ull << 61);
      uint64_t x = r();
      c.timestamp.push_back(int64_t(x));
      for (uint64_t d : residuals(r, w, n < 1024 ? n : 1023, lo)) c.timestamp.push_back(int64_t(x += d));
      if (w <= 3) for (uint64_t v : residuals(r, w, n, int64_t(r() % (8 - ((1u << w) - 1))))) c.tag.push_back(uint8_t(v));
      if (w <= 8) for (uint64_t v : residuals(r, w, n, -128 + int64_t(r() % (256 - ((1u << w) - 1))))) c.order.push_back(int8_t(int64_t(v)));
      if (w <= 32) {
        const uint64_t sp = (1ull << w) - 1;
        for (uint64_t v : residuals(r, w, n, INT32_MIN + int64_t(r() % ((1ull << 32) - sp)))) c.rng.push_back(int32_t(int64_t(v)));
        for (uint64_t v : residuals(r, w, n, INT32_MAX - int64_t(sp))) c.buffer_built.push_back(int32_t(int64_t(v)));
      }
      Packed pk(c);
      REQUIRE(pk.desc[pk.p.blk_base[2]].width == w);
      if (w <= 3) REQUIRE(pk.desc[pk.p.blk_base[0]].width == w);
      if (w <= 8) REQUIRE(pk.desc[pk.p.blk_base[1]].width == w);
      if (w <= 32) REQUIRE(pk.desc[pk.p.blk_base[3]].width == w && pk.desc[pk.p.blk_base[4]].width == w);
      round_trip(c);
    }
}

Cols mixed(std::mt19937_64& r, size_t n, int variant) {
  Cols c;
  int64_t t = 1700000000000ll;
  for (size_t i = 0; i < n; ++i) {
    c.tag.push_back(variant == 1 ? 7 : uint8_t(r() % 8));
    c.order.push_back(variant == 1 ? -3 : int8_t(r() % 4));
    c.timestamp.push_back(variant == 1 ? t += 5 : t += int64_t(r() % 6));
    c.rng.push_back(variant == 1 ? INT32_MIN : int32_t(r()));
    c.buffer_built.push_back(variant == 2 ? int32_t(r() % 65536) : 4096);
  }
  if (variant == 2) c.order.clear(), c.rng.clear();  // streams of different lengths, some empty
  return c;
}

void lengths() {
  std::mt19937_64 r(0xBEEF);
  const size_t lens[] = {0, 1, 2, 1023, 1024, 1025, 3073};
  for (size_t n : lens)
    for (int variant = 0; variant < 3; ++variant) round_trip(mixed(r, n, variant));
}

void extremes() {
  Cols c;
  const int64_t pat[] = {INT64_MIN, INT64_MAX, INT64_MIN, 0, INT64_MAX, INT64_MAX, INT64_MIN, -1, 1};
  for (int k = 0; k < 300; ++k)
    for (int64_t v : pat) c.timestamp.push_back(v);
  c.rng = {INT32_MIN, INT32_MAX, INT32_MIN, -1, 0, 1, INT32_MAX};
  c.order = {-128, 127, -128, 0};
  c.tag = {0, 255, 7, 0};
  round_trip(c);
}

// Blocks need not lie in payload order, and may share payload bytes: they are only read.
void any_payload_order() {
  std::mt19937_64 r(0x0DD);
  Cols c = mixed(r, 3073, 0);
  Packed pk(c);
  const uint64_t n[5] = {3073, 3073, 3073, 3073, 3073};
  // the payloads laid out again in reverse block order
  std::vector<uint8_t> bits(pk.bits.size());
  uint64_t pos = 0;
  for (size_t b = pk.desc.size(); b-- > 0;) {
    clg_pack_block& d = pk.desc[b];
    const uint32_t bytes = clg::pack_payload_bytes(clg::pack_resid(b >= pk.p.blk_base[2] && b < pk.p.blk_base[3] ? 2 : 0, d.count), d.width);
    if (bytes) memcpy(bits.data() + pos, pk.bits.data() + d.pos, bytes);
    d.pos = pos;
    pos += bytes;
  }
  REQUIRE(pos == bits.size());
  pk.bits = bits, pk.refresh();
  Out o(n);
  REQUIRE(clg::pack_unpack_all_host(&pk.p, &o.c, nullptr) == CLG_OK && o.holds(c));
  // two equal blocks of one stream sharing one payload
  Cols twice;
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 1024; ++i) twice.rng.push_back(int32_t(i * 7919 % 100003));
  Packed p2(twice);
  REQUIRE(p2.desc.size() == 2 && p2.desc[0].width == p2.desc[1].width);
  p2.desc[1].pos = p2.desc[0].pos;
  p2.p.n_bits = p2.desc[1].pos + (p2.bits.size() / 2);
  const uint64_t n2[5] = {0, 0, 0, 2048, 0};
  Out o2(n2);
  REQUIRE(clg::pack_unpack_all_host(&p2.p, &o2.c, nullptr) == CLG_OK && o2.holds(twice));
}

// Every rejection: the bytes may come from another process.
void malformed() {
  std::mt19937_64 r(0xBAD);
  Cols c;
  int64_t t = 0;
  for (int i = 0; i < 2500; ++i) c.timestamp.push_back(t += int64_t(r() % 1000)), c.rng.push_back(int32_t(r() % 100000));
  for (int i = 0; i < 1500; ++i) c.tag.push_back(uint8_t(r() % 8)), c.order.push_back(int8_t(r() % 4));
  Packed pk(c);
  const clg_packed good = pk.p;
  const std::vector<clg_pack_block> saved = pk.desc;
  const uint64_t n[5] = {1500, 1500, 2500, 2500, 0};
  const auto run = [&](const clg_packed& p, int want, uint32_t what, uint32_t stream, uint64_t block) {
    Out o(n, 3);
    clg_unpack_bad bad{9, 9, 9};
    REQUIRE(clg::pack_unpack_all_host(&p, &o.c, &bad) == want);
    REQUIRE(bad_is(bad, what, stream, block));
    REQUIRE(want == CLG_OK ? o.holds(c) : o.untouched());
    pk.desc = saved;
  };
  const int E = CLG_E_INVALID_ARG;
  run(good, CLG_OK, CLG_UNPACK_BAD_NONE, 0, ~0ull);
  const uint64_t b2 = good.blk_base[2], b3 = good.blk_base[3];
  clg_pack_block* d = pk.desc.data();

  // blocks
  d[b2 + 1].width = 65; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 1);
  d[b2 + 1].width = 0xFFFFFFFFu; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 1);
  d[b2].count = 0; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 0);
  d[b2].count = 1025; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 0);
  d[b2].count = 1023; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 0);       // not the last block: 1024
  d[b2 + 2].count = 453; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 2);    // the last block: 2500 - 2048
  d[b2 + 2].count = 1024; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 2);
  d[b2 + 2].pos = good.n_bits; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 2);      // pos + size > n_bits
  d[b2 + 2].pos = ~0ull - 15; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 2);       // ... wrapping
  d[b3 + 2].width = 64; run(good, E, CLG_UNPACK_BAD_BLOCK, 3, 2);             // its size passes n_bits
  d[b3 + 1].pos += 8; run(good, E, CLG_UNPACK_BAD_BLOCK, 3, 1);               // pos % 16 != 0
  d[b2 + 1].pos -= 15; run(good, E, CLG_UNPACK_BAD_BLOCK, 2, 1);
  REQUIRE(saved[b3 + 1].pos % 16 == 0 && saved[b3 + 1].pos >= 16);
  // two bad blocks in different streams: the lower; within a stream: the lower block
  d[b3].width = 65, d[1].count = 7; run(good, E, CLG_UNPACK_BAD_BLOCK, 0, 1);
  d[b3 + 2].width = 65, d[b3 + 1].count = 7; run(good, E, CLG_UNPACK_BAD_BLOCK, 3, 1);
  // a bad value and, above it, a bad block: the block
  d[0].ref = 250, d[b3 + 2].width = 99; run(good, E, CLG_UNPACK_BAD_BLOCK, 3, 2);

  // layout
  clg_packed p = good;
  p.n_bits = 16; run(p, E, CLG_UNPACK_BAD_BLOCK, 0, 0);  // (the first block whose payload lies past it)
  p = good, p.n_bits = p.cap_bits + 16; run(p, E, CLG_UNPACK_BAD_LAYOUT, 0, 0);
  p = good, p.blk_base[3] += 1; run(p, E, CLG_UNPACK_BAD_LAYOUT, 2, 0);
  p = good, p.blk_base[2] = p.blk_base[3] + 1; run(p, E, CLG_UNPACK_BAD_LAYOUT, 1, 0);
  p = good, p.blk_base[0] = 1; run(p, E, CLG_UNPACK_BAD_LAYOUT, 0, 0);
  p = good, p.cap_desc = p.blk_base[5] - 1; run(p, E, CLG_UNPACK_BAD_LAYOUT, 0, 0);
  p = good, p.n_val[2] = 2500 + 1024; run(p, E, CLG_UNPACK_BAD_LAYOUT, 2, 0);
  p = good, p.n_val[4] = 1; run(p, E, CLG_UNPACK_BAD_LAYOUT, 4, 0);
  p = good, p.n_val[1] = ~0ull; run(p, E, CLG_UNPACK_BAD_LAYOUT, 1, 0);
  p = good, p.desc = nullptr; run(p, E, CLG_UNPACK_BAD_LAYOUT, 0, 0);
  p = good, p.bits = nullptr; run(p, E, CLG_UNPACK_BAD_LAYOUT, 0, 0);
  // a layout error beside a bad block: the layout
  p = good, p.blk_base[3] += 1, d[0].width = 65; run(p, E, CLG_UNPACK_BAD_LAYOUT, 2, 0);
  {
    Out o(n);
    clg_unpack_bad bad{9, 9, 9};
    REQUIRE(clg::pack_unpack_all_host(nullptr, &o.c, &bad) == E && bad.what == CLG_UNPACK_BAD_NONE && o.untouched());
    REQUIRE(clg::pack_unpack_all_host(&good, nullptr, &bad) == E);
  }

  // values outside the stream's type
  d[b3].ref = int64_t(INT32_MAX) - 5; run(good, E, CLG_UNPACK_BAD_VALUE, 3, 0);
  d[b3 + 1].ref = int64_t(INT32_MIN) - 1; run(good, E, CLG_UNPACK_BAD_VALUE, 3, 1);
  d[0].ref = 250; run(good, E, CLG_UNPACK_BAD_VALUE, 0, 0);
  d[1].ref = -1; run(good, E, CLG_UNPACK_BAD_VALUE, 0, 1);
  d[good.blk_base[1]].ref = 126; run(good, E, CLG_UNPACK_BAD_VALUE, 1, 0);
  d[good.blk_base[1] + 1].ref = -131; run(good, E, CLG_UNPACK_BAD_VALUE, 1, 1);
  d[b3 + 2].ref = INT64_MAX; run(good, E, CLG_UNPACK_BAD_VALUE, 3, 2);  // (ref + p wraps)
  d[b3 + 2].ref = INT64_MIN; run(good, E, CLG_UNPACK_BAD_VALUE, 3, 2);
  d[b3 + 1].ref = INT32_MAX, d[0].ref = 253; run(good, E, CLG_UNPACK_BAD_VALUE, 0, 0);  // two: the lower
  // a reference that moves the values but keeps them inside the type is fine: tags 0..7 from 248
  d[0].ref = 248;
  {
    Out o(n);
    clg_unpack_bad bad{};
    REQUIRE(clg::pack_unpack_all_host(&good, &o.c, &bad) == CLG_OK && bad.what == CLG_UNPACK_BAD_NONE);
    REQUIRE(o.c.tag[0] == uint8_t(c.tag[0] - saved[0].ref + 248));
    pk.desc = saved;
  }
  // timestamps take any bits
  d[b2].ref = INT64_MIN, d[b2].first = INT64_MAX;
  {
    Out o(n);
    REQUIRE(clg::pack_unpack_all_host(&good, &o.c, nullptr) == CLG_OK && o.c.timestamp[0] == INT64_MAX);
    pk.desc = saved;
  }

  // the helpers on their own
  REQUIRE(clg::pack_range_inside(0, 0, 8) && !clg::pack_range_inside(0, 1, 8) && !clg::pack_range_inside(0, -1, 0));
  REQUIRE(clg::pack_range_inside(1, -128, 8) && !clg::pack_range_inside(1, -128, 9) && !clg::pack_range_inside(1, 128, 0));
  REQUIRE(clg::pack_range_inside(3, INT32_MIN, 32) && !clg::pack_range_inside(3, INT32_MIN, 33));
  REQUIRE(!clg::pack_range_inside(4, INT64_MIN, 0) && !clg::pack_range_inside(4, INT64_MAX, 64) && clg::pack_range_inside(4, INT32_MAX, 0));
  REQUIRE(clg::pack_range_inside(2, INT64_MAX, 64));
  REQUIRE(clg::pack_blocks_of(~0ull) == (1ull << 54) && clg::pack_blocks_of(1024) == 1 && clg::pack_blocks_of(1025) == 2);
}

}  // namespace

int main() {
  widths();
  lengths();
  extremes();
  any_payload_order();
  malformed();
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
